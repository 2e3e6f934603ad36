// The run-time switches of the library: every environment variable it reads, with the value an unset variable stands
// for and the moment of reading.  This is the one place that reads the environment (host code only, plain C++).
//   kOnce      the first read is kept for the life of the process
//   kEachCall  read at every use: tests and tools change these inside one process
//   kOnceAndEachCall  EK_HIP_PIPE_TRACE: whether a call traces is kept from the first read (switch_once), the level of
//              detail of its report is read when the report is written (switch_int)
// A set variable counts as atoi() of its text, so "" and "abc" are 0; the text-valued row is used as it stands.
#pragma once
#include <cstdlib>

namespace ek {

enum Switch {
  kSwTwoStageMin, kSwDistMinRanks, kSwRcclLib, kSwPipeMin, kSwPipeTrace, kSwPipeLower, kSwPipeThreadsOut, kSwAlias,
  kSwBandInput, kSwPlacement, kSwPlacementVerbose, kSwTeamPoison, kSwPairMin, kSwLookaheadMin, kSwDistLookaheadMin,
  kSwChase, kSwChaseWgs, kSwChaseJitter, kSwCensusSpins, kSwQ2Nblk, kSwCount
};
enum SwitchRead { kOnce, kEachCall, kOnceAndEachCall };
struct SwitchRow { const char *name; int unset; SwitchRead read; };

constexpr SwitchRow kSwitches[kSwCount] = {
  {"EK_HIP_TWO_STAGE_MIN", -1, kOnce},                // order from which two stages tridiagonalise (< 0: 512, 0: never)
  {"EK_HIP_DIST_MIN_RANKS", 3, kEachCall},            // ranks from which the Cholesky factor and the reduction are distributed
  {"EK_HIP_RCCL_LIB", 0, kEachCall},                  // text: the RCCL library to load before the usual names
  {"EK_HIP_PIPE_MIN", 2048, kEachCall},               // order from which the host path stages through the pipeline (0: never)
  {"EK_HIP_PIPE_TRACE", 0, kOnceAndEachCall},         // != 0: the pipeline's report on stderr, >= 2: with every job
  {"EK_HIP_PIPE_LOWER", 1, kOnce},                    // 0: whole matrices both ways
  {"EK_HIP_PIPE_THREADS_OUT", -1, kOnce},             // copy threads on the way out (1 .. threads per direction; else 2)
  {"EK_HIP_ALIAS", 1, kEachCall},                     // 0: always copy the caller's device arrays
  {"EK_HIP_BAND_INPUT", 1, kEachCall},                // 0: no short cut for a matrix that is a band already
  {"EK_HIP_PLACEMENT", 1, kOnce},                     // 0: no placement probes for the scratch of the tridiagonalisation
  {"EK_HIP_PLACEMENT_VERBOSE", 0, kEachCall},         // set (to anything): what the probes found, on stderr
  {"EK_HIP_TEAM_POISON", 0, kEachCall},               // text beginning with 1: NaN into the strips a rehearsed member does not own
  {"EK_SY2SB_PAIR_MIN", 5120, kEachCall},             // rows from which the panels go in pairs (0: never)
  {"EK_SY2SB_LOOKAHEAD_MIN", 5120, kOnce},            // rows from which the next panel is factored beside the update
  {"EK_SY2SB_DIST_LOOKAHEAD_MIN", -1, kEachCall},     // the same for a team (< 0: 1024, 0: never)
  {"EK_SB2ST_CHASE", 0, kOnce},                       // 1: sweeps through memory only, 2 (and 0): positions in registers
  {"EK_SB2ST_WGS", 0, kEachCall},                     // set: sweeps through memory, with this many workgroups if > 0
  {"EK_SB2ST_JITTER", 0, kEachCall},                  // seed of the pauses that shake the position kernel's timing (0: none)
  {"EK_SB2ST_CENSUS_SPINS", 1 << 16, kEachCall},      // polls a workgroup of the position kernel waits for the others
  {"EK_Q2_NBLK", 0, kEachCall},                       // 2, 3, 4: blocks of sweeps per pass of Q2 (else by the order)
};

// the variable's text as it stands now (nullptr: unset)
inline const char *switch_text(Switch s) { return getenv(kSwitches[s].name); }

// the value at the first call of this function for s
inline int switch_once(Switch s) {
  static int value[kSwCount];
  static bool read[kSwCount];
  if (!read[s]) { const char *e = switch_text(s); value[s] = e ? atoi(e) : kSwitches[s].unset; read[s] = true; }
  return value[s];
}

// the value by the row's policy
inline int switch_int(Switch s) {
  if (kSwitches[s].read == kOnce) return switch_once(s);
  const char *e = switch_text(s);
  return e ? atoi(e) : kSwitches[s].unset;
}

}  // namespace ek
