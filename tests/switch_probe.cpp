// Stand-alone check of csrc/ek_switch.h (built and run by tests/test_switches_host.py under the address and
// undefined-behaviour sanitizers): what an unset, a numeric, an empty and a non-numeric variable stand for, and which
// rows see a change of the variable after their first read.
#include "ek_switch.h"

#include <cstdio>
#include <cstring>
#include <initializer_list>

using namespace ek;

static int failures = 0;
static void expect(bool ok, const char *what) { if (!ok) { fprintf(stderr, "FAILED: %s\n", what); ++failures; } }
static void set(Switch s, const char *v) { if (v) setenv(kSwitches[s].name, v, 1); else unsetenv(kSwitches[s].name); }

int main() {
  for (int s = 0; s < kSwCount; ++s) unsetenv(kSwitches[s].name);
  // a row read at every use (the parent: pair_min = 5120; if (e) pair_min = atoi(e))
  static_assert(kSwitches[kSwPairMin].read == kEachCall, "");
  expect(switch_int(kSwPairMin) == 5120, "each call: unset is the default");
  set(kSwPairMin, "12"); expect(switch_int(kSwPairMin) == 12, "each call: 12");
  set(kSwPairMin, ""); expect(switch_int(kSwPairMin) == 0, "each call: empty is 0");
  set(kSwPairMin, "abc"); expect(switch_int(kSwPairMin) == 0, "each call: abc is 0");
  set(kSwPairMin, nullptr); expect(switch_int(kSwPairMin) == 5120, "each call: unset again is the default again");
  // rows read once (the parent: a function-local static per site), one fresh row per case
  static_assert(kSwitches[kSwLookaheadMin].read == kOnce && kSwitches[kSwTwoStageMin].read == kOnce &&
                kSwitches[kSwPipeLower].read == kOnce && kSwitches[kSwPlacement].read == kOnce, "");
  expect(switch_int(kSwLookaheadMin) == 5120, "once: unset is the default");
  set(kSwLookaheadMin, "12"); expect(switch_int(kSwLookaheadMin) == 5120, "once: a later value is not seen");
  set(kSwTwoStageMin, "12"); expect(switch_int(kSwTwoStageMin) == 12, "once: 12");
  set(kSwTwoStageMin, "7"); expect(switch_int(kSwTwoStageMin) == 12, "once: a later change is not seen");
  set(kSwTwoStageMin, nullptr); expect(switch_int(kSwTwoStageMin) == 12, "once: nor is a later unset");
  set(kSwPipeLower, ""); expect(switch_int(kSwPipeLower) == 0, "once: empty is 0");
  set(kSwPlacement, "abc"); expect(switch_int(kSwPlacement) == 0, "once: abc is 0");
  // EK_HIP_PIPE_TRACE: on / off from the first read, the level at every use
  static_assert(kSwitches[kSwPipeTrace].read == kOnceAndEachCall, "");
  set(kSwPipeTrace, "2"); expect(switch_once(kSwPipeTrace) == 2 && switch_int(kSwPipeTrace) == 2, "trace: 2");
  set(kSwPipeTrace, "0"); expect(switch_once(kSwPipeTrace) == 2 && switch_int(kSwPipeTrace) == 0, "trace: kept on, level 0");
  // the text row, as it stands at every use
  static_assert(kSwitches[kSwRcclLib].read == kEachCall, "");
  expect(switch_text(kSwRcclLib) == nullptr, "text: unset is no name");
  for (const char *v : {"12", "", "abc"}) {
    set(kSwRcclLib, v);
    expect(switch_text(kSwRcclLib) && !strcmp(switch_text(kSwRcclLib), v), "text: the value as it stands");
  }
  if (!failures) printf("switch probe ok\n");
  return failures ? 1 : 0;
}
