// ek_solve.hip -- the whole path behind the reference's solver arms (solver_main.f90:52-99) on device-resident data: the
// plan of its workspace, the Path (one method per stage; solve_device_locked runs it), and the C entries of
// include/ek_hip.h on device arrays (ek_hip_solve_device*, ek_hip_eigenvalues_device, ek_hip_eigenpairs_device,
// ek_hip_sygvx_device).  The entries on host arrays and their staging pipeline are ek_solve_host.hip.
#include "ek_api_internal.h"

namespace ek {
namespace api {

// all-gather of the packed band of a team whose members hold the columns of their own strips (strip S on rank S mod P):
// one exchange per round of P strips
void gather_band_strips(hipStream_t s, int n, int nmem, int rank0, double *const *ABs, const SytrdExchange &x) {
  const int NRB = ceil_div(n, 128), P = x.nranks;
  if (P <= 1) return;
  for (int q = 0; q * P < NRB; ++q) {
    size_t offs[kMaxTeam], counts[kMaxTeam];
    for (int r = 0; r < P; ++r) {
      const int S = q * P + r;
      const int cols = (S < NRB) ? ((n - S * 128 < 128) ? n - S * 128 : 128) : 0;
      offs[r] = (S < NRB) ? (size_t)S * 128 * kBandLd : 0; counts[r] = (size_t)cols * kBandLd;
    }
    x.allgatherv(s, nmem, rank0, ABs, offs, counts, P, x.user);
  }
}

}  // namespace api
}  // namespace ek

using namespace ek;
using namespace ek::api;

namespace {

struct StageTimer {      // events are released when the timer goes out of scope, whichever way the call ends
  hipEvent_t ev[EK_HIP_N_STAGES + 1];
  int made = 0;
  int init() {
    for (auto &e : ev) { EK_HIP_CHECK(hipEventCreate(&e)); ++made; }
    return 0;
  }
  ~StageTimer() { for (int i = 0; i < made; ++i) (void)hipEventDestroy(ev[i]); }
};

// Workspace of one whole-path call, laid out by LIFETIME.  What a stage needs lives in one of
//   persistent : L (wB) and the first stage's reflectors (wV) -- operators every rank applies in full to its own
//                eigenvector columns at the end --, the eigenvector columns this call forms (wZ: n x n on one GPU, a grid
//                cell's share n x n/P on a team), the small vectors, the band and the bulge chasing's mail;
//   X0 (one matrix): the matrix A from the stage-in to the end of dense -> band, THEN the bulge chasing's reflectors V2
//                (what the call leaves in A goes back to the caller in between);
//   X1         : the scratch of the reduction to standard form and of the Cholesky factorisation, THEN the divide &
//                conquer's bases (compact for a cell's share: 1.5 n^2 + n n/P; 2 n^2 for the full spectrum on one GPU),
//                THEN the compact-WY records of Q2 (1.55 n^2, made from V2 after the D&C), THEN the scratch of Q1.
// (a bulge chasing that abandons a bounded wait is repeated from the band it started from: no copy of the reduced matrix)
int g_debug_fail_chase = 0;     // test aid (ek_hip_debug_fail_next_chase): pretend the next k bulge chasings abandoned a wait
int g_debug_dc_team = 0;        // rehearsal aid (ek_hip_debug_stedc_team): a grid cell WITHOUT a communicator plays every rank of a
                                // team of that many in the divide & conquer's sharded heights (one GPU: tests, tools/team_timing.py)

struct PathPlan {
  int ld, nblk, zcols;
  bool two_stage, potrf_rl, compact_dc;
  size_t mat, zmat, x0, x1, sygst_dbl, potrf_wb, wb_sytrd, wb_stedc, wb_ormtr, wb_sy2sb, wb_sb2st, wb_rec, wb_q1prep,
         trsm_work, inv256, total;
};
// values_only: the plan of an eigenvalues-only call (ek_hip_eigenvalues*): the stages up to the tridiagonalisation, then
// the bisection -- no eigenvector array, no records of Q2, no scratch of Q1, of the D&C or of the back-transformation;
// X1 is then [phase A | the bisection's scratch] (never distributed).
// value_window: a RANGE = 'V' call with eigenvectors (ek_hip_eigenpairs*), whose m is known only after the
// tridiagonalisation: the full plan (n_vec = nc_loc = n), with X1 grown where the window's own D&C (compact for
// m <= n - n/2) or back-transformation scratch could need more for some m -- a few n doubles on odd orders, nothing on
// the even orders the tests check (256 ... 32768).
PathPlan plan_path(int problem, int n, int n_vec, int nc_loc, int nranks_dist /* 0: not distributed */,
                   size_t exch_bytes = 0 /* X1's last life: the eigenvector pieces on their way between the cells of a process column */,
                   bool values_only = false, bool value_window = false) {
  PathPlan p{};
  const bool dist = nranks_dist > 0;
  p.ld = pad_ld(n); p.nblk = ceil_div(n, kDiagNB);
  const int ts_min = two_stage_min();
  p.two_stage = ts_min > 0 && n >= ts_min && n >= 3;
  p.mat = al((size_t)p.ld * p.ld * 8);
  // the eigenvector work array holds the columns this call forms only (a grid cell's share, or the first n_vec of a
  // *_select arm) where the D&C can keep its bases compact; else it is n x n and doubles as the D&C's scratch
  p.compact_dc = stedc_compact(n, nc_loc);
  p.zcols = p.compact_dc ? round_up(nc_loc > 0 ? nc_loc : 1, 128) : p.ld;
  p.zmat = al((size_t)p.ld * p.zcols * 8);
  p.wb_sytrd = (p.two_stage) ? 0 : (dist ? sytrd_dist_work_bytes(n, nranks_dist) : sytrd_work_bytes(n));
  p.wb_stedc = stedc_work_bytes(n, nc_loc);
  p.wb_ormtr = ormtr_work_bytes(n, nc_loc, n_vec);
  p.trsm_work = al((size_t)256 * p.ld * 8);       // (a leaf of the solves writes its m x 256 result here before it goes back)
  p.inv256 = (problem == 1) ? al((size_t)(n / 256 > 0 ? n / 256 : 1) * 256 * 256 * 8) : 0;   // 256-block inverses of L
  p.sygst_dbl = (problem == 1) ? sygst_scratch_doubles(n) : 0;
  if (problem == 1 && dist) {
    const size_t dd = sygst_dist_scratch_doubles(n, p.ld, nranks_dist);
    if (dd > p.sygst_dbl) p.sygst_dbl = dd;
  }
  // right-looking Cholesky with look-ahead from this order on (below it the recursion is as fast)
  p.potrf_rl = problem == 1 && n >= kPotrfRlMin;
  p.potrf_wb = (problem == 1 && dist) ? al(potrf_dist_work_bytes(n, p.ld, nranks_dist)) : 0;
  if (p.potrf_rl && al(potrf_rl_work_bytes(n, p.ld)) > p.potrf_wb) p.potrf_wb = al(potrf_rl_work_bytes(n, p.ld));
  p.wb_sy2sb = p.two_stage ? al(dist ? sy2sb_dist_work_bytes(n, nranks_dist) : sy2sb_work_bytes(n)) : 0;
  p.wb_sb2st = p.two_stage ? al(sb2st_work_bytes(n, /*with_records=*/false)) : 0;
  p.wb_rec = p.two_stage ? al(sb2st_record_bytes(n)) : 0;
  p.wb_q1prep = p.two_stage ? al(ormtr_prep_bytes(n)) : 0;
  p.x0 = p.mat;
  const size_t phase_a = al(p.sygst_dbl * 8) + p.potrf_wb + al(p.wb_sytrd) + 512;   // [reduction | Cholesky | one-stage scratch]
  p.x1 = phase_a;
  if (values_only) {
    p.zcols = 0; p.zmat = 0; p.wb_stedc = 0; p.wb_ormtr = 0; p.wb_rec = 0; p.wb_q1prep = 0;
    if (al(stebz_work_bytes(n)) > p.x1) p.x1 = al(stebz_work_bytes(n));
    if (p.x1 < 4096) p.x1 = 4096;          // (the stage-in's partial maxima)
  }
  if (al(p.wb_stedc) > p.x1) p.x1 = al(p.wb_stedc);
  if (p.wb_rec > p.x1) p.x1 = p.wb_rec;
  if (al(p.wb_ormtr) > p.x1) p.x1 = al(p.wb_ormtr);
  if (al(exch_bytes) > p.x1) p.x1 = al(exch_bytes);
  if (value_window) {
    const size_t dc = al(stedc_work_bytes(n, n - n / 2));          // the compact D&C's largest selection
    if (dc > p.x1) p.x1 = dc;
    for (int c = 128; ; c += 128) {                                 // Q1 on m columns (its K split is a step function of m)
      const int mc = c < n ? c : n;
      if (al(ormtr_work_bytes(n, mc, mc)) > p.x1) p.x1 = al(ormtr_work_bytes(n, mc, mc));
      if (mc == n) break;
    }
  }
  p.total = 2 * p.mat + p.zmat + p.x0 + p.x1 + al((size_t)p.nblk * kDiagNB * kDiagNB * 8) + p.trsm_work +
            5 * al((size_t)p.ld * 8) + p.wb_sy2sb + p.wb_sb2st + p.wb_q1prep + p.inv256 + 4096;
  return p;
}

// Runs the path on user device arrays dA, dB, dZ (column-major, any ld >= n) by way of padded
// internal work arrays (ld multiple of 128, zero padding), so the kernels see aligned tiles.
//
// cell == nullptr: dZ receives the first n_vec eigenvectors (n x n_vec).  Otherwise the reduction
// and the tridiagonal eigenproblem are computed as usual (replicated on every rank) and only the
// eigenvector columns this grid cell owns are back-transformed; dZ receives the local
// block-cyclic piece numroc(n, nb, myrow, nprow) x numroc(n_vec, nb, mycol, npcol).
//
// win != nullptr: a window of the spectrum (1 x 1, no pipeline; ek_hip_eigenvalues*, ek_hip_eigenpairs*).
//   range 0: indices win->il..iu; range 1: the eigenvalues in (vl, vu], counted on the tridiagonal after stage 4 (the
//   bounds scaled as A was), which sets il and iu.  win->first = il - 1 and win->m = iu - il + 1 come back.
//   jobz 0: the bisection for il..iu in the D&C's slot, dw receives m doubles; n_vec, dZ and ldz are not referenced.
//   jobz 1: the D&C forms eigenvectors il..iu only (its rank offset), Q2, Q1 and the recovery treat those m columns, dw
//   receives their m eigenvalues and dZ (ldz) the m columns.  The caller passes n_vec = m for range 0 (the *_select
//   arm's plan) and n_vec = n for range 1 (the full plan); range 1 with m > win->zcap returns kWindowTooSmall before dw
//   or dZ is written.
//   dA / dB come back as after the full path's tridiagonalisation (A) and Cholesky factorisation (B).
//
// itype (problem 1, 1 x 1, no grid cell; ek_hip_sygvx*): the generalized problem of DSYGVX -- 1: A x = l B x, the
// reduction C = L^-1 A L^-T and the recovery x = L^-T y; 2: A B x = l x, C = L^T A L and x = L^-T y; 3: B A x = l x,
// C = L^T A L and x = L y.  Everything between the reduction and the recovery is the same for all three, and so is the
// plan: the multiplies' masked diagonal blocks of L live in the array of Q1's reflectors (wV), which is free during the
// reduction (zeroed again behind it) and after Q1.
//
// The Path holds one call: its constructor lays the call out (modes, plan, workspace, the work arrays' places), run()
// issues the stages in order, each a method.  An error return leaves through the destructors of its members.
struct Inv256Guard { ~Inv256Guard() { trsm_register_inv256(nullptr, nullptr, 0); } };   // (whichever way the call ends)
struct Path : PathCall {       // (its own copy of the request: a value window sets n_vec to its m)
  explicit Path(const PathCall &call);
  int run();
  int rc = 0;                  // what the lay-out found: run() returns it before anything is issued
  hipStream_t s = g_ctx.stream;
  // modes: the piece of Z this call returns (nr_loc x nc_out) and the columns it FORMS (nc_loc; a value window: its m)
  int nc_out = 0, nr_loc = 0, nc_loc = 0;
  bool dist = false, split_rows = false, values_only = false, value_window = false;
  // the plan and the work arrays' places
  PathPlan pl{};
  int ld = 0;
  bool two_stage = false, aliasA = false, aliasB = false, aliasZ = false;
  double *wB = nullptr, *wV = nullptr, *wZ = nullptr, *x0 = nullptr, *dInv = nullptr, *twork = nullptr, *dd = nullptr,
         *de = nullptr, *dt = nullptr, *dwv = nullptr, *dt1 = nullptr, *inv256 = nullptr;
  char *x1 = nullptr, *work_sy2sb = nullptr, *work_sb2st = nullptr, *q1prep = nullptr;
  double *wA = nullptr, *wV2 = nullptr;   // X0's two lives: the matrix (unless the caller's array serves), the chase's reflectors
  // X1, phase A: the scratch of the reduction, of the Cholesky factorisation and of the one-stage tridiagonalisation
  double *sscr = nullptr; char *pwork = nullptr; void *sytrd_work = nullptr;
  char *work = nullptr; double *q2rec = nullptr;   // X1 as the scratch of the D&C / of Q1, and as the records of Q2
  Inv256Guard inv256_guard;
  StageTimer tm;
  bool timing = false;
  int evi = 0;
  void mark() { if (timing) (void)hipEventRecord(tm.ev[evi++], s); }
  // what the stages hand on
  double sigma = 1.0;          // A was scaled by it
  bool band_input = false;     // a standard problem whose matrix is already a band of half width 64: no first stage, Q1 = I
  bool two_stage_done = false, window_too_small = false;
  double rescued_panels = 0.0;
  int zslab = 0;               // columns of Z per slab of the last stage (a staging pipeline; else all of them)
  // the stages in run()'s order, and their helpers
  int stage_in_A(), stage_in_B(), reduce(), tridiagonalise(), chase_with_repeat(), count_window(), values_tail(),
      divide_and_conquer(), stage_out(), finish(bool full), slab_width(int c0) const;
  void cholesky(), a_out(), back_transform(), recover(), z_out(int c0, int nc), exchange_rows();
};

Path::Path(const PathCall &call) : PathCall(call) {
  nc_out = cell ? numroc0(n_vec, cell->nb, cell->mycol, cell->npcol) : n_vec;    // columns of the piece of Z this call returns
  nr_loc = cell ? numroc0(n, cell->nb, cell->myrow, cell->nprow) : n;
  // A communicator attached by the host (ek_hip_comm_init) whose size is the grid's: the Cholesky factorisation, the
  // reduction and the dense -> band stage of the tridiagonalisation are distributed over the ranks (1 x P team, per panel
  // one broadcast and one all-reduce; below the two-stage orders the one-stage form with its per-column exchange); the
  // other stages are as in the replicated-input mode.
  dist = cell && g_comm.on && g_comm.nranks == cell->nprow * cell->npcol;
  if (dist && g_comm.rank != cell->myrow * cell->npcol + cell->mycol) { rc = -994; return; }
  // On a grid with more than one process ROW the cells of a process column would all form the same eigenvector columns
  // (each keeping its rows): with a communicator they split them instead -- cell (i, j) forms the blocks l of its process
  // column's share with l mod nprow = i, which is the block-cyclic share of world rank i * npcol + j among all P ranks
  // -- and exchange row pieces pairwise at the end (team_sendrecv): 1 / P of the back-transformations and of the recovery
  // on every rank whatever the grid's shape, as PDORMTR / PDTRTRS have it on the reference's 2 x 4 grid
  // (solver_scalapack_all.f90:115, generalized_to_standard.f90:103, processes.f90:56-65).
  split_rows = dist && cell->nprow > 1;
  nc_loc = split_rows ? numroc0(n_vec, cell->nb, g_comm.rank, g_comm.nranks) : nc_out;
  size_t exch_bytes = 0;
  if (split_rows) exch_bytes = ((size_t)n * (nc_loc > 0 ? nc_loc : 1) + (size_t)(nr_loc > 0 ? nr_loc : 1) * (nc_out > 0 ? nc_out : 1)) * 8 + 4096;
  values_only = win && win->jobz == 0;
  value_window = win && win->jobz == 1 && win->range == 1;
  if (win && (cell || pipe)) { rc = -1; return; }
  if (itype != 1 && (problem != 1 || cell)) { rc = -1; return; }
  pl = plan_path(problem, n, n_vec, nc_loc, dist ? g_comm.nranks : 0, exch_bytes, values_only, value_window);
  ld = pl.ld; two_stage = pl.two_stage;
  const int zcols = pl.zcols;
  void *ws;
  g_comm.err = 0;                        // (sticky from here to the end of the call: the votes of the stages keep it)
  rc = workspace(pl.total, &ws);
  if (dist) rc = comm_agree(rc);         // a rank that cannot get its workspace takes the team out with it (-993)
  if (rc) return;
  Arena a(ws, g_ctx.ws_bytes);
  // A caller's device array IS the internal work array when it already has the internal layout (order a multiple of 128,
  // leading dimension = order, 256-byte aligned: the bench's and the host path's arrays at the BASELINE orders): the
  // stage-in / stage-out copies of A, B and Z -- five passes over 2 GiB at N = 16384, 4.4 ms of a 0.86 s solve -- are
  // then not made (EK_HIP_ALIAS=0: always copy).  The plan above keeps its sizes: an upper bound.
  const int alias_env = switch_int(kSwAlias);            // (read per call: the tests switch it)
  auto alias_ok = [&](const double *p, int ldu) {
    return alias_env && p && n % 128 == 0 && ldu == ld && (((size_t)p) & 255) == 0;
  };
  aliasA = alias_ok(dA, lda); aliasB = problem == 1 && alias_ok(dB, ldb);
  aliasZ = !values_only && !value_window && !cell && nc_loc == n && zcols == ld && alias_ok(dZ, ldz);
  // (the order of these is the layout: dd, de, dt and dwv are cleared as one piece, the placement probes see addresses)
  wB = aliasB ? dB : a.get<double>((size_t)ld * ld);
  wV = a.get<double>((size_t)ld * ld);
  wZ = (aliasZ || values_only) ? dZ : a.get<double>((size_t)ld * zcols);
  x0 = a.get<double>((size_t)ld * ld);
  x1 = a.get<char>(pl.x1);
  dInv = a.get<double>((size_t)pl.nblk * kDiagNB * kDiagNB);
  twork = a.get<double>((size_t)256 * ld);
  dd = a.get<double>(ld); de = a.get<double>(ld); dt = a.get<double>(ld); dwv = a.get<double>(ld);
  dt1 = a.get<double>(ld);
  work_sy2sb = two_stage ? a.get<char>(pl.wb_sy2sb) : nullptr;
  work_sb2st = two_stage ? a.get<char>(pl.wb_sb2st) : nullptr;
  q1prep = (two_stage && !values_only) ? a.get<char>(pl.wb_q1prep) : nullptr;
  inv256 = pl.inv256 ? (double *)a.get<char>(pl.inv256) : nullptr;
  wA = aliasA ? dA : x0;
  wV2 = x0;
  sscr = (problem == 1) ? (double *)x1 : nullptr;
  pwork = pl.potrf_wb ? x1 + al(pl.sygst_dbl * 8) : nullptr;
  work = x1;
  q2rec = (double *)x1;
  // (the place is probed once per workspace; the probe overwrites the matrix it is given: X0, never the caller's array)
  char *sytrd_arena = x1 + al(pl.sygst_dbl * 8) + pl.potrf_wb + 256;
  sytrd_work = two_stage ? nullptr : choose_sytrd_scratch(n, ld, x0, sytrd_arena, dd, pl.wb_sytrd);
  timing = stage_seconds && n_stages > 0;
}

// The stages in order, with the nine events 0 .. 8 between them.  With a staging pipeline B comes in first and A is
// waited for only after the Cholesky factorisation has been issued (it is still crossing PCIe meanwhile); L leaves
// only after A is in: the output workers' memcpys would share the host's memory bandwidth with the input that the next
// stage is waiting for -- A came in at 24 GB/s beside them, B alone at 51.
int Path::run() {
  if (rc) return rc;
  if (timing) EK_TRY(tm.init());
  EK_HIP_CHECK(hipMemsetAsync(g_ctx.d_info, 0, 4 * sizeof(int), s));
  mark();                                                              // 0
  EK_HIP_CHECK(hipMemsetAsync(wV, 0, (size_t)ld * ld * 8, s));
  EK_HIP_CHECK(hipMemsetAsync(dd, 0, 4 * al((size_t)ld * 8), s));      // dd, de, dt, dwv
  if (!pipe) EK_TRY(stage_in_A());
  EK_TRY(stage_in_B());
  mark();                                                              // 1
  cholesky();
  mark();                                                              // 2
  if (pipe) {
    EK_TRY(stage_in_A());
    if (problem == 1) {        // L leaves while the reduction runs
      if (!aliasB) copy_matrix(s, n, n, wB, ld, dB, ldb);
      pipe_out(pipe, s, 'B', dB, ldb, n, 0, n);
    }
  }
  EK_TRY(reduce());
  mark();                                                              // 3
  EK_TRY(tridiagonalise());
  mark();                                                              // 4
  EK_TRY(count_window());
  // the bisection takes the D&C's slot; nothing of the back-transformation or of the recovery runs (nor anything after
  // the count for an empty window or one that dZ cannot hold)
  if (values_only || (win && (win->m == 0 || window_too_small))) return values_tail();
  EK_TRY(divide_and_conquer());
  mark();                                                              // 5
  back_transform();
  mark();                                                              // 6
  recover();
  mark();                                                              // 7
  EK_TRY(stage_out());
  mark();                                                              // 8
  return finish(/*full=*/true);
}

// stage-in: padded, zero-filled work copies
int Path::stage_in_B() {
  if (problem != 1) return 0;
  if (pipe) EK_TRY(pipe_wait_in(pipe, 0));
  if (aliasB) return 0;
  if (ld != n) EK_HIP_CHECK(hipMemsetAsync(wB, 0, (size_t)ld * ld * 8, s));
  copy_matrix(s, n, n, dB, ldb, wB, ld);
  return 0;
}

int Path::stage_in_A() {
  if (pipe) EK_TRY(pipe_wait_in(pipe, 1));
  if (!aliasA) {
    if (ld != n) EK_HIP_CHECK(hipMemsetAsync(wA, 0, (size_t)ld * ld * 8, s));   // (the copy covers all of an unpadded array)
    copy_matrix(s, n, n, dA, lda, wA, ld);
  }
  // Scale A into the safe range when its entries are extreme (as DSYEV / PDSYEV do before
  // DSYTRD): the Householder norms are plain sums of squares.  Eigenvalues scale back linearly.
  double *d_part = (double *)work;   // stage scratch, free until the reduction starts
  maxabs_lower(s, n, wA, ld, d_part, kBandW);
  double part[512];
  EK_HIP_CHECK(hipMemcpyAsync(part, d_part, sizeof(part), hipMemcpyDeviceToHost, s));
  EK_HIP_CHECK(hipStreamSynchronize(s));
  double anrm = 0.0, offband = 0.0;
  for (int q = 0; q < 256; ++q) { if (part[q] > anrm) anrm = part[q]; if (!(part[256 + q] <= offband)) offband = part[256 + q]; }
  // the reference's own inputs are sparse Hamiltonians, often banded: a matrix with nothing below its 64th subdiagonal
  // IS the output of the dense -> band stage (EK_HIP_BAND_INPUT=0 turns the short cut off)
  band_input = switch_int(kSwBandInput) != 0 && problem == 0 && !dist && offband == 0.0;
  if (!(anrm <= 1.7e308)) return -4;   // NaN / Inf in A: illegal value, as XERBLA
  // the tridiagonalisation forms x^T A x of the unscaled column (|A|^3 n^2): keep cubes in range
  const double rmin = 1e-90, rmax = 1e90;
  if (anrm > 0.0 && anrm < rmin) sigma = rmin / anrm;
  else if (anrm > rmax) sigma = rmax / anrm;
  if (sigma != 1.0) scale_lower(s, n, sigma, wA, ld);
  return 0;
}

void Path::cholesky() {
  if (problem == 1) {
    // right-looking sweep with one panel broadcast per strip: pays from three ranks on
    if (dist && g_comm.nranks >= dist_min_ranks()) {
      const PotrfMember me{wB, ld, dInv, g_ctx.d_info, pwork, g_comm.rank};
      potrf_lower_dist(s, g_ctx.stream2, n, 1, &me, team_exchange(0));
    } else if (pl.potrf_rl) {
      potrf_lower_rl(s, g_ctx.stream2, n, wB, ld, dInv, g_ctx.d_info, pwork);
    } else {
      potrf_lower(s, n, wB, ld, dInv, g_ctx.d_info, twork);
    }
  }
  // leaves of 256 for the solves of the reduction and of the recovery (ek_chol.hip); types 2 and 3 reduce by multiplies,
  // and only type 2 solves (in the recovery)
  if (problem == 1 && n >= 256 && (itype == 1 || (itype == 2 && !values_only))) {
    trtri256_blocks(s, n, wB, ld, dInv, inv256, twork);
    trsm_register_inv256(dInv, inv256, n);
  }
}

int Path::reduce() {
  if (problem != 1) return 0;
  // sharding the two solves costs 2 n^3 / P flops per rank against 1.0 - 1.57 n^3 replicated
  if (dist && g_comm.nranks >= dist_min_ranks()) {
    const SygstMember me{wA, ld, wB, ld, dInv, twork, sscr, g_comm.rank};
    sygst_lower_dist(s, n, 1, &me, team_exchange(0));
  } else if (itype == 1) {
    sygst_lower(s, n, wA, ld, wB, ld, dInv, twork, sscr);
  } else {
    trmm_diag_blocks(s, n, wB, ld, wV);
    sygst2_lower(s, n, wA, ld, wB, ld, wV, twork, sscr);
    EK_HIP_CHECK(hipMemsetAsync(wV, 0, trmm_diag_doubles(n) * 8, s));   // (as the stage-in left it)
  }
  return 0;
}

// what the call leaves in A -- PDSYTRD's reflectors; after a two-stage reduction the band and the first stage's R factors
//  -- goes back to the caller as soon as it is final: its place (X0) is needed again
void Path::a_out() {
  if (!aliasA) copy_matrix(s, n, n, wA, ld, dA, lda);
  if (pipe) pipe_out(pipe, s, 'A', dA, lda, n, 0, n);
}

int Path::tridiagonalise() {
  if (dist && !two_stage) {
    const SytrdMember me{wA, ld, dd, de, dt, wV, ld, sytrd_work, g_comm.rank};
    sytrd_lower_dist(s, n, 1, &me, team_exchange(0, n));
    a_out();
    return 0;
  }
  if (!two_stage) {
    sytrd_lower(s, n, wA, ld, dd, de, dt, wV, ld, sytrd_work);
    a_out();
    return 0;
  }
  // dense -> band -> tridiagonal.  The panel factorisation of the first stage is CholeskyQR2 with a device-side check;
  // a panel it cannot handle (rank deficient, cond > 1e7: e.g. an input that is nearly banded) is factored by
  // Householder reflections inside the stage (per-panel rescue, ek_sy2sb.hip): the stage never gives up.
  EK_HIP_CHECK(hipMemsetAsync(dt1, 0, (size_t)ld * 8, s));
  double *AB0 = sb2st_band(work_sb2st, n);
  if (dist) {
    // On a team the first stage is distributed over the 128-wide column strips (strip S on rank S mod P: where
    // the distributed reduction to standard form left the matrix, so nothing is gathered in front of it): per panel
    // one broadcast of [V | T | tau] and one all-reduce of Y, the next panel's chain and broadcast on the second stream
    // beside the rest of the update (ek_sy2sb.hip).  Then ONE all-gather of the band (65 n doubles); the bulge chasing
    // and the D&C below its top merge run replicated, bit-identical on all ranks.
    const SytrdExchange x = team_exchange(0);
    const Sy2sbMember me{wA, ld, wV, ld, dt1, g_ctx.d_info + 2, work_sy2sb, g_comm.rank};
    sy2sb_lower_dist(s, g_ctx.stream2, n, 1, &me, x);
    double *ABs[1] = {AB0};
    pack_band(s, n, wA, ld, AB0);
    gather_band_strips(s, n, 1, g_comm.rank, ABs, x);
  } else {
    if (!band_input) sy2sb_lower(s, g_ctx.stream2, n, wA, ld, wV, ld, dt1, g_ctx.d_info + 2, work_sy2sb);
    pack_band(s, n, wA, ld, AB0);
  }
  a_out();                               // X0 changes hands: the matrix leaves, the reflectors of the chase move in
  EK_HIP_CHECK(hipMemsetAsync(wV2, 0, (size_t)ld * ld * 8, s));
  sb2st_lower(s, n, nullptr, 0, dd, de, wV2, ld, g_ctx.d_info + 2, work_sb2st, /*band_packed=*/true);
  return chase_with_repeat();
}

// The low byte of the flag says that the bulge chasing abandoned a bounded wait (a matter of timing, not of the
// data; nothing has raised it yet).  The stage is then repeated from the band it started from -- kept beside the
// working copy -- with the older kernel alone, twice at most.  A team decides together: a flag that only one rank
// has raised must not leave the ranks with eigenvectors of two different decompositions.
int Path::chase_with_repeat() {
  for (int attempt = 0; ; ++attempt) {
    int flag = 0;
    EK_HIP_CHECK(hipMemcpyAsync(&flag, g_ctx.d_info + 2, sizeof(int), hipMemcpyDeviceToHost, s));
    EK_HIP_CHECK(hipStreamSynchronize(s));
    rescued_panels = (double)(flag >> 8);      // panels of the first stage that took the Householder rescue
    if (g_debug_fail_chase > 0) { --g_debug_fail_chase; flag |= 4; }
    int low = flag & 0xff;
    if (dist) { low = comm_any(low); if (low < 0) return low; }
    if (low == 0) { two_stage_done = true; return 0; }
    if (attempt == 2) return -992;
    flag &= ~0xff;
    EK_HIP_CHECK(hipMemcpyAsync(g_ctx.d_info + 2, &flag, sizeof(int), hipMemcpyHostToDevice, s));
    EK_HIP_CHECK(hipStreamSynchronize(s));
    EK_HIP_CHECK(hipMemsetAsync(wV2, 0, (size_t)ld * ld * 8, s));
    sb2st_lower(s, n, nullptr, 0, dd, de, wV2, ld, g_ctx.d_info + 2, work_sb2st, /*band_packed=*/true, /*chase_mode=*/1);
  }
}

// a window's il, iu, first and m, and whether dZ can hold it
int Path::count_window() {
  if (!win) return 0;
  if (win->range == 1) {
    // the value window's indices: one count at each bound on the tridiagonal (X1 is free until the D&C), read back here
    const int *d_ilu = stebz_window(s, n, dd, de, win->vl * sigma, win->vu * sigma, x1);
    int ilu[2] = {1, 0};
    EK_HIP_CHECK(hipMemcpyAsync(ilu, d_ilu, sizeof(ilu), hipMemcpyDeviceToHost, s));
    EK_HIP_CHECK(hipStreamSynchronize(s));
    win->il = ilu[0]; win->iu = ilu[1] >= ilu[0] ? ilu[1] : ilu[0] - 1;
  }
  win->first = win->il - 1;
  win->m = win->iu - win->il + 1;
  window_too_small = win->jobz == 1 && win->m > win->zcap;
  return 0;
}

// the rest of a call that forms no eigenvectors: kWindowTooSmall comes back before dw or dZ is written
int Path::values_tail() {
  const int m = win->m;
  if (values_only && m > 0) stebz(s, n, dd, de, win->il, win->iu, dwv, x1);
  mark(); mark(); mark();                                            // 5, 6, 7
  if (values_only && m > 0 && sigma != 1.0) scale_vector(s, m, 1.0 / sigma, dwv);
  if (values_only && m > 0) EK_HIP_CHECK(hipMemcpyAsync(dw, dwv, (size_t)m * 8, hipMemcpyDeviceToDevice, s));
  if (problem == 1 && !aliasB) copy_matrix(s, n, n, wB, ld, dB, ldb);
  mark();                                                            // 8
  EK_TRY(finish(/*full=*/false));
  return window_too_small ? kWindowTooSmall : 0;
}

int Path::divide_and_conquer() {
  if (value_window) { nc_loc = win->m; n_vec = win->m; }   // (the plan holds any m; the columns formed are m)
  // eigenvector columns wanted: the first n_vec, or this grid cell's share of them; the D&C
  // forms only those (columns 0..nc_loc-1 of wZ) and the two remaining stages treat the
  // columns of Z independently
  const StedcSelect pick{nc_loc, cell ? cell->nb : (n > 0 ? n : 1), split_rows ? g_comm.nranks : (cell ? cell->npcol : 1),
                         split_rows ? g_comm.rank : (cell ? cell->mycol : 0), win ? win->first : 0};
  // On a team the heights right below the top merge are sharded as well (strips of the compact bases, one all-gather
  // round per P strips: ek_stedc.hip); the top merge forms this cell's columns only, as in the replicated-input mode.
  SytrdExchange dcx{};
  StedcTeam dct{0, 0, nullptr, 0};
  if (dist && g_comm.nranks >= 2) {
    // (the team form needs the compact bases, and EVERY rank must take the same decision or the all-gathers never meet:
    // a team of two on a ragged order can leave one rank with more than half of the columns -- then nobody shards)
    const int P = g_comm.nranks, nbz = cell->nb, Pc = split_rows ? P : cell->npcol;
    bool all_compact = true;
    for (int r = 0; r < Pc; ++r) all_compact = all_compact && stedc_compact(n, numroc0(n_vec, nbz, r, Pc));
    dcx = team_exchange(0);
    dct = StedcTeam{P, g_comm.rank, &dcx, all_compact ? stedc_team_levels(n, P) : 0};
  }
  else if (cell && !dist && g_debug_dc_team >= 2) dct = StedcTeam{g_debug_dc_team, -1, nullptr, stedc_team_levels(n, g_debug_dc_team)};
  stedc(s, n, dd, de, dwv, wZ, ld, work, g_ctx.d_info + 1, &pick, g_ctx.d_stats, nullptr, dct.levels > 0 ? &dct : nullptr);
  return 0;
}

// (the last slabs are narrower: what remains exposed at the end of the call is the last slab's way out)
int Path::slab_width(int c0) const {
  const int left = nc_loc - c0;
  if (zslab >= nc_loc) return left;
  if (left > 2 * zslab) return zslab;
  if (left > zslab) return zslab / 2 < left ? zslab / 2 : left;
  return (left > 512) ? (left + 1) / 2 : left;
}

void Path::z_out(int c0, int nc) {
  if (!aliasZ) copy_matrix(s, n, nc, wZ + (size_t)c0 * ld, ld, dZ + (size_t)c0 * ldz, ldz);
  pipe_out(pipe, s, 'Z', dZ, ldz, n, c0, nc);
}

void Path::back_transform() {
  // with a staging pipeline the LAST stage (the recovery; the back-transformation of a standard problem) runs in column
  // slabs, each leaving for the host while the next is computed (columns of Z are independent there)
  zslab = (pipe && two_stage_done && nc_loc > pipe_z_slab(pipe)) ? pipe_z_slab(pipe) : nc_loc;
  if (two_stage_done) {
    // (the records of Q2 are made from V2 here, after the D&C whose scratch they take over)
    sb2st_apply_q2(s, n, nc_loc, wV2, ld, wZ, ld, g_ctx.d_info + 2, work_sb2st, q2rec);
    // (the T factors of the block reflectors do not depend on Z; forming them on the second stream beside the
    // bulge chasing was measured: the skinny GEMMs take CUs and issue slots from the latency-bound pipeline,
    // which loses 11 ms to gain 6)
    const bool q1 = !band_input;               // (a band on entry: the first stage did nothing, Q1 = I)
    if (q1) ormtr_prepare(s, n, wV, ld, dt1, q1prep);
    if (pipe && problem == 0 && zslab < nc_loc) {
      for (int c0 = 0, nc = 0; c0 < nc_loc; c0 += nc) {
        nc = slab_width(c0);
        if (q1) ormtr_apply(s, n, nc, wV, ld, q1prep, wZ + (size_t)c0 * ld, ld, work, n_vec);
        z_out(c0, nc);
      }
    } else if (q1) {
      ormtr_apply(s, n, nc_loc, wV, ld, q1prep, wZ, ld, work, n_vec);
    }
  } else {
    ormtr_lower(s, n, nc_loc, wV, ld, dt, wZ, ld, work, n_vec);
  }
}

// x = L^-T y (types 1, 2) or x = L y (type 3, against the masked blocks of L in wV: Q1 is done with it); with a
// staging pipeline in slabs, each leaving behind it (a standard problem's Z leaves here unless Q1's slabs took it)
void Path::recover() {
  if (problem != 1) {
    if (pipe && !(two_stage_done && zslab < nc_loc)) z_out(0, nc_loc);
    return;
  }
  if (itype == 3) trmm_diag_blocks(s, n, wB, ld, wV);
  auto apply = [&](int nc, double *zp) {
    if (itype == 3) trmm_lln(s, n, nc, wB, ld, wV, trmm_block_ld(n), zp, ld, twork);
    else trsm_llt(s, n, nc, wB, ld, dInv, zp, ld, twork);
  };
  if (!pipe) { apply(nc_loc, wZ); return; }
  for (int c0 = 0, nc = 0; c0 < nc_loc; c0 += nc) {
    nc = slab_width(c0);
    apply(nc, wZ + (size_t)c0 * ld);
    z_out(c0, nc);
  }
}

// stage-out: eigenvalues, eigenvectors, and the in-place results the reference leaves behind (L in B; the reflectors
// in A left with a_out)
int Path::stage_out() {
  const int nw = win ? win->m : n;                      // (a window: its own eigenvalues, from rank first on)
  double *wsrc = win ? dwv + win->first : dwv;
  if (sigma != 1.0) scale_vector(s, nw, 1.0 / sigma, wsrc);
  EK_HIP_CHECK(hipMemcpyAsync(dw, wsrc, (size_t)nw * 8, hipMemcpyDeviceToDevice, s));
  if (pipe) return 0;                                   // (Z left in slabs, L behind the Cholesky factorisation)
  if (split_rows) exchange_rows();
  else if (cell) gather_block_cyclic(s, nr_loc, nc_loc, wZ, ld, cell->nb, cell->nprow, cell->myrow, 1, 0, dZ, ldz);
  else if (!aliasZ) copy_matrix(s, n, n_vec, wZ, ld, dZ, ldz);
  if (problem == 1 && !aliasB) copy_matrix(s, n, n, wB, ld, dB, ldb);
  return 0;
}

// every cell of this process column receives its rows of the columns the others formed: per peer one packed piece
// each way (X1, free by now), then the pieces' columns take their places in the cell's block-cyclic piece
void Path::exchange_rows() {
  const int nb = cell->nb, R = cell->nprow, C = cell->npcol, P = g_comm.nranks;
  double *buf = (double *)x1;
  int peers[kMaxTeam]; double *sp[kMaxTeam], *rp[kMaxTeam]; size_t sc[kMaxTeam], rcn[kMaxTeam];
  int np = 0;
  double *own = nullptr;
  for (int i = 0; i < R; ++i) {               // what goes out (and this cell's own rows of its own columns)
    const int nr_i = numroc0(n, nb, i, R);
    const size_t cnt = (size_t)nr_i * nc_loc;
    if (cnt > 0) gather_block_cyclic(s, nr_i, nc_loc, wZ, ld, nb, R, i, 1, 0, buf, nr_i > 1 ? nr_i : 1);
    if (i == cell->myrow) own = buf;
    else { peers[np] = i * C + cell->mycol; sp[np] = buf; sc[np] = cnt; ++np; }
    buf += cnt;
  }
  for (int i = 0, q = 0; i < R; ++i) {        // what comes in
    if (i == cell->myrow) continue;
    rcn[q] = (size_t)nr_loc * numroc0(n_vec, nb, i * C + cell->mycol, P);
    rp[q] = buf; buf += rcn[q]; ++q;
  }
  team_sendrecv(s, np, peers, sp, sc, rp, rcn);
  const int ldp = nr_loc > 1 ? nr_loc : 1;
  for (int i = 0, q = 0; i < R; ++i) {
    const int nc_i = numroc0(n_vec, nb, i * C + cell->mycol, P);
    const double *src = (i == cell->myrow) ? own : rp[q++];
    scatter_block_cyclic(s, nr_loc, nc_i, src, ldp, nb, 1, 0, R, i, dZ, ldz);
  }
}

// The end of every call that got this far: info, what ek_hip_debug_last_solve_stats reports, the events' times as
// stage seconds, the return code.  full: the call formed eigenvectors -- the D&C's counters are read back, Q1's and the
// recovery's times count, and the team votes on the abandoned wait of Q2 (-992) and on its exchanges (-996), which go
// before the Cholesky factorisation's info and the D&C's (100000 + ...).
int Path::finish(bool full) {
  EK_HIP_CHECK(hipGetLastError());
  int info[4] = {0, 0, 0, 0};
  EK_HIP_CHECK(hipMemcpyAsync(info, g_ctx.d_info, sizeof(info), hipMemcpyDeviceToHost, s));
  if (full) EK_HIP_CHECK(hipMemcpyAsync(g_ctx.stats, g_ctx.d_stats, sizeof(g_ctx.stats), hipMemcpyDeviceToHost, s));
  EK_HIP_CHECK(hipStreamSynchronize(s));
  if (!full) g_ctx.stats[0] = 0.0;
  g_ctx.stats[1] = two_stage_done ? 1.0 : 0.0;
  g_ctx.stats[2] = rescued_panels;
  g_ctx.stats[3] = (two_stage_done && band_input) ? 1.0 : 0.0;      // the band short cut was taken
  if (timing) {
    float ms[8];
    for (int i = 0; i < 8; ++i) (void)hipEventElapsedTime(&ms[i], tm.ev[i], tm.ev[i + 1]);
    double st[EK_HIP_N_STAGES] = {0};                                // (GATHER: 0)
    st[EK_STAGE_COPY] = (ms[0] + ms[7]) * 1e-3;
    st[EK_STAGE_POTRF] = ms[1] * 1e-3; st[EK_STAGE_SYGST] = ms[2] * 1e-3;
    st[EK_STAGE_SYTRD] = ms[3] * 1e-3; st[EK_STAGE_STEDC] = ms[4] * 1e-3;
    if (full) { st[EK_STAGE_ORMTR] = ms[5] * 1e-3; st[EK_STAGE_TRTRS] = ms[6] * 1e-3; }
    for (int i = 0; i < n_stages && i < EK_HIP_N_STAGES; ++i) stage_seconds[i] = st[i];
  }
  if (full) {
    // the pipelined back-transformation was abandoned (a bounded wait ran out): on a team, for all ranks -- and an
    // exchange that failed on ANY rank (its sticky record travels in the same vote) ends the call on all of them
    int bad = two_stage_done && (info[2] & 0xff) != 0;
    if (dist) {
      bad = comm_any(bad);
      if (bad < 0) {
        if (g_comm.err) fprintf(stderr, "[ek_hip] exchange failed: %s\n", comm_error_string());
        return -996;
      }
    }
    if (bad) return -992;
  }
  if (info[0] != 0) return info[0];          // Cholesky: leading minor not positive definite
  if (full && info[1] != 0) return 100000 + info[1];  // tridiagonal eigensolver did not converge
  return 0;
}

}  // namespace

extern "C" {

int ek_hip_solve_device(int problem, int n, int n_vec, double *dA, int lda, double *dB, int ldb,
                        double *dw, double *dZ, int ldz, double *stage_seconds, int n_stages) {
  int rc = solve_args(problem, n, n_vec, dA, lda, dB, ldb, dw, dZ); if (rc) return rc;
  if (ldz < (n > 1 ? n : 1)) return -10;
  rc = ensure_init(); if (rc) return rc;
  if (n == 0) return 0;
  std::lock_guard<std::mutex> lk(g_mu);
  return solve_device_locked(path_call(problem, n, n_vec, dA, lda, dB, ldb, dw, dZ, ldz, stage_seconds, n_stages));
}

int ek_hip_eigenvalues_device(int problem, int n, int il, int iu, double *dA, int lda, double *dB, int ldb,
                              double *dw, double *stage_seconds, int n_stages) {
  int rc = eigenvalues_args(problem, n, il, iu, dA, lda, dB, ldb, dw); if (rc) return rc;
  rc = ensure_init(); if (rc) return rc;
  if (n == 0) return 0;
  std::lock_guard<std::mutex> lk(g_mu);
  return eigenvalues_locked(problem, n, il, iu, dA, lda, dB, ldb, dw, stage_seconds, n_stages);
}

}  // extern "C"

namespace ek {
namespace api {
int solve_device_locked(const PathCall &call) { return Path(call).run(); }

int solve_args(int problem, int n, int n_vec, const void *A, int lda, const void *B, int ldb, const void *w, const void *Z) {
  if (problem != 0 && problem != 1) return -1;
  if (n < 0) return -2;
  if (n_vec < 0 || n_vec > n) return -3;
  if (n > 0 && !A) return -4;
  if (lda < (n > 1 ? n : 1)) return -5;
  if (problem == 1 && n > 0 && !B) return -6;
  if (problem == 1 && ldb < (n > 1 ? n : 1)) return -7;
  if (n > 0 && !w) return -8;
  return (n > 0 && !Z) ? -9 : 0;
}

int eigenvalues_args(int problem, int n, int il, int iu, const void *A, int lda, const void *B, int ldb, const void *w) {
  if (problem != 0 && problem != 1) return -1;
  if (n < 0) return -2;
  if (n > 0 && (il < 1 || il > n)) return -3;
  if (n > 0 && (iu < il || iu > n)) return -4;
  if (n > 0 && !A) return -5;
  if (lda < (n > 1 ? n : 1)) return -6;
  if (problem == 1 && n > 0 && !B) return -7;
  if (problem == 1 && ldb < (n > 1 ? n : 1)) return -8;
  return (n > 0 && !w) ? -9 : 0;
}

// both entries of ek_hip_eigenvalues*, under the lock
int eigenvalues_locked(int problem, int n, int il, int iu, double *dA, int lda, double *dB, int ldb, double *dw,
                       double *stage_seconds, int n_stages) {
  Window r{0, 0, il, iu, 0.0, 0.0, 0, 0, 0};
  PathCall c = path_call(problem, n, n, dA, lda, dB, ldb, dw, nullptr, n, stage_seconds, n_stages);
  c.win = &r;
  const int rc = solve_device_locked(c);
  return rc == -4 ? -5 : rc;                // NaN / Inf in A: A is argument 5 here
}

// The argument checks of ek_hip_eigenpairs*, in argument order (LAPACK -k); zcap is checked against an index window's m
// here, against a value window's after the count.
int eigenpairs_args(int problem, int jobz, int range, int n, double vl, double vu, int il, int iu, const void *A, int lda,
                    const void *B, int ldb, const int *m, const int *ifirst, const void *w, const void *Z, int ldz,
                    int zcap) {
  if (problem != 0 && problem != 1) return -1;
  if (jobz != 0 && jobz != 1) return -2;
  if (range != 0 && range != 1) return -3;
  if (n < 0) return -4;
  if (range == 1 && vl != vl) return -5;
  if (range == 1 && !(vl < vu)) return -6;                    // (vu NaN, or an empty interval)
  if (range == 0 && n > 0 && (il < 1 || il > n)) return -7;
  if (range == 0 && n > 0 && (iu < il || iu > n)) return -8;
  if (n > 0 && !A) return -9;
  if (lda < (n > 1 ? n : 1)) return -10;
  if (problem == 1 && n > 0 && !B) return -11;
  if (problem == 1 && ldb < (n > 1 ? n : 1)) return -12;
  if (!m) return -13;
  if (!ifirst) return -14;
  if (n > 0 && !w) return -15;
  if (jobz == 1 && n > 0 && !Z) return -16;
  if (jobz == 1 && ldz < (n > 1 ? n : 1)) return -17;
  if (jobz == 1 && zcap < 0) return -18;
  return 0;
}

// both entries, under the lock: m, ifirst are set on success and on a value window too wide for zcap (-18)
int eigenpairs_locked(int problem, int jobz, int range, int n, double vl, double vu, int il, int iu, double *dA, int lda,
                      double *dB, int ldb, int *m, int *ifirst, double *dw, double *dZ, int ldz, int zcap,
                      double *stage_seconds, int n_stages, int itype) {
  Window win{jobz, range, il, iu, vl, vu, zcap, 0, 0};
  // plans: values only -> the eigenvalues-only plan; an index window -> the *_select arm's for n_vec = m; a value window
  // -> the full plan (its m is not known yet)
  const int n_vec = (jobz == 1 && range == 0) ? iu - il + 1 : n;
  PathCall c = path_call(problem, n, n_vec, dA, lda, dB, ldb, dw, dZ, ldz, stage_seconds, n_stages);
  c.win = &win; c.itype = itype;
  int info = solve_device_locked(c);
  if (info == -4) info = -9;                 // NaN / Inf in A: A is argument 9 here
  if (info == kWindowTooSmall) info = -18;
  if (info == 0 || info == -18) { *m = win.m; *ifirst = win.first + 1; }
  return info;
}
}  // namespace api
}  // namespace ek

namespace {
// the device entries of ek_hip_eigenpairs* (itype 1) and ek_hip_sygvx* (problem 1), after their own checks
int eigenpairs_device(int problem, int itype, int jobz, int range, int n, double vl, double vu, int il, int iu,
                      double *dA, int lda, double *dB, int ldb, int *m, int *ifirst, double *dw, double *dZ,
                      int ldz, int zcap, double *stage_seconds, int n_stages) {
  int rc = eigenpairs_args(problem, jobz, range, n, vl, vu, il, iu, dA, lda, dB, ldb, m, ifirst, dw, dZ, ldz, zcap);
  if (rc) return rc;
  *m = 0; *ifirst = range == 0 ? il : 1;
  if (jobz == 1 && range == 0 && n > 0 && iu - il + 1 > zcap) { *m = iu - il + 1; return -18; }
  rc = ensure_init(); if (rc) return rc;
  if (n == 0) return 0;
  std::lock_guard<std::mutex> lk(g_mu);
  return eigenpairs_locked(problem, jobz, range, n, vl, vu, il, iu, dA, lda, dB, ldb, m, ifirst, dw, dZ, ldz, zcap,
                           stage_seconds, n_stages, itype);
}
}  // namespace

extern "C" {

int ek_hip_eigenpairs_device(int problem, int jobz, int range, int n, double vl, double vu, int il, int iu,
                             double *dA, int lda, double *dB, int ldb, int *m, int *ifirst, double *dw, double *dZ,
                             int ldz, int zcap, double *stage_seconds, int n_stages) {
  return eigenpairs_device(problem, 1, jobz, range, n, vl, vu, il, iu, dA, lda, dB, ldb, m, ifirst, dw, dZ, ldz, zcap,
                           stage_seconds, n_stages);
}

// DSYGVX's three problem types on the window path: argument 1 is itype, the rest are ek_hip_eigenpairs*'s with B
int ek_hip_sygvx_device(int itype, int jobz, int range, int n, double vl, double vu, int il, int iu, double *dA, int lda,
                        double *dB, int ldb, int *m, int *ifirst, double *dw, double *dZ, int ldz, int zcap,
                        double *stage_seconds, int n_stages) {
  if (itype < 1 || itype > 3) return -1;
  return eigenpairs_device(1, itype, jobz, range, n, vl, vu, il, iu, dA, lda, dB, ldb, m, ifirst, dw, dZ, ldz, zcap,
                           stage_seconds, n_stages);
}

// Pure host arithmetic: the workspace of ek_hip_sygvx* -- type 1's window plan, whatever the type
unsigned long long ek_hip_debug_sygvx_workspace_bytes(int itype, int n, int jobz, int range, int m) {
  if (itype < 1 || itype > 3) return 0;
  return ek_hip_debug_window_workspace_bytes(1, n, jobz, range, m);
}

// Pure host arithmetic: the workspace of a window call (ek_hip_eigenpairs*) with m pairs (range 1: any m)
unsigned long long ek_hip_debug_window_workspace_bytes(int problem, int n, int jobz, int range, int m) {
  if (n < 1 || (problem != 0 && problem != 1) || (jobz != 0 && jobz != 1) || (range != 0 && range != 1)) return 0;
  if (m < 0 || m > n) return 0;
  if (jobz == 0) return plan_path(problem, n, n, n, 0, 0, /*values_only=*/true).total;
  if (range == 0) return plan_path(problem, n, m, m, 0).total;
  return plan_path(problem, n, n, n, 0, 0, false, /*value_window=*/true).total;
}

// Pure host arithmetic: the workspace of an eigenvalues-only call (ek_hip_eigenvalues*)
unsigned long long ek_hip_debug_values_workspace_bytes(int problem, int n) {
  if (n < 1 || (problem != 0 && problem != 1)) return 0;
  return plan_path(problem, n, n, n, 0, 0, /*values_only=*/true).total;
}

int ek_hip_debug_set_stebz(int lanes) { return stebz_set_lanes(lanes); }

// Pure host arithmetic (no GPU needed): bytes of workspace one whole-path call asks for -- on one GPU (nranks <= 1: all
// n_vec eigenvector columns) or as rank 0 of a 1 x nranks team with a communicator attached (its share of the columns,
// 64-wide blocks dealt round robin).  parts (optional, 6 entries): matrix bytes (one padded n x n array), persistent
// operators (L, the first stage's reflectors), eigenvector columns, X0, X1, the rest.
unsigned long long ek_hip_debug_workspace_bytes(int problem, int n, int n_vec, int nranks, unsigned long long *parts) {
  if (n < 1 || n_vec < 0 || n_vec > n) return 0;
  const int P = nranks > 1 ? nranks : 1;
  const int nc_loc = P > 1 ? numroc0(n_vec, 64, 0, P) : n_vec;
  const PathPlan p = plan_path(problem, n, n_vec, nc_loc, P > 1 ? P : 0);
  if (parts) {
    parts[0] = p.mat; parts[1] = 2 * p.mat; parts[2] = p.zmat; parts[3] = p.x0; parts[4] = p.x1;
    parts[5] = p.total - (2 * p.mat + p.zmat + p.x0 + p.x1);
  }
  return p.total;
}

// Rehearsal of the divide & conquer's team form on one GPU: while nranks >= 2, a grid cell solved WITHOUT a communicator
// (ek_hip_solve_device_grid, replicated inputs) forms the sharded heights as a team of nranks would, rank after rank (no
// exchange).  levels: heights below the top merge that are sharded (-1: the library's default for the order); profile != 0:
// HIP events around the call and every rank's sections, read by ek_hip_debug_stedc_team_get ([0] the D&C, [1] all ranks'
// sections, [2] the longest rank's per height: a rank of a real team computes for [0] - [1] + [2] seconds).
int ek_hip_debug_stedc_team(int nranks, int levels, int profile) {
  if (nranks < 0 || nranks > kMaxTeam) return -1;
  std::lock_guard<std::mutex> lk(g_mu);
  g_debug_dc_team = nranks;
  stedc_team_set_levels(levels);
  stedc_team_profile(profile != 0);
  return 0;
}
int ek_hip_debug_stedc_team_get(double *seconds) {
  if (!seconds) return -1;
  int rc = ensure_init(); if (rc) return rc;
  std::lock_guard<std::mutex> lk(g_mu);
  EK_HIP_CHECK(hipStreamSynchronize(g_ctx.stream));
  stedc_team_profile_collect(seconds);
  return 0;
}

// Test aid: the whole-path call treats its next `times` bulge chasings as if they had abandoned a bounded wait (the
// repetition from the saved band with the older kernel, and -992 after the third failure, are otherwise unreachable).
int ek_hip_debug_fail_next_chase(int times) {
  std::lock_guard<std::mutex> lk(g_mu);
  g_debug_fail_chase = times > 0 ? times : 0;
  return 0;
}

int ek_hip_solve_device_grid(int problem, int n, int n_vec, double *dA, int lda, double *dB, int ldb,
                             double *dw, double *dZ_loc, int ldz_loc, int nb, int nprow, int npcol,
                             int myrow, int mycol, double *stage_seconds, int n_stages) {
  int rc = solve_args(problem, n, n_vec, dA, lda, dB, ldb, dw, dZ_loc); if (rc) return rc;
  if (nb < 1) return -11;
  if (nprow < 1) return -12;
  if (npcol < 1) return -13;
  if (myrow < 0 || myrow >= nprow) return -14;
  if (mycol < 0 || mycol >= npcol) return -15;
  const int nr_loc = numroc0(n, nb, myrow, nprow);
  if (ldz_loc < (nr_loc > 1 ? nr_loc : 1)) return -10;
  rc = ensure_init(); if (rc) return rc;
  if (n == 0) return 0;
  std::lock_guard<std::mutex> lk(g_mu);
  const GridCell cell{nb, nprow, npcol, myrow, mycol};
  PathCall c = path_call(problem, n, n_vec, dA, lda, dB, ldb, dw, dZ_loc, ldz_loc, stage_seconds, n_stages);
  c.cell = &cell;
  return solve_device_locked(c);
}

}  // extern "C"
