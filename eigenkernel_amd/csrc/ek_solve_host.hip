// ek_solve_host.hip -- the whole path on host arrays: the C entries ek_hip_solve (1 x 1 through the staging pipeline or
// plain; grids through a communicator or the host's allgatherv hook), ek_hip_solve_replicated, ek_hip_solve_sparse
// (the same on triplets: the images are densified in HBM, ek_sparse.hip), ek_hip_eigenvalues,
// ek_hip_eigenpairs and ek_hip_sygvx of include/ek_hip.h.  Each stages device images of its arrays (HostImages) around
// one call of the Path (ek_solve.hip: solve_device_locked).
#include "ek_api_internal.h"
#include "ek_sparse_csr.h"

#include <condition_variable>
#include <sched.h>
#include <deque>
#include <memory>
#include <new>
#include <thread>

using namespace ek;
using namespace ek::api;

namespace {

// local piece (nr x nc, lld) <-> its place in the full matrix; blocks of nb rows are contiguous
template <typename F>
void for_each_local_block(int m, int n, int nb, int pr, int nprow, int pc, int npcol, F f) {
  const int nr = numroc0(m, nb, pr, nprow), nc = numroc0(n, nb, pc, npcol);
  for (int lc = 0; lc < nc; ++lc) {
    const size_t gc = (size_t)((lc / nb) * npcol + pc) * nb + lc % nb;
    for (int lr0 = 0; lr0 < nr; lr0 += nb) {
      const size_t gr0 = (size_t)((lr0 / nb) * nprow + pr) * nb;
      f(lr0, lc, gr0, gc, (nr - lr0 < nb) ? nr - lr0 : nb, nr);
    }
  }
}

// M_full (m x n, ldf) <- all ranks' pieces of a block-cyclic matrix, through the host hook.
int gather_full(int m, int n, const double *M_loc, const int *desc, const GridCell &g, double *M_full,
                int ldf) {
  if (!g_allgatherv) return -998;
  const int nb = desc[4], P = g.nprow * g.npcol;
  std::vector<long long> counts(P), displs(P);
  long long tot = 0;
  for (int r = 0; r < P; ++r) {            // ranks in row-major grid order (processes.f90:23, 'R')
    counts[r] = (long long)numroc0(m, nb, r / g.npcol, g.nprow) * numroc0(n, nb, r % g.npcol, g.npcol);
    displs[r] = tot; tot += counts[r];
  }
  const int me = g.myrow * g.npcol + g.mycol;
  double *send = (double *)malloc((size_t)(counts[me] > 0 ? counts[me] : 1) * 8);
  double *recv = (double *)malloc((size_t)(tot > 0 ? tot : 1) * 8);
  if (!send || !recv) { free(send); free(recv); return hip_rc(hipErrorOutOfMemory); }
  const int lld = desc[8];
  for_each_local_block(m, n, nb, g.myrow, g.nprow, g.mycol, g.npcol,
                       [&](int lr0, int lc, size_t, size_t, int len, int nr) {
                         memcpy(send + (size_t)lr0 + (size_t)lc * nr, M_loc + (size_t)lr0 + (size_t)lc * lld,
                                (size_t)len * 8);
                       });
  const int rc = g_allgatherv(send, counts[me], recv, counts.data(), displs.data(), g_allgatherv_user);
  if (rc == 0) {
    for (int r = 0; r < P; ++r) {
      const double *piece = recv + displs[r];
      for_each_local_block(m, n, nb, r / g.npcol, g.nprow, r % g.npcol, g.npcol,
                           [&](int lr0, int lc, size_t gr0, size_t gc, int len, int nr) {
                             memcpy(M_full + gr0 + gc * (size_t)ldf, piece + (size_t)lr0 + (size_t)lc * nr,
                                    (size_t)len * 8);
                           });
    }
  }
  free(send); free(recv);
  return rc == 0 ? 0 : -999;
}

// M_loc <- this cell's piece of M_full
void extract_local(int m, int n, const double *M_full, int ldf, const int *desc, const GridCell &g,
                   double *M_loc) {
  const int lld = desc[8];
  for_each_local_block(m, n, desc[4], g.myrow, g.nprow, g.mycol, g.npcol,
                       [&](int lr0, int lc, size_t gr0, size_t gc, int len, int) {
                         memcpy(M_loc + (size_t)lr0 + (size_t)lc * lld, M_full + gr0 + gc * (size_t)ldf,
                                (size_t)len * 8);
                       });
}
}  // namespace

namespace ek {
namespace api {
namespace {
// Staging pipeline of ek_hip_solve on a 1 x 1 grid (host arrays in, host arrays out: solver_main.f90:64-65).  The
// copies run on worker threads with their own non-blocking streams while the main thread issues the stages:
//   in : B, then A (B is needed first: the Cholesky factorisation runs while A is still on its way);
//   out: L as soon as it is final (it leaves during the reduction), the reflectors / band of A after the
//        tridiagonalisation, Z in column slabs as the last stage finishes them, w last.
// The caller's arrays are pageable and handed to the runtime as they are: on every box met since round 4 it moves them at
// link rate (57 GB/s in).  Round 4's ring of pinned bounce buffers was measured slower under every runtime met (37 - 51
// GB/s in, ~1 GB/s per worker out beside running kernels; profiles/r04_host_path.txt) and is gone (round 5).  The number
// of workers on the way in follows the cores the process may run on, the way out has two (HostPipe::start says why).
// what the last staging pipeline did (ek_hip_debug_last_pipe_stats): [0] bytes in, [1] span of the input transfers (s),
// [2] busy seconds of the input workers, [3..5] the same on the way out, [6] seconds the main thread waited for inputs,
// [7] for the drain at the end, [8] workers per direction, [9] 0 (round 4: directions through a pinned ring), [10] seconds from the
// start of the pipeline to its end, [11] seconds before the first input job started
double g_pipe_stats[12] = {0};
// the pipeline's streams live as long as the process (creating its 14 streams took a call ~25 ms)
struct PipeStreams {
  hipStream_t cs[2 * 8] = {};
  int made = 0;
  int ensure(int n) {
    for (; made < n; ++made) EK_HIP_CHECK(hipStreamCreateWithFlags(&cs[made], hipStreamNonBlocking));
    return 0;
  }
  void release() {          // ek_hip_finalize: they come back with the next call that needs them
    for (int i = 0; i < made; ++i) { (void)hipStreamDestroy(cs[i]); cs[i] = nullptr; }
    made = 0;
  }
};
PipeStreams g_pipe_streams;

int usable_cores() {
  cpu_set_t set;
  CPU_ZERO(&set);
  if (sched_getaffinity(0, sizeof(set), &set) == 0) { const int c = CPU_COUNT(&set); if (c > 0) return c; }
  const unsigned h = std::thread::hardware_concurrency();
  return h > 0 ? (int)h : 1;
}
}  // namespace

struct HostPipe {
  // tri: a square diagonal block on the way out of which only the lower triangle may reach the caller's array (m == n)
  struct Job { double *dev; int ldd; double *host; int ldh; int m, n; hipEvent_t after; int tag; bool to_host; bool tri = false; };
  static constexpr int kMaxThreads = 8;
  static constexpr int kTri = 512;           // columns of a diagonal block on the way out (2 MiB of scratch per worker)
  int kThreads = 2;                          // per direction (by the cores the process has)
  int kOutThreads = 2;                       // of them on the way out (see start())
  bool lower_only = true;                    // EK_HIP_PIPE_LOWER=0: whole matrices both ways, as round 3
  std::mutex mu;
  std::condition_variable cv;
  std::deque<Job> in_q, out_q;
  int pending_in[2] = {0, 0};                // tag 0 = B, 1 = A: pieces not yet in HBM
  int pending_out = 0;
  bool closing = false;
  int err = 0;
  std::vector<std::thread> th;
  hipStream_t cs[2 * kMaxThreads] = {};
  int device = 0;
  int z_slab = 2048;
  // EK_HIP_PIPE_TRACE=1: what every copy job and every wait of the main thread took (stderr, at the end of the call)
  bool trace = false;
  std::chrono::steady_clock::time_point t_origin;
  struct TraceRec { double t0, t1; double bytes; int kind; };      // kind 0 = in, 1 = out, 2 = wait_in, 3 = finish
  std::vector<TraceRec> trace_log;
  double now() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_origin).count(); }
  double busy[2], bytes[2], first[2], last[2];             // per direction, summed by collect_stats()
  void collect_stats() {
    double win = 0, wdrain = 0;
    for (int k = 0; k < 2; ++k) { busy[k] = bytes[k] = last[k] = 0; first[k] = 1e30; }
    for (const auto &r : trace_log) {
      if (r.kind < 2) {
        busy[r.kind] += r.t1 - r.t0; bytes[r.kind] += r.bytes;
        if (r.t0 < first[r.kind]) first[r.kind] = r.t0;
        if (r.t1 > last[r.kind]) last[r.kind] = r.t1;
      } else if (r.kind == 2) win += r.t1 - r.t0;
      else wdrain += r.t1 - r.t0;
    }
    for (int k = 0; k < 2; ++k) {
      g_pipe_stats[3 * k] = bytes[k]; g_pipe_stats[3 * k + 1] = bytes[k] > 0 ? last[k] - first[k] : 0.0; g_pipe_stats[3 * k + 2] = busy[k];
    }
    g_pipe_stats[6] = win; g_pipe_stats[7] = wdrain; g_pipe_stats[8] = 100.0 * kThreads + kOutThreads; g_pipe_stats[9] = 0;
    g_pipe_stats[10] = now(); g_pipe_stats[11] = bytes[0] > 0 ? first[0] : 0.0;
  }
  void report() {
    collect_stats();
    if (!trace) return;
    for (const auto &r : trace_log)
      if (r.kind >= 2)
        fprintf(stderr, "[pipe] main thread waited %.4f s (%s) at t = %.4f\n", r.t1 - r.t0, r.kind == 2 ? "input" : "drain", r.t0);
    if (switch_int(kSwPipeTrace) >= 2)       // every job
      for (const auto &r : trace_log)
        if (r.kind < 2) fprintf(stderr, "[pipe] job %s %8.1f MB  t = %.4f .. %.4f  (%.1f GB/s)\n", r.kind ? "out" : "in ", r.bytes / 1e6, r.t0, r.t1,
                                r.bytes / 1e9 / (r.t1 - r.t0 > 1e-9 ? r.t1 - r.t0 : 1e-9));
    for (int k = 0; k < 2; ++k)
      if (bytes[k] > 0)
        fprintf(stderr, "[pipe] %s: %.2f GB between t = %.4f and %.4f s (%.1f GB/s over the span), %d threads busy %.3f s in all (%.1f GB/s per busy thread), %s\n",
                k ? "out" : "in", bytes[k] / 1e9, first[k], last[k], bytes[k] / 1e9 / (last[k] - first[k]), k ? kOutThreads : kThreads, busy[k],
                bytes[k] / 1e9 / busy[k], "pageable");
  }

  int start(int dev) {
    device = dev;
    t_origin = std::chrono::steady_clock::now();
    trace = switch_once(kSwPipeTrace) != 0;
    lower_only = switch_int(kSwPipeLower) != 0;
    const int cores = usable_cores();
    kThreads = cores >= 16 ? 6 : cores >= 8 ? 4 : 2;      // (both directions are rarely busy at once)
    { const int rc = g_pipe_streams.ensure(2 * kThreads); if (rc) return rc; }
    for (int i = 0; i < 2 * kThreads; ++i) cs[i] = g_pipe_streams.cs[i];
    // The way out hands pageable memory to the runtime: two threads saturate the link (30 GB/s
    // each), and MORE than two collapse under the HIP runtime PyTorch bundles (2.10: 1.7 GB/s per thread with three, 0.9
    // with six, beside running kernels; the system's runtime does 10 - 20 with any number) -- which is the runtime that
    // serves a process that imported torch first.  EK_HIP_PIPE_THREADS_OUT overrides.
    const int env_out = switch_int(kSwPipeThreadsOut);
    kOutThreads = kThreads < 2 ? kThreads : 2;
    if (env_out >= 1 && env_out <= kThreads) kOutThreads = env_out;
    for (int i = 0; i < kThreads + kOutThreads; ++i) th.emplace_back([this, i]() { run(i < kThreads, cs[i]); });
    return 0;
  }
  void run(bool input, hipStream_t c) {
    (void)hipSetDevice(device);
    std::deque<Job> &q = input ? in_q : out_q;
    while (true) {
      Job j;
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&]() { return !q.empty() || closing; });
        if (q.empty()) return;
        j = q.front(); q.pop_front();
      }
      hipError_t e = hipSuccess;
      if (j.after) e = hipEventSynchronize(j.after);
      const double tj0 = now();
      if (e == hipSuccess && j.m > 0 && j.n > 0 && j.tri) {
        // the block crosses into a scratch of this thread; the caller's array receives the entries on and below the
        // diagonal only (its strictly upper triangle is neither read nor written: PDPOTRF / PDSYTRD with uplo = 'L')
        std::vector<double> tmp((size_t)j.n * j.n);
        e = hipMemcpy2DAsync(tmp.data(), (size_t)j.n * 8, j.dev, (size_t)j.ldd * 8, (size_t)j.n * 8, j.n, hipMemcpyDeviceToHost, c);
        if (e == hipSuccess) e = hipStreamSynchronize(c);
        if (e == hipSuccess)
          for (int cc = 0; cc < j.n; ++cc)
            memcpy(j.host + (size_t)cc * j.ldh + cc, tmp.data() + (size_t)cc * j.n + cc, (size_t)(j.n - cc) * 8);
      } else if (e == hipSuccess && j.m > 0 && j.n > 0) {
        if (j.to_host)
          e = hipMemcpy2DAsync(j.host, (size_t)j.ldh * 8, j.dev, (size_t)j.ldd * 8, (size_t)j.m * 8, j.n, hipMemcpyDeviceToHost, c);
        else
          e = hipMemcpy2DAsync(j.dev, (size_t)j.ldd * 8, j.host, (size_t)j.ldh * 8, (size_t)j.m * 8, j.n, hipMemcpyHostToDevice, c);
        if (e == hipSuccess) e = hipStreamSynchronize(c);
      }
      {
        std::lock_guard<std::mutex> lk(mu);
        if (e != hipSuccess && !err) err = hip_rc(e);
        trace_log.push_back(TraceRec{tj0, now(), (double)j.m * j.n * 8.0, input ? 0 : 1});
        if (input) --pending_in[j.tag]; else --pending_out;
      }
      cv.notify_all();
    }
  }
  // host array (m x n, ldh) <-> device image (ldd), cut into column pieces for the threads (in column order: the
  // first columns of a matrix arrive first)
  // lower: a square matrix of which only the lower triangle is referenced (A, B on the way in; what the call leaves in A,
  // L on the way out: uplo = 'L' throughout the reference, generalized_to_standard.f90:24,37, solver_scalapack_all.f90:59):
  // a piece then carries the rows from its first column down -- half the bytes, the upper triangle of the destination is
  // not touched (as PDPOTRF / PDSYTRD leave it) -- and the pieces are cut to equal areas
  void push(bool to_host, double *dev, int ldd, double *host, int ldh, int m, int n, hipEvent_t after, int tag,
            bool lower = false) {
    const int pieces = (n >= 256) ? 4 * kThreads : 1;
    lower = lower && lower_only && m == n;
    {
      std::lock_guard<std::mutex> lk(mu);
      int c0 = 0;
      for (int p = 0; p < pieces; ++p) {
        int c1 = (int)((long long)n * (p + 1) / pieces);
        if (lower) c1 = (p + 1 == pieces) ? n : (int)((double)n * (1.0 - sqrt(1.0 - (double)(p + 1) / pieces)));
        if (c1 < c0) c1 = c0;
        if (lower && to_host) {
          // on the way out a piece is cut into chunks of at most kTri columns: the rows below a chunk's diagonal block as
          // one 2-D copy, the diagonal block as a `tri` job -- nothing above the diagonal of the caller's array is written
          for (int a = c0; a < c1; a += kTri) {
            const int b = (c1 - a < kTri) ? c1 : a + kTri;
            Job t{dev + (size_t)a * ldd + a, ldd, host + (size_t)a * ldh + a, ldh, b - a, b - a, after, tag, true, true};
            out_q.push_back(t); ++pending_out;
            if (b < m) {
              Job r{dev + (size_t)a * ldd + b, ldd, host + (size_t)a * ldh + b, ldh, m - b, b - a, after, tag, true};
              out_q.push_back(r); ++pending_out;
            }
          }
          c0 = c1;
          continue;
        }
        const int r0 = lower ? (c0 & ~1) : 0;                          // (even: 16-byte aligned rows)
        Job j{dev + (size_t)c0 * ldd + r0, ldd, host + (size_t)c0 * ldh + r0, ldh, m - r0, c1 - c0, after, tag, to_host};
        if (to_host) { out_q.push_back(j); ++pending_out; } else { in_q.push_back(j); ++pending_in[tag]; }
        c0 = c1;
      }
    }
    cv.notify_all();
  }
  int wait_in(int tag) {
    const double t0 = now();
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&]() { return pending_in[tag] == 0; });
    trace_log.push_back(TraceRec{t0, now(), 0.0, 2});
    return err;
  }
  int finish() {                              // all copies done; threads joined; streams released
    {
      const double t0 = now();
      std::unique_lock<std::mutex> lk(mu);
      cv.wait(lk, [&]() { return pending_out == 0 && pending_in[0] == 0 && pending_in[1] == 0; });
      closing = true;
      trace_log.push_back(TraceRec{t0, now(), 0.0, 3});
    }
    cv.notify_all();
    for (auto &t : th) t.join();
    th.clear();
    for (auto &c : cs) c = nullptr;              // (the streams belong to the process-wide pool)
    for (auto &e : evs) (void)hipEventDestroy(e);
    evs.clear();
    report();
    return err;
  }
  ~HostPipe() { if (!th.empty()) (void)finish(); }
  // an event recorded on stream s now (the device image is final there)
  std::vector<hipEvent_t> evs;
  hipEvent_t mark(hipStream_t s) {
    hipEvent_t e = nullptr;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
    (void)hipEventRecord(e, s);
    evs.push_back(e);
    return e;
  }
  // what the solve hands over: host destinations of the in-place results
  double *hA = nullptr, *hB = nullptr, *hZ = nullptr; int ldha = 0, ldhb = 0, ldhz = 0;
};

int pipe_wait_in(HostPipe *p, int tag) { return p->wait_in(tag); }
int pipe_z_slab(const HostPipe *p) { return p->z_slab; }
void pipe_out(HostPipe *p, hipStream_t s, char which, double *dev, int ldd, int n, int c0, int nc) {
  if (which == 'Z')
    p->push(true, dev + (size_t)c0 * ldd, ldd, p->hZ + (size_t)c0 * p->ldhz, p->ldhz, n, nc, p->mark(s), 0);
  else
    p->push(true, dev, ldd, which == 'A' ? p->hA : p->hB, which == 'A' ? p->ldha : p->ldhb, n, n, p->mark(s), 0,
            /*lower=*/true);
}
void release_pipe_streams() { g_pipe_streams.release(); }
}  // namespace api
}  // namespace ek

namespace {
using Clock = std::chrono::steady_clock;
double seconds(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double>(b - a).count(); }

// Device images of one call on host arrays, and the call's staging: alloc(), in() (the matrices cross, the stream is
// waited for), the path, then -- while back(info) says that results travel (info > -1000: also with info > 0, so that
// the host can inspect them, as with ScaLAPACK) -- out() / out_w() per result, and finish(), which waits, lets a
// failed copy stand for info == 0 and adds both ways' wall time to EK_STAGE_COPY.
struct HostImages {
  hipStream_t s = g_ctx.stream;
  DevMem mem;                      // (released on every way out; nothing in it when the library keeps the images)
  double *uA = nullptr, *uB = nullptr, *uZ = nullptr, *uw = nullptr;
  Clock::time_point t0 = Clock::now(), t1 = t0, t2 = t0;
  int rc = 0;                      // the first copy back that failed
  // exact n x n images of A (and B), w_doubles of w, z_doubles of Z (0: none).  kept: one allocation that the library
  // keeps between calls like its workspace (6 GiB of hipMalloc + hipFree per call were 0.05 s of a 1.0 s call at
  // N = 16384) and releases in ek_hip_finalize
  int alloc(int problem, int n, size_t w_doubles, size_t z_doubles, bool kept = false) {
    const size_t nn = (size_t)n * n * 8;
    if (kept) {
      const size_t need = (problem == 1 ? 2 : 1) * al(nn) + al(z_doubles * 8) + al(w_doubles * 8);
      EK_TRY(user_images(need, (void **)&uA));
      uZ = (double *)((char *)uA + al(nn));
      uw = (double *)((char *)uZ + al(z_doubles * 8));
      if (problem == 1) uB = (double *)((char *)uw + al(w_doubles * 8));
      return 0;
    }
    EK_TRY(mem.alloc(&uA, nn));
    if (z_doubles) EK_TRY(mem.alloc(&uZ, z_doubles * 8));
    EK_TRY(mem.alloc(&uw, w_doubles * 8));
    if (problem == 1) EK_TRY(mem.alloc(&uB, nn));
    return 0;
  }
  int in(int problem, int n, const double *A, int lda, const double *B, int ldb) {
    int r = h2d_matrix(n, n, A, lda, uA, n, s);
    if (!r && problem == 1) r = h2d_matrix(n, n, B, ldb, uB, n, s);
    if (!r) r = hip_rc(hipStreamSynchronize(s));
    t1 = Clock::now();
    return r;
  }
  PathCall call(int problem, int n, int n_vec, int ldz, double *stage_seconds, int n_stages) const {
    return path_call(problem, n, n_vec, uA, n, uB, n, uw, uZ, ldz, stage_seconds, n_stages);
  }
  bool back(int info) { t2 = Clock::now(); return info > -1000; }
  void out(int m, int n, const double *d, int ldd, double *h, int ldh) { if (!rc) rc = d2h_matrix(m, n, d, ldd, h, ldh, s); }
  void out_w(double *w, size_t count) { if (!rc) rc = hip_rc(hipMemcpyAsync(w, uw, count * 8, hipMemcpyDeviceToHost, s)); }
  int wait(int info) {
    if (!rc) rc = hip_rc(hipStreamSynchronize(s));
    return (rc && info == 0) ? rc : info;
  }
  // gather_seconds: the part of the way in that belongs to EK_STAGE_GATHER (a team's all-gathers)
  int finish(int info, double *stage_seconds, int n_stages, double gather_seconds = 0.0) {
    info = wait(info);
    const double both = seconds(t0, t1) - gather_seconds + seconds(t2, Clock::now());
    if (stage_seconds && n_stages > EK_STAGE_COPY) stage_seconds[EK_STAGE_COPY] += both;
    if (stage_seconds && n_stages > EK_STAGE_GATHER) stage_seconds[EK_STAGE_GATHER] += gather_seconds;
    return info;
  }
};

// Replicated host inputs (full A, B on every rank) -> this cell's block-cyclic piece of Z.
int replicated_host_locked(int problem, int n, int n_vec, double *A, int lda, double *B, int ldb, double *w,
                           double *Z_loc, int lldz, const GridCell &cell, double *stage_seconds,
                           int n_stages) {
  const int nr_loc = numroc0(n, cell.nb, cell.myrow, cell.nprow);
  const int nc_loc = numroc0(n_vec, cell.nb, cell.mycol, cell.npcol);
  const int ldzl = nr_loc > 1 ? nr_loc : 1;
  HostImages im;
  EK_TRY(im.alloc(problem, n, n, (size_t)ldzl * (nc_loc > 0 ? nc_loc : 1)));
  int info = im.in(problem, n, A, lda, B, ldb);
  PathCall c = im.call(problem, n, n_vec, ldzl, stage_seconds, n_stages);
  c.cell = &cell;
  if (!info) info = solve_device_locked(c);
  if (im.back(info)) {
    if (nr_loc > 0 && nc_loc > 0) im.out(nr_loc, nc_loc, im.uZ, ldzl, Z_loc, lldz);
    im.out(n, n, im.uA, n, A, lda);
    if (problem == 1) im.out(n, n, im.uB, n, B, ldb);
    im.out_w(w, n);
  }
  return im.finish(info, stage_seconds, n_stages);
}

// Replicated TRIPLETS (the reference's own matrix arguments) -> this cell's block-cyclic piece of Z: the images of
// replicated_host_locked, built in HBM from the CSRs of the mirrored matrices instead of crossing PCIe, then the same
// call of the Path.  A and B are not returned (the reference deallocates them unread).  The CSR build, the upload and
// the densification are the way in: EK_STAGE_COPY.
int sparse_host_locked(int problem, int n, int n_vec, long long nnzA, const int *sufA, const double *valA,
                       long long nnzB, const int *sufB, const double *valB, double *w, double *Z_loc, int lldz,
                       const GridCell &cell, double *stage_seconds, int n_stages) {
  const int nr_loc = numroc0(n, cell.nb, cell.myrow, cell.nprow);
  const int nc_loc = numroc0(n_vec, cell.nb, cell.mycol, cell.npcol);
  const int ldzl = nr_loc > 1 ? nr_loc : 1;
  HostImages im;
  const sparse::Csr *hA = nullptr, *hB = nullptr;
  EK_TRY(csr_build(n, nnzA, sufA, valA, &hA, problem == 1, nnzB, sufB, valB, &hB));
  // the images and the CSRs in the one allocation the library keeps between calls (HostImages::alloc says why)
  const size_t nn = al((size_t)n * n * 8), zb = al((size_t)ldzl * (nc_loc > 0 ? nc_loc : 1) * 8), wb = al((size_t)n * 8);
  const size_t ca = csr_device_bytes(n, nnzA), cb = problem == 1 ? csr_device_bytes(n, nnzB) : 0;
  char *base = nullptr;
  EK_TRY(user_images((problem == 1 ? 2 : 1) * nn + zb + wb + ca + cb, (void **)&base));
  im.uA = (double *)base;
  im.uZ = (double *)(base + nn);
  im.uw = (double *)(base + nn + zb);
  char *cA = base + nn + zb + wb, *cB = cA + ca;
  if (problem == 1) im.uB = (double *)(cB + cb);
  DevCsr dA{}, dB{};
  int info = csr_upload(im.s, *hA, nnzA, cA, &dA);
  if (!info && problem == 1) info = csr_upload(im.s, *hB, nnzB, cB, &dB);
  if (!info) {
    sparse_densify(im.s, n, dA, im.uA, n);
    if (problem == 1) sparse_densify(im.s, n, dB, im.uB, n);
    info = hip_rc(hipGetLastError());
  }
  if (!info) info = hip_rc(hipStreamSynchronize(im.s));
  im.t1 = Clock::now();
  PathCall c = im.call(problem, n, n_vec, ldzl, stage_seconds, n_stages);
  c.cell = &cell;
  if (!info) info = solve_device_locked(c);
  if (info == -4) info = -6;                 // NaN / Inf in A: the value argument of this prototype
  if (im.back(info)) {
    if (nr_loc > 0 && nc_loc > 0) im.out(nr_loc, nc_loc, im.uZ, ldzl, Z_loc, lldz);
    im.out_w(w, n);
  }
  return im.finish(info, stage_seconds, n_stages);
}

int eigenpairs_host(int problem, int itype, int jobz, int range, int n, double vl, double vu, int il, int iu,
                    const double *A, int lda, const double *B, int ldb, int *m, int *ifirst, double *w, double *Z,
                    int ldz, int zcap, double *stage_seconds, int n_stages) {
  int rc = eigenpairs_args(problem, jobz, range, n, vl, vu, il, iu, A, lda, B, ldb, m, ifirst, w, Z, ldz, zcap);
  if (rc) return rc;
  *m = 0; *ifirst = range == 0 ? il : 1;
  if (jobz == 1 && range == 0 && n > 0 && iu - il + 1 > zcap) { *m = iu - il + 1; return -18; }
  rc = ensure_init(); if (rc) return rc;
  if (n == 0) return 0;
  std::lock_guard<std::mutex> lk(g_mu);
  const int mw = range == 0 ? iu - il + 1 : n;                          // eigenvalues w can receive
  const int zc = jobz == 0 ? 0 : (range == 0 ? iu - il + 1 : (zcap < n ? zcap : n));   // columns Z can receive
  // the caller's arrays are left as they are: the path works on device copies of them
  HostImages im;
  EK_TRY(im.alloc(problem, n, mw, jobz == 1 ? (size_t)n * (zc > 0 ? zc : 1) : 0));
  EK_TRY(im.in(problem, n, A, lda, B, ldb));
  int info = eigenpairs_locked(problem, jobz, range, n, vl, vu, il, iu, im.uA, n, im.uB, n, m, ifirst, im.uw, im.uZ, n, zc,
                               stage_seconds, n_stages, itype);
  if (im.back(info) && info == 0 && *m > 0) {       // (w and Z are written on success only)
    im.out_w(w, *m);
    if (jobz == 1) im.out(n, *m, im.uZ, n, Z, ldz);
  }
  return im.finish(info, stage_seconds, n_stages);
}

// distributed inputs with a communicator attached: only the local pieces cross PCIe; the full matrices are assembled in
// HBM by one all-gather per matrix (RCCL over xGMI, or the host hook of a host communicator) and the pieces of the
// reflectors / of L are cut out on the device
int solve_team_host(int problem, int n, int n_vec, double *A_loc, const int *desc_A, double *B_loc, const int *desc_B,
                    double *w, double *Z_loc, const int *desc_Z, const GridCell &cell, double *stage_seconds,
                    int n_stages) {
  const int nprow = cell.nprow, npcol = cell.npcol, myrow = cell.myrow, mycol = cell.mycol;
  if (g_comm.rank != myrow * npcol + mycol) return -994;
  const int P = nprow * npcol, me = g_comm.rank;
  const SytrdExchange x = team_exchange(0);
  const int nrz = numroc0(n, cell.nb, myrow, nprow), ncz = numroc0(n_vec, cell.nb, mycol, npcol);
  const int ldzl = nrz > 1 ? nrz : 1;
  HostImages im;
  hipStream_t s = im.s;
  double *pk = nullptr;
  int rc = im.alloc(problem, n, n, (size_t)ldzl * (ncz > 0 ? ncz : 1));
  if (!rc) rc = im.mem.alloc(&pk, (size_t)n * n * 8);
  g_comm.err = 0;
  rc = comm_agree(rc);                 // nobody enters the all-gathers below unless everybody can
  if (rc) return rc;
  auto assemble = [&](const double *M_loc, const int *desc, double *full) -> int {
    const int nb = desc[4];
    size_t offs[kMaxTeam], counts[kMaxTeam];
    size_t tot = 0;
    for (int r = 0; r < P; ++r) {
      counts[r] = (size_t)numroc0(n, nb, r / npcol, nprow) * numroc0(n, nb, r % npcol, npcol);
      offs[r] = tot; tot += counts[r];
    }
    const int nr = numroc0(n, nb, myrow, nprow), nc = numroc0(n, nb, mycol, npcol);
    if (nr > 0 && nc > 0) EK_TRY(h2d_matrix(nr, nc, M_loc, desc[8], pk + offs[me], nr, s));
    double *bufs[1] = {pk};
    x.allgatherv(s, 1, me, bufs, offs, counts, P, x.user);
    for (int r = 0; r < P; ++r)
      scatter_block_cyclic(s, numroc0(n, nb, r / npcol, nprow), numroc0(n, nb, r % npcol, npcol), pk + offs[r],
                           numroc0(n, nb, r / npcol, nprow) > 1 ? numroc0(n, nb, r / npcol, nprow) : 1, nb, nprow,
                           r / npcol, npcol, r % npcol, full, n);
    return 0;
  };
  // this cell's piece of a full matrix, by way of pk
  auto cut = [&](const double *full, const int *desc, double *M_loc) {
    const int nb = desc[4], nr = numroc0(n, nb, myrow, nprow), nc = numroc0(n, nb, mycol, npcol);
    if (nr <= 0 || nc <= 0) return;
    gather_block_cyclic(s, nr, nc, full, n, nb, nprow, myrow, npcol, mycol, pk, nr);
    im.out(nr, nc, pk, nr, M_loc, desc[8]);
  };
  const Clock::time_point tg0 = Clock::now();
  int info = assemble(A_loc, desc_A, im.uA);
  if (!info && problem == 1) info = assemble(B_loc, desc_B, im.uB);
  if (!info) info = hip_rc(hipStreamSynchronize(s));
  if (!info && g_comm.err) info = -996;
  info = comm_agree(info);             // a staging failure on one rank ends the call on all of them
  im.t1 = Clock::now();
  const double tg = seconds(tg0, im.t1);
  PathCall c = im.call(problem, n, n_vec, ldzl, stage_seconds, n_stages);
  c.cell = &cell;
  if (!info) info = solve_device_locked(c);
  if (im.back(info)) {
    if (nrz > 0 && ncz > 0) im.out(nrz, ncz, im.uZ, ldzl, Z_loc, desc_Z[8]);
    cut(im.uA, desc_A, A_loc);
    if (!im.rc) im.rc = hip_rc(hipStreamSynchronize(s));       // pk is reused
    if (problem == 1) cut(im.uB, desc_B, B_loc);
    im.out_w(w, n);
  }
  return im.finish(info, stage_seconds, n_stages, tg);
}

// distributed inputs without a communicator: assemble the full matrices on every rank through the hook, then proceed as
// in the replicated-input mode; A_loc / B_loc receive their pieces of the reflectors / of L, as every rank of the
// reference ends up with
int solve_hook_host(int problem, int n, int n_vec, double *A_loc, const int *desc_A, double *B_loc, const int *desc_B,
                    double *w, double *Z_loc, const int *desc_Z, const GridCell &cell, double *stage_seconds,
                    int n_stages) {
  double *Af = (double *)malloc((size_t)n * n * 8);
  double *Bf = problem == 1 ? (double *)malloc((size_t)n * n * 8) : nullptr;
  int info = (!Af || (problem == 1 && !Bf)) ? hip_rc(hipErrorOutOfMemory) : 0;
  const Clock::time_point t0 = Clock::now();
  if (!info) info = gather_full(n, n, A_loc, desc_A, cell, Af, n);
  if (!info && problem == 1) info = gather_full(n, n, B_loc, desc_B, cell, Bf, n);
  const double tg = seconds(t0, Clock::now());
  if (!info) {
    info = replicated_host_locked(problem, n, n_vec, Af, n, Bf, n, w, Z_loc, desc_Z[8], cell,
                                  stage_seconds, n_stages);
    if (info > -1000) {
      extract_local(n, n, Af, n, desc_A, cell, A_loc);
      if (problem == 1) extract_local(n, n, Bf, n, desc_B, cell, B_loc);
    }
    if (stage_seconds && n_stages > EK_STAGE_GATHER) stage_seconds[EK_STAGE_GATHER] += tg;
  }
  free(Af); free(Bf);
  return info;
}

// A or B back as an uplo = 'L' array, in chunks of at most kTri columns as the pipeline's way out cuts them: the rows
// below a chunk's diagonal block straight into the caller's array (one 2-D copy), the diagonal block through a scratch
// of kTri x kTri doubles (2 MiB whatever the order -- EK_HIP_PIPE_MIN=0 sends N = 16384 down this path too), of which
// the caller's array receives the entries on and below the diagonal only.
int d2h_lower(hipStream_t s, int n, const double *u, double *M_loc, int ldm, double *tri) {
  constexpr int kTri = HostPipe::kTri;
  if (!tri) return hip_rc(hipErrorOutOfMemory);
  for (int a = 0; a < n; a += kTri) {
    const int b = (n - a < kTri) ? n : a + kTri, wdt = b - a;
    int r = d2h_matrix(wdt, wdt, u + (size_t)a * n + a, n, tri, wdt, s);
    if (!r && b < n) r = d2h_matrix(n - b, wdt, u + (size_t)a * n + b, n, M_loc + (size_t)a * ldm + b, ldm, s);
    if (!r) r = hip_rc(hipStreamSynchronize(s));
    if (r) return r;
    for (int c = 0; c < wdt; ++c)
      memcpy(M_loc + (size_t)(a + c) * ldm + a + c, tri + (size_t)c * wdt + c, (size_t)(wdt - c) * 8);
  }
  return 0;
}

// 1 x 1, through the staging pipeline: the copies overlap the stages (HostPipe): what remains exposed is B's way in, the
// rest of A's behind the Cholesky factorisation, and the last slab of Z
int solve_piped_host(int problem, int n, int n_vec, double *A_loc, int lda, double *B_loc, int ldb, double *w,
                     double *Z_loc, int ldz, HostImages &im, double *stage_seconds, int n_stages) {
  hipStream_t s = im.s;
  HostPipe pipe;
  pipe.hA = A_loc; pipe.ldha = lda; pipe.hB = B_loc; pipe.ldhb = problem == 1 ? ldb : 0;
  pipe.hZ = Z_loc; pipe.ldhz = ldz;
  EK_TRY(pipe.start(g_ctx.device));
  // (only the lower triangles travel: the device images' upper triangles are zeros, never garbage)
  auto zero_first = [&](double *u) -> int {
    if (!pipe.lower_only) return 0;
    EK_HIP_CHECK(hipMemsetAsync(u, 0, (size_t)n * n * 8, s));
    EK_HIP_CHECK(hipStreamSynchronize(s));
    return 0;
  };
  if (problem == 1) { EK_TRY(zero_first(im.uB)); pipe.push(false, im.uB, n, B_loc, ldb, n, n, nullptr, 0, /*lower=*/true); }
  EK_TRY(zero_first(im.uA));
  pipe.push(false, im.uA, n, A_loc, lda, n, n, nullptr, 1, /*lower=*/true);
  double st[EK_HIP_N_STAGES] = {0};
  PathCall c = im.call(problem, n, n_vec, n, st, EK_HIP_N_STAGES);
  c.pipe = &pipe;
  int info = solve_device_locked(c);
  const int rcp = pipe.finish();
  if (info == 0 && rcp) info = rcp;
  if (im.back(info)) im.out_w(w, n);
  info = im.wait(info);
  const double wall = seconds(im.t0, Clock::now());
  if (stage_seconds) {
    double dev = 0.0;
    for (int i = 0; i < EK_HIP_N_STAGES; ++i) if (i != EK_STAGE_COPY) dev += st[i];
    st[EK_STAGE_COPY] = wall > dev ? wall - dev : 0.0;     // what the copies add to the stages: their exposed part
    for (int i = 0; i < n_stages && i < EK_HIP_N_STAGES; ++i) stage_seconds[i] = st[i];
  }
  return info;
}

// 1 x 1: the caller's pointers are borrowed for the duration of the call only; from order EK_HIP_PIPE_MIN on through the
// staging pipeline (0: never), else copies before and after -- A and B then go back as uplo = 'L' arrays
int solve_single_host(int problem, int n, int n_vec, double *A_loc, int lda, double *B_loc, int ldb, double *w,
                      double *Z_loc, int ldz, double *stage_seconds, int n_stages) {
  HostImages im;
  EK_TRY(im.alloc(problem, n, n, (size_t)n * n, /*kept=*/true));
  const int pipe_min = switch_int(kSwPipeMin);
  if (pipe_min > 0 && n >= pipe_min)
    return solve_piped_host(problem, n, n_vec, A_loc, lda, B_loc, ldb, w, Z_loc, ldz, im, stage_seconds, n_stages);
  int info = im.in(problem, n, A_loc, lda, B_loc, ldb);
  if (!info) info = solve_device_locked(im.call(problem, n, n_vec, n, stage_seconds, n_stages));
  if (im.back(info)) {
    im.out(n, n_vec, im.uZ, n, Z_loc, ldz);
    // (no allocation that can throw across the C ABI)
    std::unique_ptr<double[]> tri(new (std::nothrow) double[(size_t)HostPipe::kTri * HostPipe::kTri]);
    if (!im.rc) im.rc = d2h_lower(im.s, n, im.uA, A_loc, lda, tri.get());
    if (!im.rc && problem == 1) im.rc = d2h_lower(im.s, n, im.uB, B_loc, ldb, tri.get());
    im.out_w(w, n);
  }
  return im.finish(info, stage_seconds, n_stages);
}
}  // namespace

extern "C" {

int ek_hip_eigenvalues(int problem, int n, int il, int iu, const double *A, int lda, const double *B, int ldb,
                       double *w, double *stage_seconds, int n_stages) {
  int rc = eigenvalues_args(problem, n, il, iu, A, lda, B, ldb, w); if (rc) return rc;
  rc = ensure_init(); if (rc) return rc;
  if (n == 0) return 0;
  std::lock_guard<std::mutex> lk(g_mu);
  const int m = iu - il + 1;
  // the caller's arrays are left as they are: the path works on device copies of them
  HostImages im;
  EK_TRY(im.alloc(problem, n, m, 0));
  EK_TRY(im.in(problem, n, A, lda, B, ldb));
  const int info = eigenvalues_locked(problem, n, il, iu, im.uA, n, im.uB, n, im.uw, stage_seconds, n_stages);
  if (im.back(info)) im.out_w(w, m);
  return im.finish(info, stage_seconds, n_stages);
}

int ek_hip_eigenpairs(int problem, int jobz, int range, int n, double vl, double vu, int il, int iu, const double *A,
                      int lda, const double *B, int ldb, int *m, int *ifirst, double *w, double *Z, int ldz, int zcap,
                      double *stage_seconds, int n_stages) {
  return eigenpairs_host(problem, 1, jobz, range, n, vl, vu, il, iu, A, lda, B, ldb, m, ifirst, w, Z, ldz, zcap,
                         stage_seconds, n_stages);
}

int ek_hip_sygvx(int itype, int jobz, int range, int n, double vl, double vu, int il, int iu, const double *A, int lda,
                 const double *B, int ldb, int *m, int *ifirst, double *w, double *Z, int ldz, int zcap,
                 double *stage_seconds, int n_stages) {
  if (itype < 1 || itype > 3) return -1;
  return eigenpairs_host(1, itype, jobz, range, n, vl, vu, il, iu, A, lda, B, ldb, m, ifirst, w, Z, ldz, zcap,
                         stage_seconds, n_stages);
}

int ek_hip_debug_last_pipe_stats(double *out, int count) {
  std::lock_guard<std::mutex> lk(g_mu);
  for (int i = 0; i < count && i < 12; ++i) out[i] = g_pipe_stats[i];
  return 0;
}

int ek_hip_set_allgatherv(ek_hip_allgatherv_fn fn, void *user) {
  std::lock_guard<std::mutex> lk(g_mu);
  g_allgatherv = fn; g_allgatherv_user = user;
  return 0;
}

// Pure host code (no GPU needed): the exchange step of ek_hip_solve for distributed inputs.
int ek_hip_gather_matrix(int m, int n, const double *M_loc, const int desc[9], int nprow, int npcol,
                         int myrow, int mycol, double *M_full, int ldf) {
  if (m < 0) return -1;
  if (n < 0) return -2;
  if (m > 0 && n > 0 && !M_loc) return -3;
  if (nprow < 1) return -5;
  if (npcol < 1) return -6;
  if (myrow < 0 || myrow >= nprow) return -7;
  if (mycol < 0 || mycol >= npcol) return -8;
  if (!desc) return -4;
  if (desc[4] < 1) return -405;
  int rc = check_desc(desc, 4, m, n, numroc0(m, desc[4], myrow, nprow)); if (rc) return rc;
  if (m > 0 && n > 0 && !M_full) return -9;
  if (ldf < (m > 1 ? m : 1)) return -10;
  std::lock_guard<std::mutex> lk(g_mu);
  if (!g_allgatherv) return -998;
  if (m == 0 || n == 0) return 0;
  const GridCell cell{desc[4], nprow, npcol, myrow, mycol};
  return gather_full(m, n, M_loc, desc, cell, M_full, ldf);
}

int ek_hip_solve_replicated(int problem, int n, int n_vec, double *A, int lda, double *B, int ldb,
                            double *w, double *Z_loc, const int desc_Z[9], int nprow, int npcol,
                            int myrow, int mycol, double *stage_seconds, int n_stages) {
  int rc = solve_args(problem, n, n_vec, A, lda, B, ldb, w, Z_loc); if (rc) return rc;
  if (nprow < 1) return -11;
  if (npcol < 1) return -12;
  if (myrow < 0 || myrow >= nprow) return -13;
  if (mycol < 0 || mycol >= npcol) return -14;
  if (!desc_Z) return -10;
  if (desc_Z[4] < 1) return -(10 * 100 + 5);
  rc = check_desc(desc_Z, 10, n, n, numroc0(n, desc_Z[4], myrow, nprow)); if (rc) return rc;
  rc = ensure_init(); if (rc) return rc;
  if (n == 0) return 0;
  std::lock_guard<std::mutex> lk(g_mu);
  const GridCell cell{desc_Z[4], nprow, npcol, myrow, mycol};
  return replicated_host_locked(problem, n, n_vec, A, lda, B, ldb, w, Z_loc, desc_Z[8], cell, stage_seconds,
                                n_stages);
}

int ek_hip_solve_sparse(int problem, int n, int n_vec, long long nnzA, const int *sufA, const double *valA,
                        long long nnzB, const int *sufB, const double *valB, double *w, double *Z_loc,
                        const int desc_Z[9], int nprow, int npcol, int myrow, int mycol, double *stage_seconds,
                        int n_stages) {
  if (problem != 0 && problem != 1) return -1;
  if (n < 0) return -2;
  if (n == 0) return 0;
  if (n_vec < 0 || n_vec > n) return -3;
  int rc = triplet_args(n, nnzA, sufA, valA, 4); if (rc) return rc;
  if (problem == 1) { rc = triplet_args(n, nnzB, sufB, valB, 7); if (rc) return rc; }
  if (!w) return -10;
  if (!Z_loc) return -11;
  if (nprow < 1) return -13;
  if (npcol < 1) return -14;
  if (myrow < 0 || myrow >= nprow) return -15;
  if (mycol < 0 || mycol >= npcol) return -16;
  if (!desc_Z) return -12;
  if (desc_Z[4] < 1) return -(12 * 100 + 5);
  rc = check_desc(desc_Z, 12, n, n, numroc0(n, desc_Z[4], myrow, nprow)); if (rc) return rc;
  rc = ensure_init(); if (rc) return rc;
  std::lock_guard<std::mutex> lk(g_mu);
  const GridCell cell{desc_Z[4], nprow, npcol, myrow, mycol};
  return sparse_host_locked(problem, n, n_vec, nnzA, sufA, valA, nnzB, sufB, valB, w, Z_loc, desc_Z[8], cell,
                            stage_seconds, n_stages);
}

int ek_hip_solve(int problem, int n, int n_vec, double *A_loc, const int desc_A[9], double *B_loc,
                 const int desc_B[9], double *w, double *Z_loc, const int desc_Z[9], int nprow,
                 int npcol, int myrow, int mycol, double *stage_seconds, int n_stages) {
  if (problem != 0 && problem != 1) return -1;
  if (n < 0) return -2;
  if (n_vec < 0 || n_vec > n) return -3;
  if (n > 0 && !A_loc) return -4;
  const bool cell_ok = nprow >= 1 && npcol >= 1 && myrow >= 0 && myrow < nprow;
  auto rows_of = [&](const int *d) {   // local row count the descriptor's lld must cover
    return (d && d[4] >= 1 && cell_ok) ? numroc0(n, d[4], myrow, nprow) : n;
  };
  int rc = check_desc(desc_A, 5, n, n, rows_of(desc_A)); if (rc) return rc;
  if (problem == 1) {
    if (n > 0 && !B_loc) return -6;
    rc = check_desc(desc_B, 7, n, n, rows_of(desc_B)); if (rc) return rc;
  }
  if (n > 0 && !w) return -8;
  if (n > 0 && !Z_loc) return -9;
  rc = check_desc(desc_Z, 10, n, n, rows_of(desc_Z)); if (rc) return rc;
  // grids other than 1x1 need the host's exchange hook (ek_hip_set_allgatherv)
  const bool have_exchange = g_allgatherv || (g_comm.on && nprow > 0 && npcol > 0 && g_comm.nranks == nprow * npcol);
  if (nprow != 1 && !(nprow > 1 && have_exchange)) return -11;
  if (npcol != 1 && !(npcol > 1 && have_exchange)) return -12;
  if (myrow < 0 || myrow >= nprow) return -13;
  if (mycol < 0 || mycol >= npcol) return -14;
  rc = ensure_init(); if (rc) return rc;
  if (n == 0) return 0;
  std::lock_guard<std::mutex> lk(g_mu);
  const GridCell cell{desc_Z[4], nprow, npcol, myrow, mycol};
  if (nprow * npcol == 1)
    return solve_single_host(problem, n, n_vec, A_loc, desc_A[8], B_loc, problem == 1 ? desc_B[8] : 0, w, Z_loc,
                             desc_Z[8], stage_seconds, n_stages);
  if (g_comm.on && g_comm.nranks == nprow * npcol)
    return solve_team_host(problem, n, n_vec, A_loc, desc_A, B_loc, desc_B, w, Z_loc, desc_Z, cell, stage_seconds, n_stages);
  return solve_hook_host(problem, n, n_vec, A_loc, desc_A, B_loc, desc_B, w, Z_loc, desc_Z, cell, stage_seconds, n_stages);
}

}  // extern "C"
