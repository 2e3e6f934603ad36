// ek_batched_check.hip -- ek_hip_check_batched* / ek_hip_check_vbatched*: the reference's acceptance checks and the
// inverse participation ratios of EVERY problem of a batch, with the normalisations of ek_verify.hip (and of
// eigenkernel_amd/verifier.py), in one launch per kernel class.
//
// One workgroup owns a problem from its first load to its last store; the classes are the solver's (order <= 32, 64,
// 128, T = 2 NC threads).  Z lives in LDS the whole time, as an image with the odd leading dimension NC + 1 of
// ek_batched.hip; thread (r, h) = (t % NC, t / NC) owns column r of Z and half h of the work on it.
//
//   1  the rows of the symmetric A and B stream from global memory through staged LDS vectors, two rows a step (row
//      2m + h for half h), loaded one step ahead: entry (i, k) with k > i is read as (k, i), so that only the lower
//      triangles are referenced.  Thread (r, h) forms (A Z)_ir and s_ir = (B Z)_ir over k in ascending order and adds
//      r_ir^2 = ((A Z)_ir - w_r s_ir)^2, z_ir s_ir and z_ir^4 to its own sums in row order; the square of the entry of
//      A it staged goes to its own sum for ||A||_F.  Generalized problems leave S = B Z in a device scratch of n^2
//      doubles (standard problems need none: S = Z)
//   2  the halves' sums meet in a fixed order: ||r_j||, G_jj = sum_i z_ij s_ij (the IPR's denominator and the scaling
//      of the orthogonality check), sum_i z_ij^4
//   3  column of S by column of S (two a step, staged like the rows; for a standard problem read from the image
//      itself), thread (l, h) forms G_lj = sum_i z_il s_ij and adds (G_lj / sqrt(G_ll) / sqrt(G_jj))^2, j != l, to
//      its own sum
//
// Same bits wherever a problem sits: a problem's outputs depend on (n, A, B, w, Z) alone -- fixed loop orders, sums
// across the workgroup by a fixed butterfly and a fixed order over the waves, no atomics, one code path per class, the
// same kernel body for the strided and the table form.  A, B, w and Z are read only.
//
// ek_hip_check_sygv_batched* / ek_hip_check_sygv_vbatched*  check DSYGV's types 2 (A B x = l x) and 3
// (B A x = l x): the same entries, classes, table and scatter, with the kernel of ek_batched_check_sygv.hip in the place of
// the one below (a translation unit of its own, so that the code generated for this one stays what it was).
//
// The host side of EVERY uniform-order check entry lives below the kernel: one argument checker, one device
// pool with one release function, one run function and one stager of host arrays, declared in ek_batched_check.h.
// ek_batched_check_x.hip and ek_batched_check_sygv_x.hip (orders above EK_HIP_BATCH_NMAX) keep their kernel, its launch
// and thin entries, and hand this driver a launch function.  All entries serialise on g_mu, so one pool serves them all.
// ek_batched_check_window.hip (ek_hip_check_window_xbatched*) does the same with the window driver beside it
// (window_arguments, window_entry): the same pool, events, chunk size and fetch, a count m[b] per problem.
// ek_batched_check_sygv_window.hip (ek_hip_check_sygv_window_xbatched*) is that driver's second user.
//
// The variable-order entries for orders up to EK_HIP_XBATCH_NMAX (ek_hip_check_xvbatched*, ek_hip_check_sygv_xvbatched*,
// DESIGN.md 24) are this unit's too: the variable driver with a fourth class in front, whose launches are those two units'
// table instantiations (bcheck::launch_x, bcheck::launch_sygv_x).
//
// The variable-order window checks (ek_hip_check_window_xvbatched*, ek_hip_check_sygv_window_xvbatched*) are
// this unit's as well: the window driver's count m[b] per problem on the variable driver's table, one class for every
// order (vwindow_check, vwindow_entry), launching the table instantiations of the two window units' kernels.
#include "ek_batched_check.h"

#include <algorithm>

namespace ek {
namespace bcheck {

// ARGS: how the workgroup finds its problem -- Args (one order, strided) or VArgs (a table entry)
template <int NC, int T, typename ARGS>
__global__ __launch_bounds__(T) void check_kernel(ARGS a) {
  constexpr int LD = NC + 1, NW = T / 64;
  static_assert(T == 2 * NC && T % 64 == 0, "two threads per column");
  extern __shared__ double smem[];
  double *Zs = smem;                      // NC x NC image of Z, leading dimension LD
  double *sa = Zs + NC * LD;              // [buffer][half][NC]: rows of A; step 3: columns of S
  double *sb = sa + 4 * NC;               // the same for B
  double *sg = sb + 4 * NC;               // 1 / sqrt(G_jj)
  double *red = sg + NC;                  // a word per wave
  double *sx = sa;                        // step 2: [3][half][NC], the halves' sums of r^2, z s and z^4

  const Problem p = locate(a);
  const int t = threadIdx.x, n = p.n;
  const int r = t % NC, h = t / NC;
  const bool col = r < n;
  const bool gen = a.problem != 0;
  cgdouble *A = p.A;
  cgdouble *B = p.B;
  const int lda = p.lda, ldb = p.ldb;
  gdouble *S = p.S;

  if (col)
    for (int j = h; j < n; j += 2) Zs[r + j * LD] = p.Z[r + (size_t)j * p.ldz];
  const double wr = col ? p.w[r] : 0.0;

  // ---- 1: R = A Z - B Z diag(w), S = B Z, the diagonal of G = Z^T S, sum z^4, ||A||_F^2
  // entry (i, r) of the symmetric matrix whose lower triangle is M
  auto entry = [&](cgdouble *M, int ld, int i) { return (r <= i) ? M[i + (size_t)r * ld] : M[r + (size_t)i * ld]; };
  double asq = 0.0, rs = 0.0, gd = 0.0, p4 = 0.0;
  {
    double xa = 0.0, xb = 0.0;
    if (col && h < n) {
      xa = entry(A, lda, h);
      if (gen) xb = entry(B, ldb, h);
    }
    sa[h * NC + r] = xa;
    sb[h * NC + r] = xb;
    asq = fma(xa, xa, asq);
  }
  __syncthreads();
  const double *zc = Zs + r * LD;
  const int steps = (n + 1) >> 1;
  for (int m = 0; m < steps; ++m) {
    const int i = 2 * m + h, in = i + 2;
    double xa = 0.0, xb = 0.0;                      // the row after this one: in flight while this one is used
    if (col && in < n) {
      xa = entry(A, lda, in);
      if (gen) xb = entry(B, ldb, in);
    }
    if (col && i < n) {
      const int off = ((m & 1) * 2 + h) * NC;
      const double zi = zc[i];
      double az, bz;
      if (gen) {
        lds_dot2(sa + off, sb + off, zc, n, az, bz);
        S[i + (size_t)r * n] = bz;
      } else {
        az = lds_dot(sa + off, zc, n);
        bz = zi;
      }
      const double rr = fma(-wr, bz, az);
      const double z2 = zi * zi;
      rs = fma(rr, rr, rs);
      gd = fma(zi, bz, gd);
      p4 = fma(z2, z2, p4);
    }
    const int offn = (((m + 1) & 1) * 2 + h) * NC;
    sa[offn + r] = xa;
    sb[offn + r] = xb;
    asq = fma(xa, xa, asq);
    __syncthreads();
  }

  // ---- 2: the halves meet
  sx[h * NC + r] = rs;
  sx[(2 + h) * NC + r] = gd;
  sx[(4 + h) * NC + r] = p4;
  __syncthreads();
  double rn = 0.0;
  if (h == 0 && col) {
    rn = sqrt(sx[r] + sx[NC + r]);
    const double g = sx[2 * NC + r] + sx[3 * NC + r];
    const double q = sx[4 * NC + r] + sx[5 * NC + r];
    sg[r] = 1.0 / sqrt(g);
    if (p.ipr) p.ipr[r] = q / (g * g);
  }
  const double rsum = wg_reduce<NW, false>(rn, red);
  const double rmax = wg_reduce<NW, true>(rn, red);
  const double anorm = sqrt(wg_reduce<NW, false>(asq, red));
  __syncthreads();                                  // sg is written, S is in the scratch for the whole workgroup

  // ---- 3: || D^-1/2 G D^-1/2 - its diagonal ||_F
  double os = 0.0;
  if (gen) {
    sa[h * NC + r] = (col && h < n) ? S[r + (size_t)h * n] : 0.0;
    __syncthreads();
    for (int m = 0; m < steps; ++m) {
      const int j = 2 * m + h, jn = j + 2;
      double xs = 0.0;
      if (col && jn < n) xs = S[r + (size_t)jn * n];
      if (col && j < n && j != r) {
        const double g = lds_dot(zc, sa + ((m & 1) * 2 + h) * NC, n) * sg[r] * sg[j];
        os = fma(g, g, os);
      }
      sa[(((m + 1) & 1) * 2 + h) * NC + r] = xs;
      __syncthreads();
    }
  } else if (col) {
    for (int j = h; j < n; j += 2) {
      if (j == r) continue;
      const double g = lds_dot(zc, Zs + j * LD, n) * sg[r] * sg[j];
      os = fma(g, g, os);
    }
  }
  const double osum = wg_reduce<NW, false>(os, red);
  if (t == 0) {
    p.out[0] = anorm;
    p.out[1] = rsum / anorm / (double)n;
    p.out[2] = rmax / anorm;
    p.out[3] = sqrt(osum);
  }
}

// itype: 0 the standard problem and type 1 (this unit's kernel), 2 or 3 those types (launch_sygv)
template <int NC, int T, typename ARGS>
static int launch_class(hipStream_t s, int count, const ARGS &a, int itype) {
  if (itype) return launch_sygv(s, itype, NC, count, a);
  constexpr size_t lds = (size_t)lds_doubles(NC) * sizeof(double);
  static bool raised = false;                       // one per instantiation
  if (lds > 64 * 1024 && !raised) {
    EK_HIP_CHECK(hipFuncSetAttribute((const void *)check_kernel<NC, T, ARGS>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    raised = true;
  }
  hipLaunchKernelGGL((check_kernel<NC, T, ARGS>), dim3(count), dim3(T), lds, s, a);
  EK_HIP_CHECK(hipGetLastError());
  return 0;
}

static int class_of(int n) { return n <= 32 ? 32 : n <= 64 ? 64 : 128; }
constexpr int kClasses = 4;                         // the variable form's: 256 (orders above EK_HIP_BATCH_NMAX), 128, 64, 32

// Device memory the entries of all three units keep (grown, never shrunk, released in ek_hip_finalize): the scratch S, the
// output words (out, then the IPRs), the table or the map of the problems to check; two events for `seconds`.  A call
// writes what it reads: the map or table is uploaded whenever it is used, the scratch is written before it is read
static double *g_scratch = nullptr, *g_dout = nullptr;
static void *g_dtable = nullptr;
static size_t g_scratch_count = 0, g_dout_count = 0, g_dtable_bytes = 0;
static hipEvent_t g_ev[2] = {nullptr, nullptr};
// the variable form's last call that was given `seconds` (ek_hip_debug_check_xvbatched_last): an event before each class
// and one behind the last, created by the first such call
static hipEvent_t g_cev[kClasses + 1] = {nullptr, nullptr, nullptr, nullptr, nullptr};
static double g_class_seconds[kClasses] = {0.0, 0.0, 0.0, 0.0};
static int g_class_count[kClasses] = {0, 0, 0, 0};
static std::vector<Desc> g_htable;                  // host images: an upload may still read them when an error returns
static std::vector<int> g_hmap;
static std::vector<double> g_hout;
constexpr int kChunk = 1024;                        // problems per launch of the kernels above EK_HIP_BATCH_NMAX, whose
static int g_chunk = kChunk;                        // scratch is per workgroup (ek_hip_debug_check_xbatched_chunk)

template <typename P>
static int grow(P **p, size_t *have, size_t want, size_t unit) {
  if (want <= *have) return 0;
  if (*p) (void)hipFree((void *)*p);
  *p = nullptr;
  *have = 0;
  EK_HIP_CHECK(hipMalloc((void **)p, want * unit));
  *have = want;
  return 0;
}

static int ensure(size_t scratch, size_t dout, size_t table_bytes) {
  { int rc = grow(&g_scratch, &g_scratch_count, scratch, sizeof(double)); if (rc) return rc; }
  { int rc = grow(&g_dout, &g_dout_count, dout, sizeof(double)); if (rc) return rc; }
  { int rc = grow((char **)&g_dtable, &g_dtable_bytes, table_bytes, 1); if (rc) return rc; }
  for (int k = 0; k < 2; ++k)
    if (!g_ev[k]) EK_HIP_CHECK(hipEventCreate(&g_ev[k]));
  return 0;
}

}  // namespace bcheck

namespace api {
void release_batched_check() {
  using namespace bcheck;
  if (g_scratch) (void)hipFree(g_scratch);
  if (g_dout) (void)hipFree(g_dout);
  if (g_dtable) (void)hipFree(g_dtable);
  g_scratch = g_dout = nullptr;
  g_dtable = nullptr;
  g_scratch_count = g_dout_count = g_dtable_bytes = 0;
  for (int k = 0; k < 2; ++k) {
    if (g_ev[k]) (void)hipEventDestroy(g_ev[k]);
    g_ev[k] = nullptr;
  }
  for (int k = 0; k <= kClasses; ++k) {
    if (g_cev[k]) (void)hipEventDestroy(g_cev[k]);
    g_cev[k] = nullptr;
  }
  std::vector<Desc>().swap(g_htable);
  std::vector<int>().swap(g_hmap);
  std::vector<double>().swap(g_hout);
}
}  // namespace api
}  // namespace ek

using namespace ek;
using namespace ek::api;

static const double kNaN = std::nan("");

// The argument errors of every uniform-order entry: nmax is the entry's largest order, B is looked at when u.problem is 1
// (the entries of DSYGV's types call with problem = 1, after their own test of itype).  No data pointer is dereferenced.
int ek::bcheck::uniform_arguments(const Uniform &u, int nmax, bool *nothing) {
  const int n = u.n;
  *nothing = false;
  if (u.problem != 0 && u.problem != 1) return -1;
  if (n < 0 || n > nmax) return -2;
  if (u.batch < 0) return -3;
  if (n == 0 || u.batch == 0) { *nothing = true; return 0; }
  if (!u.A) return -4;
  if (u.lda < n) return -5;
  if (u.sA < (long long)u.lda * n) return -6;
  if (u.problem == 1) {
    if (!u.B) return -7;
    if (u.ldb < n) return -8;
    if (u.sB < (long long)u.ldb * n) return -9;
  }
  if (!u.w) return -10;
  if (!u.Z) return -11;
  if (u.ldz < n) return -12;
  if (u.sZ < (long long)u.ldz * n) return -13;
  if (!u.out) return -15;                           // 14 is info: NULL means every problem
  return 0;
}

// The launches' end: the output words come to the host, and problem b's go to the caller's out and ipr unless it was
// skipped.  ipr_of(b): where the caller wants problem b's IPRs (or nullptr); off[b]: where they are behind the out words.
template <typename NOF, typename IPR>
static void scatter(int batch, NOF n_of, const int *info, const std::vector<size_t> &off, double *out, IPR ipr_of) {
  const double *h = bcheck::g_hout.data();
  for (int b = 0; b < batch; ++b) {
    double *o = out + (size_t)b * EK_HIP_CHECK_NOUT;
    const int n = n_of(b);
    if (info && info[b] != 0) {
      o[0] = o[1] = o[2] = o[3] = kNaN;
    } else if (n == 0) {
      o[0] = 0.0;
      o[1] = o[2] = o[3] = kNaN;
    } else {
      std::memcpy(o, h + (size_t)b * EK_HIP_CHECK_NOUT, EK_HIP_CHECK_NOUT * sizeof(double));
      double *q = ipr_of(b);
      if (q) std::memcpy(q, h + off[b], (size_t)n * sizeof(double));
    }
  }
}

// launches on the context's stream between the two events, the output words to the host, one synchronise
template <typename LAUNCH>
static int run_and_fetch(size_t words, double *seconds, LAUNCH launch) {
  using namespace bcheck;
  hipStream_t s = g_ctx.stream;
  if (seconds) (void)hipEventRecord(g_ev[0], s);
  int rc = launch(s);
  if (seconds) (void)hipEventRecord(g_ev[1], s);
  g_hout.resize(words);
  hipError_t e = hipSuccess;
  if (!rc) e = hipMemcpyAsync(g_hout.data(), g_dout, words * sizeof(double), hipMemcpyDeviceToHost, s);
  hipError_t es = hipStreamSynchronize(s);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess && !rc) rc = -1000 - (int)e;
  if (seconds && !rc) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, g_ev[0], g_ev[1]) == hipSuccess) *seconds = (double)ms * 1e-3;
  }
  return rc;
}

// arguments checked (n > 0, batch > 0), context up, g_mu held; u.A, u.B, u.w, u.Z device.  Everything of a call but the
// kernel: the map of the problems to check from info, the pool, the events, the launches, the fetch, the scatter.
// `chunked` says how the kernel indexes its scratch of `scratch` doubles: by problem number (false: one launch for all),
// or by workgroup (true: g_chunk problems a launch, one after the other on the stream because they share the scratch)
static int uniform_run(const bcheck::Uniform &u, size_t scratch, bool chunked, bcheck::UniformLaunch launch) {
  using namespace bcheck;
  const int n = u.n, batch = u.batch;
  g_hmap.clear();
  bool skip = false;
  if (u.info)
    for (int b = 0; b < batch; ++b) {
      if (u.info[b] == 0) g_hmap.push_back(b); else skip = true;
    }
  const int count = skip ? (int)g_hmap.size() : batch;
  const size_t nout = (size_t)batch * EK_HIP_CHECK_NOUT, words = nout + (u.ipr ? (size_t)batch * n : 0);
  std::vector<size_t> off((size_t)batch);
  for (int b = 0; b < batch; ++b) off[b] = nout + (size_t)b * n;
  if (count > 0) {
    const int K = chunked ? g_chunk : count;
    int rc = ensure((size_t)(chunked ? std::min(count, K) : batch) * scratch, words, skip ? g_hmap.size() * sizeof(int) : 0);
    if (rc) return rc;
    rc = run_and_fetch(words, u.seconds, [&](hipStream_t s) -> int {
      if (skip) EK_HIP_CHECK(hipMemcpyAsync(g_dtable, g_hmap.data(), g_hmap.size() * sizeof(int), hipMemcpyHostToDevice, s));
      for (int c0 = 0; c0 < count; c0 += K) {
        const int rcl = launch(s, u, skip ? (const int *)g_dtable : nullptr, c0, std::min(K, count - c0), g_scratch, g_dout,
                               u.ipr ? g_dout + nout : nullptr);
        if (rcl) return rcl;
      }
      return 0;
    });
    if (rc) return rc;
  }
  scatter(batch, [&](int) { return n; }, u.info, off, u.out,
          [&](int b) { return u.ipr ? u.ipr + (size_t)b * n : nullptr; });
  return 0;
}

// What follows the argument check in every uniform-order entry.  host: A, B, w and Z are host arrays and get device copies
// with the caller's own layout, as in ek_hip_eigenpairs_batched (B only when the call has one)
int ek::bcheck::uniform_entry(const Uniform &u, bool nothing, bool host, size_t scratch, bool chunked,
                              UniformLaunch launch) {
  if (u.seconds) *u.seconds = 0.0;
  if (nothing) return 0;
  int rc = ensure_init(); if (rc) return rc;
  std::lock_guard<std::mutex> lk(g_mu);
  if (!host) return uniform_run(u, scratch, chunked, launch);
  hipStream_t s = g_ctx.stream;
  const int n = u.n, batch = u.batch, problem = u.problem;
  auto span = [&](int ld, long long stride) { return (size_t)(batch - 1) * (size_t)stride + (size_t)ld * (n - 1) + n; };
  const size_t cA = span(u.lda, u.sA), cB = problem ? span(u.ldb, u.sB) : 0, cZ = span(u.ldz, u.sZ);
  const size_t cw = (size_t)batch * n;
  DevMem mem;
  double *uA = nullptr, *uB = nullptr, *uw = nullptr, *uZ = nullptr;
  rc = mem.alloc(&uA, cA * 8);
  if (!rc) rc = mem.alloc(&uw, cw * 8);
  if (!rc && problem) rc = mem.alloc(&uB, cB * 8);
  if (!rc) rc = mem.alloc(&uZ, cZ * 8);
  if (rc) return rc;
  EK_HIP_CHECK(hipMemcpyAsync(uA, u.A, cA * 8, hipMemcpyHostToDevice, s));
  if (problem) EK_HIP_CHECK(hipMemcpyAsync(uB, u.B, cB * 8, hipMemcpyHostToDevice, s));
  EK_HIP_CHECK(hipMemcpyAsync(uw, u.w, cw * 8, hipMemcpyHostToDevice, s));
  EK_HIP_CHECK(hipMemcpyAsync(uZ, u.Z, cZ * 8, hipMemcpyHostToDevice, s));
  Uniform d = u;
  d.A = uA; d.B = uB; d.w = uw; d.Z = uZ;
  return uniform_run(d, scratch, chunked, launch);
}

// ---- the window check (ek_hip_check_window_xbatched*): the driver above with a count m[b] per problem
static bool window_skipped(const bcheck::Window &w, int b) { return w.u.info && w.u.info[b] != 0; }

// The argument errors in the order of the prototype (17 arguments before ipr and seconds: 10 is m, 14 zcap, 16 info).  m and
// info are host arrays and are read; no data pointer is dereferenced
int ek::bcheck::window_arguments(const Window &w, int nmax, bool *nothing) {
  const Uniform &u = w.u;
  const int n = u.n;
  *nothing = false;
  // the sygv form carries the caller's itype and problem = 1: B is required for every type
  if (w.sygv ? (u.itype < 1 || u.itype > 3) : (u.problem != 0 && u.problem != 1)) return -1;
  if (n < 0 || n > nmax) return -2;
  if (u.batch < 0) return -3;
  if (n == 0 || u.batch == 0) { *nothing = true; return 0; }
  if (!u.A) return -4;
  if (u.lda < n) return -5;
  if (u.sA < (long long)u.lda * n) return -6;
  if (u.problem == 1) {
    if (!u.B) return -7;
    if (u.ldb < n) return -8;
    if (u.sB < (long long)u.ldb * n) return -9;
  }
  if (!w.m) return -10;
  for (int b = 0; b < u.batch; ++b)
    if (!window_skipped(w, b) && (w.m[b] < 0 || w.m[b] > n)) return -10;
  if (!u.w) return -11;
  if (!u.Z) return -12;
  if (u.ldz < n) return -13;
  if (w.zcap < 0) return -14;
  for (int b = 0; b < u.batch; ++b)
    if (!window_skipped(w, b) && w.m[b] > w.zcap) return -14;
  if (u.sZ < (long long)u.ldz * std::max(1, w.zcap)) return -15;
  if (!u.out) return -17;                           // 16 is info: NULL means every problem
  return 0;
}

// arguments checked, at least one problem to check, context up, g_mu held; u.A, u.B, u.w, u.Z device.  g_hmap holds the
// pairs (problem, m) by descending m -- the widest windows first, so that a launch ends on its cheapest problems; the bit
// contract makes the order invisible
static int window_run(const bcheck::Window &w, bcheck::WindowLaunch launch) {
  using namespace bcheck;
  const Uniform &u = w.u;
  const int n = u.n, batch = u.batch, count = (int)(g_hmap.size() / 2), cmax = g_hmap[1];
  const size_t nout = (size_t)batch * EK_HIP_CHECK_NOUT, words = nout + (u.ipr ? (size_t)batch * n : 0);
  const int K = g_chunk;
  // S = B Z (problem 1, type 2) or U = A Z, then W^T (type 3): n x the widest window; type 3: the factor in front of it
  const long long sS = u.problem ? (long long)n * cmax + (u.itype == 3 ? (long long)n * n : 0) : 0;
  int rc = ensure((size_t)std::min(count, K) * (size_t)sS, words, g_hmap.size() * sizeof(int));
  if (rc) return rc;
  rc = run_and_fetch(words, u.seconds, [&](hipStream_t s) -> int {
    EK_HIP_CHECK(hipMemcpyAsync(g_dtable, g_hmap.data(), g_hmap.size() * sizeof(int), hipMemcpyHostToDevice, s));
    for (int c0 = 0; c0 < count; c0 += K) {
      const int rcl = launch(s, w, (const int *)g_dtable, c0, std::min(K, count - c0), sS, g_scratch, g_dout,
                             u.ipr ? g_dout + nout : nullptr);
      if (rcl) return rcl;
    }
    return 0;
  });
  if (rc) return rc;
  const double *h = g_hout.data();
  for (int b = 0; b < batch; ++b) {
    double *o = u.out + (size_t)b * EK_HIP_CHECK_NOUT;
    if (window_skipped(w, b) || w.m[b] == 0) {
      o[0] = o[1] = o[2] = o[3] = kNaN;
    } else {
      std::memcpy(o, h + (size_t)b * EK_HIP_CHECK_NOUT, EK_HIP_CHECK_NOUT * sizeof(double));
      if (u.ipr) std::memcpy(u.ipr + (size_t)b * n, h + nout + (size_t)b * n, (size_t)w.m[b] * sizeof(double));
    }
  }
  return 0;
}

int ek::bcheck::window_entry(const Window &w, bool nothing, bool host, WindowLaunch launch) {
  const Uniform &u = w.u;
  if (u.seconds) *u.seconds = 0.0;
  if (nothing) return 0;
  const int n = u.n, batch = u.batch, problem = u.problem;
  std::vector<int> order;
  for (int b = 0; b < batch; ++b)
    if (!window_skipped(w, b) && w.m[b] > 0) order.push_back(b);
  if (order.empty()) {                              // nothing to check: no context, no device
    for (size_t k = 0; k < (size_t)batch * EK_HIP_CHECK_NOUT; ++k) u.out[k] = kNaN;
    return 0;
  }
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return w.m[x] > w.m[y]; });
  int rc = ensure_init(); if (rc) return rc;
  std::lock_guard<std::mutex> lk(g_mu);
  g_hmap.clear();
  for (int b : order) { g_hmap.push_back(b); g_hmap.push_back(w.m[b]); }
  if (!host) return window_run(w, launch);
  // device copies with the caller's own layout; zcap >= 1 here, since some m[b] is
  hipStream_t s = g_ctx.stream;
  auto span = [&](int ld, long long stride, int cols) {
    return (size_t)(batch - 1) * (size_t)stride + (size_t)ld * (cols - 1) + n;
  };
  const size_t cA = span(u.lda, u.sA, n), cB = problem ? span(u.ldb, u.sB, n) : 0, cZ = span(u.ldz, u.sZ, w.zcap);
  const size_t cw = (size_t)batch * n;
  DevMem mem;
  double *uA = nullptr, *uB = nullptr, *uw = nullptr, *uZ = nullptr;
  rc = mem.alloc(&uA, cA * 8);
  if (!rc) rc = mem.alloc(&uw, cw * 8);
  if (!rc && problem) rc = mem.alloc(&uB, cB * 8);
  if (!rc) rc = mem.alloc(&uZ, cZ * 8);
  if (rc) return rc;
  EK_HIP_CHECK(hipMemcpyAsync(uA, u.A, cA * 8, hipMemcpyHostToDevice, s));
  if (problem) EK_HIP_CHECK(hipMemcpyAsync(uB, u.B, cB * 8, hipMemcpyHostToDevice, s));
  EK_HIP_CHECK(hipMemcpyAsync(uw, u.w, cw * 8, hipMemcpyHostToDevice, s));
  EK_HIP_CHECK(hipMemcpyAsync(uZ, u.Z, cZ * 8, hipMemcpyHostToDevice, s));
  Window d = w;
  d.u.A = uA; d.u.B = uB; d.u.w = uw; d.u.Z = uZ;
  return window_run(d, launch);
}

// this unit's part of a call: the class kernels (orders up to EK_HIP_BATCH_NMAX) index everything by problem number
static int launch_uniform(hipStream_t s, const bcheck::Uniform &u, const int *map, int, int count, double *S, double *dout,
                          double *dipr) {
  using namespace bcheck;
  Args a{u.problem, u.n, u.A, u.lda, u.sA, u.B, u.ldb, u.sB, u.w, u.Z, u.ldz, u.sZ, map, S, dout, dipr};
  switch (class_of(u.n)) {
    case 32: return launch_class<32, 64>(s, count, a, u.itype);
    case 64: return launch_class<64, 128>(s, count, a, u.itype);
    default: return launch_class<128, 256>(s, count, a, u.itype);
  }
}

// All arrays are host arrays of `batch` entries; the pointers in the pointer arrays are not dereferenced.  nmax is the
// entry's largest order (EK_HIP_BATCH_NMAX, or EK_HIP_XBATCH_NMAX for ek_hip_check_*xvbatched*).
static int variable_check(int problem, int batch, const int *n, const void *const *A, const int *lda,
                          const void *const *B, const int *ldb, const void *const *w, const void *const *Z,
                          const int *ldz, const double *out, int nmax, bool *nothing) {
  *nothing = false;
  if (problem != 0 && problem != 1) return -1;
  if (batch < 0) return -2;
  if (batch == 0) { *nothing = true; return 0; }
  if (!n) return -3;
  for (int b = 0; b < batch; ++b)
    if (n[b] < 0 || n[b] > nmax) return -3;
  auto entries = [&](const void *const *P) {
    if (!P) return false;
    for (int b = 0; b < batch; ++b)
      if (n[b] > 0 && !P[b]) return false;
    return true;
  };
  auto leading = [&](const int *ld) {
    if (!ld) return false;
    for (int b = 0; b < batch; ++b)
      if (ld[b] < (n[b] > 1 ? n[b] : 1)) return false;
    return true;
  };
  if (!entries(A)) return -4;
  if (!leading(lda)) return -5;
  if (problem == 1) {
    if (!entries(B)) return -6;
    if (!leading(ldb)) return -7;
  }
  if (!entries(w)) return -8;
  if (!entries(Z)) return -9;
  if (!leading(ldz)) return -10;
  if (!out) return -12;                             // 11 is info: NULL means every problem
  return 0;
}

// arguments checked (batch > 0), context up, g_mu held; the pointers in dA, dB, dw, dZ are device addresses; itype as above.
// The orders above EK_HIP_BATCH_NMAX (ek_hip_check_*xvbatched* alone let them through) form a class of their own in front
// of the other three: chunk c of at most g_chunk entries runs over the table's slice [c g_chunk, ...) with the kernels of
// ek_batched_check_x.hip / ek_batched_check_sygv_x.hip, and every entry of a chunk names its own slot of the chunk's
// scratch (prefix sums inside the chunk), which the next chunk uses again.  Everything runs on the context's stream, a
// launch behind the other, so the classes up to 128 lay their n^2 per problem over the same buffer from its start.
static int variable_device_locked(int itype, int problem, int batch, const int *n, const double *const *dA,
                                  const int *lda, const double *const *dB, const int *ldb, const double *const *dw,
                                  const double *const *dZ, const int *ldz, const int *info, double *out,
                                  double *const *ipr, double *seconds) {
  using namespace bcheck;
  // the solver's order: a class after the other, the largest first, descending order inside a class
  std::vector<int> order;
  order.reserve((size_t)batch);
  for (int b = 0; b < batch; ++b)
    if (n[b] > 0 && !(info && info[b] != 0)) order.push_back(b);
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return n[x] > n[y]; });
  const size_t nout = (size_t)batch * EK_HIP_CHECK_NOUT;
  const int K = g_chunk;
  const size_t slots = itype == 3 ? 2 : problem ? 1 : 0;   // of n^2 doubles, per entry of the class of 256
  std::vector<size_t> off((size_t)batch, 0), offs((size_t)batch, 0);
  size_t words = nout, scratch = 0, small = 0, chunk = 0;
  int count[kClasses] = {0, 0, 0, 0};               // classes of 256, 128, 64, 32
  for (int b : order) {
    if (ipr && ipr[b]) { off[b] = words; words += (size_t)n[b]; }
    if (n[b] > EK_HIP_BATCH_NMAX) {
      if (count[0] % K == 0) chunk = 0;             // a chunk's first entry
      offs[b] = chunk;
      chunk += slots * (size_t)n[b] * n[b];
      scratch = std::max(scratch, chunk);
      ++count[0];
    } else {
      const int c = class_of(n[b]);
      ++count[c == 128 ? 1 : c == 64 ? 2 : 3];
      if (problem) { offs[b] = small; small += (size_t)n[b] * n[b]; }
    }
  }
  scratch = std::max(scratch, small);
  if (seconds)
    for (int k = 0; k < kClasses; ++k) { g_class_seconds[k] = 0.0; g_class_count[k] = count[k]; }
  if (!order.empty()) {
    int rc = ensure(scratch, words, order.size() * sizeof(Desc));
    if (rc) return rc;
    if (seconds)
      for (int k = 0; k <= kClasses; ++k)
        if (!g_cev[k]) EK_HIP_CHECK(hipEventCreate(&g_cev[k]));
    g_htable.resize(order.size());
    for (size_t i = 0; i < order.size(); ++i) {
      const int b = order[i];
      const bool has_s = n[b] > EK_HIP_BATCH_NMAX ? slots != 0 : problem != 0;
      g_htable[i] = Desc{dA[b], problem ? dB[b] : nullptr, dw[b], dZ[b], has_s ? g_scratch + offs[b] : nullptr,
                         (ipr && ipr[b]) ? g_dout + off[b] : nullptr, n[b], lda[b], problem ? ldb[b] : 1, ldz[b], b, 0};
    }
    rc = run_and_fetch(words, seconds, [&](hipStream_t s) -> int {
      EK_HIP_CHECK(hipMemcpyAsync(g_dtable, g_htable.data(), g_htable.size() * sizeof(Desc), hipMemcpyHostToDevice, s));
      int rcl = 0, at = 0;
      for (int k = 0; k < kClasses && !rcl; ++k) {
        if (seconds) (void)hipEventRecord(g_cev[k], s);
        if (!count[k]) continue;
        if (k == 0) {
          for (int c0 = 0; c0 < count[0] && !rcl; c0 += K) {
            VArgs a{problem, (const Desc *)g_dtable + c0, g_dout};
            const int cnt = std::min(K, count[0] - c0);
            rcl = itype ? launch_sygv_x(s, itype, cnt, a) : launch_x(s, cnt, a);
          }
        } else {
          VArgs a{problem, (const Desc *)g_dtable + at, g_dout};
          rcl = k == 1 ? launch_class<128, 256>(s, count[k], a, itype)
              : k == 2 ? launch_class<64, 128>(s, count[k], a, itype) : launch_class<32, 64>(s, count[k], a, itype);
        }
        at += count[k];
      }
      if (seconds && !rcl) (void)hipEventRecord(g_cev[kClasses], s);
      return rcl;
    });
    if (rc) return rc;
    if (seconds)
      for (int k = 0; k < kClasses; ++k) {
        float ms = 0.f;
        if (count[k] && hipEventElapsedTime(&ms, g_cev[k], g_cev[k + 1]) == hipSuccess) g_class_seconds[k] = (double)ms * 1e-3;
      }
  }
  scatter(batch, [&](int b) { return n[b]; }, info, off, out,
          [&](int b) { return (ipr && ipr[b]) ? ipr[b] : nullptr; });
  return 0;
}

// The entries behind both families: ek_hip_check_*batched* (itype = 0) and ek_hip_check_sygv_*batched* (itype = 2, 3
// with problem = 1; their itype 1 is problem 1 of the first family)
static int class_entry(const bcheck::Uniform &u, bool host) {
  bool nothing;
  int rc = bcheck::uniform_arguments(u, EK_HIP_BATCH_NMAX, &nothing);
  if (rc) return rc;
  return bcheck::uniform_entry(u, nothing, host, u.problem ? (size_t)u.n * u.n : 0, false, launch_uniform);
}

static int variable_device_entry(int itype, int problem, int batch, const int *n, const double *const *dA,
                                 const int *lda, const double *const *dB, const int *ldb, const double *const *dw,
                                 const double *const *dZ, const int *ldz, const int *info, double *out,
                                 double *const *ipr, double *seconds, int nmax) {
  bool nothing;
  int rc = variable_check(problem, batch, n, (const void *const *)dA, lda, (const void *const *)dB, ldb,
                          (const void *const *)dw, (const void *const *)dZ, ldz, out, nmax, &nothing);
  if (rc) return rc;
  if (seconds) *seconds = 0.0;
  if (nothing) return 0;
  bool work = false;
  for (int b = 0; b < batch && !work; ++b) work = n[b] > 0 && !(info && info[b] != 0);
  if (work) {
    rc = ensure_init(); if (rc) return rc;
  }
  std::lock_guard<std::mutex> lk(g_mu);
  return variable_device_locked(itype, problem, batch, n, dA, lda, dB, ldb, dw, dZ, ldz, info, out, ipr, seconds);
}

static int variable_host_entry(int itype, int problem, int batch, const int *n, const double *const *A,
                               const int *lda, const double *const *B, const int *ldb, const double *const *w,
                               const double *const *Z, const int *ldz, const int *info, double *out,
                               double *const *ipr, double *seconds, int nmax) {
  bool nothing;
  int rc = variable_check(problem, batch, n, (const void *const *)A, lda, (const void *const *)B, ldb,
                          (const void *const *)w, (const void *const *)Z, ldz, out, nmax, &nothing);
  if (rc) return rc;
  if (seconds) *seconds = 0.0;
  if (nothing) return 0;
  // compact device layout (ld = n[b]), a problem behind the other; a skipped problem takes no room and is not read
  std::vector<size_t> offm((size_t)batch + 1, 0), offv((size_t)batch + 1, 0);
  for (int b = 0; b < batch; ++b) {
    const size_t k = (info && info[b] != 0) ? 0 : (size_t)n[b];
    offm[b + 1] = offm[b] + k * k;
    offv[b + 1] = offv[b] + k;
  }
  const size_t cm = offm[batch], cv = offv[batch];
  std::vector<const double *> pA((size_t)batch), pB((size_t)batch), pw((size_t)batch), pZ((size_t)batch);
  std::vector<int> ldc((size_t)batch);
  for (int b = 0; b < batch; ++b) ldc[b] = n[b] > 1 ? n[b] : 1;
  std::lock_guard<std::mutex> lk(g_mu);
  if (cm == 0)                                      // nothing to launch: the slots are filled on the host
    return variable_device_locked(itype, problem, batch, n, pA.data(), ldc.data(), pB.data(), ldc.data(), pw.data(),
                                  pZ.data(), ldc.data(), info, out, ipr, seconds);
  rc = ensure_init(); if (rc) return rc;
  hipStream_t s = g_ctx.stream;
  // one staging buffer per matrix kind: the lower triangles of A and B column by column (what lies above them is
  // never read), the columns of Z, w
  auto live = [&](int b) { return offm[b + 1] > offm[b]; };
  auto pack = [&](const double *const *M, const int *ld, bool lower, std::vector<double> &h) {
    h.assign(cm, 0.0);
    for (int b = 0; b < batch; ++b) {
      if (!live(b)) continue;
      for (int j = 0; j < n[b]; ++j) {
        const int i0 = lower ? j : 0;
        std::memcpy(&h[offm[b] + (size_t)j * n[b] + i0], M[b] + (size_t)j * ld[b] + i0, (size_t)(n[b] - i0) * 8);
      }
    }
  };
  std::vector<double> hA, hB, hZ, hw(cv);
  pack(A, lda, true, hA);
  if (problem) pack(B, ldb, true, hB);
  pack(Z, ldz, false, hZ);
  for (int b = 0; b < batch; ++b)
    if (live(b)) std::memcpy(&hw[offv[b]], w[b], (size_t)n[b] * 8);
  DevMem mem;
  double *uA = nullptr, *uB = nullptr, *uw = nullptr, *uZ = nullptr;
  rc = mem.alloc(&uA, cm * 8);
  if (!rc) rc = mem.alloc(&uw, cv * 8);
  if (!rc && problem) rc = mem.alloc(&uB, cm * 8);
  if (!rc) rc = mem.alloc(&uZ, cm * 8);
  if (rc) return rc;
  for (int b = 0; b < batch; ++b) {
    pA[b] = uA + offm[b];
    pB[b] = problem ? uB + offm[b] : nullptr;
    pw[b] = uw + offv[b];
    pZ[b] = uZ + offm[b];
  }
  EK_HIP_CHECK(hipMemcpyAsync(uA, hA.data(), cm * 8, hipMemcpyHostToDevice, s));
  if (problem) EK_HIP_CHECK(hipMemcpyAsync(uB, hB.data(), cm * 8, hipMemcpyHostToDevice, s));
  EK_HIP_CHECK(hipMemcpyAsync(uw, hw.data(), cv * 8, hipMemcpyHostToDevice, s));
  EK_HIP_CHECK(hipMemcpyAsync(uZ, hZ.data(), cm * 8, hipMemcpyHostToDevice, s));
  return variable_device_locked(itype, problem, batch, n, pA.data(), ldc.data(), pB.data(), ldc.data(), pw.data(),
                                pZ.data(), ldc.data(), info, out, ipr, seconds);
}

// ---- the variable window check (ek_hip_check_window_xvbatched*, ek_hip_check_sygv_window_xvbatched*): the
// window driver's count m[b] per problem on the variable driver's table.  One kernel class serves every order, so there are
// no classes here: one table by descending work, g_chunk entries a launch
static bool vwindow_skipped(const int *info, int b) { return info && info[b] != 0; }

// The argument errors in the order of the prototype (8 is m, 12 zcap, 13 info, 14 out).  sygv: `first` is itype (1 .. 3) and
// B is required for every type; otherwise it is problem (0, 1).  All arrays are host arrays of `batch` entries; m and info
// are read, the pointers in the pointer arrays are not dereferenced
static int vwindow_check(bool sygv, int first, int batch, const int *n, const void *const *A, const int *lda,
                         const void *const *B, const int *ldb, const int *m, const void *const *w, const void *const *Z,
                         const int *ldz, const int *zcap, const int *info, const double *out, bool *nothing) {
  *nothing = false;
  if (sygv ? (first < 1 || first > 3) : (first != 0 && first != 1)) return -1;
  if (batch < 0) return -2;
  if (batch == 0) { *nothing = true; return 0; }
  if (!n) return -3;
  for (int b = 0; b < batch; ++b)
    if (n[b] < 0 || n[b] > EK_HIP_XBATCH_NMAX) return -3;
  auto entries = [&](const void *const *P) {
    if (!P) return false;
    for (int b = 0; b < batch; ++b)
      if (n[b] > 0 && !P[b]) return false;
    return true;
  };
  auto leading = [&](const int *ld) {
    if (!ld) return false;
    for (int b = 0; b < batch; ++b)
      if (ld[b] < (n[b] > 1 ? n[b] : 1)) return false;
    return true;
  };
  if (!entries(A)) return -4;
  if (!leading(lda)) return -5;
  if (sygv || first == 1) {
    if (!entries(B)) return -6;
    if (!leading(ldb)) return -7;
  }
  if (!m) return -8;
  for (int b = 0; b < batch; ++b)
    if (!vwindow_skipped(info, b) && (m[b] < 0 || m[b] > n[b])) return -8;
  if (!entries(w)) return -9;
  if (!Z) return -10;
  if (zcap)                                         // the solver allows a NULL entry where zcap[b] = 0; a NULL zcap is -12
    for (int b = 0; b < batch; ++b)
      if (n[b] > 0 && zcap[b] > 0 && !Z[b]) return -10;
  if (!leading(ldz)) return -11;
  if (!zcap) return -12;
  for (int b = 0; b < batch; ++b)
    if (zcap[b] < 0 || (!vwindow_skipped(info, b) && zcap[b] < m[b])) return -12;
  if (!out) return -14;                             // 13 is info: NULL means every problem
  return 0;
}

// the problems to check (not skipped, m[b] > 0) in the order of execution: by descending estimated work -- n^2 m per
// product, n^3 / 3 for type 3's factor -- so that a launch ends on its cheapest problems; the bit contract makes the order
// invisible
static std::vector<int> vwindow_order(int itype, int batch, const int *n, const int *m, const int *info) {
  std::vector<int> order;
  for (int b = 0; b < batch; ++b)
    if (!vwindow_skipped(info, b) && m[b] > 0) order.push_back(b);
  auto work = [&](int b) {
    const long long nn = n[b];
    return nn * nn * m[b] + (itype == 3 ? nn * nn * nn / 3 : 0);
  };
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return work(x) > work(y); });
  return order;
}

// arguments checked, `order` not empty, context up, g_mu held; the pointers in dA, dB, dw, dZ are device addresses; itype: 0
// (`problem` says which), 2 or 3.  Entry e of the table belongs to chunk e / g_chunk and names its own slot of that chunk's
// scratch (prefix sums inside the chunk; the next chunk starts at the buffer's beginning): n m doubles for problem 1 and
// type 2, n^2 more for type 3 -- the layouts of the uniform kernels, which depend on (n, m) alone.  The launches follow one
// another on the context's stream, so they may share the buffer
static int vwindow_device_locked(int itype, int problem, int batch, const std::vector<int> &order, const int *n,
                                 const double *const *dA, const int *lda, const double *const *dB, const int *ldb,
                                 const int *m, const double *const *dw, const double *const *dZ, const int *ldz,
                                 const int *info, double *out, double *const *ipr, double *seconds) {
  using namespace bcheck;
  const size_t nout = (size_t)batch * EK_HIP_CHECK_NOUT;
  const int K = g_chunk, count = (int)order.size();
  auto slot = [&](int b) {
    const size_t nn = (size_t)n[b];
    return problem ? nn * (size_t)m[b] + (itype == 3 ? nn * nn : 0) : (size_t)0;
  };
  std::vector<size_t> off((size_t)batch, 0), offs((size_t)batch, 0);
  size_t words = nout, scratch = 0, chunk = 0;
  for (int e = 0; e < count; ++e) {
    const int b = order[e];
    if (ipr && ipr[b]) { off[b] = words; words += (size_t)m[b]; }
    if (e % K == 0) chunk = 0;                      // a chunk's first entry
    offs[b] = chunk;
    chunk += slot(b);
    scratch = std::max(scratch, chunk);
  }
  int rc = ensure(scratch, words, (size_t)count * sizeof(Desc));
  if (rc) return rc;
  g_htable.resize((size_t)count);
  for (int e = 0; e < count; ++e) {
    const int b = order[e];
    g_htable[e] = Desc{dA[b], problem ? dB[b] : nullptr, dw[b], dZ[b], problem ? g_scratch + offs[b] : nullptr,
                       (ipr && ipr[b]) ? g_dout + off[b] : nullptr, n[b], lda[b], problem ? ldb[b] : 1, ldz[b], b, m[b]};
  }
  rc = run_and_fetch(words, seconds, [&](hipStream_t s) -> int {
    EK_HIP_CHECK(hipMemcpyAsync(g_dtable, g_htable.data(), g_htable.size() * sizeof(Desc), hipMemcpyHostToDevice, s));
    for (int c0 = 0; c0 < count; c0 += K) {
      VArgs a{problem, (const Desc *)g_dtable + c0, g_dout};
      const int cnt = std::min(K, count - c0);
      const int rcl = itype ? launch_sygv_window_v(s, itype, cnt, a) : launch_window_v(s, cnt, a);
      if (rcl) return rcl;
    }
    return 0;
  });
  if (rc) return rc;
  const double *h = g_hout.data();
  for (int b = 0; b < batch; ++b) {
    double *o = out + (size_t)b * EK_HIP_CHECK_NOUT;
    if (vwindow_skipped(info, b) || m[b] == 0) {
      o[0] = o[1] = o[2] = o[3] = kNaN;
    } else {
      std::memcpy(o, h + (size_t)b * EK_HIP_CHECK_NOUT, EK_HIP_CHECK_NOUT * sizeof(double));
      if (ipr && ipr[b]) std::memcpy(ipr[b], h + off[b], (size_t)m[b] * sizeof(double));
    }
  }
  return 0;
}

// The four entries.  sygv: `first` is itype, and type 1 is the other family's problem 1 after this one's argument check.
// host: the pointers in A, B, w, Z are host addresses; the lower triangles of A and B, m[b] values of w and m[b] columns of
// Z of every problem to check go to a compact device image (ld = n[b]), one copy per matrix kind, as in
// variable_host_entry; nothing of a skipped or empty problem is staged
static int vwindow_entry(bool sygv, int first, int batch, const int *n, const double *const *A, const int *lda,
                         const double *const *B, const int *ldb, const int *m, const double *const *w,
                         const double *const *Z, const int *ldz, const int *zcap, const int *info, double *out,
                         double *const *ipr, double *seconds, bool host) {
  bool nothing;
  int rc = vwindow_check(sygv, first, batch, n, (const void *const *)A, lda, (const void *const *)B, ldb, m,
                         (const void *const *)w, (const void *const *)Z, ldz, zcap, info, out, &nothing);
  if (rc) return rc;
  if (sygv && first == 1)
    return host ? ek_hip_check_window_xvbatched(1, batch, n, A, lda, B, ldb, m, w, Z, ldz, zcap, info, out, ipr, seconds)
                : ek_hip_check_window_xvbatched_device(1, batch, n, A, lda, B, ldb, m, w, Z, ldz, zcap, info, out, ipr,
                                                       seconds);
  const int itype = sygv ? first : 0, problem = sygv ? 1 : first;
  if (seconds) *seconds = 0.0;
  if (nothing) return 0;
  const std::vector<int> order = vwindow_order(itype, batch, n, m, info);
  if (order.empty()) {                              // nothing to check: no context, no device
    for (size_t k = 0; k < (size_t)batch * EK_HIP_CHECK_NOUT; ++k) out[k] = kNaN;
    return 0;
  }
  rc = ensure_init(); if (rc) return rc;
  std::lock_guard<std::mutex> lk(g_mu);
  if (!host)
    return vwindow_device_locked(itype, problem, batch, order, n, A, lda, B, ldb, m, w, Z, ldz, info, out, ipr, seconds);
  hipStream_t s = g_ctx.stream;
  std::vector<size_t> offm((size_t)batch, 0), offz((size_t)batch, 0), offv((size_t)batch, 0);
  size_t cm = 0, cz = 0, cv = 0;
  for (int b : order) {
    offm[b] = cm; offz[b] = cz; offv[b] = cv;
    cm += (size_t)n[b] * n[b];
    cz += (size_t)n[b] * m[b];
    cv += (size_t)m[b];
  }
  auto pack = [&](const double *const *M, const int *ld, std::vector<double> &h) {   // the lower triangles
    h.assign(cm, 0.0);
    for (int b : order)
      for (int j = 0; j < n[b]; ++j)
        std::memcpy(&h[offm[b] + (size_t)j * n[b] + j], M[b] + (size_t)j * ld[b] + j, (size_t)(n[b] - j) * 8);
  };
  std::vector<double> hA, hB, hZ(cz), hw(cv);
  pack(A, lda, hA);
  if (problem) pack(B, ldb, hB);
  for (int b : order) {
    for (int j = 0; j < m[b]; ++j)
      std::memcpy(&hZ[offz[b] + (size_t)j * n[b]], Z[b] + (size_t)j * ldz[b], (size_t)n[b] * 8);
    std::memcpy(&hw[offv[b]], w[b], (size_t)m[b] * 8);
  }
  DevMem mem;
  double *uA = nullptr, *uB = nullptr, *uw = nullptr, *uZ = nullptr;
  rc = mem.alloc(&uA, cm * 8);
  if (!rc) rc = mem.alloc(&uw, cv * 8);
  if (!rc && problem) rc = mem.alloc(&uB, cm * 8);
  if (!rc) rc = mem.alloc(&uZ, cz * 8);
  if (rc) return rc;
  std::vector<const double *> pA((size_t)batch), pB((size_t)batch), pw((size_t)batch), pZ((size_t)batch);
  std::vector<int> ldc((size_t)batch);
  for (int b = 0; b < batch; ++b) ldc[b] = n[b] > 1 ? n[b] : 1;
  for (int b : order) {
    pA[b] = uA + offm[b];
    pB[b] = problem ? uB + offm[b] : nullptr;
    pw[b] = uw + offv[b];
    pZ[b] = uZ + offz[b];
  }
  EK_HIP_CHECK(hipMemcpyAsync(uA, hA.data(), cm * 8, hipMemcpyHostToDevice, s));
  if (problem) EK_HIP_CHECK(hipMemcpyAsync(uB, hB.data(), cm * 8, hipMemcpyHostToDevice, s));
  EK_HIP_CHECK(hipMemcpyAsync(uw, hw.data(), cv * 8, hipMemcpyHostToDevice, s));
  EK_HIP_CHECK(hipMemcpyAsync(uZ, hZ.data(), cz * 8, hipMemcpyHostToDevice, s));
  return vwindow_device_locked(itype, problem, batch, order, n, pA.data(), ldc.data(), pB.data(), ldc.data(), m, pw.data(),
                               pZ.data(), ldc.data(), info, out, ipr, seconds);
}

extern "C" {

int ek_hip_check_batched_device(int problem, int n, int batch, const double *dA, int lda, long long strideA,
                                const double *dB, int ldb, long long strideB, const double *dw, const double *dZ,
                                int ldz, long long strideZ, const int *info, double *out, double *ipr,
                                double *seconds) {
  return class_entry({0, problem, n, batch, dA, lda, strideA, dB, ldb, strideB, dw, dZ, ldz, strideZ, info, out, ipr, seconds},
                     false);
}

int ek_hip_check_batched(int problem, int n, int batch, const double *A, int lda, long long strideA, const double *B,
                         int ldb, long long strideB, const double *w, const double *Z, int ldz, long long strideZ,
                         const int *info, double *out, double *ipr, double *seconds) {
  return class_entry({0, problem, n, batch, A, lda, strideA, B, ldb, strideB, w, Z, ldz, strideZ, info, out, ipr, seconds},
                     true);
}

int ek_hip_check_vbatched_device(int problem, int batch, const int *n, const double *const *dA, const int *lda,
                                 const double *const *dB, const int *ldb, const double *const *dw,
                                 const double *const *dZ, const int *ldz, const int *info, double *out,
                                 double *const *ipr, double *seconds) {
  return variable_device_entry(0, problem, batch, n, dA, lda, dB, ldb, dw, dZ, ldz, info, out, ipr, seconds,
                               EK_HIP_BATCH_NMAX);
}

int ek_hip_check_vbatched(int problem, int batch, const int *n, const double *const *A, const int *lda,
                          const double *const *B, const int *ldb, const double *const *w, const double *const *Z,
                          const int *ldz, const int *info, double *out, double *const *ipr, double *seconds) {
  return variable_host_entry(0, problem, batch, n, A, lda, B, ldb, w, Z, ldz, info, out, ipr, seconds, EK_HIP_BATCH_NMAX);
}

// DSYGV's types: -1 for an itype outside 1 .. 3, then the family above with problem = 1 (type 1 is that problem itself)
int ek_hip_check_sygv_batched_device(int itype, int n, int batch, const double *dA, int lda, long long strideA,
                                     const double *dB, int ldb, long long strideB, const double *dw, const double *dZ,
                                     int ldz, long long strideZ, const int *info, double *out, double *ipr,
                                     double *seconds) {
  if (itype < 1 || itype > 3) return -1;
  return class_entry({itype == 1 ? 0 : itype, 1, n, batch, dA, lda, strideA, dB, ldb, strideB, dw, dZ, ldz, strideZ, info,
                      out, ipr, seconds}, false);
}

int ek_hip_check_sygv_batched(int itype, int n, int batch, const double *A, int lda, long long strideA, const double *B,
                              int ldb, long long strideB, const double *w, const double *Z, int ldz, long long strideZ,
                              const int *info, double *out, double *ipr, double *seconds) {
  if (itype < 1 || itype > 3) return -1;
  return class_entry({itype == 1 ? 0 : itype, 1, n, batch, A, lda, strideA, B, ldb, strideB, w, Z, ldz, strideZ, info, out,
                      ipr, seconds}, true);
}

int ek_hip_check_sygv_vbatched_device(int itype, int batch, const int *n, const double *const *dA, const int *lda,
                                      const double *const *dB, const int *ldb, const double *const *dw,
                                      const double *const *dZ, const int *ldz, const int *info, double *out,
                                      double *const *ipr, double *seconds) {
  if (itype < 1 || itype > 3) return -1;
  return variable_device_entry(itype == 1 ? 0 : itype, 1, batch, n, dA, lda, dB, ldb, dw, dZ, ldz, info, out, ipr,
                               seconds, EK_HIP_BATCH_NMAX);
}

int ek_hip_check_sygv_vbatched(int itype, int batch, const int *n, const double *const *A, const int *lda,
                               const double *const *B, const int *ldb, const double *const *w, const double *const *Z,
                               const int *ldz, const int *info, double *out, double *const *ipr, double *seconds) {
  if (itype < 1 || itype > 3) return -1;
  return variable_host_entry(itype == 1 ? 0 : itype, 1, batch, n, A, lda, B, ldb, w, Z, ldz, info, out, ipr, seconds,
                             EK_HIP_BATCH_NMAX);
}

// The variable forms for orders up to EK_HIP_XBATCH_NMAX: the entries above with the larger bound; the
// driver puts the orders above EK_HIP_BATCH_NMAX into a class of their own
int ek_hip_check_xvbatched_device(int problem, int batch, const int *n, const double *const *dA, const int *lda,
                                  const double *const *dB, const int *ldb, const double *const *dw,
                                  const double *const *dZ, const int *ldz, const int *info, double *out,
                                  double *const *ipr, double *seconds) {
  return variable_device_entry(0, problem, batch, n, dA, lda, dB, ldb, dw, dZ, ldz, info, out, ipr, seconds,
                               EK_HIP_XBATCH_NMAX);
}

int ek_hip_check_xvbatched(int problem, int batch, const int *n, const double *const *A, const int *lda,
                           const double *const *B, const int *ldb, const double *const *w, const double *const *Z,
                           const int *ldz, const int *info, double *out, double *const *ipr, double *seconds) {
  return variable_host_entry(0, problem, batch, n, A, lda, B, ldb, w, Z, ldz, info, out, ipr, seconds, EK_HIP_XBATCH_NMAX);
}

int ek_hip_check_sygv_xvbatched_device(int itype, int batch, const int *n, const double *const *dA, const int *lda,
                                       const double *const *dB, const int *ldb, const double *const *dw,
                                       const double *const *dZ, const int *ldz, const int *info, double *out,
                                       double *const *ipr, double *seconds) {
  if (itype < 1 || itype > 3) return -1;
  return variable_device_entry(itype == 1 ? 0 : itype, 1, batch, n, dA, lda, dB, ldb, dw, dZ, ldz, info, out, ipr,
                               seconds, EK_HIP_XBATCH_NMAX);
}

int ek_hip_check_sygv_xvbatched(int itype, int batch, const int *n, const double *const *A, const int *lda,
                                const double *const *B, const int *ldb, const double *const *w, const double *const *Z,
                                const int *ldz, const int *info, double *out, double *const *ipr, double *seconds) {
  if (itype < 1 || itype > 3) return -1;
  return variable_host_entry(itype == 1 ? 0 : itype, 1, batch, n, A, lda, B, ldb, w, Z, ldz, info, out, ipr, seconds,
                             EK_HIP_XBATCH_NMAX);
}

// The variable window checks: what ek_hip_eigenpairs_window_xvbatched* and ek_hip_sygv_window_xvbatched*
// return, m[b] columns of an n[b] x zcap[b] array per problem, in one call
int ek_hip_check_window_xvbatched_device(int problem, int batch, const int *n, const double *const *dA, const int *lda,
                                         const double *const *dB, const int *ldb, const int *m, const double *const *dw,
                                         const double *const *dZ, const int *ldz, const int *zcap, const int *info,
                                         double *out, double *const *ipr, double *seconds) {
  return vwindow_entry(false, problem, batch, n, dA, lda, dB, ldb, m, dw, dZ, ldz, zcap, info, out, ipr, seconds, false);
}

int ek_hip_check_window_xvbatched(int problem, int batch, const int *n, const double *const *A, const int *lda,
                                  const double *const *B, const int *ldb, const int *m, const double *const *w,
                                  const double *const *Z, const int *ldz, const int *zcap, const int *info, double *out,
                                  double *const *ipr, double *seconds) {
  return vwindow_entry(false, problem, batch, n, A, lda, B, ldb, m, w, Z, ldz, zcap, info, out, ipr, seconds, true);
}

int ek_hip_check_sygv_window_xvbatched_device(int itype, int batch, const int *n, const double *const *dA, const int *lda,
                                              const double *const *dB, const int *ldb, const int *m,
                                              const double *const *dw, const double *const *dZ, const int *ldz,
                                              const int *zcap, const int *info, double *out, double *const *ipr,
                                              double *seconds) {
  return vwindow_entry(true, itype, batch, n, dA, lda, dB, ldb, m, dw, dZ, ldz, zcap, info, out, ipr, seconds, false);
}

int ek_hip_check_sygv_window_xvbatched(int itype, int batch, const int *n, const double *const *A, const int *lda,
                                       const double *const *B, const int *ldb, const int *m, const double *const *w,
                                       const double *const *Z, const int *ldz, const int *zcap, const int *info,
                                       double *out, double *const *ipr, double *seconds) {
  return vwindow_entry(true, itype, batch, n, A, lda, B, ldb, m, w, Z, ldz, zcap, info, out, ipr, seconds, true);
}

// the classes of the last variable-order check that was given `seconds` (include/ek_hip_debug.h)
int ek_hip_debug_check_xvbatched_last(double *class_seconds, int *class_count) {
  std::lock_guard<std::mutex> lk(g_mu);
  for (int k = 0; k < bcheck::kClasses; ++k) {      // classes of 256, 128, 64, 32
    if (class_seconds) class_seconds[k] = bcheck::g_class_seconds[k];
    if (class_count) class_count[k] = bcheck::g_class_count[k];
  }
  return 0;
}

// the problems per launch above EK_HIP_BATCH_NMAX (include/ek_hip_debug.h)
int ek_hip_debug_check_xbatched_chunk(int problems) {
  std::lock_guard<std::mutex> lk(g_mu);
  const int before = bcheck::g_chunk;
  bcheck::g_chunk = problems > 0 ? problems : bcheck::kChunk;
  return before;
}

}  // extern "C"
