// ek_batched.hip -- ek_hip_eigenpairs_batched*: many small problems (order <= EK_HIP_BATCH_NMAX) in ONE launch.
//
// One workgroup owns a problem from its first load to its last store, and the matrix it works on lives in LDS the
// whole time: there is no launch and no host synchronise between the stages.  block_reduce, stage 0 and
// the rank sort are those of ek_batched_stages.h, which ek_batched_x.hip uses too.
//
//   0  scan_a: A's lower triangle is read once for NaN / Inf (info -5) and for max|a|: outside 2^-256 .. 2^256 the image
//      of stage 2 is A times an exact power of two, and d, e, w go out multiplied back
//   1  B's lower triangle -> LDS, right-looking Cholesky in LDS, L -> dB (lower triangle); a pivot that is not
//      positive (or outside 1e-290 .. 1e290, or NaN) ends the problem with info = its 1-based index
//   2  A's lower triangle -> LDS as a full symmetric image; X = L^-1 A (a thread per column), C = X L^-T (a thread
//      per row, lower half, then mirrored).  L is read back from dB, a column per step, staged through LDS one step
//      ahead: at order 128 the image (129 KiB) leaves no room for a second one
//   3  unblocked Householder tridiagonalisation of the image (DSYTD2, lower): d, e and the reflectors' tails go to
//      dA's lower triangle as LAPACK lays them out; tau stays in LDS (tau_k = 2 / (1 + |tail_k|^2) restores it)
//   4  implicit QL on (d, e), scaled by a power of two and taken upside down when d[0] outweighs d[n-1]: lane 0
//      runs a sweep's rotation chain and leaves (c, s) in LDS, then every thread applies the sweep to the row of Z it
//      owns -- dc_leaf_kernel's arithmetic with the barriers taken out of the chain; rank sort, w -> dw
//   5  Z <- Q Z (reflector tails read back from dA, staged like L), Z <- L^-T Z, columns stored in ascending order
//
// ek_hip_sygv_batched*: DSYGV's problem types 2 and 3 (A B x = l x, B A x = l x) differ from type 1 in two stages only.
//   2  C = L^T A L, in place in the image: X = A L (a thread pair per row: X[t, j] = sum_{k >= j} A[t, k] L[k, j] for
//      ascending j reads columns >= j of its own row, which are still A), then C = L^T X, lower half (a thread pair per
//      column: C[i, t] = sum_{k >= i} L[k, i] X[k, t] for ascending i reads rows >= i of its own column), then the
//      mirror.  The two threads of a pair take every other term and the two partial sums are added in one order
//   5  type 2 keeps Z <- L^-T Z; type 3 runs Z <- L Z (a thread per column, the columns of L in descending order)
// Everything between works on C unchanged, so the two types return the same w and leave the same image in dA, and
// itype 1 is problem 1.  The two types have an instantiation of their own (CONG), so that the kernel of the standard
// problem and of type 1 holds nothing of them.  Scaling of A is stage 0's; what is amplified here is lambda_max(B),
// not 1 / lambda_min(B).
//
// ek_hip_eigenpairs_window_batched*: a window of eigenpairs (RANGE 'I' / 'V') per problem.  A third argument type, WArgs,
// selects stage 4W of ek_batched_window.h in place of stage 4's QL -- Sturm bisection of the wanted values, inverse
// iteration for their vectors -- and stage 5 then runs on the window's columns only.  Stages 0 to 3 are
// the same lines for every argument type, and the instantiations of Args and VArgs hold nothing of the window.
// ek_hip_sygv_window_batched*: the same with itype.  Types 2 and 3 run WArgs with CONG: stages 0 to 3 are CONG's, stage 4W
// is the window's, and type 3's Z <- L Z (multiply_window_by_l) works on the window's columns alone.
//
// Image layout: column-major with leading dimension NC + 1 (odd), NC the class size 32 / 64 / 128.  A wave that walks
// down a column (consecutive rows) and a wave that walks along a row (stride NC + 1, odd) both hit 32 different
// 64-bit banks per 32 lanes.  Threads: T = 2 NC; thread t is (row or column t % NC, half t / NC).
//
// Same bits wherever a problem sits: a problem's arithmetic depends on (n, A, B) alone -- fixed loop orders, sums
// across a workgroup by a fixed butterfly and a fixed order over the waves, no atomics, one code path per class.
//
// ek_hip_eigenpairs_vbatched*: the same kernel for problems of different orders.  A workgroup then finds its problem in
// a table instead of at blockIdx.x * stride; every problem runs in the class its own order picks (the uniform call's
// bits), the classes as one launch each, the problems of a class in descending order.
//
// ek_hip_eigenpairs_window_xvbatched*, ek_hip_sygv_window_xvbatched*: a window per problem for problems of different orders.
// A fourth argument type, VWArgs: the table form, and beside the problem's entry an entry of a second table with its
// window and the place of its LU slot.  Stages 0 to 3 are the table kernels' lines, stage 4W and stage 5 the window
// kernels'; the host side (classes, launches by count and by LU budget, a region of the LU workspace per class) is
// run_variable_window below, for ek_batched_x.hip's class too.
//
// The host side of all these entries is one driver: an entry fills a UniformCall or a VariableCall, entry()
// checks it and takes the lock, stage() makes device copies for the host-pointer forms, run() issues the launches.
#include "ek_batched_stages.h"
#include "ek_batched_window.h"

#include <algorithm>
#include <type_traits>

namespace ek {
namespace batched {
using namespace bstages;

struct Args {
  int problem, jobz, n;
  double *A; int lda; long long sA;
  double *B; int ldb; long long sB;
  double *w;
  double *Z; int ldz; long long sZ;
  int *info;
  int itype;                                        // 1 / 2 / 3 as DSYGV's, looked at when problem == 1; last, so that
};                                                  // what the kernel of type 1 loads lies where it always lay

// ek_hip_eigenpairs_vbatched*: problems of different orders in one call.  A workgroup finds its problem in a table of
// Desc (ek_api_internal.h).
struct VArgs {
  int problem, jobz;
  const Desc *table;
  int *info;
  int itype;
};

// ek_hip_eigenpairs_window_batched*: Args and the window.  The type is what selects stage 4W (ek_batched_window.h) in
// place of the QL of stage 4: the instantiations of Args and VArgs hold nothing of it.
struct WArgs : Args {
  bwindow::Window win;
};

// ek_hip_eigenpairs_window_xvbatched*: VArgs and a window per problem.  Entry blockIdx.x of `wtable` lies beside entry
// blockIdx.x of `table`; the count goes to m[entry.index] as the status word goes to info[entry.index], and the LU slot
// starts at ws + wtable[blockIdx.x].lu.  Selects stage 4W like WArgs
struct VWArgs {
  int problem, jobz;
  const Desc *table;
  const bwindow::WDesc *wtable;
  int *info;
  int *m;
  double *ws;
  int range, itype;
};

// What a workgroup works on, whichever way it found it.  The pointers are typed as global (gdouble, ek_batched_stages.h)
struct Problem {
  int n;
  gdouble *A; int lda;
  gdouble *B; int ldb;
  gdouble *w;
  gdouble *Z; int ldz;
  int *info;
};
__device__ __forceinline__ Problem locate(const Args &a) {
  const long long pb = blockIdx.x;
  return {a.n, (gdouble *)(a.A + pb * a.sA), a.lda, a.problem ? (gdouble *)(a.B + pb * a.sB) : nullptr, a.ldb,
          (gdouble *)(a.w + pb * a.n), a.jobz ? (gdouble *)(a.Z + pb * a.sZ) : nullptr, a.ldz, a.info + pb};
}
__device__ __forceinline__ Problem locate(const VArgs &a) {
  const Desc &d = a.table[blockIdx.x];
  return {d.n, (gdouble *)d.A, d.lda, (gdouble *)d.B, d.ldb, (gdouble *)d.w, (gdouble *)d.Z, d.ldz, a.info + d.index};
}
__device__ __forceinline__ Problem locate(const VWArgs &a) {
  const Desc &d = a.table[blockIdx.x];
  return {d.n, (gdouble *)d.A, d.lda, (gdouble *)d.B, d.ldb, (gdouble *)d.w, (gdouble *)d.Z, d.ldz, a.info + d.index};
}
// the window of stage 4W: the call's, or the workgroup's own
__device__ __forceinline__ const bwindow::Window &window(const WArgs &a) { return a.win; }
__device__ __forceinline__ bwindow::OwnWindow window(const VWArgs &a) {
  return bwindow::own_window(a.range, a.wtable[blockIdx.x], a.m + a.table[blockIdx.x].index, a.ws);
}

// y[i * SY] -= a * x[i] for i0 <= i < i1, x and y in LDS: four elements' loads go out before the first store, so that
// a thread pays the LDS latency once per four elements and not once per element.
template <int SY>
__device__ __forceinline__ void lds_axpy(double *y, const double *x, double a, int i0, int i1) {
  int i = i0;
  for (; i + 4 <= i1; i += 4) {
    const double y0 = y[i * SY], y1 = y[(i + 1) * SY], y2 = y[(i + 2) * SY], y3 = y[(i + 3) * SY];
    const double x0 = x[i], x1 = x[i + 1], x2 = x[i + 2], x3 = x[i + 3];
    y[i * SY] = y0 - x0 * a;
    y[(i + 1) * SY] = y1 - x1 * a;
    y[(i + 2) * SY] = y2 - x2 * a;
    y[(i + 3) * SY] = y3 - x3 * a;
  }
  for (; i < i1; ++i) y[i * SY] -= x[i] * a;
}

// sum of x[k * SX] * l[k] over k = k0, k0 + 2, ... < n, in that order: four elements' loads go out before the first
// multiply-add (lds_axpy's reason)
template <int SX>
__device__ __forceinline__ double lds_dot2(const double *x, const double *l, int k0, int n) {
  double acc = 0.0;
  int k = k0;
  for (; k + 6 < n; k += 8) {
    const double x0 = x[k * SX], x1 = x[(k + 2) * SX], x2 = x[(k + 4) * SX], x3 = x[(k + 6) * SX];
    const double l0 = l[k], l1 = l[k + 2], l2 = l[k + 4], l3 = l[k + 6];
    acc += x0 * l0;
    acc += x1 * l1;
    acc += x2 * l2;
    acc += x3 * l3;
  }
  for (; k < n; k += 2) acc += x[k * SX] * l[k];
  return acc;
}

// Types 2 and 3, stage 2: the image A (full, symmetric) becomes C = L^T A L (lower half), in place.  L comes back from
// dB a column per step through the two sl vectors, as in type 1's solves.  Thread (r, sub) sums the terms k = j + sub,
// j + sub + 2, ...; the partial sums meet in sq (2 x 2 NC doubles, the halves alternating between steps, so that a
// step needs one barrier) and are added as sub 0's plus sub 1's: the order of every sum depends on n alone.
template <int NC>
__device__ __forceinline__ void congruence_in_image(double *S, double *sl, double *sq, const gdouble *B, int ldb,
                                                    int n) {
  constexpr int LD = NC + 1;
  const int t = threadIdx.x, r = t % NC, sub = t / NC;
  const bool row = r < n;
  if (t < n) sl[t] = B[t];                          // column 0 of L
  __syncthreads();
  // X = A L: the pair r owns row r.  Step j reads columns >= j of the row, which are still A, and leaves X[r, j]
  for (int j = 0; j < n; ++j) {
    const double *cur = sl + (j & 1) * NC;
    double *q = sq + (j & 1) * 2 * NC;
    double nx = 0.0;
    if (j + 1 < n && t > j && t < n) nx = B[t + (size_t)(j + 1) * ldb];
    if (row) q[sub * NC + r] = lds_dot2<LD>(S + r, cur, j + sub, n);
    if (t < n) sl[((j + 1) & 1) * NC + t] = nx;
    __syncthreads();
    if (sub == 0 && row) S[r + j * LD] = q[r] + q[NC + r];
  }
  if (t < n) sl[t] = B[t];
  __syncthreads();
  // C = L^T X, lower half: the pair r owns column r.  Step i reads rows >= i of the column and leaves C[i, r]
  for (int i = 0; i < n; ++i) {
    const double *cur = sl + (i & 1) * NC;
    double *q = sq + (i & 1) * 2 * NC;
    double nx = 0.0;
    if (i + 1 < n && t > i && t < n) nx = B[t + (size_t)(i + 1) * ldb];
    if (row && r <= i) q[sub * NC + r] = lds_dot2<1>(S + r * LD, cur, i + sub, n);
    if (t < n) sl[((i + 1) & 1) * NC + t] = nx;
    __syncthreads();
    if (sub == 0 && row && r <= i) S[i + r * LD] = q[r] + q[NC + r];
  }
  __syncthreads();                                  // the mirror reads rows that other threads wrote
}

// Type 3, stage 5: Z <- L Z, thread t owns column t of Z.  For k = n-1 .. 0: z[i] += L[i, k] z[k] for i > k, then
// z[k] *= L[k, k]; column k of L is staged like the reflectors.
template <int NC>
__device__ __forceinline__ void multiply_by_l(double *S, double *sl, const gdouble *B, int ldb, int n) {
  constexpr int LD = NC + 1;
  const int t = threadIdx.x;
  if (t < n) sl[t] = (t == n - 1) ? B[t + (size_t)(n - 1) * ldb] : 0.0;
  __syncthreads();
  for (int k = n - 1, s = 0; k >= 0; --k, ++s) {
    const double *cur = sl + (s & 1) * NC;
    double nx = 0.0;
    if (k >= 1 && t >= k - 1 && t < n) nx = B[t + (size_t)(k - 1) * ldb];
    if (t < n) {
      double *col = S + t * LD;
      const double zk = col[k];
      lds_axpy<1>(col, cur, -zk, k + 1, n);         // y - x (-zk): the sign change is exact
      col[k] = zk * cur[k];
    }
    if (t < n) sl[((s + 1) & 1) * NC + t] = nx;
    __syncthreads();
  }
}

// The same for the window kernel: the nz wanted vectors are the columns t < nz; the columns behind them hold leftovers of
// stage 3 and are not touched.  Every t < n stages L as above, and a column sees the same steps in the same order.
template <int NC>
__device__ __forceinline__ void multiply_window_by_l(double *S, double *sl, const gdouble *B, int ldb, int n, int nz) {
  constexpr int LD = NC + 1;
  const int t = threadIdx.x;
  if (t < n) sl[t] = (t == n - 1) ? B[t + (size_t)(n - 1) * ldb] : 0.0;
  __syncthreads();
  for (int k = n - 1, s = 0; k >= 0; --k, ++s) {
    const double *cur = sl + (s & 1) * NC;
    double nx = 0.0;
    if (k >= 1 && t >= k - 1 && t < n) nx = B[t + (size_t)(k - 1) * ldb];
    if (t < nz) {
      double *col = S + t * LD;
      const double zk = col[k];
      lds_axpy<1>(col, cur, -zk, k + 1, n);
      col[k] = zk * cur[k];
    }
    if (t < n) sl[((s + 1) & 1) * NC + t] = nx;
    __syncthreads();
  }
}

// ARGS: how the workgroup finds its problem -- Args (one order, strided: blockIdx.x * stride) or VArgs (a table entry);
// WArgs and VWArgs are the two with a window
// CONG: the instantiation for types 2 and 3 (C = L^T A L; the host picks it when problem == 1 and itype != 1).  With
// CONG = false nothing of those types is compiled in: the standard problem and type 1 run the code they always ran.
// WIN (ARGS = WArgs or VWArgs): stage 4W for QL, and stage 5 on the window's columns.
template <int NC, int T, typename ARGS = Args, bool CONG = false>
__global__ __launch_bounds__(T) void batched_kernel(ARGS a) {
  constexpr int LD = NC + 1, P = T / NC, NW = T / 64;
  constexpr bool VWIN = std::is_same<ARGS, VWArgs>::value;
  constexpr bool WIN = VWIN || std::is_same<ARGS, WArgs>::value;
  static_assert(P == 2 && T % 64 == 0, "two threads per row");
  extern __shared__ double smem[];
  double *S = smem;                       // NC x NC image, leading dimension LD
  double *sd = S + NC * LD;               // d, e, tau: alive from stage 3 to the end
  double *se = sd + NC, *st = se + NC;
  double *sv = st + NC, *sw = sv + NC;    // stage 3: v, w;  stage 4: c, s of a sweep
  double *sp = sw + NC;                   // stage 3: P x NC partial sums of the symv
  double *sl = sp + P * NC;               // 2 x NC: a column of L or a reflector, and the next one
  __shared__ double red[2 * (NW > 1 ? NW : 1)];
  __shared__ int srank[NC];
  __shared__ int s_state, s_m, s_lo;

  const Problem p = locate(a);
  const int t = threadIdx.x, n = p.n;
  const int r = t % NC, sub = t / NC;
  const bool row = r < n;
  gdouble *A = p.A;
  gdouble *B = p.B;
  const int lda = p.lda, ldb = p.ldb;
  int *info = p.info;
  int phase = 0;

  // ---- 0: A finite?  max|a|: the image holds 2^-aex A; d, e and w go out times 2^aex
  int aex;
  if (!scan_a<NC, NW>(A, lda, n, red, phase, info, aex)) return;

  if (a.problem) {
    // ---- 1: B = L L^T in the image
    if (row)
      for (int j = sub; j <= r; j += P) S[r + j * LD] = B[r + (size_t)j * ldb];
    __syncthreads();
    for (int j = 0; j < n; ++j) {
      const double piv = S[j + j * LD];             // read by all after a barrier: the exit is uniform
      if (!(piv > 1e-290) || !(piv < 1e290)) {      // chol64_upper_wg's rule: ek_hip_solve_device's info
        if (t == 0) *info = j + 1;
        return;
      }
      const double l = sqrt(piv);                   // the image keeps the pivot; the diagonal of L is formed on the way out
      if (sub == 0 && row && r > j) S[r + j * LD] = S[r + j * LD] / l;
      __syncthreads();
      if (row && r > j) {
        const double lr = S[r + j * LD];
        for (int k = j + 1 + sub; k <= r; k += P) S[r + k * LD] -= lr * S[k + j * LD];
      }
      __syncthreads();
    }
    if (row)
      for (int j = sub; j <= r; j += P) B[r + (size_t)j * ldb] = (r == j) ? sqrt(S[j + j * LD]) : S[r + j * LD];
    __syncthreads();                                // L is in dB for the whole workgroup; the image is free
  }

  // ---- 2: A -> full symmetric image; C = L^-1 A L^-T (type 1), C = L^T A L (types 2 and 3)
  if (row)
    for (int j = sub; j <= r; j += P) {
      const double x = ldexp(A[r + (size_t)j * lda], -aex);   // exact; aex = 0 leaves the bits alone
      S[r + j * LD] = x;
      S[j + r * LD] = x;
    }
  if (CONG) {
    congruence_in_image<NC>(S, sl, sv, B, ldb, n);  // sv, sw, sp: 4 NC doubles, free until stage 3
    if (row)
      for (int j = sub; j < r; j += P) S[j + r * LD] = S[r + j * LD];
  } else if (a.problem) {
    if (t < n) sl[t] = B[t];                        // column 0 of L
    __syncthreads();
    // X = L^-1 A: thread t owns column t of the image
    for (int k = 0; k < n; ++k) {
      const double *cur = sl + (k & 1) * NC;
      double nx = 0.0;
      if (k + 1 < n && t > k && t < n) nx = B[t + (size_t)(k + 1) * ldb];
      if (t < n) {
        double *col = S + t * LD;
        const double xk = col[k] / cur[k];
        col[k] = xk;
        lds_axpy<1>(col, cur, xk, k + 1, n);
      }
      if (t < n) sl[((k + 1) & 1) * NC + t] = nx;
      __syncthreads();
    }
    if (t < n) sl[t] = B[t];
    __syncthreads();
    // C = X L^-T, lower half: thread t owns row t of the image, columns 0..t
    for (int k = 0; k < n; ++k) {
      const double *cur = sl + (k & 1) * NC;
      double nx = 0.0;
      if (k + 1 < n && t > k && t < n) nx = B[t + (size_t)(k + 1) * ldb];
      if (t < n && k <= t) {
        const double ck = S[t + k * LD] / cur[k];
        S[t + k * LD] = ck;
        lds_axpy<LD>(S + t, cur, ck, k + 1, t + 1);
      }
      if (t < n) sl[((k + 1) & 1) * NC + t] = nx;
      __syncthreads();
    }
    if (row)
      for (int j = sub; j < r; j += P) S[j + r * LD] = S[r + j * LD];
  }
  __syncthreads();

  // ---- 3: Householder tridiagonalisation of the image (both triangles kept, bitwise symmetric)
  for (int k = 0; k + 1 < n; ++k) {
    double x = 0.0;
    if (sub == 0 && row && r >= k + 2) x = S[r + k * LD];
    const double xn2 = block_reduce<NW, false>(x * x, red, phase);
    const double alpha = S[k + 1 + k * LD], dk = S[k + k * LD];
    double tau = 0.0, beta = alpha, scal = 0.0;
    if (xn2 != 0.0) {
      beta = -copysign(sqrt(alpha * alpha + xn2), alpha);
      tau = (beta - alpha) / beta;
      scal = 1.0 / (alpha - beta);
    }
    if (sub == 0 && row) {
      if (r >= k + 2) {
        const double vi = x * scal;
        sv[r] = vi;
        A[r + (size_t)k * lda] = vi;
      } else if (r == k + 1) {
        sv[r] = 1.0;
        se[k] = beta;
        st[k] = tau;
        A[r + (size_t)k * lda] = ldexp(beta, aex);   // d and e of the caller's A
      } else if (r == k) {
        sd[k] = dk;
        A[k + (size_t)k * lda] = ldexp(dk, aex);
      }
    }
    if (tau == 0.0) continue;                       // H = I (uniform: tau has the same bits in every thread)
    __syncthreads();
    if (row && r > k) {                             // p = C v, the columns split between the two halves
      double acc = 0.0;
      for (int j = k + 1 + sub; j < n; j += P) acc += S[r + j * LD] * sv[j];
      sp[sub * NC + r] = acc;
    }
    __syncthreads();
    double pr = 0.0, vr = 0.0;
    if (sub == 0 && row && r > k) {
      pr = tau * (sp[r] + sp[NC + r]);
      vr = sv[r];
    }
    const double dot = block_reduce<NW, false>(pr * vr, red, phase);
    const double al2 = -0.5 * tau * dot;
    if (sub == 0 && row && r > k) sw[r] = pr + al2 * vr;
    __syncthreads();
    if (row && r > k) {                             // C -= v w^T + w v^T; (r, j) and (j, r) evaluate the same expression
      const double vr2 = sv[r], wr2 = sw[r];
      auto term = [&](int j, double vj, double wj) {
        const bool up = j > r;
        const double vh = up ? vj : vr2, wh = up ? wj : wr2, vl = up ? vr2 : vj, wl = up ? wr2 : wj;
        return vh * wl + wh * vl;
      };
      int j = k + 1 + sub;
      for (; j + 3 * P < n; j += 4 * P) {             // four elements' loads before the first store
        double *c0 = S + r + j * LD;
        const double a0 = c0[0], a1 = c0[P * LD], a2 = c0[2 * P * LD], a3 = c0[3 * P * LD];
        const double v0 = sv[j], v1 = sv[j + P], v2 = sv[j + 2 * P], v3 = sv[j + 3 * P];
        const double w0 = sw[j], w1 = sw[j + P], w2 = sw[j + 2 * P], w3 = sw[j + 3 * P];
        c0[0] = a0 - term(j, v0, w0);
        c0[P * LD] = a1 - term(j + P, v1, w1);
        c0[2 * P * LD] = a2 - term(j + 2 * P, v2, w2);
        c0[3 * P * LD] = a3 - term(j + 3 * P, v3, w3);
      }
      for (; j < n; j += P) S[r + j * LD] -= term(j, sv[j], sw[j]);
    }
    __syncthreads();
  }
  if (t == 0) {
    const double dl = S[(n - 1) * (LD + 1)];
    sd[n - 1] = dl;
    se[n - 1] = 0.0;
    A[(size_t)(n - 1) * lda + (n - 1)] = ldexp(dl, aex);
  }
  __syncthreads();

  // ---- 4: implicit QL with Z in the image
  int wex = aex;                                    // w = 2^wex d: stage 0's scaling and the one below
  {
    double mx = 0.0;
    int bad = 0;
    if (sub == 0 && row) {
      mx = fmax(fabs(sd[r]), fabs(se[r]));
      bad = !(mx <= DBL_MAX);
    }
    if (__syncthreads_or(bad)) {                    // the reduction overflowed: a non-finite eigenvalue (k = n + 1)
      if (t == 0) *info = 100000 + n + 1;
      return;
    }
    const double anorm = block_reduce<NW, true>(mx, red, phase);
    if (anorm > 0.0) {
      int ex;
      (void)frexp(anorm, &ex);
      const double sc = ldexp(1.0, -ex);
      wex += ex;
      __syncthreads();
      if (sub == 0 && row) { sd[r] *= sc; se[r] *= sc; }
    }
  }
  __syncthreads();
  // QL converges fast towards a small top; a matrix graded the other way (rank one: everything in d[0]) is taken
  // upside down, T' = P T P, which QL sees as DSTEQR's QR sees T.  Z starts as P, so that Z' comes out as P Z'.
  const bool flip = !WIN && fabs(sd[0]) > fabs(sd[n - 1]);
  {
    double dr = 0.0, er = 0.0;
    if (flip && sub == 0 && row) {
      dr = sd[n - 1 - r];
      er = (r < n - 1) ? se[n - 2 - r] : 0.0;
    }
    __syncthreads();
    if (flip && sub == 0 && row) { sd[r] = dr; se[r] = er; }
  }
  if (!WIN && a.jobz && row)
    for (int j = sub; j < n; j += P) S[r + j * LD] = (r == (flip ? n - 1 - j : j)) ? 1.0 : 0.0;
  __syncthreads();
  if constexpr (!WIN) {
    const double eps = 1.1102230246251565e-16;
    double *sc_ = sv, *ss_ = sw;
    int failed = 0;
    int iter = 0;                                   // lane 0's: sweeps so far, 30 n in all as in DSTEQR
    for (int l = 0; l < n && !failed; ++l) {
      while (true) {
        if (t == 0) {
          int m = l;                                // the first negligible e from l on, eight tests per round of loads
          for (bool found = false; !found;) {
            double dv[9], ev[8];
#pragma unroll
            for (int q = 0; q < 9; ++q) dv[q] = sd[min(m + q, n - 1)];
#pragma unroll
            for (int q = 0; q < 8; ++q) ev[q] = se[min(m + q, n - 1)];
            int hit = -1;
#pragma unroll
            for (int q = 7; q >= 0; --q)
              if (m + q >= n - 1 || fabs(ev[q]) <= eps * (fabs(dv[q]) + fabs(dv[q + 1]))) hit = q;
            if (hit >= 0) { m = min(m + hit, n - 1); found = true; } else m += 8;
          }
          if (m == l) {
            s_state = 0;
          } else if (iter++ == 30 * n) {
            s_state = 2;
          } else {
            const double dl = sd[l], el = se[l];
            double g = (sd[l + 1] - dl) / (2.0 * el);
            double rr = sqrt(g * g + 1.0);
            g = sd[m] - dl + el / (g + copysign(rr, g));
            double s = 1.0, c = 1.0, p = 0.0;
            int i, lo = l;
            bool under = false;
            // d[i], e[i] are loaded one rotation ahead (no store of the chain touches them before their use), so
            // that the chain waits for arithmetic only
            double ei = se[m - 1], di = sd[m - 1], dup = sd[m];
            for (i = m - 1; i >= l; --i) {
              double en = 0.0, dn = 0.0;
              if (i > l) { en = se[i - 1]; dn = sd[i - 1]; }
              const double f = s * ei, bb = c * ei;
              const double h = f * f + g * g;
              if (!(h >= 1e-280)) {                 // recover from underflow (T has norm 1/2..1): split here
                se[i + 1] = 0.0;
                sd[i + 1] = dup - p;
                se[m] = 0.0;
                under = true;
                lo = i + 1;
                break;
              }
              // one lane works, but every instruction costs a whole wave's issue slot: 1 / sqrt(h) by the hardware's
              // seed and two Newton steps serves r, s and c at a third of the instructions of a square root and two
              // divisions (rounding: a few ulp in s and c, as DLARTG's own)
              double y = __builtin_amdgcn_rsq(h);
              y = y * (1.5 - 0.5 * h * y * y);
              y = y * (1.5 - 0.5 * h * y * y);
              rr = h * y;
              se[i + 1] = rr;
              s = f * y;
              c = g * y;
              g = dup - p;
              rr = (di - g) * s + 2.0 * c * bb;
              p = s * rr;
              sd[i + 1] = g + p;
              g = c * rr - bb;
              sc_[i] = c;
              ss_[i] = s;
              dup = di; di = dn; ei = en;
            }
            if (!under) {
              sd[l] = dup - p;
              se[l] = g;
              se[m] = 0.0;
            }
            s_state = 1; s_m = m; s_lo = lo;
          }
        }
        __syncthreads();
        const int state = s_state, m = s_m, lo = s_lo;
        if (state == 1 && a.jobz && t < n) {        // the sweep's rotations on row t of Z
          double *zr = S + t;
          double f = zr[m * LD];
          int i = m - 1;
          for (; i - 3 >= lo; i -= 4) {             // four rotations' loads before the first store
            const double z0 = zr[i * LD], z1 = zr[(i - 1) * LD], z2 = zr[(i - 2) * LD], z3 = zr[(i - 3) * LD];
            const double c0 = sc_[i], c1 = sc_[i - 1], c2 = sc_[i - 2], c3 = sc_[i - 3];
            const double s0 = ss_[i], s1 = ss_[i - 1], s2 = ss_[i - 2], s3 = ss_[i - 3];
            zr[(i + 1) * LD] = s0 * z0 + c0 * f; f = c0 * z0 - s0 * f;
            zr[i * LD] = s1 * z1 + c1 * f; f = c1 * z1 - s1 * f;
            zr[(i - 1) * LD] = s2 * z2 + c2 * f; f = c2 * z2 - s2 * f;
            zr[(i - 2) * LD] = s3 * z3 + c3 * f; f = c3 * z3 - s3 * f;
          }
          for (; i >= lo; --i) {
            const double c = sc_[i], s = ss_[i], z0 = zr[i * LD];
            zr[(i + 1) * LD] = s * z0 + c * f;
            f = c * z0 - s * f;
          }
          zr[lo * LD] = f;
        }
        __syncthreads();
        if (state == 2) failed = l + 1;
        if (state != 1) break;
      }
    }
    if (failed) {
      if (t == 0) *info = 100000 + failed;
      return;
    }
  }
  int nz = n;                                       // columns of Z: n, or the window's m
  if constexpr (WIN) {
    constexpr int OWNER = VWIN ? 2 + CONG : CONG;   // s_rounds: one variable per kernel
    if (!bwindow::stage4w<NC, NW, bwindow::ColumnsInLds, OWNER>(window(a), a.jobz, n, wex, S, sd, se, sv, sw, sp, sl, red,
                                                                phase, srank, p.w, info, nz))
      return;
  } else {
    if (!rank_sort<NC>(n, wex, sd, srank, p.w, info)) return;
  }
  if (!a.jobz) {
    if (t == 0) *info = 0;
    return;
  }
  gdouble *Z = p.Z;
  const int ldz = p.ldz;

  // ---- 5: Z <- H_0 ... H_{n-3} Z (H_{n-2} = I), thread t owns column t of Z
  if (n >= 3) {
    if (t < n) sl[t] = (t >= n - 1) ? A[t + (size_t)(n - 3) * lda] : 0.0;
    __syncthreads();
    for (int k = n - 3, s = 0; k >= 0; --k, ++s) {
      const double *cur = sl + (s & 1) * NC;
      double nx = 0.0;
      if (k >= 1 && t > k && t < n) nx = A[t + (size_t)(k - 1) * lda];
      const double tau = st[k];
      if (tau != 0.0 && t < nz) {
        double *col = S + t * LD;
        double dot = col[k + 1];
        for (int i = k + 2; i < n; ++i) dot += cur[i] * col[i];
        dot *= tau;
        col[k + 1] -= dot;
        lds_axpy<1>(col, cur, dot, k + 2, n);
      }
      if (t < n) sl[((s + 1) & 1) * NC + t] = nx;
      __syncthreads();
    }
  }
  // Z <- L^-T Z (types 1 and 2), Z <- L Z (type 3)
  if (CONG && a.itype == 3) {
    __syncthreads();
    if constexpr (WIN) multiply_window_by_l<NC>(S, sl, B, ldb, n, nz);
    else multiply_by_l<NC>(S, sl, B, ldb, n);
  } else if (a.problem) {
    __syncthreads();
    if (t < n) sl[t] = (t == n - 1) ? B[t + (size_t)(n - 1) * ldb] : 0.0;
    __syncthreads();
    for (int i = n - 1, s = 0; i >= 0; --i, ++s) {
      const double *cur = sl + (s & 1) * NC;
      double nx = 0.0;
      if (i >= 1 && t >= i - 1 && t < n) nx = B[t + (size_t)(i - 1) * ldb];
      if (t < nz) {
        double *col = S + t * LD;
        double acc = col[i];
        for (int k = i + 1; k < n; ++k) acc -= cur[k] * col[k];
        col[i] = acc / cur[i];
      }
      if (t < n) sl[((s + 1) & 1) * NC + t] = nx;
      __syncthreads();
    }
  }
  __syncthreads();
  if (row)
    for (int j = sub; j < nz; j += P) Z[r + (size_t)srank[j] * ldz] = S[r + j * LD];
  if (t == 0) *info = 0;
}

template <int NC, int T, typename ARGS, bool CONG>
static int launch_instance(hipStream_t s, int batch, const ARGS &a) {
  constexpr size_t lds = (size_t)(NC * (NC + 1) + 9 * NC) * sizeof(double);
  static bool raised = false;                       // one per instantiation, the variable ones and CONG's included
  if (lds > 64 * 1024 && !raised) {
    EK_HIP_CHECK(hipFuncSetAttribute((const void *)batched_kernel<NC, T, ARGS, CONG>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    raised = true;
  }
  hipLaunchKernelGGL((batched_kernel<NC, T, ARGS, CONG>), dim3(batch), dim3(T), lds, s, a);
  EK_HIP_CHECK(hipGetLastError());
  return 0;
}

template <int NC, int T, typename ARGS>
static int launch_class(hipStream_t s, int batch, const ARGS &a) {
  return (a.problem && a.itype != 1) ? launch_instance<NC, T, ARGS, true>(s, batch, a)
                                     : launch_instance<NC, T, ARGS, false>(s, batch, a);
}

// LDS bytes (dynamic part) and threads of the class that takes order n: host arithmetic for tools and DESIGN.md 12
static int class_of(int n) { return n <= 32 ? 32 : n <= 64 ? 64 : 128; }

// the one switch over the three classes of LDS: `count` workgroups of the class that takes order n
template <typename ARGS>
static int launch_order(int n, hipStream_t s, int count, const ARGS &a) {
  switch (class_of(n)) {
    case 32: return launch_class<32, 64>(s, count, a);
    case 64: return launch_class<64, 128>(s, count, a);
    default: return launch_class<128, 256>(s, count, a);
  }
}

// ---- the host driver of every entry family

// a device array that is grown, never shrunk, and released in ek_hip_finalize
template <typename T>
struct Pool {
  T *p = nullptr;
  size_t count = 0;
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    count = 0;
  }
  int grow(size_t need) {
    if (need <= count) return 0;
    release();
    EK_HIP_CHECK(hipMalloc((void **)&p, need * sizeof(T)));
    count = need;
    return 0;
  }
};
static Pool<int> g_dinfo;                           // per-problem status words
// the window entries: a count per problem, and the LU factors of inverse iteration -- one slot per workgroup of a
// launch, the batch running in chunks of g_wchunk problems that share the slots (the stream's order separates two users
// of a slot, as in ek_batched_x.hip)
static Pool<int> g_dm;
static Pool<double> g_wws;
// the variable forms' problem table and, for ek_hip_*_window_xvbatched*, the window table beside it; their host images are
// static because the asynchronous upload may still read them when an error returns
static Pool<Desc> g_dtable;
static Pool<WDesc> g_dwtable;
static std::vector<Desc> g_htable;
static std::vector<WDesc> g_hwtable;

constexpr int kWindowChunk = 1024;
constexpr size_t kWindowBytes = (size_t)256 << 20;
static int g_wchunk = kWindowChunk;
// ek_hip_eigenpairs_window_xbatched* above EK_HIP_BATCH_NMAX: ek_batched_x.hip's class keeps two workgroups on a compute
// unit, 512 on the device, and a slot of LU is up to 2.6 MB (n = c = 256): 1024 problems a launch, or as many slots as fit
// 1 GiB where that is fewer, in whole rounds of 512 and never under one round (ek_hip_debug_window_xbatched_chunk)
constexpr int kXWindowChunk = 1024, kXWindowRound = 512;
constexpr size_t kXWindowBytes = (size_t)1 << 30;
static int g_xwchunk = kXWindowChunk;
static long long g_vwbudget = 0;                    // LU bytes a launch may hold (ek_hip_debug_window_xvbatched_budget)

// the variable forms: the streams of the classes behind the largest one present (that one runs on the context's stream)
// and the events that tie them to it, kept like the pools
constexpr int kClasses = 4;                         // 256 (ek_batched_x.hip's kernel; ek_hip_*_xvbatched* only), 128, 64, 32
constexpr int kClassOrder[kClasses] = {EK_HIP_XBATCH_NMAX, 128, 64, 32};
static hipStream_t g_side[kClasses - 1] = {};
constexpr int kEvents = 3 * kClasses + 1;           // fork, joins, start / end of each class, end of the call
static hipEvent_t g_ev[kEvents] = {};
static int g_streams = 3;                           // 3: a stream per class; 1: one stream (ek_hip_debug_vbatched_streams)
static double g_class_seconds[kClasses] = {};       // the last timed variable call's kernels, by class
static int g_class_count[kClasses] = {};

static int create_event(hipEvent_t *e) {
  EK_HIP_CHECK(hipEventCreate(e));
  return 0;
}

}  // namespace batched

namespace api {
void release_batched() {
  using namespace batched;
  g_dinfo.release();
  g_dtable.release();
  g_dm.release();
  g_wws.release();
  g_dwtable.release();
  std::vector<Desc>().swap(g_htable);
  std::vector<WDesc>().swap(g_hwtable);
  for (int k = 0; k < kClasses - 1; ++k) {
    if (g_side[k]) (void)hipStreamDestroy(g_side[k]);
    g_side[k] = nullptr;
  }
  for (int k = 0; k < kEvents; ++k) {
    if (g_ev[k]) (void)hipEventDestroy(g_ev[k]);
    g_ev[k] = nullptr;
  }
}
}  // namespace api
}  // namespace ek

using namespace ek;
using namespace ek::api;
using namespace ek::batched;

// One call, as its extern "C" entry fills it: ek_hip_eigenpairs_* pass itype 1, ek_hip_sygv_* problem 1 (argument k of
// the one is argument k of the other).  A, B, w, Z are host or device arrays as the entry says and device arrays from
// run() on; everything else is the host's.  win: the window of the ek_hip_*_window_* entries, nullptr in the others
struct UniformWindow {
  int range;
  double vl, vu;
  int il, iu, zcap;
  int *m;
};
struct UniformCall {
  int problem, itype, jobz, n, batch;
  double *A; int lda; long long sA;
  double *B; int ldb; long long sB;
  double *w;
  double *Z; int ldz; long long sZ;
  int *info;
  double *seconds;
  const UniformWindow *win;
};
// the variable-order forms: host arrays of `batch` entries
struct VariableWindow {
  int range;
  const double *vl, *vu;
  const int *il, *iu, *zcap;
  int *m;
};
struct VariableCall {
  int problem, itype, jobz, batch;
  const int *n;
  double *const *A; const int *lda;
  double *const *B; const int *ldb;
  double *const *w;
  double *const *Z; const int *ldz;
  int *info;
  double *seconds;
  const VariableWindow *win;
};

// ---- argument checks: the arguments of the prototype in their order, every error the number include/ek_hip.h gives it;
// no data pointer is dereferenced, and the pointers in a pointer array are not either

// 0, or which of a matrix argument's three is wrong: 1 the pointer, 2 the leading dimension, 3 the stride
static int matrix_fault(const void *M, int ld, long long stride, int n) {
  if (!M) return 1;
  if (ld < n) return 2;
  if (stride < (long long)ld * n) return 3;
  return 0;
}

// the 22 checked arguments of a window entry
static int check_window(const UniformCall &u, int nmax, bool *nothing) {
  const UniformWindow &v = *u.win;
  if (u.problem != 0 && u.problem != 1) return -1;
  if (u.jobz != 0 && u.jobz != 1) return -2;
  if (v.range != 0 && v.range != 1) return -3;
  if (u.n < 0 || u.n > nmax) return -4;
  if (u.batch < 0) return -5;
  if (u.n == 0 || u.batch == 0) { *nothing = true; return 0; }
  if (v.range == 1) {
    if (v.vl != v.vl) return -6;
    if (!(v.vl < v.vu)) return -7;                  // vu NaN, or an empty interval
  } else {
    if (v.il < 1 || v.il > u.n) return -8;
    if (v.iu < v.il || v.iu > u.n) return -9;
  }
  if (int f = matrix_fault(u.A, u.lda, u.sA, u.n)) return -9 - f;
  if (u.problem == 1)
    if (int f = matrix_fault(u.B, u.ldb, u.sB, u.n)) return -12 - f;
  if (!v.m) return -16;
  if (!u.w) return -17;
  if (u.jobz == 1) {
    if (!u.Z) return -18;
    if (u.ldz < u.n) return -19;
  }
  if (v.zcap < 0 || (v.range == 0 && v.zcap < v.iu - v.il + 1)) return -20;   // with and without vectors
  if (u.jobz == 1 && u.sZ < (long long)u.ldz * std::max(1, v.zcap)) return -21;
  if (!u.info) return -22;
  return 0;
}

// nmax is the largest order the entry takes: EK_HIP_XBATCH_NMAX for the xbatched entries, which are the batched entries up
// to EK_HIP_BATCH_NMAX and ek_batched_x.hip's kernel above it
static int check(const UniformCall &u, int nmax, bool *nothing) {
  *nothing = false;
  if (u.win) return check_window(u, nmax, nothing);
  if (u.problem != 0 && u.problem != 1) return -1;
  if (u.jobz != 0 && u.jobz != 1) return -2;
  if (u.n < 0 || u.n > nmax) return -3;
  if (u.batch < 0) return -4;
  if (u.n == 0 || u.batch == 0) { *nothing = true; return 0; }
  if (int f = matrix_fault(u.A, u.lda, u.sA, u.n)) return -4 - f;
  if (u.problem == 1)
    if (int f = matrix_fault(u.B, u.ldb, u.sB, u.n)) return -7 - f;
  if (!u.w) return -11;
  if (u.jobz == 1)
    if (int f = matrix_fault(u.Z, u.ldz, u.sZ, u.n)) return -11 - f;
  if (!u.info) return -15;
  return 0;
}

// a pointer array with an entry for every problem of order > 0; a leading dimension for every problem
static bool entries(const VariableCall &v, double *const *P) {
  if (!P) return false;
  for (int b = 0; b < v.batch; ++b)
    if (v.n[b] > 0 && !P[b]) return false;
  return true;
}
static bool leading(const VariableCall &v, const int *ld) {
  if (!ld) return false;
  for (int b = 0; b < v.batch; ++b)
    if (ld[b] < (v.n[b] > 1 ? v.n[b] : 1)) return false;
  return true;
}

// the 19 checked arguments of a variable window entry; per-problem conditions hold for the problems of order > 0
static int check_window(const VariableCall &v, int nmax, bool *nothing) {
  const VariableWindow &x = *v.win;
  const int batch = v.batch, *n = v.n;
  if (v.problem != 0 && v.problem != 1) return -1;
  if (v.jobz != 0 && v.jobz != 1) return -2;
  if (x.range != 0 && x.range != 1) return -3;
  if (batch < 0) return -4;
  if (batch == 0) { *nothing = true; return 0; }
  if (!n) return -5;
  for (int b = 0; b < batch; ++b)
    if (n[b] < 0 || n[b] > nmax) return -5;
  if (x.range == 1) {
    if (!x.vl) return -6;
    for (int b = 0; b < batch; ++b)
      if (n[b] > 0 && x.vl[b] != x.vl[b]) return -6;
    if (!x.vu) return -7;
    for (int b = 0; b < batch; ++b)
      if (n[b] > 0 && !(x.vl[b] < x.vu[b])) return -7;   // vu NaN, or an empty interval
  } else {
    if (!x.il) return -8;
    for (int b = 0; b < batch; ++b)
      if (n[b] > 0 && (x.il[b] < 1 || x.il[b] > n[b])) return -8;
    if (!x.iu) return -9;
    for (int b = 0; b < batch; ++b)
      if (n[b] > 0 && (x.iu[b] < x.il[b] || x.iu[b] > n[b])) return -9;
  }
  if (!entries(v, v.A)) return -10;
  if (!leading(v, v.lda)) return -11;
  if (v.problem == 1) {
    if (!entries(v, v.B)) return -12;
    if (!leading(v, v.ldb)) return -13;
  }
  if (!x.m) return -14;
  if (!entries(v, v.w)) return -15;
  if (v.jobz == 1) {
    if (!v.Z) return -16;
    for (int b = 0; b < batch; ++b)                 // no Z is needed where it has no column
      if (n[b] > 0 && !v.Z[b] && !(x.zcap && x.zcap[b] == 0)) return -16;
    if (!leading(v, v.ldz)) return -17;
  }
  if (!x.zcap) return -18;
  for (int b = 0; b < batch; ++b)                   // with and without vectors, as the uniform call
    if (n[b] > 0 && (x.zcap[b] < 0 || (x.range == 0 && x.zcap[b] < x.iu[b] - x.il[b] + 1))) return -18;
  if (!v.info) return -19;
  return 0;
}

static int check(const VariableCall &v, int nmax, bool *nothing) {
  *nothing = false;
  if (v.win) return check_window(v, nmax, nothing);
  if (v.problem != 0 && v.problem != 1) return -1;
  if (v.jobz != 0 && v.jobz != 1) return -2;
  if (v.batch < 0) return -3;
  if (v.batch == 0) { *nothing = true; return 0; }
  if (!v.n) return -4;
  for (int b = 0; b < v.batch; ++b)
    if (v.n[b] < 0 || v.n[b] > nmax) return -4;
  if (!entries(v, v.A)) return -5;
  if (!leading(v, v.lda)) return -6;
  if (v.problem == 1) {
    if (!entries(v, v.B)) return -7;
    if (!leading(v, v.ldb)) return -8;
  }
  if (!entries(v, v.w)) return -9;
  if (v.jobz == 1) {
    if (!entries(v, v.Z)) return -10;
    if (!leading(v, v.ldz)) return -11;
  }
  if (!v.info) return -12;
  return 0;
}

// ---- uniform orders.  From here on: arguments checked, context up, g_mu held, device arrays

// The launches of a uniform call between two timing events (where the caller wants seconds), then info (and a window's m)
// back and the call's one synchronise.  launches(s) issues them on the context's stream and returns the first error
template <typename Launches>
static int run_uniform(const UniformCall &u, Launches launches) {
  hipStream_t s = g_ctx.stream;
  const size_t words = (size_t)u.batch * sizeof(int);
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (u.seconds) {
    int rc0 = create_event(&e0);
    if (rc0) return rc0;
    rc0 = create_event(&e1);
    if (rc0) { (void)hipEventDestroy(e0); return rc0; }
    (void)hipEventRecord(e0, s);
  }
  int rc = launches(s);
  if (u.seconds) (void)hipEventRecord(e1, s);
  hipError_t e = hipSuccess;
  if (!rc) e = hipMemcpyAsync(u.info, g_dinfo.p, words, hipMemcpyDeviceToHost, s);
  if (!rc && e == hipSuccess && u.win) e = hipMemcpyAsync(u.win->m, g_dm.p, words, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess && !rc) rc = -1000 - (int)e;
  if (u.seconds) {
    float ms = 0.f;
    if (!rc && hipEventElapsedTime(&ms, e0, e1) == hipSuccess) *u.seconds = (double)ms * 1e-3;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
  }
  return rc;
}

// a window of eigenpairs per problem (ek_hip_eigenpairs_window_*batched*; ek_hip_sygv_window_*batched* with itype)
static int run_window(const UniformCall &u) {
  const UniformWindow &v = *u.win;
  const int n = u.n, batch = u.batch;
  const int wcols = !u.jobz ? 0 : v.range == 0 ? v.iu - v.il + 1 : std::min(v.zcap, n);
  const size_t slot = (size_t)5 * n * wcols * sizeof(double);
  // wide slots: fewer problems per launch, so that the workspace stays near kWindowBytes -- in whole rounds of 256
  // workgroups (class 128 runs one per compute unit: a chunk of 409 would be three rounds for 512 problems), two at least
  const int fit = (int)std::min<size_t>(kWindowBytes / std::max(slot, (size_t)1), (size_t)g_wchunk);
  const bool x = n > EK_HIP_BATCH_NMAX;              // ek_batched_x.hip's class: its own chunk rule, and an image per slot
  const int xfit = (int)std::min<size_t>(kXWindowBytes / std::max(slot, (size_t)1), (size_t)g_xwchunk);
  const int K = x ? std::min(g_xwchunk, std::max(kXWindowRound, xfit / kXWindowRound * kXWindowRound))
                  : std::min(g_wchunk, std::max(512, fit / 256 * 256));
  int rc0 = g_dinfo.grow((size_t)batch);
  if (!rc0) rc0 = g_dm.grow((size_t)batch);
  if (!rc0) rc0 = g_wws.grow((size_t)std::min(batch, K) * slot / sizeof(double));
  if (!rc0 && x) rc0 = xwindow_prepare(std::min(batch, K));
  if (rc0) return rc0;
  // a problem that ends before stage 4W: m = 0
  EK_HIP_CHECK(hipMemsetAsync(g_dm.p, 0, (size_t)batch * sizeof(int), g_ctx.stream));
  return run_uniform(u, [&](hipStream_t s) {
    int rc = 0;
    for (int c0 = 0; c0 < batch && !rc; c0 += K) {
      const int count = std::min(K, batch - c0);
      double *A = u.A + (long long)c0 * u.sA, *B = u.problem ? u.B + (long long)c0 * u.sB : nullptr;
      double *w = u.w + (long long)c0 * n, *Z = u.jobz ? u.Z + (long long)c0 * u.sZ : nullptr;
      if (x)
        rc = xwindow_launch(s, u.problem, u.itype, u.jobz, n, count, A, u.lda, u.sA, B, u.ldb, u.sB, w, Z, u.ldz, u.sZ,
                            g_dinfo.p + c0, v.range, v.il, v.iu, v.zcap, v.vl, v.vu, g_dm.p + c0, g_wws.p, wcols);
      else
        rc = launch_order(n, s, count,
                          WArgs{{u.problem, u.jobz, n, A, u.lda, u.sA, B, u.ldb, u.sB, w, Z, u.ldz, u.sZ, g_dinfo.p + c0,
                                 u.itype},
                                {v.range, v.il, v.iu, v.zcap, v.vl, v.vu, g_dm.p + c0, g_wws.p, wcols}});
    }
    return rc;
  });
}

// above EK_HIP_BATCH_NMAX (the xbatched and ybatched entries only) the image in device memory: ek_batched_x.hip's kernel,
// its class of 256 rows up to EK_HIP_XBATCH_NMAX and its class of 512 rows above (the ybatched entries only)
static int run(const UniformCall &u) {
  if (u.win) return run_window(u);
  { int rc0 = g_dinfo.grow((size_t)u.batch); if (rc0) return rc0; }
  return run_uniform(u, [&](hipStream_t s) {
    if (u.n > EK_HIP_XBATCH_NMAX)                    // the ybatched entries only: the class of 512 rows
      return ybatched_launch(s, u.problem, u.itype, u.jobz, u.n, u.batch, u.A, u.lda, u.sA, u.B, u.ldb, u.sB, u.w, u.Z,
                             u.ldz, u.sZ, g_dinfo.p);
    if (u.n > EK_HIP_BATCH_NMAX)
      return xbatched_launch(s, u.problem, u.itype, u.jobz, u.n, u.batch, u.A, u.lda, u.sA, u.B, u.ldb, u.sB, u.w, u.Z,
                             u.ldz, u.sZ, g_dinfo.p);
    return launch_order(u.n, s, u.batch, Args{u.problem, u.jobz, u.n, u.A, u.lda, u.sA, u.B, u.ldb, u.sB, u.w, u.Z, u.ldz,
                                              u.sZ, g_dinfo.p, u.itype});
  });
}

// The host-pointer form: the caller's arrays are left as they are, the kernel works on device copies with the caller's own
// layout (what lies between the columns and between the problems travels with them, and comes back as it was).  Z has n
// columns a problem, or a window's zcap; a window's w and Z travel both ways, so that what the kernel leaves alone (the
// rest of a row of w, the columns from m[b] on, a failed problem's slots) comes back as the caller had it
static int stage(const UniformCall &u) {
  hipStream_t s = g_ctx.stream;
  const int n = u.n, zcols = u.win ? u.win->zcap : n;
  auto span = [&](int ld, long long stride, int cols) {
    return (size_t)(u.batch - 1) * (size_t)stride + (size_t)ld * (cols - 1) + n;
  };
  const size_t cA = span(u.lda, u.sA, n), cB = u.problem ? span(u.ldb, u.sB, n) : 0, cw = (size_t)u.batch * n;
  const size_t cZ = (u.jobz && zcols > 0) ? span(u.ldz, u.sZ, zcols) : 0;
  const bool zin = u.win ? cZ > 0 : u.jobz && (u.ldz != n || u.sZ != (long long)n * n);
  DevMem mem;
  UniformCall d = u;
  d.B = d.Z = nullptr;
  int rc = mem.alloc(&d.A, cA * 8);
  if (!rc) rc = mem.alloc(&d.w, cw * 8);
  if (!rc && u.problem) rc = mem.alloc(&d.B, cB * 8);
  if (!rc && u.jobz) rc = mem.alloc(&d.Z, std::max(cZ, (size_t)1) * 8);
  if (rc) return rc;
  EK_HIP_CHECK(hipMemcpyAsync(d.A, u.A, cA * 8, hipMemcpyHostToDevice, s));
  if (u.win) EK_HIP_CHECK(hipMemcpyAsync(d.w, u.w, cw * 8, hipMemcpyHostToDevice, s));
  if (u.problem) EK_HIP_CHECK(hipMemcpyAsync(d.B, u.B, cB * 8, hipMemcpyHostToDevice, s));
  if (zin) EK_HIP_CHECK(hipMemcpyAsync(d.Z, u.Z, cZ * 8, hipMemcpyHostToDevice, s));
  rc = run(d);
  if (rc) return rc;
  EK_HIP_CHECK(hipMemcpyAsync(u.w, d.w, cw * 8, hipMemcpyDeviceToHost, s));
  if (cZ) EK_HIP_CHECK(hipMemcpyAsync(u.Z, d.Z, cZ * 8, hipMemcpyDeviceToHost, s));
  EK_HIP_CHECK(hipStreamSynchronize(s));
  return 0;
}
static bool all_empty(const UniformCall &) { return false; }

// ---- problems of different orders (ek_hip_*_vbatched*, ek_hip_*_xvbatched*, ek_hip_*_window_xvbatched*; DESIGN.md 13, 21,
// 34).  The pointers in A, B, w, Z are device addresses.  Orders above EK_HIP_BATCH_NMAX make a class of their own in front
// of the three, which runs ek_batched_x.hip's kernel

// The host images of the problem table (and of a window's table beside it) and the problems of each class.  A class
// after the other, the largest first; inside a class descending order: the dispatcher hands out workgroups in index order
// and a workgroup's time grows like n^2 .. n^3, so this is longest-first list scheduling
static void classify(const VariableCall &v, int *count) {
  const int *n = v.n;
  std::vector<int> order;
  order.reserve((size_t)v.batch);
  for (int b = 0; b < v.batch; ++b)
    if (n[b] > 0) order.push_back(b);
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return n[x] > n[y]; });
  g_htable.resize(order.size());
  if (v.win) g_hwtable.resize(order.size());
  std::fill(count, count + kClasses, 0);
  for (size_t i = 0; i < order.size(); ++i) {
    const int b = order[i], c = class_of(n[b]);
    ++count[n[b] > EK_HIP_BATCH_NMAX ? 0 : c == 128 ? 1 : c == 64 ? 2 : 3];
    g_htable[i] = Desc{v.A[b], v.problem ? v.B[b] : nullptr, v.w[b], v.jobz ? v.Z[b] : nullptr, n[b], v.lda[b],
                       v.problem ? v.ldb[b] : 1, v.jobz ? v.ldz[b] : 1, b, 0};
    if (const VariableWindow *x = v.win) {
      const int range = x->range;
      const int wcols = !v.jobz ? 0 : range == 0 ? x->iu[b] - x->il[b] + 1 : std::min(x->zcap[b], n[b]);
      g_hwtable[i] = WDesc{range ? x->vl[b] : 0.0, range ? x->vu[b] : 0.0, range ? 0 : x->il[b], range ? 0 : x->iu[b],
                           x->zcap[b], wcols, 0};
    }
  }
}

// the largest class present runs on the context's stream (-1), every other one on a side stream of its own behind the
// fork event; returns the side streams used
static int assign_sides(const int *count, int *side) {
  int sides = 0;
  for (int k = 0, used = 0; k < kClasses; ++k)
    side[k] = (g_streams == 3 && count[k] && used++ > 0) ? sides++ : -1;
  return sides;
}

// the status words and the table of a classified call, its side streams and the events
static int ensure_variable(const VariableCall &v, const int *count) {
  int side[kClasses];
  const int sides = std::max(assign_sides(count, side), 2);   // the third: with four classes
  int rc = g_dinfo.grow((size_t)v.batch);
  if (!rc) rc = g_dtable.grow(g_htable.size());
  if (rc) return rc;
  for (int k = 0; k < sides; ++k)
    if (!g_side[k]) EK_HIP_CHECK(hipStreamCreateWithFlags(&g_side[k], hipStreamNonBlocking));
  for (int k = 0; k < kEvents && !rc; ++k)
    if (!g_ev[k]) rc = create_event(&g_ev[k]);
  return rc;
}

// A classified call whose pools stand: the tables go up, the classes present run beside each other from the fork event
// to their joins, info (and a window's m) come back, and the context's stream is synchronised once; the side streams
// only when an error may have left a class outside the join.  per_class(k, stream, off) issues the launches of class k,
// whose entries start at `off` in the table, and returns the first error
template <typename PerClass>
static int run_classes(const VariableCall &v, const int *count, PerClass per_class) {
  hipStream_t s = g_ctx.stream;
  const size_t words = (size_t)v.batch * sizeof(int);
  EK_HIP_CHECK(hipMemcpyAsync(g_dtable.p, g_htable.data(), g_htable.size() * sizeof(Desc), hipMemcpyHostToDevice, s));
  if (v.win) {
    EK_HIP_CHECK(hipMemcpyAsync(g_dwtable.p, g_hwtable.data(), g_hwtable.size() * sizeof(WDesc), hipMemcpyHostToDevice, s));
    EK_HIP_CHECK(hipMemsetAsync(g_dm.p, 0, words, s));   // a problem that ends before stage 4W: m = 0
  }
  int side[kClasses];
  assign_sides(count, side);
  hipStream_t cs[kClasses];
  for (int k = 0; k < kClasses; ++k) cs[k] = side[k] < 0 ? s : g_side[side[k]];
  EK_HIP_CHECK(hipEventRecord(g_ev[0], s));         // before the first launch
  int rc = 0, off = 0;
  hipError_t e = hipSuccess;
  for (int k = 0; k < kClasses && !rc && e == hipSuccess; ++k) {
    if (!count[k]) continue;
    if (cs[k] != s) e = hipStreamWaitEvent(cs[k], g_ev[0], 0);
    if (e != hipSuccess) break;
    if (v.seconds) (void)hipEventRecord(g_ev[kClasses + 2 * k], cs[k]);
    rc = per_class(k, cs[k], off);
    if (v.seconds) (void)hipEventRecord(g_ev[kClasses + 1 + 2 * k], cs[k]);
    if (cs[k] != s) {                               // join
      e = hipEventRecord(g_ev[k], cs[k]);
      if (e == hipSuccess) e = hipStreamWaitEvent(s, g_ev[k], 0);
    }
    off += count[k];
  }
  if (v.seconds) (void)hipEventRecord(g_ev[kEvents - 1], s);   // after the last launch has ended
  if (!rc && e == hipSuccess) e = hipMemcpyAsync(v.info, g_dinfo.p, words, hipMemcpyDeviceToHost, s);
  if (!rc && e == hipSuccess && v.win) e = hipMemcpyAsync(v.win->m, g_dm.p, words, hipMemcpyDeviceToHost, s);
  hipError_t es = hipStreamSynchronize(s);
  if (e != hipSuccess || rc)                        // an error may have left a class outside the join
    for (int k = 0; k < kClasses - 1; ++k)
      if (g_side[k]) (void)hipStreamSynchronize(g_side[k]);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess && !rc) rc = -1000 - (int)e;
  if (v.seconds && !rc) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, g_ev[0], g_ev[kEvents - 1]) == hipSuccess) *v.seconds = (double)ms * 1e-3;
    for (int k = 0; k < kClasses; ++k) {
      g_class_count[k] = count[k];
      g_class_seconds[k] = 0.0;
      if (count[k] && hipEventElapsedTime(&ms, g_ev[kClasses + 2 * k], g_ev[kClasses + 1 + 2 * k]) == hipSuccess)
        g_class_seconds[k] = (double)ms * 1e-3;
    }
  }
  if (!rc)
    for (int b = 0; b < v.batch; ++b)
      if (v.n[b] == 0) {
        v.info[b] = 0;
        if (v.win) v.win->m[b] = 0;
      }
  return rc;
}

// The launches of a variable window call, the slot offsets inside each (into the window table's lu), and a region of the LU
// workspace per class as wide as its widest launch: the classes run beside each other, the launches of a class share its
// region in the order of the class's stream.  A class runs in launches of consecutive table entries: a launch ends at K
// problems or where its LU slots, summed, would pass the class's budget.  The three classes of LDS share the uniform
// calls' kWindowBytes in equal parts, the class of 256 has its kXWindowBytes
struct VLaunch { int cls, first, count; };          // a launch: `count` table entries from `first`
struct WindowPlan {
  std::vector<VLaunch> launches;
  size_t base[kClasses];                            // where a class's region starts, in doubles
  size_t doubles;                                   // all regions
  int xslots;                                       // the widest launch of the class of 256
};
static WindowPlan plan_window_launches(const int *count) {
  WindowPlan p{{}, {0, 0, 0, 0}, 0, 0};
  int small = 0;
  for (int k = 1; k < kClasses; ++k) small += count[k] ? 1 : 0;
  size_t region[kClasses] = {0, 0, 0, 0};
  for (int k = 0, off = 0; k < kClasses; off += count[k], ++k) {
    if (!count[k]) continue;
    const int K = k == 0 ? g_xwchunk : g_wchunk;
    const size_t budget = (g_vwbudget > 0 ? (size_t)g_vwbudget : k == 0 ? kXWindowBytes : kWindowBytes / small) / 8;
    VLaunch cur{k, off, 0};
    size_t sum = 0;
    for (int i = off; i < off + count[k]; ++i) {
      const size_t slot = (size_t)5 * g_htable[i].n * g_hwtable[i].wcols;
      if (cur.count > 0 && (cur.count >= K || sum + slot > budget)) {   // a launch always takes one problem
        p.launches.push_back(cur);
        cur = VLaunch{k, i, 0};
        sum = 0;
      }
      g_hwtable[i].lu = (long long)sum;
      sum += slot;
      ++cur.count;
      region[k] = std::max(region[k], sum);
      if (k == 0) p.xslots = std::max(p.xslots, cur.count);
    }
    p.launches.push_back(cur);
  }
  for (int k = 1; k < kClasses; ++k) p.base[k] = p.base[k - 1] + region[k - 1];
  p.doubles = p.base[kClasses - 1] + region[kClasses - 1];
  return p;
}

static int run_variable_window(const VariableCall &v) {
  int count[kClasses];
  classify(v, count);
  const WindowPlan plan = plan_window_launches(count);
  int rc0 = ensure_variable(v, count);
  if (!rc0) rc0 = g_dwtable.grow(g_htable.size());
  if (!rc0) rc0 = g_dm.grow((size_t)v.batch);
  if (!rc0) rc0 = g_wws.grow(plan.doubles);
  if (!rc0 && plan.xslots) rc0 = xwindow_prepare(plan.xslots);
  if (rc0) return rc0;
  size_t next = 0;                                  // the launches stand in the order of their classes
  return run_classes(v, count, [&](int k, hipStream_t cs, int) {
    int rc = 0;
    for (; next < plan.launches.size() && plan.launches[next].cls == k && !rc; ++next) {
      const VLaunch &l = plan.launches[next];
      const Desc *table = g_dtable.p + l.first;
      const WDesc *wtable = g_dwtable.p + l.first;
      double *lu = g_wws.p + plan.base[k];
      rc = k == 0 ? xvwindow_launch(cs, v.problem, v.itype, v.jobz, v.win->range, l.count, table, wtable, g_dinfo.p,
                                    g_dm.p, lu)
                  : launch_order(kClassOrder[k], cs, l.count, VWArgs{v.problem, v.jobz, table, wtable, g_dinfo.p, g_dm.p, lu,
                                                                     v.win->range, v.itype});
    }
    return rc;
  });
}

// a launch per class; the class of 256 in chunks of its own (xvbatched_launch)
static int run(const VariableCall &v) {
  if (v.win) return run_variable_window(v);
  int count[kClasses];
  classify(v, count);
  int rc0 = ensure_variable(v, count);
  if (!rc0 && count[0]) rc0 = xvbatched_prepare(count[0]);
  if (rc0) return rc0;
  return run_classes(v, count, [&](int k, hipStream_t cs, int off) {
    return k == 0 ? xvbatched_launch(cs, v.problem, v.itype, v.jobz, count[k], g_dtable.p + off, g_dinfo.p)
                  : launch_order(kClassOrder[k], cs, count[k], VArgs{v.problem, v.jobz, g_dtable.p + off, g_dinfo.p, v.itype});
  });
}

// a batch without a problem of order > 0 is answered without the device
static bool all_empty(const VariableCall &v) {
  for (int b = 0; b < v.batch; ++b)
    if (v.n[b] > 0) return false;
  for (int b = 0; b < v.batch; ++b) {
    v.info[b] = 0;
    if (v.win) v.win->m[b] = 0;
  }
  return true;
}

// The host-pointer form.  Compact device layout (ld = n[b]; Z with n[b] columns, or a window's zcap[b]), a problem behind
// the other: the caller's padding never travels.  One staging buffer per matrix kind: A and B go in as lower triangles,
// column by column (what lies above them is never read).  Only what the kernel wrote comes back -- n[b] values and
// columns, or a window's m[b] -- and, like the device form, a failed problem leaves its slots alone
static int stage(const VariableCall &v) {
  hipStream_t s = g_ctx.stream;
  const int batch = v.batch, *n = v.n;
  std::vector<size_t> offm((size_t)batch + 1, 0), offv((size_t)batch + 1, 0), offz((size_t)batch + 1, 0);
  for (int b = 0; b < batch; ++b) {
    offm[b + 1] = offm[b] + (size_t)n[b] * n[b];
    offv[b + 1] = offv[b] + (size_t)n[b];
    offz[b + 1] = offz[b] + (v.jobz && n[b] > 0 ? (size_t)n[b] * (v.win ? v.win->zcap[b] : n[b]) : 0);
  }
  const size_t cm = offm[batch], cv = offv[batch], cz = offz[batch];
  auto pack = [&](double *const *M, const int *ld, std::vector<double> &h) {
    h.assign(cm, 0.0);
    for (int b = 0; b < batch; ++b)
      for (int j = 0; j < n[b]; ++j)
        std::memcpy(&h[offm[b] + (size_t)j * n[b] + j], M[b] + (size_t)j * ld[b] + j, (size_t)(n[b] - j) * 8);
  };
  std::vector<double> hA, hB, hw, hZ;
  pack(v.A, v.lda, hA);
  if (v.problem) pack(v.B, v.ldb, hB);
  DevMem mem;
  double *uA = nullptr, *uB = nullptr, *uw = nullptr, *uZ = nullptr;
  int rc = mem.alloc(&uA, cm * 8);
  if (!rc) rc = mem.alloc(&uw, cv * 8);
  if (!rc && v.problem) rc = mem.alloc(&uB, cm * 8);
  if (!rc && v.jobz) rc = mem.alloc(&uZ, std::max(cz, (size_t)1) * 8);
  if (rc) return rc;
  std::vector<double *> pA((size_t)batch), pB((size_t)batch), pw((size_t)batch), pZ((size_t)batch);
  std::vector<int> ldc((size_t)batch);
  for (int b = 0; b < batch; ++b) {
    pA[b] = uA + offm[b];
    pB[b] = v.problem ? uB + offm[b] : nullptr;
    pw[b] = uw + offv[b];
    pZ[b] = v.jobz ? uZ + offz[b] : nullptr;
    ldc[b] = n[b] > 1 ? n[b] : 1;
  }
  EK_HIP_CHECK(hipMemcpyAsync(uA, hA.data(), cm * 8, hipMemcpyHostToDevice, s));
  if (v.problem) EK_HIP_CHECK(hipMemcpyAsync(uB, hB.data(), cm * 8, hipMemcpyHostToDevice, s));
  VariableCall d = v;
  d.A = pA.data(); d.B = pB.data(); d.w = pw.data(); d.Z = pZ.data();
  d.lda = d.ldb = d.ldz = ldc.data();
  rc = run(d);
  if (rc) return rc;
  hw.resize(cv);
  EK_HIP_CHECK(hipMemcpyAsync(hw.data(), uw, cv * 8, hipMemcpyDeviceToHost, s));
  if (v.jobz && cz) {
    hZ.resize(cz);
    EK_HIP_CHECK(hipMemcpyAsync(hZ.data(), uZ, cz * 8, hipMemcpyDeviceToHost, s));
  }
  EK_HIP_CHECK(hipStreamSynchronize(s));
  for (int b = 0; b < batch; ++b) {
    if (v.info[b] != 0 || n[b] == 0) continue;
    const int cols = v.win ? v.win->m[b] : n[b];
    std::memcpy(v.w[b], &hw[offv[b]], (size_t)cols * 8);
    if (v.jobz)
      for (int j = 0; j < cols; ++j)
        std::memcpy(v.Z[b] + (size_t)j * v.ldz[b], &hZ[offz[b] + (size_t)j * n[b]], (size_t)n[b] * 8);
  }
  return 0;
}

// The body of every entry: check, *seconds = 0, nothing to do (or nothing but empty problems: filled here), the context,
// g_mu, and the call in its host-pointer or device-pointer form
template <typename Call>
static int entry(const Call &c, int nmax, bool host) {
  bool nothing;
  int rc = check(c, nmax, &nothing);
  if (rc) return rc;
  if (c.seconds) *c.seconds = 0.0;
  if (nothing || all_empty(c)) return 0;
  rc = ensure_init(); if (rc) return rc;
  std::lock_guard<std::mutex> lk(g_mu);
  return host ? stage(c) : run(c);
}

// The entries fill their call: the eigenpairs entries with itype 1; the sygv entries, DSYGV's three problem types, with
// problem 1 and itype in its place, so that every other argument keeps its number.  The host-pointer forms do not write
// through A and B.  The x entries take orders up to EK_HIP_XBATCH_NMAX: above EK_HIP_BATCH_NMAX ek_batched_x.hip's kernel
// (CONG for types 2 and 3), every other problem the kernel the entries without x give it
extern "C" {

int ek_hip_eigenpairs_batched_device(int problem, int jobz, int n, int batch, double *dA, int lda, long long strideA,
                                     double *dB, int ldb, long long strideB, double *dw, double *dZ, int ldz,
                                     long long strideZ, int *info, double *seconds) {
  return entry(UniformCall{problem, 1, jobz, n, batch, dA, lda, strideA, dB, ldb, strideB, dw, dZ, ldz, strideZ, info,
                           seconds, nullptr}, EK_HIP_BATCH_NMAX, false);
}

int ek_hip_eigenpairs_batched(int problem, int jobz, int n, int batch, const double *A, int lda, long long strideA,
                              const double *B, int ldb, long long strideB, double *w, double *Z, int ldz,
                              long long strideZ, int *info, double *seconds) {
  return entry(UniformCall{problem, 1, jobz, n, batch, (double *)A, lda, strideA, (double *)B, ldb, strideB, w, Z, ldz,
                           strideZ, info, seconds, nullptr}, EK_HIP_BATCH_NMAX, true);
}

int ek_hip_eigenpairs_xbatched_device(int problem, int jobz, int n, int batch, double *dA, int lda, long long strideA,
                                      double *dB, int ldb, long long strideB, double *dw, double *dZ, int ldz,
                                      long long strideZ, int *info, double *seconds) {
  return entry(UniformCall{problem, 1, jobz, n, batch, dA, lda, strideA, dB, ldb, strideB, dw, dZ, ldz, strideZ, info,
                           seconds, nullptr}, EK_HIP_XBATCH_NMAX, false);
}

int ek_hip_eigenpairs_xbatched(int problem, int jobz, int n, int batch, const double *A, int lda, long long strideA,
                               const double *B, int ldb, long long strideB, double *w, double *Z, int ldz,
                               long long strideZ, int *info, double *seconds) {
  return entry(UniformCall{problem, 1, jobz, n, batch, (double *)A, lda, strideA, (double *)B, ldb, strideB, w, Z, ldz,
                           strideZ, info, seconds, nullptr}, EK_HIP_XBATCH_NMAX, true);
}

int ek_hip_sygv_batched_device(int itype, int jobz, int n, int batch, double *dA, int lda, long long strideA,
                               double *dB, int ldb, long long strideB, double *dw, double *dZ, int ldz,
                               long long strideZ, int *info, double *seconds) {
  if (itype < 1 || itype > 3) return -1;
  return entry(UniformCall{1, itype, jobz, n, batch, dA, lda, strideA, dB, ldb, strideB, dw, dZ, ldz, strideZ, info,
                           seconds, nullptr}, EK_HIP_BATCH_NMAX, false);
}

int ek_hip_sygv_batched(int itype, int jobz, int n, int batch, const double *A, int lda, long long strideA,
                        const double *B, int ldb, long long strideB, double *w, double *Z, int ldz, long long strideZ,
                        int *info, double *seconds) {
  if (itype < 1 || itype > 3) return -1;
  return entry(UniformCall{1, itype, jobz, n, batch, (double *)A, lda, strideA, (double *)B, ldb, strideB, w, Z, ldz,
                           strideZ, info, seconds, nullptr}, EK_HIP_BATCH_NMAX, true);
}

int ek_hip_sygv_xbatched_device(int itype, int jobz, int n, int batch, double *dA, int lda, long long strideA,
                                double *dB, int ldb, long long strideB, double *dw, double *dZ, int ldz,
                                long long strideZ, int *info, double *seconds) {
  if (itype < 1 || itype > 3) return -1;
  return entry(UniformCall{1, itype, jobz, n, batch, dA, lda, strideA, dB, ldb, strideB, dw, dZ, ldz, strideZ, info,
                           seconds, nullptr}, EK_HIP_XBATCH_NMAX, false);
}

int ek_hip_sygv_xbatched(int itype, int jobz, int n, int batch, const double *A, int lda, long long strideA,
                         const double *B, int ldb, long long strideB, double *w, double *Z, int ldz,
                         long long strideZ, int *info, double *seconds) {
  if (itype < 1 || itype > 3) return -1;
  return entry(UniformCall{1, itype, jobz, n, batch, (double *)A, lda, strideA, (double *)B, ldb, strideB, w, Z, ldz,
                           strideZ, info, seconds, nullptr}, EK_HIP_XBATCH_NMAX, true);
}

// the y entries take orders up to EK_HIP_YBATCH_NMAX: above EK_HIP_XBATCH_NMAX ek_batched_x.hip's class of 512 rows, every
// other problem what the x entries give it
int ek_hip_eigenpairs_ybatched_device(int problem, int jobz, int n, int batch, double *dA, int lda, long long strideA,
                                      double *dB, int ldb, long long strideB, double *dw, double *dZ, int ldz,
                                      long long strideZ, int *info, double *seconds) {
  return entry(UniformCall{problem, 1, jobz, n, batch, dA, lda, strideA, dB, ldb, strideB, dw, dZ, ldz, strideZ, info,
                           seconds, nullptr}, EK_HIP_YBATCH_NMAX, false);
}

int ek_hip_eigenpairs_ybatched(int problem, int jobz, int n, int batch, const double *A, int lda, long long strideA,
                               const double *B, int ldb, long long strideB, double *w, double *Z, int ldz,
                               long long strideZ, int *info, double *seconds) {
  return entry(UniformCall{problem, 1, jobz, n, batch, (double *)A, lda, strideA, (double *)B, ldb, strideB, w, Z, ldz,
                           strideZ, info, seconds, nullptr}, EK_HIP_YBATCH_NMAX, true);
}

int ek_hip_sygv_ybatched_device(int itype, int jobz, int n, int batch, double *dA, int lda, long long strideA,
                                double *dB, int ldb, long long strideB, double *dw, double *dZ, int ldz,
                                long long strideZ, int *info, double *seconds) {
  if (itype < 1 || itype > 3) return -1;
  return entry(UniformCall{1, itype, jobz, n, batch, dA, lda, strideA, dB, ldb, strideB, dw, dZ, ldz, strideZ, info,
                           seconds, nullptr}, EK_HIP_YBATCH_NMAX, false);
}

int ek_hip_sygv_ybatched(int itype, int jobz, int n, int batch, const double *A, int lda, long long strideA,
                         const double *B, int ldb, long long strideB, double *w, double *Z, int ldz,
                         long long strideZ, int *info, double *seconds) {
  if (itype < 1 || itype > 3) return -1;
  return entry(UniformCall{1, itype, jobz, n, batch, (double *)A, lda, strideA, (double *)B, ldb, strideB, w, Z, ldz,
                           strideZ, info, seconds, nullptr}, EK_HIP_YBATCH_NMAX, true);
}

// problems of different orders
int ek_hip_eigenpairs_vbatched_device(int problem, int jobz, int batch, const int *n, double *const *dA, const int *lda,
                                      double *const *dB, const int *ldb, double *const *dw, double *const *dZ,
                                      const int *ldz, int *info, double *seconds) {
  return entry(VariableCall{problem, 1, jobz, batch, n, dA, lda, dB, ldb, dw, dZ, ldz, info, seconds, nullptr},
               EK_HIP_BATCH_NMAX, false);
}

int ek_hip_eigenpairs_vbatched(int problem, int jobz, int batch, const int *n, const double *const *A, const int *lda,
                               const double *const *B, const int *ldb, double *const *w, double *const *Z,
                               const int *ldz, int *info, double *seconds) {
  return entry(VariableCall{problem, 1, jobz, batch, n, (double *const *)A, lda, (double *const *)B, ldb, w, Z, ldz, info,
                            seconds, nullptr}, EK_HIP_BATCH_NMAX, true);
}

int ek_hip_sygv_vbatched_device(int itype, int jobz, int batch, const int *n, double *const *dA, const int *lda,
                                double *const *dB, const int *ldb, double *const *dw, double *const *dZ,
                                const int *ldz, int *info, double *seconds) {
  if (itype < 1 || itype > 3) return -1;
  return entry(VariableCall{1, itype, jobz, batch, n, dA, lda, dB, ldb, dw, dZ, ldz, info, seconds, nullptr},
               EK_HIP_BATCH_NMAX, false);
}

int ek_hip_sygv_vbatched(int itype, int jobz, int batch, const int *n, const double *const *A, const int *lda,
                         const double *const *B, const int *ldb, double *const *w, double *const *Z, const int *ldz,
                         int *info, double *seconds) {
  if (itype < 1 || itype > 3) return -1;
  return entry(VariableCall{1, itype, jobz, batch, n, (double *const *)A, lda, (double *const *)B, ldb, w, Z, ldz, info,
                            seconds, nullptr}, EK_HIP_BATCH_NMAX, true);
}

int ek_hip_eigenpairs_xvbatched_device(int problem, int jobz, int batch, const int *n, double *const *dA,
                                       const int *lda, double *const *dB, const int *ldb, double *const *dw,
                                       double *const *dZ, const int *ldz, int *info, double *seconds) {
  return entry(VariableCall{problem, 1, jobz, batch, n, dA, lda, dB, ldb, dw, dZ, ldz, info, seconds, nullptr},
               EK_HIP_XBATCH_NMAX, false);
}

int ek_hip_eigenpairs_xvbatched(int problem, int jobz, int batch, const int *n, const double *const *A, const int *lda,
                                const double *const *B, const int *ldb, double *const *w, double *const *Z,
                                const int *ldz, int *info, double *seconds) {
  return entry(VariableCall{problem, 1, jobz, batch, n, (double *const *)A, lda, (double *const *)B, ldb, w, Z, ldz, info,
                            seconds, nullptr}, EK_HIP_XBATCH_NMAX, true);
}

int ek_hip_sygv_xvbatched_device(int itype, int jobz, int batch, const int *n, double *const *dA, const int *lda,
                                 double *const *dB, const int *ldb, double *const *dw, double *const *dZ,
                                 const int *ldz, int *info, double *seconds) {
  if (itype < 1 || itype > 3) return -1;
  return entry(VariableCall{1, itype, jobz, batch, n, dA, lda, dB, ldb, dw, dZ, ldz, info, seconds, nullptr},
               EK_HIP_XBATCH_NMAX, false);
}

int ek_hip_sygv_xvbatched(int itype, int jobz, int batch, const int *n, const double *const *A, const int *lda,
                          const double *const *B, const int *ldb, double *const *w, double *const *Z, const int *ldz,
                          int *info, double *seconds) {
  if (itype < 1 || itype > 3) return -1;
  return entry(VariableCall{1, itype, jobz, batch, n, (double *const *)A, lda, (double *const *)B, ldb, w, Z, ldz, info,
                            seconds, nullptr}, EK_HIP_XBATCH_NMAX, true);
}

// a window of eigenpairs per problem
int ek_hip_eigenpairs_window_batched_device(int problem, int jobz, int range, int n, int batch, double vl, double vu,
                                            int il, int iu, double *dA, int lda, long long strideA, double *dB, int ldb,
                                            long long strideB, int *m, double *dw, double *dZ, int ldz, int zcap,
                                            long long strideZ, int *info, double *seconds) {
  const UniformWindow win{range, vl, vu, il, iu, zcap, m};
  return entry(UniformCall{problem, 1, jobz, n, batch, dA, lda, strideA, dB, ldb, strideB, dw, dZ, ldz, strideZ, info,
                           seconds, &win}, EK_HIP_BATCH_NMAX, false);
}

int ek_hip_eigenpairs_window_batched(int problem, int jobz, int range, int n, int batch, double vl, double vu, int il,
                                     int iu, const double *A, int lda, long long strideA, const double *B, int ldb,
                                     long long strideB, int *m, double *w, double *Z, int ldz, int zcap,
                                     long long strideZ, int *info, double *seconds) {
  const UniformWindow win{range, vl, vu, il, iu, zcap, m};
  return entry(UniformCall{problem, 1, jobz, n, batch, (double *)A, lda, strideA, (double *)B, ldb, strideB, w, Z, ldz,
                           strideZ, info, seconds, &win}, EK_HIP_BATCH_NMAX, true);
}

int ek_hip_eigenpairs_window_xbatched_device(int problem, int jobz, int range, int n, int batch, double vl, double vu,
                                             int il, int iu, double *dA, int lda, long long strideA, double *dB,
                                             int ldb, long long strideB, int *m, double *dw, double *dZ, int ldz,
                                             int zcap, long long strideZ, int *info, double *seconds) {
  const UniformWindow win{range, vl, vu, il, iu, zcap, m};
  return entry(UniformCall{problem, 1, jobz, n, batch, dA, lda, strideA, dB, ldb, strideB, dw, dZ, ldz, strideZ, info,
                           seconds, &win}, EK_HIP_XBATCH_NMAX, false);
}

int ek_hip_eigenpairs_window_xbatched(int problem, int jobz, int range, int n, int batch, double vl, double vu, int il,
                                      int iu, const double *A, int lda, long long strideA, const double *B, int ldb,
                                      long long strideB, int *m, double *w, double *Z, int ldz, int zcap,
                                      long long strideZ, int *info, double *seconds) {
  const UniformWindow win{range, vl, vu, il, iu, zcap, m};
  return entry(UniformCall{problem, 1, jobz, n, batch, (double *)A, lda, strideA, (double *)B, ldb, strideB, w, Z, ldz,
                           strideZ, info, seconds, &win}, EK_HIP_XBATCH_NMAX, true);
}

int ek_hip_sygv_window_batched_device(int itype, int jobz, int range, int n, int batch, double vl, double vu, int il,
                                      int iu, double *dA, int lda, long long strideA, double *dB, int ldb,
                                      long long strideB, int *m, double *dw, double *dZ, int ldz, int zcap,
                                      long long strideZ, int *info, double *seconds) {
  if (itype < 1 || itype > 3) return -1;
  const UniformWindow win{range, vl, vu, il, iu, zcap, m};
  return entry(UniformCall{1, itype, jobz, n, batch, dA, lda, strideA, dB, ldb, strideB, dw, dZ, ldz, strideZ, info,
                           seconds, &win}, EK_HIP_BATCH_NMAX, false);
}

int ek_hip_sygv_window_batched(int itype, int jobz, int range, int n, int batch, double vl, double vu, int il, int iu,
                               const double *A, int lda, long long strideA, const double *B, int ldb, long long strideB,
                               int *m, double *w, double *Z, int ldz, int zcap, long long strideZ, int *info,
                               double *seconds) {
  if (itype < 1 || itype > 3) return -1;
  const UniformWindow win{range, vl, vu, il, iu, zcap, m};
  return entry(UniformCall{1, itype, jobz, n, batch, (double *)A, lda, strideA, (double *)B, ldb, strideB, w, Z, ldz,
                           strideZ, info, seconds, &win}, EK_HIP_BATCH_NMAX, true);
}

int ek_hip_sygv_window_xbatched_device(int itype, int jobz, int range, int n, int batch, double vl, double vu, int il,
                                       int iu, double *dA, int lda, long long strideA, double *dB, int ldb,
                                       long long strideB, int *m, double *dw, double *dZ, int ldz, int zcap,
                                       long long strideZ, int *info, double *seconds) {
  if (itype < 1 || itype > 3) return -1;
  const UniformWindow win{range, vl, vu, il, iu, zcap, m};
  return entry(UniformCall{1, itype, jobz, n, batch, dA, lda, strideA, dB, ldb, strideB, dw, dZ, ldz, strideZ, info,
                           seconds, &win}, EK_HIP_XBATCH_NMAX, false);
}

int ek_hip_sygv_window_xbatched(int itype, int jobz, int range, int n, int batch, double vl, double vu, int il, int iu,
                                const double *A, int lda, long long strideA, const double *B, int ldb,
                                long long strideB, int *m, double *w, double *Z, int ldz, int zcap, long long strideZ,
                                int *info, double *seconds) {
  if (itype < 1 || itype > 3) return -1;
  const UniformWindow win{range, vl, vu, il, iu, zcap, m};
  return entry(UniformCall{1, itype, jobz, n, batch, (double *)A, lda, strideA, (double *)B, ldb, strideB, w, Z, ldz,
                           strideZ, info, seconds, &win}, EK_HIP_XBATCH_NMAX, true);
}

// a window per problem, for problems of different orders up to EK_HIP_XBATCH_NMAX
int ek_hip_eigenpairs_window_xvbatched_device(int problem, int jobz, int range, int batch, const int *n, const double *vl,
                                              const double *vu, const int *il, const int *iu, double *const *dA,
                                              const int *lda, double *const *dB, const int *ldb, int *m,
                                              double *const *dw, double *const *dZ, const int *ldz, const int *zcap,
                                              int *info, double *seconds) {
  const VariableWindow win{range, vl, vu, il, iu, zcap, m};
  return entry(VariableCall{problem, 1, jobz, batch, n, dA, lda, dB, ldb, dw, dZ, ldz, info, seconds, &win},
               EK_HIP_XBATCH_NMAX, false);
}

int ek_hip_eigenpairs_window_xvbatched(int problem, int jobz, int range, int batch, const int *n, const double *vl,
                                       const double *vu, const int *il, const int *iu, const double *const *A,
                                       const int *lda, const double *const *B, const int *ldb, int *m, double *const *w,
                                       double *const *Z, const int *ldz, const int *zcap, int *info, double *seconds) {
  const VariableWindow win{range, vl, vu, il, iu, zcap, m};
  return entry(VariableCall{problem, 1, jobz, batch, n, (double *const *)A, lda, (double *const *)B, ldb, w, Z, ldz, info,
                            seconds, &win}, EK_HIP_XBATCH_NMAX, true);
}

int ek_hip_sygv_window_xvbatched_device(int itype, int jobz, int range, int batch, const int *n, const double *vl,
                                        const double *vu, const int *il, const int *iu, double *const *dA,
                                        const int *lda, double *const *dB, const int *ldb, int *m, double *const *dw,
                                        double *const *dZ, const int *ldz, const int *zcap, int *info, double *seconds) {
  if (itype < 1 || itype > 3) return -1;
  const VariableWindow win{range, vl, vu, il, iu, zcap, m};
  return entry(VariableCall{1, itype, jobz, batch, n, dA, lda, dB, ldb, dw, dZ, ldz, info, seconds, &win},
               EK_HIP_XBATCH_NMAX, false);
}

int ek_hip_sygv_window_xvbatched(int itype, int jobz, int range, int batch, const int *n, const double *vl,
                                 const double *vu, const int *il, const int *iu, const double *const *A, const int *lda,
                                 const double *const *B, const int *ldb, int *m, double *const *w, double *const *Z,
                                 const int *ldz, const int *zcap, int *info, double *seconds) {
  if (itype < 1 || itype > 3) return -1;
  const VariableWindow win{range, vl, vu, il, iu, zcap, m};
  return entry(VariableCall{1, itype, jobz, batch, n, (double *const *)A, lda, (double *const *)B, ldb, w, Z, ldz, info,
                            seconds, &win}, EK_HIP_XBATCH_NMAX, true);
}

long long ek_hip_debug_window_xvbatched_budget(long long bytes) {
  std::lock_guard<std::mutex> lk(g_mu);
  const long long before = g_vwbudget;
  g_vwbudget = bytes > 0 ? bytes : 0;
  return before;
}

int ek_hip_debug_window_xbatched_chunk(int problems) {
  std::lock_guard<std::mutex> lk(g_mu);
  const int before = g_xwchunk;
  g_xwchunk = problems > 0 ? problems : kXWindowChunk;
  return before;
}

int ek_hip_debug_window_batched_chunk(int problems) {
  std::lock_guard<std::mutex> lk(g_mu);
  const int before = g_wchunk;
  g_wchunk = problems > 0 ? problems : kWindowChunk;
  return before;
}

int ek_hip_debug_vbatched_streams(int streams) {
  if (streams != 1 && streams != 3) streams = 3;
  std::lock_guard<std::mutex> lk(g_mu);
  g_streams = streams;
  return 0;
}

int ek_hip_debug_vbatched_last(double *class_seconds, int *class_count) {
  std::lock_guard<std::mutex> lk(g_mu);
  for (int k = 0; k < 3; ++k) {                     // classes of 128, 64, 32
    if (class_seconds) class_seconds[k] = g_class_seconds[k + 1];
    if (class_count) class_count[k] = g_class_count[k + 1];
  }
  return 0;
}

int ek_hip_debug_xvbatched_last(double *class_seconds, int *class_count) {
  std::lock_guard<std::mutex> lk(g_mu);
  for (int k = 0; k < kClasses; ++k) {              // classes of 256, 128, 64, 32
    if (class_seconds) class_seconds[k] = g_class_seconds[k];
    if (class_count) class_count[k] = g_class_count[k];
  }
  return 0;
}

}  // extern "C"
