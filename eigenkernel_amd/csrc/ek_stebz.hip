// ek_stebz.hip -- eigenvalues il..iu of a symmetric tridiagonal (d, e) by bisection with Sturm counts: the GPU
// counterpart of DSTEBZ with RANGE = 'I' (no eigenvectors).  Two kernels:
//   stebz_prep   one workgroup: e^2, the Gershgorin interval [gl, gu] widened as DSTEBZ widens it, pivmin =
//                safmin max(1, max e^2), the absolute tolerance 2 eps max(|gl|, |gu|) + 2 pivmin and the number of
//                passes every index makes (all of it min / max reductions: no order dependence);
//   stebz_bisect G lanes per index, each lane evaluating K points per pass: one pass splits the index's bracket into
//                S = G K equal parts (x_j = lo + (hi - lo) j / S, j = 0..S-1) and keeps the part holding the index,
//                log2(S) bits per pass.  Every index makes the same number of passes from the same starting interval,
//                so a bracket is always a cell of one fixed grid: the value returned for index k depends on (d, e, k)
//                alone -- not on il, iu or on the other indices (no atomics) -- and the returned values are
//                non-decreasing in k (cells of one level do not overlap, the result is the cell's midpoint).
//   stebz_window_count  one wave: the counts at vl and vu (RANGE = 'V', the half-open interval (vl, vu]) with the same
//                recurrence, pivmin and [gl, gu] as the bisection -> il = count(vl) + 1, iu = count(vu).
// The count of T - x I is the number of negative pivots of q_i = (d_i - x) - e_{i-1}^2 / q_{i-1}, |q| < pivmin clamped
// to -pivmin (DLAEBZ).  It is monotone in x under IEEE arithmetic with every operation rounded on its own (Demmel,
// Dhillon and Ren 1995): hence fp contract(off) in the recurrence and in the grid points.
#include "ek_common.h"

#include <cfloat>

namespace ek {

namespace {

constexpr int kStebzK = 2;           // points per lane (independent division chains a lane interleaves)
int g_stebz_lanes = 4;               // lanes per index (ek_hip_debug_set_stebz); S = 4 * 2 = 8 parts per pass
constexpr int kPrepThreads = 1024;

// params[0..4]: gl, gu, pivmin, tolerance, passes (as a double)
__global__ void __launch_bounds__(kPrepThreads) stebz_prep(int n, const double *__restrict__ d,
                                                          const double *__restrict__ e, double *__restrict__ e2,
                                                          double *__restrict__ params, int bits) {
#pragma clang fp contract(off)
  __shared__ double s_lo[kPrepThreads], s_hi[kPrepThreads], s_e2[kPrepThreads];
  const int t = threadIdx.x;
  double lo = DBL_MAX, hi = -DBL_MAX, m2 = 0.0;
  for (int i = t; i < n; i += kPrepThreads) {
    const double ei = (i < n - 1) ? e[i] : 0.0;
    const double ep = (i > 0) ? e[i - 1] : 0.0;
    const double sq = ei * ei;
    e2[i] = sq;
    if (sq > m2) m2 = sq;
    const double r = fabs(ep) + fabs(ei);
    const double a = d[i] - r, b = d[i] + r;
    if (a < lo) lo = a;
    if (b > hi) hi = b;
  }
  s_lo[t] = lo; s_hi[t] = hi; s_e2[t] = m2;
  __syncthreads();
  for (int w = kPrepThreads / 2; w > 0; w >>= 1) {
    if (t < w) {
      if (s_lo[t + w] < s_lo[t]) s_lo[t] = s_lo[t + w];
      if (s_hi[t + w] > s_hi[t]) s_hi[t] = s_hi[t + w];
      if (s_e2[t + w] > s_e2[t]) s_e2[t] = s_e2[t + w];
    }
    __syncthreads();
  }
  if (t == 0) {
    const double eps = DBL_EPSILON * 0.5, safmin = DBL_MIN, fudge = 2.1;
    const double pivmin = safmin * (s_e2[0] > 1.0 ? s_e2[0] : 1.0);
    double gl = s_lo[0], gu = s_hi[0];
    const double tnorm = fabs(gl) > fabs(gu) ? fabs(gl) : fabs(gu);
    gl = gl - fudge * tnorm * eps * n - fudge * 2.0 * pivmin;      // (DSTEBZ's widening)
    gu = gu + fudge * tnorm * eps * n + fudge * pivmin;
    const double tol = 2.0 * (2.0 * eps) * tnorm + 2.0 * pivmin;   // 2 eps max(|gl|, |gu|) in LAPACK's eps (2^-52)
    if (tnorm == 0.0) { gl = 0.0; gu = 0.0; }                        // the zero matrix: every eigenvalue is 0, exactly
    // passes: the fewest that bring the cell width under tol (a cell of level p is (gu - gl) / 2^(bits p))
    double w = gu - gl;
    int passes = 0;
    const double shrink = 1.0 / (double)(1 << bits);
    while (w > tol && passes < 64) { w *= shrink; ++passes; }
    params[0] = gl; params[1] = gu; params[2] = pivmin; params[3] = tol; params[4] = (double)passes;
  }
}

// Number of eigenvalues below each of the K points (negative pivots of the LDL^T of T - x I)
template <int K>
__device__ __forceinline__ void sturm_counts(int n, const double *__restrict__ d, const double *__restrict__ e2,
                                             double pivmin, const double (&x)[K], int (&cnt)[K]) {
#pragma clang fp contract(off)
  double q[K];
  const double d0 = d[0];
#pragma unroll
  for (int p = 0; p < K; ++p) {
    double v = d0 - x[p];
    if (fabs(v) < pivmin) v = -pivmin;
    q[p] = v; cnt[p] = v < 0.0 ? 1 : 0;
  }
#pragma unroll 4
  for (int i = 1; i < n; ++i) {
    const double di = d[i], ei = e2[i - 1];
#pragma unroll
    for (int p = 0; p < K; ++p) {
      double v = (di - x[p]) - ei / q[p];
      if (fabs(v) < pivmin) v = -pivmin;
      q[p] = v; cnt[p] += v < 0.0 ? 1 : 0;
    }
  }
}

// one group of G lanes per index k = il + group (1-based); w[k - il] = midpoint of the final cell
template <int G, int K>
__global__ void __launch_bounds__(256) stebz_bisect(int n, const double *__restrict__ d,
                                                   const double *__restrict__ e2,
                                                   const double *__restrict__ params, int il, int m,
                                                   double *__restrict__ w) {
#pragma clang fp contract(off)
  constexpr int S = G * K;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int grp = t / G, g = t % G;
  if (grp >= m) return;                  // (whole groups: G divides the wave)
  const int k = il + grp;
  double lo = params[0], hi = params[1];
  const double pivmin = params[2];
  const int passes = (int)params[4];
  const double inv_s = 1.0 / (double)S;  // (exact: S is a power of two)
  for (int pass = 0; pass < passes; ++pass) {
    const double h = hi - lo;
    double x[K];
    int cnt[K];
#pragma unroll
    for (int p = 0; p < K; ++p) x[p] = lo + h * ((double)(g * K + p) * inv_s);
    sturm_counts<K>(n, d, e2, pivmin, x, cnt);
    // the points below index k form a prefix of j = 0..S-1 (counts are monotone in x): J of them in the group
    int below = 0;
#pragma unroll
    for (int p = 0; p < K; ++p) below += (cnt[p] <= k - 1) ? 1 : 0;
#pragma unroll
    for (int off = 1; off < G; off <<= 1) below += __shfl_xor(below, off, G);
    const int J = below > 0 ? below : 1;           // (x_0 = lo is below k by construction)
    const double nlo = lo + h * ((double)(J - 1) * inv_s);
    const double nhi = (J < S) ? lo + h * ((double)J * inv_s) : hi;
    lo = nlo; hi = nhi;
  }
  if (g == 0) w[grp] = lo + (hi - lo) * 0.5;
}

// out[0] = count(vl) + 1, out[1] = count(vu): the indices il..iu of the eigenvalues in (vl, vu] (iu < il: none).  A bound
// below gl counts 0 and one at or above gu counts n (so -Inf / +Inf are legal); in between the clamped zero pivot counts an
// eigenvalue equal to x as <= x, as DSTEBZ.  The two counts are the two interleaved chains of one lane (K = 2).
__global__ void __launch_bounds__(64) stebz_window_count(int n, const double *__restrict__ d,
                                                         const double *__restrict__ e2,
                                                         const double *__restrict__ params, double vl, double vu,
                                                         int *__restrict__ out) {
#pragma clang fp contract(off)
  if (threadIdx.x != 0) return;
  const double gl = params[0], gu = params[1], pivmin = params[2];
  const double x[2] = {vl < gl ? gl : (vl > gu ? gu : vl), vu < gl ? gl : (vu > gu ? gu : vu)};
  int cnt[2];
  sturm_counts<2>(n, d, e2, pivmin, x, cnt);
  if (vl < gl) cnt[0] = 0; else if (vl >= gu) cnt[0] = n;
  if (vu < gl) cnt[1] = 0; else if (vu >= gu) cnt[1] = n;
  out[0] = cnt[0] + 1;
  out[1] = cnt[1];
}

template <int G>
void launch_bisect(hipStream_t s, int n, const double *d, const double *e2, const double *params, int il, int m,
                   double *w) {
  const int threads = m * G;
  hipLaunchKernelGGL((stebz_bisect<G, kStebzK>), dim3(ceil_div(threads, 256)), dim3(256), 0, s, n, d, e2, params, il,
                     m, w);
}

int log2i(int v) { int b = 0; while ((1 << b) < v) ++b; return b; }

}  // namespace

size_t stebz_work_bytes(int n) { return ((size_t)(n > 0 ? n : 1) * 8 + 255) / 256 * 256 + 256; }

int stebz_set_lanes(int lanes) {
  if (lanes <= 0) { g_stebz_lanes = 4; return 0; }
  if (lanes != 1 && lanes != 2 && lanes != 4 && lanes != 8 && lanes != 16) return -1;
  g_stebz_lanes = lanes;
  return 0;
}

void stebz(hipStream_t s, int n, const double *d, const double *e, int il, int iu, double *w, void *work) {
  if (n <= 0 || iu < il) return;
  double *e2 = (double *)work;
  double *params = (double *)((char *)work + stebz_work_bytes(n) - 256);
  const int G = g_stebz_lanes, m = iu - il + 1;
  hipLaunchKernelGGL(stebz_prep, dim3(1), dim3(kPrepThreads), 0, s, n, d, e, e2, params, log2i(G * kStebzK));
  switch (G) {
    case 1: launch_bisect<1>(s, n, d, e2, params, il, m, w); break;
    case 2: launch_bisect<2>(s, n, d, e2, params, il, m, w); break;
    case 8: launch_bisect<8>(s, n, d, e2, params, il, m, w); break;
    case 16: launch_bisect<16>(s, n, d, e2, params, il, m, w); break;
    default: launch_bisect<4>(s, n, d, e2, params, il, m, w); break;
  }
}

int *stebz_window(hipStream_t s, int n, const double *d, const double *e, double vl, double vu, void *work) {
  double *e2 = (double *)work;
  double *params = (double *)((char *)work + stebz_work_bytes(n) - 256);
  int *out = (int *)(params + 8);            // (the last 256 bytes: params[0..4], then the two indices)
  if (n <= 0) return out;
  const int G = g_stebz_lanes;
  hipLaunchKernelGGL(stebz_prep, dim3(1), dim3(kPrepThreads), 0, s, n, d, e, e2, params, log2i(G * kStebzK));
  hipLaunchKernelGGL(stebz_window_count, dim3(1), dim3(64), 0, s, n, d, e2, params, vl, vu, out);
  return out;
}

}  // namespace ek
