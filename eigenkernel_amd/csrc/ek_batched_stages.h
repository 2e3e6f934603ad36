// ek_batched_stages.h -- what the two kernels of the batched solver share (not installed):
//   ek_batched.hip    orders up to EK_HIP_BATCH_NMAX, the n x n image in LDS, classes NC = 32 / 64 / 128
//   ek_batched_x.hip  orders up to EK_HIP_YBATCH_NMAX, the image in device memory, NC = 256 / 512
// One workgroup of 2 NC threads (NW waves) owns a problem; thread t is (row or column r = t % NC, half sub = t / NC).
//      gdouble, cgdouble, block_reduce
//   0  scan_a       the lower triangle of A is read once for NaN / Inf (info -5) and for max|a|
//   4  rank_sort    the end of stage 4: ascending order as ranks, the overflow exit, w -> dw
// scan_a and rank_sort are called by the whole workgroup with the same arguments and hold barriers; neither touches the
// image.  Everything that does -- the strided axpy and dot, stage 3 (DSYTD2) and the QL loop of stage 4, which are the same
// algorithm in both kernels -- still stands in each kernel: moved here it changed bits or cost time.
#pragma once
#include "ek_api_internal.h"

#include <cfloat>

namespace ek {
namespace bstages {

// Global address space: a pointer that arrives as a kernel argument is known to be global, but one loaded from a table is
// generic to the compiler, which would emit flat loads and stores for it (64-bit addresses in VGPRs, waits shared with
// LDS).  The solver's kernels and the checks' (ek_batched_check.h) type their problems' pointers with these.
typedef __attribute__((address_space(1))) double gdouble;
typedef const __attribute__((address_space(1))) double cgdouble;

// Sum (or maximum) over the workgroup, the same bits in every thread: a butterfly inside the wave, then the waves in
// ascending order.  `red` holds 2 * NW doubles; the two halves alternate so that a call needs one barrier: between two
// uses of a half lies the barrier of the call between them.
template <int NW, bool MAX>
__device__ __forceinline__ double block_reduce(double x, double *red, int &phase) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double y = __shfl_xor(x, o, 64);
    x = MAX ? fmax(x, y) : x + y;
  }
  if (NW == 1) return x;
  double *rr = red + phase * NW;
  phase ^= 1;
  if ((threadIdx.x & 63) == 0) rr[threadIdx.x >> 6] = x;
  __syncthreads();
  double s = rr[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) s = MAX ? fmax(s, rr[w]) : s + rr[w];
  return s;
}

// ---- 0: A finite?  max|a| comes off the same pass: an A whose squares would leave the normal range is scaled.  The
// image of stage 2 holds 2^-aex A; d, e and w go out times 2^aex.  False: the problem ended with info = -5.
template <int NC, int NW>
__device__ __forceinline__ bool scan_a(const gdouble *A, int lda, int n, double *red, int &phase, int *info, int &aex) {
  const int t = threadIdx.x, r = t % NC, sub = t / NC;
  aex = 0;
  double mx = 0.0;
  if (r < n)
    for (int j = sub; j <= r; j += 2) {
      const double ax = fabs(A[r + (size_t)j * lda]);
      mx = (ax <= DBL_MAX) ? fmax(mx, ax) : INFINITY;   // a NaN counts as Inf: fmax would drop it
    }
  const double amax = block_reduce<NW, true>(mx, red, phase);
  if (!(amax <= DBL_MAX)) {                         // uniform: amax has the same bits in every thread
    if (t == 0) *info = -5;
    return false;
  }
  // Stage 3 forms plain sums of squares (DSYEV scales for the same reason, and so does ek_solve.hip's stage_in_A).
  // Inside 2^-256 .. 2^256 nothing is done and the arithmetic is the unscaled kernel's to the bit: there the square
  // of every entry down to eps / n of max|a| is a normal number (>= 2^-632) and n^1.5 max|a|^2 is finite (<= 2^523),
  // and the other half of the exponent range is left to what L^-1 . L^-T amplifies (1 / lambda_min(B) up to 2^250).
  // Outside, max|a| goes to [1/2, 1) by an exact power of two (not by rmin / anrm as DSYEV does), so that the
  // result is that of the scaled matrix to the bit.
  if (amax > 0.0 && (amax < 0x1p-256 || amax > 0x1p256)) (void)frexp(amax, &aex);
  return true;
}

// Ascending order: rank sort (ties by index; a NaN sorts last so that the ranks stay a permutation), w = 2^wex d -> dw.
// False: an eigenvalue beyond the range of a double (or a NaN that QL made) is reported like a reduction that
// overflowed, info = 100000 + n + 1, and nothing is written.
template <int NC>
__device__ __forceinline__ bool rank_sort(int n, int wex, const double *sd, int *srank, gdouble *w, int *info) {
  const int t = threadIdx.x, r = t % NC, sub = t / NC;
  int rank = 0, bad = 0;
  double wr = 0.0;
  if (sub == 0 && r < n) {
    const double di = sd[r], ki = (di == di) ? di : INFINITY;
    for (int j = 0; j < n; ++j) {
      const double dj = sd[j], kj = (dj == dj) ? dj : INFINITY;
      rank += (kj < ki || (kj == ki && j < r)) ? 1 : 0;
    }
    srank[r] = rank;
    wr = ldexp(di, wex);                            // one rounding at most (a denormal result), as di * 2^ex had
    bad = !(fabs(wr) <= DBL_MAX);
  }
  if (__syncthreads_or(bad)) {
    if (t == 0) *info = 100000 + n + 1;
    return false;
  }
  if (sub == 0 && r < n) w[rank] = wr;
  return true;
}

}  // namespace bstages
}  // namespace ek
