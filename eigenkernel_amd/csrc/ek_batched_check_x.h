// ek_batched_check_x.h -- what the two translation units of the batched checks above EK_HIP_BATCH_NMAX share (not
// installed): the shape of a workgroup, the staged tiles, their loaders and the step on the fp64 matrix cores.
//   ek_batched_check_x.hip       ek_hip_check_xbatched*: the standard problem and type 1
//   ek_batched_check_sygv_x.hip  ek_hip_check_sygv_xbatched*: DSYGV's types 2 and 3
// Everything here is inlined into its caller; the code generated for the first unit is what it was before the second
// existed (DESIGN.md 20 records the comparison).
// Both units hold a kernel, its launch and thin entries; their host side is the driver of ek_batched_check.h.
#pragma once
#include "ek_batched_check.h"

namespace ek {
namespace xcheck {

using bcheck::cgdouble;
using bcheck::gdouble;
using bcheck::wg_reduce;
typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int T = 512, NW = T / 64;                 // threads, waves
constexpr int TM = 128, TN = 64, KT = 16;           // output tile, step of the inner dimension
constexpr int LDP = TM + 16, LDQ = TN + 16;         // leading dimensions of the staged tiles [k][row], [k][column]: 16 mod 32,
                                                    // so that the four k of an operand read fall on different banks
constexpr int kTileP = KT * LDP, kTileQ = KT * LDQ;
static_assert(TM == 16 * NW, "a wave per 16 rows of the tile");
static_assert(EK_HIP_XBATCH_NMAX % TN == 0 && EK_HIP_XBATCH_NMAX <= T, "a thread per column in the reductions");

// ---- loaders: global -> registers (tile), registers -> LDS (put).  Thread t of a symmetric tile: half = t / 256 takes the
// 16 x 16 blocks 2 q + half, q = 0 .. 3, as (a, b) = (t % 16, t / 16 % 16)
__device__ __forceinline__ void sym_tile(cgdouble *M, int ld, int n, int i0, int k0, double (&v)[4]) {
  const int t = threadIdx.x, half = t >> 8, a = t & 15, b = (t >> 4) & 15;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int ib = i0 + 16 * (2 * q + half);
    const bool low = ib >= k0;                      // on or below the diagonal: along i; above it: the mirrored block along k
    const int i = ib + (low ? a : b), k = k0 + (low ? b : a);
    // the load is unconditional: past n it takes the last row or column (inside the lower triangle) and is dropped
    const int ic = min(i, n - 1), kc = min(k, n - 1), hi = max(ic, kc), lo = min(ic, kc);
    const double x = M[hi + (size_t)lo * ld];
    v[q] = (i < n && k < n) ? x : 0.0;
  }
}
__device__ __forceinline__ void sym_put(double *s, int i0, int k0, const double (&v)[4]) {
  const int t = threadIdx.x, half = t >> 8, a = t & 15, b = (t >> 4) & 15;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int blk = 16 * (2 * q + half);
    s[(i0 + blk >= k0) ? b * LDP + blk + a : a * LDP + blk + b] = v[q];
  }
}
// KT x W tile of a column-major matrix, rows k0 .. (the inner dimension), columns c0 ..: along k
template <int W>
__device__ __forceinline__ void col_tile(cgdouble *M, int ld, int n, int k0, int c0, double (&v)[W / 32]) {
  const int t = threadIdx.x, k = k0 + (t & 15);
#pragma unroll
  for (int q = 0; q < W / 32; ++q) {
    const int c = c0 + (t >> 4) + 32 * q;
    const double x = M[min(k, n - 1) + (size_t)min(c, n - 1) * ld];   // unconditional, as above
    v[q] = (k < n && c < n) ? x : 0.0;
  }
}
template <int W, int LD>
__device__ __forceinline__ void col_put(double *s, const double (&v)[W / 32]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int q = 0; q < W / 32; ++q) s[(t & 15) * LD + (t >> 4) + 32 * q] = v[q];
}

// one step of 16 of the inner dimension: acc += P^T-tile rows of this wave x Q-tile
template <bool TWO>
__device__ __forceinline__ void step_mfma(const double *sp, const double *sp2, const double *sq, double4_t (&acc)[4],
                                          double4_t (&acc2)[4]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4;
#pragma unroll
  for (int kk = 0; kk < KT; kk += 4) {
    const double x = sp[(kk + l4) * LDP + 16 * wave + l15];
    const double x2 = TWO ? sp2[(kk + l4) * LDP + 16 * wave + l15] : 0.0;
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
      const double y = sq[(kk + l4) * LDQ + 16 * jt + l15];
      acc[jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, acc[jt], 0, 0, 0);
      if (TWO) acc2[jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(x2, y, acc2[jt], 0, 0, 0);
    }
  }
}

// x - w s with the product rounded on its own, whatever the compiler contracts elsewhere: (A Z)_ij and w_j s_ij that agree
// as doubles give a residual of exactly zero
__device__ __forceinline__ double minus_product(double x, double w, double s) {
#pragma clang fp contract(off)
  const double p = w * s;
  return x - p;
}

}  // namespace xcheck
}  // namespace ek
