// ek_batched_check_x.h -- the batched checks on the fp64 matrix cores (not installed): the shape of a workgroup, the staged
// tiles, their loaders, the step, the products, the passes and the two kernel bodies, each once.  Four
// translation units instantiate the kernels, each with its uniform Args, its launches and its entries:
//   ek_batched_check_x.hip            check_kernel<GEN, false, .>: the standard problem and type 1 above EK_HIP_BATCH_NMAX
//   ek_batched_check_sygv_x.hip       check_sygv_kernel<ITYPE, false, .>: DSYGV's types 2 and 3 above EK_HIP_BATCH_NMAX
//   ek_batched_check_window.hip       check_kernel<GEN, true, .>: the c = m[b] columns of a window, every order
//   ek_batched_check_sygv_window.hip  check_sygv_kernel<ITYPE, true, .>: the same for types 2 and 3
// Everything but the kernels is inlined into its caller.  The host side is the drivers of ek_batched_check.h.
//
// One workgroup of 512 threads (8 waves) owns a problem from its first load to its last store.  At these orders neither Z
// nor a product with it fits in LDS, so the n^2 c products run on the matrix cores (v_mfma_f64_16x16x4_f64) over LDS-staged
// tiles: an output tile has 128 rows x 64 columns, wave v owns its rows 16 v .. 16 v + 15 (its strip) as four 16 x 16
// accumulator subtiles, and the inner dimension advances 16 at a time through two LDS buffers (the next step's operands
// travel global -> registers while this step's are multiplied, then go to the other buffer: one barrier per step).
//
// RECT = false: the full check, c = n.  Every strip and subtile is multiplied, the ragged ones against staged zeros.
// RECT = true: the columns 0 .. c-1 of Z and the first c of w alone (1 <= c <= n); a strip that lies wholly past the last
// row and a subtile wholly past column c issue no matrix instruction, so a window of c <= 16, 32, 48 columns pays for a tile
// of that width and the ragged last row tile of n = 129 for one strip; type 3's factor and solve are split over the
// threads by (n, c).  Nothing of w or Z from c on is read.
//
// Same bits wherever a problem sits: every loop bound, every skipped strip, every split and every summation order depends
// on (n, c) alone; no atomics; the same kernel behind the host and the device form.  A, B, w and Z are read only; nothing
// strictly above a diagonal, at or beyond row n or between the problems is read.
#pragma once
#include "ek_batched_check.h"

namespace ek {
namespace xcheck {

using bcheck::cgdouble;
using bcheck::gdouble;
using bcheck::wg_reduce;
typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int NX = EK_HIP_XBATCH_NMAX;
constexpr int T = 512, NW = T / 64;                 // threads, waves
constexpr int TM = 128, TN = 64, KT = 16;           // output tile, step of the inner dimension
constexpr int LDP = TM + 16, LDQ = TN + 16;         // leading dimensions of the staged tiles [k][row], [k][column]: 16 mod 32,
                                                    // so that the four k of an operand read fall on different banks
constexpr int kTileP = KT * LDP, kTileQ = KT * LDQ;
static_assert(TM == 16 * NW, "a wave per 16 rows of the tile");
static_assert(NX % TN == 0 && T == 2 * NX, "a thread per column in the reductions, at least two in type 3's factor and solve");

// ---- loaders: global -> registers (tile), registers -> LDS (put).  Thread t of a symmetric tile: half = t / 256 takes the
// 16 x 16 blocks 2 q + half, q = 0 .. 3, as (a, b) = (t % 16, t / 16 % 16).  A block below the diagonal is read along i, one
// above it as the mirrored block along k and transposed on its way into LDS, the diagonal block entry by entry
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
// KT x W tile of a column-major rows x cols matrix, rows k0 .. (the inner dimension), columns c0 ..: along k
template <int W>
__device__ __forceinline__ void col_tile(cgdouble *M, int ld, int rows, int cols, int k0, int c0, double (&v)[W / 32]) {
  const int t = threadIdx.x, k = k0 + (t & 15);
#pragma unroll
  for (int q = 0; q < W / 32; ++q) {
    const int c = c0 + (t >> 4) + 32 * q;
    // unconditional, as above: past the edge it takes the last row or column that exists and is dropped
    const double x = M[min(k, rows - 1) + (size_t)min(c, cols - 1) * ld];
    v[q] = (k < rows && c < cols) ? x : 0.0;
  }
}
template <int W, int LD>
__device__ __forceinline__ void col_put(double *s, const double (&v)[W / 32]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int q = 0; q < W / 32; ++q) s[(t & 15) * LD + (t >> 4) + 32 * q] = v[q];
}
// the same tile of the TRANSPOSE of a column-major cols x rows matrix: entry (k, c) is M[c + k ld], along c
template <int W>
__device__ __forceinline__ void row_tile(cgdouble *M, int ld, int rows, int cols, int k0, int c0, double (&v)[W / 32]) {
  const int t = threadIdx.x, c = c0 + t % W;
#pragma unroll
  for (int q = 0; q < W / 32; ++q) {
    const int k = k0 + t / W + (T / W) * q;
    const double x = M[min(c, cols - 1) + (size_t)min(k, rows - 1) * ld];
    v[q] = (k < rows && c < cols) ? x : 0.0;
  }
}
template <int W, int LD>
__device__ __forceinline__ void row_put(double *s, const double (&v)[W / 32]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int q = 0; q < W / 32; ++q) s[(t / W + (T / W) * q) * LD + t % W] = v[q];
}

// ---- one step of 16 of the inner dimension for this wave's strip: acc += P^T-tile rows x the first NSUB subtiles of the
// Q-tile; TWO: a second P tile against the same Q into acc2 (A and B against one staged tile of Z)
template <int NSUB, bool TWO>
__device__ __forceinline__ void step_subtiles(const double *sp, const double *sp2, const double *sq, int wave,
                                              double4_t (&acc)[4], double4_t (&acc2)[4]) {
  const int lane = threadIdx.x & 63, l15 = lane & 15, l4 = lane >> 4;
#pragma unroll
  for (int kk = 0; kk < KT; kk += 4) {
    const double x = sp[(kk + l4) * LDP + 16 * wave + l15];
    const double x2 = TWO ? sp2[(kk + l4) * LDP + 16 * wave + l15] : 0.0;
#pragma unroll
    for (int jt = 0; jt < NSUB; ++jt) {
      const double y = sq[(kk + l4) * LDQ + 16 * jt + l15];
      acc[jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, acc[jt], 0, 0, 0);
      if (TWO) acc2[jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(x2, y, acc2[jt], 0, 0, 0);
    }
  }
}
// Which subtiles a step multiplies.  kAll: the four of the tile, every strip (the full checks).  The window checks skip a
// strip that holds no row and the subtiles past column c (nsub of them are live, the same count in the whole workgroup):
// kSwitch takes one straight-line body per count, kTests one body with a test per subtile.  Both stay, because each costs
// the other's kernels registers: check_sygv_kernel needs 208 VGPRs with kSwitch, and 256 and 16 bytes of
// scratch with kTests; check_kernel needs 190 (GEN) and 162 with kTests, and with kSwitch 256 and 20 bytes of scratch
// (GEN) and 202
enum Step { kAll, kSwitch, kTests };
template <Step STEP, bool TWO>
__device__ __forceinline__ void step(const double *sp, const double *sp2, const double *sq, int wave, bool strip, int nsub,
                                     double4_t (&acc)[4], double4_t (&acc2)[4]) {
  if (STEP == kAll) {
    // the wave from threadIdx.x, unsigned, and not the kernel's int: with that one the compiler pairs the LDS reads of a
    // step differently, and the full checks of types 2 and 3 ran 0.5 .. 0.9 % slower
    step_subtiles<4, TWO>(sp, sp2, sq, threadIdx.x >> 6, acc, acc2);
  } else if (STEP == kSwitch) {
    if (strip) switch (nsub) {
      case 1: step_subtiles<1, TWO>(sp, sp2, sq, wave, acc, acc2); break;
      case 2: step_subtiles<2, TWO>(sp, sp2, sq, wave, acc, acc2); break;
      case 3: step_subtiles<3, TWO>(sp, sp2, sq, wave, acc, acc2); break;
      default: step_subtiles<4, TWO>(sp, sp2, sq, wave, acc, acc2); break;
    }
  } else if (strip) {                               // step_subtiles<4, TWO> with the test; folded into it, the code changes
    const int lane = threadIdx.x & 63, l15 = lane & 15, l4 = lane >> 4;
#pragma unroll
    for (int kk = 0; kk < KT; kk += 4) {
      const double x = sp[(kk + l4) * LDP + 16 * wave + l15];
      const double x2 = TWO ? sp2[(kk + l4) * LDP + 16 * wave + l15] : 0.0;
#pragma unroll
      for (int jt = 0; jt < 4; ++jt)
        if (jt < nsub) {
          const double y = sq[(kk + l4) * LDQ + 16 * jt + l15];
          acc[jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, acc[jt], 0, 0, 0);
          if (TWO) acc2[jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(x2, y, acc2[jt], 0, 0, 0);
        }
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

// ---- the pieces of a pass.  KB: the doubles of one LDS buffer, KQ: where its Q tile starts (the P tile starts at 0)
// acc <- tile (i0, j0) of M Q: M symmetric of order n, its lower triangle referenced; Q column-major n x c.  With `squares`
// the squares of the staged entries of M are added to sq.  Ends behind a barrier: the buffers are free
template <Step STEP, int KB, int KQ>
__device__ __forceinline__ void sym_product(cgdouble *M, int ldm, cgdouble *Q, int ldq, int n, int c, int i0, int j0,
                                            int wave, double *buf, double4_t (&acc)[4], bool squares, double &sq) {
  const int nk = (n + KT - 1) / KT, nsub = min(4, (c - j0 + 15) >> 4);
  const bool strip = i0 + 16 * wave < n;
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) acc[jt] = (double4_t){0.0, 0.0, 0.0, 0.0};
  double vm[4], vq[2];
  auto fetch = [&](int k0) {
    sym_tile(M, ldm, n, i0, k0, vm);
    col_tile<TN>(Q, ldq, n, c, k0, j0, vq);
  };
  auto put = [&](int k0, double *s) {
    sym_put(s, i0, k0, vm);
    col_put<TN, LDQ>(s + KQ, vq);
    if (squares) {
#pragma unroll
      for (int q = 0; q < 4; ++q) sq = fma(vm[q], vm[q], sq);
    }
  };
  fetch(0);
  put(0, buf);
  __syncthreads();
#pragma unroll 1
  for (int s = 0; s < nk; ++s) {
    const double *cur = buf + (s & 1) * KB;
    const bool more = s + 1 < nk;
    if (more) fetch((s + 1) * KT);
    step<STEP, false>(cur, cur, cur + KQ, wave, strip, nsub, acc, acc);
    if (more) put((s + 1) * KT, buf + ((s + 1) & 1) * KB);
    __syncthreads();
  }
}

// The sum over a tile's rows of three per-column values of the epilogue (check_kernel holds the same sums inline): in the wave over the four lane >> 4 groups, over
// the waves in ascending order through cs; thread x < TN returns column j0 + x's sums in x0 .. x2.  Ends behind a barrier
// for the threads that read; the next write of cs lies behind the next tile's barriers
__device__ __forceinline__ void column_sums(double (&c0)[4], double (&c1)[4], double (&c2)[4], double *cs, int wave,
                                            double &x0, double &x1, double &x2) {
  const int t = threadIdx.x, lane = t & 63, l15 = lane & 15, l4 = lane >> 4;
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) {
    double a = c0[jt], b = c1[jt], c = c2[jt];
    a += __shfl_xor(a, 16, 64); a += __shfl_xor(a, 32, 64);
    b += __shfl_xor(b, 16, 64); b += __shfl_xor(b, 32, 64);
    c += __shfl_xor(c, 16, 64); c += __shfl_xor(c, 32, 64);
    if (l4 == 0) {
      cs[(0 * NW + wave) * TN + 16 * jt + l15] = a;
      cs[(1 * NW + wave) * TN + 16 * jt + l15] = b;
      cs[(2 * NW + wave) * TN + 16 * jt + l15] = c;
    }
  }
  __syncthreads();
  x0 = x1 = x2 = 0.0;
  if (t < TN) {
    x0 = cs[t]; x1 = cs[NW * TN + t]; x2 = cs[2 * NW * TN + t];
#pragma unroll
    for (int v = 1; v < NW; ++v) {
      x0 += cs[(0 * NW + v) * TN + t];
      x1 += cs[(1 * NW + v) * TN + t];
      x2 += cs[(2 * NW + v) * TN + t];
    }
  }
}

// sum over l != j of (G_lj sg_l sg_j)^2 of this thread's entries, G = P^T Q of order c with the inner dimension n, both
// operands from global memory, over the c x c tiles only (ROWS: P^T and Q^T are what lies in memory, c x n, their rows
// are read: consecutive addresses along the columns).  check_kernel holds the sum with ROWS = false inline
template <bool ROWS, Step STEP, int KB, int KQ>
__device__ __forceinline__ double gram_offdiag(cgdouble *P, int ldp, cgdouble *Q, int ldq, int n, int c, int wave,
                                               double *buf, const double *sg) {
  const int lane = threadIdx.x & 63, l15 = lane & 15, l4 = lane >> 4;
  const int nk = (n + KT - 1) / KT;
  double os = 0.0;
#pragma unroll 1
  for (int j0 = 0; j0 < c; j0 += TN) {
    const int nsub = min(4, (c - j0 + 15) >> 4);
#pragma unroll 1
    for (int l0 = 0; l0 < c; l0 += TM) {
      const bool strip = l0 + 16 * wave < c;
      double4_t acc[4];
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) acc[jt] = (double4_t){0.0, 0.0, 0.0, 0.0};
      double vp[4], vq[2];
      auto fetch = [&](int k0) {
        if (ROWS) {
          row_tile<TM>(P, ldp, n, c, k0, l0, vp);
          row_tile<TN>(Q, ldq, n, c, k0, j0, vq);
        } else {
          col_tile<TM>(P, ldp, n, c, k0, l0, vp);
          col_tile<TN>(Q, ldq, n, c, k0, j0, vq);
        }
      };
      auto put = [&](double *s) {
        if (ROWS) {
          row_put<TM, LDP>(s, vp);
          row_put<TN, LDQ>(s + KQ, vq);
        } else {
          col_put<TM, LDP>(s, vp);
          col_put<TN, LDQ>(s + KQ, vq);
        }
      };
      fetch(0);
      put(buf);
      __syncthreads();
#pragma unroll 1
      for (int s = 0; s < nk; ++s) {
        const double *cur = buf + (s & 1) * KB;
        const bool more = s + 1 < nk;
        if (more) fetch((s + 1) * KT);
        step<STEP, false>(cur, cur, cur + KQ, wave, strip, nsub, acc, acc);
        if (more) put(buf + ((s + 1) & 1) * KB);
        __syncthreads();
      }
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        const int j = j0 + 16 * jt + l15;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int l = l0 + 16 * wave + l4 + 4 * r;
          if (l < c && j < c && l != j) {
            const double g = acc[jt][r] * sg[l] * sg[j];
            os = fma(g, g, os);
          }
        }
      }
    }
  }
  return os;
}

// y[i sy] -= x[i] a for i = i0, i0 + st, ... < i1; y in the scratch, x in LDS: eight loads before the first store.  The
// update is one fma wherever it is written, so an entry's bits do not depend on which loop reaches it
__device__ __forceinline__ void img_axpy(gdouble *y, int sy, const double *x, double a, int i0, int i1, int st) {
  int i = i0;
  for (; i + 7 * st < i1; i += 8 * st) {
    double yv[8], xv[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) yv[q] = y[(i + q * st) * sy];
#pragma unroll
    for (int q = 0; q < 8; ++q) xv[q] = x[i + q * st];
#pragma unroll
    for (int q = 0; q < 8; ++q) y[(i + q * st) * sy] = fma(-xv[q], a, yv[q]);
  }
  for (; i < i1; i += st) y[i * sy] = fma(-x[i], a, y[i * sy]);
}

// ---- what the units' uniform Args have in common: problem pb of a strided batch, c columns of it, sS doubles of scratch
// per workgroup of the launch.  pencil = false: neither B nor a scratch
template <typename ARGS>
__device__ __forceinline__ bcheck::Problem strided(const ARGS &a, long long pb, int c, bool pencil, long long sS) {
  return {a.n, c, (cgdouble *)(a.A + pb * a.sA), a.lda, pencil ? (cgdouble *)(a.B + pb * a.sB) : nullptr, a.ldb,
          (cgdouble *)(a.w + pb * a.n), (cgdouble *)(a.Z + pb * a.sZ), a.ldz,
          pencil ? (gdouble *)(a.S + (long long)blockIdx.x * sS) : nullptr, (gdouble *)(a.out + pb * EK_HIP_CHECK_NOUT),
          a.ipr ? (gdouble *)(a.ipr + pb * a.n) : nullptr};
}

// LDS doubles of the two kernels: two buffers, the waves' column sums, the words per column, a word per wave
constexpr int kBuf = 2 * kTileP + kTileQ;           // A, B, Z of one step (pass 2: Z^T, unused, S)
constexpr int kLdsDoubles = 2 * kBuf + 3 * NW * TN + NX + NW;
constexpr int kBufSygv = kTileP + kTileQ;           // the two operands of one step
constexpr int kLdsDoublesSygv = 2 * kBufSygv + 3 * NW * TN + 4 * NX + NW;
static_assert(2 * kBufSygv >= 3 * NX, "the factor's vectors fit in the buffers");

// ---- the standard problem (GEN = false) and A x = l B x (GEN = true): a_norm, res_ave, res_max, orthogonality, IPRs
//   1  over the column tiles j0 < c and the row tiles i0 < n: A Z and, for a generalized problem, S = B Z in the same sweep
//      (one staged tile of Z feeds both).  The squares of the staged entries of A of the first column tile give ||A||_F.
//      The epilogue works in the accumulators: r_ij = (A Z)_ij - w_j s_ij, and r^2, z s and z^4 are summed per column -- in
//      the lane over its four rows, in the wave over the four lane >> 4 groups, over the waves in ascending order through
//      LDS, over the row tiles in ascending order.  S goes to a device scratch of n x c doubles, leading dimension n (a
//      standard problem has S = Z and needs neither the scratch nor the second accumulators)
//   2  G = Z^T S over the c x c tiles, inner dimension n; entry (l, j), l != j, is scaled by G_ll^-1/2 G_jj^-1/2 from
//      step 1, squared and added to its thread's sum in tile order
// ARGS: how the workgroup finds its problem -- a unit's Args (one order, strided; the scratch by workgroup) or bcheck::VArgs
// (entry blockIdx.x of the launch's slice of the table, which names the entry's order, its m and its own scratch)
template <bool GEN, bool RECT, typename ARGS>
__global__ __launch_bounds__(T) void check_kernel(ARGS a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  constexpr int kB = kBuf, kQ = 2 * kTileP;         // a buffer; where its tile of Z (or S) starts
  constexpr Step STEP = RECT ? kTests : kAll;       // see Step
  double *buf = smem;                               // [2][kB]
  double *cs = buf + 2 * kB;                        // [3][NW][TN]: the waves' column sums
  double *sg = cs + 3 * NW * TN;                    // 1 / sqrt(G_jj)
  double *red = sg + NX;                            // a word per wave

  const int t = threadIdx.x, lane = t & 63;
  // RECT: scalar, so that a skipped strip is a branch, not a mask
  const int wave = RECT ? __builtin_amdgcn_readfirstlane(t >> 6) : t >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  const bcheck::Problem p = locate(a, (int)GEN);
  const int n = p.n, c = RECT ? p.c : n;
  cgdouble *A = p.A;
  cgdouble *B = GEN ? p.B : nullptr;
  cgdouble *w = p.w;
  cgdouble *Z = p.Z;
  gdouble *S = GEN ? p.S : nullptr;
  gdouble *out = p.out;
  gdouble *ipr = p.ipr;
  const int lda = p.lda, ldb = p.ldb, ldz = p.ldz;
  const int nk = (n + KT - 1) / KT;

  // ---- 1: A Z, S = B Z, per column ||r_j||^2, G_jj, sum z^4; ||A||_F^2
  double asq = 0.0, rsum = 0.0, rmax = 0.0;
#pragma unroll 1
  for (int j0 = 0; j0 < c; j0 += TN) {
    const int nsub = min(4, (c - j0 + 15) >> 4);
    double wj[4];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
      const int j = j0 + 16 * jt + l15;
      wj[jt] = (j < c) ? w[j] : 0.0;
    }
    double tr = 0.0, tg = 0.0, tp = 0.0;            // thread x < TN: column j0 + x, over the row tiles
#pragma unroll 1
    for (int i0 = 0; i0 < n; i0 += TM) {
      const bool strip = i0 + 16 * wave < n;
      double4_t accA[4], accB[4];
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) accA[jt] = accB[jt] = (double4_t){0.0, 0.0, 0.0, 0.0};
      double va[4], vb[4], vz[2];
      auto fetch = [&](int k0) {
        sym_tile(A, lda, n, i0, k0, va);
        if (GEN) sym_tile(B, ldb, n, i0, k0, vb);
        col_tile<TN>(Z, ldz, n, c, k0, j0, vz);
      };
      auto put = [&](int k0, double *s) {
        sym_put(s, i0, k0, va);
        if (GEN) sym_put(s + kTileP, i0, k0, vb);
        col_put<TN, LDQ>(s + kQ, vz);
        if (j0 == 0) {
#pragma unroll
          for (int q = 0; q < 4; ++q) asq = fma(va[q], va[q], asq);
        }
      };
      fetch(0);
      put(0, buf);
      __syncthreads();
#pragma unroll 1
      for (int s = 0; s < nk; ++s) {
        const double *cur = buf + (s & 1) * kB;
        const bool more = s + 1 < nk;
        if (more) fetch((s + 1) * KT);
        step<STEP, GEN>(cur, cur + kTileP, cur + kQ, wave, strip, nsub, accA, accB);
        if (more) put((s + 1) * KT, buf + ((s + 1) & 1) * kB);
        __syncthreads();
      }
      // the epilogue, in the accumulators: acc[jt][r] is entry (i0 + 16 wave + l4 + 4 r, j0 + 16 jt + l15).  The sums are
      // column_sums' own, in its order, written out a subtile at a time: so the compiler emits the code these kernels had
      // before the pieces were shared; through column_sums it does not, and that form was not timed alone
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        const int j = j0 + 16 * jt + l15;
        double cr = 0.0, cg = 0.0, cp = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = i0 + 16 * wave + l4 + 4 * r;
          if (i < n && j < c) {
            const double z = Z[i + (size_t)j * ldz];
            const double sv = GEN ? accB[jt][r] : z;
            const double rr = minus_product(accA[jt][r], wj[jt], sv);
            const double z2 = z * z;
            cr = fma(rr, rr, cr);
            cg = fma(z, sv, cg);
            cp = fma(z2, z2, cp);
            if (GEN) S[i + (size_t)j * n] = sv;
          }
        }
        cr += __shfl_xor(cr, 16, 64); cr += __shfl_xor(cr, 32, 64);
        cg += __shfl_xor(cg, 16, 64); cg += __shfl_xor(cg, 32, 64);
        cp += __shfl_xor(cp, 16, 64); cp += __shfl_xor(cp, 32, 64);
        if (l4 == 0) {
          cs[(0 * NW + wave) * TN + 16 * jt + l15] = cr;
          cs[(1 * NW + wave) * TN + 16 * jt + l15] = cg;
          cs[(2 * NW + wave) * TN + 16 * jt + l15] = cp;
        }
      }
      __syncthreads();
      if (t < TN) {                                 // the next write of cs lies behind the next tile's barriers
        double xr = cs[t], xg = cs[NW * TN + t], xp = cs[2 * NW * TN + t];
#pragma unroll
        for (int v = 1; v < NW; ++v) {
          xr += cs[(0 * NW + v) * TN + t];
          xg += cs[(1 * NW + v) * TN + t];
          xp += cs[(2 * NW + v) * TN + t];
        }
        tr += xr; tg += xg; tp += xp;
      }
    }
    if (t < TN && j0 + t < c) {
      const double rn = sqrt(tr);
      sg[j0 + t] = 1.0 / sqrt(tg);
      if (ipr) ipr[j0 + t] = tp / (tg * tg);
      rsum += rn;
      rmax = (rn > rmax || rn != rn) ? rn : rmax;
    }
  }
  rsum = wg_reduce<NW, false>(rsum, red);
  rmax = wg_reduce<NW, true>(rmax, red);
  const double anorm = sqrt(wg_reduce<NW, false>(asq, red));
  __syncthreads();                                  // sg is written, S is in the scratch for the whole workgroup

  // ---- 2: || D^-1/2 G D^-1/2 - its diagonal ||_F, G = Z^T S of order c
  cgdouble *Q = GEN ? (cgdouble *)S : Z;
  const int ldq = GEN ? n : ldz;
  // gram_offdiag<false, .>(Z, ldz, Q, ldq, ...) written out: called, it is the same sum, but in check_kernel<true, false, .>
  // the compiler then waits for every LDS read of the step before the first matrix instruction, and the full check of
  // problem 1 ran 1.4 .. 2.0 % slower than before
  double os = 0.0;
#pragma unroll 1
  for (int j0 = 0; j0 < c; j0 += TN) {
    const int nsub = min(4, (c - j0 + 15) >> 4);
#pragma unroll 1
    for (int l0 = 0; l0 < c; l0 += TM) {
      const bool strip = l0 + 16 * wave < c;
      double4_t acc[4];
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) acc[jt] = (double4_t){0.0, 0.0, 0.0, 0.0};
      double vp[4], vq[2];
      col_tile<TM>(Z, ldz, n, c, 0, l0, vp);
      col_tile<TN>(Q, ldq, n, c, 0, j0, vq);
      col_put<TM, LDP>(buf, vp);
      col_put<TN, LDQ>(buf + kQ, vq);
      __syncthreads();
#pragma unroll 1
      for (int s = 0; s < nk; ++s) {
        const double *cur = buf + (s & 1) * kB;
        double *nxt = buf + ((s + 1) & 1) * kB;
        const bool more = s + 1 < nk;
        if (more) {
          col_tile<TM>(Z, ldz, n, c, (s + 1) * KT, l0, vp);
          col_tile<TN>(Q, ldq, n, c, (s + 1) * KT, j0, vq);
        }
        step<STEP, false>(cur, cur, cur + kQ, wave, strip, nsub, acc, acc);
        if (more) {
          col_put<TM, LDP>(nxt, vp);
          col_put<TN, LDQ>(nxt + kQ, vq);
        }
        __syncthreads();
      }
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        const int j = j0 + 16 * jt + l15;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int l = l0 + 16 * wave + l4 + 4 * r;
          if (l < c && j < c && l != j) {
            const double g = acc[jt][r] * sg[l] * sg[j];
            os = fma(g, g, os);
          }
        }
      }
    }
  }
  const double osum = wg_reduce<NW, false>(os, red);
  if (t == 0) {
    out[0] = anorm;
    out[1] = rsum / anorm / (double)c;
    out[2] = rmax / anorm;
    out[3] = sqrt(osum);
  }
}

// ---- DSYGV's types 2 (A B x = l x) and 3 (B A x = l x); the quantities are those of DESIGN.md 16.  S and W live in the
// device scratch: n c doubles (type 2) or n^2 + n c (type 3), leading dimension n
//   type 2   1  S = B Z to the scratch; per column G_jj = sum z s, sum z^4, ||z_j||^2; ||B||_F^2.  Tile order, K step,
//               epilogue and reduction order are those of the B side of check_kernel<true, .>
//            2  R = A S - fl(w_j z_ij) in the accumulators (minus_product), ||r_j||^2 per column; ||A||_F^2
//            3  G = Z^T S: pass 2 of check_kernel.  Slot 3 and the IPRs are type 1's bits for the same (B, Z, c)
//   type 3   1  U = A Z to the first n c doubles of the scratch; sum z^4, ||z_j||^2; ||A||_F^2
//            2  R = B U - fl(w_j z_ij); ||B||_F^2
//            3  B = L L^T from the caller's lower triangle into the first n^2 of the scratch (U is dead): right-looking,
//               512 / NR threads per row, the scaled column of a step kept in LDS; a pivot takes a square root and a
//               division.  RECT: NR = 64, 128 or 256, the power of two that holds n; otherwise 256.  A pivot that is not
//               positive and finite ends the type's part for the whole workgroup (the word is the same in every thread):
//               slot 3 and the c IPRs are NaN, the residual slots stand
//            4  W = L^-1 Z for the c columns, kept TRANSPOSED (c x n, leading dimension c) behind the factor: a column of
//               L a step, staged in LDS a step ahead, axpy form with eight loads in flight.  A column of W belongs to
//               512 / CP threads.  RECT: CP is the power of two (at least 16) that holds c: 2 threads at c > 128, 32 at
//               c <= 16; otherwise 256.  Every thread of a group carries the pivot and G_jj = sum_i w_ij^2 itself and takes
//               every (512 / CP)-th entry of the axpy; an entry's updates come in the order of the steps whoever applies
//               them, and nothing is summed across threads
//            5  G = W^T W of order c, both operands from rows of the transposed image
template <int ITYPE, bool RECT, typename ARGS>
__global__ __launch_bounds__(T) void check_sygv_kernel(ARGS a) {
  static_assert(ITYPE == 2 || ITYPE == 3, "type 1 is check_kernel<true, .>");
  extern __shared__ __attribute__((aligned(16))) double smem[];
  constexpr int kB = kBufSygv, kQ = kTileP;
  constexpr Step STEP = RECT ? kSwitch : kAll;      // see Step
  double *buf = smem;                               // [2][kB]
  double *cs = buf + 2 * kB;                        // [3][NW][TN]: the waves' column sums
  double *sg = cs + 3 * NW * TN;                    // 1 / sqrt(G_jj)
  double *rn2 = sg + NX;                            // ||r_j||^2
  double *zn2 = rn2 + NX;                           // ||z_j||^2
  double *p4 = zn2 + NX;                            // sum z^4 (type 3: G_jj comes later)
  double *red = p4 + NX;                            // a word per wave

  const int t = threadIdx.x, lane = t & 63, l15 = lane & 15, l4 = lane >> 4;
  const int wave = RECT ? __builtin_amdgcn_readfirstlane(t >> 6) : t >> 6;   // as in check_kernel
  const bcheck::Problem p = locate(a, ITYPE);
  const int n = p.n, c = RECT ? p.c : n;
  cgdouble *A = p.A;
  cgdouble *B = p.B;
  cgdouble *w = p.w;
  cgdouble *Z = p.Z;
  gdouble *S = p.S;
  gdouble *out = p.out;
  gdouble *ipr = p.ipr;
  const int lda = p.lda, ldb = p.ldb, ldz = p.ldz;
  cgdouble *M1 = ITYPE == 2 ? B : A, *M2 = ITYPE == 2 ? A : B;   // the first product's matrix, the second's
  const int ld1 = ITYPE == 2 ? ldb : lda, ld2 = ITYPE == 2 ? lda : ldb;

  // ---- 1: S = M1 Z to the scratch; per column sum z s (type 2), sum z^4, ||z_j||^2; ||M1||_F^2
  double sq1 = 0.0;
#pragma unroll 1
  for (int j0 = 0; j0 < c; j0 += TN) {
    double tg = 0.0, tp = 0.0, tz = 0.0;            // thread x < TN: column j0 + x, over the row tiles
#pragma unroll 1
    for (int i0 = 0; i0 < n; i0 += TM) {
      double4_t acc[4];
      sym_product<STEP, kB, kQ>(M1, ld1, Z, ldz, n, c, i0, j0, wave, buf, acc, j0 == 0, sq1);
      // the epilogue, in the accumulators: acc[jt][r] is entry (i0 + 16 wave + l4 + 4 r, j0 + 16 jt + l15)
      double cg[4], cp[4], cz[4];
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        const int j = j0 + 16 * jt + l15;
        cg[jt] = cp[jt] = cz[jt] = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = i0 + 16 * wave + l4 + 4 * r;
          if (i < n && j < c) {
            const double z = Z[i + (size_t)j * ldz];
            const double sv = acc[jt][r];
            const double z2 = z * z;
            cg[jt] = fma(z, sv, cg[jt]);
            cp[jt] = fma(z2, z2, cp[jt]);
            // a rounding that callers see, kept per entry: ek_hip_check_sygv_xbatched* rounds z^2 before it adds (its kernel
            // was compiled so), ek_hip_check_sygv_window_xbatched* adds it fused
            cz[jt] = RECT ? fma(z, z, cz[jt]) : cz[jt] + z2;
            S[i + (size_t)j * n] = sv;
          }
        }
      }
      double xg, xp, xz;
      column_sums(cg, cp, cz, cs, wave, xg, xp, xz);
      tg += xg; tp += xp; tz += xz;
    }
    if (t < TN && j0 + t < c) {
      zn2[j0 + t] = tz;
      if (ITYPE == 2) {
        sg[j0 + t] = 1.0 / sqrt(tg);
        if (ipr) ipr[j0 + t] = tp / (tg * tg);
      } else {
        p4[j0 + t] = tp;
      }
    }
  }
  __syncthreads();                                  // S is in the scratch for the whole workgroup

  // ---- 2: R = M2 S - fl(w_j z_ij), ||r_j||^2 per column; ||M2||_F^2
  double sq2 = 0.0;
#pragma unroll 1
  for (int j0 = 0; j0 < c; j0 += TN) {
    double wj[4];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
      const int j = j0 + 16 * jt + l15;
      wj[jt] = (j < c) ? w[j] : 0.0;
    }
    double tr = 0.0;
#pragma unroll 1
    for (int i0 = 0; i0 < n; i0 += TM) {
      double4_t acc[4];
      sym_product<STEP, kB, kQ>(M2, ld2, (cgdouble *)S, n, n, c, i0, j0, wave, buf, acc, j0 == 0, sq2);
      double cr[4], c1[4], c2[4];
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        const int j = j0 + 16 * jt + l15;
        cr[jt] = c1[jt] = c2[jt] = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = i0 + 16 * wave + l4 + 4 * r;
          if (i < n && j < c) {
            const double rr = minus_product(acc[jt][r], wj[jt], Z[i + (size_t)j * ldz]);
            cr[jt] = fma(rr, rr, cr[jt]);
          }
        }
      }
      double xr, x1, x2;
      column_sums(cr, c1, c2, cs, wave, xr, x1, x2);
      tr += xr;
    }
    if (t < TN && j0 + t < c) rn2[j0 + t] = tr;
  }
  const double nrm = sqrt(wg_reduce<NW, false>(sq1, red)) * sqrt(wg_reduce<NW, false>(sq2, red));
  __syncthreads();                                  // rn2 is written
  const double rho = (t < c) ? sqrt(rn2[t]) / (nrm * sqrt(zn2[t])) : 0.0;
  const double rsum = wg_reduce<NW, false>(rho, red);
  const double rmax = wg_reduce<NW, true>(rho, red);

  // ---- 3: || D^-1/2 G D^-1/2 - its diagonal ||_F, G of order c
  double os = 0.0;
  bool spd = true;
  if (ITYPE == 2) {
    os = gram_offdiag<false, STEP, kB, kQ>(Z, ldz, (cgdouble *)S, n, n, c, wave, buf, sg);
  } else {
    // the factor: NR rows of 512 / NR threads each, by n alone
    const int NR = !RECT ? NX : n <= 64 ? 64 : n <= 128 ? 128 : NX, PF = T / NR;
    const int r = t & (NR - 1), sub = t / NR;
    const bool row = r < n;
    gdouble *L = S, *Wt = S + (size_t)n * n;
    double *sv = buf, *sl = buf + NX;               // the scaled column; a column of L and the next one
    __syncthreads();                                // every reader of U and of the buffers is through
    if (row)
      for (int j = sub; j <= r; j += PF) L[r + j * n] = B[r + (size_t)j * ldb];
    __syncthreads();
    // B = L L^T, right-looking
    for (int j = 0; j < n; ++j) {
      const double piv = L[j + j * n];              // the same word in every thread: the exit is uniform
      if (!(piv > 0.0 && piv < INFINITY)) { spd = false; break; }
      const double l = sqrt(piv);
      if (sub == 0 && row && r > j) {
        const double lr = L[r + j * n] / l;
        L[r + j * n] = lr;
        sv[r] = lr;
      }
      __syncthreads();
      if (t == j) L[j + j * n] = l;
      if (row && r > j) img_axpy(L + r, n, sv, sv[r], j + 1 + sub, r + 1, PF);
      __syncthreads();
    }
    if (spd) {
      // the solve: CP columns of 512 / CP threads each, by c alone
      const int CP = !RECT ? NX : c <= 16 ? 16 : c <= 32 ? 32 : c <= 64 ? 64 : c <= 128 ? 128 : NX, PS = T / CP;
      const int col = t & (CP - 1), part = t / CP;
      const bool act = col < c;
      // Z^T into the image behind the factor: the group `col` owns column col of Z as row col
      if (act)
        for (int i = part; i < n; i += PS) Wt[col + i * c] = Z[i + (size_t)col * ldz];
      if (t < n) sl[t] = L[t];                      // column 0 of L
      __syncthreads();
      // W = L^-1 Z: step k finishes w_k,col = pv / l_kk and subtracts l_ik w_k,col from the entries i > k; the threads of
      // a group take every PS-th entry; the next step's pivot is carried in a register by all of them, part 0 stores it
      double pv = act ? Wt[col] : 0.0, gd = 0.0;
      __syncthreads();                              // every part holds the first pivot before part 0 overwrites it
      for (int k = 0; k < n; ++k) {
        const double *cur = sl + (k & 1) * NX;
        double nx = 0.0, nv = 0.0;
        if (k + 1 < n && t > k && t < n) nx = L[t + (k + 1) * n];
        if (act) {
          if (k + 1 < n) nv = Wt[col + (k + 1) * c];   // step k - 1 wrote it; this step leaves it alone
          const double xk = pv / cur[k];
          if (part == 0) Wt[col + k * c] = xk;
          gd = fma(xk, xk, gd);
          pv = fma(-cur[min(k + 1, n - 1)], xk, nv);
          img_axpy(Wt + col, c, cur, xk, k + 2 + part, n, PS);
        }
        if (t < n) sl[((k + 1) & 1) * NX + t] = nx;
        __syncthreads();
      }
      if (t < c) {                                  // part 0: col = t
        sg[t] = 1.0 / sqrt(gd);
        if (ipr) ipr[t] = p4[t] / (gd * gd);
      }
      __syncthreads();                              // sg and W are written, the buffers are free
      os = gram_offdiag<true, STEP, kB, kQ>((cgdouble *)Wt, c, (cgdouble *)Wt, c, n, c, wave, buf, sg);
    } else if (t < c && ipr) {
      ipr[t] = __builtin_nan("");
    }
  }
  const double osum = wg_reduce<NW, false>(os, red);
  if (t == 0) {
    out[0] = nrm;
    out[1] = rsum / (double)c;
    out[2] = rmax;
    out[3] = spd ? sqrt(osum) : __builtin_nan("");
  }
}

// one launch of KERNEL for `count` problems; the dynamic-LDS attribute is raised once per kernel
template <auto KERNEL, typename ARGS>
static int launch(hipStream_t s, int count, int lds_doubles, const ARGS &a) {
  const size_t lds = (size_t)lds_doubles * sizeof(double);
  static bool raised = false;                       // one per instantiation
  if (!raised) {
    EK_HIP_CHECK(hipFuncSetAttribute((const void *)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    raised = true;
  }
  hipLaunchKernelGGL(KERNEL, dim3(count), dim3(T), lds, s, a);
  EK_HIP_CHECK(hipGetLastError());
  return 0;
}

}  // namespace xcheck
}  // namespace ek
