// ek_batched_check_sygv_window.hip -- ek_hip_check_sygv_window_xbatched*: the batched acceptance checks of DSYGV's types 2
// (A B x = l x) and 3 (B A x = l x) for what ek_hip_sygv_window_xbatched* and ek_hip_sygv_window_batched* return: per
// problem the c = m[b] values w[0 .. c) and the columns 0 .. c-1 of an n x zcap array, every order 1 .. EK_HIP_XBATCH_NMAX
// in one kernel class.  Type 1 is ek_hip_check_window_xbatched*(problem = 1) itself.  This unit holds the
// kernel, its launch and the entries; the argument checker, the device pool, the chunk loop, the fetch and the scatter are
// ek_batched_check.hip's (bcheck::window_arguments, bcheck::window_entry).
//
// One workgroup of 512 threads (8 waves) owns a problem from its first load to its last store.  The quantities are those
// of DESIGN.md 16 / 20 on c columns; the passes are ek_batched_check_sygv_x.hip's made rectangular with the pieces of
// ek_batched_check_window.hip (rect_tile, step_strip: a 16-row strip or a 16-column subtile that holds nothing issues no
// matrix instruction), so every product costs n^2 c.  The scratch is n c (type 2) or n^2 + n c (type 3) doubles per
// workgroup of a launch.
//
//   type 2   1  S = B Z (n x c, leading dimension n) to the scratch; per column G_jj = sum z s, sum z^4, ||z_j||^2;
//               ||B||_F^2.  Tile order, K step, epilogue and reduction order are those of the B side of wcheck_kernel<true>
//            2  R = A S - fl(w_j z_ij) in the accumulators (minus_product), ||r_j||^2 per column; ||A||_F^2
//            3  G = Z^T S over the c x c tiles: pass 2 of wcheck_kernel.  Slot 3 and the IPRs are type 1's bits for the
//               same (B, Z, c)
//   type 3   1  U = A Z to the first n c doubles of the scratch; sum z^4, ||z_j||^2; ||A||_F^2
//            2  R = B U - fl(w_j z_ij); ||B||_F^2
//            3  B = L L^T from the caller's lower triangle into the first n^2 of the scratch (U is dead): right-looking,
//               512 / NR threads per row, NR = 64, 128 or 256 the power of two that holds n; a pivot that is not positive
//               and finite ends the type's part for the whole workgroup: slot 3 and the c IPRs are NaN, the residual
//               slots stand
//            4  W = L^-1 Z for the c columns, kept TRANSPOSED (c x n, leading dimension c) behind the factor: a column of
//               L a step, staged in LDS a step ahead.  A column of W belongs to 512 / CP threads, CP the power of two
//               (at least 16) that holds c: 2 at c > 128, 32 at c <= 16.  Every thread of a group carries the pivot and
//               G_jj = sum_i w_ij^2 itself and takes every (512 / CP)-th entry of the axpy; an entry's updates come in
//               the order of the steps whoever applies them, and nothing is summed across threads
//            5  G = W^T W of order c, both operands from rows of the transposed image
//
// Same bits wherever a problem sits: every loop bound, every skipped strip, the split of the factor and of the solve and
// every summation order depend on (n, c) alone; no atomics; the same kernel behind the host and the device form.  A, B, w
// and Z are read only; nothing of w or Z from m[b] on, strictly above a diagonal, at or beyond row n or between the problems
// is read.
//
// Each type's kernel has a second instantiation that finds order, c and addresses in the variable form's table
// (bcheck::launch_sygv_window_v, behind ek_hip_check_sygv_window_xvbatched*: DESIGN.md 37); the passes exist once.
#include "ek_batched_check_x.h"

namespace ek {
namespace wcheck_sygv {

using namespace xcheck;

constexpr int NX = EK_HIP_XBATCH_NMAX;
constexpr int kBuf = kTileP + kTileQ;               // the two operands of one step
// LDS doubles: two buffers (type 3's factor and solve keep the scaled column and two columns of L there), the waves' column
// sums, four words per column (1 / sqrt(G_jj), ||r_j||^2, ||z_j||^2, sum z^4), a word per wave
constexpr int kLdsDoubles = 2 * kBuf + 3 * NW * TN + 4 * NX + NW;
static_assert(2 * kBuf >= 3 * NX, "the factor's vectors fit in the buffers");
static_assert(T == 2 * NX, "at least two threads per row in the factor and per column in the solve");

struct Args {
  int n;
  const double *A; int lda; long long sA;
  const double *B; int ldb; long long sB;
  const double *w;
  const double *Z; int ldz; long long sZ;
  const int *map;       // entry e: the pair (problem, m[problem]) in map[2 e], map[2 e + 1]
  int first;            // this launch's first entry of the map
  double *S; long long sS;   // sS doubles per workgroup of a launch: n x (the largest checked m), type 3: n^2 more
  double *out;          // EK_HIP_CHECK_NOUT doubles per problem
  double *ipr;          // n doubles per problem, or nullptr
};

// ---- the rectangular pieces of ek_batched_check_window.hip (that unit keeps its source; these are its functions)
// KT x W tile of a column-major rows x cols matrix, rows k0 .. (the inner dimension), columns c0 ..: along k
template <int W>
__device__ __forceinline__ void rect_tile(cgdouble *M, int ld, int rows, int cols, int k0, int c0, double (&v)[W / 32]) {
  const int t = threadIdx.x, k = k0 + (t & 15);
#pragma unroll
  for (int q = 0; q < W / 32; ++q) {
    const int c = c0 + (t >> 4) + 32 * q;
    // unconditional: past the edge it takes the last row or column that exists and is dropped
    const double x = M[min(k, rows - 1) + (size_t)min(c, cols - 1) * ld];
    v[q] = (k < rows && c < cols) ? x : 0.0;
  }
}
// the same tile of the TRANSPOSE of a column-major cols x rows matrix: entry (k, c) is M[c + k ld], along c
template <int W>
__device__ __forceinline__ void rect_row_tile(cgdouble *M, int ld, int rows, int cols, int k0, int c0,
                                              double (&v)[W / 32]) {
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

// one step of 16 of the inner dimension for this wave's strip: acc += P^T-tile rows x the first NSUB subtiles of the Q-tile
template <int NSUB>
__device__ __forceinline__ void step_subtiles(const double *sp, const double *sq, int wave, double4_t (&acc)[4]) {
  const int lane = threadIdx.x & 63, l15 = lane & 15, l4 = lane >> 4;
#pragma unroll
  for (int kk = 0; kk < KT; kk += 4) {
    const double x = sp[(kk + l4) * LDP + 16 * wave + l15];
#pragma unroll
    for (int jt = 0; jt < NSUB; ++jt) {
      const double y = sq[(kk + l4) * LDQ + 16 * jt + l15];
      acc[jt] = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, acc[jt], 0, 0, 0);
    }
  }
}
// nsub is the same in the whole workgroup: one straight-line body per count (a test per subtile inside the unrolled body
// cost this unit's kernels their registers); the instructions of a subtile and their order are those of step_strip
__device__ __forceinline__ void step_strip(const double *sp, const double *sq, int wave, int nsub, double4_t (&acc)[4]) {
  switch (nsub) {
    case 1: step_subtiles<1>(sp, sq, wave, acc); break;
    case 2: step_subtiles<2>(sp, sq, wave, acc); break;
    case 3: step_subtiles<3>(sp, sq, wave, acc); break;
    default: step_subtiles<4>(sp, sq, wave, acc); break;
  }
}

// acc <- tile (i0, j0) of M Q: M symmetric of order n, its lower triangle referenced; Q column-major n x c.  With `squares`
// the squares of the staged entries of M are added to sq.  Ends behind a barrier: the buffers are free
__device__ __forceinline__ void sym_product(cgdouble *M, int ldm, cgdouble *Q, int ldq, int n, int c, int i0, int j0,
                                            int wave, double *buf, double4_t (&acc)[4], bool squares, double &sq) {
  const int nk = (n + KT - 1) / KT, nsub = min(4, (c - j0 + 15) >> 4);
  const bool strip = i0 + 16 * wave < n;
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) acc[jt] = (double4_t){0.0, 0.0, 0.0, 0.0};
  double vm[4], vq[2];
  auto fetch = [&](int k0) {
    sym_tile(M, ldm, n, i0, k0, vm);
    rect_tile<TN>(Q, ldq, n, c, k0, j0, vq);
  };
  auto put = [&](int k0, double *s) {
    sym_put(s, i0, k0, vm);
    col_put<TN, LDQ>(s + kTileP, vq);
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
    const double *cur = buf + (s & 1) * kBuf;
    const bool more = s + 1 < nk;
    if (more) fetch((s + 1) * KT);
    if (strip) step_strip(cur, cur + kTileP, wave, nsub, acc);
    if (more) put((s + 1) * KT, buf + ((s + 1) & 1) * kBuf);
    __syncthreads();
  }
}

// The sum over a tile's rows of three per-column values of the epilogue: in the wave over the four lane >> 4 groups, over
// the waves in ascending order through cs; thread c < TN returns column j0 + c's sums in x0 .. x2.  Ends behind a barrier
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

// sum over l != j of (G_lj sg_l sg_j)^2 of this thread's entries, G = P^T Q of order c with the inner dimension n (ROWS:
// P^T and Q^T are what lies in memory, c x n, their rows are read); pass 2 of wcheck_kernel
template <bool ROWS>
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
          rect_row_tile<TM>(P, ldp, n, c, k0, l0, vp);
          rect_row_tile<TN>(Q, ldq, n, c, k0, j0, vq);
        } else {
          rect_tile<TM>(P, ldp, n, c, k0, l0, vp);
          rect_tile<TN>(Q, ldq, n, c, k0, j0, vq);
        }
      };
      auto put = [&](double *s) {
        if (ROWS) {
          row_put<TM, LDP>(s, vp);
          row_put<TN, LDQ>(s + kTileP, vq);
        } else {
          col_put<TM, LDP>(s, vp);
          col_put<TN, LDQ>(s + kTileP, vq);
        }
      };
      fetch(0);
      put(buf);
      __syncthreads();
#pragma unroll 1
      for (int s = 0; s < nk; ++s) {
        const double *cur = buf + (s & 1) * kBuf;
        const bool more = s + 1 < nk;
        if (more) fetch((s + 1) * KT);
        if (strip) step_strip(cur, cur + kTileP, wave, nsub, acc);
        if (more) put(buf + ((s + 1) & 1) * kBuf);
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
    for (int q = 0; q < 8; ++q) yv[q] = y[(size_t)(i + q * st) * sy];
#pragma unroll
    for (int q = 0; q < 8; ++q) xv[q] = x[i + q * st];
#pragma unroll
    for (int q = 0; q < 8; ++q) y[(size_t)(i + q * st) * sy] = fma(-xv[q], a, yv[q]);
  }
  for (; i < i1; i += st) y[(size_t)i * sy] = fma(-x[i], a, y[(size_t)i * sy]);
}

// the uniform launch's problem: entry first + workgroup of the map, the scratch by workgroup
__device__ __forceinline__ bcheck::WProblem locate_w(const Args &a) {
  const int n = a.n;
  const int e = a.first + (int)blockIdx.x;
  const long long pb = a.map[2 * e];
  const int c = a.map[2 * e + 1];                   // 1 <= c <= n
  return {n, c, (cgdouble *)(a.A + pb * a.sA), a.lda, (cgdouble *)(a.B + pb * a.sB), a.ldb, (cgdouble *)(a.w + pb * n),
          (cgdouble *)(a.Z + pb * a.sZ), a.ldz, (gdouble *)(a.S + (long long)blockIdx.x * a.sS),
          (gdouble *)(a.out + pb * EK_HIP_CHECK_NOUT), a.ipr ? (gdouble *)(a.ipr + pb * n) : nullptr};
}
__device__ __forceinline__ bcheck::WProblem locate_w(const bcheck::VArgs &a) { return bcheck::locate_window(a); }

// ARGS: how the workgroup finds its problem -- Args (one order, strided; the scratch by workgroup) or bcheck::VArgs (entry
// blockIdx.x of the launch's slice of the table, which names the entry's order, its m and its own scratch: DESIGN.md 37)
template <int ITYPE, typename ARGS>
__global__ __launch_bounds__(T) void wcheck_sygv_kernel(ARGS a) {
  static_assert(ITYPE == 2 || ITYPE == 3, "type 1 is ek_batched_check_window.hip's");
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double *buf = smem;                               // [2][kBuf]
  double *cs = buf + 2 * kBuf;                      // [3][NW][TN]: the waves' column sums
  double *sg = cs + 3 * NW * TN;                    // 1 / sqrt(G_jj)
  double *rn2 = sg + NX;                            // ||r_j||^2
  double *zn2 = rn2 + NX;                           // ||z_j||^2
  double *p4 = zn2 + NX;                            // sum z^4 (type 3: G_jj comes later)
  double *red = p4 + NX;                            // a word per wave

  const int t = threadIdx.x, lane = t & 63, l15 = lane & 15, l4 = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);   // scalar: a skipped strip is a branch, not a mask
  const bcheck::WProblem p = locate_w(a);
  const int n = p.n, c = p.c;
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
      sym_product(M1, ld1, Z, ldz, n, c, i0, j0, wave, buf, acc, j0 == 0, sq1);
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
            cz[jt] = fma(z, z, cz[jt]);
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
      wj[jt] = (j < c) ? w[min(j, c - 1)] : 0.0;
    }
    double tr = 0.0;
#pragma unroll 1
    for (int i0 = 0; i0 < n; i0 += TM) {
      double4_t acc[4];
      sym_product(M2, ld2, (cgdouble *)S, n, n, c, i0, j0, wave, buf, acc, j0 == 0, sq2);
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
    os = gram_offdiag<false>(Z, ldz, (cgdouble *)S, n, n, c, wave, buf, sg);
  } else {
    // the factor: NR rows of 512 / NR threads each, by n alone
    const int NR = n <= 64 ? 64 : n <= 128 ? 128 : NX, PF = T / NR;
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
      const int CP = c <= 16 ? 16 : c <= 32 ? 32 : c <= 64 ? 64 : c <= 128 ? 128 : NX, PS = T / CP;
      const int col = t & (CP - 1), part = t / CP;
      const bool act = col < c;
      // Z^T into the image behind the factor: the group `col` owns column col of Z as row col
      if (act)
        for (int i = part; i < n; i += PS) Wt[col + (size_t)i * c] = Z[i + (size_t)col * ldz];
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
          if (k + 1 < n) nv = Wt[col + (size_t)(k + 1) * c];   // step k - 1 wrote it; this step leaves it alone
          const double xk = pv / cur[k];
          if (part == 0) Wt[col + (size_t)k * c] = xk;
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
      os = gram_offdiag<true>((cgdouble *)Wt, c, (cgdouble *)Wt, c, n, c, wave, buf, sg);
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

template <int ITYPE, typename ARGS>
static int launch(hipStream_t s, int count, const ARGS &a) {
  constexpr size_t lds = (size_t)kLdsDoubles * sizeof(double);
  static bool raised = false;                       // one per instantiation
  if (!raised) {
    EK_HIP_CHECK(hipFuncSetAttribute((const void *)wcheck_sygv_kernel<ITYPE, ARGS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds));
    raised = true;
  }
  hipLaunchKernelGGL((wcheck_sygv_kernel<ITYPE, ARGS>), dim3(count), dim3(T), lds, s, a);
  EK_HIP_CHECK(hipGetLastError());
  return 0;
}

// this unit's part of a call (bcheck::window_entry does the rest): the scratch is indexed by workgroup
static int launch_window(hipStream_t s, const bcheck::Window &w, const int *map, int first, int count, long long sS,
                         double *S, double *dout, double *dipr) {
  const bcheck::Uniform &u = w.u;
  Args a{u.n, u.A, u.lda, u.sA, u.B, u.ldb, u.sB, u.w, u.Z, u.ldz, u.sZ, map, first, S, sS, dout, dipr};
  return u.itype == 2 ? launch<2>(s, count, a) : launch<3>(s, count, a);
}

static int entry(int itype, int n, int batch, const double *A, int lda, long long strideA, const double *B, int ldb,
                 long long strideB, const int *m, const double *w, const double *Z, int ldz, int zcap, long long strideZ,
                 const int *info, double *out, double *ipr, double *seconds, bool host) {
  // the -1 rule is the driver's: itype 1 .. 3 here, with problem = 1 (B is always required)
  const bcheck::Window win{{itype, 1, n, batch, A, lda, strideA, B, ldb, strideB, w, Z, ldz, strideZ, info, out, ipr,
                            seconds}, m, zcap, true};
  bool nothing;
  int rc = bcheck::window_arguments(win, EK_HIP_XBATCH_NMAX, &nothing);
  if (rc) return rc;
  if (itype == 1)                                   // type 1 is problem 1 of the window check itself: the same kernel
    return host ? ek_hip_check_window_xbatched(1, n, batch, A, lda, strideA, B, ldb, strideB, m, w, Z, ldz, zcap, strideZ,
                                               info, out, ipr, seconds)
                : ek_hip_check_window_xbatched_device(1, n, batch, A, lda, strideA, B, ldb, strideB, m, w, Z, ldz, zcap,
                                                      strideZ, info, out, ipr, seconds);
  return bcheck::window_entry(win, nothing, host, launch_window);
}

}  // namespace wcheck_sygv

// the variable form's launch (ek_batched_check.h): `count` entries of the table, itype 2 or 3
int bcheck::launch_sygv_window_v(hipStream_t s, int itype, int count, const VArgs &a) {
  return itype == 2 ? wcheck_sygv::launch<2>(s, count, a) : wcheck_sygv::launch<3>(s, count, a);
}

}  // namespace ek

using namespace ek;

extern "C" {

int ek_hip_check_sygv_window_xbatched_device(int itype, int n, int batch, const double *dA, int lda, long long strideA,
                                             const double *dB, int ldb, long long strideB, const int *m, const double *dw,
                                             const double *dZ, int ldz, int zcap, long long strideZ, const int *info,
                                             double *out, double *ipr, double *seconds) {
  return wcheck_sygv::entry(itype, n, batch, dA, lda, strideA, dB, ldb, strideB, m, dw, dZ, ldz, zcap, strideZ, info, out,
                            ipr, seconds, false);
}

int ek_hip_check_sygv_window_xbatched(int itype, int n, int batch, const double *A, int lda, long long strideA,
                                      const double *B, int ldb, long long strideB, const int *m, const double *w,
                                      const double *Z, int ldz, int zcap, long long strideZ, const int *info, double *out,
                                      double *ipr, double *seconds) {
  return wcheck_sygv::entry(itype, n, batch, A, lda, strideA, B, ldb, strideB, m, w, Z, ldz, zcap, strideZ, info, out, ipr,
                            seconds, true);
}

}  // extern "C"
