// ek_batched_check_sygv_x.hip -- ek_hip_check_sygv_xbatched*: the batched acceptance checks of DSYGV's types 2
// (A B x = l x) and 3 (B A x = l x) for the orders EK_HIP_BATCH_NMAX + 1 .. EK_HIP_XBATCH_NMAX that ek_hip_sygv_xbatched*
// solves.  Orders up to EK_HIP_BATCH_NMAX are forwarded to ek_hip_check_sygv_batched*, type 1 above them to
// ek_hip_check_xbatched*(problem = 1).  This unit holds the kernel, its launch and the entries; the argument checker, the
// device pool, the chunk loop, the fetch and the scatter are ek_batched_check.hip's.
// The kernel has a second instantiation per type that finds its problem in the variable form's table
// (bcheck::launch_sygv_x, behind ek_hip_check_sygv_xvbatched*: DESIGN.md 24); the passes exist once.
//
// One workgroup of 512 threads (8 waves) owns a problem from its first load to its last store.  The quantities are those
// of DESIGN.md 16.  The three n^3 products of a type run on the fp64 matrix cores with the tiles, the loaders, the K step
// and the two LDS buffers of ek_batched_check_x.hip (ek_batched_check_x.h); S and W live in a device scratch of n^2
// (type 2) or 2 n^2 (type 3) doubles per workgroup of a launch, leading dimension n.
//
//   type 2   1  S = B Z to the scratch; per column G_jj = sum z s, sum z^4, ||z_j||^2; ||B||_F^2.  Tile order, K step,
//               epilogue and reduction order are those of the B side of xcheck_kernel<true>
//            2  R = A S - fl(w_j z_ij) in the accumulators (minus_product), ||r_j||^2 per column; ||A||_F^2
//            3  G = Z^T S: pass 2 of xcheck_kernel.  Slot 3 and the IPRs are type 1's bits for the same (B, Z)
//   type 3   1  U = A Z to the scratch; sum z^4, ||z_j||^2; ||A||_F^2
//            2  R = B U - fl(w_j z_ij); ||B||_F^2
//            3  B = L L^T from the caller's lower triangle into the first n^2 of the scratch (U is dead): right-looking,
//               lane = row, the scaled column of a step kept in LDS (stage 1 of ek_batched_x.hip); a pivot takes a square
//               root and a division.  A pivot that is not positive and finite ends the type's part for the whole
//               workgroup (the word is the same in every thread): slot 3 and the IPRs are NaN, the residual slots stand
//            4  W = L^-1 Z, kept TRANSPOSED in the second n^2 (the pair t owns column t of W = row t of that image): a
//               column of L a step, staged in LDS a step ahead, axpy form with eight loads in flight (stage 2 of
//               ek_batched_x.hip); G_jj = sum_i w_ij^2 is summed as the entries become final
//            5  G = W^T W, both operands from rows of the transposed image (consecutive addresses along the columns)
//
// Same bits wherever a problem sits: every loop bound and every summation order depends on n alone; no atomics; the same
// kernel behind the host and the device form.  A, B, w and Z are read only; nothing strictly above a diagonal, at or
// beyond row n or between the problems is read.
#include "ek_batched_check_x.h"

namespace ek {
namespace xcheck_sygv {

using namespace xcheck;

constexpr int NX = EK_HIP_XBATCH_NMAX;
constexpr int kBuf = kTileP + kTileQ;               // the two operands of one step
// LDS doubles: two buffers (type 3's factor and solve keep the scaled column and two columns of L there), the waves' column
// sums, four words per column (1 / sqrt(G_jj), ||r_j||^2, ||z_j||^2, sum z^4), a word per wave
constexpr int kLdsDoubles = 2 * kBuf + 3 * NW * TN + 4 * NX + NW;
static_assert(2 * kBuf >= 3 * NX, "the factor's vectors fit in the buffers");
static_assert(T == 2 * NX, "two threads per row in the factor and the solve");

struct Args {
  int itype, n;
  const double *A; int lda; long long sA;
  const double *B; int ldb; long long sB;
  const double *w;
  const double *Z; int ldz; long long sZ;
  const int *map;       // the problems to check; nullptr: every problem
  int first;            // this launch's first entry of the map (or first problem)
  double *S;            // (itype - 1) n^2 doubles per workgroup of a launch
  double *out;          // EK_HIP_CHECK_NOUT doubles per problem
  double *ipr;          // n doubles per problem, or nullptr
};

// KT x W tile of the TRANSPOSE of a column-major matrix: entry (k, c) is M[c + k ld], consecutive addresses along c
template <int W>
__device__ __forceinline__ void row_tile(cgdouble *M, int ld, int n, int k0, int c0, double (&v)[W / 32]) {
  const int t = threadIdx.x, c = c0 + t % W;
#pragma unroll
  for (int q = 0; q < W / 32; ++q) {
    const int k = k0 + t / W + (T / W) * q;
    const double x = M[min(c, n - 1) + (size_t)min(k, n - 1) * ld];   // unconditional, as the other loaders
    v[q] = (k < n && c < n) ? x : 0.0;
  }
}
template <int W, int LD>
__device__ __forceinline__ void row_put(double *s, const double (&v)[W / 32]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int q = 0; q < W / 32; ++q) s[(t / W + (T / W) * q) * LD + t % W] = v[q];
}

// acc <- tile (i0, j0) of M Q: M symmetric, its lower triangle referenced; Q column-major.  With `squares` the squares of
// the staged entries of M are added to sq.  Ends behind a barrier: the buffers are free
__device__ __forceinline__ void sym_product(cgdouble *M, int ldm, cgdouble *Q, int ldq, int n, int i0, int j0,
                                            double *buf, double4_t (&acc)[4], bool squares, double &sq) {
  const int nk = (n + KT - 1) / KT;
#pragma unroll
  for (int jt = 0; jt < 4; ++jt) acc[jt] = (double4_t){0.0, 0.0, 0.0, 0.0};
  double vm[4], vq[2];
  auto fetch = [&](int k0) {
    sym_tile(M, ldm, n, i0, k0, vm);
    col_tile<TN>(Q, ldq, n, k0, j0, vq);
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
    step_mfma<false>(cur, cur, cur + kTileP, acc, acc);
    if (more) put((s + 1) * KT, buf + ((s + 1) & 1) * kBuf);
    __syncthreads();
  }
}

// The sum over a tile's rows of three per-column values of the epilogue: in the wave over the four lane >> 4 groups, over
// the waves in ascending order through cs; thread c < TN returns column j0 + c's sums in x0 .. x2.  Ends behind a barrier
// for the threads that read; the next write of cs lies behind the next tile's barriers
__device__ __forceinline__ void column_sums(double (&c0)[4], double (&c1)[4], double (&c2)[4], double *cs, double &x0,
                                            double &x1, double &x2) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l15 = lane & 15, l4 = lane >> 4;
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

// sum over l != j of (G_lj sg_l sg_j)^2 of this thread's entries, G = P^T Q (ROWS: P^T and Q^T are what lies in memory,
// their rows are read); pass 2 of xcheck_kernel
template <bool ROWS>
__device__ __forceinline__ double gram_offdiag(cgdouble *P, int ldp, cgdouble *Q, int ldq, int n, double *buf,
                                               const double *sg) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l15 = lane & 15, l4 = lane >> 4;
  const int nk = (n + KT - 1) / KT;
  double os = 0.0;
#pragma unroll 1
  for (int j0 = 0; j0 < n; j0 += TN)
#pragma unroll 1
    for (int l0 = 0; l0 < n; l0 += TM) {
      double4_t acc[4];
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) acc[jt] = (double4_t){0.0, 0.0, 0.0, 0.0};
      double vp[4], vq[2];
      auto fetch = [&](int k0) {
        if (ROWS) {
          row_tile<TM>(P, ldp, n, k0, l0, vp);
          row_tile<TN>(Q, ldq, n, k0, j0, vq);
        } else {
          col_tile<TM>(P, ldp, n, k0, l0, vp);
          col_tile<TN>(Q, ldq, n, k0, j0, vq);
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
        step_mfma<false>(cur, cur, cur + kTileP, acc, acc);
        if (more) put(buf + ((s + 1) & 1) * kBuf);
        __syncthreads();
      }
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        const int j = j0 + 16 * jt + l15;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int l = l0 + 16 * wave + l4 + 4 * r;
          if (l < n && j < n && l != j) {
            const double g = acc[jt][r] * sg[l] * sg[j];
            os = fma(g, g, os);
          }
        }
      }
    }
  return os;
}

// y[i sy] -= x[i] a for i = i0, i0 + 2, ... < i1; y in the scratch, x in LDS: eight loads before the first store
__device__ __forceinline__ void img_axpy(gdouble *y, int sy, const double *x, double a, int i0, int i1) {
  int i = i0;
  for (; i + 14 < i1; i += 16) {
    double yv[8], xv[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) yv[q] = y[(i + 2 * q) * sy];
#pragma unroll
    for (int q = 0; q < 8; ++q) xv[q] = x[i + 2 * q];
#pragma unroll
    for (int q = 0; q < 8; ++q) y[(i + 2 * q) * sy] = yv[q] - xv[q] * a;
  }
  for (; i < i1; i += 2) y[i * sy] -= x[i] * a;
}

// the uniform launch's problem: entry first + workgroup of the map (or that problem), the scratch by workgroup
template <int ITYPE>
__device__ __forceinline__ bcheck::Problem locate_sygv(const Args &a) {
  const int n = a.n;
  const long long pb = a.map ? a.map[a.first + (int)blockIdx.x] : a.first + (int)blockIdx.x;
  return {n, (cgdouble *)(a.A + pb * a.sA), a.lda, (cgdouble *)(a.B + pb * a.sB), a.ldb, (cgdouble *)(a.w + pb * n),
          (cgdouble *)(a.Z + pb * a.sZ), a.ldz, (gdouble *)(a.S + (long long)blockIdx.x * (ITYPE - 1) * n * n),
          (gdouble *)(a.out + pb * EK_HIP_CHECK_NOUT), a.ipr ? (gdouble *)(a.ipr + pb * n) : nullptr};
}
template <int ITYPE>
__device__ __forceinline__ bcheck::Problem locate_sygv(const bcheck::VArgs &a) { return bcheck::locate(a); }

// ARGS: Args (one order, strided; the scratch by workgroup) or bcheck::VArgs (entry blockIdx.x of the launch's slice of the
// table, which names the entry's own scratch of (ITYPE - 1) n^2 doubles)
template <int ITYPE, typename ARGS>
__global__ __launch_bounds__(T) void xcheck_sygv_kernel(ARGS a) {
  static_assert(ITYPE == 2 || ITYPE == 3, "type 1 is ek_batched_check_x.hip's");
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double *buf = smem;                               // [2][kBuf]
  double *cs = buf + 2 * kBuf;                      // [3][NW][TN]: the waves' column sums
  double *sg = cs + 3 * NW * TN;                    // 1 / sqrt(G_jj)
  double *rn2 = sg + NX;                            // ||r_j||^2
  double *zn2 = rn2 + NX;                           // ||z_j||^2
  double *p4 = zn2 + NX;                            // sum z^4 (type 3: G_jj comes later)
  double *red = p4 + NX;                            // a word per wave

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l15 = lane & 15, l4 = lane >> 4;
  const bcheck::Problem p = locate_sygv<ITYPE>(a);
  const int n = p.n;
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
  for (int j0 = 0; j0 < n; j0 += TN) {
    double tg = 0.0, tp = 0.0, tz = 0.0;            // thread c < TN: column j0 + c, over the row tiles
#pragma unroll 1
    for (int i0 = 0; i0 < n; i0 += TM) {
      double4_t acc[4];
      sym_product(M1, ld1, Z, ldz, n, i0, j0, buf, acc, j0 == 0, sq1);
      // the epilogue, in the accumulators: acc[jt][r] is entry (i0 + 16 wave + l4 + 4 r, j0 + 16 jt + l15)
      double cg[4], cp[4], cz[4];
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        const int j = j0 + 16 * jt + l15;
        cg[jt] = cp[jt] = cz[jt] = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = i0 + 16 * wave + l4 + 4 * r;
          if (i < n && j < n) {
            const double z = Z[i + (size_t)j * ldz];
            const double sv = acc[jt][r];
            const double z2 = z * z;
            cg[jt] = fma(z, sv, cg[jt]);
            cp[jt] = fma(z2, z2, cp[jt]);
            cz[jt] += z2;
            S[i + (size_t)j * n] = sv;
          }
        }
      }
      double xg, xp, xz;
      column_sums(cg, cp, cz, cs, xg, xp, xz);
      tg += xg; tp += xp; tz += xz;
    }
    if (t < TN && j0 + t < n) {
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
  for (int j0 = 0; j0 < n; j0 += TN) {
    double wj[4];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
      const int j = j0 + 16 * jt + l15;
      wj[jt] = (j < n) ? w[j] : 0.0;
    }
    double tr = 0.0;
#pragma unroll 1
    for (int i0 = 0; i0 < n; i0 += TM) {
      double4_t acc[4];
      sym_product(M2, ld2, (cgdouble *)S, n, n, i0, j0, buf, acc, j0 == 0, sq2);
      double cr[4], c1[4], c2[4];
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) {
        const int j = j0 + 16 * jt + l15;
        cr[jt] = c1[jt] = c2[jt] = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = i0 + 16 * wave + l4 + 4 * r;
          if (i < n && j < n) {
            const double rr = minus_product(acc[jt][r], wj[jt], Z[i + (size_t)j * ldz]);
            cr[jt] = fma(rr, rr, cr[jt]);
          }
        }
      }
      double xr, x1, x2;
      column_sums(cr, c1, c2, cs, xr, x1, x2);
      tr += xr;
    }
    if (t < TN && j0 + t < n) rn2[j0 + t] = tr;
  }
  const double nrm = sqrt(wg_reduce<NW, false>(sq1, red)) * sqrt(wg_reduce<NW, false>(sq2, red));
  __syncthreads();                                  // rn2 is written
  const double rho = (t < n) ? sqrt(rn2[t]) / (nrm * sqrt(zn2[t])) : 0.0;
  const double rsum = wg_reduce<NW, false>(rho, red);
  const double rmax = wg_reduce<NW, true>(rho, red);

  // ---- 3: || D^-1/2 G D^-1/2 - its diagonal ||_F
  double os = 0.0;
  bool spd = true;
  if (ITYPE == 2) {
    os = gram_offdiag<false>(Z, ldz, (cgdouble *)S, n, n, buf, sg);
  } else {
    const int r = t % NX, sub = t / NX;
    const bool row = r < n;
    gdouble *L = S, *Wt = S + (size_t)n * n;
    double *sv = buf, *sl = buf + NX;               // the scaled column; a column of L and the next one
    __syncthreads();                                // every reader of U and of the buffers is through
    if (row)
      for (int j = sub; j <= r; j += 2) L[r + j * n] = B[r + (size_t)j * ldb];
    __syncthreads();
    // B = L L^T, right-looking, lane = row
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
      if (row && r > j) img_axpy(L + r, n, sv, sv[r], j + 1 + sub, r + 1);
      __syncthreads();
    }
    if (spd) {
      // Z^T into the second image: the pair r owns column r of Z as row r
      if (row)
        for (int i = sub; i < n; i += 2) Wt[r + i * n] = Z[i + (size_t)r * ldz];
      if (t < n) sl[t] = L[t];                      // column 0 of L
      __syncthreads();
      // W = L^-1 Z: step k finishes w_kr = pv / l_kk and subtracts l_ik w_kr from the entries i > k; the two threads of a
      // pair take every other entry; the next step's pivot is carried in a register by both, only the half 0 stores it
      double pv = row ? Wt[r] : 0.0, gd = 0.0;
      __syncthreads();                              // both halves hold the first pivot before half 0 overwrites it
      for (int k = 0; k < n; ++k) {
        const double *cur = sl + (k & 1) * NX;
        double nx = 0.0, nv = 0.0;
        if (k + 1 < n && t > k && t < n) nx = L[t + (k + 1) * n];
        if (row) {
          if (k + 1 < n) nv = Wt[r + (k + 1) * n];  // step k - 1 wrote it; this step leaves it alone
          const double xk = pv / cur[k];
          if (sub == 0) Wt[r + k * n] = xk;
          gd = fma(xk, xk, gd);
          pv = nv - cur[min(k + 1, n - 1)] * xk;
          img_axpy(Wt + r, n, cur, xk, k + 2 + sub, n);
        }
        if (t < n) sl[((k + 1) & 1) * NX + t] = nx;
        __syncthreads();
      }
      if (t < n) {                                  // half 0: r = t
        sg[t] = 1.0 / sqrt(gd);
        if (ipr) ipr[t] = p4[t] / (gd * gd);
      }
      __syncthreads();                              // sg and W are written, the buffers are free
      os = gram_offdiag<true>((cgdouble *)Wt, n, (cgdouble *)Wt, n, n, buf, sg);
    } else if (t < n && ipr) {
      ipr[t] = __builtin_nan("");
    }
  }
  const double osum = wg_reduce<NW, false>(os, red);
  if (t == 0) {
    out[0] = nrm;
    out[1] = rsum / (double)n;
    out[2] = rmax;
    out[3] = spd ? sqrt(osum) : __builtin_nan("");
  }
}

template <int ITYPE, typename ARGS>
static int launch(hipStream_t s, int count, const ARGS &a) {
  constexpr size_t lds = (size_t)kLdsDoubles * sizeof(double);
  static bool raised = false;                       // one per instantiation
  if (!raised) {
    EK_HIP_CHECK(hipFuncSetAttribute((const void *)xcheck_sygv_kernel<ITYPE, ARGS>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    raised = true;
  }
  hipLaunchKernelGGL((xcheck_sygv_kernel<ITYPE, ARGS>), dim3(count), dim3(T), lds, s, a);
  EK_HIP_CHECK(hipGetLastError());
  return 0;
}

// this unit's part of a call (bcheck::uniform_entry does the rest): the scratch is indexed by workgroup
static int launch_uniform(hipStream_t s, const bcheck::Uniform &u, const int *map, int first, int count, double *S,
                          double *dout, double *dipr) {
  Args a{u.itype, u.n, u.A, u.lda, u.sA, u.B, u.ldb, u.sB, u.w, u.Z, u.ldz, u.sZ, map, first, S, dout, dipr};
  return u.itype == 2 ? launch<2>(s, count, a) : launch<3>(s, count, a);
}

static int entry(const bcheck::Uniform &u, bool nothing, bool host) {
  return bcheck::uniform_entry(u, nothing, host, (size_t)(u.itype - 1) * u.n * u.n, true, launch_uniform);
}

}  // namespace xcheck_sygv

// the variable form's launch (ek_batched_check.h): `count` entries of the table, every one of an order above
// EK_HIP_BATCH_NMAX, itype 2 or 3
int bcheck::launch_sygv_x(hipStream_t s, int itype, int count, const VArgs &a) {
  return itype == 2 ? xcheck_sygv::launch<2>(s, count, a) : xcheck_sygv::launch<3>(s, count, a);
}

}  // namespace ek

using namespace ek;

extern "C" {

// the argument errors of ek_hip_check_sygv_batched* with EK_HIP_XBATCH_NMAX in the place of EK_HIP_BATCH_NMAX
int ek_hip_check_sygv_xbatched_device(int itype, int n, int batch, const double *dA, int lda, long long strideA,
                                      const double *dB, int ldb, long long strideB, const double *dw, const double *dZ,
                                      int ldz, long long strideZ, const int *info, double *out, double *ipr,
                                      double *seconds) {
  if (itype < 1 || itype > 3) return -1;
  const bcheck::Uniform u{itype, 1, n, batch, dA, lda, strideA, dB, ldb, strideB, dw, dZ, ldz, strideZ, info, out, ipr,
                          seconds};
  bool nothing;
  int rc = bcheck::uniform_arguments(u, EK_HIP_XBATCH_NMAX, &nothing);
  if (rc) return rc;
  if (n <= EK_HIP_BATCH_NMAX)                       // n = 0 included: the same answers, the same kernel, the same bits
    return ek_hip_check_sygv_batched_device(itype, n, batch, dA, lda, strideA, dB, ldb, strideB, dw, dZ, ldz, strideZ,
                                            info, out, ipr, seconds);
  if (itype == 1)                                   // type 1 is problem 1 of the first family
    return ek_hip_check_xbatched_device(1, n, batch, dA, lda, strideA, dB, ldb, strideB, dw, dZ, ldz, strideZ, info, out,
                                        ipr, seconds);
  return xcheck_sygv::entry(u, nothing, false);
}

int ek_hip_check_sygv_xbatched(int itype, int n, int batch, const double *A, int lda, long long strideA, const double *B,
                               int ldb, long long strideB, const double *w, const double *Z, int ldz, long long strideZ,
                               const int *info, double *out, double *ipr, double *seconds) {
  if (itype < 1 || itype > 3) return -1;
  const bcheck::Uniform u{itype, 1, n, batch, A, lda, strideA, B, ldb, strideB, w, Z, ldz, strideZ, info, out, ipr,
                          seconds};
  bool nothing;
  int rc = bcheck::uniform_arguments(u, EK_HIP_XBATCH_NMAX, &nothing);
  if (rc) return rc;
  if (n <= EK_HIP_BATCH_NMAX)
    return ek_hip_check_sygv_batched(itype, n, batch, A, lda, strideA, B, ldb, strideB, w, Z, ldz, strideZ, info, out, ipr,
                                     seconds);
  if (itype == 1)
    return ek_hip_check_xbatched(1, n, batch, A, lda, strideA, B, ldb, strideB, w, Z, ldz, strideZ, info, out, ipr,
                                 seconds);
  return xcheck_sygv::entry(u, nothing, true);
}

}  // extern "C"
