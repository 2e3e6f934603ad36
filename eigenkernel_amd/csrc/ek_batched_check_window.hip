// ek_batched_check_window.hip -- ek_hip_check_window_xbatched*: the batched acceptance checks for what
// ek_hip_eigenpairs_window_xbatched* returns: per problem the c = m[b] values w[0 .. c) and the columns 0 .. c-1 of an
// n x zcap array, every order 1 .. EK_HIP_XBATCH_NMAX in one kernel class.  This unit holds the kernel, its
// launch and the entries; the argument checker, the device pool, the chunk loop, the fetch and the scatter are
// ek_batched_check.hip's (bcheck::window_arguments, bcheck::window_entry).
//
// The machinery is ek_batched_check_x.hip's made rectangular: one workgroup of 512 threads (8 waves) owns a problem from
// its first load to its last store, the products run on the fp64 matrix cores over LDS-staged tiles of 128 rows x 64
// columns with the operands in device memory, the inner dimension advances 16 at a time through two LDS buffers with one
// barrier per step, and the symmetric loader mirrors the blocks above the diagonal.
//
//   1  over the column tiles j0 < c and the row tiles i0 < n: A Z and, for a generalized problem, S = B Z in one sweep;
//      ||A||_F from the staged entries of A of the first column tile; r, z s and z^4 summed per column in the accumulators
//      in the order of ek_batched_check_x.hip.  S goes to a device scratch of n x c doubles, leading dimension n
//   2  G = Z^T S over the c x c tiles only, inner dimension n; entry (l, j), l != j, scaled by G_ll^-1/2 G_jj^-1/2
//
// A tile is made of 16-row strips (one per wave) and 16-column subtiles; a strip that lies wholly past the last row (n in
// step 1, c in step 2) and a subtile wholly past column c issue no matrix instruction, so a window of c <= 16, 32, 48
// columns pays for a tile of that width and the ragged last row tile of n = 129 for one strip.  The loader of Z bounds
// rows by n and columns by c: nothing of w or Z from m[b] on is read.
//
// Same bits wherever a problem sits: every loop bound, every skipped strip and every summation order depends on (n, c)
// alone; no atomics; the same kernel behind the host and the device form.  A, B, w and Z are read only.
//
// The kernel has a second instantiation per problem kind that finds order, c and addresses in the variable form's table
// (bcheck::launch_window_v, behind ek_hip_check_window_xvbatched*: DESIGN.md 37); the passes exist once.
#include "ek_batched_check_x.h"

namespace ek {
namespace wcheck {

using namespace xcheck;

constexpr int kBuf = 2 * kTileP + kTileQ;           // A, B, Z of one step (step 2: Z^T, unused, S)

// LDS doubles: two buffers, the waves' column sums of r^2, z s and z^4, 1 / sqrt(G_jj), a word per wave
constexpr int kLdsDoubles = 2 * kBuf + 3 * NW * TN + EK_HIP_XBATCH_NMAX + NW;

struct Args {
  int problem, n;
  const double *A; int lda; long long sA;
  const double *B; int ldb; long long sB;
  const double *w;
  const double *Z; int ldz; long long sZ;
  const int *map;       // entry e: the pair (problem, m[problem]) in map[2 e], map[2 e + 1]
  int first;            // this launch's first entry of the map
  double *S; long long sS;   // problem 1: sS = n x (the largest checked m) doubles per workgroup of a launch
  double *out;          // EK_HIP_CHECK_NOUT doubles per problem
  double *ipr;          // n doubles per problem, or nullptr
};

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

// one step of 16 of the inner dimension for this wave's strip: acc += P^T-tile rows x the first nsub subtiles of the Q-tile
template <bool TWO>
__device__ __forceinline__ void step_strip(const double *sp, const double *sp2, const double *sq, int wave, int nsub,
                                           double4_t (&acc)[4], double4_t (&acc2)[4]) {
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

// the uniform launch's problem: entry first + workgroup of the map, the scratch by workgroup
template <bool GEN>
__device__ __forceinline__ bcheck::WProblem locate_w(const Args &a) {
  const int n = a.n;
  const int e = a.first + (int)blockIdx.x;
  const long long pb = a.map[2 * e];
  const int c = a.map[2 * e + 1];                   // 1 <= c <= n
  return {n, c, (cgdouble *)(a.A + pb * a.sA), a.lda, GEN ? (cgdouble *)(a.B + pb * a.sB) : nullptr, a.ldb,
          (cgdouble *)(a.w + pb * n), (cgdouble *)(a.Z + pb * a.sZ), a.ldz,
          GEN ? (gdouble *)(a.S + (long long)blockIdx.x * a.sS) : nullptr, (gdouble *)(a.out + pb * EK_HIP_CHECK_NOUT),
          a.ipr ? (gdouble *)(a.ipr + pb * n) : nullptr};
}
template <bool GEN>
__device__ __forceinline__ bcheck::WProblem locate_w(const bcheck::VArgs &a) { return bcheck::locate_window(a); }

// ARGS: how the workgroup finds its problem -- Args (one order, strided; the scratch by workgroup) or bcheck::VArgs (entry
// blockIdx.x of the launch's slice of the table, which names the entry's order, its m and its own scratch: DESIGN.md 37)
template <bool GEN, typename ARGS>
__global__ __launch_bounds__(T) void wcheck_kernel(ARGS a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  constexpr int kB = kBuf, kQ = 2 * kTileP;         // a buffer; where its tile of Z (or S) starts
  double *buf = smem;                               // [2][kB]
  double *cs = buf + 2 * kB;                        // [3][NW][TN]: the waves' column sums
  double *sg = cs + 3 * NW * TN;                    // 1 / sqrt(G_jj)
  double *red = sg + EK_HIP_XBATCH_NMAX;            // a word per wave

  const int t = threadIdx.x, lane = t & 63, l15 = lane & 15, l4 = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);   // scalar: a skipped strip is a branch, not a mask
  const bcheck::WProblem p = locate_w<GEN>(a);
  const int n = p.n, c = p.c;
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
      wj[jt] = (j < c) ? w[min(j, c - 1)] : 0.0;
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
        rect_tile<TN>(Z, ldz, n, c, k0, j0, vz);
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
        if (strip) step_strip<GEN>(cur, cur + kTileP, cur + kQ, wave, nsub, accA, accB);
        if (more) put((s + 1) * KT, buf + ((s + 1) & 1) * kB);
        __syncthreads();
      }
      // the epilogue, in the accumulators: acc[jt][r] is entry (i0 + 16 wave + l4 + 4 r, j0 + 16 jt + l15)
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
      rect_tile<TM>(Z, ldz, n, c, 0, l0, vp);
      rect_tile<TN>(Q, ldq, n, c, 0, j0, vq);
      col_put<TM, LDP>(buf, vp);
      col_put<TN, LDQ>(buf + kQ, vq);
      __syncthreads();
#pragma unroll 1
      for (int s = 0; s < nk; ++s) {
        const double *cur = buf + (s & 1) * kB;
        double *nxt = buf + ((s + 1) & 1) * kB;
        const bool more = s + 1 < nk;
        if (more) {
          rect_tile<TM>(Z, ldz, n, c, (s + 1) * KT, l0, vp);
          rect_tile<TN>(Q, ldq, n, c, (s + 1) * KT, j0, vq);
        }
        if (strip) step_strip<false>(cur, cur, cur + kQ, wave, nsub, acc, acc);
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

template <bool GEN, typename ARGS>
static int launch(hipStream_t s, int count, const ARGS &a) {
  constexpr size_t lds = (size_t)kLdsDoubles * sizeof(double);
  static bool raised = false;                       // one per instantiation
  if (!raised) {
    EK_HIP_CHECK(hipFuncSetAttribute((const void *)wcheck_kernel<GEN, ARGS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds));
    raised = true;
  }
  hipLaunchKernelGGL((wcheck_kernel<GEN, ARGS>), dim3(count), dim3(T), lds, s, a);
  EK_HIP_CHECK(hipGetLastError());
  return 0;
}

// this unit's part of a call (bcheck::window_entry does the rest): the scratch is indexed by workgroup
static int launch_window(hipStream_t s, const bcheck::Window &w, const int *map, int first, int count, long long sS,
                         double *S, double *dout, double *dipr) {
  const bcheck::Uniform &u = w.u;
  Args a{u.problem, u.n, u.A, u.lda, u.sA, u.B, u.ldb, u.sB, u.w, u.Z, u.ldz, u.sZ, map, first, S, sS, dout, dipr};
  return u.problem ? launch<true>(s, count, a) : launch<false>(s, count, a);
}

static int entry(int problem, int n, int batch, const double *A, int lda, long long strideA, const double *B, int ldb,
                 long long strideB, const int *m, const double *w, const double *Z, int ldz, int zcap, long long strideZ,
                 const int *info, double *out, double *ipr, double *seconds, bool host) {
  const bcheck::Window win{{0, problem, n, batch, A, lda, strideA, B, ldb, strideB, w, Z, ldz, strideZ, info, out, ipr,
                            seconds}, m, zcap};
  bool nothing;
  int rc = bcheck::window_arguments(win, EK_HIP_XBATCH_NMAX, &nothing);
  if (rc) return rc;
  return bcheck::window_entry(win, nothing, host, launch_window);
}

}  // namespace wcheck

// the variable form's launch (ek_batched_check.h): `count` entries of the table, a.problem says which instantiation
int bcheck::launch_window_v(hipStream_t s, int count, const VArgs &a) {
  return a.problem ? wcheck::launch<true>(s, count, a) : wcheck::launch<false>(s, count, a);
}

}  // namespace ek

using namespace ek;

extern "C" {

int ek_hip_check_window_xbatched_device(int problem, int n, int batch, const double *dA, int lda, long long strideA,
                                        const double *dB, int ldb, long long strideB, const int *m, const double *dw,
                                        const double *dZ, int ldz, int zcap, long long strideZ, const int *info,
                                        double *out, double *ipr, double *seconds) {
  return wcheck::entry(problem, n, batch, dA, lda, strideA, dB, ldb, strideB, m, dw, dZ, ldz, zcap, strideZ, info, out, ipr,
                       seconds, false);
}

int ek_hip_check_window_xbatched(int problem, int n, int batch, const double *A, int lda, long long strideA,
                                 const double *B, int ldb, long long strideB, const int *m, const double *w,
                                 const double *Z, int ldz, int zcap, long long strideZ, const int *info, double *out,
                                 double *ipr, double *seconds) {
  return wcheck::entry(problem, n, batch, A, lda, strideA, B, ldb, strideB, m, w, Z, ldz, zcap, strideZ, info, out, ipr,
                       seconds, true);
}

}  // extern "C"
