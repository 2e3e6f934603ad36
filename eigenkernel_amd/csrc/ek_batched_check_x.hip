// ek_batched_check_x.hip -- ek_hip_check_xbatched*: the batched acceptance checks for the orders
// EK_HIP_BATCH_NMAX + 1 .. EK_HIP_XBATCH_NMAX that ek_hip_eigenpairs_xbatched* solves.  Orders up to
// EK_HIP_BATCH_NMAX are forwarded to ek_hip_check_batched*.  This unit holds the kernel, its launch and the entries; the
// argument checker, the device pool, the chunk loop, the fetch and the scatter are ek_batched_check.hip's.
// The kernel has a second instantiation per problem kind that finds its problem in the variable form's table
// (bcheck::launch_x, behind ek_hip_check_xvbatched*: DESIGN.md 24); the passes exist once.
//
// One workgroup of 512 threads (8 waves) owns a problem from its first load to its last store.  At these orders neither Z
// nor S = B Z nor A Z fits in LDS (512 KB each at n = 256), so the three products run on the fp64 matrix cores
// (v_mfma_f64_16x16x4_f64) over LDS-staged tiles: an output tile has 128 rows x 64 columns, wave v owns its rows
// 16 v .. 16 v + 15 as four 16 x 16 accumulator tiles per product, and the inner dimension advances 16 at a time through two
// LDS buffers (the next step's operands travel global -> registers while this step's are multiplied, then go to the other
// buffer: one barrier per step).
//
//   1  A Z and, for a generalized problem, S = B Z in the same sweep (one staged tile of Z feeds both).  The loader of the
//      symmetric operands takes entry (i, k) with k > i from (k, i): a 16 x 16 block below the diagonal is read along i,
//      one above it as the mirrored block along k and transposed on its way into LDS, the diagonal block entry by entry;
//      nothing strictly above the diagonal and nothing at or beyond row n is read, and the tile is zero past n.  The
//      squares of the staged entries of A give ||A||_F.  The epilogue works in the accumulators: r_ij = (A Z)_ij - w_j s_ij,
//      and r^2, z s and z^4 are summed per column -- in the lane over its four rows, in the wave over the four lane >> 4
//      groups, over the waves in ascending order through LDS, over the row tiles in ascending order.  S goes to a device
//      scratch of n^2 doubles (a standard problem has S = Z and needs neither the scratch nor the second accumulators)
//   2  G = Z^T S with the same machinery, both operands from global memory; entry (l, j), l != j, is scaled by
//      G_ll^-1/2 G_jj^-1/2 from step 1, squared and added to its thread's sum in tile order
//
// Same bits wherever a problem sits: every loop bound and every summation order depends on n alone; no atomics; the same
// kernel behind the host and the device form.  A, B, w and Z are read only.
#include "ek_batched_check_x.h"

namespace ek {
namespace xcheck {

constexpr int kBuf = 2 * kTileP + kTileQ;           // A, B, Z of one step (step 2: Z^T, unused, S)

// LDS doubles: two buffers, the waves' column sums of r^2, z s and z^4, 1 / sqrt(G_jj), a word per wave
constexpr int kLdsDoubles = 2 * kBuf + 3 * NW * TN + EK_HIP_XBATCH_NMAX + NW;

struct Args {
  int problem, n;
  const double *A; int lda; long long sA;
  const double *B; int ldb; long long sB;
  const double *w;
  const double *Z; int ldz; long long sZ;
  const int *map;       // the problems to check; nullptr: every problem
  int first;            // this launch's first entry of the map (or first problem)
  double *S;            // problem 1: n^2 doubles per workgroup of a launch
  double *out;          // EK_HIP_CHECK_NOUT doubles per problem
  double *ipr;          // n doubles per problem, or nullptr
};

// the uniform launch's problem: entry first + workgroup of the map (or that problem), the scratch by workgroup
template <bool GEN>
__device__ __forceinline__ bcheck::Problem locate_x(const Args &a) {
  const int n = a.n;
  const long long pb = a.map ? a.map[a.first + (int)blockIdx.x] : a.first + (int)blockIdx.x;
  return {n, (cgdouble *)(a.A + pb * a.sA), a.lda, GEN ? (cgdouble *)(a.B + pb * a.sB) : nullptr, a.ldb,
          (cgdouble *)(a.w + pb * n), (cgdouble *)(a.Z + pb * a.sZ), a.ldz,
          GEN ? (gdouble *)(a.S + (long long)blockIdx.x * n * n) : nullptr, (gdouble *)(a.out + pb * EK_HIP_CHECK_NOUT),
          a.ipr ? (gdouble *)(a.ipr + pb * n) : nullptr};
}
template <bool GEN>
__device__ __forceinline__ bcheck::Problem locate_x(const bcheck::VArgs &a) { return bcheck::locate(a); }

// ARGS: how the workgroup finds its problem -- Args (one order, strided; the scratch by workgroup) or bcheck::VArgs (entry
// blockIdx.x of the launch's slice of the table, which names the entry's own scratch)
template <bool GEN, typename ARGS>
__global__ __launch_bounds__(T) void xcheck_kernel(ARGS a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double *buf = smem;                               // [2][kBuf]
  double *cs = buf + 2 * kBuf;                      // [3][NW][TN]: the waves' column sums
  double *sg = cs + 3 * NW * TN;                    // 1 / sqrt(G_jj)
  double *red = sg + EK_HIP_XBATCH_NMAX;            // a word per wave

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l15 = lane & 15, l4 = lane >> 4;
  const bcheck::Problem p = locate_x<GEN>(a);
  const int n = p.n;
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
  for (int j0 = 0; j0 < n; j0 += TN) {
    double wj[4];
#pragma unroll
    for (int jt = 0; jt < 4; ++jt) {
      const int j = j0 + 16 * jt + l15;
      wj[jt] = (j < n) ? w[j] : 0.0;
    }
    double tr = 0.0, tg = 0.0, tp = 0.0;            // thread c < TN: column j0 + c, over the row tiles
#pragma unroll 1
    for (int i0 = 0; i0 < n; i0 += TM) {
      double4_t accA[4], accB[4];
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) accA[jt] = accB[jt] = (double4_t){0.0, 0.0, 0.0, 0.0};
      double va[4], vb[4], vz[2];
      auto fetch = [&](int k0) {
        sym_tile(A, lda, n, i0, k0, va);
        if (GEN) sym_tile(B, ldb, n, i0, k0, vb);
        col_tile<TN>(Z, ldz, n, k0, j0, vz);
      };
      auto put = [&](int k0, double *s) {
        sym_put(s, i0, k0, va);
        if (GEN) sym_put(s + kTileP, i0, k0, vb);
        col_put<TN, LDQ>(s + 2 * kTileP, vz);
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
        const double *cur = buf + (s & 1) * kBuf;
        const bool more = s + 1 < nk;
        if (more) fetch((s + 1) * KT);
        step_mfma<GEN>(cur, cur + kTileP, cur + 2 * kTileP, accA, accB);
        if (more) put((s + 1) * KT, buf + ((s + 1) & 1) * kBuf);
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
          if (i < n && j < n) {
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
    if (t < TN && j0 + t < n) {
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

  // ---- 2: || D^-1/2 G D^-1/2 - its diagonal ||_F, G = Z^T S
  cgdouble *Q = GEN ? (cgdouble *)S : Z;
  const int ldq = GEN ? n : ldz;
  double os = 0.0;
#pragma unroll 1
  for (int j0 = 0; j0 < n; j0 += TN)
#pragma unroll 1
    for (int l0 = 0; l0 < n; l0 += TM) {
      double4_t acc[4];
#pragma unroll
      for (int jt = 0; jt < 4; ++jt) acc[jt] = (double4_t){0.0, 0.0, 0.0, 0.0};
      double vp[4], vq[2];
      col_tile<TM>(Z, ldz, n, 0, l0, vp);
      col_tile<TN>(Q, ldq, n, 0, j0, vq);
      col_put<TM, LDP>(buf, vp);
      col_put<TN, LDQ>(buf + 2 * kTileP, vq);
      __syncthreads();
#pragma unroll 1
      for (int s = 0; s < nk; ++s) {
        const double *cur = buf + (s & 1) * kBuf;
        double *nxt = buf + ((s + 1) & 1) * kBuf;
        const bool more = s + 1 < nk;
        if (more) {
          col_tile<TM>(Z, ldz, n, (s + 1) * KT, l0, vp);
          col_tile<TN>(Q, ldq, n, (s + 1) * KT, j0, vq);
        }
        step_mfma<false>(cur, cur, cur + 2 * kTileP, acc, acc);
        if (more) {
          col_put<TM, LDP>(nxt, vp);
          col_put<TN, LDQ>(nxt + 2 * kTileP, vq);
        }
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
  const double osum = wg_reduce<NW, false>(os, red);
  if (t == 0) {
    out[0] = anorm;
    out[1] = rsum / anorm / (double)n;
    out[2] = rmax / anorm;
    out[3] = sqrt(osum);
  }
}

template <bool GEN, typename ARGS>
static int launch(hipStream_t s, int count, const ARGS &a) {
  constexpr size_t lds = (size_t)kLdsDoubles * sizeof(double);
  static bool raised = false;                       // one per instantiation
  if (!raised) {
    EK_HIP_CHECK(hipFuncSetAttribute((const void *)xcheck_kernel<GEN, ARGS>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds));
    raised = true;
  }
  hipLaunchKernelGGL((xcheck_kernel<GEN, ARGS>), dim3(count), dim3(T), lds, s, a);
  EK_HIP_CHECK(hipGetLastError());
  return 0;
}

// this unit's part of a call (bcheck::uniform_entry does the rest): the scratch is indexed by workgroup
static int launch_uniform(hipStream_t s, const bcheck::Uniform &u, const int *map, int first, int count, double *S,
                          double *dout, double *dipr) {
  Args a{u.problem, u.n, u.A, u.lda, u.sA, u.B, u.ldb, u.sB, u.w, u.Z, u.ldz, u.sZ, map, first, S, dout, dipr};
  return u.problem ? launch<true>(s, count, a) : launch<false>(s, count, a);
}

static int entry(const bcheck::Uniform &u, bool nothing, bool host) {
  return bcheck::uniform_entry(u, nothing, host, u.problem ? (size_t)u.n * u.n : 0, true, launch_uniform);
}

}  // namespace xcheck

// the variable form's launch (ek_batched_check.h): `count` entries of the table, every one of an order above
// EK_HIP_BATCH_NMAX, a.problem says which instantiation
int bcheck::launch_x(hipStream_t s, int count, const VArgs &a) {
  return a.problem ? xcheck::launch<true>(s, count, a) : xcheck::launch<false>(s, count, a);
}

}  // namespace ek

using namespace ek;

extern "C" {

// the argument errors of ek_hip_check_batched* with EK_HIP_XBATCH_NMAX in the place of EK_HIP_BATCH_NMAX
int ek_hip_check_xbatched_device(int problem, int n, int batch, const double *dA, int lda, long long strideA,
                                 const double *dB, int ldb, long long strideB, const double *dw, const double *dZ,
                                 int ldz, long long strideZ, const int *info, double *out, double *ipr,
                                 double *seconds) {
  const bcheck::Uniform u{0, problem, n, batch, dA, lda, strideA, dB, ldb, strideB, dw, dZ, ldz, strideZ, info, out, ipr,
                          seconds};
  bool nothing;
  int rc = bcheck::uniform_arguments(u, EK_HIP_XBATCH_NMAX, &nothing);
  if (rc) return rc;
  if (n <= EK_HIP_BATCH_NMAX)                       // n = 0 included: the same answers, the same kernel, the same bits
    return ek_hip_check_batched_device(problem, n, batch, dA, lda, strideA, dB, ldb, strideB, dw, dZ, ldz, strideZ, info,
                                       out, ipr, seconds);
  return xcheck::entry(u, nothing, false);
}

int ek_hip_check_xbatched(int problem, int n, int batch, const double *A, int lda, long long strideA, const double *B,
                          int ldb, long long strideB, const double *w, const double *Z, int ldz, long long strideZ,
                          const int *info, double *out, double *ipr, double *seconds) {
  const bcheck::Uniform u{0, problem, n, batch, A, lda, strideA, B, ldb, strideB, w, Z, ldz, strideZ, info, out, ipr,
                          seconds};
  bool nothing;
  int rc = bcheck::uniform_arguments(u, EK_HIP_XBATCH_NMAX, &nothing);
  if (rc) return rc;
  if (n <= EK_HIP_BATCH_NMAX)
    return ek_hip_check_batched(problem, n, batch, A, lda, strideA, B, ldb, strideB, w, Z, ldz, strideZ, info, out, ipr,
                                seconds);
  return xcheck::entry(u, nothing, true);
}

}  // extern "C"
