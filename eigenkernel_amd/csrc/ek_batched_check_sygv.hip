// ek_batched_check_sygv.hip -- the kernel behind ek_hip_check_sygv_batched* / ek_hip_check_sygv_vbatched* for DSYGV's types
// 2 (A B x = l x) and 3 (B A x = l x): the quantities of DESIGN.md 16 for every problem of a batch, one workgroup per
// problem, with the classes, the LDS image, the staged row streaming, the sums and the output words of
// ek_batched_check.hip, whose host side launches it (launch_sygv).  B = L L^T:
//   r_j = A (B z_j) - w_j z_j (type 2), B (A z_j) - w_j z_j (type 3);  rho_j = ||r_j|| / (||A||_F ||B||_F ||z_j||)
//   G = Z^T B Z (type 2), (L^-1 Z)^T (L^-1 Z) (type 3);  ipr_j = sum_i z_ij^4 / G_jj^2
//   out: ||A||_F ||B||_F, sum_j rho_j / n, max_j rho_j, || D^-1/2 G D^-1/2 with zero diagonal ||_F
// Fixed loop orders, every multiply-add an fma(), sums over the workgroup by wg_reduce, no atomics: a problem's outputs
// depend on (itype, n, A, B, w, Z) alone.  A, B, w and Z are read only.
#include "ek_batched_check.h"

namespace ek {
namespace bcheck {

// The rows of the symmetric M (lower triangle referenced) stream through the staged vectors st ([buffer][half][NC]), two
// a step (row 2m + h for half h), loaded a step ahead, as in stage 1 of the kernel of ek_batched_check.hip.  f(i, row, z)
// runs in thread (r, h) for its row i with the row in LDS; with ZR, z = z_ir of the caller's Z travels with the row.
// Returns the sum of the squares of the entries this thread staged: over the workgroup, ||M||_F^2.  Ends behind a barrier.
template <int NC, bool ZR, typename F>
__device__ __forceinline__ double stream_rows(cgdouble *M, int ld, cgdouble *Z, int ldz, int n, int r, int h, double *st,
                                              F f) {
  const bool col = r < n;
  auto entry = [&](int i) { return (r <= i) ? M[i + (size_t)r * ld] : M[r + (size_t)i * ld]; };
  double sq = 0.0, z = 0.0;
  {
    double x = 0.0;
    if (col && h < n) {
      x = entry(h);
      if (ZR) z = Z[h + (size_t)r * ldz];
    }
    st[h * NC + r] = x;
    sq = fma(x, x, sq);
  }
  __syncthreads();
  const int steps = (n + 1) >> 1;
  for (int m = 0; m < steps; ++m) {
    const int i = 2 * m + h, in = i + 2;
    double xn = 0.0, zn = 0.0;                      // the row after this one: in flight while this one is used
    if (col && in < n) {
      xn = entry(in);
      if (ZR) zn = Z[in + (size_t)r * ldz];
    }
    if (col && i < n) f(i, st + ((m & 1) * 2 + h) * NC, z);
    st[(((m + 1) & 1) * 2 + h) * NC + r] = xn;
    sq = fma(xn, xn, sq);
    z = zn;
    __syncthreads();
  }
  return sq;
}

// the image <- the n x n matrix X (leading dimension ldx), thread (r, h) row r of the columns of its half
template <int NC>
__device__ __forceinline__ void load_image(double *Zs, cgdouble *X, int ldx, int n, int r, int h) {
  if (r < n)
    for (int j = h; j < n; j += 2) Zs[r + j * (NC + 1)] = X[r + (size_t)j * ldx];
}

// Types 2 and 3 of a problem.  With S the scratch of n^2 doubles and the image in LDS:
//   type 2   the rows of B stream over the image of Z: S = B Z, G_jj = sum_i z_ij s_ij, sum z^4, ||z_j||^2, ||B||_F^2;
//            G = Z^T S column of S by column of S (stage 3 of that kernel: slot 3 and the IPRs are type 1's bits
//            for the same B and Z); the image <- S; the rows of A stream: r_ir = (A S)_ir - w_r z_ir, ||A||_F^2
//   type 3   the rows of A stream over the image of Z: U = A Z to S, sum z^4, ||z_j||^2, ||A||_F^2; the image <- U; the
//            rows of B stream: r_ir = (B U)_ir - w_r z_ir, ||B||_F^2; the image <- the lower triangle of B, factored in
//            place (right-looking, a column a step); L to S; the image <- Z, W = L^-1 Z by forward substitution (a
//            thread pair per column, a column of L a step, staged from S a step ahead); G = W^T W from the image
// A pivot of B that is not positive and finite: slot 3 and the IPRs are NaN, the residual slots stand.
template <int NC, int T, int ITYPE>
__device__ __forceinline__ void check_sygv(const Problem &p, double *smem) {
  constexpr int LD = NC + 1, NW = T / 64;
  double *Zs = smem;
  double *sa = Zs + NC * LD;                        // [buffer][half][NC]; the halves' sums; columns of S and of L
  double *sg = sa + 8 * NC;                         // 1 / sqrt(G_jj); type 3: the diagonal of L before that
  double *red = sg + NC;
  const int t = threadIdx.x, n = p.n;
  const int r = t % NC, h = t / NC;
  const bool col = r < n, own = col && h == 0;
  gdouble *S = p.S;
  double *zc = Zs + r * LD;
  const double wr = col ? p.w[r] : 0.0;
  const int steps = (n + 1) >> 1;

  load_image<NC>(Zs, p.Z, p.ldz, n, r, h);
  // ---- the first product: S = B Z (type 2) or A Z (type 3), and what depends on Z alone
  double gd = 0.0, p4 = 0.0, zz = 0.0;
  const double sq1 = stream_rows<NC, false>(ITYPE == 2 ? p.B : p.A, ITYPE == 2 ? p.ldb : p.lda, nullptr, 0, n, r, h, sa,
                                            [&](int i, const double *row, double) {
    const double zi = zc[i];
    const double sz = lds_dot(row, zc, n);
    S[i + (size_t)r * n] = sz;
    const double z2 = zi * zi;
    if (ITYPE == 2) gd = fma(zi, sz, gd);
    p4 = fma(z2, z2, p4);
    zz += z2;
  });
  sa[h * NC + r] = gd;
  sa[(2 + h) * NC + r] = p4;
  sa[(4 + h) * NC + r] = zz;
  __syncthreads();
  double q = 0.0, znorm = 0.0;                      // of column r, in its thread of half 0
  if (own) {
    q = sa[2 * NC + r] + sa[3 * NC + r];
    znorm = sqrt(sa[4 * NC + r] + sa[5 * NC + r]);
    if (ITYPE == 2) {
      const double g = sa[r] + sa[NC + r];
      sg[r] = 1.0 / sqrt(g);
      if (p.ipr) p.ipr[r] = q / (g * g);
    }
  }
  __syncthreads();                                  // sg is written, S is in the scratch for the whole workgroup

  double os = 0.0;
  if (ITYPE == 2) {                                 // || D^-1/2 (Z^T S) D^-1/2 - its diagonal ||_F
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
  }

  // ---- the second product over the image of the first: r_ir = (A S)_ir - w_r z_ir (type 3: B U)
  load_image<NC>(Zs, S, n, n, r, h);
  double rs = 0.0;
  const double sq2 = stream_rows<NC, true>(ITYPE == 2 ? p.A : p.B, ITYPE == 2 ? p.lda : p.ldb, p.Z, p.ldz, n, r, h, sa,
                                           [&](int, const double *row, double z) {
    const double rr = fma(-wr, z, lds_dot(row, zc, n));
    rs = fma(rr, rr, rs);
  });
  sa[h * NC + r] = rs;
  __syncthreads();
  const double rn = own ? sqrt(sa[r] + sa[NC + r]) : 0.0;
  const double nrm = sqrt(wg_reduce<NW, false>(sq1, red)) * sqrt(wg_reduce<NW, false>(sq2, red));
  const double rho = own ? rn / (nrm * znorm) : 0.0;
  const double rsum = wg_reduce<NW, false>(rho, red);
  const double rmax = wg_reduce<NW, true>(rho, red);

  bool spd = true;
  if (ITYPE == 3) {
    __syncthreads();                                // the image and the staged vectors are free
    if (col)
      for (int j = h; j <= r; j += 2) Zs[r + j * LD] = p.B[r + (size_t)j * p.ldb];
    __syncthreads();
    // B = L L^T in the image, right-looking: column k scaled (staged in sa, so that nobody overwrites what another still
    // reads), then the columns to its right updated, thread (r, h) row r of the columns of its half
    for (int k = 0; k < n; ++k) {
      const double d = Zs[k + k * LD];              // the same word in every thread: the exit is uniform
      if (!(d > 0.0 && d < INFINITY)) { spd = false; break; }
      const double s = sqrt(d);
      double l = 0.0;
      if (col && r >= k) l = (r == k) ? s : Zs[r + k * LD] / s;
      if (own && r >= k) sa[r] = l;
      __syncthreads();
      if (own && r >= k) Zs[r + k * LD] = l;
      if (col)
        for (int j = k + 1 + h; j <= r; j += 2) Zs[r + j * LD] = fma(-l, sa[j], Zs[r + j * LD]);
      __syncthreads();
    }
    if (spd) {
      if (col)
        for (int j = h; j <= r; j += 2) S[r + (size_t)j * n] = Zs[r + j * LD];
      if (own) sg[r] = Zs[r + r * LD];
      __syncthreads();                              // L is in the scratch, its diagonal in sg
      load_image<NC>(Zs, p.Z, p.ldz, n, r, h);
      if (h == 0) sa[r] = col ? S[r] : 0.0;
      __syncthreads();
      // W = L^-1 Z: step k subtracts l_ik w_kr from the rows i > k of column r, half h the rows i = h (mod 2); the owner
      // of row k + 1 finishes it (the division by l_k+1,k+1) in the same step, so that step k + 1 finds w_k+1,r
      if (own) zc[0] = zc[0] / sg[0];
      __syncthreads();
      for (int k = 0; k + 1 < n; ++k) {
        double xn = 0.0;                            // column k + 1 of L, below its diagonal
        if (own && r > k + 1) xn = S[r + (size_t)(k + 1) * n];
        if (col) {
          const double wk = zc[k];
          const double *lk = sa + (k & 1) * NC;
          for (int i = k + 1 + ((k + 1 + h) & 1); i < n; i += 2) {
            double zi = fma(-lk[i], wk, zc[i]);
            if (i == k + 1) zi = zi / sg[i];
            zc[i] = zi;
          }
        }
        if (h == 0) sa[((k + 1) & 1) * NC + r] = xn;
        __syncthreads();
      }
      if (own) {
        const double g = lds_dot(zc, zc, n);
        sg[r] = 1.0 / sqrt(g);                      // every reader of the diagonal of L is behind the last barrier
        if (p.ipr) p.ipr[r] = q / (g * g);
      }
      __syncthreads();
      if (col)
        for (int j = h; j < n; j += 2) {
          if (j == r) continue;
          const double g = lds_dot(zc, Zs + j * LD, n) * sg[r] * sg[j];
          os = fma(g, g, os);
        }
    } else if (own && p.ipr) {
      p.ipr[r] = __builtin_nan("");
    }
  }
  const double osum = wg_reduce<NW, false>(os, red);
  if (t == 0) {
    p.out[0] = nrm;
    p.out[1] = rsum / (double)n;
    p.out[2] = rmax;
    p.out[3] = spd ? sqrt(osum) : __builtin_nan("");
  }
}

// ITYPE: 2 or 3; ARGS as in ek_batched_check.hip, one kernel body for the strided and the table form
template <int NC, int T, int ITYPE, typename ARGS>
__global__ __launch_bounds__(T) void check_sygv_kernel(ARGS a) {
  static_assert(T == 2 * NC && T % 64 == 0, "two threads per column");
  extern __shared__ double smem[];
  check_sygv<NC, T, ITYPE>(locate(a), smem);
}

template <int NC, int T, int ITYPE, typename ARGS>
static int launch_instance(hipStream_t s, int count, const ARGS &a) {
  constexpr size_t lds = (size_t)lds_doubles(NC) * sizeof(double);
  static bool raised = false;                       // one per instantiation
  if (lds > 64 * 1024 && !raised) {
    EK_HIP_CHECK(hipFuncSetAttribute((const void *)check_sygv_kernel<NC, T, ITYPE, ARGS>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    raised = true;
  }
  hipLaunchKernelGGL((check_sygv_kernel<NC, T, ITYPE, ARGS>), dim3(count), dim3(T), lds, s, a);
  EK_HIP_CHECK(hipGetLastError());
  return 0;
}

template <typename ARGS>
static int launch_any(hipStream_t s, int itype, int nc, int count, const ARGS &a) {
  if (itype == 2)
    return nc == 32 ? launch_instance<32, 64, 2>(s, count, a)
         : nc == 64 ? launch_instance<64, 128, 2>(s, count, a) : launch_instance<128, 256, 2>(s, count, a);
  return nc == 32 ? launch_instance<32, 64, 3>(s, count, a)
       : nc == 64 ? launch_instance<64, 128, 3>(s, count, a) : launch_instance<128, 256, 3>(s, count, a);
}

int launch_sygv(hipStream_t s, int itype, int nc, int count, const Args &a) { return launch_any(s, itype, nc, count, a); }
int launch_sygv(hipStream_t s, int itype, int nc, int count, const VArgs &a) { return launch_any(s, itype, nc, count, a); }

}  // namespace bcheck
}  // namespace ek
