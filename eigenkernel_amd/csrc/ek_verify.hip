// ek_verify.hip -- the reference's acceptance checks and IPR on GPU-resident data
// (SURVEY.md 8(f) rows 1-2): the same quantities, the same normalisations, the two
// SYMM/GEMM passes on the matrix cores.
//
//   residual       verifier.f90:75-204   R = A V - B V diag(w); avg/max of ||r_j||_2 / ||A||_F
//   orthogonality  verifier.f90:233-330  G = V^T B V, scaled by 1/sqrt(G_jj), zero diagonal, ||G||_F
//   IPR            distribute_matrix.f90:18-78   sum_i v_ij^4 / (sum_i v_ij (S v)_ij)^2
//
// All reductions run in a fixed order (one workgroup per column, no atomics).
#include "ek_common.h"

namespace ek {
namespace {

__device__ __forceinline__ double wg_sum(double v, double *red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// out[j] = sum_i A(i,j)^2  (one workgroup per column)
__global__ __launch_bounds__(256) void col_sumsq_kernel(int m, const double *__restrict__ A, int lda,
                                                        double *__restrict__ out) {
  __shared__ double red[4];
  const double *col = A + (size_t)blockIdx.x * lda;
  double s = 0.0;
  for (int i = threadIdx.x; i < m; i += 256) s += col[i] * col[i];
  s = wg_sum(s, red);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// R(:,j) *= -w[j]   (verifier.f90:160-163)
__global__ void scale_cols_kernel(int m, int n, double *R, int ldr, const double *__restrict__ w) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  for (int j = blockIdx.y; j < n; j += gridDim.y) R[(size_t)i + (size_t)j * ldr] *= -w[j];
}

// result[0] = sum, result[1] = max of sqrt(v[j]) over j < n (a NaN is kept); result[2] = sqrt(sum_j a[j])
__global__ __launch_bounds__(256) void finish_residual_kernel(int n, const double *__restrict__ colsq,
                                                              int na, const double *__restrict__ asq,
                                                              double *result) {
  __shared__ double red[4];
  __shared__ double mx[256];
  double s = 0.0, m = 0.0, a = 0.0;
  for (int j = threadIdx.x; j < n; j += 256) { const double r = sqrt(colsq[j]); s += r; m = (r > m || r != r) ? r : m; }
  for (int j = threadIdx.x; j < na; j += 256) a += asq[j];
  s = wg_sum(s, red);
  a = wg_sum(a, red);
  mx[threadIdx.x] = m;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      const double y = mx[threadIdx.x + o], x = mx[threadIdx.x];
      mx[threadIdx.x] = (y > x || y != y) ? y : x;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { result[0] = s; result[1] = mx[0]; result[2] = sqrt(a); }
}

// G(i,j) <- G(i,j) / sqrt(G_ii G_jj), diagonal zeroed; colsq[j] = sum_i of the scaled squares
__global__ __launch_bounds__(256) void ortho_scale_kernel(int n, const double *__restrict__ G, int ldg,
                                                          double *__restrict__ colsq) {
  __shared__ double red[4];
  const int j = blockIdx.x;
  const double sj = 1.0 / sqrt(G[(size_t)j + (size_t)j * ldg]);
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    if (i == j) continue;
    const double g = G[(size_t)i + (size_t)j * ldg] * sj / sqrt(G[(size_t)i + (size_t)i * ldg]);
    s += g * g;
  }
  s = wg_sum(s, red);
  if (threadIdx.x == 0) colsq[j] = s;
}

// ipr[j] = sum v^4 / (sum v * sv)^2
__global__ __launch_bounds__(256) void ipr_kernel(int m, const double *__restrict__ V, int ldv,
                                                  const double *__restrict__ SV, int ldsv,
                                                  double *__restrict__ ipr) {
  __shared__ double red[4];
  const double *v = V + (size_t)blockIdx.x * ldv, *sv = SV + (size_t)blockIdx.x * ldsv;
  double p4 = 0.0, p2 = 0.0;
  for (int i = threadIdx.x; i < m; i += 256) {
    const double x = v[i], x2 = x * x;
    p4 += x2 * x2; p2 += x * sv[i];
  }
  p4 = wg_sum(p4, red);
  p2 = wg_sum(p2, red);
  if (threadIdx.x == 0) ipr[blockIdx.x] = p4 / (p2 * p2);
}

// ipr[j] = sum_i v_ij^4 / (sum_i x_ij y_ij)^2: the metric of DSYGV's types 2 (X = Z, Y = B Z) and 3 (X = Y = L^-1 Z)
__global__ __launch_bounds__(256) void ipr_metric_kernel(int m, const double *__restrict__ V, int ldv,
                                                         const double *__restrict__ X, int ldx,
                                                         const double *__restrict__ Y, int ldy,
                                                         double *__restrict__ ipr) {
  __shared__ double red[4];
  const double *v = V + (size_t)blockIdx.x * ldv, *x = X + (size_t)blockIdx.x * ldx, *y = Y + (size_t)blockIdx.x * ldy;
  double p4 = 0.0, p2 = 0.0;
  for (int i = threadIdx.x; i < m; i += 256) {
    const double z = v[i], z2 = z * z;
    p4 += z2 * z2; p2 += x[i] * y[i];
  }
  p4 = wg_sum(p4, red);
  p2 = wg_sum(p2, red);
  if (threadIdx.x == 0) ipr[blockIdx.x] = p4 / (p2 * p2);
}

// Types 2 and 3: rho_j = sqrt(rsq[j]) / (||A||_F ||B||_F sqrt(zsq[j])), j < nc, with ||A||_F^2 = sum asq[0..n), ||B||_F^2 =
// sum bsq[0..n).  out[0] = ||A||_F ||B||_F, out[1] = sum_j rho_j / nc, out[2] = max_j rho_j (a NaN is kept)
__global__ __launch_bounds__(256) void finish_sygv_kernel(int nc, const double *__restrict__ rsq,
                                                          const double *__restrict__ zsq, int n,
                                                          const double *__restrict__ asq,
                                                          const double *__restrict__ bsq, double *out) {
  __shared__ double red[4];
  __shared__ double mx[256];
  double a = 0.0, b = 0.0;
  for (int j = threadIdx.x; j < n; j += 256) { a += asq[j]; b += bsq[j]; }
  a = wg_sum(a, red);
  b = wg_sum(b, red);
  const double nrm = sqrt(a) * sqrt(b);
  double s = 0.0, m = 0.0;
  for (int j = threadIdx.x; j < nc; j += 256) {
    const double rho = sqrt(rsq[j]) / (nrm * sqrt(zsq[j]));
    s += rho;
    m = (rho > m || rho != rho) ? rho : m;
  }
  s = wg_sum(s, red);
  mx[threadIdx.x] = m;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      const double y = mx[threadIdx.x + o], x = mx[threadIdx.x];
      mx[threadIdx.x] = (y > x || y != y) ? y : x;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { out[0] = nrm; out[1] = s / (double)nc; out[2] = mx[0]; }
}

// out[3] and the IPRs of a B whose factorisation failed (*d_info != 0): NaN
__global__ void sygv_not_spd_kernel(const int *__restrict__ d_info, int nc, double *out, double *ipr) {
  if (*d_info == 0) return;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j == 0) out[3] = __builtin_nan("");
  if (j < nc) ipr[j] = __builtin_nan("");
}

inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

// ---- the check from the triplets (sparse_check below)
// out[b] = the sum of the squares of block b's slice of the CSR values; the slices are cut by the entry count alone
__global__ __launch_bounds__(256) void csr_sumsq_kernel(long long nnz, long long per_block, const double *__restrict__ val,
                                                        double *__restrict__ out) {
  __shared__ double red[4];
  const long long k0 = (long long)blockIdx.x * per_block, k1 = k0 + per_block < nnz ? k0 + per_block : nnz;
  double s = 0.0;
  for (long long k = k0 + threadIdx.x; k < k1; k += 256) s += val[k] * val[k];
  s = wg_sum(s, red);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// One pass over the rows for the columns j < ncu of Z, held transposed (Zt(j, c) = z(c, j), ld ldt, a multiple of 64): a
// lane owns a column, a wave a chunk of `rows` consecutive rows.  Per row i: a = sum_c A(i,c) z(c,j) and s = sum_c B(i,c)
// z(c,j) (GEN; else s = z(i,j)), both in ascending c by this one lane; St(j, i) = s (GEN); the lane's running sum takes
// (a - w_j s)^2 for j < n_check.  part(j, chunk) receives the running sum: sparse_colsq_kernel adds the chunks in order.
// The CSR arrays are read at wave-uniform addresses; every load of z(c, .) is one line of 64 doubles.
// The pass runs as two launches so that the host can sort A's triplets while the device already works on what needs B
// alone -- mode kPassS: s and St for the columns j < ncu (A is not looked at); mode kPassRes: a and the running sums for the
// columns j < n_check, s read back from St (GEN) or z.
enum { kPassS = 1, kPassRes = 2 };
template <bool GEN>
__global__ __launch_bounds__(256) void sparse_residual_kernel(
    int mode, int n, int ncu, int n_check, int ldt, int rows, const long long *__restrict__ rpA,
    const int *__restrict__ ciA, const double *__restrict__ vA, const long long *__restrict__ rpB,
    const int *__restrict__ ciB, const double *__restrict__ vB, const double *__restrict__ w,
    const double *__restrict__ Zt, double *__restrict__ St, double *__restrict__ part) {
  const int j = blockIdx.x * 64 + (threadIdx.x & 63);
  const int chunk = blockIdx.y * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int r0 = chunk * rows;
  const bool do_s = GEN && mode == kPassS, do_res = mode == kPassRes;
  if (r0 >= n || j >= (do_s ? ncu : n_check)) return;
  const int r1 = r0 + rows < n ? r0 + rows : n;
  const bool res = do_res && j < n_check;
  const double wj = res ? w[j] : 0.0;
  const double *z = Zt + j;
  double acc = 0.0;
  for (int i = r0; i < r1; ++i) {
    double a = 0.0, sv;
    if (do_res) {
      const long long k1 = rpA[i + 1];
#pragma unroll 4
      for (long long k = rpA[i]; k < k1; ++k) a += vA[k] * z[(size_t)ciA[k] * ldt];
    }
    if (do_s) {
      sv = 0.0;
      const long long k1 = rpB[i + 1];
#pragma unroll 4
      for (long long k = rpB[i]; k < k1; ++k) sv += vB[k] * z[(size_t)ciB[k] * ldt];
      St[(size_t)i * ldt + j] = sv;
    } else {
      sv = GEN ? St[(size_t)i * ldt + j] : z[(size_t)i * ldt];
    }
    if (res) { const double r = a - wj * sv; acc += r * r; }
  }
  if (do_res) part[(size_t)chunk * ldt + j] = acc;
}

// colsq[j] = the chunks' sums of column j, in ascending chunk order
__global__ void sparse_colsq_kernel(int n_check, int chunks, int ldt, const double *__restrict__ part,
                                    double *__restrict__ colsq) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_check) return;
  double s = 0.0;
  for (int c = 0; c < chunks; ++c) s += part[(size_t)c * ldt + j];
  colsq[j] = s;
}

constexpr int kCsrSumBlocks = 512;

}  // namespace

// rows of a wave's chunk in sparse_residual_kernel: at most 128 chunks, so that the partial sums stay a sliver of Z
static inline int sparse_chunk_rows(int n) { const int r = ceil_div(n, 128); return r > 8 ? r : 8; }

SparseCheckLayout::SparseCheckLayout(int problem, int n, int n_check, int n_orth, int hi_orth, int n_ipr) {
  ncu = n_check;
  if (problem == 1) { if (hi_orth > ncu) ncu = hi_orth; if (n_ipr > ncu) ncu = n_ipr; }
  ldt = round_up(ncu > 0 ? ncu : 1, 64);
  rows = sparse_chunk_rows(n);
  chunks = ceil_div(n > 0 ? n : 1, rows);
  size_t o = 0;
  auto take = [&](size_t doubles) { const size_t at = o; o += al256(doubles * 8); return at; };
  Zt = take(ncu > 0 ? (size_t)ldt * n : 0);
  St = take(problem == 1 && ncu > 0 ? (size_t)ldt * n : 0);
  S = take(problem == 1 ? (size_t)n * ncu : 0);
  G = take((size_t)n_orth * n_orth);
  part = take(ncu > 0 ? (size_t)chunks * ldt : 0);
  vec = take((size_t)(n_check > n_orth ? n_check : n_orth) + kCsrSumBlocks + 8);
  total = o;
}

size_t sparse_check_work_bytes(int problem, int n, int n_check, int n_orth, int hi_orth, int n_ipr) {
  return SparseCheckLayout(problem, n, n_check, n_orth, hi_orth, n_ipr).total;
}

// d_out (device, 8 doubles): [0] sum_j ||r_j||, [1] max_j ||r_j||, [2] ||A||_F over the first n_check columns (n_check > 0);
// [6] the orthogonality of the columns c0 .. c0 + n_orth - 1 (n_orth > 0); d_ipr (device): n_ipr ratios (n_ipr > 0).
// B is looked at for problem 1 only.  The products with A and B are sparse; G = V^T S, the scaling of G, the finish and the
// IPR are the calls and kernels of orthogonality() and ipratios() above -- for problem 0 with their very operands.
static void sparse_check_metric_tail(hipStream_t s, bool gen, int n, const double *Z, int ldz, const double *S, double *G,
                                     double *colsq, int c0, int n_orth, int n_ipr, double *d_out, double *d_ipr);

// phases: kSparseMetric: what needs B alone (S, the orthogonality, the IPRs); kSparseResidual: what needs A (to be
// launched after the other, on the same stream; the caller uploads A's CSR in between); both: one after the other.
void sparse_check(hipStream_t s, int phases, int problem, int n, const DevCsr &A, const DevCsr &B, const double *w,
                  const double *Z, int ldz, int n_check, int c0, int n_orth, int n_ipr, double *d_out, double *d_ipr,
                  void *work) {
  const SparseCheckLayout lay(problem, n, n_check, n_orth, c0 + n_orth, n_ipr);
  char *p = (char *)work;
  double *Zt = (double *)(p + lay.Zt), *St = (double *)(p + lay.St), *S = (double *)(p + lay.S);
  double *G = (double *)(p + lay.G), *part = (double *)(p + lay.part), *colsq = (double *)(p + lay.vec);
  double *asq = colsq + (n_check > n_orth ? n_check : n_orth);
  const bool gen = problem == 1, metric = (phases & kSparseMetric) != 0, residual = (phases & kSparseResidual) != 0;
  const dim3 grid(lay.ldt / 64, ceil_div(lay.chunks, 4));
  // Z^T belongs to whichever phase first reads it: the metric's for problem 1, the residual's for problem 0
  if (lay.ncu > 0 && (gen ? metric : residual)) transpose_rows(s, lay.ncu, n, Z, ldz, 0, Zt, lay.ldt);
  if (gen && metric && lay.ncu > 0) {
    hipLaunchKernelGGL(sparse_residual_kernel<true>, grid, dim3(256), 0, s, kPassS, n, lay.ncu, n_check, lay.ldt, lay.rows,
                       nullptr, nullptr, nullptr, B.rowptr, B.col, B.val, w, Zt, St, part);
    transpose_rows(s, n, lay.ncu, St, lay.ldt, 0, S, n);
  }
  if (metric) sparse_check_metric_tail(s, gen, n, Z, ldz, S, G, colsq, c0, n_orth, n_ipr, d_out, d_ipr);
  if (residual && n_check > 0) {
    const dim3 rgrid(ceil_div(n_check, 64), grid.y);
    if (gen)
      hipLaunchKernelGGL(sparse_residual_kernel<true>, rgrid, dim3(256), 0, s, kPassRes, n, lay.ncu, n_check, lay.ldt,
                         lay.rows, A.rowptr, A.col, A.val, B.rowptr, B.col, B.val, w, Zt, St, part);
    if (!gen)
      hipLaunchKernelGGL(sparse_residual_kernel<false>, rgrid, dim3(256), 0, s, kPassRes, n, lay.ncu, n_check, lay.ldt,
                         lay.rows, A.rowptr, A.col, A.val, nullptr, nullptr, nullptr, w, Zt, St, part);
    hipLaunchKernelGGL(sparse_colsq_kernel, dim3(ceil_div(n_check, 256)), dim3(256), 0, s, n_check, lay.chunks, lay.ldt,
                       part, colsq);
    const long long per = (A.nnz + kCsrSumBlocks - 1) / kCsrSumBlocks > 1024 ? (A.nnz + kCsrSumBlocks - 1) / kCsrSumBlocks : 1024;
    const int nb = A.nnz > 0 ? (int)((A.nnz + per - 1) / per) : 1;
    hipLaunchKernelGGL(csr_sumsq_kernel, dim3(nb), dim3(256), 0, s, A.nnz, per, A.val, asq);
    hipLaunchKernelGGL(finish_residual_kernel, dim3(1), dim3(256), 0, s, n_check, colsq, nb, asq, d_out);
  }
}

// G = V^T S (problem 0: V^T V), its scaling and finish, and the IPRs: the calls and kernels of orthogonality() and ipratios()
static void sparse_check_metric_tail(hipStream_t s, bool gen, int n, const double *Z, int ldz, const double *S, double *G,
                                     double *colsq, int c0, int n_orth, int n_ipr, double *d_out, double *d_ipr) {
  if (n_orth > 0) {
    const double *Vs = Z + (size_t)c0 * ldz;
    if (gen) gemm(s, true, false, n_orth, n_orth, n, 1.0, Vs, ldz, S + (size_t)c0 * n, n, 0.0, G, n_orth);
    else gemm(s, true, false, n_orth, n_orth, n, 1.0, Vs, ldz, Vs, ldz, 0.0, G, n_orth);
    hipLaunchKernelGGL(ortho_scale_kernel, dim3(n_orth), dim3(256), 0, s, n_orth, G, n_orth, colsq);
    hipLaunchKernelGGL(finish_residual_kernel, dim3(1), dim3(256), 0, s, 0, colsq, n_orth, colsq, d_out + 4);
  }
  if (n_ipr > 0) {
    if (gen) hipLaunchKernelGGL(ipr_kernel, dim3(n_ipr), dim3(256), 0, s, n, Z, ldz, S, n, d_ipr);
    else hipLaunchKernelGGL(ipr_kernel, dim3(n_ipr), dim3(256), 0, s, n, Z, ldz, Z, ldz, d_ipr);
  }
}

size_t verify_work_bytes(int n, int ncols) {
  const size_t nn = (size_t)n * (n > 0 ? n : 1), nc = (size_t)n * (ncols > 0 ? ncols : 1);
  return 2 * al256(nn * 8) + 2 * al256(nc * 8) + al256((size_t)(ncols > n ? ncols : n) * (size_t)(ncols > 0 ? ncols : 1) * 8) +
         4 * al256((size_t)(n + ncols + 8) * 8);
}

// d_result (device, 3 doubles): sum_j ||r_j||, max_j ||r_j||, ||A||_F
void residual_norms(hipStream_t s, int n, int n_check, const double *A, int lda, const double *B, int ldb,
                    const double *w, const double *V, int ldv, double *d_result, void *work) {
  char *p = (char *)work;
  const size_t nn = (size_t)n * n;
  double *As = (double *)p; p += al256(nn * 8);
  double *Bs = (double *)p; p += al256(nn * 8);
  double *R = (double *)p; p += al256((size_t)n * n_check * 8);
  p += al256((size_t)n * n_check * 8);
  p += al256((size_t)(n_check > n ? n_check : n) * n_check * 8);
  double *colsq = (double *)p; p += al256((size_t)(n + n_check + 8) * 8);
  double *asq = (double *)p;
  // 'L' semantics of PDSYMM: only the lower triangles of A and B are referenced
  copy_matrix(s, n, n, A, lda, As, n);
  symmetrize_lower(s, n, As, n);
  if (B) {
    copy_matrix(s, n, n, B, ldb, Bs, n);
    symmetrize_lower(s, n, Bs, n);
    gemm(s, false, false, n, n_check, n, 1.0, Bs, n, V, ldv, 0.0, R, n);   // Residual <- B V  (:142)
  } else {
    copy_matrix(s, n, n_check, V, ldv, R, n);                               // Residual <- V    (:151)
  }
  hipLaunchKernelGGL(scale_cols_kernel, dim3(ceil_div(n, 256), n_check < 1024 ? n_check : 1024), dim3(256), 0, s,
                     n, n_check, R, n, w);                                  // * -lambda_j      (:160)
  gemm(s, false, false, n, n_check, n, 1.0, As, n, V, ldv, 1.0, R, n);      // += A V           (:169)
  hipLaunchKernelGGL(col_sumsq_kernel, dim3(n_check), dim3(256), 0, s, n, R, n, colsq);
  hipLaunchKernelGGL(col_sumsq_kernel, dim3(n), dim3(256), 0, s, n, As, n, asq);
  hipLaunchKernelGGL(finish_residual_kernel, dim3(1), dim3(256), 0, s, n_check, colsq, n, asq, d_result);
}

// d_result[0] = || scaled (V^T B V) with zero diagonal ||_F for columns [c0, c0+nc)
void orthogonality(hipStream_t s, int n, int c0, int nc, const double *B, int ldb, const double *V, int ldv,
                   double *d_result, void *work) {
  char *p = (char *)work;
  const size_t nn = (size_t)n * n;
  p += al256(nn * 8);
  double *Bs = (double *)p; p += al256(nn * 8);
  p += al256((size_t)n * nc * 8);
  double *BV = (double *)p; p += al256((size_t)n * nc * 8);
  double *G = (double *)p; p += al256((size_t)(nc > n ? nc : n) * nc * 8);
  double *colsq = (double *)p; p += al256((size_t)(n + nc + 8) * 8);
  double *zero = (double *)p;
  const double *Vs = V + (size_t)c0 * ldv;
  if (B) {
    copy_matrix(s, n, n, B, ldb, Bs, n);
    symmetrize_lower(s, n, Bs, n);
    gemm(s, false, false, n, nc, n, 1.0, Bs, n, Vs, ldv, 0.0, BV, n);       // BV <- B V        (:279)
    gemm(s, true, false, nc, nc, n, 1.0, Vs, ldv, BV, n, 0.0, G, nc);       // V^T BV           (:289)
  } else {
    gemm(s, true, false, nc, nc, n, 1.0, Vs, ldv, Vs, ldv, 0.0, G, nc);     // V^T V            (:299)
  }
  hipLaunchKernelGGL(ortho_scale_kernel, dim3(nc), dim3(256), 0, s, nc, G, nc, colsq);
  (void)hipMemsetAsync(zero, 0, 8, s);
  // reuse finish: result[2] = sqrt(sum colsq) -> Frobenius norm
  hipLaunchKernelGGL(finish_residual_kernel, dim3(1), dim3(256), 0, s, 0, colsq, nc, colsq, d_result);
}

void ipratios(hipStream_t s, int n, int n_vec, const double *B, int ldb, const double *V, int ldv,
              double *d_ipr, void *work) {
  char *p = (char *)work;
  const size_t nn = (size_t)n * n;
  p += al256(nn * 8);
  double *Bs = (double *)p; p += al256(nn * 8);
  double *SV = (double *)p;
  if (B) {
    copy_matrix(s, n, n, B, ldb, Bs, n);
    symmetrize_lower(s, n, Bs, n);
    gemm(s, false, false, n, n_vec, n, 1.0, Bs, n, V, ldv, 0.0, SV, n);     // SV <- S V (distribute_matrix.f90:47)
    hipLaunchKernelGGL(ipr_kernel, dim3(n_vec), dim3(256), 0, s, n, V, ldv, SV, n, d_ipr);
  } else {
    hipLaunchKernelGGL(ipr_kernel, dim3(n_vec), dim3(256), 0, s, n, V, ldv, V, ldv, d_ipr);
  }
}

// ---- DSYGV's types 2 and 3 for one problem of any order (ek_hip_check_sygvx*), the first nc columns of Z
struct SygvCheckLayout {
  size_t As, Bs, T1, T2, G, L, inv, twork, vec, total;
  int ld;
  SygvCheckLayout(int itype, int n, int nc) {
    const size_t nn = (size_t)n * n, nz = (size_t)n * nc;
    ld = round_up(n, kDiagNB);                      // the factor's leading dimension, as the Cholesky entries pad it
    size_t o = 0;
    auto take = [&](size_t doubles) { const size_t at = o; o += al256(doubles * 8); return at; };
    As = take(nn); Bs = take(nn); T1 = take(nz); T2 = take(nz); G = take((size_t)nc * nc);
    vec = take(4 * (size_t)n + 2 * (size_t)nc + 8);
    L = inv = twork = o;
    if (itype == 3) {
      L = take((size_t)ld * n);
      inv = take((size_t)ceil_div(n, kDiagNB) * kDiagNB * kDiagNB);
      twork = take((size_t)256 * (ld > nc ? ld : nc));
    }
    total = o;
  }
};

size_t sygv_check_work_bytes(int itype, int n, int ncols) { return SygvCheckLayout(itype, n, ncols).total; }

// d_out (device, 4 doubles): ||A||_F ||B||_F, res_ave, res_max, orthogonality; d_ipr (device, nc doubles); *d_info (device
// int): type 3's factorisation of a copy of B, 0 or the failing pivot -- then d_out[3] and d_ipr are NaN
void sygv_check(hipStream_t s, int itype, int n, int nc, const double *A, int lda, const double *B, int ldb,
                const double *w, const double *Z, int ldz, double *d_out, double *d_ipr, int *d_info, void *work) {
  const SygvCheckLayout lay(itype, n, nc);
  char *p = (char *)work;
  double *As = (double *)(p + lay.As), *Bs = (double *)(p + lay.Bs), *T1 = (double *)(p + lay.T1);
  double *T2 = (double *)(p + lay.T2), *G = (double *)(p + lay.G), *vec = (double *)(p + lay.vec);
  double *asq = vec, *bsq = vec + n, *rsq = vec + 2 * (size_t)n, *zsq = rsq + nc, *gsq = zsq + nc;
  copy_matrix(s, n, n, A, lda, As, n);
  symmetrize_lower(s, n, As, n);
  copy_matrix(s, n, n, B, ldb, Bs, n);
  symmetrize_lower(s, n, Bs, n);
  // T1 = S = B Z (type 2), U = A Z (type 3); T2 = R = -Z diag(w) + A S (type 2), + B U (type 3)
  gemm(s, false, false, n, nc, n, 1.0, itype == 2 ? Bs : As, n, Z, ldz, 0.0, T1, n);
  copy_matrix(s, n, nc, Z, ldz, T2, n);
  hipLaunchKernelGGL(scale_cols_kernel, dim3(ceil_div(n, 256), nc < 1024 ? nc : 1024), dim3(256), 0, s, n, nc, T2, n, w);
  gemm(s, false, false, n, nc, n, 1.0, itype == 2 ? As : Bs, n, T1, n, 1.0, T2, n);
  hipLaunchKernelGGL(col_sumsq_kernel, dim3(nc), dim3(256), 0, s, n, T2, n, rsq);
  hipLaunchKernelGGL(col_sumsq_kernel, dim3(nc), dim3(256), 0, s, n, Z, ldz, zsq);
  hipLaunchKernelGGL(col_sumsq_kernel, dim3(n), dim3(256), 0, s, n, As, n, asq);
  hipLaunchKernelGGL(col_sumsq_kernel, dim3(n), dim3(256), 0, s, n, Bs, n, bsq);
  hipLaunchKernelGGL(finish_sygv_kernel, dim3(1), dim3(256), 0, s, nc, rsq, zsq, n, asq, bsq, d_out);
  (void)hipMemsetAsync(d_info, 0, sizeof(int), s);
  if (itype == 2) {                                 // G = Z^T (B Z)
    gemm(s, true, false, nc, nc, n, 1.0, Z, ldz, T1, n, 0.0, G, nc);
    hipLaunchKernelGGL(ipr_metric_kernel, dim3(nc), dim3(256), 0, s, n, Z, ldz, Z, ldz, T1, n, d_ipr);
  } else {                                          // W = L^-1 Z over U, G = W^T W
    double *L = (double *)(p + lay.L), *inv = (double *)(p + lay.inv), *tw = (double *)(p + lay.twork);
    copy_matrix(s, n, n, B, ldb, L, lay.ld);
    potrf_lower(s, n, L, lay.ld, inv, d_info, tw);
    copy_matrix(s, n, nc, Z, ldz, T1, n);
    trsm_lln(s, n, nc, L, lay.ld, inv, T1, n, tw);
    gemm(s, true, false, nc, nc, n, 1.0, T1, n, T1, n, 0.0, G, nc);
    hipLaunchKernelGGL(ipr_metric_kernel, dim3(nc), dim3(256), 0, s, n, Z, ldz, T1, n, T1, n, d_ipr);
  }
  hipLaunchKernelGGL(ortho_scale_kernel, dim3(nc), dim3(256), 0, s, nc, G, nc, gsq);
  hipLaunchKernelGGL(finish_residual_kernel, dim3(1), dim3(256), 0, s, 0, gsq, nc, gsq, T2);   // T2[2] = ||.||_F
  (void)hipMemcpyAsync(d_out + 3, T2 + 2, 8, hipMemcpyDeviceToDevice, s);
  hipLaunchKernelGGL(sygv_not_spd_kernel, dim3(ceil_div(nc, 256)), dim3(256), 0, s, d_info, nc, d_out, d_ipr);
}

}  // namespace ek
