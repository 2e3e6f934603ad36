// ek_sparse.hip -- the reference's own matrix arguments (ek_sparse_mat_t: replicated 1-based triplets) at the C-ABI:
// the CSR of the mirrored matrix is built on the host (ek_sparse_csr.h), uploaded, and either densified in HBM for the
// Path (ek_hip_solve_sparse in ek_solve_host.hip, ek_hip_sparse_to_dense here) or multiplied as it is by the check
// (ek_hip_check_sparse*; kernels in ek_verify.hip).  No dense matrix but Z exists on the host.  DESIGN.md 27.
#include "ek_api_internal.h"
#include "ek_sparse_csr.h"

#include <new>
#include <system_error>
#include <thread>

using namespace ek;
using namespace ek::api;

namespace ek {
namespace {
// column `row` of M from row `row` of the CSR (the matrix is symmetric): a wave per row, lanes along its entries, whose
// ascending columns are ascending addresses.  Every (row, col) occurs once in the CSR: no two lanes share an address.
__global__ __launch_bounds__(256) void densify_kernel(int n, const long long *__restrict__ rowptr,
                                                      const int *__restrict__ col, const double *__restrict__ val,
                                                      double *__restrict__ M, int ld) {
  const int row = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (row >= n) return;
  const long long k1 = rowptr[row + 1];
  for (long long k = rowptr[row] + (threadIdx.x & 63); k < k1; k += 64) M[(size_t)col[k] + (size_t)row * ld] = val[k];
}
}  // namespace

void sparse_densify(hipStream_t s, int n, const DevCsr &m, double *M, int ld) {
  if (n <= 0) return;
  if (ld == n) (void)hipMemsetAsync(M, 0, (size_t)n * n * 8, s);
  else (void)hipMemset2DAsync(M, (size_t)ld * 8, 0, (size_t)n * 8, n, s);
  if (m.nnz > 0) hipLaunchKernelGGL(densify_kernel, dim3(ceil_div(n, 4)), dim3(256), 0, s, n, m.rowptr, m.col, m.val, M, ld);
}

namespace api {
int triplet_args(int n, long long nnz, const int *suf, const double *val, int pos) {
  if (nnz < 0) return -pos;
  if (nnz > 0 && !suf) return -(pos + 1);
  if (nnz > 0 && sparse::first_bad_index(n, nnz, suf)) return -(pos + 1);
  if (nnz > 0 && !val) return -(pos + 2);
  return 0;
}

// the device arrays of a CSR are sized by the list (at most two entries per triplet), not by what survives
size_t csr_device_bytes(int n, long long nnz) {
  const size_t m = 2 * (size_t)(nnz > 0 ? nnz : 0);
  return al(((size_t)n + 1) * 8) + al(m * 4) + al(m * 8);
}

namespace {
// the host CSRs of A (0) and B (1) and the arrays of their sorts keep their pages between calls (g_mu held by every user;
// ek_hip_finalize releases them): a fresh 10 MB of vectors per call cost more in page faults than the sort itself
struct HostCsr { sparse::Csr csr; sparse::Scratch scratch; void *pinned = nullptr; size_t pinned_bytes = 0; };
HostCsr g_host_csr[2];

int build_one(int which, int n, long long nnz, const int *suf, const double *val) {
  try {
    return sparse::build_csr(n, nnz, suf, val, g_host_csr[which].csr, &g_host_csr[which].scratch) ? -1 : 0;
  } catch (const std::bad_alloc &) {        // (nothing may be thrown across the C ABI)
    return hip_rc(hipErrorOutOfMemory);
  }
}
}  // namespace

int csr_build(int n, long long nnzA, const int *sufA, const double *valA, const sparse::Csr **hA, bool with_b,
              long long nnzB, const int *sufB, const double *valB, const sparse::Csr **hB) {
  int rb = 0;
  std::thread side;
  if (with_b) {
    try {
      side = std::thread([&]() { rb = build_one(1, n, nnzB, sufB, valB); });
    } catch (const std::system_error &) {   // no second thread to be had: one after the other
    }
  }
  const int ra = build_one(0, n, nnzA, sufA, valA);
  if (side.joinable()) side.join();
  else if (with_b) rb = build_one(1, n, nnzB, sufB, valB);
  *hA = &g_host_csr[0].csr;
  if (hB) *hB = &g_host_csr[1].csr;
  return ra ? ra : rb;
}

void release_sparse_host() {
  for (HostCsr &h : g_host_csr) {
    if (h.pinned) (void)hipHostFree(h.pinned);
    h = HostCsr();
  }
}

// One of the two kept host CSRs goes through its pinned image of the device layout: one copy that the stream really
// takes asynchronously (three copies from pageable vectors each wait for the runtime's own staging).  Any other CSR, or
// no pinned memory to be had: the three copies; h then stays alive until the stream has been waited for.
int csr_upload(hipStream_t s, const sparse::Csr &h, long long nnz_list, void *dst, DevCsr *d) {
  const size_t m = 2 * (size_t)(nnz_list > 0 ? nnz_list : 0), have = (size_t)h.nnz();
  const size_t o_ci = al(((size_t)h.n + 1) * 8), o_v = o_ci + al(m * 4);
  char *p = (char *)dst;
  long long *rp = (long long *)p;
  int *ci = (int *)(p + o_ci);
  double *v = (double *)(p + o_v);
  *d = DevCsr{rp, ci, v, (long long)have};
  for (HostCsr &k : g_host_csr) {
    if (&k.csr != &h) continue;
    const size_t bytes = o_v + have * 8;
    if (k.pinned_bytes < bytes) {
      if (k.pinned) (void)hipHostFree(k.pinned);
      k.pinned = nullptr; k.pinned_bytes = 0;
      if (hipHostMalloc(&k.pinned, bytes, hipHostMallocDefault) != hipSuccess) { k.pinned = nullptr; (void)hipGetLastError(); break; }
      k.pinned_bytes = bytes;
    }
    char *q = (char *)k.pinned;
    memcpy(q, h.rowptr.data(), ((size_t)h.n + 1) * 8);
    if (have) { memcpy(q + o_ci, h.col.data(), have * 4); memcpy(q + o_v, h.val.data(), have * 8); }
    EK_HIP_CHECK(hipMemcpyAsync(dst, q, bytes, hipMemcpyHostToDevice, s));
    return 0;
  }
  EK_HIP_CHECK(hipMemcpyAsync(rp, h.rowptr.data(), ((size_t)h.n + 1) * 8, hipMemcpyHostToDevice, s));
  if (have) {
    EK_HIP_CHECK(hipMemcpyAsync(ci, h.col.data(), have * 4, hipMemcpyHostToDevice, s));
    EK_HIP_CHECK(hipMemcpyAsync(v, h.val.data(), have * 8, hipMemcpyHostToDevice, s));
  }
  return 0;
}
}  // namespace api
}  // namespace ek

namespace {
// what a check call does, from its counts: the residual part, the orthogonality part, the IPR part
struct Parts {
  bool res, orth, ipr;
  int c0, n_orth;
  Parts(int n_check, int index1, int index2, int n_ipr, const double *ipr_host)
      : res(n_check > 0), orth(index2 >= index1), ipr(n_ipr > 0 && ipr_host != nullptr), c0(orth ? index1 - 1 : 0),
        n_orth(orth ? index2 - index1 + 1 : 0) {}
  bool any() const { return res || orth || ipr; }
};

// arguments of ek_hip_check_sparse* in argument order; n == 0 is decided by the callers
int check_sparse_args(int problem, int n, long long nnzA, const int *sufA, const double *valA, long long nnzB,
                      const int *sufB, const double *valB, const void *w, const void *Z, int ldz, int n_check, int index1,
                      int index2, int n_ipr, const double *out, const double *ipr_host) {
  int rc = triplet_args(n, nnzA, sufA, valA, 3); if (rc) return rc;
  if (problem == 1) { rc = triplet_args(n, nnzB, sufB, valB, 6); if (rc) return rc; }
  const Parts p(n_check, index1, index2, n_ipr, ipr_host);
  if (p.res && !w) return -9;
  if (p.any() && !Z) return -10;
  if (ldz < (n > 1 ? n : 1)) return -11;
  if (n_check < 0 || n_check > n) return -12;
  if (p.orth && index1 < 1) return -13;
  if (p.orth && index2 > n) return -14;
  if (n_ipr < 0 || n_ipr > n) return -15;
  if ((p.res || p.orth) && !out) return -16;
  return 0;
}
}  // namespace

extern "C" {

int ek_hip_check_sparse_device(int problem, int n, long long nnzA, const int *sufA, const double *valA, long long nnzB,
                               const int *sufB, const double *valB, const double *dw, const double *dZ, int ldz,
                               int n_check, int index1, int index2, int n_ipr, double out[4], double *ipr_host) {
  if (problem != 0 && problem != 1) return -1;
  if (n < 0) return -2;
  if (n == 0) return 0;
  int rc = check_sparse_args(problem, n, nnzA, sufA, valA, nnzB, sufB, valB, dw, dZ, ldz, n_check, index1, index2, n_ipr,
                             out, ipr_host);
  if (rc) return rc;
  const Parts p(n_check, index1, index2, n_ipr, ipr_host);
  if (!p.any()) return 0;
  if (!p.ipr) n_ipr = 0;
  rc = ensure_init(); if (rc) return rc;
  std::lock_guard<std::mutex> lk(g_mu);
  hipStream_t s = g_ctx.stream;
  const bool gen = problem == 1;
  // A is read by the residual part alone, and that part comes last: A's triplets are sorted on a second thread (or, where
  // none is to be had, by this one after the launches below) while this thread sorts B's and the device works on what
  // needs B alone -- S, the GEMM, the IPRs.  A's CSR then travels on the second stream, behind no kernel.
  int ra = 0;
  bool a_built = !p.res;
  std::thread side;
  struct Join { std::thread &t; ~Join() { if (t.joinable()) t.join(); } } join{side};
  if (p.res) {
    try {
      side = std::thread([&]() { ra = build_one(0, n, nnzA, sufA, valA); });
      a_built = true;
    } catch (const std::system_error &) {
    }
  }
  if (gen) EK_TRY(build_one(1, n, nnzB, sufB, valB));
  const size_t ba = csr_device_bytes(n, nnzA), bb = gen ? csr_device_bytes(n, nnzB) : 0;
  const size_t wb = sparse_check_work_bytes(problem, n, n_check, p.n_orth, p.c0 + p.n_orth, n_ipr);
  void *ws;
  rc = workspace(ba + bb + wb + al((size_t)(n_ipr + 8) * 8), &ws); if (rc) return rc;
  char *base = (char *)ws, *work = base + ba + bb;
  DevCsr dA{}, dB{};
  if (gen) EK_TRY(csr_upload(s, g_host_csr[1].csr, nnzB, base + ba, &dB));
  double *d_out = (double *)(work + wb), *d_ipr = d_out + 8;
  sparse_check(s, kSparseMetric, problem, n, dA, dB, dw, dZ, ldz, n_check, p.c0, p.n_orth, n_ipr, d_out, d_ipr, work);
  EK_HIP_CHECK(hipGetLastError());
  if (p.res) {
    if (!a_built) ra = build_one(0, n, nnzA, sufA, valA);
    if (side.joinable()) side.join();
    EK_TRY(ra);
    hipStream_t s2 = g_ctx.stream2 ? g_ctx.stream2 : s;
    EK_TRY(csr_upload(s2, g_host_csr[0].csr, nnzA, base, &dA));
    if (s2 != s) {
      hipEvent_t up = nullptr;
      EK_HIP_CHECK(hipEventCreateWithFlags(&up, hipEventDisableTiming));
      hipError_t e = hipEventRecord(up, s2);
      if (e == hipSuccess) e = hipStreamWaitEvent(s, up, 0);
      (void)hipEventDestroy(up);                 // (released once the work recorded so far is done)
      EK_HIP_CHECK(e);
    }
    sparse_check(s, kSparseResidual, problem, n, dA, dB, dw, dZ, ldz, n_check, p.c0, p.n_orth, n_ipr, d_out, d_ipr, work);
  }
  EK_HIP_CHECK(hipGetLastError());
  double r[8] = {0};
  EK_HIP_CHECK(hipMemcpyAsync(r, d_out, sizeof(r), hipMemcpyDeviceToHost, s));
  if (p.ipr) EK_HIP_CHECK(hipMemcpyAsync(ipr_host, d_ipr, (size_t)n_ipr * 8, hipMemcpyDeviceToHost, s));
  EK_HIP_CHECK(hipStreamSynchronize(s));
  if (p.res) {                                   // the normalisations of ek_hip_residual_device (verifier.f90:198-199)
    out[0] = r[2];
    out[1] = r[0] / r[2] / (double)n_check;
    out[2] = r[1] / r[2];
  }
  if (p.orth) out[3] = r[6];
  return 0;
}

int ek_hip_check_sparse(int problem, int n, long long nnzA, const int *sufA, const double *valA, long long nnzB,
                        const int *sufB, const double *valB, const double *w, const double *Z, int ldz, int n_check,
                        int index1, int index2, int n_ipr, double out[4], double *ipr_host) {
  if (problem != 0 && problem != 1) return -1;
  if (n < 0) return -2;
  if (n == 0) return 0;
  int rc = check_sparse_args(problem, n, nnzA, sufA, valA, nnzB, sufB, valB, w, Z, ldz, n_check, index1, index2, n_ipr, out,
                             ipr_host);
  if (rc) return rc;
  const Parts p(n_check, index1, index2, n_ipr, ipr_host);
  if (!p.any()) return 0;
  rc = ensure_init(); if (rc) return rc;
  int ncols = p.res ? n_check : 0;               // the columns of Z a part reads
  if (p.orth && index2 > ncols) ncols = index2;
  if (p.ipr && n_ipr > ncols) ncols = n_ipr;
  double *uZ = nullptr, *uw = nullptr;
  DevMem mem;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    hipStream_t s = g_ctx.stream;
    rc = mem.alloc(&uZ, (size_t)n * ncols * 8); if (rc) return rc;
    rc = mem.alloc(&uw, (size_t)(n_check > 0 ? n_check : 1) * 8); if (rc) return rc;
    rc = h2d_matrix(n, ncols, Z, ldz, uZ, n, s); if (rc) return rc;
    if (p.res) EK_HIP_CHECK(hipMemcpyAsync(uw, w, (size_t)n_check * 8, hipMemcpyHostToDevice, s));
    EK_HIP_CHECK(hipStreamSynchronize(s));
  }
  return ek_hip_check_sparse_device(problem, n, nnzA, sufA, valA, nnzB, sufB, valB, uw, uZ, n, n_check, index1, index2,
                                    n_ipr, out, ipr_host);
}

int ek_hip_sparse_to_dense(int n, long long nnz, const int *suf, const double *val, double *M, int ldm) {
  if (n < 0) return -1;
  if (n == 0) return 0;
  int rc = triplet_args(n, nnz, suf, val, 2); if (rc) return rc;
  if (!M) return -5;
  if (ldm < n) return -6;
  rc = ensure_init(); if (rc) return rc;
  std::lock_guard<std::mutex> lk(g_mu);
  hipStream_t s = g_ctx.stream;
  const sparse::Csr *h = nullptr;
  EK_TRY(csr_build(n, nnz, suf, val, &h, false, 0, nullptr, nullptr, nullptr));
  const size_t nn = al((size_t)n * n * 8);
  void *ws;
  rc = workspace(nn + csr_device_bytes(n, nnz), &ws); if (rc) return rc;
  DevCsr d{};
  EK_TRY(csr_upload(s, *h, nnz, (char *)ws + nn, &d));
  sparse_densify(s, n, d, (double *)ws, n);
  EK_HIP_CHECK(hipGetLastError());
  EK_TRY(d2h_matrix(n, n, (const double *)ws, n, M, ldm, s));
  EK_HIP_CHECK(hipStreamSynchronize(s));
  return 0;
}

// host arithmetic only: the canonical form itself, for tests and tools
long long ek_hip_debug_sparse_csr(int n, long long nnz, const int *suf, const double *val, long long *rowptr, int *col,
                                  double *csr_val) {
  if (n < 0) return -1;
  const int rc = triplet_args(n, nnz, suf, val, 2); if (rc) return rc;
  if (!rowptr) return -5;
  if (nnz > 0 && !col) return -6;
  if (nnz > 0 && !csr_val) return -7;
  std::lock_guard<std::mutex> lk(g_mu);
  const sparse::Csr *h = nullptr;
  const int rb = csr_build(n, nnz, suf, val, &h, false, 0, nullptr, nullptr, nullptr); if (rb) return rb;
  const size_t m = (size_t)h->nnz();
  memcpy(rowptr, h->rowptr.data(), ((size_t)n + 1) * 8);
  if (m) { memcpy(col, h->col.data(), m * 4); memcpy(csr_val, h->val.data(), m * 8); }
  return (long long)m;
}

unsigned long long ek_hip_debug_sparse_check_workspace_bytes(int problem, int n, long long nnzA, long long nnzB,
                                                             int n_check, int index1, int index2, int n_ipr) {
  if ((problem != 0 && problem != 1) || n <= 0 || nnzA < 0 || (problem == 1 && nnzB < 0)) return 0;
  if (n_check < 0 || n_check > n || n_ipr < 0 || n_ipr > n) return 0;
  if (index2 >= index1 && (index1 < 1 || index2 > n)) return 0;
  const int n_orth = index2 >= index1 ? index2 - index1 + 1 : 0, hi = n_orth ? index2 : 0;
  if (n_check == 0 && n_orth == 0 && n_ipr == 0) return 0;
  return csr_device_bytes(n, nnzA) + (problem == 1 ? csr_device_bytes(n, nnzB) : 0) +
         sparse_check_work_bytes(problem, n, n_check, n_orth, hi, n_ipr) + al((size_t)(n_ipr + 8) * 8);
}

}  // extern "C"
