// ek_api_internal.h -- what the translation units behind the C-ABI of libek_hip.so share (not installed):
//   ek_api.hip    boundary: context, memory, the stage-level entries (one per ScaLAPACK call), acceptance checks
//   ek_comm.hip   the communicator that stands where the reference has its BLACS context: RCCL (bound at run time),
//                 the host-hook exchange, the team's agreements
//   ek_solve.hip  the whole-path driver (the Path behind solve_device_locked), its plan, the device and window entries
//   ek_solve_host.hip  the entries on host arrays (ek_hip_solve, ..._replicated, ...) and their staging pipeline
//   ek_debug.hip  tuning / profiling / rehearsal hooks of include/ek_hip_debug.h and the *_team entries
#pragma once
#include "../../include/ek_hip.h"
#include "../../include/ek_hip_debug.h"
#include "ek_common.h"
#include "ek_switch.h"

#include <rccl/rccl.h>   // types only: the library is bound at run time (dlopen), see ek_comm.hip

#include <chrono>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

namespace ek {
namespace batched {
// The variable-order entries' problem table (ek_batched.hip builds it, its kernel and ek_batched_x.hip's read it): one
// entry per problem of order > 0, a class after the other, descending order inside a class; `index` is the problem's
// place in the caller's batch, where its status word goes.
struct Desc {
  double *A, *B, *w, *Z;
  int n, lda, ldb, ldz, index, pad;
};
static_assert(sizeof(Desc) == 56, "the table's entry");
// ek_hip_*_window_xvbatched*: an entry of the second table, beside the Desc of the same index: the problem's window, the
// vectors its LU slot holds, and where that slot starts in its class's region of the LU workspace (in doubles: the
// prefix sum of 5 n wcols inside its launch)
struct WDesc {
  double vl, vu;
  int il, iu, zcap, wcols;
  long long lu;
};
static_assert(sizeof(WDesc) == 40, "the window table's entry");
}  // namespace batched

namespace api {

struct Context {
  bool ready = false;
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;   // look-ahead work (panel chain of the Cholesky factorisation)
  // cached device workspace (grown on demand, never shrunk until finalize)
  void *ws = nullptr;         // what the stages use (may sit inside a larger allocation, see place_workspace)
  void *ws_alloc = nullptr;   // what hipFree gets
  size_t ws_bytes = 0;
  int *d_info = nullptr;
  double *d_status = nullptr;   // one word for the team's status agreements (comm_agree)
  double *d_stats = nullptr;    // [8] counters of the last whole-path solve ([0] flops the D&C merge products executed)
  double stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};
extern Context g_ctx;
extern std::mutex g_mu;

int ensure_init();
int workspace(size_t bytes, void **p);

// simple bump allocator over the cached workspace, 256-byte aligned pieces
struct Arena {
  char *base; size_t off = 0, cap;
  Arena(void *p, size_t c) : base((char *)p), cap(c) {}
  template <typename T> T *get(size_t count) {
    size_t bytes = (count * sizeof(T) + 255) & ~(size_t)255;
    T *r = (T *)(base + off);
    off += bytes;
    return r;
  }
};
inline size_t al(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

void release_scratch_choice();
int user_images(size_t bytes, void **p);   // device images of host arrays, kept between calls (ek_api.hip)
void release_user_images();
void release_pipe_streams();       // the staging pipeline's copy streams (ek_solve_host.hip)
void release_batched();            // the batched entries' per-problem status words (ek_batched.hip)
void release_xbatched();           // the images of ek_hip_eigenpairs_xbatched* (ek_batched_x.hip)
// orders above EK_HIP_BATCH_NMAX: the chunks' launches on s, status words to dinfo (device); g_mu held
// (itype as DSYGV's, looked at when problem == 1)
int xbatched_launch(hipStream_t s, int problem, int itype, int jobz, int n, int batch, double *dA, int lda,
                    long long strideA, double *dB, int ldb, long long strideB, double *dw, double *dZ, int ldz,
                    long long strideZ, int *dinfo);
// ek_hip_*_ybatched*, orders above EK_HIP_XBATCH_NMAX: the same arguments, the class of 512 rows and its chunks of 256
int ybatched_launch(hipStream_t s, int problem, int itype, int jobz, int n, int batch, double *dA, int lda,
                    long long strideA, double *dB, int ldb, long long strideB, double *dw, double *dZ, int ldz,
                    long long strideZ, int *dinfo);
// the same for `count` entries of the variable-order table (device), all of order above EK_HIP_BATCH_NMAX: chunk c
// takes the entries [c K, c K + K) and the image slots 0 .. K-1; the status word of an entry goes to dinfo[index]
int xvbatched_prepare(int count);  // its images (min(count, K) slots), to be called before the call's first event
int xvbatched_launch(hipStream_t s, int problem, int itype, int jobz, int count, const batched::Desc *table,
                     int *dinfo);
// ek_hip_eigenpairs_window_xbatched* above EK_HIP_BATCH_NMAX: the images of `slots` workgroups (before the call's first
// event), then one chunk of count <= slots problems on s.  The pointers are the chunk's; dm, dinfo: a word per problem of
// it; lu: a slot of 5 n wcols doubles per workgroup (jobz = 1).  The host driver (counts, chunks, LU slots) is
// ek_batched.hip's
int xwindow_prepare(int slots);
int xwindow_launch(hipStream_t s, int problem, int itype, int jobz, int n, int count, double *dA, int lda,
                   long long strideA, double *dB, int ldb, long long strideB, double *dw, double *dZ, int ldz,
                   long long strideZ, int *dinfo, int range, int il, int iu, int zcap, double vl, double vu, int *dm,
                   double *lu, int wcols);
// ek_hip_*_window_xvbatched*: one launch of count <= slots entries of the variable-order table and of the window table
// beside it (device), all of order above EK_HIP_BATCH_NMAX; dinfo, dm: a word per problem of the caller's batch; lu: the
// class's region of the LU workspace.  xwindow_prepare(slots) done
int xvwindow_launch(hipStream_t s, int problem, int itype, int jobz, int range, int count, const batched::Desc *table,
                    const batched::WDesc *wtable, int *dinfo, int *dm, double *lu);
void release_batched_check();     // every batched check's scratch, output words, table and events (ek_batched_check.hip)
void *choose_sytrd_scratch(int n, int ld, double *wA, void *arena_work, double *vecs, size_t need);

// device buffers of one host-array call: released on every exit path
struct DevMem {
  std::vector<void *> ptrs;
  ~DevMem() { for (void *p : ptrs) (void)hipFree(p); }
  int alloc(double **p, size_t bytes) {
    EK_HIP_CHECK(hipMalloc((void **)p, bytes > 0 ? bytes : 8));
    ptrs.push_back(*p);
    return 0;
  }
};

int check_desc(const int *desc, int argpos, int m, int n, int lld_rows = -1);
int numroc0(int n, int nb, int me, int np);
// Owner cell of a process grid for the replicated-input mode (ek_hip_solve_replicated)
struct GridCell { int nb, nprow, npcol, myrow, mycol; };

// Exchange hook for block-cyclically distributed inputs (ek_hip_set_allgatherv)
extern ek_hip_allgatherv_fn g_allgatherv;
extern void *g_allgatherv_user;

int pad_ld(int n);
int h2d_matrix(int m, int n, const double *h, int ldh, double *d, int ldd, hipStream_t s);
int d2h_matrix(int m, int n, const double *d, int ldd, double *h, int ldh, hipStream_t s);
int fetch_info(int *info);
// test aids: NaN into the strips a member does not own; entries in which two arrays differ (bitwise)
void poison_foreign_strips(hipStream_t s, int n, double *A, int lda, int P, int rank);
void count_mismatch(hipStream_t s, int m, int n, const double *X, int ldx, const double *Y, int ldy, int lower,
                    unsigned long long *count);

// ---- communicator (ek_comm.hip)
struct Comm {
  bool on = false;
  bool host = false;    // exchanges go through the host's allgatherv hook instead of RCCL
  ncclComm_t comm = nullptr;
  int nranks = 0, rank = 0;
  int err = 0;          // first failing collective since the last check (ncclResult_t)
};
extern Comm g_comm;
constexpr int kPotrfRlMin = 1024;
extern int g_two_stage_min;
int two_stage_min();
int dist_min_ranks();
void comm_teardown();     // the communicator itself (ek_hip_finalize)
SytrdExchange team_exchange(int nteam, int n = 0);
// Pairwise exchange over the attached communicator (RCCL: grouped ncclSend / ncclRecv; host communicator: two rounds of
// the allgatherv hook): this rank sends send[i] (send_counts[i] doubles, device) to world rank peers[i] and receives
// recv_counts[i] doubles from it into recv[i]; stream-ordered, collective over the communicator (a rank with no peer
// calls it with npeers = 0).  Failures are recorded in g_comm.err like those of every other exchange.
void team_sendrecv(hipStream_t s, int npeers, const int *peers, double *const *send, const size_t *send_counts,
                   double *const *recv, const size_t *recv_counts);
int comm_any(int local);
int comm_agree(int local_rc);
const char *comm_error_string();

// ---- whole path (ek_solve.hip)
void gather_band_strips(hipStream_t s, int n, int nmem, int rank0, double *const *ABs, const SytrdExchange &x);

// the library's return code for a runtime error (0 for hipSuccess); EK_TRY passes a stage's nonzero code on
inline int hip_rc(hipError_t e) { return e == hipSuccess ? 0 : -1000 - (int)e; }
#define EK_TRY(call) do { const int rc_ = (call); if (rc_) return rc_; } while (0)

// a window of the spectrum (ek_hip_eigenvalues*, ek_hip_eigenpairs*, ek_hip_sygvx*): see the Path of ek_solve.hip
struct Window {
  int jobz, range, il, iu;
  double vl, vu;
  int zcap;
  int m, first;            // out
};
constexpr int kWindowTooSmall = -990;

// One call of the whole path on device arrays (column-major, any ld >= n); callers fill in the fields they use.
struct HostPipe;
struct PathCall {
  int problem = 0, itype = 1, n = 0, n_vec = 0;
  double *dA = nullptr; int lda = 0;
  double *dB = nullptr; int ldb = 0;
  double *dw = nullptr, *dZ = nullptr; int ldz = 0;
  double *stage_seconds = nullptr; int n_stages = 0;
  const GridCell *cell = nullptr;       // a grid cell's share of the eigenvectors
  HostPipe *pipe = nullptr;             // the host path's staging pipeline
  Window *win = nullptr;
};
// the arguments of ek_hip_solve_device, in its order, as a request (cell, pipe, win and itype are the caller's to add)
inline PathCall path_call(int problem, int n, int n_vec, double *dA, int lda, double *dB, int ldb, double *dw, double *dZ,
                          int ldz, double *stage_seconds, int n_stages) {
  PathCall c;
  c.problem = problem; c.n = n; c.n_vec = n_vec;
  c.dA = dA; c.lda = lda; c.dB = dB; c.ldb = ldb; c.dw = dw; c.dZ = dZ; c.ldz = ldz;
  c.stage_seconds = stage_seconds; c.n_stages = n_stages;
  return c;
}
int solve_device_locked(const PathCall &call);      // g_mu held
// arguments 1 .. 9 of ek_hip_solve_device, ..._device_grid and ..._replicated, and of ek_hip_eigenvalues*, in order (LAPACK -k)
int solve_args(int problem, int n, int n_vec, const void *A, int lda, const void *B, int ldb, const void *w, const void *Z);
int eigenvalues_args(int problem, int n, int il, int iu, const void *A, int lda, const void *B, int ldb, const void *w);
// both entries of ek_hip_eigenvalues* under the lock (the arrays are the device's)
int eigenvalues_locked(int problem, int n, int il, int iu, double *dA, int lda, double *dB, int ldb, double *dw,
                       double *stage_seconds, int n_stages);
// the argument checks of ek_hip_eigenpairs* / ek_hip_sygvx* in argument order, and both entries under the lock
int eigenpairs_args(int problem, int jobz, int range, int n, double vl, double vu, int il, int iu, const void *A, int lda,
                    const void *B, int ldb, const int *m, const int *ifirst, const void *w, const void *Z, int ldz,
                    int zcap);
int eigenpairs_locked(int problem, int jobz, int range, int n, double vl, double vu, int il, int iu, double *dA, int lda,
                      double *dB, int ldb, int *m, int *ifirst, double *dw, double *dZ, int ldz, int zcap,
                      double *stage_seconds, int n_stages, int itype);

// ---- triplet inputs (ek_sparse.hip); sparse::Csr is the host form of ek_sparse_csr.h
}  // namespace api
namespace sparse { struct Csr; }
namespace api {
// (nnz, suffix, value) at argument positions pos, pos + 1, pos + 2: -position of the first offender (a negative count; a
// NULL suffix or an index outside 1 .. n; a NULL value), or 0
int triplet_args(int n, long long nnz, const int *suf, const double *val, int pos);
// the host CSRs of A and, with_b, of B (built side by side on two threads) in storage the library keeps between calls:
// g_mu held; valid until the next call; never throws
int csr_build(int n, long long nnzA, const int *sufA, const double *valA, const sparse::Csr **hA, bool with_b,
              long long nnzB, const int *sufB, const double *valB, const sparse::Csr **hB);
void release_sparse_host();                          // that storage (ek_hip_finalize)
size_t csr_device_bytes(int n, long long nnz);       // device bytes of a CSR, bounded by the list: 2 nnz entries
// the CSR into dst (csr_device_bytes(n, nnz_list) bytes of device memory) on stream s; h must outlive the stream's work
int csr_upload(hipStream_t s, const sparse::Csr &h, long long nnz_list, void *dst, DevCsr *d);

// ---- host entries and their staging pipeline (ek_solve_host.hip); what the Path asks of a pipeline:
int pipe_wait_in(HostPipe *p, int tag);           // B (tag 0) or A (1) is in HBM; the pipeline's error, if any
int pipe_z_slab(const HostPipe *p);               // columns of Z per slab on the way out
// what stream s has made final leaves for the host: the lower triangle of A ('A') or L ('B') from the caller's device
// array dev (ldd), or columns c0 .. c0 + nc - 1 of Z ('Z')
void pipe_out(HostPipe *p, hipStream_t s, char which, double *dev, int ldd, int n, int c0, int nc);

}  // namespace api
}  // namespace ek
