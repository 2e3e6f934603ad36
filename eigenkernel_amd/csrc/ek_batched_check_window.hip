// ek_batched_check_window.hip -- ek_hip_check_window_xbatched*: the batched acceptance checks for what
// ek_hip_eigenpairs_window_xbatched* returns: per problem the c = m[b] values w[0 .. c) and the columns 0 .. c-1 of an
// n x zcap array, every order 1 .. EK_HIP_XBATCH_NMAX in one kernel class.  This unit holds its uniform Args,
// the launches and the entries; the kernel is xcheck::check_kernel<GEN, true, .> of ek_batched_check_x.h, which describes
// its passes; the argument checker, the device pool, the chunk loop, the fetch and the scatter are ek_batched_check.hip's
// (bcheck::window_arguments, bcheck::window_entry).
// The kernel has a second instantiation per problem kind that finds order, c and addresses in the variable form's table
// (bcheck::launch_window_v, behind ek_hip_check_window_xvbatched*: DESIGN.md 37).
#include "ek_batched_check_x.h"

namespace ek {
namespace wcheck {

using namespace xcheck;

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

// the uniform launch's problem: entry first + workgroup of the map, the scratch by workgroup
__device__ __forceinline__ bcheck::Problem locate(const Args &a, int gen) {
  const int e = a.first + (int)blockIdx.x;          // 1 <= map[2 e + 1] <= n
  return strided(a, a.map[2 * e], a.map[2 * e + 1], gen, a.sS);
}

template <bool GEN, typename ARGS>
static int launch_kernel(hipStream_t s, int count, const ARGS &a) {
  return launch<check_kernel<GEN, true, ARGS>>(s, count, kLdsDoubles, a);
}

// this unit's part of a call (bcheck::window_entry does the rest): the scratch is indexed by workgroup
static int launch_window(hipStream_t s, const bcheck::Window &w, const int *map, int first, int count, long long sS,
                         double *S, double *dout, double *dipr) {
  const bcheck::Uniform &u = w.u;
  Args a{u.problem, u.n, u.A, u.lda, u.sA, u.B, u.ldb, u.sB, u.w, u.Z, u.ldz, u.sZ, map, first, S, sS, dout, dipr};
  return u.problem ? launch_kernel<true>(s, count, a) : launch_kernel<false>(s, count, a);
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
  return a.problem ? wcheck::launch_kernel<true>(s, count, a) : wcheck::launch_kernel<false>(s, count, a);
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
