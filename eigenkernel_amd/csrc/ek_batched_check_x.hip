// ek_batched_check_x.hip -- ek_hip_check_xbatched*: the batched acceptance checks for the orders
// EK_HIP_BATCH_NMAX + 1 .. EK_HIP_XBATCH_NMAX that ek_hip_eigenpairs_xbatched* solves.  Orders up to
// EK_HIP_BATCH_NMAX are forwarded to ek_hip_check_batched*.  This unit holds its uniform Args, the launches and the entries;
// the kernel is xcheck::check_kernel<GEN, false, .> of ek_batched_check_x.h, which describes its passes (c = n here); the
// argument checker, the device pool, the chunk loop, the fetch and the scatter are ek_batched_check.hip's.
// The kernel has a second instantiation per problem kind that finds its problem in the variable form's table
// (bcheck::launch_x, behind ek_hip_check_xvbatched*: DESIGN.md 24).
#include "ek_batched_check_x.h"

namespace ek {
namespace xcheck {

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
__device__ __forceinline__ bcheck::Problem locate(const Args &a, int gen) {
  const long long pb = a.map ? a.map[a.first + (int)blockIdx.x] : a.first + (int)blockIdx.x;
  return strided(a, pb, a.n, gen, (long long)a.n * a.n);
}

template <bool GEN, typename ARGS>
static int launch_kernel(hipStream_t s, int count, const ARGS &a) {
  return launch<check_kernel<GEN, false, ARGS>>(s, count, kLdsDoubles, a);
}

// this unit's part of a call (bcheck::uniform_entry does the rest): the scratch is indexed by workgroup
static int launch_uniform(hipStream_t s, const bcheck::Uniform &u, const int *map, int first, int count, double *S,
                          double *dout, double *dipr) {
  Args a{u.problem, u.n, u.A, u.lda, u.sA, u.B, u.ldb, u.sB, u.w, u.Z, u.ldz, u.sZ, map, first, S, dout, dipr};
  return u.problem ? launch_kernel<true>(s, count, a) : launch_kernel<false>(s, count, a);
}

static int entry(const bcheck::Uniform &u, bool nothing, bool host) {
  return bcheck::uniform_entry(u, nothing, host, u.problem ? (size_t)u.n * u.n : 0, true, launch_uniform);
}

}  // namespace xcheck

// the variable form's launch (ek_batched_check.h): `count` entries of the table, every one of an order above
// EK_HIP_BATCH_NMAX, a.problem says which instantiation
int bcheck::launch_x(hipStream_t s, int count, const VArgs &a) {
  return a.problem ? xcheck::launch_kernel<true>(s, count, a) : xcheck::launch_kernel<false>(s, count, a);
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
