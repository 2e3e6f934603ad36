// ek_batched_check_sygv_x.hip -- ek_hip_check_sygv_xbatched*: the batched acceptance checks of DSYGV's types 2
// (A B x = l x) and 3 (B A x = l x) for the orders EK_HIP_BATCH_NMAX + 1 .. EK_HIP_XBATCH_NMAX that ek_hip_sygv_xbatched*
// solves.  Orders up to EK_HIP_BATCH_NMAX are forwarded to ek_hip_check_sygv_batched*, type 1 above them to
// ek_hip_check_xbatched*(problem = 1).  This unit holds its uniform Args, the launches and the entries; the kernel is
// xcheck::check_sygv_kernel<ITYPE, false, .> of ek_batched_check_x.h, which describes its passes (c = n here: a scratch of
// n^2 doubles for type 2 and 2 n^2 for type 3 per workgroup of a launch, two threads per row of the factor and per column of
// the solve); the argument checker, the device pool, the chunk loop, the fetch and the scatter are ek_batched_check.hip's
// (DESIGN.md 22).  The kernel has a second instantiation per type that finds its problem in the variable form's table
// (bcheck::launch_sygv_x, behind ek_hip_check_sygv_xvbatched*: DESIGN.md 24).
#include "ek_batched_check_x.h"

namespace ek {
namespace xcheck_sygv {

using namespace xcheck;

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

// the uniform launch's problem: entry first + workgroup of the map (or that problem), the scratch by workgroup
__device__ __forceinline__ bcheck::Problem locate(const Args &a, int itype) {
  const long long pb = a.map ? a.map[a.first + (int)blockIdx.x] : a.first + (int)blockIdx.x;
  return strided(a, pb, a.n, true, (long long)(itype - 1) * a.n * a.n);
}

template <int ITYPE, typename ARGS>
static int launch_kernel(hipStream_t s, int count, const ARGS &a) {
  return launch<check_sygv_kernel<ITYPE, false, ARGS>>(s, count, kLdsDoublesSygv, a);
}

// this unit's part of a call (bcheck::uniform_entry does the rest): the scratch is indexed by workgroup
static int launch_uniform(hipStream_t s, const bcheck::Uniform &u, const int *map, int first, int count, double *S,
                          double *dout, double *dipr) {
  Args a{u.itype, u.n, u.A, u.lda, u.sA, u.B, u.ldb, u.sB, u.w, u.Z, u.ldz, u.sZ, map, first, S, dout, dipr};
  return u.itype == 2 ? launch_kernel<2>(s, count, a) : launch_kernel<3>(s, count, a);
}

static int entry(const bcheck::Uniform &u, bool nothing, bool host) {
  return bcheck::uniform_entry(u, nothing, host, (size_t)(u.itype - 1) * u.n * u.n, true, launch_uniform);
}

}  // namespace xcheck_sygv

// the variable form's launch (ek_batched_check.h): `count` entries of the table, every one of an order above
// EK_HIP_BATCH_NMAX, itype 2 or 3
int bcheck::launch_sygv_x(hipStream_t s, int itype, int count, const VArgs &a) {
  return itype == 2 ? xcheck_sygv::launch_kernel<2>(s, count, a) : xcheck_sygv::launch_kernel<3>(s, count, a);
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
