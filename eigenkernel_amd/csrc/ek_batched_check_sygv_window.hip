// ek_batched_check_sygv_window.hip -- ek_hip_check_sygv_window_xbatched*: the batched acceptance checks of DSYGV's types 2
// (A B x = l x) and 3 (B A x = l x) for what ek_hip_sygv_window_xbatched* and ek_hip_sygv_window_batched* return: per
// problem the c = m[b] values w[0 .. c) and the columns 0 .. c-1 of an n x zcap array, every order 1 .. EK_HIP_XBATCH_NMAX
// in one kernel class.  Type 1 is ek_hip_check_window_xbatched*(problem = 1) itself.  This unit holds its
// uniform Args, the launches and the entries; the kernel is xcheck::check_sygv_kernel<ITYPE, true, .> of
// ek_batched_check_x.h, which describes its passes: every product costs n^2 c, and the scratch is n c (type 2) or
// n^2 + n c (type 3) doubles per workgroup of a launch.  The argument checker, the device pool, the chunk loop, the fetch
// and the scatter are ek_batched_check.hip's (bcheck::window_arguments, bcheck::window_entry).
// Each type's kernel has a second instantiation that finds order, c and addresses in the variable form's table
// (bcheck::launch_sygv_window_v, behind ek_hip_check_sygv_window_xvbatched*: DESIGN.md 37).
#include "ek_batched_check_x.h"

namespace ek {
namespace wcheck_sygv {

using namespace xcheck;

struct Args {
  int n;
  const double *A; int lda; long long sA;
  const double *B; int ldb; long long sB;
  const double *w;
  const double *Z; int ldz; long long sZ;
  const int *map;       // entry e: the pair (problem, m[problem]) in map[2 e], map[2 e + 1]
  int first;            // this launch's first entry of the map
  double *S; long long sS;   // sS doubles per workgroup of a launch: n x (the largest checked m), type 3: n^2 more
  double *out;          // EK_HIP_CHECK_NOUT doubles per problem
  double *ipr;          // n doubles per problem, or nullptr
};

// the uniform launch's problem: entry first + workgroup of the map, the scratch by workgroup
__device__ __forceinline__ bcheck::Problem locate(const Args &a, int) {
  const int e = a.first + (int)blockIdx.x;          // 1 <= map[2 e + 1] <= n
  return strided(a, a.map[2 * e], a.map[2 * e + 1], true, a.sS);
}

template <int ITYPE, typename ARGS>
static int launch_kernel(hipStream_t s, int count, const ARGS &a) {
  return launch<check_sygv_kernel<ITYPE, true, ARGS>>(s, count, kLdsDoublesSygv, a);
}

// this unit's part of a call (bcheck::window_entry does the rest): the scratch is indexed by workgroup
static int launch_window(hipStream_t s, const bcheck::Window &w, const int *map, int first, int count, long long sS,
                         double *S, double *dout, double *dipr) {
  const bcheck::Uniform &u = w.u;
  Args a{u.n, u.A, u.lda, u.sA, u.B, u.ldb, u.sB, u.w, u.Z, u.ldz, u.sZ, map, first, S, sS, dout, dipr};
  return u.itype == 2 ? launch_kernel<2>(s, count, a) : launch_kernel<3>(s, count, a);
}

static int entry(int itype, int n, int batch, const double *A, int lda, long long strideA, const double *B, int ldb,
                 long long strideB, const int *m, const double *w, const double *Z, int ldz, int zcap, long long strideZ,
                 const int *info, double *out, double *ipr, double *seconds, bool host) {
  // the -1 rule is the driver's: itype 1 .. 3 here, with problem = 1 (B is always required)
  const bcheck::Window win{{itype, 1, n, batch, A, lda, strideA, B, ldb, strideB, w, Z, ldz, strideZ, info, out, ipr,
                            seconds}, m, zcap, true};
  bool nothing;
  int rc = bcheck::window_arguments(win, EK_HIP_XBATCH_NMAX, &nothing);
  if (rc) return rc;
  if (itype == 1)                                   // type 1 is problem 1 of the window check itself: the same kernel
    return host ? ek_hip_check_window_xbatched(1, n, batch, A, lda, strideA, B, ldb, strideB, m, w, Z, ldz, zcap, strideZ,
                                               info, out, ipr, seconds)
                : ek_hip_check_window_xbatched_device(1, n, batch, A, lda, strideA, B, ldb, strideB, m, w, Z, ldz, zcap,
                                                      strideZ, info, out, ipr, seconds);
  return bcheck::window_entry(win, nothing, host, launch_window);
}

}  // namespace wcheck_sygv

// the variable form's launch (ek_batched_check.h): `count` entries of the table, itype 2 or 3
int bcheck::launch_sygv_window_v(hipStream_t s, int itype, int count, const VArgs &a) {
  return itype == 2 ? wcheck_sygv::launch_kernel<2>(s, count, a) : wcheck_sygv::launch_kernel<3>(s, count, a);
}

}  // namespace ek

using namespace ek;

extern "C" {

int ek_hip_check_sygv_window_xbatched_device(int itype, int n, int batch, const double *dA, int lda, long long strideA,
                                             const double *dB, int ldb, long long strideB, const int *m, const double *dw,
                                             const double *dZ, int ldz, int zcap, long long strideZ, const int *info,
                                             double *out, double *ipr, double *seconds) {
  return wcheck_sygv::entry(itype, n, batch, dA, lda, strideA, dB, ldb, strideB, m, dw, dZ, ldz, zcap, strideZ, info, out,
                            ipr, seconds, false);
}

int ek_hip_check_sygv_window_xbatched(int itype, int n, int batch, const double *A, int lda, long long strideA,
                                      const double *B, int ldb, long long strideB, const int *m, const double *w,
                                      const double *Z, int ldz, int zcap, long long strideZ, const int *info, double *out,
                                      double *ipr, double *seconds) {
  return wcheck_sygv::entry(itype, n, batch, A, lda, strideA, B, ldb, strideB, m, w, Z, ldz, zcap, strideZ, info, out, ipr,
                            seconds, true);
}

}  // extern "C"
