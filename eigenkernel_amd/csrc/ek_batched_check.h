// ek_batched_check.h -- what the translation units of the batched acceptance checks share (not installed):
//   ek_batched_check.hip       the entries up to EK_HIP_BATCH_NMAX, the kernel of the standard problem and of type 1, and
//                              the host side of every uniform-order entry: the argument checker, the device
//                              pool with its one release function, the run function, the stager of host arrays; the
//                              driver of every variable-order entry, ek_hip_check_*xvbatched* included:
//                              four classes (256, 128, 64, 32) from one table, the class of 256 in chunks
//   ek_batched_check_sygv.hip  the kernel of DSYGV's types 2 and 3
//   ek_batched_check_x.h       the checks on the matrix cores: loaders, step, products, passes and the two kernel bodies
//                              (DESIGN.md 38), instantiated by four units that each hold their uniform Args, their
//                              launches and their entries and hand the host driver a launch function:
//     ek_batched_check_x.hip, ek_batched_check_sygv_x.hip  the full checks above EK_HIP_BATCH_NMAX, and the launches of
//                              their table form for the variable driver (launch_x, launch_sygv_x)
//     ek_batched_check_window.hip, ek_batched_check_sygv_window.hip  the window checks (m[b] columns per problem, every
//                              order up to EK_HIP_XBATCH_NMAX), and the launches of their table form
//                              (launch_window_v, launch_sygv_window_v) for ek_hip_check_*window_xvbatched* (DESIGN.md
//                              37), whose driver and entries are ek_batched_check.hip's
// The kernels are instantiated in units of their own so that a unit's code generation does not depend on what else is
// compiled beside it.
#pragma once
#include "ek_batched_stages.h"

#include <cmath>

namespace ek {
namespace bcheck {

struct Args {
  int problem, n;
  const double *A; int lda; long long sA;
  const double *B; int ldb; long long sB;
  const double *w;
  const double *Z; int ldz; long long sZ;
  const int *map;       // the problems to check, one per workgroup; nullptr: workgroup b takes problem b
  double *S;            // problem 1: n^2 doubles per problem
  double *out;          // EK_HIP_CHECK_NOUT doubles per problem
  double *ipr;          // n doubles per problem, or nullptr
};

// the variable form's table: one entry per problem to check, a class after the other, descending order inside a class.
// S: the entry's own scratch -- n^2 doubles per problem in the classes up to 128; in the class of 256 a slot of the
// entry's chunk (n^2 doubles, 2 n^2 for type 3), reused by the next chunk.  m: the columns to check in the variable window
// form, whose S is a slot of n m doubles (type 3: n^2 more) of the entry's chunk; 0 and unread elsewhere
struct Desc {
  const double *A, *B, *w, *Z;
  double *S, *ipr;
  int n, lda, ldb, ldz, index, m;
};
struct VArgs {
  int problem;
  const Desc *table;
  double *out;
};

// global address space, the solver's own types: a pointer loaded from the table would otherwise cost flat accesses
using bstages::gdouble;
using bstages::cgdouble;
// What a workgroup works on.  c: the columns of Z to check -- n in the kernels up to EK_HIP_BATCH_NMAX; the window kernels
// take it (the table's m), the full kernels above EK_HIP_BATCH_NMAX take n and leave it unread (ek_batched_check_x.h)
struct Problem {
  int n, c;
  cgdouble *A; int lda;
  cgdouble *B; int ldb;
  cgdouble *w;
  cgdouble *Z; int ldz;
  gdouble *S, *out, *ipr;
};
// One locate per argument form.  The kernels of ek_batched_check_x.h call locate(a, kind) with the problem or the type: the
// uniform Args of their units, each with a locate of its own beside it, size the scratch by it; the table does not need it
__device__ __forceinline__ Problem locate(const Args &a) {
  const long long pb = a.map ? a.map[blockIdx.x] : (int)blockIdx.x;
  return {a.n, a.n, (cgdouble *)(a.A + pb * a.sA), a.lda, a.problem ? (cgdouble *)(a.B + pb * a.sB) : nullptr, a.ldb,
          (cgdouble *)(a.w + pb * a.n), (cgdouble *)(a.Z + pb * a.sZ), a.ldz,
          a.problem ? (gdouble *)(a.S + pb * a.n * a.n) : nullptr, (gdouble *)(a.out + pb * EK_HIP_CHECK_NOUT),
          a.ipr ? (gdouble *)(a.ipr + pb * a.n) : nullptr};
}
// the table form: entry blockIdx.x of the launch's slice of the table
__device__ __forceinline__ Problem locate(const VArgs &a, int /* kind */ = 0) {
  const Desc &d = a.table[blockIdx.x];
  return {d.n, d.m, (cgdouble *)d.A, d.lda, (cgdouble *)d.B, d.ldb, (cgdouble *)d.w, (cgdouble *)d.Z, d.ldz,
          (gdouble *)d.S, (gdouble *)(a.out + (long long)d.index * EK_HIP_CHECK_NOUT), (gdouble *)d.ipr};
}

// Sum (or maximum) over the workgroup, the same bits in every thread: a butterfly inside the wave, then the waves in
// ascending order.  The maximum keeps a NaN (fmax would drop it): a problem with a NaN residual reports NaN.
template <int NW, bool MAX>
__device__ __forceinline__ double wg_reduce(double x, double *red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double y = __shfl_xor(x, o, 64);
    x = MAX ? ((y > x || y != y) ? y : x) : x + y;
  }
  if (NW == 1) return x;
  __syncthreads();                                  // the previous call's readers are through
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int w = 1; w < NW; ++w) {
    const double y = red[w];
    s = MAX ? ((y > s || y != y) ? y : s) : s + y;
  }
  return s;
}

// sum_{k < n} x[k] y[k] in ascending order, x and y in LDS: four elements' loads go out before the first use.  Every
// multiply-add of this file is written as fma(): the instantiations must round alike, whatever the compiler contracts
__device__ __forceinline__ double lds_dot(const double *x, const double *y, int n) {
  double acc = 0.0;
  int k = 0;
  for (; k + 4 <= n; k += 4) {
    const double x0 = x[k], x1 = x[k + 1], x2 = x[k + 2], x3 = x[k + 3];
    const double y0 = y[k], y1 = y[k + 1], y2 = y[k + 2], y3 = y[k + 3];
    acc = fma(x0, y0, acc); acc = fma(x1, y1, acc); acc = fma(x2, y2, acc); acc = fma(x3, y3, acc);
  }
  for (; k < n; ++k) acc = fma(x[k], y[k], acc);
  return acc;
}
// the same for two vectors against one y (a row of A and a row of B against a column of Z)
__device__ __forceinline__ void lds_dot2(const double *xa, const double *xb, const double *y, int n, double &da,
                                         double &db) {
  double a = 0.0, b = 0.0;
  int k = 0;
  for (; k + 4 <= n; k += 4) {
    const double y0 = y[k], y1 = y[k + 1], y2 = y[k + 2], y3 = y[k + 3];
    const double a0 = xa[k], a1 = xa[k + 1], a2 = xa[k + 2], a3 = xa[k + 3];
    const double b0 = xb[k], b1 = xb[k + 1], b2 = xb[k + 2], b3 = xb[k + 3];
    a = fma(a0, y0, a); b = fma(b0, y0, b); a = fma(a1, y1, a); b = fma(b1, y1, b);
    a = fma(a2, y2, a); b = fma(b2, y2, b); a = fma(a3, y3, a); b = fma(b3, y3, b);
  }
  for (; k < n; ++k) { a = fma(xa[k], y[k], a); b = fma(xb[k], y[k], b); }
  da = a; db = b;
}

// LDS doubles of a class: the image, 2 buffers x 2 rows of A and of B, 1 / sqrt(G_jj), a word per wave for the sums
// over the workgroup.  At 64 that is 37 920 B: four workgroups share a CU's 160 KiB
constexpr int lds_doubles(int NC) { return NC * (NC + 1) + 8 * NC + NC + 4; }

// one launch of the kernel of types 2 and 3 (itype) for `count` problems of class nc (32, 64, 128)
int launch_sygv(hipStream_t s, int itype, int nc, int count, const Args &a);
int launch_sygv(hipStream_t s, int itype, int nc, int count, const VArgs &a);
// one launch of the kernels above EK_HIP_BATCH_NMAX for `count` entries of the table, each of such an order:
// ek_batched_check_x.hip's (the standard problem and type 1, a.problem says which), ek_batched_check_sygv_x.hip's (itype 2, 3)
int launch_x(hipStream_t s, int count, const VArgs &a);
int launch_sygv_x(hipStream_t s, int itype, int count, const VArgs &a);
// one launch of the window kernels' table form for `count` entries of the table, each with 1 <= m <= n:
// ek_batched_check_window.hip's (a.problem says which), ek_batched_check_sygv_window.hip's (itype 2, 3)
int launch_window_v(hipStream_t s, int count, const VArgs &a);
int launch_sygv_window_v(hipStream_t s, int itype, int count, const VArgs &a);

// ---- the host driver of the uniform-order entries (ek_batched_check.hip)
// One call.  itype: 0 the standard problem and type 1 (`problem` says which), 2 or 3 those types (problem = 1).  A, B, w
// and Z are host or device arrays as the entry says, device arrays when a UniformLaunch sees them; the rest is host
struct Uniform {
  int itype, problem, n, batch;
  const double *A; int lda; long long sA;
  const double *B; int ldb; long long sB;
  const double *w;
  const double *Z; int ldz; long long sZ;
  const int *info;
  double *out, *ipr, *seconds;
};
// A unit's own part of a call: its Args and one launch of its kernel for the entries first .. first + count - 1 of the map
// (nullptr: those problems), with the pool's scratch S and output words dout, dipr (nullptr: no IPRs)
typedef int (*UniformLaunch)(hipStream_t s, const Uniform &u, const int *map, int first, int count, double *S, double *dout,
                             double *dipr);
// -1 .. -13, -15 as include/ek_hip.h lists them, n against nmax; *nothing: n == 0 or batch == 0
int uniform_arguments(const Uniform &u, int nmax, bool *nothing);
// the rest of an entry whose arguments are checked: *seconds = 0, the context, g_mu, device copies of host arrays, the
// launches, the fetch and the scatter.  scratch: doubles per problem (chunked = false: one launch, indexed by problem
// number) or per workgroup of a launch (chunked = true: ek_hip_debug_check_xbatched_chunk problems a launch)
int uniform_entry(const Uniform &u, bool nothing, bool host, size_t scratch, bool chunked, UniformLaunch launch);

// ---- the same driver for the window check (ek_batched_check_window.hip): problem b has m[b] values and the
// columns 0 .. m[b]-1 of an n x zcap array; m is a host array.  sygv = false: ek_hip_check_window_xbatched*, u.itype is 0
// and u.problem the caller's; sygv = true: ek_hip_check_sygv_window_xbatched* (ek_batched_check_sygv_window.hip, DESIGN.md
// 36), u.itype is the caller's (1 .. 3, anything else is -1) and u.problem is 1, so that B is required and staged
struct Window {
  Uniform u;
  const int *m;
  int zcap;
  bool sygv;
};
// One launch for the entries first .. first + count - 1 of the map, whose entry e is the pair (problem, m[problem]) in
// map[2 e], map[2 e + 1]; S: sS doubles per workgroup of the launch (problem 1 and type 2: n x the largest checked m;
// type 3: n^2 more for the factor)
typedef int (*WindowLaunch)(hipStream_t s, const Window &w, const int *map, int first, int count, long long sS, double *S,
                            double *dout, double *dipr);
// -1 .. -15, -17 as include/ek_hip.h lists them; *nothing: n == 0 or batch == 0
int window_arguments(const Window &w, int nmax, bool *nothing);
// the rest of the entry: a batch without a problem to check is filled here without the device; otherwise the map by
// descending m, the pool, g_chunk problems a launch, the fetch, and a scatter of m[b] IPRs per row
int window_entry(const Window &w, bool nothing, bool host, WindowLaunch launch);

}  // namespace bcheck
}  // namespace ek
