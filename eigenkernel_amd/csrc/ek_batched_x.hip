// ek_batched_x.hip -- ek_hip_eigenpairs_xbatched*: orders EK_HIP_BATCH_NMAX + 1 .. EK_HIP_XBATCH_NMAX of the batched solver.
//
// The six stages of ek_batched.hip, one workgroup per problem from its first load to its last store and no launch between
// the stages -- but the n x n image lies in a device workspace (column-major, leading dimension 257, one slot per workgroup
// of a launch) and not in LDS: 256 x 257 doubles are 514 KiB.  The vectors stay in LDS (d, e, tau, v, w, the partial sums,
// the two staged columns: 9 x 256 doubles).  One class: NC = 256, 512 threads, thread t is (row or column t % 256, half
// t / 256).  Problem 0 and problem 1; problem 1 in DSYGV's three types: A x = l B x (itype 1), A B x = l x
// (2), B A x = l x (3).
// block_reduce, stage 0 (scan_a) and the rank sort that ends stage 4 (rank_sort) are those of ek_batched_stages.h, which
// ek_batched.hip uses too.  The rest is written here with ek_batched.hip's arithmetic rules: eight loads from
// the image ahead of the first store where that file has four, and in stages 1, 2 and 5 another owner for every entry.
//
// Every n^3 loop over the image runs with the lanes of a wave along consecutive rows (consecutive addresses):
//   1  right-looking Cholesky: lane = row; the scaled column of a step is kept in LDS for the update
//   2  X = L^-1 A is kept TRANSPOSED (A is symmetric, so the image of A is its own transpose): the pair t owns column t
//      of X, which is row t of the image.  The upper triangle is then copied to the lower one (X's lower half the right
//      way round) and C = X L^-T runs with the pair t on row t, as in ek_batched.hip.  Both solves are column-oriented
//      (axpy form): every entry sees the same updates in the same order whichever thread applies them, so the two
//      threads of a pair take every other entry; the entry that is the next step's pivot is carried in a register by
//      both (the same instruction on the same operands), and only the half 0 stores it
//   3  DSYTD2 as in ek_batched.hip: lane = row in the symv and in the rank-2 update
//   4  QL: lane = row of Z
//   5  Z is transposed in place, so that the pair t owns column t of Z as row t of the image; the dot of a reflector
//      (and of a row of L^-T) is split between the two threads of a pair -- even and odd offsets, each in ascending
//      order; a reflector's dot is half 0's sum plus half 1's, a row of L^-T gives (z - half 0's sum) - half 1's sum --
//      and the last pass stores Z^T's rows as Z's columns
// Five n^2 passes do have the lanes 257 doubles apart on one side (a cache line per lane): the mirror fill of A's image,
// the copy of X's lower half, the mirror of C, the transpose of Z, and the reads of the last pass.
// Types 2 and 3 have an instantiation of their own (CONG), so that the kernel of the standard problem and of type 1 is the
// code it always was.  Its stages 2 and 5, lane = row in every n^3 loop again:
//   2  C = L^T A L in two passes of one form: Y = A L in place (the pair t owns row t of the full symmetric image;
//      S[t, j] <- sum over k >= j of S[t, k] L[k, j] for ascending j reads columns >= j of its own row, which still hold
//      A), the image transposed in place (a sixth n^2 pass; A is symmetric: Y^T = L^T A), then C = Y^T L by the same pass
//      on the columns 0 .. t of row t, and type 1's mirror.  The two threads of a pair take every other term of a sum;
//      the sum is half 0's part plus half 1's
//   5  type 3: Z <- L Z on the transposed image, column-oriented: for k = n-1 .. 0, z[i] += L[i, k] z[k] for i > k, then
//      z[k] *= L[k, k]; the two threads of a pair take every other entry i.  z[k] is untouched until its own step: both
//      halves load it a step ahead and only the half 0 stores it.  Types 1 and 2 keep Z <- L^-T Z
// Loads from the image are issued eight at a time before the first use: a dependent round trip to L2 / Infinity Cache /
// HBM is paid once per eight entries.  All traffic to the image between threads is ordered by __syncthreads(); plain
// loads and stores, no atomics.  The order of every sum depends on n alone: same bits wherever a problem sits.
//
// A batch runs in chunks of at most K problems (K = 1024; ek_hip_debug_xbatched_chunk), launched one after the other on
// the context's stream without a host synchronise; problem i of a chunk works in slot i of the workspace.
//
// ek_hip_eigenpairs_window_xbatched*: a third argument type, XWArgs, selects stage 4W of ek_batched_window.h in place of
// stage 4's QL; the wanted vectors are rows of the image from the start, and stage 5 works on those rows.
// ek_hip_sygv_window_xbatched*: XWArgs with CONG for types 2 and 3; type 3's Z <- L Z works on those rows too
// (DESIGN.md 33).
//
// ek_hip_*_window_xvbatched*: a fourth argument type, XVWArgs: the table form with a window per problem.
//
// ek_hip_*_xvbatched*: the same kernel for problems of different orders.  A workgroup then finds its problem in entry
// blockIdx.x of its launch's slice of the variable-order table (ek_batched.hip builds it) instead of at blockIdx.x *
// stride; the image slot is blockIdx.x either way.
//
// ek_hip_eigenpairs_ybatched*, ek_hip_sygv_ybatched*: orders EK_HIP_XBATCH_NMAX + 1 .. EK_HIP_YBATCH_NMAX.  A second class
// of the same kernel text, NC = 512, 1024 threads, leading dimension 513: the class is a template parameter (Class below)
// and what is said above about 256, 257 and 512 threads reads 512, 513 and 1024 for it.  One workgroup of 16 waves per
// compute unit, chunks of 256 problems in the same workspace, the Args form alone, CONG false and true.
#include "ek_batched_stages.h"
#include "ek_batched_window.h"

#include <algorithm>
#include <type_traits>

namespace ek {
namespace batchedx {

using namespace bstages;

// A class of this file: NC rows, T threads, the image's leading dimension, threads per row, waves, the doubles of one
// image and the problems of one launch.  The kernel and its helpers take the class as a template parameter and name its
// constants as they always did
template <int NC_, int T_, int CHUNK_>
struct Class {
  static constexpr int NC = NC_, T = T_, LD = NC + 1, P = T / NC, NW = T / 64;
  static constexpr size_t kSlot = (size_t)NC * LD;
  static constexpr int kChunk = CHUNK_;
  static_assert(P == 2, "two threads per row");
};
using ClassX = Class<256, 512, 1024>;               // orders 129 .. 256: 1024 slots are 539 MB
using ClassY = Class<512, 1024, 256>;               // orders 257 .. 512 (ek_hip_*_ybatched*): 256 slots are 538 MB
static_assert(ClassX::NC == EK_HIP_XBATCH_NMAX && ClassY::NC == EK_HIP_YBATCH_NMAX, "the classes' orders");

struct Args {
  int problem, jobz, n;
  double *A; int lda; long long sA;
  double *B; int ldb; long long sB;
  double *w;
  double *Z; int ldz; long long sZ;
  int *info;
  double *ws;
  int itype;                                        // 1 / 2 / 3 as DSYGV's, looked at when problem == 1; last, so that
};                                                  // the fields before it keep their offsets

// The table form: entry blockIdx.x of `table` (this launch's slice), image slot blockIdx.x of ws, status word at
// info[entry.index]
using batched::Desc;
struct XVArgs {
  int problem, jobz;
  const Desc *table;
  int *info;
  double *ws;
  int itype;
};

// ek_hip_eigenpairs_window_xbatched*: Args and the window.  The type is what selects stage 4W (ek_batched_window.h, the
// vectors as rows of the image) in place of stage 4's QL, so the instantiations of Args and XVArgs hold nothing of it
struct XWArgs : Args {
  bwindow::Window win;
};

// ek_hip_eigenpairs_window_xvbatched*: XVArgs and a window per problem -- entry blockIdx.x of `wtable` beside entry
// blockIdx.x of `table`, the count to m[entry.index], the LU slot at lu + wtable[blockIdx.x].lu
struct XVWArgs {
  int problem, jobz;
  const Desc *table;
  const bwindow::WDesc *wtable;
  int *info;
  int *m;
  double *ws;
  double *lu;
  int range, itype;
};

// What a workgroup works on, whichever way it found it.  The pointers are typed as global (gdouble).  n is the same in
// every lane either way (a kernel argument or a load at an address that depends on blockIdx.x alone): every barrier and
// every loop bound depends on it.
struct Problem {
  int n;
  gdouble *A; int lda;
  gdouble *B; int ldb;
  gdouble *w;
  gdouble *Z; int ldz;                              // Z: the table form's; the uniform form leaves it to vectors()
  gdouble *S;
  int *info;
};
template <typename C>
__device__ __forceinline__ Problem locate(const Args &a) {
  const long long pb = blockIdx.x;
  return {a.n, (gdouble *)(a.A + pb * a.sA), a.lda, a.problem ? (gdouble *)(a.B + pb * a.sB) : nullptr, a.ldb,
          (gdouble *)(a.w + pb * a.n), nullptr, a.ldz,
          (gdouble *)(a.ws + (size_t)pb * C::kSlot), a.info + pb};
}
template <typename C>
__device__ __forceinline__ Problem locate(const XVArgs &a) {
  const Desc &d = a.table[blockIdx.x];
  return {d.n, (gdouble *)d.A, d.lda, (gdouble *)d.B, d.ldb, (gdouble *)d.w, (gdouble *)d.Z, d.ldz,
          (gdouble *)(a.ws + (size_t)blockIdx.x * C::kSlot), a.info + d.index};
}
template <typename C>
__device__ __forceinline__ Problem locate(const XVWArgs &a) {
  const Desc &d = a.table[blockIdx.x];
  return {d.n, (gdouble *)d.A, d.lda, (gdouble *)d.B, d.ldb, (gdouble *)d.w, (gdouble *)d.Z, d.ldz,
          (gdouble *)(a.ws + (size_t)blockIdx.x * C::kSlot), a.info + d.index};
}
// the window of stage 4W: the call's, or the workgroup's own
__device__ __forceinline__ const bwindow::Window &window(const XWArgs &a) { return a.win; }
__device__ __forceinline__ bwindow::OwnWindow window(const XVWArgs &a) {
  return bwindow::own_window(a.range, a.wtable[blockIdx.x], a.m + a.table[blockIdx.x].index, a.lu);
}
// Z where the kernel first needs it, behind the exit of jobz = 0 (whose callers pass no Z): the uniform form does its
// address arithmetic only there, as it always did; the table form loaded the pointer with the rest of its entry
__device__ __forceinline__ gdouble *vectors(const Args &a, const Problem &) {
  return (gdouble *)(a.Z + (long long)blockIdx.x * a.sZ);
}
__device__ __forceinline__ gdouble *vectors(const XVArgs &, const Problem &p) { return p.Z; }
__device__ __forceinline__ gdouble *vectors(const XVWArgs &, const Problem &p) { return p.Z; }

// y[i * SY] -= x[i] * a for i = i0, i0 + STEP, ... < i1; y in the image, x in LDS: eight loads before the first store
template <int SY, int STEP>
__device__ __forceinline__ void img_axpy(gdouble *y, const double *x, double a, int i0, int i1) {
  int i = i0;
  for (; i + 7 * STEP < i1; i += 8 * STEP) {
    double yv[8], xv[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) yv[q] = y[(i + q * STEP) * SY];
#pragma unroll
    for (int q = 0; q < 8; ++q) xv[q] = x[i + q * STEP];
#pragma unroll
    for (int q = 0; q < 8; ++q) y[(i + q * STEP) * SY] = yv[q] - xv[q] * a;
  }
  for (; i < i1; i += STEP) y[i * SY] -= x[i] * a;
}

// acc + sum of x[k * SX] * l[k] over k = k0, k0 + STEP, ... < k1, in that order; x in the image, l in LDS
template <int SX, int STEP>
__device__ __forceinline__ double img_dot(const gdouble *x, const double *l, int k0, int k1, double acc) {
  int k = k0;
  for (; k + 7 * STEP < k1; k += 8 * STEP) {
    double xv[8], lv[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) xv[q] = x[(k + q * STEP) * SX];
#pragma unroll
    for (int q = 0; q < 8; ++q) lv[q] = l[k + q * STEP];
#pragma unroll
    for (int q = 0; q < 8; ++q) acc += xv[q] * lv[q];
  }
  for (; k < k1; k += STEP) acc += x[k * SX] * l[k];
  return acc;
}

// One pass of the congruence C = L^T A L (CONG, types 2 and 3): S[r, j] <- sum over k >= j of S[r, k] L[k, j] for
// j = 0 .. n-1 ascending (LOWER: j = 0 .. r), in place: a step reads the columns >= j of its own row and nothing reads
// column j afterwards.  Column j of L comes from B through the two sl vectors, staged a step ahead.  The two threads of a
// pair take every other term, each in ascending order; the sum is half 0's part plus half 1's.  The parts of an even step
// lie in e0 / e1 (half 0's, half 1's), those of an odd step in o0 / o1, so that a step costs one barrier.  Ends behind a
// barrier.
template <typename C, bool LOWER>
__device__ __forceinline__ void cong_pass(gdouble *S, const gdouble *B, int ldb, int n, int t, int r, int sub, bool row,
                                          double *sl, double *e0, double *e1, double *o0, double *o1) {
  constexpr int NC = C::NC, LD = C::LD, P = C::P;
  if (t < n) sl[t] = B[t];                          // column 0 of L
  __syncthreads();
  const int last = LOWER ? r : n - 1;
  for (int j = 0; j < n; ++j) {
    const double *cur = sl + (j & 1) * NC;
    double *p0 = (j & 1) ? o0 : e0, *p1 = (j & 1) ? o1 : e1;
    double nx = 0.0;
    if (j + 1 < n && t > j && t < n) nx = B[t + (size_t)(j + 1) * ldb];
    if (row && j <= last) (sub ? p1 : p0)[r] = img_dot<LD, P>(S + r, cur, j + sub, n, 0.0);
    if (t < n) sl[((j + 1) & 1) * NC + t] = nx;
    __syncthreads();
    if (sub == 0 && row && j <= last) S[r + j * LD] = p0[r] + p1[r];
  }
  __syncthreads();
}

// CONG: the instantiation for types 2 and 3 (C = L^T A L; the host picks it when problem == 1 and itype != 1).  With
// CONG = false nothing of those types is compiled in: the standard problem and type 1 run the code they always ran.
// ARGS: how the workgroup finds its problem -- Args (one order, strided: blockIdx.x * stride) or XVArgs (a table entry);
// XWArgs and XVWArgs are the two with a window.
// WIN (ARGS = XWArgs or XVWArgs): stage 4W for QL, and stage 5 on the window's m rows of the image.
// The table-and-window instantiations are held to four waves a SIMD, that is 128 vector registers and two workgroups on a
// compute unit like the other three argument types: left alone, one of the two came out at 129.  The attribute's value for
// the other types, 2, is what 512 threads imply anyway, and their code is unchanged by it
// C: the class.  ClassY's 1024 threads are four waves a SIMD, which is the attribute's value for it too
template <bool CONG, typename ARGS = Args, typename C = ClassX>
__global__ __launch_bounds__(C::T)
__attribute__((amdgpu_waves_per_eu(std::is_same<ARGS, XVWArgs>::value ? 4 : C::T / 256)))
void xbatched_kernel(ARGS a) {
  constexpr int NC = C::NC, LD = C::LD, P = C::P, NW = C::NW;
  constexpr bool VWIN = std::is_same<ARGS, XVWArgs>::value;
  constexpr bool WIN = VWIN || std::is_same<ARGS, XWArgs>::value;
  __shared__ double sd[NC], se[NC], st[NC];         // d, e, tau: alive from stage 3 to the end
  __shared__ double sv[NC], sw[NC];                 // stage 1: the scaled column; 3: v, w; 4: c, s of a sweep
  __shared__ double sp[P * NC];                     // partial sums of a pair
  __shared__ double sl[2 * NC];                     // a column of L or a reflector, and the next one
  __shared__ double red[2 * NW];
  __shared__ int srank[NC];
  __shared__ int s_state, s_m, s_lo;

  const Problem p = locate<C>(a);
  const int t = threadIdx.x, n = p.n;
  const int r = t % NC, sub = t / NC;
  const bool row = r < n;
  gdouble *A = p.A, *B = p.B, *S = p.S, *W = p.w;
  const int lda = p.lda, ldb = p.ldb;
  int *info = p.info;
  int phase = 0;

  // ---- 0: A finite?  max|a|: the image holds 2^-aex A (scan_a)
  int aex;
  if (!scan_a<NC, NW>(A, lda, n, red, phase, info, aex)) return;

  if (a.problem) {
    // ---- 1: B = L L^T in the image
    if (row)
      for (int j = sub; j <= r; j += P) S[r + j * LD] = B[r + (size_t)j * ldb];
    __syncthreads();
    for (int j = 0; j < n; ++j) {
      const double piv = S[j + j * LD];
      if (!(piv > 1e-290) || !(piv < 1e290)) {
        if (t == 0) *info = j + 1;
        return;
      }
      const double l = sqrt(piv);
      if (sub == 0 && row && r > j) {
        const double lr = S[r + j * LD] / l;
        S[r + j * LD] = lr;
        sv[r] = lr;
      }
      __syncthreads();
      if (row && r > j) img_axpy<LD, P>(S + r, sv, sv[r], j + 1 + sub, r + 1);
      __syncthreads();
    }
    if (row)
      for (int j = sub; j <= r; j += P) B[r + (size_t)j * ldb] = (r == j) ? sqrt(S[j + j * LD]) : S[r + j * LD];
    __syncthreads();
  }

  // ---- 2: A -> full symmetric image; C = L^-1 A L^-T (CONG: C = L^T A L)
  if (row)
    for (int j = sub; j <= r; j += P) {
      const double x = ldexp(A[r + (size_t)j * lda], -aex);
      S[r + j * LD] = x;
      S[j + r * LD] = x;
    }
  if (CONG) {
    __syncthreads();
    // Y = A L: the pair r owns row r of the full image
    cong_pass<C, false>(S, B, ldb, n, t, r, sub, row, sl, sp, sp + NC, sv, sw);
    // Y^T = L^T A (A is symmetric): the image transposed in place
    if (row)
      for (int j = sub; j < r; j += P) {
        const double lo = S[r + j * LD], up = S[j + r * LD];
        S[r + j * LD] = up;
        S[j + r * LD] = lo;
      }
    __syncthreads();
    // C = Y^T L, lower half: the pair r owns row r, columns 0 .. r
    cong_pass<C, true>(S, B, ldb, n, t, r, sub, row, sl, sp, sp + NC, sv, sw);
    if (row)
      for (int j = sub; j < r; j += P) S[j + r * LD] = S[r + j * LD];
  } else if (a.problem) {
    if (t < n) sl[t] = B[t];                        // column 0 of L
    __syncthreads();
    // X = L^-1 A, transposed: the pair r owns column r of X = row r of the image
    {
      double pv = row ? S[r] : 0.0;
      __syncthreads();                              // both halves hold the first pivot before half 0 overwrites it
      for (int k = 0; k < n; ++k) {
        const double *cur = sl + (k & 1) * NC;
        double nx = 0.0, nv = 0.0;
        if (k + 1 < n && t > k && t < n) nx = B[t + (size_t)(k + 1) * ldb];
        if (row) {
          if (k + 1 < n) nv = S[r + (k + 1) * LD];  // step k - 1 wrote it; this step leaves it alone
          const double xk = pv / cur[k];
          if (sub == 0) S[r + k * LD] = xk;
          pv = nv - cur[min(k + 1, n - 1)] * xk;
          img_axpy<LD, P>(S + r, cur, xk, k + 2 + sub, n);
        }
        if (t < n) sl[((k + 1) & 1) * NC + t] = nx;
        __syncthreads();
      }
    }
    // the lower half of X the right way round: X[r, j] = image[j, r]
    if (row)
      for (int j = sub; j < r; j += P) S[r + j * LD] = S[j + r * LD];
    if (t < n) sl[t] = B[t];
    __syncthreads();
    // C = X L^-T, lower half: the pair r owns row r, columns 0 .. r
    {
      double pv = row ? S[r] : 0.0;
      __syncthreads();                              // both halves hold the first pivot before half 0 overwrites it
      for (int k = 0; k < n; ++k) {
        const double *cur = sl + (k & 1) * NC;
        double nx = 0.0, nv = 0.0;
        if (k + 1 < n && t > k && t < n) nx = B[t + (size_t)(k + 1) * ldb];
        if (row && k <= r) {
          if (k + 1 <= r) nv = S[r + (k + 1) * LD];
          const double ck = pv / cur[k];
          if (sub == 0) S[r + k * LD] = ck;
          pv = nv - cur[min(k + 1, n - 1)] * ck;
          img_axpy<LD, P>(S + r, cur, ck, k + 2 + sub, r + 1);
        }
        if (t < n) sl[((k + 1) & 1) * NC + t] = nx;
        __syncthreads();
      }
    }
    if (row)
      for (int j = sub; j < r; j += P) S[j + r * LD] = S[r + j * LD];
  }
  __syncthreads();

  // ---- 3: Householder tridiagonalisation of the image (both triangles kept, bitwise symmetric)
  for (int k = 0; k + 1 < n; ++k) {
    double x = 0.0;
    if (sub == 0 && row && r >= k + 2) x = S[r + k * LD];
    const double xn2 = block_reduce<NW, false>(x * x, red, phase);
    const double alpha = S[k + 1 + k * LD], dk = S[k + k * LD];
    double tau = 0.0, beta = alpha, scal = 0.0;
    if (xn2 != 0.0) {
      beta = -copysign(sqrt(alpha * alpha + xn2), alpha);
      tau = (beta - alpha) / beta;
      scal = 1.0 / (alpha - beta);
    }
    if (sub == 0 && row) {
      if (r >= k + 2) {
        const double vi = x * scal;
        sv[r] = vi;
        A[r + (size_t)k * lda] = vi;
      } else if (r == k + 1) {
        sv[r] = 1.0;
        se[k] = beta;
        st[k] = tau;
        A[r + (size_t)k * lda] = ldexp(beta, aex);
      } else if (r == k) {
        sd[k] = dk;
        A[k + (size_t)k * lda] = ldexp(dk, aex);
      }
    }
    if (tau == 0.0) continue;                       // H = I (uniform)
    __syncthreads();
    if (row && r > k) sp[sub * NC + r] = img_dot<LD, P>(S + r, sv, k + 1 + sub, n, 0.0);   // p = C v
    __syncthreads();
    double pr = 0.0, vr = 0.0;
    if (sub == 0 && row && r > k) {
      pr = tau * (sp[r] + sp[NC + r]);
      vr = sv[r];
    }
    const double dot = block_reduce<NW, false>(pr * vr, red, phase);
    const double al2 = -0.5 * tau * dot;
    if (sub == 0 && row && r > k) sw[r] = pr + al2 * vr;
    __syncthreads();
    if (row && r > k) {                             // C -= v w^T + w v^T; (r, j) and (j, r) evaluate the same expression
      const double vr2 = sv[r], wr2 = sw[r];
      auto term = [&](int j, double vj, double wj) {
        const bool up = j > r;
        const double vh = up ? vj : vr2, wh = up ? wj : wr2, vl = up ? vr2 : vj, wl = up ? wr2 : wj;
        return vh * wl + wh * vl;
      };
      int j = k + 1 + sub;
      for (; j + 7 * P < n; j += 8 * P) {
        gdouble *c0 = S + r + j * LD;
        double av[8], vv[8], wv[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) av[q] = c0[q * P * LD];
#pragma unroll
        for (int q = 0; q < 8; ++q) { vv[q] = sv[j + q * P]; wv[q] = sw[j + q * P]; }
#pragma unroll
        for (int q = 0; q < 8; ++q) c0[q * P * LD] = av[q] - term(j + q * P, vv[q], wv[q]);
      }
      for (; j < n; j += P) S[r + j * LD] -= term(j, sv[j], sw[j]);
    }
    __syncthreads();
  }
  if (t == 0) {
    const double dl = S[(n - 1) * (LD + 1)];
    sd[n - 1] = dl;
    se[n - 1] = 0.0;
    A[(size_t)(n - 1) * lda + (n - 1)] = ldexp(dl, aex);
  }
  __syncthreads();

  // ---- 4: implicit QL with Z in the image (ek_batched.hip's stage 4)
  int wex = aex;
  {
    double mx = 0.0;
    int bad = 0;
    if (sub == 0 && row) {
      mx = fmax(fabs(sd[r]), fabs(se[r]));
      bad = !(mx <= DBL_MAX);
    }
    if (__syncthreads_or(bad)) {
      if (t == 0) *info = 100000 + n + 1;
      return;
    }
    const double anorm = block_reduce<NW, true>(mx, red, phase);
    if (anorm > 0.0) {
      int ex;
      (void)frexp(anorm, &ex);
      const double sc = ldexp(1.0, -ex);
      wex += ex;
      __syncthreads();
      if (sub == 0 && row) { sd[r] *= sc; se[r] *= sc; }
    }
  }
  __syncthreads();
  int nz = n;                                       // pairs that stage 5 works on: n, or the window's m
  if constexpr (WIN) {
    // ---- 4W: the window's values by bisection, their vectors by inverse iteration as rows 0 .. nz - 1 of the image
    constexpr int OWNER = VWIN ? 2 + CONG : CONG;   // s_rounds: one variable per kernel
    if (!bwindow::stage4w<NC, NW, bwindow::RowsInMemory, OWNER>(window(a), a.jobz, n, wex, S, sd, se, sv, sw, sp, sl, red,
                                                                phase, srank, W, info, nz))
      return;
  } else {
    const bool flip = fabs(sd[0]) > fabs(sd[n - 1]);
    {
      double dr = 0.0, er = 0.0;
      if (flip && sub == 0 && row) {
        dr = sd[n - 1 - r];
        er = (r < n - 1) ? se[n - 2 - r] : 0.0;
      }
      __syncthreads();
      if (flip && sub == 0 && row) { sd[r] = dr; se[r] = er; }
    }
    if (a.jobz && row)
      for (int j = sub; j < n; j += P) S[r + j * LD] = (r == (flip ? n - 1 - j : j)) ? 1.0 : 0.0;
    __syncthreads();
    {
      const double eps = 1.1102230246251565e-16;
      double *sc_ = sv, *ss_ = sw;
      int failed = 0;
      int iter = 0;
      for (int l = 0; l < n && !failed; ++l) {
        while (true) {
          if (t == 0) {
            int m = l;
            for (bool found = false; !found;) {
              double dv[9], ev[8];
#pragma unroll
              for (int q = 0; q < 9; ++q) dv[q] = sd[min(m + q, n - 1)];
#pragma unroll
              for (int q = 0; q < 8; ++q) ev[q] = se[min(m + q, n - 1)];
              int hit = -1;
#pragma unroll
              for (int q = 7; q >= 0; --q)
                if (m + q >= n - 1 || fabs(ev[q]) <= eps * (fabs(dv[q]) + fabs(dv[q + 1]))) hit = q;
              if (hit >= 0) { m = min(m + hit, n - 1); found = true; } else m += 8;
            }
            if (m == l) {
              s_state = 0;
            } else if (iter++ == 30 * n) {
              s_state = 2;
            } else {
              const double dl = sd[l], el = se[l];
              double g = (sd[l + 1] - dl) / (2.0 * el);
              double rr = sqrt(g * g + 1.0);
              g = sd[m] - dl + el / (g + copysign(rr, g));
              double s = 1.0, c = 1.0, p = 0.0;
              int i, lo = l;
              bool under = false;
              double ei = se[m - 1], di = sd[m - 1], dup = sd[m];
              for (i = m - 1; i >= l; --i) {
                double en = 0.0, dn = 0.0;
                if (i > l) { en = se[i - 1]; dn = sd[i - 1]; }
                const double f = s * ei, bb = c * ei;
                const double h = f * f + g * g;
                if (!(h >= 1e-280)) {                 // recover from underflow: split here
                  se[i + 1] = 0.0;
                  sd[i + 1] = dup - p;
                  se[m] = 0.0;
                  under = true;
                  lo = i + 1;
                  break;
                }
                double y = __builtin_amdgcn_rsq(h);
                y = y * (1.5 - 0.5 * h * y * y);
                y = y * (1.5 - 0.5 * h * y * y);
                rr = h * y;
                se[i + 1] = rr;
                s = f * y;
                c = g * y;
                g = dup - p;
                rr = (di - g) * s + 2.0 * c * bb;
                p = s * rr;
                sd[i + 1] = g + p;
                g = c * rr - bb;
                sc_[i] = c;
                ss_[i] = s;
                dup = di; di = dn; ei = en;
              }
              if (!under) {
                sd[l] = dup - p;
                se[l] = g;
                se[m] = 0.0;
              }
              s_state = 1; s_m = m; s_lo = lo;
            }
          }
          __syncthreads();
          const int state = s_state, m = s_m, lo = s_lo;
          if (state == 1 && a.jobz && t < n) {        // the sweep's rotations on row t of Z
            gdouble *zr = S + t;
            double f = zr[m * LD];
            int i = m - 1;
            for (; i - 7 >= lo; i -= 8) {             // eight rotations' loads before the first store
              double zv[8], cv[8], sv8[8];
#pragma unroll
              for (int q = 0; q < 8; ++q) zv[q] = zr[(i - q) * LD];
#pragma unroll
              for (int q = 0; q < 8; ++q) { cv[q] = sc_[i - q]; sv8[q] = ss_[i - q]; }
#pragma unroll
              for (int q = 0; q < 8; ++q) {
                zr[(i + 1 - q) * LD] = sv8[q] * zv[q] + cv[q] * f;
                f = cv[q] * zv[q] - sv8[q] * f;
              }
            }
            for (; i >= lo; --i) {
              const double c = sc_[i], s = ss_[i], z0 = zr[i * LD];
              zr[(i + 1) * LD] = s * z0 + c * f;
              f = c * z0 - s * f;
            }
            zr[lo * LD] = f;
          }
          __syncthreads();
          if (state == 2) failed = l + 1;
          if (state != 1) break;
        }
      }
      if (failed) {
        if (t == 0) *info = 100000 + failed;
        return;
      }
    }
    if (!rank_sort<NC>(n, wex, sd, srank, W, info)) return;
  }
  if (!a.jobz) {
    if (t == 0) *info = 0;
    return;
  }
  gdouble *Z = vectors(a, p);
  const int ldz = p.ldz;

  // ---- 5: the image becomes Z^T: the pair r owns column r of Z = row r of the image (WIN: stage 4W left its nz vectors
  // as rows already, and only the pairs r < nz work)
  const bool zrow = WIN ? r < nz : row;
  if (!WIN && row)
    for (int j = sub; j < r; j += P) {
      const double lo = S[r + j * LD], up = S[j + r * LD];
      S[r + j * LD] = up;
      S[j + r * LD] = lo;
    }
  // Z <- H_0 ... H_{n-3} Z (H_{n-2} = I)
  if (n >= 3) {
    if (t < n) sl[t] = (t >= n - 1) ? A[t + (size_t)(n - 3) * lda] : 0.0;
    __syncthreads();
    for (int k = n - 3, s = 0; k >= 0; --k, ++s) {
      const double *cur = sl + (s & 1) * NC;
      double nx = 0.0;
      if (k >= 1 && t > k && t < n) nx = A[t + (size_t)(k - 1) * lda];
      const double tau = st[k];
      if (tau != 0.0) {                             // uniform
        double c1 = 0.0;
        if (zrow) {
          if (sub == 0) c1 = S[r + (k + 1) * LD];
          sp[sub * NC + r] = img_dot<LD, P>(S + r, cur, k + 2 + sub, n, c1);
        }
        __syncthreads();
        if (zrow) {
          const double dot = (sp[r] + sp[NC + r]) * tau;
          if (sub == 0) S[r + (k + 1) * LD] = c1 - dot;
          img_axpy<LD, P>(S + r, cur, dot, k + 2 + sub, n);
        }
      }
      if (t < n) sl[((s + 1) & 1) * NC + t] = nx;
      __syncthreads();
    }
  }
  if (CONG && a.itype == 3) {
    // Z <- L Z, a column of L per step from the last: entry i > k sees the steps k = i-1 .. 0 in that order whichever
    // thread applies them; z[k] is as stage 4 and the reflectors left it until step k, loaded by both halves a step ahead
    __syncthreads();
    if (t < n) sl[t] = (t == n - 1) ? B[t + (size_t)(n - 1) * ldb] : 0.0;
    double pv = zrow ? S[r + (n - 1) * LD] : 0.0;
    __syncthreads();
    for (int k = n - 1, s = 0; k >= 0; --k, ++s) {
      const double *cur = sl + (s & 1) * NC;
      double nx = 0.0;
      if (k >= 1 && t >= k - 1 && t < n) nx = B[t + (size_t)(k - 1) * ldb];
      if (zrow) {
        double nv = 0.0;
        if (k >= 1) nv = S[r + (k - 1) * LD];       // no step before its own writes it
        if (sub == 0) S[r + k * LD] = pv * cur[k];
        img_axpy<LD, P>(S + r, cur, -pv, k + 1 + sub, n);
        pv = nv;
      }
      if (t < n) sl[((s + 1) & 1) * NC + t] = nx;
      __syncthreads();
    }
  } else if (a.problem) {                           // Z <- L^-T Z
    __syncthreads();
    if (t < n) sl[t] = (t == n - 1) ? B[t + (size_t)(n - 1) * ldb] : 0.0;
    __syncthreads();
    for (int i = n - 1, s = 0; i >= 0; --i, ++s) {
      const double *cur = sl + (s & 1) * NC;
      double nx = 0.0;
      if (i >= 1 && t >= i - 1 && t < n) nx = B[t + (size_t)(i - 1) * ldb];
      double zi = 0.0;
      if (zrow) {
        if (sub == 0) zi = S[r + i * LD];
        sp[sub * NC + r] = img_dot<LD, P>(S + r, cur, i + 1 + sub, n, 0.0);
      }
      __syncthreads();
      if (sub == 0 && zrow) S[r + i * LD] = ((zi - sp[r]) - sp[NC + r]) / cur[i];
      if (t < n) sl[((s + 1) & 1) * NC + t] = nx;
      __syncthreads();
    }
  }
  __syncthreads();
  if (row) {                                        // Z[r, j] = image[j, r], j < nz
    int j = sub;
    for (; j + 7 * P < nz; j += 8 * P) {
      double zv[8];
      int rk[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) zv[q] = S[j + q * P + r * LD];
#pragma unroll
      for (int q = 0; q < 8; ++q) rk[q] = srank[j + q * P];
#pragma unroll
      for (int q = 0; q < 8; ++q) Z[r + (size_t)rk[q] * ldz] = zv[q];
    }
    for (; j < nz; j += P) Z[r + (size_t)srank[j] * ldz] = S[j + r * LD];
  }
  if (t == 0) *info = 0;
}

// the images: grown, never shrunk, released in ek_hip_finalize.  One allocation serves both classes, counted in doubles: a
// launch of either holds g_mu, and every call ends with a synchronise, so no two launches ever share it
static double *g_ws = nullptr;
static size_t g_ws_doubles = 0;
static int g_chunk = ClassX::kChunk, g_ychunk = ClassY::kChunk;

// room for `slots` images of `slot` doubles each
static int ensure_images(size_t slots, size_t slot = ClassX::kSlot) {
  const size_t need = slots * slot;
  if (need <= g_ws_doubles) return 0;
  if (g_ws) (void)hipFree(g_ws);
  g_ws = nullptr;
  g_ws_doubles = 0;
  EK_HIP_CHECK(hipMalloc((void **)&g_ws, need * sizeof(double)));
  g_ws_doubles = need;
  return 0;
}
static bool images_hold(int slots) { return (size_t)slots * ClassX::kSlot <= g_ws_doubles; }

}  // namespace batchedx

namespace api {

void release_xbatched() {
  using namespace batchedx;
  if (g_ws) (void)hipFree(g_ws);
  g_ws = nullptr;
  g_ws_doubles = 0;
}

// arguments checked (EK_HIP_BATCH_NMAX < n <= EK_HIP_XBATCH_NMAX, batch > 0), g_mu held; dinfo holds `batch` words
int xbatched_launch(hipStream_t s, int problem, int itype, int jobz, int n, int batch, double *dA, int lda,
                    long long strideA, double *dB, int ldb, long long strideB, double *dw, double *dZ, int ldz,
                    long long strideZ, int *dinfo) {
  using namespace batchedx;
  const int K = g_chunk;
  { int rc0 = ensure_images((size_t)std::min(batch, K)); if (rc0) return rc0; }
  for (int c0 = 0; c0 < batch; c0 += K) {
    const int count = std::min(K, batch - c0);
    Args a{problem, jobz, n, dA + (long long)c0 * strideA, lda, strideA,
           problem ? dB + (long long)c0 * strideB : nullptr, ldb, strideB, dw + (long long)c0 * n,
           jobz ? dZ + (long long)c0 * strideZ : nullptr, ldz, strideZ, dinfo + c0, g_ws, itype};
    if (problem && itype != 1) hipLaunchKernelGGL((xbatched_kernel<true, Args>), dim3(count), dim3(ClassX::T), 0, s, a);
    else hipLaunchKernelGGL((xbatched_kernel<false, Args>), dim3(count), dim3(ClassX::T), 0, s, a);
    EK_HIP_CHECK(hipGetLastError());
  }
  return 0;
}

// ek_hip_*_ybatched*: arguments checked (EK_HIP_XBATCH_NMAX < n <= EK_HIP_YBATCH_NMAX, batch > 0), g_mu held; dinfo holds
// `batch` words.  ClassY's two instantiations of the kernel: a workgroup of 1024 threads fills a compute unit, so a chunk
// is one round of 256 workgroups; the chunks share the slots 0 .. K-1 in the order of the stream
int ybatched_launch(hipStream_t s, int problem, int itype, int jobz, int n, int batch, double *dA, int lda,
                    long long strideA, double *dB, int ldb, long long strideB, double *dw, double *dZ, int ldz,
                    long long strideZ, int *dinfo) {
  using namespace batchedx;
  const int K = g_ychunk;
  { int rc0 = ensure_images((size_t)std::min(batch, K), ClassY::kSlot); if (rc0) return rc0; }
  for (int c0 = 0; c0 < batch; c0 += K) {
    const int count = std::min(K, batch - c0);
    Args a{problem, jobz, n, dA + (long long)c0 * strideA, lda, strideA,
           problem ? dB + (long long)c0 * strideB : nullptr, ldb, strideB, dw + (long long)c0 * n,
           jobz ? dZ + (long long)c0 * strideZ : nullptr, ldz, strideZ, dinfo + c0, g_ws, itype};
    if (problem && itype != 1)
      hipLaunchKernelGGL((xbatched_kernel<true, Args, ClassY>), dim3(count), dim3(ClassY::T), 0, s, a);
    else
      hipLaunchKernelGGL((xbatched_kernel<false, Args, ClassY>), dim3(count), dim3(ClassY::T), 0, s, a);
    EK_HIP_CHECK(hipGetLastError());
  }
  return 0;
}

// the images of a variable call with `count` > 0 problems above EK_HIP_BATCH_NMAX, before its first event: growing them
// frees and allocates, which synchronises the device and belongs neither into `seconds` nor beside a running class
int xvbatched_prepare(int count) {
  using namespace batchedx;
  return ensure_images((size_t)std::min(count, g_chunk));
}

// ek_hip_eigenpairs_window_xbatched*: the images of a launch of `slots` workgroups, before the call's first event
int xwindow_prepare(int slots) {
  using namespace batchedx;
  return ensure_images((size_t)slots);
}

// One chunk of `count` <= slots problems of order EK_HIP_BATCH_NMAX + 1 .. EK_HIP_XBATCH_NMAX through the window
// instantiation (CONG's for types 2 and 3): the pointers are the chunk's, dm and dinfo hold a word per problem of it, lu
// a slot of 5 n wcols doubles per workgroup (jobz = 1).  g_mu held, xwindow_prepare(slots) done
int xwindow_launch(hipStream_t s, int problem, int itype, int jobz, int n, int count, double *dA, int lda,
                   long long strideA, double *dB, int ldb, long long strideB, double *dw, double *dZ, int ldz,
                   long long strideZ, int *dinfo, int range, int il, int iu, int zcap, double vl, double vu, int *dm,
                   double *lu, int wcols) {
  using namespace batchedx;
  if (!images_hold(count)) return -1000 - (int)hipErrorInvalidValue;
  XWArgs a{{problem, jobz, n, dA, lda, strideA, problem ? dB : nullptr, ldb, strideB, dw, jobz ? dZ : nullptr, ldz,
            strideZ, dinfo, g_ws, itype},
           {range, il, iu, zcap, vl, vu, dm, lu, wcols}};
  if (problem && itype != 1) hipLaunchKernelGGL((xbatched_kernel<true, XWArgs>), dim3(count), dim3(ClassX::T), 0, s, a);
  else hipLaunchKernelGGL((xbatched_kernel<false, XWArgs>), dim3(count), dim3(ClassX::T), 0, s, a);
  EK_HIP_CHECK(hipGetLastError());
  return 0;
}

// ek_hip_*_window_xvbatched*: one launch of `count` <= slots entries of the two tables (device; orders above
// EK_HIP_BATCH_NMAX) through the table-and-window instantiation; dinfo and dm hold a word per problem of the caller's
// batch; lu is the base of the class's region of the LU workspace, the entries' offsets counted from it.  g_mu held,
// xwindow_prepare(slots) done
int xvwindow_launch(hipStream_t s, int problem, int itype, int jobz, int range, int count, const batched::Desc *table,
                    const batched::WDesc *wtable, int *dinfo, int *dm, double *lu) {
  using namespace batchedx;
  if (!images_hold(count)) return -1000 - (int)hipErrorInvalidValue;
  XVWArgs a{problem, jobz, table, wtable, dinfo, dm, g_ws, lu, range, itype};
  if (problem && itype != 1) hipLaunchKernelGGL((xbatched_kernel<true, XVWArgs>), dim3(count), dim3(ClassX::T), 0, s, a);
  else hipLaunchKernelGGL((xbatched_kernel<false, XVWArgs>), dim3(count), dim3(ClassX::T), 0, s, a);
  EK_HIP_CHECK(hipGetLastError());
  return 0;
}

// arguments checked, g_mu held, xvbatched_prepare(count) done; `table` (device) holds `count` > 0 entries of orders
// EK_HIP_BATCH_NMAX + 1 .. EK_HIP_XBATCH_NMAX; dinfo holds a word per problem of the caller's batch.  The chunks share the
// slots 0 .. K-1: the order of the stream is what separates two users of a slot, so every chunk goes on s.
int xvbatched_launch(hipStream_t s, int problem, int itype, int jobz, int count, const batched::Desc *table,
                     int *dinfo) {
  using namespace batchedx;
  const int K = g_chunk;
  if (!images_hold(std::min(count, K))) return -1000 - (int)hipErrorInvalidValue;
  for (int c0 = 0; c0 < count; c0 += K) {
    const int chunk = std::min(K, count - c0);
    XVArgs a{problem, jobz, table + c0, dinfo, g_ws, itype};
    if (problem && itype != 1) hipLaunchKernelGGL((xbatched_kernel<true, XVArgs>), dim3(chunk), dim3(ClassX::T), 0, s, a);
    else hipLaunchKernelGGL((xbatched_kernel<false, XVArgs>), dim3(chunk), dim3(ClassX::T), 0, s, a);
    EK_HIP_CHECK(hipGetLastError());
  }
  return 0;
}

}  // namespace api
}  // namespace ek

extern "C" int ek_hip_debug_xbatched_chunk(int problems) {
  std::lock_guard<std::mutex> lk(ek::api::g_mu);
  const int before = ek::batchedx::g_chunk;
  ek::batchedx::g_chunk = problems > 0 ? problems : ek::batchedx::ClassX::kChunk;
  return before;
}

extern "C" int ek_hip_debug_ybatched_chunk(int problems) {
  std::lock_guard<std::mutex> lk(ek::api::g_mu);
  const int before = ek::batchedx::g_ychunk;
  ek::batchedx::g_ychunk = problems > 0 ? problems : ek::batchedx::ClassY::kChunk;
  return before;
}
