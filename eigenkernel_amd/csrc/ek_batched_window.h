// ek_batched_window.h -- stage 4W of the batched kernels (ek_batched.hip, ek_batched_x.hip; not installed; DESIGN.md 30,
// 32): a window of eigenpairs of the scaled tridiagonal (d, e) in LDS by Sturm bisection and inverse iteration, in place
// of the QL of stage 4.  Called by the whole workgroup of the window instantiations (ek_hip_eigenpairs_window_batched*,
// ek_hip_eigenpairs_window_xbatched*) and by no other.
//
//   count    Gershgorin interval, pivmin, tolerance and number of passes by ek_stebz.hip's rules; RANGE 'V' counts at
//            vl and vu (every thread runs the two chains: the result is uniform without a broadcast)
//   bisect   kLanes lanes per wanted index, kPts points per lane and pass: a pass splits the index's bracket into
//            S = kLanes kPts equal parts and keeps the one that holds the index.  Every index makes the same passes from
//            the same interval, so a bracket is a cell of one grid that (d, e) fix: the value of index k depends on
//            (d, e, k) alone.  S is a constant, not a function of the window's width.  ek_stebz.hip's tolerance is
//            absolute, 4 eps |T|; an eigenvalue that is small against |T| goes on, up to kRefine passes, until its
//            bracket meets DSTEBZ's relative criterion: where T determines it to high relative accuracy (a pencil
//            whose spectrum spans cond(B)) the residual of its vector is measured against that value, not against |T|
//   vectors  DSTEIN on the whole of T: lane j owns wanted vector j, which lives in column j of the image.  DLAGTF's LU of
//            T - lambda I goes to the workgroup's slot of a device workspace, [array][row][vector] so that the lanes of
//            a wave read consecutive addresses; DLAGTS(-1) solves from it.  Eigenvalues closer than 10 eps |lambda| are
//            separated, clusters are runs with gaps <= 1e-3 |T|_1, and the clusters are worked in rounds: round r
//            iterates every vector that is the r-th of its cluster, and between its solves the whole workgroup
//            orthogonalises those vectors against the r finished ones in front of them (classical Gram-Schmidt, twice,
//            every sum in a fixed order).  Threads meet at barriers only; every loop is bounded by n, m and constants.
//            Where this is not DSTEIN: T is not split into its blocks, so |T|_1 in ortol and in the scaling of the
//            right-hand side is the whole matrix's; that scaling uses eps = 2^-53 where DSTEIN has DLAMCH('P'); and a
//            vector has 5 iterations to meet the growth test and then 2 more (DSTEIN: 5 in all).
//
// The image comes in two layouts (the LAY parameter of stage4w):
//   ColumnsInLds   ek_batched.hip: the image in LDS, wanted vector j is column j, entry i at S[i + j LD]
//   RowsInMemory   ek_batched_x.hip: the image in device memory, wanted vector j is ROW j, entry i at
//                  S[j + i LD], so that the lanes of a wave that iterate consecutive vectors touch consecutive addresses
//                  and stage 5 of that kernel finds Z^T where it wants it.  Its loops over a vector load eight entries
//                  ahead of their use, and the two Gram-Schmidt passes have a thread map of their own (see there)
#pragma once
#include "ek_batched_stages.h"

#include <cstdint>

namespace ek {
namespace bwindow {
using namespace bstages;

constexpr int kLanes = 2, kPts = 4, kParts = kLanes * kPts;   // 3 bits per pass
constexpr int kRefine = 18;                                   // further passes an eigenvalue small against |T| may take
constexpr int kMaxIts = 5, kExtra = 2;                        // DSTEIN: 5 iterations to grow, then 2 more

// where the wanted vectors live (see the head of this file)
struct ColumnsInLds { typedef double elem; static constexpr bool rows = false; };
struct RowsInMemory { typedef gdouble elem; static constexpr bool rows = true; };
constexpr int kTree = 16;                           // RowsInMemory: members in front from which an update sums by a tree

// what the window entries add to the batched kernel's arguments
struct Window {
  int range, il, iu, zcap;
  double vl, vu;
  int *m;                                           // device: a word per problem of the launch
  double *ws;                                       // LU workspace: a slot of 5 n wcols doubles per workgroup
  int wcols;                                        // vectors a slot holds
};
// The variable-order form (ek_hip_*_window_xvbatched*): the same fields filled from the workgroup's entry of the window
// table, m the problem's own word and ws the base of its own LU slot.  The type is what tells stage4w how to find the two
struct OwnWindow : Window {};
__device__ __forceinline__ int *m_word(const Window &a) { return a.m + blockIdx.x; }
__device__ __forceinline__ int *m_word(const OwnWindow &a) { return a.m; }
__device__ __forceinline__ gdouble *lu_slot(const Window &a, int n, int wc) {
  return (gdouble *)(a.ws + (size_t)blockIdx.x * 5 * (size_t)n * wc);
}
__device__ __forceinline__ gdouble *lu_slot(const OwnWindow &a, int, int) { return (gdouble *)a.ws; }

using batched::WDesc;                              // the window table's entry (ek_api_internal.h)
__device__ __forceinline__ OwnWindow own_window(int range, const WDesc &e, int *m, double *ws) {
  return OwnWindow{{range, e.il, e.iu, e.zcap, e.vl, e.vu, m, ws + e.lu, e.wcols}};
}

// negative pivots of the LDL^T of T - x I at K points (ek_stebz.hip's sturm_counts on LDS operands)
template <int K>
__device__ __forceinline__ void counts(int n, const double *d, const double *e2, double pivmin, const double (&x)[K],
                                       int (&cnt)[K]) {
#pragma clang fp contract(off)
  double q[K];
  const double d0 = d[0];
#pragma unroll
  for (int p = 0; p < K; ++p) {
    double v = d0 - x[p];
    if (fabs(v) < pivmin) v = -pivmin;
    q[p] = v; cnt[p] = v < 0.0 ? 1 : 0;
  }
#pragma unroll 2
  for (int i = 1; i < n; ++i) {
    const double di = d[i], ei = e2[i - 1];
#pragma unroll
    for (int p = 0; p < K; ++p) {
      double v = (di - x[p]) - ei / q[p];
      if (fabs(v) < pivmin) v = -pivmin;
      q[p] = v; cnt[p] += v < 0.0 ? 1 : 0;
    }
  }
}

// the start vector of global index k (0-based), row i: uniform in [-1, 1), the same wherever the problem runs
__device__ __forceinline__ double start_entry(int k, int i) {
  uint32_t h = (uint32_t)k * 0x9E3779B1u ^ ((uint32_t)i * 0x85EBCA77u + 0x165667B1u);
  h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12; h *= 0x297A2D39u; h ^= h >> 15;
  return (double)(int32_t)h * 0x1p-31;
}

// RowsInMemory: the vectors of round `round` (pos[j] == round, not finished) against the `round` finished members in
// front of each, classical Gram-Schmidt twice, by the whole workgroup of 2 NC threads.  Vector j is row j of the image.
//   dots     thread (r, sub) takes finished vector r and the round's vector of its cluster: the entries sub, sub + 2, ...
//            in ascending order from 0.0; a product is half 0's sum plus half 1's.  The lanes of a wave are consecutive
//            vectors: consecutive addresses, and one address for the mate of a cluster
//   update   round < kTree: thread (r, sub) takes the round's vector r and every other entry of it; an entry's sum runs
//            over the members in front in ascending order.  The lanes are vectors again: the many small clusters.
//            round >= kTree: the round's vectors one after the other; a wave takes eight entries at a time, lane l the
//            members l, l + 64, ... in front (consecutive addresses), in ascending order, and the 64 partial sums are
//            added by a butterfly: the few large clusters, where one lane per vector would leave the workgroup idle.
// Either way the order of a sum depends on the position in the cluster (round, member) and on n alone, not on where the
// cluster lies in the window.  Starts with a barrier; the caller's barrier ends it.
template <int NC, int NW>
__device__ __forceinline__ void gram_schmidt_rows(gdouble *S, int n, int m, int round, const int *pos, const int *fin,
                                                  double *sl) {
  constexpr int LD = NC + 1;
  const int t = threadIdx.x, r = t % NC, sub = t / NC;
  for (int pass = 0; pass < 2; ++pass) {
    __syncthreads();
    if (r < m) {
      const int j = r - pos[r] + round;
      if (pos[r] < round && j < m && pos[j] == round && !fin[j]) {
        const gdouble *xp = S + r, *xj = S + j;
        double acc = 0.0;
        for (int i0 = sub; i0 < n; i0 += 16) {
          double pv[8], jv[8];
#pragma unroll
          for (int q = 0; q < 8; ++q) {
            const int i = min(i0 + 2 * q, n - 1);
            pv[q] = xp[i * LD];
            jv[q] = xj[i * LD];
          }
#pragma unroll
          for (int q = 0; q < 8; ++q)
            if (i0 + 2 * q < n) acc += pv[q] * jv[q];
        }
        sl[sub * NC + r] = acc;
      }
    }
    __syncthreads();
    if (round < kTree) {
      if (r < m && pos[r] == round && !fin[r]) {
        const gdouble *xq = S + (r - round);
        const double *c0 = sl + (r - round), *c1 = c0 + NC;
        for (int i = sub; i < n; i += 2) {
          double acc = 0.0;
          for (int q0 = 0; q0 < round; q0 += 8) {
            double v8[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v8[q] = xq[min(q0 + q, round - 1) + i * LD];
#pragma unroll
            for (int q = 0; q < 8; ++q)
              if (q0 + q < round) acc += (c0[q0 + q] + c1[q0 + q]) * v8[q];
          }
          S[r + i * LD] -= acc;
        }
      }
    } else {
      const int wv = t >> 6, ln = t & 63;
      for (int j = 0; j < m; ++j) {
        if (pos[j] != round || fin[j]) continue;    // uniform
        const gdouble *xq = S + (j - round);
        const double *c0 = sl + (j - round), *c1 = c0 + NC;
        for (int ib = 0; ib < n; ib += 8 * NW) {    // entries ib + wv + NW q
          double acc[8];
#pragma unroll
          for (int q = 0; q < 8; ++q) acc[q] = 0.0;
          for (int c = ln; c < round; c += 64) {
            const double cf = c0[c] + c1[c];
            double v8[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v8[q] = xq[c + min(ib + wv + NW * q, n - 1) * LD];
#pragma unroll
            for (int q = 0; q < 8; ++q) acc[q] += cf * v8[q];
          }
#pragma unroll
          for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
            for (int q = 0; q < 8; ++q) acc[q] += __shfl_xor(acc[q], off, 64);
          }
          if (ln == 0) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
              const int i = ib + wv + NW * q;
              if (i < n) S[j + i * LD] -= acc[q];
            }
          }
        }
      }
    }
  }
}

// Stage 4W.  In: sd, se the scaled tridiagonal (|T| in [1/2, 1), or T = 0), w = 2^wex lambda.  Scratch: sv (lambda),
// sw (e^2), sp (2 NC doubles: positions in the cluster, done flags), sl (2 NC: dot products); st is not touched.
// True: mout values went to w, and with jobz their vectors stand in columns 0 .. mout - 1 of the image, srank is the
// identity.  False: the problem has ended (info and m[b] written): an empty window, -20, or a failure.
// OWNER: nothing but a name.  s_rounds below is one LDS variable per instantiation of this function; a kernel passes a
// value of its own, so that no two kernels share the variable and each keeps it in its own LDS frame.
// WINDOW: Window (the uniform calls: the m word and the LU slot at blockIdx.x) or OwnWindow (the variable-order calls: both
// are the problem's own).
template <int NC, int NW, typename LAY = ColumnsInLds, int OWNER = 0, typename WINDOW = Window>
__device__ __forceinline__ bool stage4w(const WINDOW &a, int jobz, int n, int wex, typename LAY::elem *S, double *sd,
                                        double *se,
                                        double *sv, double *sw, double *sp, double *sl, double *red, int &phase,
                                        int *srank, gdouble *w, int *info, int &mout) {
  constexpr int LD = NC + 1;
  constexpr int XS = LAY::rows ? LD : 1;            // from an entry of a vector to the next, from a vector to the next
  constexpr int VS = LAY::rows ? 1 : LD;
  constexpr int KB = LAY::rows ? 4 : 8;             // rows DLAGTS loads ahead of their use: registers
  typedef typename LAY::elem elem;
  const int t = threadIdx.x, r = t % NC, sub = t / NC;
  const bool row = r < n;
  int *mword = m_word(a);
  __shared__ int s_rounds;
  mout = 0;

  // ---- count: e^2, Gershgorin, |T|_1
  double glo = -DBL_MAX, ghi = -DBL_MAX, m2 = 0.0, cs = 0.0;   // maxima of -(d - r), d + r, e^2, the column sums
  {
#pragma clang fp contract(off)
    if (sub == 0 && row) {
      const double ei = (r < n - 1) ? se[r] : 0.0, ep = (r > 0) ? se[r - 1] : 0.0;
      const double sq = ei * ei, rad = fabs(ep) + fabs(ei);
      sw[r] = sq;
      m2 = sq;
      glo = -(sd[r] - rad);
      ghi = sd[r] + rad;
      cs = fabs(sd[r]) + rad;
    }
  }
  glo = block_reduce<NW, true>(glo, red, phase);
  ghi = block_reduce<NW, true>(ghi, red, phase);
  m2 = block_reduce<NW, true>(m2, red, phase);
  const double onenrm = block_reduce<NW, true>(cs, red, phase);
  __syncthreads();                                  // e^2 is in sw for everyone
  double gl = -glo, gu = ghi, pivmin;
  int passes = 0;
  {
#pragma clang fp contract(off)
    const double eps = DBL_EPSILON * 0.5, fudge = 2.1;
    pivmin = DBL_MIN * (m2 > 1.0 ? m2 : 1.0);
    const double tnorm = fabs(gl) > fabs(gu) ? fabs(gl) : fabs(gu);
    gl = gl - fudge * tnorm * eps * n - fudge * 2.0 * pivmin;
    gu = gu + fudge * tnorm * eps * n + fudge * pivmin;
    const double tol = 2.0 * (2.0 * eps) * tnorm + 2.0 * pivmin;
    if (tnorm == 0.0) { gl = 0.0; gu = 0.0; }
    double wd = gu - gl;
    while (wd > tol && passes < 64) { wd *= 1.0 / kParts; ++passes; }
  }
  const bool zero = (gl == 0.0 && gu == 0.0);       // T = 0: every eigenvalue is 0, the vectors are unit vectors

  int first = a.il, m = a.iu - a.il + 1;            // 1-based index of the first wanted value, their number
  if (a.range == 1) {
    const double vl = ldexp(a.vl, -wex), vu = ldexp(a.vu, -wex);   // the kernel's own scaling: exact
    const double x[2] = {vl < gl ? gl : (vl > gu ? gu : vl), vu < gl ? gl : (vu > gu ? gu : vu)};
    int cnt[2];
    counts<2>(n, sd, sw, pivmin, x, cnt);
    if (vl < gl) cnt[0] = 0; else if (vl >= gu) cnt[0] = n;
    if (vu < gl) cnt[1] = 0; else if (vu >= gu) cnt[1] = n;
    first = cnt[0] + 1;
    m = cnt[1] - cnt[0];
    if (m < 0) m = 0;
    if (jobz && m > a.zcap) {                       // the window is wider than Z: the count, and nothing else
      if (t == 0) { *mword = m; *info = -20; }
      return false;
    }
  }
  if (m == 0) {
    if (t == 0) { *mword = 0; *info = 0; }
    return false;
  }

  // ---- bisect: lanes 2 j, 2 j + 1 work on wanted index j
  const int idx = t / kLanes, g = t % kLanes;
  int bad = 0;
  double lam = 0.0, wr = 0.0;
  if (idx < m) {
#pragma clang fp contract(off)
    const int k = first + idx;
    double lo = gl, hi = gu;
    const double inv_s = 1.0 / (double)kParts;
    for (int pass = 0; pass < passes + kRefine; ++pass) {
      const double h = hi - lo;
      // past the common passes a bracket is refined while it is wider than DSTEBZ's relative criterion, 2 ulp of its
      // larger end: the decision is a function of the cell, so the value still depends on (d, e, k) alone
      if (pass >= passes && !(h > fmax(2.0 * DBL_EPSILON * fmax(fabs(lo), fabs(hi)), 2.0 * pivmin))) break;
      double x[kPts];
      int cnt[kPts];
#pragma unroll
      for (int p = 0; p < kPts; ++p) x[p] = lo + h * ((double)(g * kPts + p) * inv_s);
      counts<kPts>(n, sd, sw, pivmin, x, cnt);
      int below = 0;
#pragma unroll
      for (int p = 0; p < kPts; ++p) below += (cnt[p] <= k - 1) ? 1 : 0;
#pragma unroll
      for (int off = 1; off < kLanes; off <<= 1) below += __shfl_xor(below, off, kLanes);
      const int J = below > 0 ? below : 1;
      const double nlo = lo + h * ((double)(J - 1) * inv_s);
      const double nhi = (J < kParts) ? lo + h * ((double)J * inv_s) : hi;
      lo = nlo; hi = nhi;
    }
    lam = lo + (hi - lo) * 0.5;
    wr = ldexp(lam, wex);
    bad = !(fabs(wr) <= DBL_MAX);
  }
  if (__syncthreads_or(bad)) {                      // an eigenvalue beyond a double: rank_sort's exit
    if (t == 0) { *mword = 0; *info = 100000 + n + 1; }
    return false;
  }
  if (idx < m && g == 0) {
    w[idx] = wr;
    sv[idx] = lam;
  }
  if (t < NC) srank[t] = t;
  mout = m;
  if (t == 0) *mword = m;
  if (!jobz) return true;
  __syncthreads();

  // ---- vectors
  if (zero) {
    if constexpr (LAY::rows) {
      if (r < m)
        for (int i = sub; i < n; i += 2) S[r + i * LD] = (i == first - 1 + r) ? 1.0 : 0.0;
    } else if (row)
      for (int j = sub; j < m; j += 2) S[r + j * LD] = (r == first - 1 + j) ? 1.0 : 0.0;
    __syncthreads();
    return true;
  }
  int *pos = (int *)sp, *fin = pos + NC;            // position in the cluster; 1: the vector needs no more work
  const double eps2 = DBL_EPSILON, ortol = 1e-3 * onenrm;
  if (t == 0) {                                     // DSTEIN's separation of close values and its clusters, in order
    int mx = 0;
    pos[0] = 0;
    double xjm = sv[0];
    for (int j = 1; j < m; ++j) {
      double xj = sv[j];
      const double pertol = 10.0 * fabs(eps2 * xj);
      if (xj - xjm < pertol) xj = xjm + pertol;
      sv[j] = xj;
      const int pj = (fabs(xj - xjm) > ortol) ? 0 : pos[j - 1] + 1;
      pos[j] = pj;
      mx = pj > mx ? pj : mx;
      xjm = xj;
    }
    s_rounds = mx + 1;
  }
  if (t < m) fin[t] = 0;
  __syncthreads();
  const int rounds = s_rounds;

  // lane t < m: vector t.  LU of T - lambda I in the slot, element (array q, row i) of vector t at ((q n + i) wcols + t)
  const int wc = a.wcols;
  gdouble *lu = lu_slot(a, n, wc) + t;
  const bool lane = t < m;
  elem *x = S + (lane ? t : 0) * VS;
  const int mypos = lane ? pos[t] : -1;
  const double lamj = lane ? sv[t] : 0.0;
  const double dtpcrt = sqrt(0.1 / n), epsm = DBL_EPSILON * 0.5;
  int failed = 0;

  for (int round = 0; round < rounds; ++round) {
    const bool mine = mypos == round;
    double unn = 0.0, tol = 0.0, xmax = 0.0;
    int jmax = 0, nrmchk = 0, done = 0;
    if (mine) {
      // DLAGTF: a, b, c, d, in -> arrays 0 .. 4
      double ak = sd[0] - lamj, bk = (n > 1) ? se[0] : 0.0;
      double scale1 = fabs(ak) + fabs(bk);
      for (int k = 0; k + 1 < n; ++k) {
        const double ck = se[k];
        const bool inner = k < n - 2;
        double an1 = sd[k + 1] - lamj, bn = inner ? se[k + 1] : 0.0;
        const double scale2 = fabs(ck) + fabs(an1) + (inner ? fabs(bn) : 0.0);
        const double piv1 = (ak == 0.0) ? 0.0 : fabs(ak) / scale1;
        double oa = ak, ob = bk, oc = 0.0, od = 0.0, oin = 0.0;
        if (ck == 0.0) {
          scale1 = scale2;
        } else {
          const double piv2 = fabs(ck) / scale2;
          if (piv2 <= piv1) {
            scale1 = scale2;
            oc = ck / ak;
            an1 = an1 - oc * bk;
          } else {
            oin = 1.0;
            const double mult = ak / ck, temp = an1;
            oa = ck;
            an1 = bk - mult * temp;
            if (inner) { od = bn; bn = -mult * od; }
            ob = temp;
            oc = mult;
          }
        }
        lu[(0 * (size_t)n + k) * wc] = oa;
        lu[(1 * (size_t)n + k) * wc] = ob;
        lu[(2 * (size_t)n + k) * wc] = oc;
        lu[(3 * (size_t)n + k) * wc] = od;
        lu[(4 * (size_t)n + k) * wc] = oin;
        tol = fmax(tol, fmax(fabs(oa), fmax(fabs(ob), fabs(od))));
        ak = an1; bk = bn;
      }
      lu[(0 * (size_t)n + n - 1) * wc] = ak;
      lu[(1 * (size_t)n + n - 1) * wc] = 0.0;
      lu[(3 * (size_t)n + n - 1) * wc] = 0.0;
      unn = ak;
      tol = fmax(tol, fabs(ak)) * epsm;
      if (tol == 0.0) tol = epsm;
      for (int i = 0; i < n; ++i) {
        const double v = start_entry(first - 1 + t, i);
        x[i * XS] = v;
        if (fabs(v) > xmax) { xmax = fabs(v); jmax = i; }
      }
    }
    for (int it = 0; it < kMaxIts + kExtra; ++it) {
      if (mine && !done) {
        const double scl = n * onenrm * fmax(epsm, fabs(unn)) / xmax;
        // DLAGTS(-1): forward through the multipliers and interchanges, KB rows' loads ahead of their use
        double yp = x[0] * scl;
        for (int k0 = 1; k0 < n; k0 += KB) {
          double c8[KB], i8[KB], y8[KB];
#pragma unroll
          for (int q = 0; q < KB; ++q) {
            const int k = min(k0 + q, n - 1);
            c8[q] = lu[(2 * (size_t)n + k - 1) * wc];
            i8[q] = lu[(4 * (size_t)n + k - 1) * wc];
            y8[q] = x[k * XS] * scl;
          }
#pragma unroll
          for (int q = 0; q < KB; ++q) {
            const int k = k0 + q;
            if (k < n) {
              if (i8[q] == 0.0) {
                x[(k - 1) * XS] = yp;
                yp = y8[q] - c8[q] * yp;
              } else {
                x[(k - 1) * XS] = y8[q];
                yp = yp - c8[q] * y8[q];
              }
            }
          }
        }
        x[(n - 1) * XS] = yp;
        // back through U, tiny pivots perturbed
        double y1 = 0.0, y2 = 0.0;
        for (int k0 = n - 1; k0 >= 0; k0 -= KB) {
          double a8[KB], b8[KB], d8[KB], y8[KB];
#pragma unroll
          for (int q = 0; q < KB; ++q) {
            const int k = max(k0 - q, 0);
            a8[q] = lu[(0 * (size_t)n + k) * wc];
            b8[q] = lu[(1 * (size_t)n + k) * wc];
            d8[q] = lu[(3 * (size_t)n + k) * wc];
            y8[q] = x[k * XS];
          }
#pragma unroll
          for (int q = 0; q < KB; ++q) {
            const int k = k0 - q;
            if (k >= 0) {
              double temp = y8[q] - b8[q] * y1 - d8[q] * y2;
              double ak = a8[q], pert = copysign(tol, ak);
              for (int tries = 0; tries < 2200; ++tries) {   // pert doubles: it ends long before
                const double absak = fabs(ak);
                if (absak >= 1.0) break;
                if (absak < DBL_MIN) {
                  if (absak == 0.0 || fabs(temp) * DBL_MIN > absak) { ak += pert; pert *= 2.0; continue; }
                  temp *= 1.0 / DBL_MIN;
                  ak *= 1.0 / DBL_MIN;
                  break;
                }
                if (fabs(temp) > absak * (1.0 / DBL_MIN)) { ak += pert; pert *= 2.0; continue; }
                break;
              }
              const double y = temp / ak;
              x[k * XS] = y;
              y2 = y1; y1 = y;
            }
          }
        }
      }
      if (round > 0) {
        // the round's vectors against the finished members in front of them, by the whole workgroup, twice
        if constexpr (LAY::rows) {
          gram_schmidt_rows<NC, NW>(S, n, m, round, pos, fin, sl);
        } else {
          for (int pass = 0; pass < 2; ++pass) {
            __syncthreads();
            if (t < m) {                            // thread t: the dot product with finished vector t
              const int j = t - pos[t] + round;
              if (pos[t] < round && j < m && pos[j] == round && !fin[j]) {
                const double *xp = S + t * LD, *xj = S + j * LD;
                double acc = 0.0;
                for (int i = 0; i < n; ++i) acc += xp[i] * xj[i];
                sl[t] = acc;
              }
            }
            __syncthreads();
            if (row)                                // thread (r, sub): row r of every other vector
              for (int j = sub; j < m; j += 2)
                if (pos[j] == round && !fin[j]) {
                  double acc = 0.0;
                  for (int q = j - round; q < j; ++q) acc += sl[q] * S[r + q * LD];
                  S[r + j * LD] -= acc;
                }
          }
        }
        __syncthreads();
      }
      if (mine && !done) {
        xmax = 0.0;
        if constexpr (LAY::rows) {
          for (int i0 = 0; i0 < n; i0 += 8) {
            double v8[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v8[q] = fabs(x[min(i0 + q, n - 1) * XS]);   // a repeated last entry is no new maximum
#pragma unroll
            for (int q = 0; q < 8; ++q)
              if (v8[q] > xmax) { xmax = v8[q]; jmax = min(i0 + q, n - 1); }
          }
        } else {
          for (int i = 0; i < n; ++i) {
            const double v = fabs(x[i]);
            if (v > xmax) { xmax = v; jmax = i; }
          }
        }
        if (xmax >= dtpcrt) ++nrmchk;              // DSTEIN's growth test, then kExtra more solves
        if (nrmchk >= kExtra + 1) done = 1;
        else if (it + 1 >= kMaxIts && nrmchk == 0) { done = 1; failed = 1; }
        else if (!(xmax > 0.0)) { done = 1; failed = 1; }   // a zero or non-finite iterate cannot be scaled
        if (done) {
          double ss = 0.0;
          if constexpr (LAY::rows) {                // the same sums and products, eight entries' loads ahead
            for (int i0 = 0; i0 < n; i0 += 8) {
              double v8[8];
#pragma unroll
              for (int q = 0; q < 8; ++q) v8[q] = x[min(i0 + q, n - 1) * XS];
#pragma unroll
              for (int q = 0; q < 8; ++q)
                if (i0 + q < n) ss += v8[q] * v8[q];
            }
            double scl = 1.0 / sqrt(ss);
            if (x[jmax * XS] < 0.0) scl = -scl;
            for (int i0 = 0; i0 < n; i0 += 8) {
              double v8[8];
#pragma unroll
              for (int q = 0; q < 8; ++q) v8[q] = x[min(i0 + q, n - 1) * XS];
#pragma unroll
              for (int q = 0; q < 8; ++q)
                if (i0 + q < n) x[(i0 + q) * XS] = v8[q] * scl;
            }
          } else {
            for (int i = 0; i < n; ++i) ss += x[i] * x[i];
            double scl = 1.0 / sqrt(ss);
            if (x[jmax] < 0.0) scl = -scl;
            for (int i = 0; i < n; ++i) x[i] *= scl;
          }
          fin[t] = 1;
        }
      }
      if (__syncthreads_and(!mine || done)) break;  // every vector of the round is finished
    }
    if (mine && !done) failed = 1;
  }
  if (lane) fin[t] = failed;
  if (__syncthreads_or(failed)) {
    if (t == 0) {
      int k = 0;
      while (k < m && !fin[k]) ++k;
      *mword = 0;
      *info = 200000 + first + k;
    }
    return false;
  }
  return true;
}

}  // namespace bwindow
}  // namespace ek
