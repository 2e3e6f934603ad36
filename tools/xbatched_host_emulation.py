#!/usr/bin/env python3
"""ek_batched_x.hip's kernel on the CPU: the kernel's source, unchanged, compiled for the host with one OS thread per GPU
thread, __syncthreads() as a barrier and __shared__ as static storage; one problem per run (tools, not product).

  python tools/xbatched_host_emulation.py [--n 129] [--problem 1] [--itype 1|2|3] [--table] [--tsan] [--stop 0|1|2]
                                          [--window IL,IU | --vl X --vu Y] [--case random|all_equal] [--class 256|512]
      --class  512: the class of 512 rows and 1024 threads (ek_hip_*_ybatched*, orders 257 .. 512); it has
               the uniform instantiations alone, so no --table and no window.  1024 OS threads: slow above order 300
      --window the window instantiation (ek_hip_eigenpairs_window_xbatched*): the pairs IL .. IU (1-based)
               by stage 4W -- bisection, inverse iteration on the rows of the image -- and stage 5 on those rows
      --vl, --vu  the same by value: the pairs in (vl, vu]; a missing bound is infinite
      --case   all_equal: A = 3 B (problem 0: 3 I), one cluster of n, a round per wanted vector: the Gram-Schmidt maps
      --table  the kernel's table instantiation (ek_hip_*_xvbatched*): the problem as the one entry of a variable-order
               table, image slot 0, the status word at info[entry.index]; with --window or --vl / --vu the
               table-and-window instantiation (ek_hip_*_window_xvbatched*): the window in the entry of a second
               table, the count at m[entry.index], the LU slot at the entry's offset into a workspace of NaNs
      --itype  DSYGV's problem type (problem 1): 2 and 3 run the kernel's CONG instantiation; with
               --window or --vl / --vu the CONG instantiation of the window kernel (ek_hip_sygv_window_xbatched*,
               DESIGN.md 33), judged with the type's quantities on the window's m columns
      --tsan   build with -fsanitize=thread: a missing barrier shows as a data race with both source lines
      --stop   1: end after X = L^-1 A and compare the image with a forward substitution's X^T (type 1 only); 2: after
               stage 2 (C = L^-1 A L^-T; types 2 and 3: C = L^T A L formed by plain loops in the kernel's summation order)

--stop compares bit for bit (the reference applies the same updates in the same order) and exits 1 on a difference.
Prints info, residual and (B-)orthogonality against their bounds (types 2 and 3: the normalisations of the type, module
docstring of tests/test_gpu_sygv_batched.py, type 3 with the factor left in B) and whether the NaNs planted in the strict
upper triangles of A and B survived; exit status 0 when all hold.  Needs g++ with C++20 (std::barrier).  The butterfly of
block_reduce is ordered by barriers of the emulation's own, so this says nothing about that function."""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=129)
ap.add_argument("--problem", type=int, default=1)
ap.add_argument("--itype", type=int, default=1, choices=(1, 2, 3))
ap.add_argument("--table", action="store_true")
ap.add_argument("--tsan", action="store_true")
ap.add_argument("--stop", type=int, default=0)
ap.add_argument("--window", default=None)
ap.add_argument("--vl", type=float, default=None)
ap.add_argument("--vu", type=float, default=None)
ap.add_argument("--case", default="random", choices=("random", "all_equal"))
ap.add_argument("--class", dest="cls", type=int, default=256, choices=(256, 512))
args = ap.parse_args()
by_value = args.vl is not None or args.vu is not None
window = args.window is not None or by_value
assert not (args.window and by_value), "--window or --vl / --vu"
assert not window or not args.stop, "the window: --stop 0"
assert args.cls == 256 or not (window or args.table), "--class 512: the uniform call alone"
assert 0 < args.n <= args.cls, "--n within the class"
assert args.itype == 1 or (args.problem == 1 and args.stop != 1), "--itype 2|3: problem 1, and --stop 0 or 2"
CSRC = os.path.join(ROOT, "eigenkernel_amd", "csrc")
src = open(os.path.join(CSRC, "ek_batched_x.hip")).read()
def patch(text, old, new):
    assert text.count(old) == 1, "anchor not found exactly once in ek_batched_x.hip and its headers: %r" % old
    return text.replace(old, new)


src = src[:src.index("// the images: grown")]
# the two headers the kernel shares with ek_batched.hip, in place of their #include lines
stages = open(os.path.join(CSRC, "ek_batched_stages.h")).read().replace("#pragma once\n", "")
wind = open(os.path.join(CSRC, "ek_batched_window.h")).read().replace("#pragma once\n", "")
wind = patch(wind, '#include "ek_batched_stages.h"\n', "")
src = patch(src, '#include "ek_batched_window.h"\n', wind)
src = patch(src, '#include "ek_batched_stages.h"\n', stages)
# the table's entry, shared through ek_api_internal.h: the struct as it stands there
internal = open(os.path.join(ROOT, "eigenkernel_amd", "csrc", "ek_api_internal.h")).read()
assert internal.count("struct Desc {") == 1, "struct Desc not found exactly once in ek_api_internal.h"
desc = internal[internal.index("struct Desc {"):]
desc = desc[:desc.index("};") + 2]
assert internal.count("struct WDesc {") == 1, "struct WDesc not found exactly once in ek_api_internal.h"
wdesc = internal[internal.index("struct WDesc {"):]
desc += "\n" + wdesc[:wdesc.index("};") + 2]
hdr = r'''
#include <barrier>
#include <thread>
#include <vector>
#include <cmath>
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstdint>
#include <type_traits>
#define EK_HIP_XBATCH_NMAX 256
#define EK_HIP_YBATCH_NMAX 512
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __attribute__(x)                            // the occupancy attribute of the kernel: nothing for the host
#define __shared__ static
struct Idx { int x; };
static thread_local Idx threadIdx, blockIdx;
static std::barrier<> *g_bar;
static double g_xch[1024]; static int g_or;
static inline void __syncthreads() { g_bar->arrive_and_wait(); }
static inline int __syncthreads_or(int v) { if (threadIdx.x == 0) g_or = 0; g_bar->arrive_and_wait(); if (v) __atomic_store_n(&g_or, 1, __ATOMIC_RELAXED); g_bar->arrive_and_wait(); int r = g_or; g_bar->arrive_and_wait(); return r; }
static inline int __syncthreads_and(int v) { return !__syncthreads_or(!v); }
static std::barrier<> *g_pair[256];                 // stage 4W's bisection exchanges inside a pair of lanes, under a condition
static inline double __shfl_xor(double x, int o, int w) { if (w == 2) { std::barrier<> *b = g_pair[threadIdx.x >> 1]; g_xch[threadIdx.x] = x; b->arrive_and_wait(); double y = g_xch[threadIdx.x ^ o]; b->arrive_and_wait(); return y; } g_xch[threadIdx.x] = x; g_bar->arrive_and_wait(); double y = g_xch[threadIdx.x ^ o]; g_bar->arrive_and_wait(); return y; }
static inline double __builtin_amdgcn_rsq(double h) { return 1.0 / std::sqrt(h); }
using std::min;
using std::max;
static int g_stop2 = 0;
namespace ek { namespace batched { @DESC@ } }
'''.replace("@DESC@", desc)
src = patch(src, '#include "ek_api_internal.h"', hdr)
src = patch(src, "typedef __attribute__((address_space(1))) double gdouble;", "typedef double gdouble;")
src = patch(src, "typedef const __attribute__((address_space(1))) double cgdouble;", "typedef const double cgdouble;")
src = patch(src, "  // ---- 3: Householder", "  if (g_stop2) return;\n  // ---- 3: Householder")
src = patch(src, "    // the lower half of X the right way round", "    if (g_stop2 == 1) return;\n    // the lower half of X the right way round")
src += r'''
}  // namespace batchedx
}  // namespace ek
using namespace ek::batchedx;
using CL = @CLASS@;                                 // the class under test
int main(int argc, char **argv) {
  const int n = argc > 1 ? atoi(argv[1]) : 129, problem = argc > 2 ? atoi(argv[2]) : 1;
  const int itype = argc > 3 ? atoi(argv[3]) : 1;
  const bool cong = problem && itype != 1;
  std::vector<double> A((size_t)n * n), B((size_t)n * n), Z((size_t)n * n, -7.0), w(n, -7.0), ws(CL::kSlot, NAN);
  unsigned long long s = 12345 + n;
  auto rnd = [&]() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return ((double)(s >> 11) / 9007199254740992.0) * 2.0 - 1.0; };
  for (int j = 0; j < n; ++j)
    for (int i = 0; i < n; ++i) {
      if (i < j) { A[i + (size_t)j * n] = NAN; B[i + (size_t)j * n] = NAN; continue; }   // the upper triangles are never read
      A[i + (size_t)j * n] = rnd();
      B[i + (size_t)j * n] = (i == j) ? 2.0 + 0.5 * rnd() : rnd() / n;
    }
  const bool all_equal = argc > 10 && atoi(argv[10]);
  if (all_equal)                                      // A = 3 B (3 I): every eigenvalue is 3, one cluster of n
    for (int j = 0; j < n; ++j)
      for (int i = j; i < n; ++i) A[i + (size_t)j * n] = problem ? 3.0 * B[i + (size_t)j * n] : (i == j ? 3.0 : 0.0);
  std::vector<double> A0 = A, B0 = B;
  const bool table = argc > 4 && atoi(argv[4]);
  // the window: argv 5 .. 9 = range (-1: none), il, iu, vl, vu
  const int range = argc > 5 ? atoi(argv[5]) : -1;
  if (range >= 0) {
    const int il = atoi(argv[6]), iu = atoi(argv[7]);
    const double vl = atof(argv[8]), vu = atof(argv[9]);
    const int zcap = range ? n : iu - il + 1;
    int m = 777, winfo = 777;
    const size_t luoff = table ? 1000 : 0;             // the table form: a slot that does not start at the workspace's base
    std::vector<double> lu(luoff + (size_t)5 * n * zcap, NAN);
    int ms[3] = {777, 777, 777}, winfos[3] = {777, 777, 777};
    Desc wd{A.data(), problem ? B.data() : nullptr, w.data(), Z.data(), n, n, n, n, 2, 0};
    ek::batched::WDesc ww{vl, vu, il, iu, zcap, zcap, (long long)luoff};
    XVWArgs xvw{problem, 1, &wd, &ww, winfos, ms, ws.data(), lu.data(), range, itype};
    XWArgs xw{{problem, 1, n, A.data(), n, (long long)n * n, B.data(), n, (long long)n * n, w.data(), Z.data(), n, (long long)n * n, &winfo, ws.data(), itype},
              {range, il, iu, zcap, vl, vu, &m, lu.data(), zcap}};
    std::barrier<> wbar(ClassX::T);
    g_bar = &wbar;
    for (int q = 0; q < 256; ++q) g_pair[q] = new std::barrier<>(2);
    std::vector<std::thread> wth;
    for (int t = 0; t < ClassX::T; ++t) wth.emplace_back([&, t]() { threadIdx.x = t; blockIdx.x = 0; if (table) { if (cong) xbatched_kernel<true>(xvw); else xbatched_kernel<false>(xvw); } else if (cong) xbatched_kernel<true>(xw); else xbatched_kernel<false>(xw); });
    for (auto &x : wth) x.join();
    if (table) {
      m = ms[2]; winfo = winfos[2];
      bool own = ms[0] == 777 && ms[1] == 777 && winfos[0] == 777 && winfos[1] == 777;
      for (size_t q = 0; q < luoff; ++q) own = own && std::isnan(lu[q]);
      if (!own) { printf("a word outside the entry's index, or the workspace in front of the entry's LU slot, was written\n"); return 1; }
    }
    auto a0 = [&](int i, int j) { return i >= j ? A0[i + (size_t)j * n] : A0[j + (size_t)i * n]; };
    auto b0 = [&](int i, int j) { if (!problem) return i == j ? 1.0 : 0.0; return i >= j ? B0[i + (size_t)j * n] : B0[j + (size_t)i * n]; };
    if (winfo != 0 || m < 0 || m > zcap) { printf("n=%d window: info=%d m=%d\n", n, winfo, m); return 1; }
    double res = 0, orth = 0, wmax = 0; bool asc = true, rest = true;
    if (cong) {
      // the quantities of the type on the m columns: |M z - w z|_2 / (max|A| |B|_2 |z|_2) with M = A B (2), B A (3);
      // max|Z^T B Z - I_m| (2), max|(L^-1 Z)^T (L^-1 Z) - I_m| (3) with the factor left in B
      std::vector<double> Y((size_t)n * std::max(m, 1)), x(n, 1.0), y(n), u(n), v(n);
      auto mul = [&](auto mat, const double *in, double *out) { for (int i = 0; i < n; ++i) { double sacc = 0; for (int j = 0; j < n; ++j) sacc += mat(i, j) * in[j]; out[i] = sacc; } };
      double amax = 0, bnorm = 0;
      for (int j = 0; j < n; ++j) for (int i = j; i < n; ++i) amax = std::max(amax, std::fabs(A0[i + (size_t)j * n]));
      for (int it = 0; it < 300; ++it) { mul(b0, x.data(), y.data()); bnorm = 0; for (int i = 0; i < n; ++i) bnorm += y[i] * y[i]; bnorm = std::sqrt(bnorm); for (int i = 0; i < n; ++i) x[i] = y[i] / bnorm; }
      for (int k = 0; k < m; ++k) {
        const double *z = &Z[(size_t)k * n];
        if (itype == 2) { mul(b0, z, u.data()); mul(a0, u.data(), v.data()); } else { mul(a0, z, u.data()); mul(b0, u.data(), v.data()); }
        double rn = 0, zn = 0;
        for (int i = 0; i < n; ++i) { const double d = v[i] - w[k] * z[i]; rn += d * d; zn += z[i] * z[i]; }
        res = std::max(res, std::sqrt(rn) / (amax * bnorm * std::sqrt(zn)));
        wmax = std::max(wmax, std::fabs(w[k])); if (k && w[k] < w[k - 1]) asc = false;
        if (range && !(w[k] > vl && w[k] <= vu)) asc = false;
        if (itype == 2) mul(b0, z, &Y[(size_t)k * n]);
        else for (int i = 0; i < n; ++i) { double sacc = z[i]; for (int j = 0; j < i; ++j) sacc -= B[i + (size_t)j * n] * Y[j + (size_t)k * n]; Y[i + (size_t)k * n] = sacc / B[i + (size_t)i * n]; }
      }
      for (int k = 0; k < m; ++k) for (int l = 0; l < m; ++l) {
        double sacc = 0;
        for (int i = 0; i < n; ++i) sacc += (itype == 2 ? Z[i + (size_t)k * n] : Y[i + (size_t)k * n]) * Y[i + (size_t)l * n];
        orth = std::max(orth, std::fabs(sacc - (k == l ? 1.0 : 0.0)));
      }
      for (int k = m; k < n; ++k) { rest = rest && w[k] == -7.0; for (int i = 0; i < n; ++i) rest = rest && Z[i + (size_t)k * n] == -7.0; }
      const double lim = 256 * n * 2.220446049250313e-16;
      printf("n=%d itype=%d window range=%d info=%d m=%d in order and inside=%d max|w|=%.3f residual %.3e (bound %.3e) orthogonality %.3e (bound %.3e)\n", n, itype, range, winfo, m, (int)asc, wmax, res, lim, orth, lim);
      bool upper = true; for (int j = 0; j < n; ++j) for (int i = 0; i < j; ++i) upper = upper && std::isnan(A[i + (size_t)j * n]) && std::isnan(B[i + (size_t)j * n]);
      printf("upper triangles untouched: %d; w and Z behind m untouched: %d\n", (int)upper, (int)rest);
      return (asc && res <= lim && orth <= lim && upper && rest && (range || m == iu - il + 1)) ? 0 : 1;
    }
    std::vector<double> BZ((size_t)n * std::max(m, 1));
    for (int k = 0; k < m; ++k) for (int i = 0; i < n; ++i) { double sacc = 0; for (int j = 0; j < n; ++j) sacc += b0(i, j) * Z[j + (size_t)k * n]; BZ[i + (size_t)k * n] = sacc; }
    for (int k = 0; k < m; ++k) {
      wmax = std::max(wmax, std::fabs(w[k])); if (k && w[k] < w[k - 1]) asc = false;
      if (range && !(w[k] > vl && w[k] <= vu)) asc = false;
      for (int i = 0; i < n; ++i) { double sacc = 0; for (int j = 0; j < n; ++j) sacc += a0(i, j) * Z[j + (size_t)k * n]; res = std::max(res, std::fabs(sacc - w[k] * BZ[i + (size_t)k * n])); }
      for (int l = 0; l < m; ++l) { double sacc = 0; for (int i = 0; i < n; ++i) sacc += Z[i + (size_t)k * n] * BZ[i + (size_t)l * n]; orth = std::max(orth, std::fabs(sacc - (k == l ? 1.0 : 0.0))); }
    }
    for (int k = m; k < n; ++k) { rest = rest && w[k] == -7.0; for (int i = 0; i < n; ++i) rest = rest && Z[i + (size_t)k * n] == -7.0; }
    const double eps = 2.220446049250313e-16, c = problem ? 256 : 64;
    printf("n=%d problem=%d window range=%d info=%d m=%d in order and inside=%d max|w|=%.3f residual %.3e (bound %.3e) orthogonality %.3e (bound %.3e)\n", n, problem, range, winfo, m, (int)asc, wmax, res, c * n * eps, orth, c * n * eps);
    bool upper = true; for (int j = 0; j < n; ++j) for (int i = 0; i < j; ++i) upper = upper && std::isnan(A[i + (size_t)j * n]) && std::isnan(B[i + (size_t)j * n]);
    printf("upper triangles untouched: %d; w and Z behind m untouched: %d\n", (int)upper, (int)rest);
    return (asc && res <= c * n * eps && orth <= c * n * eps && upper && rest && (range || m == iu - il + 1)) ? 0 : 1;
  }
  int infos[3] = {777, 777, 777};
  int &info = infos[table ? 2 : 0];                   // the table form: the status word of the entry's index
  Args a{problem, 1, n, A.data(), n, (long long)n * n, B.data(), n, (long long)n * n, w.data(), Z.data(), n, (long long)n * n, infos, ws.data(), itype};
  Desc d{A.data(), problem ? B.data() : nullptr, w.data(), Z.data(), n, n, n, n, 2, 0};
  XVArgs v{problem, 1, &d, infos, ws.data(), itype};
  g_stop2 = getenv("STOP2") ? atoi(getenv("STOP2")) : 0;
  std::barrier<> bar(CL::T);
  g_bar = &bar;
  std::vector<std::thread> th;
  for (int t = 0; t < CL::T; ++t) th.emplace_back([&, t]() { threadIdx.x = t; blockIdx.x = 0; if (table) { if (cong) xbatched_kernel<true>(v); else xbatched_kernel<false>(v); } else if (cong) xbatched_kernel<true, Args, CL>(a); else xbatched_kernel<false, Args, CL>(a); });
  for (auto &x : th) x.join();
  if (table && (infos[0] != 777 || infos[1] != 777)) { printf("a status word outside the entry's index was written\n"); return 1; }
  if (g_stop2) {
    // C = L^-1 A L^-T (types 2 and 3: L^T A L) from the L left in B
    std::vector<double> X((size_t)n * n), C((size_t)n * n);
    auto Lf = [&](int i, int j) { return B[i + (size_t)j * n]; };
    auto a00 = [&](int i, int j) { return i >= j ? A0[i + (size_t)j * n] : A0[j + (size_t)i * n]; };
    if (cong) {
      // a sum over k >= j: the terms j, j + 2, ... and j + 1, j + 3, ... each from 0.0 in ascending order, then added
      auto halves = [&](auto row, int j) { double p[2] = {0.0, 0.0}; for (int h = 0; h < 2; ++h) for (int k = j + h; k < n; k += 2) p[h] += row(k) * Lf(k, j); return p[0] + p[1]; };
      for (int r = 0; r < n; ++r) for (int j = 0; j < n; ++j) X[r + (size_t)j * n] = halves([&](int k) { return a00(r, k); }, j);      // Y = A L
      for (int r = 0; r < n; ++r) for (int i = 0; i <= r; ++i) C[r + (size_t)i * n] = halves([&](int k) { return X[k + (size_t)r * n]; }, i);   // C = Y^T L
    } else {
    for (int c = 0; c < n; ++c) for (int i = 0; i < n; ++i) { double v = a00(i, c); for (int k = 0; k < i; ++k) v -= Lf(i, k) * X[k + (size_t)c * n]; X[i + (size_t)c * n] = v / Lf(i, i); }
    for (int r = 0; r < n; ++r) for (int j = 0; j < n; ++j) { double v = X[r + (size_t)j * n]; for (int k = 0; k < j; ++k) v -= Lf(j, k) * C[r + (size_t)k * n]; C[r + (size_t)j * n] = v / Lf(j, j); }
    if (g_stop2 == 1) for (int j = 0; j < n; ++j) for (int i = 0; i < n; ++i) C[i + (size_t)j * n] = X[j + (size_t)i * n];
    }
    double worst = 0; int wi = -1, wj = -1, bad = 0;
    for (int j = 0; j < n; ++j) for (int i = 0; i < n; ++i) { if (g_stop2 == 2 && i < j) continue; double e = std::fabs(ws[i + (size_t)j * CL::LD] - C[i + (size_t)j * n]); if (e != 0.0) ++bad; if (e > worst) { worst = e; wi = i; wj = j; } }
    printf("%s: worst |image - reference| = %.3e at (%d, %d), %d entries differ in their bits\n", g_stop2 == 1 ? "after X = L^-1 A (all entries, against X^T)" : cong ? "after stage 2 (lower triangle, against L^T A L)" : "after stage 2 (lower triangle, against C)", worst, wi, wj, bad);
    int shown = 0;
    for (int j = 0; j < n && shown < 12; ++j) for (int i = 0; i < n && shown < 12; ++i) if (!(g_stop2 == 2 && i < j) && ws[i + (size_t)j * CL::LD] != C[i + (size_t)j * n]) { printf("  (%d, %d): %.6e vs %.6e\n", i, j, ws[i + (size_t)j * CL::LD], C[i + (size_t)j * n]); ++shown; }
    return bad ? 1 : 0;
  }
  // residual and orthogonality on the host
  auto a0 = [&](int i, int j) { return i >= j ? A0[i + (size_t)j * n] : A0[j + (size_t)i * n]; };
  auto b0 = [&](int i, int j) { if (!problem) return i == j ? 1.0 : 0.0; return i >= j ? B0[i + (size_t)j * n] : B0[j + (size_t)i * n]; };
  if (cong) {
    // the quantities of the type: |M z - w z|_2 / (max|A| |B|_2 |z|_2) with M = A B (2), B A (3); max|Z^T B Z - I| (2),
    // max|(L^-1 Z)^T (L^-1 Z) - I| (3) with the factor left in B
    std::vector<double> BZ((size_t)n * n), G((size_t)n * n), x(n, 1.0), y(n);
    auto mul = [&](auto m, const double *in, double *out) { for (int i = 0; i < n; ++i) { double sacc = 0; for (int j = 0; j < n; ++j) sacc += m(i, j) * in[j]; out[i] = sacc; } };
    double amax = 0, bnorm = 0, res = 0, orth = 0, wmax = 0; bool asc = true;
    for (int j = 0; j < n; ++j) for (int i = j; i < n; ++i) amax = std::max(amax, std::fabs(A0[i + (size_t)j * n]));
    for (int it = 0; it < 300; ++it) { mul(b0, x.data(), y.data()); bnorm = 0; for (int i = 0; i < n; ++i) bnorm += y[i] * y[i]; bnorm = std::sqrt(bnorm); for (int i = 0; i < n; ++i) x[i] = y[i] / bnorm; }
    for (int k = 0; k < n; ++k) {
      const double *z = &Z[(size_t)k * n];
      std::vector<double> u(n), v(n);
      if (itype == 2) { mul(b0, z, u.data()); mul(a0, u.data(), v.data()); } else { mul(a0, z, u.data()); mul(b0, u.data(), v.data()); }
      double rn = 0, zn = 0;
      for (int i = 0; i < n; ++i) { const double d = v[i] - w[k] * z[i]; rn += d * d; zn += z[i] * z[i]; }
      res = std::max(res, std::sqrt(rn) / (amax * bnorm * std::sqrt(zn)));
      wmax = std::max(wmax, std::fabs(w[k])); if (k && w[k] < w[k - 1]) asc = false;
      if (itype == 2) mul(b0, z, &BZ[(size_t)k * n]);
      else for (int i = 0; i < n; ++i) { double sacc = z[i]; for (int j = 0; j < i; ++j) sacc -= B[i + (size_t)j * n] * BZ[j + (size_t)k * n]; BZ[i + (size_t)k * n] = sacc / B[i + (size_t)i * n]; }
    }
    for (int k = 0; k < n; ++k) for (int l = 0; l < n; ++l) {
      double sacc = 0;
      for (int i = 0; i < n; ++i) sacc += (itype == 2 ? Z[i + (size_t)k * n] : BZ[i + (size_t)k * n]) * BZ[i + (size_t)l * n];
      orth = std::max(orth, std::fabs(sacc - (k == l ? 1.0 : 0.0)));
    }
    const double lim = 256 * n * 2.220446049250313e-16;
    printf("n=%d itype=%d info=%d ascending=%d max|w|=%.3f residual %.3e (bound %.3e) orthogonality %.3e (bound %.3e)\n", n, itype, info, (int)asc, wmax, res, lim, orth, lim);
    bool upper = true; for (int j = 0; j < n; ++j) for (int i = 0; i < j; ++i) upper = upper && std::isnan(A[i + (size_t)j * n]) && std::isnan(B[i + (size_t)j * n]);
    printf("upper triangles untouched: %d\n", (int)upper);
    return (info == 0 && asc && res <= lim && orth <= lim && upper) ? 0 : 1;
  }
  double res = 0, orth = 0, wmax = 0; bool asc = true;
  std::vector<double> BZ((size_t)n * n);
  for (int k = 0; k < n; ++k) for (int i = 0; i < n; ++i) { double sacc = 0; for (int j = 0; j < n; ++j) sacc += b0(i, j) * Z[j + (size_t)k * n]; BZ[i + (size_t)k * n] = sacc; }
  for (int k = 0; k < n; ++k) {
    wmax = std::max(wmax, std::fabs(w[k])); if (k && w[k] < w[k - 1]) asc = false;
    for (int i = 0; i < n; ++i) { double sacc = 0; for (int j = 0; j < n; ++j) sacc += a0(i, j) * Z[j + (size_t)k * n]; res = std::max(res, std::fabs(sacc - w[k] * BZ[i + (size_t)k * n])); }
    for (int l = 0; l < n; ++l) { double sacc = 0; for (int i = 0; i < n; ++i) sacc += Z[i + (size_t)k * n] * BZ[i + (size_t)l * n]; orth = std::max(orth, std::fabs(sacc - (k == l ? 1.0 : 0.0))); }
  }
  const double eps = 2.220446049250313e-16, c = problem ? 256 : 64;
  printf("n=%d problem=%d info=%d ascending=%d max|w|=%.3f residual %.3e (bound %.3e) orthogonality %.3e (bound %.3e)\n", n, problem, info, (int)asc, wmax, res, c * n * eps, orth, c * n * eps);
  // L L^T = B, upper triangles untouched
  bool upper = true; for (int j = 0; j < n; ++j) for (int i = 0; i < j; ++i) upper = upper && std::isnan(A[i + (size_t)j * n]) && std::isnan(B[i + (size_t)j * n]);
  printf("upper triangles untouched: %d\n", (int)upper);
  return (info == 0 && asc && res <= c * n * eps && orth <= c * n * eps && upper) ? 0 : 1;
}
'''
work = tempfile.mkdtemp(prefix="xbatched_emu_")
cpp, exe = os.path.join(work, "emu.cpp"), os.path.join(work, "emu")
open(cpp, "w").write(src.replace("@CLASS@", "ClassX" if args.cls == 256 else "ClassY"))
flags = ["-O1", "-g", "-fsanitize=thread"] if args.tsan else ["-O2"]
subprocess.check_call(["g++", "-std=c++20", "-pthread", "-ffp-contract=off"] + flags + [cpp, "-o", exe])
env = dict(os.environ)
if args.stop:
    env["STOP2"] = str(args.stop)
if args.tsan:
    env.setdefault("TSAN_OPTIONS", "halt_on_error=1 history_size=4")
argv = [exe, str(args.n), str(args.problem), str(args.itype), str(int(args.table))]
if window:
    il, iu = (int(x) for x in args.window.split(",")) if args.window else (0, 0)
    assert by_value or 1 <= il <= iu <= args.n, "--window IL,IU with 1 <= IL <= IU <= n"
    argv += [str(int(by_value)), str(il), str(iu), repr(-float("inf") if args.vl is None else args.vl),
             repr(float("inf") if args.vu is None else args.vu)]
else:
    argv += ["-1", "0", "0", "0", "0"]
argv.append(str(int(args.case == "all_equal")))
sys.exit(subprocess.call(argv, env=env))
