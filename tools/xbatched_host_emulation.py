#!/usr/bin/env python3
"""ek_batched_x.hip's kernel on the CPU: the kernel's source, unchanged, compiled for the host with one OS thread per GPU
thread, __syncthreads() as a barrier and __shared__ as static storage; one problem per run (tools, not product).

  python tools/xbatched_host_emulation.py [--n 129] [--problem 1] [--tsan] [--stop 0|1|2]
      --tsan   build with -fsanitize=thread: a missing barrier shows as a data race with both source lines
      --stop   1: end after X = L^-1 A and compare the image with a forward substitution's X^T; 2: after stage 2 (C)

--stop compares bit for bit (the reference applies the same updates in the same order) and exits 1 on a difference.
Prints info, residual and (B-)orthogonality against their bounds and whether the NaNs planted in the strict upper
triangles of A and B survived; exit status 0 when all hold.  Needs g++ with C++20 (std::barrier).  The butterfly of
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
ap.add_argument("--tsan", action="store_true")
ap.add_argument("--stop", type=int, default=0)
args = ap.parse_args()
src = open(os.path.join(ROOT, "eigenkernel_amd", "csrc", "ek_batched_x.hip")).read()
def patch(text, old, new):
    assert text.count(old) == 1, "anchor not found exactly once in ek_batched_x.hip: %r" % old
    return text.replace(old, new)


src = src[:src.index("// the images: grown")]
hdr = r'''
#include <barrier>
#include <thread>
#include <vector>
#include <cmath>
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#define EK_HIP_XBATCH_NMAX 256
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__ static
struct Idx { int x; };
static thread_local Idx threadIdx, blockIdx;
static std::barrier<> *g_bar;
static double g_xch[512]; static int g_or;
static inline void __syncthreads() { g_bar->arrive_and_wait(); }
static inline int __syncthreads_or(int v) { if (threadIdx.x == 0) g_or = 0; g_bar->arrive_and_wait(); if (v) __atomic_store_n(&g_or, 1, __ATOMIC_RELAXED); g_bar->arrive_and_wait(); int r = g_or; g_bar->arrive_and_wait(); return r; }
static inline double __shfl_xor(double x, int o, int) { g_xch[threadIdx.x] = x; g_bar->arrive_and_wait(); double y = g_xch[threadIdx.x ^ o]; g_bar->arrive_and_wait(); return y; }
static inline double __builtin_amdgcn_rsq(double h) { return 1.0 / std::sqrt(h); }
using std::min;
static int g_stop2 = 0;
'''
src = patch(src, '#include "ek_api_internal.h"', hdr)
src = patch(src, "typedef __attribute__((address_space(1))) double gdouble;", "typedef double gdouble;")
src = patch(src, "  // ---- 3: Householder", "  if (g_stop2) return;\n  // ---- 3: Householder")
src = patch(src, "    // the lower half of X the right way round", "    if (g_stop2 == 1) return;\n    // the lower half of X the right way round")
src += r'''
}  // namespace batchedx
}  // namespace ek
using namespace ek::batchedx;
int main(int argc, char **argv) {
  const int n = argc > 1 ? atoi(argv[1]) : 129, problem = argc > 2 ? atoi(argv[2]) : 1;
  std::vector<double> A((size_t)n * n), B((size_t)n * n), Z((size_t)n * n, -7.0), w(n, -7.0), ws(kSlot, NAN);
  unsigned long long s = 12345 + n;
  auto rnd = [&]() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return ((double)(s >> 11) / 9007199254740992.0) * 2.0 - 1.0; };
  for (int j = 0; j < n; ++j)
    for (int i = 0; i < n; ++i) {
      if (i < j) { A[i + (size_t)j * n] = NAN; B[i + (size_t)j * n] = NAN; continue; }   // the upper triangles are never read
      A[i + (size_t)j * n] = rnd();
      B[i + (size_t)j * n] = (i == j) ? 2.0 + 0.5 * rnd() : rnd() / n;
    }
  std::vector<double> A0 = A, B0 = B;
  int info = 777;
  Args a{problem, 1, n, A.data(), n, (long long)n * n, B.data(), n, (long long)n * n, w.data(), Z.data(), n, (long long)n * n, &info, ws.data()};
  g_stop2 = getenv("STOP2") ? atoi(getenv("STOP2")) : 0;
  std::barrier<> bar(T);
  g_bar = &bar;
  std::vector<std::thread> th;
  for (int t = 0; t < T; ++t) th.emplace_back([&, t]() { threadIdx.x = t; blockIdx.x = 0; xbatched_kernel(a); });
  for (auto &x : th) x.join();
  if (g_stop2) {
    // C = L^-1 A L^-T from the L left in B
    std::vector<double> X((size_t)n * n), C((size_t)n * n);
    auto Lf = [&](int i, int j) { return B[i + (size_t)j * n]; };
    auto a00 = [&](int i, int j) { return i >= j ? A0[i + (size_t)j * n] : A0[j + (size_t)i * n]; };
    for (int c = 0; c < n; ++c) for (int i = 0; i < n; ++i) { double v = a00(i, c); for (int k = 0; k < i; ++k) v -= Lf(i, k) * X[k + (size_t)c * n]; X[i + (size_t)c * n] = v / Lf(i, i); }
    for (int r = 0; r < n; ++r) for (int j = 0; j < n; ++j) { double v = X[r + (size_t)j * n]; for (int k = 0; k < j; ++k) v -= Lf(j, k) * C[r + (size_t)k * n]; C[r + (size_t)j * n] = v / Lf(j, j); }
    if (g_stop2 == 1) for (int j = 0; j < n; ++j) for (int i = 0; i < n; ++i) C[i + (size_t)j * n] = X[j + (size_t)i * n];
    double worst = 0; int wi = -1, wj = -1, bad = 0;
    for (int j = 0; j < n; ++j) for (int i = 0; i < n; ++i) { if (g_stop2 == 2 && i < j) continue; double e = std::fabs(ws[i + (size_t)j * LD] - C[i + (size_t)j * n]); if (e != 0.0) ++bad; if (e > worst) { worst = e; wi = i; wj = j; } }
    printf("%s: worst |image - reference| = %.3e at (%d, %d), %d entries differ in their bits\n", g_stop2 == 1 ? "after X = L^-1 A (all entries, against X^T)" : "after stage 2 (lower triangle, against C)", worst, wi, wj, bad);
    int shown = 0;
    for (int j = 0; j < n && shown < 12; ++j) for (int i = 0; i < n && shown < 12; ++i) if (!(g_stop2 == 2 && i < j) && ws[i + (size_t)j * LD] != C[i + (size_t)j * n]) { printf("  (%d, %d): %.6e vs %.6e\n", i, j, ws[i + (size_t)j * LD], C[i + (size_t)j * n]); ++shown; }
    return bad ? 1 : 0;
  }
  // residual and orthogonality on the host
  auto a0 = [&](int i, int j) { return i >= j ? A0[i + (size_t)j * n] : A0[j + (size_t)i * n]; };
  auto b0 = [&](int i, int j) { if (!problem) return i == j ? 1.0 : 0.0; return i >= j ? B0[i + (size_t)j * n] : B0[j + (size_t)i * n]; };
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
open(cpp, "w").write(src)
flags = ["-O1", "-g", "-fsanitize=thread"] if args.tsan else ["-O2"]
subprocess.check_call(["g++", "-std=c++20", "-pthread", "-ffp-contract=off"] + flags + [cpp, "-o", exe])
env = dict(os.environ)
if args.stop:
    env["STOP2"] = str(args.stop)
if args.tsan:
    env.setdefault("TSAN_OPTIONS", "halt_on_error=1 history_size=4")
sys.exit(subprocess.call([exe, str(args.n), str(args.problem)], env=env))
