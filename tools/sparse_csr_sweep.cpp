// tools/sparse_csr_sweep.cpp -- the canonical form of a triplet list (eigenkernel_amd/csrc/ek_sparse_csr.h: the CSR of
// the mirrored symmetric matrix) on random lists and on the edge cases of tests/test_sparse_host.py, each held against
// a dense loop that does what the reference's serial pdelset loop does (distribute_matrix.f90:411-418).  The header is
// plain C++: this program needs no HIP and no GPU, and is meant for a build with a sanitizer, on the CPU:
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all \
//           -Ieigenkernel_amd/csrc tools/sparse_csr_sweep.cpp -o /tmp/sparse_csr_sweep && /tmp/sparse_csr_sweep
// Prints the number of lists and a checksum of their CSRs; exits 1 at the first disagreement.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <vector>

#include "ek_sparse_csr.h"

namespace {
uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint64_t next() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return g_state; }

uint64_t g_sum = 0;
long long g_lists = 0;

bool check(long long n, const std::vector<int> &suf, const std::vector<double> &val, const char *what) {
  const long long nnz = (long long)val.size();
  ek::sparse::Csr c;
  if (ek::sparse::build_csr(n, nnz, suf.data(), val.data(), c) != 0) { printf("%s: unexpected index error\n", what); return false; }
  std::vector<double> M((size_t)(n * n), 0.0);
  std::vector<char> P((size_t)(n * n), 0);
  for (long long k = 0; k < nnz; ++k) {
    const long long i = suf[2 * k] - 1, j = suf[2 * k + 1] - 1;
    M[(size_t)(i + j * n)] = M[(size_t)(j + i * n)] = val[(size_t)k];
    P[(size_t)(i + j * n)] = P[(size_t)(j + i * n)] = 1;
  }
  long long at = 0;
  if ((long long)c.rowptr.size() != n + 1 || c.rowptr[0] != 0) { printf("%s: rowptr\n", what); return false; }
  for (long long i = 0; i < n; ++i) {
    for (long long j = 0; j < n; ++j) {
      if (!P[(size_t)(i + j * n)]) continue;
      if (at >= c.nnz() || c.col[(size_t)at] != j || memcmp(&c.val[(size_t)at], &M[(size_t)(i + j * n)], 8) != 0) {
        printf("%s: row %lld column %lld\n", what, i, j);
        return false;
      }
      uint64_t bits; memcpy(&bits, &c.val[(size_t)at], 8);
      g_sum = g_sum * 1099511628211ull + bits + (uint64_t)j;
      ++at;
    }
    if (c.rowptr[(size_t)i + 1] != at) { printf("%s: end of row %lld\n", what, i); return false; }
  }
  ++g_lists;
  return true;
}
}  // namespace

int main() {
  // the cases of the host suite
  if (!check(5, {1, 1, 3, 1, 2, 4, 5, 5, 4, 5, 1, 5}, {2.0, -1.0, 0.5, 7.0, -0.0, 3.0}, "both triangles")) return 1;
  if (!check(4, {2, 3, 1, 1, 3, 2, 4, 4, 2, 3, 1, 1}, {1.0, 4.0, 2.0, 1.0, 3.0, 5.0}, "a pair three times")) return 1;
  {
    std::vector<int> suf; std::vector<double> val;
    for (int j = 1; j <= 7; ++j) if (j != 5) { suf.push_back(3); suf.push_back(j); val.push_back(j); }
    if (!check(7, suf, val, "a full and an empty row")) return 1;
  }
  if (!check(7, {}, {}, "an empty list")) return 1;
  if (!check(0, {}, {}, "order 0")) return 1;
  if (!check(1, {1, 1, 1, 1}, {1.0, 2.0}, "order 1")) return 1;
  for (int bad = 0; bad < 4; ++bad) {          // an index 0 and an index n + 1, in either position
    const int n = 6;
    std::vector<int> suf = {1, 1, 2, 3, 6, 6};
    suf[2 + (bad & 1)] = (bad & 2) ? n + 1 : 0;
    const std::vector<double> val = {1.0, 2.0, 3.0};
    ek::sparse::Csr c;
    if (ek::sparse::build_csr(n, 3, suf.data(), val.data(), c) != 2 || !c.rowptr.empty()) { printf("index error not reported\n"); return 1; }
  }
  // random lists: duplicates, both triangles, diagonal entries, from nearly empty to several times full
  for (int round = 0; round < 4000; ++round) {
    const long long n = 1 + (long long)(next() % 48);
    const long long nnz = (long long)(next() % (uint64_t)(3 * n * n + 1));
    std::vector<int> suf((size_t)(2 * nnz)); std::vector<double> val((size_t)nnz);
    for (long long k = 0; k < nnz; ++k) {
      suf[(size_t)(2 * k)] = 1 + (int)(next() % (uint64_t)n);
      suf[(size_t)(2 * k + 1)] = 1 + (int)(next() % (uint64_t)n);
      val[(size_t)k] = (double)(int64_t)(next() % 2001) - 1000.0;
    }
    if (!check(n, suf, val, "random")) return 1;
    // a permuted duplicate-free list of the survivors gives the identical CSR
    ek::sparse::Csr c;
    (void)ek::sparse::build_csr(n, nnz, suf.data(), val.data(), c);
    std::vector<int> s2; std::vector<double> v2;
    for (long long i = 0; i < n; ++i)
      for (long long k = c.rowptr[(size_t)i]; k < c.rowptr[(size_t)i + 1]; ++k)
        if (c.col[(size_t)k] <= i) {
          const bool flip = next() & 1;
          s2.push_back(flip ? c.col[(size_t)k] + 1 : (int)i + 1); s2.push_back(flip ? (int)i + 1 : c.col[(size_t)k] + 1);
          v2.push_back(c.val[(size_t)k]);
        }
    std::vector<size_t> perm(v2.size());
    std::iota(perm.begin(), perm.end(), (size_t)0);
    for (size_t k = perm.size(); k > 1; --k) std::swap(perm[k - 1], perm[(size_t)(next() % k)]);
    std::vector<int> s3(s2.size()); std::vector<double> v3(v2.size());
    for (size_t k = 0; k < perm.size(); ++k) { s3[2 * k] = s2[2 * perm[k]]; s3[2 * k + 1] = s2[2 * perm[k] + 1]; v3[k] = v2[perm[k]]; }
    ek::sparse::Csr d;
    (void)ek::sparse::build_csr(n, (long long)v3.size(), s3.data(), v3.data(), d);
    if (d.rowptr != c.rowptr || d.col != c.col || d.val != c.val) { printf("a permuted list gave another CSR\n"); return 1; }
  }
  printf("%lld lists, checksum %llu\n", g_lists, (unsigned long long)g_sum);
  return 0;
}
