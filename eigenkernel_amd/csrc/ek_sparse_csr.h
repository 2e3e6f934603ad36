// ek_sparse_csr.h -- canonical form of the reference's triplet lists (ek_sparse_mat_t, matrix_io.f90:11-15): the CSR of
// the mirrored symmetric matrix.  Plain C++ (no HIP): libek_hip.so builds it on the host before anything is uploaded,
// and tools/sparse_csr_sweep.cpp compiles it for the CPU alone.
//
//   in : n, nnz, suffix = the memory of the Fortran suffix(2, nnz): interleaved 1-based (i_k, j_k), value(nnz)
//   out: entry k contributes (i, j) and, when i != j, (j, i) -- either triangle may appear in the list; rows by a
//        counting sort, columns ascending inside a row; of the entries that name the same unordered pair {i, j} the LAST
//        of the list survives, as in the reference's serial pdelset loop (distribute_matrix.f90:411-418), where a later
//        assignment overwrites an earlier one in both triangles.
// The result depends on the set of surviving entries alone, not on their order in the list.  Values are not looked at
// (NaN and Inf pass through).
#pragma once
#include <algorithm>
#include <utility>
#include <vector>

namespace ek {
namespace sparse {

struct Csr {
  long long n = 0;
  std::vector<long long> rowptr;   // n + 1
  std::vector<int> col;            // 0-based, ascending inside a row
  std::vector<double> val;
  long long nnz() const { return rowptr.empty() ? 0 : rowptr.back(); }
};

// 0 when every index lies in 1 .. n, else the 1-based position in the list of the first entry that does not
inline long long first_bad_index(long long n, long long nnz, const int *suffix) {
  for (long long k = 0; k < nnz; ++k) {
    const long long i = suffix[2 * k], j = suffix[2 * k + 1];
    if (i < 1 || i > n || j < 1 || j > n) return k + 1;
  }
  return 0;
}

// the sort's arrays, for a caller that builds again and again and would rather not fault their pages in every time
struct Item { int row, col; long long k; };       // k: the position in the list
struct Scratch {
  std::vector<long long> start, fill;
  std::vector<Item> by_col, by_row;
};

// Returns 0, or the value of first_bad_index (out is then left empty).  May throw std::bad_alloc.  out and scratch keep
// their capacity from one call to the next.
inline long long build_csr(long long n, long long nnz, const int *suffix, const double *value, Csr &out,
                           Scratch *scratch = nullptr) {
  out.n = 0; out.rowptr.clear(); out.col.clear(); out.val.clear();
  const long long bad = first_bad_index(n, nnz, suffix);
  if (bad) return bad;
  Scratch local;
  Scratch &sc = scratch ? *scratch : local;
  out.n = n;
  // Two stable counting sorts of the mirrored entries, no comparison: by column, then by row.  The mirrored set is
  // symmetric, so an index owns as many entries as a column as it does as a row: one table of starts serves both.
  std::vector<long long> &start = sc.start, &fill = sc.fill;
  std::vector<Item> &by_col = sc.by_col, &by_row = sc.by_row;
  start.assign((size_t)n + 1, 0);
  for (long long k = 0; k < nnz; ++k) {
    const int i = suffix[2 * k] - 1, j = suffix[2 * k + 1] - 1;
    ++start[(size_t)i + 1];
    if (i != j) ++start[(size_t)j + 1];
  }
  for (long long r = 0; r < n; ++r) start[(size_t)r + 1] += start[(size_t)r];
  const size_t total = (size_t)start[(size_t)n];
  by_col.resize(total);
  by_row.resize(total);
  fill.assign(start.begin(), start.end() - 1);
  for (long long k = 0; k < nnz; ++k) {
    const int i = suffix[2 * k] - 1, j = suffix[2 * k + 1] - 1;
    by_col[(size_t)fill[(size_t)j]++] = Item{i, j, k};
    if (i != j) by_col[(size_t)fill[(size_t)i]++] = Item{j, i, k};
  }
  std::copy(start.begin(), start.end() - 1, fill.begin());
  for (size_t p = 0; p < total; ++p) by_row[(size_t)fill[(size_t)by_col[p].row]++] = by_col[p];
  // a row now holds ascending columns, equal columns in the order of the list: the last of a run is the survivor
  out.rowptr.assign((size_t)n + 1, 0);
  out.col.resize(total);
  out.val.resize(total);
  size_t at = 0;
  for (long long r = 0; r < n; ++r) {
    const size_t e = (size_t)start[(size_t)r + 1];
    for (size_t p = (size_t)start[(size_t)r]; p < e; ++p) {
      if (p + 1 < e && by_row[p + 1].col == by_row[p].col) continue;
      out.col[at] = by_row[p].col;
      out.val[at++] = value[by_row[p].k];
    }
    out.rowptr[(size_t)r + 1] = (long long)at;
  }
  out.col.resize(at);
  out.val.resize(at);
  return 0;
}

}  // namespace sparse
}  // namespace ek
