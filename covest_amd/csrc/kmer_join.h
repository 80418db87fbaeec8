// kmer_join.h -- the cell arithmetic of the join of two k-mer tables (kmer_join.hip, abi_join.cpp; DESIGN.md section
// 6am) in plain C++: the clip of a count to a row or a column, the rectangle of low cells a workgroup keeps in LDS, the
// flat index of a cell and the bound on the matrix.  No HIP in it: the kernel and tests/join_cells_check.cpp (the host
// compiler's sanitizers) compile this very source.
//
// out[i][j], row-major n_rows x n_cols, is the number of keys x held by at least one of the tables A and B with
// min(a(x), n_rows - 1) == i and min(b(x), n_cols - 1) == j; a(x), b(x) the counts the tables hold, 0 for a key not held.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define KMER_JOIN_HD __host__ __device__
#else
#define KMER_JOIN_HD
#endif

namespace covest {
namespace kmer_join {

constexpr int64_t kMaxCells = (int64_t)1 << 22; // n_rows * n_cols at most: 32 MiB of int64

// The cells i < kLdsRows, j < kLdsCols have a bin of their own in every workgroup (16 KB of 32-bit bins, what
// kmer_histogram_kernel takes): read abundances up to a few times the coverage against the copy numbers of all but
// the longest repeats.  In a real spectrum nearly every key falls here.
constexpr int kLdsRows = 256, kLdsCols = 16;
constexpr int kLdsBins = kLdsRows * kLdsCols;

// n_rows, n_cols >= 1 and n_rows * n_cols <= kMaxCells, without forming a product that could overflow
KMER_JOIN_HD inline bool cells_ok(int64_t n_rows, int64_t n_cols)
{
    return n_rows >= 1 && n_cols >= 1 && n_rows <= kMaxCells && n_cols <= kMaxCells / n_rows;
}

// the row (column) of a count in a matrix of n (>= 1) rows (columns): the last one takes every count from n - 1 on
KMER_JOIN_HD inline uint32_t clip(unsigned long long count, uint32_t n)
{
    return count < (unsigned long long)(n - 1u) ? (uint32_t)count : n - 1u;
}

KMER_JOIN_HD inline bool in_lds(uint32_t i, uint32_t j)
{
    return i < (uint32_t)kLdsRows && j < (uint32_t)kLdsCols;
}

// the bin of cell (i, j), in_lds(i, j), whatever the matrix's own width
KMER_JOIN_HD inline uint32_t lds_index(uint32_t i, uint32_t j)
{
    return i * (uint32_t)kLdsCols + j;
}

// the place of cell (i, j) in out: below n_rows * n_cols <= kMaxCells for i < n_rows, j < n_cols
KMER_JOIN_HD inline uint32_t flat_index(uint32_t i, uint32_t j, uint32_t n_cols)
{
    return i * n_cols + j;
}

} // namespace kmer_join
} // namespace covest
