// Host arithmetic of the assembly launches (kernels_post.hip): plain C++, no HIP types.  Which of the three dense writers a
// caller-owned (B, m, n) matrix gets, the 32-bit reciprocal of the flat stream, the block counts of the flat, per-problem,
// sparse and scatter launches, and the 64-bit reciprocal of the two streams over the structural non-zeros.
// tests/post_plan_check.cpp replays the kernels' index arithmetic against these on the CPU.
//
// The flat stream (post_flat_kernel) cuts the whole (B, m*n) output into blocks of kAsmBlock x kAsmVPT vectors of 16 bytes.
// A block divides exactly once (e_blk / mn, 64-bit) and every lane gets its problem by a multiply-high:
//     numer = r_blk + lane_vector * NV   (< mn + kAsmBlock * kAsmVPT * NV),   db = umulhi(numer, magic),   magic = ceil(2^32 / mn)
// With err = magic * mn - 2^32 (< mn), db = floor(numer / mn + numer * err / (mn * 2^32)), which is floor(numer / mn) whenever
// numer * err < 2^32: the quotient's fractional part is at most 1 - 1/mn and the excess stays below 1/mn.
#pragma once

#include <cstdint>

namespace nempc {

constexpr int kAsmVPT = 4;        // 16-byte vectors per lane
constexpr int kAsmBlock = 256;    // lanes per workgroup of every assembly launch

// dense writer of the handle's most recent nempc_eval (nempc_last_dense_writer)
enum DenseWriter {
    DENSE_WRITER_NONE = 0,        // no dense matrix asked for
    DENSE_WRITER_ROWS = 1,        // the row launch wrote it (fused fixed-shape launch, rows_coop_kernel+dense)
    DENSE_WRITER_ASSEMBLE = 2,    // assemble_dense_kernel (per-problem grid, no objective)
    DENSE_WRITER_POST = 3,        // post_kernel (per-problem grid + objective blocks)
    DENSE_WRITER_FLAT = 4,        // post_flat_kernel (with or without the objective blocks)
    DENSE_WRITER_SCATTER = 5,     // post_scatter_kernel (resident matrix: the structural non-zeros alone)
};

// why the flat stream is not used; tested in this order
enum PostFlatRefusal {
    POST_FLAT_OK = 0,
    POST_FLAT_RAGGED = 1,         // m*n is not a whole number of 16-byte vectors: a vector would straddle two problems
    POST_FLAT_MISALIGNED = 2,     // the matrix does not start on a 16-byte boundary
    POST_FLAT_TOO_LARGE = 3,      // B * m*n >= 2^32: problem index and numerators are 32-bit
    POST_FLAT_INEXACT = 4,        // the 32-bit reciprocal is not exact for every numerator a block can form
};

inline unsigned post_vec_elems(unsigned esz) { return 16u / esz; }                       // NV: elements per 16-byte vector
inline unsigned post_block_elems(unsigned esz) { return (unsigned)(kAsmBlock * kAsmVPT) * post_vec_elems(esz); }

// Can post_flat_kernel write B problems of mn elements of esz bytes at `jac`?  POST_FLAT_OK: *magic = ceil(2^32 / mn).
inline PostFlatRefusal post_flat_plan(unsigned mn, int B, unsigned esz, const void* jac, unsigned* magic) {
    const unsigned NV = post_vec_elems(esz);
    if (mn == 0 || mn % NV != 0) return POST_FLAT_RAGGED;
    if ((reinterpret_cast<uintptr_t>(jac) & 15) != 0) return POST_FLAT_MISALIGNED;
    if ((unsigned long long)B * mn >= (1ull << 32)) return POST_FLAT_TOO_LARGE;
    const unsigned long long mg = ((1ull << 32) + mn - 1) / mn;
    const unsigned long long err = mg * mn - (1ull << 32);          // < mn
    const unsigned long long max_numer = (unsigned long long)mn + post_block_elems(esz);
    if (mg >= (1ull << 32) || err * max_numer >= (1ull << 32)) return POST_FLAT_INEXACT;
    *magic = (unsigned)mg;
    return POST_FLAT_OK;
}

// blocks of the flat stream over B * mn elements
inline int post_flat_blocks(unsigned mn, int B, unsigned esz) {
    const long long per = post_block_elems(esz), total = (long long)B * mn;
    return (int)((total + per - 1) / per);
}

// blocks per problem of the per-problem grid (assemble_dense_kernel, post_kernel: grid.y = B)
inline int post_problem_blocks(unsigned mn, unsigned esz) {
    const long long per = post_block_elems(esz);
    return (int)(((long long)mn + per - 1) / per);
}

// objective blocks behind a flat / sparse / scatter stream: one problem per wave, four waves per block
inline int post_objective_blocks(int B) { return (B + 3) / 4; }

// blocks of the streams over the structural non-zeros (post_sparse_kernel, post_scatter_kernel): one element per lane
inline int post_nnz_blocks(int nnz, int B) {
    const unsigned long long total = (unsigned long long)B * (unsigned long long)nnz;
    return (int)((total + kAsmBlock - 1) / kAsmBlock);
}

// magic64 = ceil(2^64 / nnz): umul64hi(e, magic64) == e / nnz for e * nnz < 2^64 (the excess e * err / (nnz * 2^64), err < nnz,
// stays below 1 / nnz).  false: nnz < 2 -- ceil(2^64 / 1) does not fit 64 bits (the expression wraps to 0, which would put
// every element into problem 0), and no pattern has fewer than two entries: every row has its -1 and a control column.
inline bool post_recip64(int nnz, unsigned long long* magic64) {
    if (nnz < 2) return false;
    *magic64 = ~0ull / (unsigned long long)nnz + 1;
    return true;
}

}  // namespace nempc
