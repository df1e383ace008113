// Stand-alone check of the host arithmetic of the assembly launches (pyneuralempc_amd/csrc/post_plan.h: plain host code).
// Built and run by tests/test_post_plan_cpu.py with -fsanitize=address,undefined.  The kernels' index arithmetic
// (post_flat_kernel, post_sparse_kernel / post_scatter_kernel in kernels_post.hip) is replayed here in the same integer
// types, with the plan's magic numbers and block counts, against plain division.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "post_plan.h"

using namespace nempc;
typedef unsigned long long u64;

static long long failures = 0, checks = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        ++checks;                                                          \
        if (!(cond)) {                                                     \
            if (++failures <= 20) std::printf("line %d: %s\n", __LINE__, #cond); \
        }                                                                  \
    } while (0)

static unsigned umulhi(unsigned a, unsigned b) { return (unsigned)(((u64)a * b) >> 32); }
static u64 umul64hi(u64 a, u64 b) { return (u64)(((unsigned __int128)a * b) >> 64); }

alignas(16) static unsigned char arena[64];      // addresses only, never dereferenced

// the refusal the plan must give, restated from the four conditions with 128-bit arithmetic
static PostFlatRefusal expected(unsigned mn, u64 B, unsigned NV, const void* p) {
    if (mn % NV != 0) return POST_FLAT_RAGGED;
    if (reinterpret_cast<uintptr_t>(p) % 16 != 0) return POST_FLAT_MISALIGNED;
    if ((unsigned __int128)B * mn >= ((unsigned __int128)1 << 32)) return POST_FLAT_TOO_LARGE;
    const unsigned __int128 two32 = (unsigned __int128)1 << 32;
    const unsigned __int128 mg = (two32 + mn - 1) / mn;
    const unsigned __int128 err = mg * mn - two32;
    if (mg >= two32 || err * ((unsigned __int128)mn + 256u * 4u * NV) >= two32) return POST_FLAT_INEXACT;
    return POST_FLAT_OK;
}

// every numerator a block of post_flat_kernel can form: r_blk is a multiple of NV below mn (e_blk and mn both are), a lane
// adds (u * 256 + tid) * NV with u * 256 + tid < 256 * kAsmVPT -- all multiples of NV below mn + 256 * kAsmVPT * NV.
// -> number of wrong quotients or straddling vectors
static long long sweep_numerators(unsigned mn, unsigned NV, unsigned magic) {
    long long bad = 0;
    const unsigned limit = mn + (unsigned)(kAsmBlock * kAsmVPT) * NV;
    unsigned q = 0, r = 0;                        // numer = q * mn + r, kept without a division
    for (unsigned numer = 0; numer < limit; numer += NV) {
        const unsigned db = umulhi(numer, magic);
        const unsigned ee = numer - db * mn;
        bad += (db != q) | (ee != r) | (ee + NV > mn);
        r += NV;
        if (r >= mn) { r -= mn; ++q; }
    }
    return bad;
}

// the block loop of post_flat_kernel for one block, against plain 64-bit division.  -> wrong lanes
static long long replay_block(unsigned blk, unsigned mn, int B, unsigned NV, unsigned magic) {
    long long bad = 0;
    const u64 e_blk = (u64)blk * ((unsigned)(kAsmBlock * kAsmVPT) * NV);
    const unsigned b_blk = (unsigned)(e_blk / mn);
    const unsigned r_blk = (unsigned)(e_blk - (u64)b_blk * mn);
    for (unsigned lane = 0; lane < (unsigned)(kAsmBlock * kAsmVPT); ++lane) {
        const unsigned numer = r_blk + lane * NV;
        const unsigned db = umulhi(numer, magic);
        const unsigned ee = numer - db * mn;
        const unsigned bb = b_blk + db;
        const u64 e = e_blk + (u64)lane * NV;                 // the element this lane's vector starts at
        const bool inside = e < (u64)B * mn;
        bad += (bb < (unsigned)B) != inside;                  // the guard is exact
        if (inside) bad += (bb != e / mn) | (ee != e % mn) | (ee + NV > mn);
    }
    return bad;
}

// every block of the smallest B whose stream is longer than 200 blocks (small mn: many problems per block; large mn: many
// blocks per problem), the ragged last block included
static void replay_blocks(unsigned mn, unsigned esz, unsigned magic) {
    const unsigned per = post_block_elems(esz), NV = post_vec_elems(esz);
    const int B = (int)((200ull * per) / mn) + 1;
    const int nb = post_flat_blocks(mn, B, esz);
    CHECK((u64)nb * per >= (u64)B * mn && (u64)(nb - 1) * per < (u64)B * mn);
    long long bad = 0;
    for (int blk = 0; blk < nb; ++blk) bad += replay_block((unsigned)blk, mn, B, NV, magic);
    CHECK(bad == 0);
}

int main() {
    // ---- 1. the whole admitted domain up to 2^17 (and a little beyond), both vector widths
    const unsigned kTop = (1u << 17) + 4096;
    for (unsigned esz : {8u, 4u}) {
        const unsigned NV = post_vec_elems(esz);
        CHECK(NV == 16 / esz && post_block_elems(esz) == 1024 * NV);
        unsigned first_inexact = 0, admitted = 0, refused = 0;
        long long numer_checked = 0;
        for (unsigned mn = 1; mn <= kTop; ++mn) {
            unsigned magic = 0xdeadbeefu;
            const PostFlatRefusal why = post_flat_plan(mn, 1, esz, arena, &magic);
            const PostFlatRefusal want = expected(mn, 1, NV, arena);
            if (mn % NV != 0) {                   // refused as ragged, magic untouched
                CHECK(why == POST_FLAT_RAGGED && want == POST_FLAT_RAGGED && magic == 0xdeadbeefu);
                continue;
            }
            if (why != POST_FLAT_OK) {
                ++refused;
                // one of the four reasons, the right one, and here (B = 1, aligned) it can only be the error bound
                CHECK(why == want && why == POST_FLAT_INEXACT && magic == 0xdeadbeefu);
                if (!first_inexact) first_inexact = mn;
                continue;
            }
            ++admitted;
            CHECK(want == POST_FLAT_OK && (u64)magic * mn >= (1ull << 32) && (u64)(magic - 1) * mn < (1ull << 32));
            CHECK(sweep_numerators(mn, NV, magic) == 0);
            numer_checked += (mn + 1024 * NV) / NV;
            // the block loop itself, as the kernel computes it, on a sample of mn and on everything next to the first refusal
            if (mn % 97 == 0 || mn < 64) replay_blocks(mn, esz, magic);
        }
        for (unsigned mn = first_inexact - 64; mn < first_inexact + 64; ++mn) {
            unsigned magic = 0;
            if (post_flat_plan(mn, 1, esz, arena, &magic) == POST_FLAT_OK) replay_blocks(mn, esz, magic);
        }
        std::printf("NV=%u: %u admitted, %u refused by the error bound, first refused mn = %u, %lld numerators\n", NV, admitted,
                    refused, first_inexact, numer_checked);
        CHECK(first_inexact != 0 && admitted > 0 && refused > 0);
        // the other two reasons, and their order
        unsigned magic = 7;
        for (unsigned off = 1; off < 16; ++off) CHECK(post_flat_plan(2400, 5, esz, arena + off, &magic) == POST_FLAT_MISALIGNED);
        CHECK(post_flat_plan(2400, 5, esz, arena + 16, &magic) == POST_FLAT_OK && magic == 1789570);      // ceil(2^32 / 2400)
        CHECK(post_flat_plan(2401, 5, esz, arena + 1, &magic) == POST_FLAT_RAGGED);
        CHECK(post_flat_plan(0, 5, esz, arena, &magic) == POST_FLAT_RAGGED);
        CHECK(post_flat_plan(65280, 2, esz, arena, &magic) == POST_FLAT_INEXACT);           // 15/2, H = 16
        CHECK(post_flat_plan(65280, 2, esz, arena + 4, &magic) == POST_FLAT_MISALIGNED);
        CHECK(post_flat_plan(65280, 1 << 17, esz, arena, &magic) == POST_FLAT_TOO_LARGE);
    }

    // ---- 2. the B * mn limit: 2^32 and beyond are refused; at the largest admitted B the last blocks' guards are exact
    for (unsigned esz : {8u, 4u}) {
        const unsigned NV = post_vec_elems(esz);
        int replayed = 0;
        for (unsigned mn : {4u, 8u, 12u, 296u, 2400u, 4800u, 32768u, 64512u, 65536u, 131072u}) {
            const int Bmax = (int)(((1ull << 32) - 1) / mn);    // (fits an int from mn = 4 on)
            unsigned magic = 0, m2 = 5;
            const PostFlatRefusal why = post_flat_plan(mn, Bmax, esz, arena, &magic);
            CHECK(why == expected(mn, (u64)Bmax, NV, arena) && why != POST_FLAT_TOO_LARGE);
            CHECK((u64)(Bmax + 1) * mn >= (1ull << 32) && post_flat_plan(mn, Bmax + 1, esz, arena, &m2) == POST_FLAT_TOO_LARGE);
            CHECK(m2 == 5 && post_flat_plan(mn, 0x7fffffff, esz, arena, &m2) == POST_FLAT_TOO_LARGE);
            if (why != POST_FLAT_OK) continue;
            ++replayed;
            const int nb = post_flat_blocks(mn, Bmax, esz);
            const u64 per = post_block_elems(esz);
            CHECK(nb > 0 && (u64)nb * per >= (u64)Bmax * mn && (u64)(nb - 1) * per < (u64)Bmax * mn);
            long long bad = 0;
            for (int blk = nb - 3; blk < nb; ++blk) bad += replay_block((unsigned)blk, mn, Bmax, NV, magic);
            bad += replay_block(0, mn, Bmax, NV, magic) + replay_block((unsigned)(nb / 2), mn, Bmax, NV, magic);
            CHECK(bad == 0);
        }
        CHECK(replayed >= 8);
    }

    // ---- 3. block counts of the per-problem, sparse and scatter launches
    for (unsigned esz : {8u, 4u}) {
        const unsigned per = post_block_elems(esz);
        CHECK(post_problem_blocks(1, esz) == 1 && post_problem_blocks(per, esz) == 1 && post_problem_blocks(per + 1, esz) == 2);
        CHECK(post_problem_blocks(2400, esz) == (esz == 8 ? 2 : 1) && post_problem_blocks(65280, esz) == (esz == 8 ? 32 : 16));
        CHECK(post_flat_blocks(2400, 5, esz) == (esz == 8 ? 6 : 3) && post_flat_blocks(6, 700, 8) == 3);
    }
    CHECK(post_objective_blocks(1) == 1 && post_objective_blocks(4) == 1 && post_objective_blocks(5) == 2 && post_objective_blocks(700) == 175);
    CHECK(post_nnz_blocks(2, 1) == 1 && post_nnz_blocks(256, 1) == 1 && post_nnz_blocks(257, 1) == 2 && post_nnz_blocks(160, 5) == 4);
    CHECK(post_nnz_blocks(1 << 16, 1 << 14) == (1 << 22));          // B * nnz = 2^30: the product is formed in 64 bits
    CHECK(post_nnz_blocks(0x7fffffff, 2) == 0x7fffffff / 128 + 1);

    // ---- 4. the 64-bit reciprocal of the non-zero streams: umul64hi(e, magic64) == e / nnz on both sides of problem boundaries
    {
        auto around = [](int nnz, u64 magic, u64 centre) {          // the elements next to the boundary nearest `centre`
            long long bad = 0;
            const u64 b0 = centre / (u64)nnz;
            for (u64 b = (b0 > 2 ? b0 - 2 : 0); b <= b0 + 2; ++b)
                for (long long d = -3; d <= 3; ++d) {
                    if (b == 0 && d < 0) continue;
                    const u64 e = b * (u64)nnz + (u64)d;
                    const u64 q = umul64hi(e, magic);
                    bad += (q != e / (u64)nnz) | (e - q * (u64)nnz >= (u64)nnz);
                }
            return bad;
        };
        unsigned long long magic = 9;
        for (int nnz = 2; nnz <= (1 << 16); ++nnz) {
            CHECK(post_recip64(nnz, &magic));
            // ceil(2^64 / nnz), said without 2^64
            CHECK((unsigned __int128)magic * (u64)nnz >= ((unsigned __int128)1 << 64) &&
                  (unsigned __int128)(magic - 1) * (u64)nnz < ((unsigned __int128)1 << 64));
            const u64 B = 1000003;                                   // near 0, near B * nnz, near 2^40
            CHECK(around(nnz, magic, 0) + around(nnz, magic, B * (u64)nnz) + around(nnz, magic, 1ull << 40) == 0);
        }
        for (int k = 1; k < 31; ++k) {                              // powers of two: magic64 is 2^(64 - k) exactly
            const int nnz = 1 << k;
            CHECK(post_recip64(nnz, &magic) && magic == (1ull << (64 - k)));
            CHECK(around(nnz, magic, 0) + around(nnz, magic, 12345ull * (u64)nnz) + around(nnz, magic, 1ull << 40) == 0);
            // ... and their odd neighbours while e * nnz < 2^64 holds near 2^40 (what the reciprocal promises)
            if (k < 23) CHECK(post_recip64(nnz + 1, &magic) && around(nnz + 1, magic, 1ull << 40) == 0);
        }
        // the largest band pattern an int holds, at the far end of what e * nnz < 2^64 allows (e < 2^33)
        CHECK(post_recip64(0x7fffffff, &magic) && around(0x7fffffff, magic, 1ull << 32) == 0);
        // nnz < 2 is refused and leaves the magic alone (~0ull / 1 + 1 would wrap to 0: every element in problem 0)
        magic = 9;
        CHECK(!post_recip64(1, &magic) && !post_recip64(0, &magic) && !post_recip64(-3, &magic) && magic == 9);
        CHECK((unsigned long long)(~0ull / 1ull + 1) == 0);
    }

    std::printf("%lld checks, %lld failures\n", checks, failures);
    return failures ? 1 : 0;
}
