// csrc/wgrad_plan.h on the CPU: for ragged row counts, chunk sizes, compute-unit counts and layer widths 1 .. 1024, walk the
// plan exactly as kernels_wgrad.hip does and check that
//   * the chunks cover every row of the call exactly once, each within the chunk capacity;
//   * per layer the K slices of a chunk cover every factor row of the chunk exactly once, start on multiples of ks, and end
//     inside the pitch (so the 16-byte operand loads of a slice never leave a feature's run);
//   * every workgroup index of the accumulation launch maps to one (layer, slice, block) and back, blocks cover G_l;
//   * factor matrices, slabs and gtheta regions are disjoint and inside the sizes the plan reports; a slab write of the last
//     slice's last block stays in bounds;
//   * ks is a power of two in [WG_KS_MIN, WG_KS_MAX] that depends on nothing but shape, compute units and chunk capacity.
// Built with -fsanitize=address,undefined and run by tests/test_weight_grad_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "wgrad_plan.h"

using namespace nempc;

static long long failures = 0, plans = 0;
#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) {                                                      \
            if (++failures < 20) std::printf("FAIL line %d: %s\n", __LINE__, #c); \
        }                                                                \
    } while (0)

static void check(const WgradShape& s, long long cap_rows, long long req, long long rows) {
    const WgradPlan p = wgrad_make_plan(s, cap_rows, req);
    ++plans;
    CHECK(p.nl == s.nl && p.nstage == s.nstage && p.P == wgrad_n_params(s));
    CHECK(p.chunk_rows >= 1 && p.pitch == p.chunk_rows * s.nstage);
    // regions
    long long off = 0, theta = 0, slab = 0;
    for (int l = 0; l < s.nl; ++l) {
        const WgradLayer& L = p.L[l];
        CHECK(L.nfeat == s.din[l] + 1 && L.nout == s.dout[l]);
        CHECK(L.ks >= WG_KS_MIN && L.ks <= WG_KS_MAX && (L.ks & (L.ks - 1)) == 0 && p.pitch % L.ks == 0);
        CHECK(L.nbi * WG_BLOCK >= L.nfeat && (L.nbi - 1) * WG_BLOCK < L.nfeat);
        CHECK(L.nbj * WG_BLOCK >= L.nout && (L.nbj - 1) * WG_BLOCK < L.nout);
        CHECK(L.offA == off); off += (long long)L.nfeat * p.pitch;
        CHECK(L.offAd == off); off += (long long)L.nfeat * p.pitch;
        CHECK(L.offD == off); off += (long long)L.nout * p.pitch;
        CHECK(L.offDd == off); off += (long long)L.nout * p.pitch;
        CHECK(L.theta_off == theta); theta += (long long)L.nfeat * L.nout;
        CHECK(L.slab_off == slab && L.max_slices == p.pitch / L.ks); slab += (long long)L.max_slices * L.nfeat * L.nout;
        CHECK(p.maxdim >= L.nfeat && p.maxdim >= L.nout);
    }
    CHECK(off == p.factor_elems && theta == p.P && slab == p.slab_elems);
    CHECK(off == wgrad_elems_per_frow(s) * p.pitch);
    // the same ks for a smaller batch on the same handle (the plan never sees B)
    // chunks
    const long long nch = wgrad_num_chunks(p, rows);
    long long next = 0;
    for (long long c = 0; c < nch; ++c) {
        long long r0, r1;
        wgrad_chunk(p, rows, c, r0, r1);
        CHECK(r0 == next && r1 > r0 && r1 - r0 <= p.chunk_rows && r1 <= rows);
        CHECK(c == nch - 1 || r1 - r0 == p.chunk_rows);
        next = r1;
        const long long crows = r1 - r0, kvalid = crows * s.nstage;
        long long first[NEMPC_MAX_LAYERS + 1];
        const long long grid = wgrad_grid(p, crows, first);
        CHECK(first[0] == 0 && first[s.nl] == grid);
        for (int l = 0; l < s.nl; ++l) {
            const WgradLayer& L = p.L[l];
            const int ns = wgrad_slices(p, l, crows);
            CHECK(ns >= 1 && ns <= L.max_slices);
            CHECK(first[l + 1] - first[l] == (long long)ns * L.nbi * L.nbj);
            long long covered = 0;
            for (int sl = 0; sl < ns; ++sl) {
                const long long k0 = (long long)sl * L.ks, k1 = k0 + L.ks < kvalid ? k0 + L.ks : kvalid;
                CHECK(k0 == covered && k1 > k0 && k0 + L.ks <= p.pitch);
                covered = k1;
            }
            CHECK(covered == kvalid);
            // the kernel's decoding of a workgroup index: first, last and one in the middle
            const long long n = first[l + 1] - first[l];
            for (long long rel : {0ll, n / 2, n - 1}) {
                const long long bj = rel % L.nbj, bi = (rel / L.nbj) % L.nbi, sl = rel / ((long long)L.nbj * L.nbi);
                CHECK(sl >= 0 && sl < ns && first[l] + (sl * L.nbi + bi) * L.nbj + bj == first[l] + rel);
            }
            // last element a workgroup of the last slice can write, and the reduce kernel's last read
            const long long last = L.slab_off + (long long)(ns - 1) * L.nfeat * L.nout + (long long)(L.nfeat - 1) * L.nout + (L.nout - 1);
            CHECK(last < p.slab_elems);
        }
    }
    CHECK(next == rows);
}

int main() {
    const int widths[] = {1, 2, 3, 7, 15, 16, 17, 31, 33, 63, 64, 65, 127, 129, 144, 255, 257, 511, 1000, 1023, 1024};
    const int cus[] = {1, 7, 64, 80, 256, 304};
    const long long reqs[] = {0, 1, 31, 32, 96, 97, 1000, 4096, 100000};
    const long long rowsets[] = {1, 15, 31, 33, 127, 129, 350, 1400, 4097, 30720};
    unsigned rnd = 12345u;
    auto next = [&]() { rnd = rnd * 1664525u + 1013904223u; return rnd >> 8; };
    for (int nstage : {1, 4})
        for (size_t esz : {(size_t)4, (size_t)8})
            for (int nc : cus)
                for (int w0 : widths)
                    for (int w1 : widths) {
                        WgradShape s{};
                        s.nstage = nstage; s.esz = esz; s.num_cus = nc;
                        // a network in -> w0 -> w1 -> nx (three layers), and the shapes around it with one and eight layers
                        const int nx = 1 + (int)(next() % 64), nin = nx + 1 + (int)(next() % 64);
                        s.nl = 3; s.din[0] = nin; s.dout[0] = w0; s.din[1] = w0; s.dout[1] = w1; s.din[2] = w1; s.dout[2] = nx;
                        for (long long req : reqs)
                            for (long long rows : rowsets) {
                                const long long cap = rows + (long long)(next() % 3) * rows;       // max_batch * H >= the call's rows
                                check(s, cap, req, rows);
                            }
                    }
    for (int w : widths) {          // one layer; eight layers
        WgradShape s{};
        s.nstage = 4; s.esz = 8; s.num_cus = 256;
        s.nl = 1; s.din[0] = w; s.dout[0] = 3;
        check(s, 5000, 0, 4999);
        s.nl = NEMPC_MAX_LAYERS;
        for (int l = 0; l < s.nl; ++l) { s.din[l] = l == 0 ? 5 : w; s.dout[l] = l == s.nl - 1 ? 3 : w; }
        check(s, 5000, 0, 4999);
        check(s, 5000, 96, 4999);
    }
    // ks does not move with the rows of a call, and a chunk size that leads to the same ks cuts K at the same places
    {
        WgradShape s{};
        s.nstage = 4; s.esz = 8; s.num_cus = 256; s.nl = 3;
        s.din[0] = 5; s.dout[0] = 16; s.din[1] = 16; s.dout[1] = 16; s.din[2] = 16; s.dout[2] = 3;
        const WgradPlan a = wgrad_make_plan(s, 350, 0), b = wgrad_make_plan(s, 350, 96);
        ++plans;
        for (int l = 0; l < 3; ++l) CHECK(a.L[l].ks == b.L[l].ks && b.pitch % a.L[l].ks == 0);
        CHECK(b.chunk_rows == 96 && wgrad_num_chunks(b, 350) == 4 && wgrad_num_chunks(a, 350) == 1);
    }
    std::printf("%lld plans checked, %lld failures\n", plans, failures);
    return failures ? 1 : 0;
}
