// nempc_weight_grad, host side, plain C++17 (no HIP): chunks of rows, the factor workspace, the K slices of the accumulation
// GEMM and their slabs, decided before anything is launched.  kernels_wgrad.hip walks a plan; tests/wgrad_plan_check.cpp
// sweeps the plans over shapes on the CPU.
//
// Names.  A row is one (problem, step) pair; a FACTOR ROW is one (row, integrator stage) pair: nstage = 4 under RK4, else 1,
// factor row = row * nstage + stage.  Per dense layer l the row sweep leaves four matrices, feature-major with the factor
// rows contiguous (pitch = the chunk's capacity in factor rows):
//     A_l, Adot_l   (in_l + 1) features: the layer's input and its tangent; feature in_l is the ones column of the bias
//                   (1 in A_l, 0 in Adot_l), so that [W_l ; b_l] is ONE (in_l + 1, out_l) product, in gtheta's own layout
//     D_l, Ddot_l   out_l features: the cotangent of the pre-activation and its tangent
// and the accumulation forms  G_l = A_l' Ddot_l + Adot_l' D_l  over the factor rows (K).  K is cut into slices of ks_l factor
// rows; one workgroup owns one 64 x 64 block of G_l over one slice and writes it into that slice's slab; a second launch adds
// the slabs in slice order onto the result of the earlier chunks.
//
// ks_l depends on the layer's shape, the compute-unit count and the chunk capacity only -- never on B -- and a chunk holds a
// whole number of slices of every layer.  Together with the compaction of skipped problems (the kept problems' rows are
// numbered consecutively) this makes the grouping of the sum a function of the kept rows alone: a batch with skipped
// problems gives the bits of the batch without them, and two chunk sizes that lead to the same ks_l give the same bits.
#pragma once

#include <cstddef>

#include "nempc.h"

namespace nempc {

constexpr int WG_BLOCK = 64;              // edge of the block of G_l one workgroup owns (4 waves, 32 x 32 each)
constexpr int WG_KS_MIN = 128;            // factor rows per K slice: a power of two in [WG_KS_MIN, WG_KS_MAX]
constexpr int WG_KS_MAX = 4096;
constexpr int WG_WGS_PER_CU = 4;          // workgroups per compute unit a full chunk aims for
constexpr long long WG_WS_BYTES = 256ll << 20;   // default bound of the factor workspace

struct WgradShape {          // what the plan depends on, of a handle
    int nl, nstage, num_cus;
    int din[NEMPC_MAX_LAYERS], dout[NEMPC_MAX_LAYERS];
    size_t esz;
};

struct WgradLayer {
    int nfeat, nout;         // in_l + 1, out_l: G_l is (nfeat, nout) row-major at theta_off of gtheta
    int nbi, nbj;            // blocks of WG_BLOCK over nfeat / nout
    int ks;                  // factor rows per K slice
    int max_slices;          // slices of a full chunk: pitch / ks
    long long offA, offAd, offD, offDd;   // element offsets of the four factor matrices in the factor region
    long long theta_off;     // element offset of [W_l | b_l] in gtheta
    long long slab_off;      // element offset of this layer's slabs (max_slices of nfeat * nout) in the slab region
};

struct WgradPlan {
    int nl, nstage;
    long long chunk_rows;    // rows per chunk (the last chunk of a call may hold fewer)
    long long pitch;         // factor rows of a chunk = chunk_rows * nstage: a multiple of every ks
    long long factor_elems;  // elements of the factor region: sum_l (2 nfeat + 2 nout) * pitch
    long long slab_elems;    // elements of the slab region
    long long P;             // parameters: sum_l nfeat * nout
    int maxdim;              // widest layer input or output (scratch of the sweep)
    WgradLayer L[NEMPC_MAX_LAYERS];
};

inline long long wgrad_n_params(const WgradShape& s) {
    long long P = 0;
    for (int l = 0; l < s.nl; ++l) P += (long long)(s.din[l] + 1) * s.dout[l];
    return P;
}

// elements of the factor region per factor row (the DESIGN section's "workspace per row" is this times nstage times esz)
inline long long wgrad_elems_per_frow(const WgradShape& s) {
    long long e = 0;
    for (int l = 0; l < s.nl; ++l) e += 2ll * (s.din[l] + 1) + 2ll * s.dout[l];
    return e;
}

inline long long wgrad_pow2_floor(long long x) {
    long long p = 1;
    while (p * 2 <= x) p *= 2;
    return p;
}

// cap_rows: rows the handle can be asked for (max_batch * H, >= 1); req_rows: NEMPC_WGRAD_CHUNK_ROWS, <= 0 = default (as
// many rows as WG_WS_BYTES of factors hold, at most cap_rows)
inline WgradPlan wgrad_make_plan(const WgradShape& s, long long cap_rows, long long req_rows) {
    WgradPlan p{};
    p.nl = s.nl; p.nstage = s.nstage;
    if (cap_rows < 1) cap_rows = 1;
    const long long per_row = wgrad_elems_per_frow(s) * s.nstage * (long long)s.esz;
    long long rows = req_rows > 0 ? req_rows : WG_WS_BYTES / per_row;
    if (rows < 1) rows = 1;
    if (rows > cap_rows) rows = cap_rows;
    const long long frows = rows * s.nstage;
    int ks_max = WG_KS_MIN;
    for (int l = 0; l < s.nl; ++l) {
        WgradLayer& L = p.L[l];
        L.nfeat = s.din[l] + 1; L.nout = s.dout[l];
        L.nbi = (L.nfeat + WG_BLOCK - 1) / WG_BLOCK; L.nbj = (L.nout + WG_BLOCK - 1) / WG_BLOCK;
        long long ks = wgrad_pow2_floor(frows * L.nbi * L.nbj / ((long long)WG_WGS_PER_CU * (s.num_cus < 1 ? 1 : s.num_cus)) + 1);
        if (ks < WG_KS_MIN) ks = WG_KS_MIN;
        if (ks > WG_KS_MAX) ks = WG_KS_MAX;
        L.ks = (int)ks;
        if (L.ks > ks_max) ks_max = L.ks;
        if (L.nfeat > p.maxdim) p.maxdim = L.nfeat;
        if (L.nout > p.maxdim) p.maxdim = L.nout;
    }
    const long long unit = ks_max / s.nstage;        // (ks_max >= 128, nstage is 1 or 4)
    p.chunk_rows = (rows + unit - 1) / unit * unit;
    p.pitch = p.chunk_rows * s.nstage;
    long long off = 0, theta = 0, slab = 0;
    for (int l = 0; l < s.nl; ++l) {
        WgradLayer& L = p.L[l];
        L.offA = off; off += (long long)L.nfeat * p.pitch;
        L.offAd = off; off += (long long)L.nfeat * p.pitch;
        L.offD = off; off += (long long)L.nout * p.pitch;
        L.offDd = off; off += (long long)L.nout * p.pitch;
        L.theta_off = theta; theta += (long long)L.nfeat * L.nout;
        L.max_slices = (int)(p.pitch / L.ks);
        L.slab_off = slab; slab += (long long)L.max_slices * L.nfeat * L.nout;
    }
    p.factor_elems = off; p.P = theta; p.slab_elems = slab;
    return p;
}

inline long long wgrad_num_chunks(const WgradPlan& p, long long rows) { return (rows + p.chunk_rows - 1) / p.chunk_rows; }
// rows [r0, r1) of chunk c of a call over `rows` rows
inline void wgrad_chunk(const WgradPlan& p, long long rows, long long c, long long& r0, long long& r1) {
    r0 = c * p.chunk_rows;
    r1 = r0 + p.chunk_rows < rows ? r0 + p.chunk_rows : rows;
}
// K slices of layer l in a chunk of `crows` rows; slice s covers the chunk's factor rows [s ks, min((s+1) ks, crows nstage))
inline int wgrad_slices(const WgradPlan& p, int l, long long crows) {
    return (int)((crows * p.nstage + p.L[l].ks - 1) / p.L[l].ks);
}
// workgroups of the accumulation launch over a chunk of `crows` rows; first[l] = the first workgroup of layer l
// (first[nl] = the total).  Workgroup first[l] + (s * nbi + bi) * nbj + bj owns block (bi, bj) of slice s.
inline long long wgrad_grid(const WgradPlan& p, long long crows, long long* first) {
    long long g = 0;
    for (int l = 0; l < p.nl; ++l) {
        first[l] = g;
        g += (long long)wgrad_slices(p, l, crows) * p.L[l].nbi * p.L[l].nbj;
    }
    first[p.nl] = g;
    return g;
}

}  // namespace nempc
