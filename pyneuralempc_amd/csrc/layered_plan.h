// Layered path, host side, plain C++17 (no HIP): what a sweep will do, decided before anything is launched.  kernels_layered.hip
// walks a plan; tests/layered_plan_check.cpp sweeps the plans over shapes on the CPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <initializer_list>

#include "nempc.h"

namespace nempc {

constexpr int LG_FIRST_KMAX = 8;        // network inputs (nin + ne) layered_first_kernel takes

// Derivatives from the stored ACTIVATION (round 5).  For the activations whose s' is a cheap function of the output (tanh, relu, sigmoid, elu, leaky_relu, selu -- not softplus, whose s' costs an exp, and not the ones written from the
// pre-activation) a layer stores a = s(z) only; whoever needs s'(z) or s''(z) later reads a and forms d1(a) / r2(a) d1(a) in
// its own loader / epilogue.  A forward product then writes one matrix instead of two (rows) or three (Hessian sweeps):
// 2 x 256 at B*H = 20480 in fp64, 42 MB per layer and matrix.
constexpr bool lg_d_from_a(int act) {        // (constexpr: host and device code both call it)
    return act == NEMPC_ACT_TANH || act == NEMPC_ACT_RELU || act == NEMPC_ACT_SIGMOID || act == NEMPC_ACT_ELU ||
           act == NEMPC_ACT_LEAKY_RELU || act == NEMPC_ACT_SELU;
}

// Every environment switch of the path (README "Environment switches"), read once per process (layered_knobs(),
// kernels_layered_impl.h).  Not among them: NEMPC_LAYERED_CHUNK_ROWS, read at every sizing of a workspace.
struct LayeredKnobs {
    // NEMPC_LAYERED_FUSE=0: the reverse sweep walks with the seed kernel, plain products and the skinny last step instead of
    // the fused forms (64-feature blocks only), and the output layer is a launch of its own (A/B knob)
    bool fuse = true;
    // NEMPC_LAYERED_DFA: 0 every layer stores s' (and s'') next to its activation, as in round 4; 1 (default) networks up to width 384
    // form them from the activation in the Hessian sweeps and, with three or more hidden layers, in the rows path; 2 everywhere
    // (A/B; each tested against the default)
    int dfa = 1;
    // NEMPC_LAYERED_HFOLD=0: the Hessian's tangents are written and contracted by layered_hcontract_kernel, as in round 4 (A/B,
    // tested against the default)
    bool hfold = true;
    bool outskip = true;    // NEMPC_LAYERED_OUTSKIP=0: a linear output layer is always formed as a product of its own (A/B, tested)
    bool first = true;      // NEMPC_LAYERED_FIRST=0: gather launch + one-chunk GEMM launch for layer 0, as before (A/B; tested against the default)
    int rm = 0;             // NEMPC_LG_RM = 2 | 4 forces the forward products' 32- or 64-row block (lg_rows32; A/B, tests)
    // (A/B, NEMPC_LG_RM_REV=2: the seed + contraction product on 32-row blocks measured 7 - 11 % slower -- 2 x 256, B*H = 20480:
    // 257 -> 274 us per evaluation in fp64, 136 -> 151 in fp32 -- so the reverse products keep the 64-row block)
    int rm_rev = 0;
    bool cot_order = true;  // NEMPC_LG_COT_ORDER=0: reverse products run cotangent-major instead of row-block-major (gemm_ft)
    bool hess = true;       // NEMPC_LAYERED_HESS=0: no Lagrangian blocks on this path (NEMPC_EUNSUPPORTED; A/B knob)
    int stamp = 11;         // NEMPC_LG_STAMP = 10 SEED + CONTRACT: the product a -DNEMPC_STAMPS build records (diagnostic)
};

struct LayeredNet {          // what the decisions depend on, of a handle
    int nx, nin, ne, nl, maxw, integrator, num_cus;
    const int *din, *dout, *act;        // per layer (the handle's arrays)
    size_t esz;
};

inline int lg_fblocks(int features) { return (features + 63) / 64; }     // 64-feature blocks of a product: one set of partial sums each

// Which networks take this path: at least one hidden layer, up to 128 decision inputs (the window times nx + nu; extra inputs
// do not count) and 64 states, plain or rolling-window models (the gather handles both); everything the register-resident
// matrix-core kernels (mfma_supported) do not take.  (The limits are where the workspaces -- nx and nin cotangent / tangent
// columns per row -- and the per-pair Hessian launches were sized and tested; nothing in the kernels is tied to them.)
inline bool layered_supported(const LayeredNet& n) {
    return n.nl >= 2 && n.nl <= NEMPC_MAX_LAYERS && n.nin <= 128 && n.nx <= 64 && n.maxw <= 1024;
}

// The forms built for wide states: nx > 16 or more than 32 decision inputs.  Shapes inside those limits launch exactly what they
// launched before the limits were lifted to 64 / 128 (same kernels, same arguments, same chunking).
inline bool lg_wide(const LayeredNet& n) { return n.nx > 16 || n.nin > 32; }

// A workspace region: `rows` rows of Rp elements, `off` such rows in (Rp: the chunk's rows in whole GEMM blocks)
struct LgRegion { size_t off, rows; };
// A region lent to a step it was not sized for (partial sums wait there), by name and rows needed: a sweep checks every loan
// against the region's capacity before its first launch, and reaches the memory through the loan only
struct LgLoan {
    LgRegion region;
    const char* name;       // (null: the plan does not use this loan)
    size_t rows;
    bool used() const { return name != nullptr; }
    bool fits() const { return rows <= region.rows; }
};

struct LayeredFwdWs {       // what the forward walk touches, in both workspaces
    LgRegion xi, x0, x1, d[NEMPC_MAX_LAYERS], f, dl;
};
struct LayeredWs : LayeredFwdWs {
    LgRegion g0, g1, j, kprev, acck, dk, dkn, accdk;
    size_t total;
};
struct LayeredHws : LayeredFwdWs {
    LgRegion e[NEMPC_MAX_LAYERS], cw[NEMPC_MAX_LAYERS], cl, wl, q0, q1, P, a0, a1, pl, hacc, l0p;
    size_t total;
};
// the next `rows` rows behind *p -- for every region of `regions`, in their order
inline void lg_take(size_t& p, size_t rows, std::initializer_list<LgRegion*> regions) {
    for (LgRegion* r : regions) {
        *r = LgRegion{p, rows};
        p += rows;
    }
}

inline LayeredWs layered_offsets(const LayeredNet& n) {
    LayeredWs o{};
    const size_t nx = (size_t)n.nx, nin = (size_t)n.nin, maxw = (size_t)n.maxw;
    size_t p = 0;
    lg_take(p, nin + n.ne, {&o.xi});
    lg_take(p, maxw, {&o.x0, &o.x1});
    for (int l = 0; l < n.nl - 1; ++l) lg_take(p, (size_t)n.dout[l], {&o.d[l]});
    lg_take(p, nx, {&o.f, &o.dl});
    // the cotangent buffers: maxw rows of nx Rp columns -- and room for the last reverse product's partial sums of J, nin rows
    // per 64-feature block of layer 0 (never more than the width up to 32 inputs; up to 2 w + 128 rows at 128)
    const size_t grows = std::max(maxw, (size_t)lg_fblocks(n.dout[0]) * nin);
    lg_take(p, grows * nx, {&o.g0, &o.g1});
    lg_take(p, nin * nx, {&o.j});
    if (n.integrator == NEMPC_RK4) {
        lg_take(p, nx, {&o.kprev, &o.acck});
        lg_take(p, nx * nin, {&o.dk, &o.dkn, &o.accdk});
    }
    o.total = p;
    return o;
}

inline LayeredHws layered_hess_offsets(const LayeredNet& n) {
    LayeredHws o{};
    const size_t nx = (size_t)n.nx, nin = (size_t)n.nin, maxw = (size_t)n.maxw;
    size_t p = 0;
    lg_take(p, nin + n.ne, {&o.xi});
    lg_take(p, maxw, {&o.x0, &o.x1});
    for (int l = 0; l < n.nl - 1; ++l) lg_take(p, (size_t)n.dout[l], {&o.d[l], &o.e[l], &o.cw[l]});
    lg_take(p, nx, {&o.f, &o.dl, &o.cl, &o.wl});
    lg_take(p, maxw, {&o.q0, &o.q1});
    lg_take(p, maxw * nin, {&o.P, &o.a0, &o.a1});
    lg_take(p, nx * nin, {&o.pl});
    lg_take(p, nin * nin, {&o.hacc});
    // curvature terms per feature block as pair-major partial sums (<= 32 pairs): layer 0's (CONTRACT_REVERSE of the product
    // that forms q_0) and, with nin <= 4, every other hidden layer's (CONTRACT_HPAIR of its tangent product)
    lg_take(p, (size_t)lg_fblocks(n.maxw) * 32 * (size_t)(n.nin <= 4 ? n.nl - 1 : 1), {&o.l0p});
    o.total = p;
    return o;
}

// ---- rows sweep (g and the compact Jacobian tiles)
struct RowsPlan {
    LayeredWs ws;
    bool rk4, wide;
    bool fuse_out;          // the output layer as a contraction in the last hidden layer's epilogue
    bool lin_skip;          // no output step: layered_finish_kernel forms f from the partial sums (plan_rows)
    // gather + layer 0 in one vector-unit launch (layered_first_kernel): few inputs, two hidden layers or more (layer 0 is
    // not the layer the output contraction leaves from), Discret / Unity (the RK4 stages' inputs carry c DT k_{s-1} and
    // their records want xi)
    bool first, first_dfa;
    // layers that store their activation only (their s' is formed from it where it is needed: lg_d_from_a); the
    // activation then lives in the layer's own slot (ws.d[l]) instead of the two alternating ones
    bool dfa[NEMPC_MAX_LAYERS];
    // two hidden layers or more: the first reverse product forms the seed in its loader, the last one contracts with
    // W_0 in its epilogue -- neither the seed matrix nor G_0 goes through memory (2 x 256, B*H = 20480, fp64:
    // 84 MB each way, twice)
    bool fused_reverse;
    LgLoan out_sums, jac_sums;      // partial sums of the network output (fuse_out) and of the Jacobian (layer 0 wider than a block)
};

// Rows sweep, measured (tools/layered_bench.py with NEMPC_LAYERED_DFA = 0 | 1 on every launch): the ROWS path gains nothing --
// 2 x 256 fp64 267 -> 269 us, 3 x 256 476 -> 467, 4 x 512 RK4 25.3 -> 25.4 ms: its layer-0 product is latency-bound,
// not store-bound, and the last hidden layer stores one matrix either way -- so it keeps s' stored; the Hessian
// sweeps, which store three matrices per layer, take it: NEMPC_LAYERED_DFA=2 forces it here too, for the A/B)
// Round 5, measured again with primed clocks (tools/layered_ab.py, us per evaluation in fp64: stored s' / activations only
// for all but the last hidden layer / for every layer): 2 x 256 213 / 215 / 216, 3 x 256 387 / 373 / 364.  The products
// between hidden layers are the ones that gain (one matrix stored instead of two); layer 0 is latency-bound either
// way.  So: 1 (default) every layer of a network with three or more hidden layers, up to width 384; 2 every layer of
// every network; 0 none.
inline bool rows_dfa(const LayeredNet& n, const LayeredKnobs& k, int l, bool first_dfa) {
    if (l == 0 && first_dfa) return true;       // (layered_first_kernel is store-bound: one matrix instead of two)
    return lg_d_from_a(n.act[l]) && (k.dfa == 2 || (k.dfa == 1 && n.maxw <= 384 && n.nl - 1 >= 3));
}
// Hessian sweeps, measured (profiles/r05_layered_dfa.txt): 2 x 256 fp64 503 -> 461 us, 3 x 256 898 -> 851 us; 4 x 512 RK4
// 83.9 -> 85.2 ms (compute-bound products: the stores were free, the extra vector work in loader and epilogue is not) --
// hence the width rule
inline bool hess_dfa(const LayeredNet& n, const LayeredKnobs& k, int l) {
    return k.dfa && (n.maxw <= 384 || k.dfa == 2) && lg_d_from_a(n.act[l]);
}

inline RowsPlan plan_rows(const LayeredNet& n, const LayeredKnobs& k) {
    RowsPlan p{};
    const int nl = n.nl;
    p.ws = layered_offsets(n);
    p.rk4 = n.integrator == NEMPC_RK4;
    p.wide = lg_wide(n);
    p.fuse_out = k.fuse;
    // a LINEAR output layer, Discret / Unity: s_L' = 1 and f = sum of the partial sums + bias is formed by layered_finish_kernel
    // (only where the partial sums -- nx rows per 64-feature block -- fit the spare activation buffer of maxw rows: a
    // network narrower than its state would write past it into x1 and the s' slots)
    p.lin_skip = k.outskip && p.fuse_out && nl >= 3 && !p.rk4 && n.act[nl - 1] == NEMPC_ACT_LINEAR &&
                 lg_fblocks(n.dout[nl - 2]) * n.nx <= n.maxw;
    p.first = k.first && !p.rk4 && nl - 1 >= 2 && n.nin + n.ne <= LG_FIRST_KMAX;
    p.first_dfa = p.first && k.dfa != 0 && lg_d_from_a(n.act[0]);
    for (int l = 0; l < nl - 1; ++l) p.dfa[l] = rows_dfa(n, k, l, p.first_dfa);
    p.fused_reverse = nl >= 3 && k.fuse;
    if (p.fuse_out) {
        const size_t rows = (size_t)lg_fblocks(n.dout[nl - 2]) * n.nx;
        // lin_skip: the sums wait in the activation buffer the last hidden layer's product does not read (the cotangent buffers
        // are overwritten by the reverse sweep before the finish kernel runs); else in the cotangent buffer, filled later
        const bool reads_x1 = nl >= 3 && !p.dfa[nl - 3] && ((nl - 3) & 1);
        if (!p.lin_skip) p.out_sums = LgLoan{p.ws.g0, "g0", rows};
        else p.out_sums = reads_x1 ? LgLoan{p.ws.x0, "x0", rows} : LgLoan{p.ws.x1, "x1", rows};
    }
    if (p.fused_reverse && lg_fblocks(n.dout[0]) > 1) {
        // (the cotangent buffer the last product does not read: products nl-3 .. 0 write g0, g1, g0, ...)
        const size_t rows = (size_t)lg_fblocks(n.dout[0]) * n.nin * n.nx;
        p.jac_sums = (nl - 3) % 2 == 0 ? LgLoan{p.ws.g0, "g0", rows} : LgLoan{p.ws.g1, "g1", rows};
    }
    return p;
}

// ---- Hessian sweeps (contracted network Hessian of every row)
struct HessPlan {
    LayeredHws ws;
    bool lin_out;
    int npair;              // input pairs p >= q
    // layer 0's curvature term from the epilogue of the product that forms q_0: two hidden layers or more (there is such a
    // product), at most 32 input pairs (nin <= 7)
    bool fuse_l0;
    // a LINEAR output layer: the Hessian sweeps need nothing of it (s_L' = 1, s_L'' = 0, and f is not an output of this
    // callback): no contraction, no output step
    bool lin_noout;
    bool contract_out;      // the output layer in the last hidden layer's epilogue
    bool first;             // as RowsPlan::first; not in direct mode, whose inputs are the stage records
    bool dfa[NEMPC_MAX_LAYERS];
    // Up to four inputs (round 5): the tangent columns are INTERLEAVED -- a tile is 16 rows x nin inputs -- so that a lane of the
    // product holds the tangents of every input of its row, and the layer's curvature term leaves from the epilogue
    // (LG_CONTRACT_HPAIR): the tangents (126 MB at 2 x 256, B*H = 20480, fp64) are neither written nor read back, and the
    // contraction launch is gone.  Otherwise: the tangents go through memory to layered_hcontract_kernel.
    bool fold;
    int l0p_at[NEMPC_MAX_LAYERS];   // feature block behind ws.l0p at which layer l's partial sums start
    int pblocks;                    // ... and how many blocks there are in all
    LgLoan out_sums;        // contract_out: the output's partial sums in the tangent buffer, free until the tangent sweep
    LgLoan l0p_stack;       // fuse_l0: the curvature terms' partial sums, npair rows per feature block
};

inline HessPlan plan_hess(const LayeredNet& n, const LayeredKnobs& k, bool direct) {
    HessPlan p{};
    const int nl = n.nl;
    p.ws = layered_hess_offsets(n);
    p.lin_out = n.act[nl - 1] == NEMPC_ACT_LINEAR;
    p.npair = n.nin * (n.nin + 1) / 2;
    p.fuse_l0 = k.fuse && nl >= 3 && p.npair <= 32;
    p.lin_noout = k.outskip && p.lin_out;
    p.contract_out = k.fuse && !p.lin_noout;
    p.first = k.first && !direct && nl - 1 >= 2 && n.nin + n.ne <= LG_FIRST_KMAX;
    for (int l = 0; l < nl - 1; ++l) p.dfa[l] = hess_dfa(n, k, l);
    p.fold = p.fuse_l0 && p.lin_out && n.nin >= 2 && n.nin <= 4 && k.hfold;
    if (p.fuse_l0) {
        p.pblocks = lg_fblocks(n.dout[0]);
        for (int l = 1; p.fold && l < nl - 1; ++l) {
            p.l0p_at[l] = p.pblocks;
            p.pblocks += lg_fblocks(n.dout[l]);
        }
        p.l0p_stack = LgLoan{p.ws.l0p, "l0p", (size_t)p.pblocks * p.npair};
    }
    if (p.contract_out) p.out_sums = LgLoan{p.ws.P, "P", (size_t)lg_fblocks(n.dout[nl - 2]) * n.nx};
    return p;
}

}  // namespace nempc
