// Batched solver, the seam between Solve<T> and a stage augmentation (stage_aug.h: the host arithmetic; solver_roll_impl.h,
// solver_rate_impl.h, solver_rows_impl.h: the kernels).  StageAug<T> is everything of one solve that is specific to the augmentation: what the
// workspace holds beyond the plain buffers, where bounds land, the augmented start and objective table, the evaluation of
// the callbacks in augmented form, the solution handed back.  Solve<T> asks it `on()` where the SCHEDULE depends on running
// augmented; which augmentation is decided here, by a switch on the kind.  Included by solver.hip only, after the kernels.
#pragma once

#include <cstring>
#include <vector>

#include "rows_index.h"
#include "stage_aug.h"

namespace nempc {

namespace {

struct BufReq { void** p; size_t bytes; };      // one device buffer of the workspace

// the callbacks on the handle's variant (plain solves: on the solver's buffers; augmented: on the caller-side ones below)
inline int callback_rows(Handle& h, int nb, const void* Zs, const void* X0s, void* g, void* tiles, void* tiles_scratch, hipStream_t s) {
    if (h.variant == NEMPC_KERNEL_VALU) return launch_rows_valu(h, nb, Zs, X0s, g, tiles ? tiles : tiles_scratch, s);
    RowsOut ro; ro.g = g; ro.tiles = tiles;
    return launch_rows_mfma(h, nb, Zs, X0s, ro, s);
}
inline int callback_blocks(Handle& h, int nb, const void* Zs, const void* X0s, const void* lam, void* blocks, hipStream_t s) {
    if (h.variant == NEMPC_KERNEL_VALU) return launch_rowhess_valu(h, nb, Zs, X0s, lam, blocks, s);
    HessOut ho; ho.blocks = blocks;
    return launch_rowhess_mfma(h, nb, Zs, X0s, lam, ho, s);
}

// what an augmentation keeps in the workspace (SolverWs::aug): the caller-side evaluation buffers, the augmented start and
// solution, the window's tables, and the host copies behind the upload-when-changed tests
struct AugWs {
    int kind = AUG_NONE;                      // the augmentation the workspace was built for
    RollTables rt;
    void *rZ = nullptr, *rg = nullptr, *rtiles = nullptr, *rhblk = nullptr, *rgrad = nullptr, *rlam = nullptr,
         *rZin = nullptr, *rS0 = nullptr, *rZout = nullptr, *robj = nullptr;
    std::vector<int> bslot;                   // bound_slots: where entry i of the bound list lands in the solver's bound vector
    std::vector<unsigned char> robj_host;     // the augmented objective table as last uploaded
};

template <typename T>
struct StageAug {
    Handle& h; AugWs& w; const hipStream_t s;
    const int kind, B, H, nx_r, nu, nin_r, n_r, m_r;      // *_r: the handle's (the caller's variables, the callbacks' shapes)
    const StageDims d;                                     // the solver's
    const RateDims rd; const RowsDims wd; const ObjOffsets ao; const unsigned gRn;      // gRn: grid of the element-wise kernels over the caller's variables
    const void* X0 = nullptr;                              // the caller's initial states (the callbacks read them by problem index)
    void *f = nullptr, *g = nullptr, *gt = nullptr, *tiles = nullptr, *hblk = nullptr, *grad = nullptr;   // the solver's evaluation buffers
    RollTablesHost th;                                     // (between buffers() and upload_tables() of a workspace being built)
    StageAug(Handle& hh, AugWs& ww, int BB, hipStream_t ss)
        : h(hh), w(ww), s(ss), kind(hh.w > 1 ? AUG_WINDOW : (hh.rate.on() ? AUG_RATE : (hh.rows.on() ? AUG_ROWS : AUG_NONE))),
          B(BB), H(hh.cfg.H), nx_r(hh.cfg.nx), nu(hh.cfg.nu), nin_r(hh.nin), n_r(hh.n), m_r(hh.m),
          d(stage_dims(kind, H, nx_r, nu, hh.w, hh.rows.nc)), rd(rate_dims(H, nx_r, nu)), wd(rows_dims(H, nx_r, nu, hh.rows.nc)), ao(obj_offsets(H, d.nx, nu)), gRn((unsigned)(((size_t)BB * n_r + 255) / 256)) {}
    bool on() const { return kind != AUG_NONE; }
    template <typename F> int each_table(F f) {
        const struct { int** p; const std::vector<int>* v; } tb[] = {{&w.rt.src, &th.src}, {&w.rt.src0, &th.src0}, {&w.rt.prim, &th.prim},
                                                                     {&w.rt.isprim, &th.isprim}, {&w.rt.dcol, &th.dcol}, {&w.rt.shift, &th.shift}};
        for (const auto& x : tb) if (int rc = f(x.p, *x.v)) return rc;
        return NEMPC_OK;
    }
    // ---- workspace: what a rebuilt one allocates beyond the plain buffers, and what it holds from the start
    void buffers(std::vector<BufReq>& al) {
        if (!on()) return;
        const size_t e = sizeof(T), Bn = (size_t)B;
        al.insert(al.end(), {
            {&w.rZ, Bn * n_r * e}, {&w.rg, Bn * m_r * e}, {&w.rtiles, Bn * H * nx_r * nin_r * e},
            {&w.rhblk, Bn * H * nin_r * nin_r * e}, {&w.rlam, Bn * m_r * e},
            {&w.rZin, Bn * d.n * e}, {&w.rS0, Bn * d.nx * e}, {&w.rZout, Bn * d.n * e}, {&w.robj, (size_t)ao.total * e}});
        if (kind != AUG_WINDOW) return;
        al.push_back({&w.rgrad, Bn * n_r * e});      // (rate, rows: the gradient comes from the augmented table)
        th = roll_tables(H, nx_r, nu, h.w, h.rev);
        (void)each_table([&](int** p, const std::vector<int>& v) { al.push_back({(void**)p, v.size() * sizeof(int)}); return 0; });
    }
    int upload_tables() {
        w.kind = kind;
        w.bslot = bound_slots(kind, H, nx_r, nu, h.w, h.rows.nc);
        if (!on()) return NEMPC_OK;
        NEMPC_HIP(hipMemsetAsync(w.rlam, 0, (size_t)B * m_r * sizeof(T), s));     // (box rows of the handle keep zero multipliers)
        if (kind != AUG_WINDOW) return NEMPC_OK;
        return each_table([](int** p, const std::vector<int>& v) -> int {
            NEMPC_HIP(hipMemcpy(*p, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice));
            return NEMPC_OK;
        });
    }
    // ---- bounds: the list the augmentation's slots index -- the caller's bounds on z, then what it adds (rate: the limits on
    //      the moves; rows: the limits of the rows)
    void append_bounds(std::vector<double>& lo, std::vector<double>& hi) const {
        if (kind != AUG_RATE && kind != AUG_ROWS) return;
        const std::vector<double>&alo = kind == AUG_RATE ? h.rate.dlo : h.rows.lo, &ahi = kind == AUG_RATE ? h.rate.dhi : h.rows.hi;
        lo.insert(lo.end(), alo.begin(), alo.end());
        hi.insert(hi.end(), ahi.begin(), ahi.end());
    }
    // ---- start: the augmented guess and start state (window: s_0 from x0 and the history; rate: s_{-1} = [x0 ; u_prev]; rows:
    //      s_{-1} = [x0 ; 0]) from the caller's, and the objective table over the augmented stage.  grid: the solver's element-wise grid
    int start(const void* Z, const void* X0_, const void* lb, const void* ub, T mu0, int has_bounds, unsigned grid) {
        X0 = X0_;
        switch (kind) {
        case AUG_WINDOW:
            hipLaunchKernelGGL(roll_build_kernel<T>, dim3(grid), dim3(256), 0, s, B, d.n, d.nx, n_r, nx_r, nu, h.w - 1, w.rt, (const T*)Z,
                               (const T*)X0, (const T*)h.d_hist_x, (const T*)h.d_hist_u, (const T*)lb, (const T*)ub, mu0, has_bounds,
                               (T*)w.rZin, (T*)w.rS0);
            break;
        case AUG_RATE:
            hipLaunchKernelGGL(rate_build_kernel<T>, dim3(grid), dim3(256), 0, s, B, rd, (const T*)Z, (const T*)X0,
                               (const T*)h.rate.u_prev, (const T*)lb, (const T*)ub, mu0, has_bounds, (T*)w.rZin, (T*)w.rS0);
            break;
        case AUG_ROWS:
            hipLaunchKernelGGL(rows_build_kernel<T>, dim3(grid), dim3(256), 0, s, B, wd, (const T*)Z, (const T*)X0,
                               h.d_rows_C.as<const T>(), (const T*)lb, (const T*)ub, mu0, has_bounds, (T*)w.rZin, (T*)w.rS0);
            break;
        }
        const ObjHost& oh = h.obj_host;
        const AugObjIn in{oh.Q.data(), oh.R.data(), (h.obj_QT.empty() ? oh.Q : h.obj_QT).data(), oh.xref.data(), oh.uref.data(),
                          oh.cx.data(), oh.cu.data(), h.rate.S.data()};
        return upload_aug_table(aug_objective_table<T>(kind, H, nx_r, nu, h.w, in, h.rows.nc));
    }
    // (uploaded when it changes, like the bounds)
    int upload_aug_table(const std::vector<T>& tab) {
        const size_t tb = tab.size() * sizeof(T);
        if (w.robj_host.size() != tb || memcmp(w.robj_host.data(), tab.data(), tb) != 0) {
            NEMPC_HIP(hipMemcpyAsync(w.robj, tab.data(), tb, hipMemcpyHostToDevice, s));
            NEMPC_HIP(hipStreamSynchronize(s));   // tab is stack-owned
            w.robj_host.assign((const unsigned char*)tab.data(), (const unsigned char*)tab.data() + tb);
        }
        return NEMPC_OK;
    }
    // ---- callbacks in augmented form: gather the caller's variables (and the multipliers of the network rows), launch the
    //      handle's kernels on them, spread the results.  Everything at an iterate -- defects, tiles, f, gradient, Lagrangian
    //      blocks, into the iterate's buffers -- or, at a trial point (lam_aug = null), the defects only, into gt (the acceptance
    //      kernel evaluates the objective from the augmented table itself).
    //      window: the network reads the primary copies, f and the gradient come from the handle's objective kernel;
    //      rate: the network reads x_t, u_{t-1} + v_t, f and the gradient come from the augmented table inside the spread kernel;
    //      rows: the network reads the x and u slots, its multipliers are lam_x + Cx' lam_y, f and the gradient as for rate
    int eval(const void* Zaug, const void* lam_aug) {
        const bool full = lam_aug != nullptr;
        T* const lam_r = full ? (T*)w.rlam : (T*)nullptr;
        switch (kind) {
        case AUG_WINDOW:
            hipLaunchKernelGGL(roll_in_kernel<T>, dim3(gRn), dim3(256), 0, s, B, d.n, n_r, H, nx_r, d.nx, m_r, w.rt, (const T*)Zaug,
                               (T*)w.rZ, (const T*)lam_aug, lam_r);
            break;
        case AUG_RATE:
            hipLaunchKernelGGL(rate_gather_kernel<T>, dim3(gRn), dim3(256), 0, s, B, rd, m_r, 0, (const T*)Zaug, (const T*)w.rS0,
                               (T*)w.rZ, (const T*)lam_aug, lam_r);
            break;
        case AUG_ROWS:
            hipLaunchKernelGGL(rows_gather_kernel<T>, dim3(gRn), dim3(256), 0, s, B, wd, m_r, h.d_rows_C.as<const T>(), (const T*)Zaug,
                               (T*)w.rZ, (const T*)lam_aug, lam_r);
            break;
        }
        int r = callback_rows(h, B, w.rZ, X0, w.rg, full ? w.rtiles : nullptr, h.d_tiles_ws.get(), s);
        if (r) return r;
        if (full && (r = callback_blocks(h, B, w.rZ, X0, w.rlam, w.rhblk, s))) return r;
        if (full && kind == AUG_WINDOW && (r = launch_objective(h, B, w.rZ, f, w.rgrad, s))) return r;
        const T *tiles_r = full ? (const T*)w.rtiles : nullptr, *hblk_r = full ? (const T*)w.rhblk : nullptr;
        T *g_a = full ? (T*)g : (T*)gt, *tiles_a = full ? (T*)tiles : nullptr, *hblk_a = full ? (T*)hblk : nullptr,
          *grad_a = full ? (T*)grad : nullptr;
        switch (kind) {
        case AUG_WINDOW:
            hipLaunchKernelGGL(roll_out_kernel<T>, dim3(B * H), dim3(256), 0, s, H, nx_r, nu, d.nx, nin_r, n_r, m_r, w.rt,
                               (const T*)Zaug, (const T*)w.rS0, (const T*)w.rg, tiles_r, hblk_r,
                               full ? (const T*)w.rgrad : (const T*)nullptr, g_a, tiles_a, hblk_a, grad_a);
            break;
        case AUG_RATE:
            hipLaunchKernelGGL(rate_spread_kernel<T>, dim3(B * H), dim3(256), 0, s, rd, m_r, (const T*)Zaug, (const T*)w.rS0,
                               (const T*)w.rg, tiles_r, hblk_r, (const T*)w.robj, ao, g_a, tiles_a, hblk_a, grad_a,
                               full ? (T*)f : (T*)nullptr);
            break;
        case AUG_ROWS:
            hipLaunchKernelGGL(rows_spread_kernel<T>, dim3(B * H), dim3(256), 0, s, wd, m_r, h.d_rows_C.as<const T>(), (const T*)Zaug,
                               (const T*)w.rg, tiles_r, hblk_r, (const T*)w.robj, ao, g_a, tiles_a, hblk_a, grad_a,
                               full ? (T*)f : (T*)nullptr);
            break;
        }
        return NEMPC_OK;
    }
    // ---- finish: the scatter writes the augmented solution to rZout, the caller's Z is its primary copies (window), the x
    //      and u slots of the state (rate) or the x slots and the stage controls (rows)
    void* solution_buffer(void* Z) const { return on() ? w.rZout : Z; }
    void hand_back(void* Z) {
        switch (kind) {
        case AUG_WINDOW:
            hipLaunchKernelGGL(roll_in_kernel<T>, dim3(gRn), dim3(256), 0, s, B, d.n, n_r, H, nx_r, d.nx, m_r, w.rt, (const T*)w.rZout,
                               (T*)Z, (const T*)nullptr, (T*)nullptr);
            break;
        case AUG_RATE:
            hipLaunchKernelGGL(rate_gather_kernel<T>, dim3(gRn), dim3(256), 0, s, B, rd, m_r, 1, (const T*)w.rZout, (const T*)w.rS0,
                               (T*)Z, (const T*)nullptr, (T*)nullptr);
            break;
        case AUG_ROWS:
            hipLaunchKernelGGL(rows_gather_kernel<T>, dim3(gRn), dim3(256), 0, s, B, wd, m_r, h.d_rows_C.as<const T>(),
                               (const T*)w.rZout, (T*)Z, (const T*)nullptr, (T*)nullptr);
            break;
        }
    }
};

}  // namespace

}  // namespace nempc
