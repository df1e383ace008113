// nempc_extra_grad, host side, plain C++17 (no HIP): how many lanes share a row, what a row keeps in LDS, and whether the saved
// activation derivatives of the backward pass stay there or go to the handle's workspace -- decided before anything is
// launched.  kernels_egrad.hip launches what a plan names; tests/egrad_plan_check.cpp sweeps the plans over shapes on the CPU.
//
// A row is one (problem, step) pair.  A GROUP of `lanes` consecutive lanes of a wave (1, 16 or 64, from the widest layer) owns
// a row; a workgroup is ONE wave, so it holds 64 / lanes rows.  Per row, in elements of the handle's dtype:
//     X     4 maxdim   two buffers of (value | tangent) of a layer's input, forward; of a layer's cotangent, backward
//     K     4 nx       (k, k.) the stage's output and (kbar, kbar.) its cotangent from the later stage (RK4)
//     E     ne         the extras' cotangent, summed over the stages in the order 3, 2, 1, 0
//     SAVE  2 nstage sum_l out_l     s'(z) and s''(z) z. of every unit of every stage, forward to backward
// X, K and E are always in LDS.  SAVE is in LDS when the workgroup's total stays inside EG_LDS_BUDGET, else in the workspace:
// one region per resident workgroup, the grid then capped (the workgroups walk the rows with a grid stride).
// LDS layout: lanes == 1: slot-major, [slot][64 lanes] (lane i on bank i: no conflicts); lanes > 1: one block of `stride`
// elements per group, stride a multiple-of-32-dwords plus 16 so that the two groups of a 32-lane half read (broadcast) and
// write (16 consecutive units) on different banks.  The workspace regions use the same two layouts with stride = save_elems.
#pragma once

#include <cstddef>

#include "nempc.h"

namespace nempc {

constexpr size_t EG_LDS_BUDGET = 64 * 1024;          // SAVE joins X, K and E in LDS while the workgroup stays inside this
constexpr size_t EG_LDS_MAX = 144 * 1024;            // what X, K and E alone may take (1024-wide layers, nx = 1024, fp64: 74 KiB);
                                                     // a plan beyond it is refused (EgradPlan::fits)
constexpr long long EG_WS_BYTES = 128ll << 20;        // bound of the SAVE workspace (at least one workgroup's region)
constexpr int EG_WGS_PER_CU = 8;                      // workgroups per compute unit a capped grid aims for

// nempc_last_extra_grad_kernel: EG_LANES_* [+ EG_SAVE_WS]
enum EgradKernel { EGRAD_NONE = 0, EG_LANES_1 = 1, EG_LANES_16 = 2, EG_LANES_64 = 3, EG_SAVE_WS = 4 };

struct EgradShape {          // what the plan depends on, of a handle
    int nl, nstage, nx, ne, num_cus;
    int din[NEMPC_MAX_LAYERS], dout[NEMPC_MAX_LAYERS];
    size_t esz;
};

struct EgradPlan {
    int lanes;               // 1 | 16 | 64
    int rows_per_wg;         // 64 / lanes
    int maxdim;              // widest layer input or output
    int save_in_lds;
    long long x_elems;       // X + K + E per row
    long long save_elems;    // SAVE per row
    long long stride;        // lanes > 1: elements from one group's LDS block to the next; lanes == 1: slots per lane
    size_t lds_bytes;
    int fits;                // lds_bytes <= EG_LDS_MAX
    long long wg_ws_elems;   // workspace elements of one workgroup (0 when SAVE is in LDS)
    long long max_wgs;       // grid cap (0x7fffffff when SAVE is in LDS)
    int code;                // EgradKernel
};

inline long long egrad_pad_stride(long long elems, size_t esz) {      // smallest >= elems with (dwords % 32) == 16
    const long long per = (long long)(esz / 4);
    long long dw = elems * per;
    long long r = ((dw - 16) % 32 + 32) % 32;
    if (r) dw += 32 - r;
    return dw / per;
}

inline EgradPlan egrad_make_plan(const EgradShape& s) {
    EgradPlan p{};
    long long outs = 0;
    for (int l = 0; l < s.nl; ++l) {
        if (s.din[l] > p.maxdim) p.maxdim = s.din[l];
        if (s.dout[l] > p.maxdim) p.maxdim = s.dout[l];
        outs += s.dout[l];
    }
    p.lanes = p.maxdim <= 8 ? 1 : (p.maxdim <= 64 ? 16 : 64);
    p.rows_per_wg = 64 / p.lanes;
    p.x_elems = 4ll * p.maxdim + 4ll * s.nx + s.ne;
    p.save_elems = 2ll * s.nstage * outs;
    auto bytes = [&](long long per_row) {
        const long long st = p.lanes == 1 ? per_row : egrad_pad_stride(per_row, s.esz);
        return (size_t)(st * (p.lanes == 1 ? 64 : p.rows_per_wg)) * s.esz;
    };
    p.save_in_lds = bytes(p.x_elems + p.save_elems) <= EG_LDS_BUDGET;
    const long long per_row = p.x_elems + (p.save_in_lds ? p.save_elems : 0);
    p.stride = p.lanes == 1 ? per_row : egrad_pad_stride(per_row, s.esz);
    p.lds_bytes = bytes(per_row);
    p.fits = p.lds_bytes <= EG_LDS_MAX;
    p.code = (p.lanes == 1 ? EG_LANES_1 : (p.lanes == 16 ? EG_LANES_16 : EG_LANES_64)) + (p.save_in_lds ? 0 : EG_SAVE_WS);
    if (p.save_in_lds) {
        p.wg_ws_elems = 0;
        p.max_wgs = 0x7fffffffll;
    } else {
        p.wg_ws_elems = p.save_elems * p.rows_per_wg;
        long long cap = EG_WS_BYTES / (p.wg_ws_elems * (long long)s.esz);
        const long long want = (long long)EG_WGS_PER_CU * (s.num_cus < 1 ? 1 : s.num_cus);
        if (cap > want) cap = want;
        p.max_wgs = cap < 1 ? 1 : cap;
    }
    return p;
}

// workgroups of a call over `rows` rows
inline long long egrad_grid(const EgradPlan& p, long long rows) {
    const long long need = (rows + p.rows_per_wg - 1) / p.rows_per_wg;
    return need < p.max_wgs ? need : p.max_wgs;
}
// workspace elements of a handle whose largest call has `cap_rows` rows
inline long long egrad_ws_elems(const EgradPlan& p, long long cap_rows) { return p.wg_ws_elems * egrad_grid(p, cap_rows < 1 ? 1 : cap_rows); }
// element offset of SAVE slot `slot` (< save_elems) of group `grp` of workgroup `wg` in the workspace
inline long long egrad_ws_offset(const EgradPlan& p, long long wg, int grp, long long slot) {
    return wg * p.wg_ws_elems + (p.lanes == 1 ? slot * 64 + grp : (long long)grp * p.save_elems + slot);
}

}  // namespace nempc
