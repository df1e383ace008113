// included by kernels_mfma_f64.hip / kernels_mfma_f32.hip and their per-activation siblings (kernels_mfma_*_a<N>.hip)
// with NEMPC_T (double | float) and NEMPC_ACT (the hidden layers' NEMPC_ACT_* code) defined: one translation unit per
// (dtype, activation), each instantiating every kernel shape for that pair
#include <cstdlib>
#include <type_traits>

#include "kernels_coop_impl.h"
#include "kernels_coopfx_impl.h"
#include "kernels_hess_impl.h"
#include "kernels_hesscoop_impl.h"
#include "kernels_hessfx_impl.h"

namespace nempc {

namespace {
constexpr int kAct = NEMPC_ACT;          // this translation unit's activation
static_assert(FX_ZCOPY == kFxZcopy, "mfma_plan.h restates it");

// a plan names an instantiation this unit does not have: the plan and the unit disagree about the table (a bug)
int no_instantiation(const char* what, int wp, int nh) {
    set_error(std::string(what) + ": internal error: the plan names an instantiation this unit does not have (width " +
              std::to_string(wp) + ", " + std::to_string(nh) + " hidden layers, activation " + std::to_string(kAct) + ")");
    return NEMPC_EINVAL;
}

// entry `idx` of the table of compiled shapes (mfma_plan.h) as a compile-time constant: f(integral_constant<int, idx>)
template <typename F, size_t... I>
int with_compiled(int idx, F&& f, std::index_sequence<I...>) {
    int rc = NEMPC_EINVAL;
    const bool found = ((idx == (int)I ? (rc = f(std::integral_constant<int, (int)I>{}), true) : false) || ...);
    return found ? rc : no_instantiation("compiled shape", 0, idx);
}
using CompiledSeq = std::make_index_sequence<kNumCompiledShapes>;

// CU-cooperative kernel: weight slices in registers; LDS holds the exchange buffer, partials, per-tile scratch
template <typename T, int WP, int NH, int TPW, bool SR = false, int NXc = 0, int NUc = 0>
int launch_coop(const MfmaParams& p, const MfmaRowsPlan& plan, hipStream_t s) {
    constexpr int MT = WP / 16;
    const int NR = coop_nr<T>(p.nin);
    const CoopLayout& lay = plan.lay;
    const size_t bytes = plan.g.lds_bytes;
    auto kern = rows_coop_kernel<T, WP, NH, TPW, SR, 2, kAct, NXc, NUc>;
    {
        hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), bytes);
        if (e != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(coop)");
    }
    const int grid = plan.g.grid;
    const int scratch2 = lay.scratch2, rowinfo2 = lay.rowinfo2;
    const LaunchGeom& gp = plan.g;
    // every constant the kernel uses, computed here once (the kernel does no setup arithmetic)
    constexpr int VEC = 16 / (int)sizeof(T);
    const T* blob = static_cast<const T*>(p.blob);
    const size_t R = (size_t)p.B * p.H;
    CoopArgs a{};
    a.Z = p.Z; a.X0 = p.X0; a.extra = p.extra;
    a.small = blob + p.off.coop_small;
    a.wslice = blob + p.off.coop_slices;
    a.tiles_per_wg = gp.tiles_per_wg;
    a.tiles_rem = gp.tiles_rem;
    a.R = (unsigned)R;
    a.invH = p.H == 1 ? 0u : (unsigned)((0x100000000ull + (unsigned)p.H - 1) / (unsigned)p.H);
    a.H = p.H; a.n = p.gk.n; a.nx = p.nx; a.nu = p.nu; a.nin = p.nin; a.ne = p.ne;
    a.small_vecs = (p.off.coop_small_elems + VEC - 1) / VEC;
    a.nload = p.off.coop_nload;
    a.early = (p.gk.w == 1 && (p.nin + p.nx + p.ne) * TPW * 16 <= StageRegs<T, MT, TPW>::ITEMS * MT * 64) ? 1 : 0;
    a.l_w0f = lay.w0f; a.l_tail = lay.w0f + p.ks * MT * 64; a.l_x = lay.x; a.l_xhalf = lay.xhalf; a.l_part = lay.part;
    a.l_scratch = lay.scratch; a.l_rowinfo = lay.rowinfo; a.l_scratch2 = scratch2; a.l_rowinfo2 = rowinfo2;
    for (int l = 0; l < NEMPC_MFMA_MAX_HIDDEN; ++l) a.bias_off[l] = p.off.bias[l] - p.off.seed;
    a.acts = p.acts;
    a.biasL_off = p.off.biasL - p.off.seed;
    a.g = p.g; a.tiles = p.tiles; a.stage_out = p.stage_out; a.dbg = p.dbg;
    a.jac = p.fuse_obj ? nullptr : p.fuse_jac;       // dense rows from this launch (ROW_COOP_DENSE)
    a.sp = p.fuse_obj ? nullptr : p.fuse_sparse;     // ... or the band values (sparse contract, ROW_COOP_SPARSE)
    a.sp_nnz = p.sp_nnz;
    if (!p.fuse_obj && p.obj && (p.fuse_f || p.fuse_grad)) {     // ... and the objective
        a.obj_f = p.fuse_f; a.obj_grad = p.fuse_grad; a.obj_P = p.obj; a.oo = p.oo; a.B = p.B;
    }
    a.m = p.m; a.NR = NR; a.jsz = 16 * p.nx * p.nin; a.spt = p.scratch_per_wave;
    a.rk4 = p.kind == NEMPC_RK4 ? 1 : 0;
    a.nstages = a.rk4 ? 4 : 1;
    a.ks = p.ks; a.kind = p.kind; a.box = p.box;
    a.xt_off = 16 * p.nin + 2 * 16 * p.nx + (a.rk4 ? 4 : 1) * a.jsz;   // after the wave-tile kernel's carve-up
    a.ex_off = a.xt_off + 16 * p.nx;                                    // [16][ne] extra inputs
    a.inv_nin = (65536 + p.nin - 1) / p.nin;                            // kd / nin == (kd * inv_nin) >> 16 for kd < 256
    a.stage_stride = p.stage_stride;
    a.inv32_jrow = (unsigned)((0x100000000ull + (unsigned)(p.nx * p.nin) - 1) / (unsigned)(p.nx * p.nin));
    a.inv32_nx = (unsigned)((0x100000000ull + (unsigned)p.nx - 1) / (unsigned)p.nx);
    a.DT = p.DT;
    a.gk = p.gk;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(MT * 64), bytes, s, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? NEMPC_OK : hip_fail(e, "rows_coop_kernel launch");
}

// fixed-shape cooperative kernel (kernels_coopfx_impl.h): plain Discret / Unity models of one of the compiled shapes
template <typename T, int WP, int NH, int TPW, int NX, int NU, bool FUSE, bool GN = false>
int launch_coopfx(const MfmaParams& p, const MfmaRowsPlan& plan, hipStream_t s) {
    using L = FxLayout<T, WP, NH, TPW, NX, NU>;
    static_assert(L::TOTAL == fx_lds_elems(WP, NH, TPW, NX, NU), "mfma_plan.h restates the layout's size");
    constexpr int MT = WP / 16;
    constexpr int VEC = 16 / (int)sizeof(T);
    const int p_elems = FUSE ? p.oo.total : 0;
    const size_t bytes = plan.g.lds_bytes;      // (layout + objective table + two Z copies: own + partner's problems)
    auto kern = rows_coopfx_kernel<T, WP, NH, TPW, NX, NU, FUSE, kAct, GN>;
    NEMPC_HIP(ensure_dynamic_lds(reinterpret_cast<const void*>(kern), bytes));
    const LaunchGeom& gp = plan.g;
    const int grid = gp.grid;
    const T* blob = static_cast<const T*>(p.blob);
    FxArgs a{};
    a.Z = p.Z; a.X0 = p.X0;
    a.small = blob + p.off.fx_small;
    a.wslice = blob + p.off.coop_slices;
    a.tiles_per_wg = gp.tiles_per_wg;
    a.tiles_rem = gp.tiles_rem;
    a.R = (unsigned)((size_t)p.B * p.H);
    a.invH = p.H == 1 ? 0u : (unsigned)((0x100000000ull + (unsigned)p.H - 1) / (unsigned)p.H);
    a.H = p.H; a.n = p.gk.n; a.m = p.m;
    a.ident = p.kind == NEMPC_DISCRET ? 1 : 0;
    a.box = (p.box ? FX_BOX_ROWS : 0) | (FUSE && p.jac_resident ? FX_BOX_CONST_RESIDENT : 0);
    a.small_vecs = (p.off.fx_small_elems + VEC - 1) / VEC;
    a.g = p.g; a.tiles = p.tiles;
    a.jac = p.fuse_jac; a.f = p.fuse_f; a.grad = p.fuse_grad; a.P = p.obj; a.p_elems = p_elems; a.oo = p.oo;
    a.jac_sp = FUSE ? p.fuse_sparse : nullptr; a.sp_nnz = p.sp_nnz;
    a.dbg = p.dbg;
    if (GN) {
        a.gn_hvals = p.gn_hvals; a.gn_sigma = p.gn_sigma; a.gn_w = p.gn_w; a.gn_smap = p.gn_smap; a.gn_objc = p.gn_objc;
        a.gn_nnz = p.gn_nnz; a.gn_n_orph = p.gn_n_orph;
    }
    a.zp_max = plan.zp_max;
    // the leading arguments (preloaded into scalar registers) repeat what the prologue's loads depend on; three small
    // integers and the two "objective wanted" bits share a dword, the horizon and the grid size another (the kernel pairs
    // workgroup i with i + ceil(grid / 2) for the objective and must not wait for the dispatch's own copy of the grid size)
    const unsigned pack = (unsigned)a.tiles_per_wg | ((unsigned)a.tiles_rem << 8) | ((unsigned)a.zp_max << 18) |
                          (a.f ? 1u << 28 : 0u) | (a.grad ? 1u << 29 : 0u) | ((a.tiles || a.jac || a.jac_sp || GN) ? 1u << 30 : 0u) |
                          (p.box ? 1u << 31 : 0u);
    // pjac is the pointer the background zeros go to (the non-zeros go to a.jac, read in the epilogue).  A resident matrix
    // (nempc_jac_dense_resident) holds its zeros already, and its constant -1 / +1 entries: the kernel is told there is no
    // background to write, and the epilogue leaves the constants out (a second bit in a.box, which it reads anyway: keeping
    // the pointer itself live to the end of the pass cost the sparse contract two spilled scalars).  Same kernel, no new
    // argument; what is left of the background is the epilogue's vmcnt(0), which then finds only the
    // next pass's input loads (waited for two lines further down anyway) and the previous pass's few stores outstanding.
    void* const bg = FUSE && !p.jac_resident ? a.jac : nullptr;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(MT * 64), bytes, s, a.Z, a.X0, a.small, a.wslice, a.P, pack, a.R, a.invH,
                       (unsigned)a.H | ((unsigned)grid << 16), bg, a);
    NEMPC_HIP(hipGetLastError());
    return NEMPC_OK;
}

template <typename T, int WP, int NH>
int launch_coop_shape(const MfmaParams& p, const MfmaRowsPlan& plan, hipStream_t s) {
    if constexpr (coop_fits_registers((int)sizeof(T), WP, NH)) {
        if (plan.stage_records && plan.tpw == 1) return launch_coop<T, WP, NH, 1, true>(p, plan, s);
        if constexpr (WP <= 64) {
            if (!plan.stage_records && plan.tpw == 3) return launch_coop<T, WP, NH, 3>(p, plan, s);
            if (!plan.stage_records && plan.tpw == 2) return launch_coop<T, WP, NH, 2>(p, plan, s);
        }
        if (!plan.stage_records && plan.tpw == 1) return launch_coop<T, WP, NH, 1>(p, plan, s);
    }
    return no_instantiation("rows_coop_kernel", WP, NH);
}

template <typename T, int WP, int NH>
int launch_tile_shape(const MfmaParams& p, const MfmaRowsPlan& plan, hipStream_t s) {
    if constexpr (tile_weights_resident((int)sizeof(T), WP, NH)) {
        if (plan.resident) return launch_one<T, WP, NH, true, kMaxWaves, kAct>(p, plan.waves, plan.g.grid, plan.g.lds_bytes, s);
    }
    // (Round 3 kept three of these streamed instantiations -- fp32 128-wide 2 layers, fp64 128-wide 2 layers, fp64 64-wide
    // 3 layers -- away from the launcher because they returned wrong rows.  The cause was a spill store the compiler had put
    // in front of an exec restore; the build repairs that placement and checks every kernel for it: _isa.py, DESIGN.md.)
    if (!plan.resident) return launch_one<T, WP, NH, false, 4, kAct>(p, plan.waves, plan.g.grid, plan.g.lds_bytes, s);
    return no_instantiation("rows_mfma_kernel", WP, NH);
}
}  // namespace

#define NEMPC_SHAPES(CASE)                                                                   \
    CASE(32, 1) CASE(32, 2) CASE(32, 3) CASE(64, 1) CASE(64, 2) CASE(64, 3) CASE(128, 1) CASE(128, 2) CASE(128, 3) \
    CASE(32, 4) CASE(64, 4)          /* a fourth hidden layer up to width 64 */

template <>
int launch_rows_mfma_act<NEMPC_T, NEMPC_ACT>(const MfmaParams& p, const MfmaRowsPlan& plan, hipStream_t s) {
    using T = NEMPC_T;
    if (plan.family == FAM_FX)
        return with_compiled(plan.compiled, [&](auto i) {
            constexpr CompiledShape c = kCompiledShapes[decltype(i)::value];
            if constexpr (c.kind == CK_FX && compiled_has(c, (int)sizeof(T), kAct)) {
                const bool t3 = plan.tpw == 3;
                if (plan.gn) {
                    // Gauss-Newton callback in one launch (tril values): fp64, two states (the epilogue sums the states by a quad permute)
                    if constexpr (sizeof(T) == 8 && c.nx == 2)
                        return t3 ? launch_coopfx<T, c.wp, c.nh, 3, c.nx, c.nu, false, true>(p, plan, s)
                                  : launch_coopfx<T, c.wp, c.nh, 2, c.nx, c.nu, false, true>(p, plan, s);
                    else return no_instantiation("rows_coopfx_kernel (Gauss-Newton)", c.wp, c.nh);
                }
                if (plan.fuse)
                    return t3 ? launch_coopfx<T, c.wp, c.nh, 3, c.nx, c.nu, true>(p, plan, s)
                              : launch_coopfx<T, c.wp, c.nh, 2, c.nx, c.nu, true>(p, plan, s);
                return t3 ? launch_coopfx<T, c.wp, c.nh, 3, c.nx, c.nu, false>(p, plan, s)
                          : launch_coopfx<T, c.wp, c.nh, 2, c.nx, c.nu, false>(p, plan, s);
            } else {
                return no_instantiation("rows_coopfx_kernel", c.wp, c.nh);
            }
        }, CompiledSeq{});
    if (plan.family == FAM_COOP && plan.compiled >= 0)      // nx / nu as compile-time constants, one tile per pass
        return with_compiled(plan.compiled, [&](auto i) {
            constexpr CompiledShape c = kCompiledShapes[decltype(i)::value];
            if constexpr (c.kind == CK_COOP_DIMS && compiled_has(c, (int)sizeof(T), kAct))
                return plan.stage_records ? launch_coop<T, c.wp, c.nh, 1, true, c.nx, c.nu>(p, plan, s)
                                          : launch_coop<T, c.wp, c.nh, 1, false, c.nx, c.nu>(p, plan, s);
            else return no_instantiation("rows_coop_kernel (compiled dimensions)", c.wp, c.nh);
        }, CompiledSeq{});
    const int width = plan.wp, nh = plan.nh;
#define NEMPC_CASE(WPV, NHV)                                                                          \
    if (width == WPV && nh == NHV)                                                                    \
        return plan.family == FAM_COOP ? launch_coop_shape<T, WPV, NHV>(p, plan, s) : launch_tile_shape<T, WPV, NHV>(p, plan, s);
    if (plan.family == FAM_COOP || plan.family == FAM_TILE) { NEMPC_SHAPES(NEMPC_CASE) }
#undef NEMPC_CASE
    return no_instantiation("row kernel", width, nh);
}

namespace {
// wave-per-tile Hessian kernel: one wave per SIMD (the kernel needs > 256 registers)
template <typename T, int WP, int NH, bool WLDS>
int launch_hess_one(const HessParams& hp, const MfmaHessPlan& plan, hipStream_t s) {
    auto kern = rowhess_mfma_kernel<T, WP, NH, WLDS, kAct>;
    NEMPC_HIP(ensure_dynamic_lds(reinterpret_cast<const void*>(kern), plan.g.lds_bytes));
    hipLaunchKernelGGL(kern, dim3(plan.g.grid), dim3(plan.g.wg), plan.g.lds_bytes, s, hp);
    NEMPC_HIP(hipGetLastError());
    return NEMPC_OK;
}
template <typename T, int WP, int NH>
int launch_hess_tile(const HessParams& hp, const MfmaHessPlan& plan, hipStream_t s) {
    if constexpr (tile_weights_resident((int)sizeof(T), WP, NH)) {
        if (plan.resident) return launch_hess_one<T, WP, NH, true>(hp, plan, s);
    }
    return plan.resident ? no_instantiation("rowhess_mfma_kernel", WP, NH) : launch_hess_one<T, WP, NH, false>(hp, plan, s);
}

template <typename T, int WP, int NH>
int launch_hess_coop(const HessParams& hp, const MfmaHessPlan& plan, hipStream_t s) {
    if constexpr (coop_fits_registers((int)sizeof(T), WP, NH)) {
        constexpr int MT = WP / 16;
        auto kern = rowhess_coop_kernel<T, WP, NH, kHessTG, kAct>;
        hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), plan.g.lds_bytes);
        if (e != hipSuccess) return hip_fail(e, "hipFuncSetAttribute(hess coop)");
        HessParams hc = hp;
        hc.base.tiles_per_wg = plan.g.tiles_per_wg;
        hc.base.tiles_rem = plan.g.tiles_rem;
        hipLaunchKernelGGL(kern, dim3(plan.g.grid), dim3(MT * 64), plan.g.lds_bytes, s, hc, plan.lay);
        e = hipGetLastError();
        return e == hipSuccess ? NEMPC_OK : hip_fail(e, "rowhess_coop_kernel launch");
    } else {
        return no_instantiation("rowhess_coop_kernel", WP, NH);
    }
}

// fixed-shape Hessian kernel (kernels_hessfx_impl.h): plain Discret / Unity models of a compiled shape
template <typename T, int WP, int NH, int NT, int NX, int NU, int TG = NX + NU, bool RWB = false, bool EV = false>
int launch_hessfx(const HessParams& hp, const MfmaHessPlan& plan, hipStream_t s) {
    using L = HfxLayout<T, WP, NH, NT, NX, NU, TG, EV>;
    static_assert(L::TOTAL == hfx_lds_elems(WP, NH, NT, NX, NU, TG, EV), "mfma_plan.h restates the layout's size");
    constexpr int MT = WP / 16;
    const MfmaParams& p = hp.base;
    const size_t bytes = plan.g.lds_bytes;
    auto kern = rowhess_coopfx_kernel<T, WP, NH, NT, NX, NU, kAct, TG, RWB, EV>;
    NEMPC_HIP(ensure_dynamic_lds(reinterpret_cast<const void*>(kern), bytes));
    const LaunchGeom& gp = plan.g;
    const T* blob = static_cast<const T*>(p.blob);
    HfxArgs a{};
    a.Z = p.Z; a.X0 = p.X0; a.lambda = hp.lambda;
    a.small = blob + p.off.fx_small;
    a.wslice = blob + p.off.coop_slices;
    a.tiles_per_wg = gp.tiles_per_wg; a.tiles_rem = gp.tiles_rem;
    a.R = (unsigned)((size_t)p.B * p.H * (hp.xi_direct ? hp.vdiv : 1));
    a.invH = p.H == 1 ? 0u : (unsigned)((0x100000000ull + (unsigned)p.H - 1) / (unsigned)p.H);
    a.H = p.H; a.n = p.gk.n; a.m = p.m;
    a.nload = p.off.coop_nload;
    a.xi_direct = hp.xi_direct; a.lam_direct = hp.lam_direct; a.xi_stride = hp.xi_stride;
    a.blocks = hp.blocks;
    a.hvals = hp.hvals; a.sigma = hp.sigma; a.smap = hp.smap; a.objc = hp.objc; a.nnz = hp.nnz; a.n_orph = hp.n_orph;
    a.g_out = hp.ev_g; a.tiles_out = hp.ev_tiles; a.ident = p.kind == NEMPC_DISCRET ? 1 : 0;
    hipLaunchKernelGGL(kern, dim3(gp.grid), dim3(MT * 64), bytes, s, a);
    NEMPC_HIP(hipGetLastError());
    return NEMPC_OK;
}
}  // namespace

template <>
int launch_rowhess_mfma_act<NEMPC_T, NEMPC_ACT>(const HessParams& hp, const MfmaHessPlan& plan, hipStream_t s) {
    using T = NEMPC_T;
    if (plan.family == FAM_FX)
        return with_compiled(plan.compiled, [&](auto i) {
            constexpr CompiledShape c = kCompiledShapes[decltype(i)::value];
            if constexpr (c.kind == CK_FX && compiled_has(c, (int)sizeof(T), kAct)) {
                constexpr int TG = c.nx + c.nu;
                return plan.ev ? launch_hessfx<T, c.wp, c.nh, 1, c.nx, c.nu, TG, false, true>(hp, plan, s)
                               : launch_hessfx<T, c.wp, c.nh, 1, c.nx, c.nu>(hp, plan, s);
            } else if constexpr (c.kind == CK_HESS_DIMS && compiled_has(c, (int)sizeof(T), kAct)) {
                // three tangent directions per exchange
                return launch_hessfx<T, c.wp, c.nh, 1, c.nx, c.nu, 3, true>(hp, plan, s);
            } else {
                return no_instantiation("rowhess_coopfx_kernel", c.wp, c.nh);
            }
        }, CompiledSeq{});
    const int width = plan.wp, nh = plan.nh;
#define NEMPC_HCASE(WPV, NHV)                                                                         \
    if (width == WPV && nh == NHV)                                                                    \
        return plan.family == FAM_COOP ? launch_hess_coop<T, WPV, NHV>(hp, plan, s) : launch_hess_tile<T, WPV, NHV>(hp, plan, s);
    if (plan.family == FAM_COOP || plan.family == FAM_TILE) { NEMPC_SHAPES(NEMPC_HCASE) }
#undef NEMPC_HCASE
    return no_instantiation("Hessian kernel", width, nh);
}
#undef NEMPC_SHAPES

}  // namespace nempc
