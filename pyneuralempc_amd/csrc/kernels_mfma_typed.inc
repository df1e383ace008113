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
constexpr int kLdsBudget = 150 * 1024;  // of the CU's 160 KiB
constexpr int kLdsBudgetCoop = 160 * 1024;
constexpr int kMaxWaves = 8;            // 512 threads: keeps 256 VGPRs per lane available
// A/B knobs read at two sites each: NEMPC_COOP_DIMS=0 keeps the 6/3 3x128 fp32 rows off their compiled-dimension
// cooperative kernel, NEMPC_HFX=0 the Lagrangian blocks off the fixed-shape kernels
inline int coop_dims_on() { static const int on = env_int("NEMPC_COOP_DIMS", 1); return on; }
inline int hfx_on() { static const int on = env_int("NEMPC_HFX", 1); return on; }

// CU-cooperative kernel: weight slices in registers; LDS holds the exchange buffer, partials, per-tile scratch
template <typename T, int WP, int NH, int TPW, bool SR = false, int OCC = 2, int NXc = 0, int NUc = 0>
bool try_launch_coop(const MfmaParams& p, hipStream_t s, int* rc) {
    constexpr int MT = WP / 16;
    const int NR = coop_nr<T>(p.nin);
    auto up16 = [](int v) { return (v + 15) & ~15; };
    CoopLayout lay{};
    int q = 0;
    lay.w0f = q; q += p.ks * MT * 64;                      // [w0f | tail] contiguous: one flat copy of off.coop_small
    lay.tail = q; q += up16(p.off.total - p.off.seed);
    lay.x = q; lay.xhalf = coop_slots<T>(TPW) * MT * 256; q += 2 * lay.xhalf;
    lay.part = q; q += up16((1 + p.nx) * TPW * MT * NR * 64);
    lay.scratch = q; q += up16(TPW * p.scratch_per_wave);
    const int scratch2 = q; q += up16(TPW * p.scratch_per_wave);           // second buffer (next pass's inputs)
    lay.rowinfo = q; q += up16(TPW * 16 * 2 * (int)sizeof(int) / (int)sizeof(T) + 1);
    const int rowinfo2 = q; q += up16(TPW * 16 * 2 * (int)sizeof(int) / (int)sizeof(T) + 1);
    lay.total = q;
    const size_t bytes = (size_t)lay.total * sizeof(T);
    const int wg_by_regs = OCC * 4 / MT;  // __launch_bounds__(MT*64, OCC): OCC waves per SIMD
    int per_cu = (int)((size_t)kLdsBudgetCoop / bytes);
    if (per_cu < 1) return false;
    if (per_cu > wg_by_regs) per_cu = wg_by_regs;
    if (per_cu < wg_by_regs && TPW > 1) return false;  // prefer a smaller pass that keeps two waves per SIMD
    auto kern = rows_coop_kernel<T, WP, NH, TPW, SR, OCC, kAct, NXc, NUc>;
    {
        hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), bytes);
        if (e != hipSuccess) { *rc = hip_fail(e, "hipFuncSetAttribute(coop)"); return true; }
    }
    const GridPlan gp = plan_grid(p.ntiles, p.num_cus, per_cu);
    const int grid = gp.grid;
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
    a.jac = p.fuse_obj ? nullptr : p.fuse_jac;       // dense rows from this launch (launch_rows_mfma_dense)
    a.sp = p.fuse_obj ? nullptr : p.fuse_sparse;     // ... or the band values (sparse contract, launch_rows_mfma_sparse)
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
    *rc = e == hipSuccess ? NEMPC_OK : hip_fail(e, "rows_coop_kernel launch");
    return true;
}

// fixed-shape cooperative kernel (kernels_coopfx_impl.h): plain Discret / Unity models of one of the compiled shapes
template <typename T, int WP, int NH, int TPW, int NX, int NU, bool FUSE, bool GN = false>
int launch_coopfx(const MfmaParams& p, hipStream_t s) {
    using L = FxLayout<T, WP, NH, TPW, NX, NU>;
    constexpr int MT = WP / 16;
    constexpr int VEC = 16 / (int)sizeof(T);
    const int p_elems = FUSE ? p.oo.total : 0;
    const size_t bytes = (size_t)(L::TOTAL + ((p_elems + 15) & ~15) + (FUSE ? 2 * FX_ZCOPY : 0)) * sizeof(T);   // (two Z copies: own + partner's problems)
    auto kern = rows_coopfx_kernel<T, WP, NH, TPW, NX, NU, FUSE, kAct, GN>;
    NEMPC_HIP(ensure_dynamic_lds(reinterpret_cast<const void*>(kern), bytes));
    int per_cu = (int)((size_t)kLdsBudgetCoop / bytes);
    if (per_cu > 8 / MT) per_cu = 8 / MT;
    if (per_cu < 1) per_cu = 1;
    const GridPlan gp = plan_grid(p.ntiles, p.num_cus, per_cu);
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
    a.box = p.box;
    a.small_vecs = (p.off.fx_small_elems + VEC - 1) / VEC;
    a.g = p.g; a.tiles = p.tiles;
    a.jac = p.fuse_jac; a.f = p.fuse_f; a.grad = p.fuse_grad; a.P = p.obj; a.p_elems = p_elems; a.oo = p.oo;
    a.jac_sp = FUSE ? p.fuse_sparse : nullptr; a.sp_nnz = p.sp_nnz;
    a.dbg = p.dbg;
    if (GN) {
        a.gn_hvals = p.gn_hvals; a.gn_sigma = p.gn_sigma; a.gn_w = p.gn_w; a.gn_smap = p.gn_smap; a.gn_objc = p.gn_objc;
        a.gn_nnz = p.gn_nnz; a.gn_n_orph = p.gn_n_orph;
    }
    if (FUSE) {
        // the background zeros of a pass's dense rows leave as flat runs of 16-byte vectors with 32-bit byte offsets
        const int nvec = p.gk.n / VEC;
        // the objective table must be complete in LDS before the first pass for the LDS-resident problems
        // (... and a side's copy of Z is fetched as two elements per thread)
        a.zp_max = p_elems <= 2 * MT * 64 ? (FX_ZCOPY < 2 * MT * 64 ? FX_ZCOPY : 2 * MT * 64) / p.gk.n : 0;
        if (a.jac && (nvec < 1 || p.gk.n % VEC != 0 || (size_t)(TPW * 16 * NX) * p.gk.n * sizeof(T) >= 0x7fffffffull))
            return NEMPC_EUNSUPPORTED;
    }
    // the leading arguments (preloaded into scalar registers) repeat what the prologue's loads depend on; three small
    // integers and the two "objective wanted" bits share a dword, the horizon and the grid size another (the kernel pairs
    // workgroup i with i + ceil(grid / 2) for the objective and must not wait for the dispatch's own copy of the grid size)
    if (a.tiles_per_wg > 0xff || a.tiles_rem > 0x3ff || a.zp_max > 0x3ff || a.n != p.H * (NX + NU) || p.H > 0xffff || grid > 0xffff)
        return NEMPC_EUNSUPPORTED;
    const unsigned pack = (unsigned)a.tiles_per_wg | ((unsigned)a.tiles_rem << 8) | ((unsigned)a.zp_max << 18) |
                          (a.f ? 1u << 28 : 0u) | (a.grad ? 1u << 29 : 0u) | ((a.tiles || a.jac || a.jac_sp || GN) ? 1u << 30 : 0u) |
                          (a.box ? 1u << 31 : 0u);
    // pjac is the pointer the background zeros go to (the non-zeros go to a.jac, read in the epilogue).  A resident matrix
    // (nempc_jac_dense_resident) holds its zeros already: the kernel is told there is no background to write.  Same kernel,
    // same registers, no new argument; what is left of the background is the epilogue's vmcnt(0), which then finds only the
    // next pass's input loads (waited for two lines further down anyway) and the previous pass's few stores outstanding.
    void* const bg = FUSE && !p.jac_resident ? a.jac : nullptr;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(MT * 64), bytes, s, a.Z, a.X0, a.small, a.wslice, a.P, pack, a.R, a.invH,
                       (unsigned)a.H | ((unsigned)grid << 16), bg, a);
    NEMPC_HIP(hipGetLastError());
    return NEMPC_OK;
}

// register budget of the weight slices: (NH-1) * 2 * MT*4 + 8 values per lane
template <typename T, int WP, int NH>
constexpr bool coop_fits_registers() {
    return ((NH - 1) * 2 * (WP / 16) * 4 + 8) * (int)(sizeof(T) / 4) <= 144;
}

template <typename T, int WP, int NH>
int launch_shape(const MfmaParams& p, bool allow_coop, hipStream_t s, int* kernel_used) {
    const size_t esz = sizeof(T);
    *kernel_used = 3;
    if constexpr (coop_fits_registers<T, WP, NH>()) {
        // Beyond ~8 tiles per SIMD the wave-per-tile kernel with two waves per SIMD is ahead (B=16384, C2 dims:
        // 209 us vs 238 us); below, the cooperative kernel's even split wins (B=256: 12.9 vs 16.5 us).
        constexpr size_t hh_lds = (size_t)(NH - 1) * 2 * (WP / 16) * (WP / 16) * 256 * sizeof(T);
        const bool tile_kernel_resident = hh_lds <= 96 * 1024;
        if (allow_coop && p.stage_out) {
            // RK4 Hessian pipeline: the stage-record instantiation, one tile per pass
            int rc = NEMPC_OK;
            if constexpr (WP == 128 && NH == 3 && sizeof(T) == 4) {
                if (coop_dims_on() && p.nx == 6 && p.nu == 3 && p.nin == 9 && p.gk.w == 1 &&
                    try_launch_coop<T, WP, NH, 1, true, 2, 6, 3>(p, s, &rc)) {
                    *kernel_used = 2;
                    return rc;
                }
            }
            if (try_launch_coop<T, WP, NH, 1, true>(p, s, &rc)) {
                *kernel_used = 2;
                return rc;
            }
        } else if (allow_coop && !(tile_kernel_resident && p.ntiles > 32 * p.num_cus)) {   // (8 tiles per SIMD)
            int rc = NEMPC_OK;
            // passes of <= 3 tiles: the 4-tile instantiation sits at the 256-VGPR cap of two waves per SIMD and
            // spills (each scratch access is a memory round trip on the critical path of a ~45k-cycle launch)
            if constexpr (WP <= 64) {
                // fp64 2x64 and larger: the 3-tile instantiation sits at the 256-VGPR cap and spills; measured 21.2 us
                // against 20.4 us for 2-tile passes at C2 dims (B=1024).  NEMPC_COOP_TPW is an A/B knob.
                constexpr int tpw_default = (sizeof(T) == 8 && WP >= 64 && NH >= 2) ? 2 : 3;
                static const int tpw_cap = env_int("NEMPC_COOP_TPW", tpw_default);
#ifdef NEMPC_EXP_OCC3   // experiment: three workgroups per CU, single-tile passes
                if constexpr (sizeof(T) == 8 && WP == 64 && NH == 2) {
                    if (try_launch_coop<T, WP, NH, 1, false, 3>(p, s, &rc)) { *kernel_used = 2; return rc; }
                }
#endif
                if ((tpw_cap >= 3 && try_launch_coop<T, WP, NH, 3>(p, s, &rc)) ||
                    (tpw_cap >= 2 && try_launch_coop<T, WP, NH, 2>(p, s, &rc))) {
                    *kernel_used = 2;
                    return rc;
                }
            }
            // width 128 = 8 waves per workgroup (two per SIMD): one tile per pass is what LDS and registers allow
            // (BASELINE configs[2] dims -- 6 states, 3 controls, plain model -- as compile-time constants)
            if constexpr (WP == 128 && NH == 3 && sizeof(T) == 4) {
                if (coop_dims_on() && p.nx == 6 && p.nu == 3 && p.nin == 9 && p.gk.w == 1 &&
                    try_launch_coop<T, WP, NH, 1, false, 2, 6, 3>(p, s, &rc)) {
                    *kernel_used = 2;
                    return rc;
                }
            }
            if (try_launch_coop<T, WP, NH, 1>(p, s, &rc)) {
                *kernel_used = 2;
                return rc;
            }
        }
    }
    if ((p.fuse_jac || p.fuse_sparse) && !p.fuse_obj) return NEMPC_EUNSUPPORTED;     // dense rows / band values leave from the cooperative kernel only
    const size_t blob_bytes = (size_t)((p.off.total + 1) & ~1) * esz;
    const size_t scratch = (size_t)p.scratch_per_wave * esz;
    // weights resident in LDS when they fit next to the per-wave scratch: one workgroup per CU,
    // as many waves as it takes to cover the tiles with <= 256 workgroups
    // hidden-to-hidden fragment arrays alone must leave room for the rest of the blob + scratch
    constexpr size_t hh_bytes = (size_t)(NH - 1) * 2 * (WP / 16) * (WP / 16) * 256 * sizeof(T);
    if constexpr (hh_bytes <= 96 * 1024) {
        int waves = (p.ntiles + p.num_cus - 1) / p.num_cus;
        waves = waves < 1 ? 1 : (waves > kMaxWaves ? kMaxWaves : waves);
        if (blob_bytes + (size_t)waves * scratch <= (size_t)kLdsBudget) {
            int grid = (p.ntiles + waves - 1) / waves;
            if (grid > p.num_cus) grid = p.num_cus;
            return launch_one<T, WP, NH, true, kMaxWaves, kAct>(p, waves, grid, blob_bytes + waves * scratch, s);
        }
    }
    // (Round 3 kept three of these streamed instantiations -- fp32 128-wide 2 layers, fp64 128-wide 2 layers, fp64 64-wide
    // 3 layers -- away from the launcher because they returned wrong rows.  The cause was a spill store the compiler had put
    // in front of an exec restore; the build repairs that placement and checks every kernel for it: _isa.py, DESIGN.md.)
    static const int waves_env = env_int("NEMPC_TILE_WAVES", 4);   // A/B knob
    int waves = waves_env < 1 ? 1 : (waves_env > 4 ? 4 : waves_env);
    while (waves > 1 && (size_t)waves * scratch > (size_t)kLdsBudget) waves >>= 1;
    const int grid = (p.ntiles + waves - 1) / waves;
    return launch_one<T, WP, NH, false, 4, kAct>(p, waves, grid, (size_t)waves * scratch, s);
}

// ---- the table of compiled fixed shapes (fast-path coverage by shape, not by hand).  One entry = (padded width, hidden
//      layers, nx, nu); every entry has the three row-kernel variants (plain, fused evaluation, Gauss-Newton callback in
//      fp64) and the fixed-shape Hessian kernel (launch_rowhess_mfma_act).  Every activation: BASELINE configs[1] /
//      configs[4] (2/1, 2 x 64, fp64).  tanh only (compile time): the reference's own example network 3 -> 30 -> 30 -> 2
//      (examples/lotka_volterra/run.py:64-98, nn_model.h5: padded width 32) in both precisions, and 2/1 2 x 64 in fp32.
template <int WP_, int NH_, int NX_, int NU_>
struct FxShape {
    static constexpr int WP = WP_, NH = NH_, NX = NX_, NU = NU_;
};
template <typename... S>
struct FxList {};
template <typename T>
struct FxTableSel;
template <>
struct FxTableSel<double> {
    using all_acts = FxList<FxShape<64, 2, 2, 1>>;
    using tanh_only = FxList<FxShape<64, 2, 2, 1>, FxShape<32, 2, 2, 1>>;
};
template <>
struct FxTableSel<float> {
    using all_acts = FxList<>;
    using tanh_only = FxList<FxShape<64, 2, 2, 1>, FxShape<32, 2, 2, 1>>;
};
template <typename T>
using FxTable = std::conditional_t<kAct == NEMPC_ACT_RUNTIME, FxList<>,      // (run-time activations: the run-time-dims kernels only)
                                   std::conditional_t<kAct == NEMPC_ACT_TANH, typename FxTableSel<T>::tanh_only,
                                                      typename FxTableSel<T>::all_acts>>;

template <typename T, typename SH>
bool fx_shape_matches(const Handle& h, const MfmaParams& p) {
    static const int fx_on = env_int("NEMPC_FX", 1);
    constexpr int MT = SH::WP / 16;
    return fx_on && h.variant != NEMPC_KERNEL_MFMA_TILE && p.mb == 1 && p.ks <= 4 &&
           (unsigned long long)p.B * p.H * p.H < 0x100000000ull && h.mfma.wp == SH::WP && h.mfma.nh == SH::NH && p.nx == SH::NX &&
           p.nu == SH::NU && p.nin == SH::NX + SH::NU && p.ne == 0 && p.gk.w == 1 && p.kind != NEMPC_RK4 && !p.stage_out &&
           p.ntiles <= 254 * (8 / MT) * p.num_cus;   // (workgroups per CU x 255 tiles: the packed per-workgroup tile count)
}

template <typename T>
int fx_rows_table(const Handle&, const MfmaParams&, bool, bool, hipStream_t, bool*, FxList<>) { return NEMPC_EUNSUPPORTED; }

template <typename T, typename SH, typename... Rest>
int fx_rows_table(const Handle& h, const MfmaParams& p, bool dense_here, bool sparse_here, hipStream_t s, bool* taken,
                  FxList<SH, Rest...>) {
    constexpr int WP = SH::WP, NH = SH::NH, NX = SH::NX, NU = SH::NU;
    if (!fx_shape_matches<T, SH>(h, p)) return fx_rows_table<T>(h, p, dense_here, sparse_here, s, taken, FxList<Rest...>{});
    static const int fx_tpw = env_int("NEMPC_FX_TPW", 3);
    constexpr int VEC = 16 / (int)sizeof(T);
    if (p.gn_hvals) {
        // Gauss-Newton callback in one launch (tril values): fp64, two states (the epilogue sums the states by a quad permute)
        *taken = true;
        if constexpr (sizeof(T) == 8 && NX == 2) {
            h.last_row_kernel = 4;
            return fx_tpw >= 3 ? launch_coopfx<T, WP, NH, 3, NX, NU, false, true>(p, s) : launch_coopfx<T, WP, NH, 2, NX, NU, false, true>(p, s);
        } else {
            return NEMPC_EUNSUPPORTED;
        }
    }
    if (p.fuse_obj) {
        // whole evaluation in one launch (objective, and the dense rows / band values if asked for, with the row work), or
        // tell the caller to take the multi-launch path
        *taken = true;
        if (p.fuse_jac && (p.gk.n % VEC != 0 || (reinterpret_cast<uintptr_t>(p.fuse_jac) & 15) != 0)) return NEMPC_EUNSUPPORTED;
        if (p.fuse_sparse && (reinterpret_cast<uintptr_t>(p.fuse_sparse) & 15) != 0) return NEMPC_EUNSUPPORTED;
        h.last_row_kernel = 4;
        return fx_tpw >= 3 ? launch_coopfx<T, WP, NH, 3, NX, NU, true>(p, s) : launch_coopfx<T, WP, NH, 2, NX, NU, true>(p, s);
    }
    if (p.tiles && !dense_here && !sparse_here) {
        *taken = true;
        h.last_row_kernel = 4;
        return fx_tpw >= 3 ? launch_coopfx<T, WP, NH, 3, NX, NU, false>(p, s) : launch_coopfx<T, WP, NH, 2, NX, NU, false>(p, s);
    }
    return NEMPC_EUNSUPPORTED;       // (not taken: the generic kernels serve this request)
}
}  // namespace

template <>
int launch_rows_mfma_act<NEMPC_T, NEMPC_ACT>(const Handle& h, MfmaParams p, hipStream_t s) {
    using T = NEMPC_T;
    const int wp = h.mfma.wp, nh = h.mfma.nh;
    // defect-only launches (tiles == null) take the wave-per-tile kernel
    const bool dense_here = p.fuse_jac && !p.fuse_obj;          // dense rows from the row launch itself
    const bool sparse_here = p.fuse_sparse && !p.fuse_obj;      // band values from the row launch itself
    const bool allow_coop = h.variant != NEMPC_KERNEL_MFMA_TILE && (p.tiles || dense_here || sparse_here) && p.mb == 1 && p.ks <= 4 &&
                            (unsigned long long)p.B * p.H * p.H < 0x100000000ull;   // row / H by multiply-high
    if (dense_here) {
        // plain models whose row blocks are whole 16-byte vectors; flat zero runs with 32-bit byte offsets
        const size_t blk = (size_t)p.nx * p.gk.n * sizeof(T);
        if (!allow_coop || p.gk.w != 1 || p.stage_out || blk % 16 != 0 || (reinterpret_cast<uintptr_t>(p.fuse_jac) & 15) != 0 ||
            4 * 16 * blk >= 0x7fffffffull)
            return NEMPC_EUNSUPPORTED;
    }
    if (sparse_here && (!allow_coop || p.gk.w != 1 || p.stage_out)) return NEMPC_EUNSUPPORTED;
    // compiled fixed shapes (kFxShapes above): plain Discret / Unity models whose (padded width, hidden layers, nx, nu) has
    // a rows_coopfx_kernel instantiation in this translation unit
    {
        bool taken = false;
        const int rc = fx_rows_table<T>(h, p, dense_here, sparse_here, s, &taken, FxTable<T>{});
        if (taken) return rc;
    }
    if (p.fuse_obj || p.gn_hvals) return NEMPC_EUNSUPPORTED;
#define NEMPC_CASE(WPV, NHV) \
    if (wp == WPV && nh == NHV) return launch_shape<T, WPV, NHV>(p, allow_coop, s, &h.last_row_kernel);
    NEMPC_CASE(32, 1) NEMPC_CASE(32, 2) NEMPC_CASE(32, 3)
    NEMPC_CASE(64, 1) NEMPC_CASE(64, 2) NEMPC_CASE(64, 3)
    NEMPC_CASE(128, 1) NEMPC_CASE(128, 2) NEMPC_CASE(128, 3)
    NEMPC_CASE(32, 4) NEMPC_CASE(64, 4)          // a fourth hidden layer up to width 64
#undef NEMPC_CASE
    set_error("launch_rows_mfma: no instantiation for this shape");
    return NEMPC_EUNSUPPORTED;
}

namespace {
template <typename T, int WP, int NH>
int launch_hess_shape(const HessParams& hp, hipStream_t s) {
    const MfmaParams& p = hp.base;
    const size_t esz = sizeof(T);
    const size_t blob_bytes = (size_t)((p.off.total + 1) & ~1) * esz;
    const size_t scratch = (size_t)p.scratch_per_wave * esz;
    int waves = (p.ntiles + p.num_cus - 1) / p.num_cus;
    waves = waves < 1 ? 1 : (waves > 4 ? 4 : waves);   // one wave per SIMD: the kernel needs > 256 registers
    constexpr size_t hh_bytes = (size_t)(NH - 1) * 2 * (WP / 16) * (WP / 16) * 256 * sizeof(T);
    if constexpr (hh_bytes <= 96 * 1024) {
        if (blob_bytes + (size_t)waves * scratch <= (size_t)kLdsBudget) {
            int grid = (p.ntiles + waves - 1) / waves;
            if (grid > p.num_cus) grid = p.num_cus;
            auto kern = rowhess_mfma_kernel<T, WP, NH, true, kAct>;
            const size_t bytes = blob_bytes + waves * scratch;
            NEMPC_HIP(ensure_dynamic_lds(reinterpret_cast<const void*>(kern), bytes));
            hipLaunchKernelGGL(kern, dim3(grid), dim3(waves * 64), bytes, s, hp);
            NEMPC_HIP(hipGetLastError());
            return NEMPC_OK;
        }
    }
    waves = 4;
    while (waves > 1 && (size_t)waves * scratch > (size_t)kLdsBudget) waves >>= 1;
    const int grid = (p.ntiles + waves - 1) / waves;
    auto kern = rowhess_mfma_kernel<T, WP, NH, false, kAct>;
    NEMPC_HIP(ensure_dynamic_lds(reinterpret_cast<const void*>(kern), (size_t)waves * scratch));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(waves * 64), (size_t)waves * scratch, s, hp);
    NEMPC_HIP(hipGetLastError());
    return NEMPC_OK;
}
}  // namespace

namespace {
constexpr int kHessTG = 3;   // tangent directions swept together by the cooperative Hessian kernel

template <typename T, int WP, int NH>
bool try_launch_hess_coop(const HessParams& hp, hipStream_t s, int* rc) {
    constexpr int MT = WP / 16;
    const MfmaParams& p = hp.base;
    const int NR = coop_nr<T>(p.nin);
    auto up16 = [](int v) { return (v + 15) & ~15; };
    HessCoopLayout lay{};
    int q = 0;
    lay.w0f = q; q += up16(p.ks * MT * 64);
    lay.tail = q; q += up16(p.off.total - p.off.p0tab);
    lay.x = q; lay.xhalf = kHessTG * MT * 256; q += 2 * lay.xhalf;
    lay.part = q; q += up16(kHessTG * MT * NR * 64);
    lay.scratch = q; q += up16(16 * (p.nin + p.nx + p.ne + p.nin * p.nin));
    lay.total = q;
    const size_t bytes = (size_t)lay.total * sizeof(T);
    const int wg_by_regs = 8 / MT;   // __launch_bounds__(MT*64, 2)
    int per_cu = (int)((size_t)kLdsBudgetCoop / bytes);
    if (per_cu < 1) return false;
    if (per_cu > wg_by_regs) per_cu = wg_by_regs;
    auto kern = rowhess_coop_kernel<T, WP, NH, kHessTG, kAct>;
    hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(kern), bytes);
    if (e != hipSuccess) { *rc = hip_fail(e, "hipFuncSetAttribute(hess coop)"); return true; }
    const GridPlan gp = plan_grid(p.ntiles, p.num_cus, per_cu);
    const int grid = gp.grid;
    HessParams hc = hp;
    hc.base.tiles_per_wg = gp.tiles_per_wg;
    hc.base.tiles_rem = gp.tiles_rem;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(MT * 64), bytes, s, hc, lay);
    e = hipGetLastError();
    *rc = e == hipSuccess ? NEMPC_OK : hip_fail(e, "rowhess_coop_kernel launch");
    return true;
}

// fixed-shape Hessian kernel (kernels_hessfx_impl.h): plain Discret / Unity models of a compiled shape
template <typename T, int WP, int NH, int NT, int NX, int NU, int TG = NX + NU, bool RWB = false, bool EV = false>
int launch_hessfx(const HessParams& hp, hipStream_t s) {
    using L = HfxLayout<T, WP, NH, NT, NX, NU, TG, EV>;
    constexpr int MT = WP / 16;
    const MfmaParams& p = hp.base;
    const size_t bytes = (size_t)L::TOTAL * sizeof(T);
    auto kern = rowhess_coopfx_kernel<T, WP, NH, NT, NX, NU, kAct, TG, RWB, EV>;
    NEMPC_HIP(ensure_dynamic_lds(reinterpret_cast<const void*>(kern), bytes));
    int per_cu = (int)((size_t)kLdsBudgetCoop / bytes);
    if (per_cu > 8 / MT) per_cu = 8 / MT;
    if (per_cu < 1) per_cu = 1;
    const GridPlan gp = plan_grid(p.ntiles, p.num_cus, per_cu);
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

template <typename T, int WP, int NH>
int launch_hess_any(const HessParams& hp, bool allow_coop, hipStream_t s, int* kernel_used) {
    if constexpr (coop_fits_registers<T, WP, NH>()) {
        int rc = NEMPC_OK;
        if (allow_coop && try_launch_hess_coop<T, WP, NH>(hp, s, &rc)) {
            *kernel_used = 2;
            return rc;
        }
    }
    if (hp.hvals) return NEMPC_EUNSUPPORTED;     // the fused assembly lives in the cooperative kernel only
    *kernel_used = 3;
    return launch_hess_shape<T, WP, NH>(hp, s);
}
}  // namespace

namespace {
template <typename T>
int fx_hess_table(const Handle&, const HessParams&, bool, hipStream_t, bool*, FxList<>) { return NEMPC_EUNSUPPORTED; }

template <typename T, typename SH, typename... Rest>
int fx_hess_table(const Handle& h, const HessParams& hp, bool allow_coop, hipStream_t s, bool* taken, FxList<SH, Rest...>) {
    const MfmaParams& p = hp.base;
    if (hfx_on() && allow_coop && h.mfma.wp == SH::WP && h.mfma.nh == SH::NH && p.nx == SH::NX && p.nu == SH::NU &&
        p.nin == SH::NX + SH::NU && p.ne == 0 && p.gk.w == 1 && p.kind != NEMPC_RK4 && !hp.xi_direct && (hp.blocks || hp.hvals) &&
        (unsigned long long)p.B * p.H * p.H < 0x100000000ull) {
        *taken = true;
        h.last_hess_kernel = 4;
        constexpr int TG = SH::NX + SH::NU;
        return hp.ev_g ? launch_hessfx<T, SH::WP, SH::NH, 1, SH::NX, SH::NU, TG, false, true>(hp, s)
                       : launch_hessfx<T, SH::WP, SH::NH, 1, SH::NX, SH::NU>(hp, s);
    }
    return fx_hess_table<T>(h, hp, allow_coop, s, taken, FxList<Rest...>{});
}
}  // namespace

namespace {
// the compiled configs[2] shape of the Hessian kernel exists for compile-time activations only (a template, so that the
// run-time-activation unit never instantiates it)
template <typename T, int ACTV>
int c3_hessfx(const HessParams& hp, hipStream_t s) {
    if constexpr (ACTV != NEMPC_ACT_RUNTIME && sizeof(T) == 4) return launch_hessfx<T, 128, 3, 1, 6, 3, 3, true>(hp, s);
    else return NEMPC_EUNSUPPORTED;
}
}  // namespace

template <>
int launch_rowhess_mfma_act<NEMPC_T, NEMPC_ACT>(const Handle& h, HessParams hp, hipStream_t s) {
    using T = NEMPC_T;
    const int wp = h.mfma.wp, nh = h.mfma.nh;
    // NEMPC_KERNEL_MFMA_TILE keeps the wave-per-tile Hessian kernel (A/B measurements), like it does for the rows
    const bool allow_coop = h.variant != NEMPC_KERNEL_MFMA_TILE && hp.base.mb == 1 && hp.base.ks <= 4;
    // compiled fixed shapes (the table above: plain Discret / Unity models)
    {
        bool taken = false;
        const int rc = fx_hess_table<T>(h, hp, allow_coop, s, &taken, FxTable<T>{});
        if (taken) return rc;
    }
    if (hp.ev_g) return NEMPC_EUNSUPPORTED;       // blocks + first-order evaluation in one launch: compiled shape only
    // BASELINE configs[2] dims (6 states, 3 controls, 3x128, fp32): the Discret / Unity blocks and the (row, stage) pairs
    // of the RK4 pipeline (direct mode), three tangent directions per exchange
    if constexpr (sizeof(T) == 4) {
        const MfmaParams& p = hp.base;
        if (kAct != NEMPC_ACT_RUNTIME && hfx_on() && allow_coop && wp == 128 && nh == 3 && p.nx == 6 && p.nu == 3 && p.nin == 9 && p.ne == 0 && p.gk.w == 1 &&
            (hp.xi_direct || p.kind != NEMPC_RK4) && (hp.blocks || hp.hvals) && !(hp.xi_direct && hp.hvals) &&
            (unsigned long long)p.B * p.H * p.H * (hp.xi_direct ? hp.vdiv : 1) < 0x100000000ull) {
            h.last_hess_kernel = 4;
            return c3_hessfx<T, kAct>(hp, s);
        }
    }
#define NEMPC_HCASE(WPV, NHV) \
    if (wp == WPV && nh == NHV) return launch_hess_any<T, WPV, NHV>(hp, allow_coop, s, &h.last_hess_kernel);
    NEMPC_HCASE(32, 1) NEMPC_HCASE(32, 2) NEMPC_HCASE(32, 3)
    NEMPC_HCASE(64, 1) NEMPC_HCASE(64, 2) NEMPC_HCASE(64, 3)
    NEMPC_HCASE(128, 1) NEMPC_HCASE(128, 2) NEMPC_HCASE(128, 3)
    NEMPC_HCASE(32, 4) NEMPC_HCASE(64, 4)
#undef NEMPC_HCASE
    set_error("launch_rowhess_mfma: no instantiation for this shape");
    return NEMPC_EUNSUPPORTED;
}

}  // namespace nempc
