// Host side of the matrix-core row kernel: shape gate, weight packing, launch geometry.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <type_traits>

#include "kernels_hess_impl.h"

namespace nempc {

namespace {

int padded_width(const Handle& h) {
    int w = 0;
    for (int l = 0; l < h.nl - 1; ++l) w = std::max(w, h.dout[l]);
    if (w <= 32) return 32;
    if (w <= 64) return 64;
    if (w <= 128) return 128;
    return 0;
}

// what the plans (mfma_plan.h) look at, of a handle and a call's batch size
MfmaShape mfma_shape(const Handle& h, int B) {
    MfmaShape s{};
    s.esz = (int)h.esz; s.wp = h.mfma.wp; s.nh = h.mfma.nh;
    s.nx = h.cfg.nx; s.nu = h.cfg.nu; s.nin = h.nin; s.ne = h.ne; s.window = h.w;
    s.integrator = h.cfg.integrator; s.variant = h.variant; s.act = h.mfma_act;
    s.n = h.n; s.m = h.m; s.B = B; s.H = h.cfg.H; s.num_cus = h.num_cus;
    s.obj_elems = h.d_obj ? obj_offsets(h.cfg.H, h.cfg.nx, h.cfg.nu).total : 0;
    s.hess_scatter = h.d_hess_smap && h.hess_n_orph >= 0;
    s.layered_hess = h.layered_hess;
    return s;
}

}  // namespace

bool mfma_supported(const Handle& h) {
    const int nh = h.nl - 1;
    if (nh < 1 || nh > NEMPC_MFMA_MAX_HIDDEN || h.mfma_act < 0) return false;
    if (nh == 4 && padded_width(h) > 64) return false;             // a fourth hidden layer: up to width 64
    // network outputs on one 16-row block; inputs (window + extras) on up to kMaxKs k-steps, the window itself on up
    // to two 16-row blocks of the last reverse step (wave-per-tile kernels; the cooperative ones take <= 16)
    if (h.cfg.nx > 16 || h.nin + h.ne > 4 * kMaxKs || h.nin > 32) return false;
    // one wave's scratch is the least LDS any row kernel asks for (the streamed wave-per-tile kernel with one wave per
    // workgroup); with the RK4 chain's four Jacobian slots an fp64 16-state / 20-input stage needs 168.5 KiB, more than the
    // CU's 160 KiB, and every launch of it was refused (hipFuncSetAttribute: invalid argument) -- such shapes are not ours
    MfmaShape s{};
    s.esz = h.cfg.dtype == NEMPC_F64 ? 8 : 4; s.nx = h.cfg.nx; s.nin = h.nin; s.ne = h.ne; s.integrator = h.cfg.integrator;
    if ((size_t)s.rows_scratch() * s.esz > (size_t)160 * 1024) return false;
    return padded_width(h) != 0;
}

// Shapes the register-resident kernels take but the layered path runs faster (AUTO then picks the layered path; asking for
// NEMPC_KERNEL_MFMA by name still gets them): fp64 networks with run-time activation codes whose weight slices do not fit
// the cooperative kernel's registers (3 x 128, a fourth layer at width 64) -- the wave-per-tile kernel with the activation
// switch inlined spills (800 B of scratch per lane) and measured 304 us against the layered path's 187 (3 x 128 relu / tanh /
// sigmoid, B = 1024, H = 20; tools/narrow_bench.py).
bool mfma_slower_than_layered(const Handle& h) {
    if (h.mfma_act != NEMPC_ACT_RUNTIME || h.cfg.dtype != NEMPC_F64 || !layered_supported(h)) return false;
    const int nh = h.nl - 1, MT = padded_width(h) / 16;
    return !coop_fits_registers(8, 16 * MT, nh);
}

// Shapes whose ROWS are fastest on the register-resident kernels but whose Lagrangian blocks are not (fp64, padded width 128,
// Discret / Unity; the RK4 pipeline keeps its own network kernel; tools/narrow_bench.py, B = 1024, H = 20, 2/1, us per callback):
//   three hidden layers, one activation: the weight slices do not fit the cooperative Hessian kernel, the wave-per-tile one
//     streams 1.5 MB of weights per tile: 565 against 250 for the layered sweeps (the rows: 154 against 150 - 190)
//   two hidden layers, run-time activation codes: the cooperative Hessian kernel with the activation switches inlined, 182
//     against 161 (the rows: 101 against 105)
bool mfma_hess_on_layered(const Handle& h) {
    // (AUTO only: asking for NEMPC_KERNEL_MFMA by name keeps the register-resident Hessian kernels -- that is the A/B)
    if (h.cfg.dtype != NEMPC_F64 || h.cfg.integrator == NEMPC_RK4 || !layered_supported(h)) return false;
    return padded_width(h) == 128 && (h.nl - 1 == 3 || (h.nl - 1 == 2 && h.mfma_act == NEMPC_ACT_RUNTIME));
}

// Pack every layer into MFMA A-operand fragments (lane-linear: element [frag*64 + lane]).
// lane = kq*16 + i16 supplies A[M index i16][K index kq]; the K index of k-step (mt, r) stands for
// feature 16*mt + row(kq, r) where row() is the accumulator register->row map of the dtype
// (f64: kq + 4r, f32: 4kq + r), so that accumulator register r of tile mt is the matching B operand.
int mfma_pack_weights(Handle& h, const double* const* W, const double* const* b) {
    const int wp = padded_width(h), nh = h.nl - 1, MT = wp / 16;
    const int nx = h.cfg.nx, nin = h.nin, ks = (nin + h.ne + 3) / 4, L = h.nl - 1;
    const bool f64 = h.cfg.dtype == NEMPC_F64;
    auto row = [&](int q, int r) { return f64 ? MfmaOps<double>::row(q, r) : MfmaOps<float>::row(q, r); };
    const MfmaOffsets o = make_offsets(wp, nh, ks, nx, nin, (int)h.esz);
    const int MB = (nin + 15) / 16;
    std::vector<double> blob((size_t)o.grand_total, 0.0);
    auto Wat = [&](int l, int i, int j) -> double {
        return (i < h.din[l] && j < h.dout[l]) ? W[l][(size_t)i * h.dout[l] + j] : 0.0;
    };
    for (int lane = 0; lane < 64; ++lane) {
        const int i16 = lane & 15, kq = lane >> 4;
        for (int k = 0; k < ks; ++k)
            for (int mo = 0; mo < MT; ++mo) blob[o.w0f + (k * MT + mo) * 64 + lane] = Wat(0, 4 * k + kq, 16 * mo + i16);
        for (int mt = 0; mt < MT; ++mt)
            for (int r = 0; r < 4; ++r) {
                const int kf = 16 * mt + row(kq, r);
                for (int l = 1; l < nh; ++l)
                    for (int mo = 0; mo < MT; ++mo) {
                        blob[o.wf[l] + ((mt * 4 + r) * MT + mo) * 64 + lane] = Wat(l, kf, 16 * mo + i16);
                        blob[o.wb[l] + ((mt * 4 + r) * MT + mo) * 64 + lane] = Wat(l, 16 * mo + i16, kf);
                    }
                blob[o.wLf + (mt * 4 + r) * 64 + lane] = (i16 < nx) ? Wat(L, kf, i16) : 0.0;
                for (int mb = 0; mb < MB; ++mb)
                    blob[o.w0b + ((mt * 4 + r) * MB + mb) * 64 + lane] = (16 * mb + i16 < nin) ? Wat(0, 16 * mb + i16, kf) : 0.0;
            }
    }
    for (int lane = 0; lane < 64; ++lane) {   // W_L as an A operand with M = hidden unit, K = network output
        const int i16 = lane & 15, kq = lane >> 4;
        for (int k = 0; k < (nx + 3) / 4; ++k)
            for (int mt = 0; mt < MT; ++mt)
                blob[o.wLb + (k * MT + mt) * 64 + lane] = (4 * k + kq < nx) ? Wat(L, 16 * mt + i16, 4 * k + kq) : 0.0;
    }
    for (int q = 0; q < 4; ++q)
        for (int r = 0; r < 4; ++r) {
            for (int mt = 0; mt < MT; ++mt) {
                const int f = 16 * mt + row(q, r);
                for (int pp = 0; pp < nin; ++pp) blob[o.p0tab + pp * MT * 16 + (mt * 4 + r) * 4 + q] = Wat(0, pp, f);
                for (int k = 0; k < nx; ++k) blob[o.seed + k * MT * 16 + (mt * 4 + r) * 4 + q] = Wat(L, f, k);
                for (int l = 0; l < nh; ++l) blob[o.bias[l] + (mt * 4 + r) * 4 + q] = (f < h.dout[l]) ? b[l][f] : 0.0;
            }
            const int oo = row(q, r);
            blob[o.biasL + r * 4 + q] = (oo < nx) ? b[L][oo] : 0.0;
        }

    // cooperative-kernel copies (only meaningful when the last reverse step has one 16-row block, MB == 1)
    {
        const int vec = 16 / (int)h.esz;
        for (int i = 0; i < ks * MT * 64; ++i) blob[o.coop_small + i] = blob[o.w0f + i];
        for (int i = 0; i < o.total - o.seed; ++i) blob[o.coop_small + ks * MT * 64 + i] = blob[o.seed + i];
        for (int w = 0; w < MT; ++w)
            for (int lane = 0; lane < 64; ++lane) {
                int fidx = 0;
                auto put = [&](double v) {
                    blob[o.coop_slices + ((size_t)(w * o.coop_nload + fidx / vec) * 64 + lane) * vec + fidx % vec] = v;
                    ++fidx;
                };
                for (int l = 1; l < nh; ++l) {
                    for (int i = 0; i < MT * 4; ++i) put(blob[o.wf[l] + (i * MT + w) * 64 + lane]);
                    for (int i = 0; i < MT * 4; ++i) put(blob[o.wb[l] + (i * MT + w) * 64 + lane]);
                }
                for (int r = 0; r < 4; ++r) put(blob[o.wLf + (w * 4 + r) * 64 + lane]);
                for (int r = 0; r < 4; ++r) put(blob[o.w0b + ((w * 4 + r) * MB) * 64 + lane]);
            }
    }

    for (int i = 0; i < o.coop_small_elems; ++i) blob[o.fx_small + i] = blob[o.coop_small + i];
    for (int i = 0; i < nin * MT * 16; ++i) blob[o.fx_small + o.coop_small_elems + i] = blob[o.p0tab + i];

    // (into a buffer of its own: a failure leaves the handle's packed network as it was)
    DevBuf<> dev;
    if (int rc = dev.alloc(blob.size() * h.esz, "mfma blob")) return rc;
    if (f64) {
        NEMPC_HIP(hipMemcpy(dev.get(), blob.data(), blob.size() * 8, hipMemcpyHostToDevice));
    } else {
        std::vector<float> tmp(blob.begin(), blob.end());
        NEMPC_HIP(hipMemcpy(dev.get(), tmp.data(), tmp.size() * 4, hipMemcpyHostToDevice));
    }
    h.mfma.blob = std::move(dev);
    h.mfma.wp = wp;
    h.mfma.nh = nh;
    h.mfma.kin = 4 * ks;
    return NEMPC_OK;
}

// one translation unit per (dtype, hidden activation) defines these (kernels_mfma_typed.inc)
#define NEMPC_DECL_ACT(T, A)                                                                                  \
    template <> int launch_rows_mfma_act<T, A>(const MfmaParams& p, const MfmaRowsPlan& plan, hipStream_t s);    \
    template <> int launch_rowhess_mfma_act<T, A>(const HessParams& hp, const MfmaHessPlan& plan, hipStream_t s);
#define NEMPC_DECL_ACTS(T)                                                                         \
    NEMPC_DECL_ACT(T, NEMPC_ACT_TANH) NEMPC_DECL_ACT(T, NEMPC_ACT_RELU) NEMPC_DECL_ACT(T, NEMPC_ACT_SIGMOID) \
    NEMPC_DECL_ACT(T, NEMPC_ACT_SOFTPLUS) NEMPC_DECL_ACT(T, NEMPC_ACT_ELU) NEMPC_DECL_ACT(T, NEMPC_ACT_RUNTIME)
NEMPC_DECL_ACTS(double)
NEMPC_DECL_ACTS(float)
#undef NEMPC_DECL_ACTS
#undef NEMPC_DECL_ACT

namespace {

// the typed unit of the handle's dtype and activation (NEMPC_ACT_RUNTIME: per-layer codes in MfmaParams::acts)
template <typename T, typename P, typename Plan>
int launch_typed(const Handle& h, const P& p, const Plan& plan, hipStream_t s) {
    auto go = [&](auto act) {
        if constexpr (std::is_same_v<P, MfmaParams>) return launch_rows_mfma_act<T, decltype(act)::value>(p, plan, s);
        else return launch_rowhess_mfma_act<T, decltype(act)::value>(p, plan, s);
    };
    switch (h.mfma_act) {
        case NEMPC_ACT_TANH: return go(std::integral_constant<int, NEMPC_ACT_TANH>{});
        case NEMPC_ACT_RELU: return go(std::integral_constant<int, NEMPC_ACT_RELU>{});
        case NEMPC_ACT_SIGMOID: return go(std::integral_constant<int, NEMPC_ACT_SIGMOID>{});
        case NEMPC_ACT_SOFTPLUS: return go(std::integral_constant<int, NEMPC_ACT_SOFTPLUS>{});
        case NEMPC_ACT_ELU: return go(std::integral_constant<int, NEMPC_ACT_ELU>{});
        case NEMPC_ACT_RUNTIME: return go(std::integral_constant<int, NEMPC_ACT_RUNTIME>{});
    }
    set_error("matrix-core launch: the kernels do not take this network's activations");
    return NEMPC_EINVAL;
}

// the parameters every matrix-core kernel reads: network, dims, inputs, gather
MfmaParams base_params(const Handle& h, int B, const void* Z, const void* X0, int ntiles, int scratch_per_wave) {
    MfmaParams p{};
    p.blob = h.mfma.blob.get();
    p.nx = h.cfg.nx; p.nu = h.cfg.nu; p.nin = h.nin; p.ks = (h.nin + h.ne + 3) / 4; p.mb = (h.nin + 15) / 16;
    p.ne = h.ne; p.extra = h.d_extra;
    p.off = make_offsets(h.mfma.wp, h.mfma.nh, p.ks, p.nx, p.nin, (int)h.esz);
    for (int l = 0; l < NEMPC_MFMA_MAX_HIDDEN; ++l) {
        p.acts.code[l] = l < h.nl - 1 ? h.act[l] : NEMPC_ACT_LINEAR;
        p.acts.par[l] = l < h.nl - 1 ? h.actp[l] : 0.0;
    }
    p.kind = h.cfg.integrator; p.DT = h.cfg.DT;
    p.B = B; p.H = h.cfg.H; p.m = h.m; p.box = h.box ? 1 : 0; p.num_cus = h.num_cus;
    p.Z = Z; p.X0 = X0;
    p.gk = h.gather();
    p.ntiles = ntiles;
    p.scratch_per_wave = scratch_per_wave;
    return p;
}

unsigned lo4(const void* p) { return (unsigned)(reinterpret_cast<uintptr_t>(p) & 15); }

}  // namespace

const MfmaKnobs& mfma_knobs() {
    static const MfmaKnobs k = [] {
        MfmaKnobs k;
        k.fx = env_int("NEMPC_FX", 1); k.hfx = env_int("NEMPC_HFX", 1); k.hfx_eval = env_int("NEMPC_HFX_EVAL", 1);
        k.gn_fused = env_int("NEMPC_GN_FUSED", 1); k.coop_dense = env_int("NEMPC_COOP_DENSE", 1);
        k.coop_sparse = env_int("NEMPC_COOP_SPARSE", 1); k.coop_dims = env_int("NEMPC_COOP_DIMS", 1);
        k.coop_tpw = env_int("NEMPC_COOP_TPW", MfmaKnobs::kUnset); k.fx_tpw = env_int("NEMPC_FX_TPW", 3);
        k.tile_waves = env_int("NEMPC_TILE_WAVES", 4);
        return k;
    }();
    return k;
}

MfmaRowsPlan mfma_plan_rows(const Handle& h, int B, const RowsOut& o) {
    RowsWant w;
    w.bits = (o.tiles || o.need_tiles ? WANT_TILES : 0u) | (o.jac ? WANT_DENSE : 0u) | (o.sparse ? WANT_SPARSE : 0u) |
             (o.f ? WANT_F : 0u) | (o.grad ? WANT_GRAD : 0u) | (o.stage_out ? WANT_STAGES : 0u) | (o.gn_hvals ? WANT_GN : 0u);
    w.dense_lo4 = lo4(o.jac); w.sparse_lo4 = lo4(o.sparse);
    return plan_rows(mfma_shape(h, B), w, mfma_knobs());
}

MfmaHessPlan mfma_plan_hess(const Handle& h, int B, const HessOut& o) {
    HessWant w;
    w.bits = (o.hvals ? HWANT_HVALS : HWANT_BLOCKS) | (o.ev_g ? HWANT_EVAL : 0u) | (o.xi_direct ? HWANT_DIRECT : 0u);
    w.vdiv = o.vdiv;
    return plan_hess(mfma_shape(h, B), w, mfma_knobs());
}

// Rows (defects, compact tiles) and whatever else of the evaluation the planned launch writes itself: the whole
// hessian-free evaluation or the Gauss-Newton callback on a compiled shape, the dense rows or the band values (and the
// objective with them) from the cooperative kernel.
int launch_rows_mfma(Handle& h, int B, const void* Z, const void* X0, const RowsOut& o, hipStream_t s, unsigned* covers) {
    if (!h.mfma.blob) {
        set_error("launch_rows_mfma: weights not packed");
        return NEMPC_ESTATE;
    }
    const MfmaRowsPlan plan = mfma_plan_rows(h, B, o);
    if (covers) *covers = plan.covers;
    MfmaParams p = base_params(h, B, Z, X0, (int)(((size_t)B * h.cfg.H + 15) / 16), mfma_shape(h, B).rows_scratch());
    p.g = o.g;
    // (a launch that writes the dense rows / band values itself has no assembly launch behind it: the caller's tiles only)
    p.tiles = o.tiles ? o.tiles : (o.need_tiles && !(plan.covers & (COVERS_DENSE | COVERS_SPARSE)) ? h.d_tiles_ws.get() : nullptr);
    p.stage_out = o.stage_out; p.stage_stride = o.stage_stride;
    p.dbg = h.d_dbg.get();
    p.fuse_obj = plan.fuse;
    if (plan.covers & COVERS_DENSE) { p.fuse_jac = o.jac; p.jac_resident = plan.fuse && o.jac_resident; }
    if (plan.covers & COVERS_SPARSE) { p.fuse_sparse = o.sparse; p.sp_nnz = (int)h.jac_rows.size(); }
    if (plan.fuse || (plan.covers & COVERS_OBJ)) {      // (the fused evaluation reads the table's size whatever it writes)
        p.fuse_f = o.f; p.fuse_grad = o.grad; p.obj = h.d_obj.get();
        p.oo = obj_offsets(h.cfg.H, h.cfg.nx, h.cfg.nu);
    }
    if (plan.covers & COVERS_GN) {
        p.g = h.d_g_ws.get(); p.tiles = nullptr;
        p.gn_hvals = o.gn_hvals; p.gn_sigma = o.gn_sigma; p.gn_w = o.gn_w; p.gn_smap = h.d_hess_smap.get();
        p.gn_objc = h.d_obj.as<const char>() + (size_t)obj_offsets(h.cfg.H, h.cfg.nx, h.cfg.nu).total * h.esz;
        p.gn_nnz = (int)h.hess_rows.size(); p.gn_n_orph = h.hess_n_orph;
    }
    const int rc = h.cfg.dtype == NEMPC_F64 ? launch_typed<double>(h, p, plan, s) : launch_typed<float>(h, p, plan, s);
    if (rc == NEMPC_OK) h.last_row_kernel = plan.kernel;
    return rc;
}

// Lagrangian blocks; on a plan that covers them, the tril values from the kernel itself (out.hvals) or the first-order
// evaluation of the same rows (out.ev_g / ev_tiles: the batched solver's trial point).  NEMPC_EUNSUPPORTED: out.ev_g on a
// shape without such a launch.  A handle whose blocks are faster on the layer-at-a-time sweeps (mfma_hess_on_layered) gets
// them there.
int launch_rowhess_mfma(Handle& h, int B, const void* Z, const void* X0, const void* lambda, const HessOut& o, hipStream_t s,
                        unsigned* covers) {
    if (covers) *covers = 0;
    if (h.layered_hess && !o.ev_g && !o.xi_direct) {
        const int rc = launch_rowhess_layered(h, B, Z, X0, lambda, o.blocks, s);
        if (rc != NEMPC_EUNSUPPORTED) return rc;        // (the layered path's own switch, NEMPC_LAYERED_HESS=0)
    }
    if (!h.mfma.blob) {
        set_error("launch_rowhess_mfma: weights not packed");
        return NEMPC_ESTATE;
    }
    const MfmaHessPlan plan = mfma_plan_hess(h, B, o);
    if (plan.kernel == HESS_NONE) return NEMPC_EUNSUPPORTED;
    if (covers) *covers = plan.covers;
    HessParams hp{};
    hp.base = base_params(h, B, Z, X0, (int)(((size_t)B * h.cfg.H * (o.xi_direct ? o.vdiv : 1) + 15) / 16),
                          mfma_shape(h, B).hess_scratch());
    const MfmaParams& p = hp.base;
    hp.xi_direct = o.xi_direct; hp.xi_stride = o.xi_stride; hp.lam_direct = o.lam_direct; hp.vdiv = o.vdiv;
    hp.lambda = lambda; hp.blocks = (plan.covers & COVERS_HVALS) ? nullptr : o.blocks;
    hp.ev_g = o.ev_g; hp.ev_tiles = o.ev_tiles;
    if (plan.covers & COVERS_HVALS) {       // the kernel assembles the tril values itself
        hp.hvals = o.hvals; hp.sigma = o.sigma; hp.smap = h.d_hess_smap.get();
        hp.objc = h.d_obj.as<const char>() + (size_t)obj_offsets(h.cfg.H, h.cfg.nx, h.cfg.nu).total * h.esz;
        hp.nnz = (int)h.hess_rows.size(); hp.n_orph = h.hess_n_orph;
    }
    hp.p0tab = p.off.p0tab; hp.wLb = p.off.wLb; hp.ksx = (h.cfg.nx + 3) / 4;
    const int rc = h.cfg.dtype == NEMPC_F64 ? launch_typed<double>(h, hp, plan, s) : launch_typed<float>(h, hp, plan, s);
    if (rc == NEMPC_OK) h.last_hess_kernel = plan.kernel;
    return rc;
}

}  // namespace nempc
