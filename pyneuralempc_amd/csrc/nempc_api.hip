// C ABI of libnempc.so: handle lifetime, parameter upload, structure export, launch sequencing.
// See include/nempc.h for the contract and the reference call sites each entry point stands for.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <utility>

#include "nempc_internal.h"
#include "activations.h"
#include "rows_index.h"     // rows_limit_entry: where a limit of nempc_bind_stage_rows is read from
#include "stage_aug.h"      // window_var: the window's column order

namespace nempc {

static thread_local std::string g_last_error;

void set_error(const std::string& msg) { g_last_error = msg; }

hipError_t ensure_dynamic_lds(const void* kernel, size_t bytes) {
    if (bytes <= 65536) return hipSuccess;
    static std::mutex mu;
    static std::map<std::pair<int, const void*>, size_t> done;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    size_t& have = done[{dev, kernel}];
    if (bytes <= have) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) have = bytes;
    return e;
}

int hip_fail(hipError_t e, const char* what) {
    set_error(std::string(what) + ": " + hipGetErrorString(e));
    return NEMPC_EHIP;
}

// dev_buf.h's raw functions: the library's only hipMalloc / hipFree outside solver.hip and comm.hip
int dev_raw_sync() {
    NEMPC_HIP(hipDeviceSynchronize());
    return NEMPC_OK;
}

int dev_raw_alloc(void** p, size_t bytes, const char* what) {
    *p = nullptr;
    const hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) return NEMPC_OK;
    *p = nullptr;
    set_error(std::string("hipMalloc (") + what + "): " + hipGetErrorString(e));
    return NEMPC_ENOMEM;
}

void dev_raw_free(void* p) { (void)hipFree(p); }

Handle::~Handle() {
    solver_free(*this);
    comm_free(*this);
}

namespace {

int fail(int code, const std::string& msg) {
    set_error(msg);
    return code;
}

int fail(int code, const char* who, const char* what) { return fail(code, std::string(who) + what); }

struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    DeviceGuard() = default;        // (nothing until set())
    explicit DeviceGuard(int dev) { set(dev); }
    void set(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) { ok = false; return; }
        if (prev != dev && hipSetDevice(dev) != hipSuccess) ok = false;
        if (prev == dev) prev = -1;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

template <typename T>
int upload_as(const std::vector<double>& src, void* dst) {
    std::vector<T> tmp(src.size());
    for (size_t i = 0; i < src.size(); ++i) tmp[i] = (T)src[i];
    NEMPC_HIP(hipMemcpy(dst, tmp.data(), tmp.size() * sizeof(T), hipMemcpyHostToDevice));
    return NEMPC_OK;
}

int upload(const Handle& h, const std::vector<double>& src, void* dst) {
    if (src.empty()) return NEMPC_OK;
    return h.cfg.dtype == NEMPC_F64 ? upload_as<double>(src, dst) : upload_as<float>(src, dst);
}

// a fresh device copy of a host array of int32 codes
int upload_map(DevBuf<int32_t>& dst, const std::vector<int32_t>& src, const char* what) {
    if (int rc = dst.alloc(src.size() * sizeof(int32_t), what)) return rc;
    NEMPC_HIP(hipMemcpy(dst.get(), src.data(), src.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    return NEMPC_OK;
}

// the row count, the Jacobian's structure and its assembly maps
int rebuild_structure(Handle& h) {
    const int H = h.cfg.H, nx = h.cfg.nx, nu = h.cfg.nu, nin = h.nin, n = h.n;
    h.m = H * nx + (h.box ? H * nx : 0);
    const int m = h.m;
    // the dense map changes: a resident dense Jacobian of the old shape holds non-zeros where the new one has none
    h.jac_resident.drop_all();
    std::vector<int32_t> dense((size_t)m * n, MAP_ZERO), sparse, pos;
    h.jac_rows.clear();
    h.jac_cols.clear();
    auto put = [&](int r, int c, int32_t code) {
        dense[(size_t)r * n + c] = code;
        h.jac_rows.push_back(r);
        h.jac_cols.push_back(c);
        sparse.push_back(code);
        pos.push_back(r * n + c);
    };
    std::vector<std::pair<int, int32_t>> ent;
    for (int t = 0; t < H; ++t)
        for (int i = 0; i < nx; ++i) {
            const int r = t * nx + i;
            const int base = t * nx * nin + i * nin;
            ent.clear();
            for (int d = 0; d < nin; ++d) {
                const int v = window_var(H, nx, nu, h.w, h.rev, t, d);
                if (v >= 0) ent.emplace_back(v, base + d);
            }
            ent.emplace_back(t * nx + i, MAP_MINUS_ONE);   // -x_t; the window only reaches state blocks < t
            std::sort(ent.begin(), ent.end());
            for (const auto& e : ent) put(r, e.first, e.second);
        }
    if (h.box)
        for (int k = 0; k < H * nx; ++k) put(H * nx + k, k, MAP_PLUS_ONE);

    h.d_sparse_map.reset(); h.d_sparse_pos.reset();     // (no map of the old shape behind a failure)
    int rc;
    if ((rc = upload_map(h.d_dense_map, dense, "dense map"))) return rc;
    if ((rc = upload_map(h.d_sparse_map, sparse, "sparse map"))) return rc;
    return upload_map(h.d_sparse_pos, pos, "sparse positions");
}

// Objective upload, in two parts.  The Hessian maps (tril structure, gather / scatter maps) depend on the problem's
// SHAPE only and are built once per handle; the parameter block [Q | Qs | R | Rs | xref | uref | cx | cu | QT | QTs |
// objective constants of every tril entry and of the dense (n,n) matrix] depends on the VALUES and is what a tracking
// MPC changes every step (a moving xref / uref): that path overwrites d_obj in place -- no map rebuild, no hipFree
// (a device synchronisation), no re-allocation.
int upload_objective(Handle& h, const ObjHost& o_in) {
    h.obj_host = o_in;
    const ObjHost& o = h.obj_host;
    const int H = h.cfg.H, nx = h.cfg.nx, nu = h.cfg.nu, n = h.n;
    ObjOffsets off = obj_offsets(H, nx, nu);
    std::vector<double> Qs(nx * nx), Rs(nu * nu), QT(h.obj_QT.empty() ? o.Q : h.obj_QT), QTs(nx * nx);
    for (int i = 0; i < nx; ++i)
        for (int j = 0; j < nx; ++j) {
            Qs[i * nx + j] = o.Q[i * nx + j] + o.Q[j * nx + i];
            QTs[i * nx + j] = QT[i * nx + j] + QT[j * nx + i];
        }
    for (int i = 0; i < nu; ++i)
        for (int j = 0; j < nu; ++j) Rs[i * nu + j] = o.R[i * nu + j] + o.R[j * nu + i];

    auto obj_const = [&](int r, int c, bool* structural) -> double {
        *structural = false;
        const bool rx = r < H * nx, cx = c < H * nx;
        if (rx && cx && r / nx == c / nx) {
            *structural = true;
            return (r / nx == H - 1 ? QTs : Qs)[(r % nx) * nx + (c % nx)];
        }
        if (!rx && !cx && (r - H * nx) / nu == (c - H * nx) / nu) {
            *structural = true;
            return Rs[((r - H * nx) % nu) * nu + ((c - H * nx) % nu)];
        }
        return 0.0;
    };

    int rc;
    if (!h.hess_maps_built) {
        // Hessian structure (tril, row-major) + maps.  Entry (r,c) sums the block elements of every step whose window
        // holds both variables (<= w of them; exactly one for plain models, integrator/discret.py:61-81) on top of the
        // constant objective term.
        const int nin = h.nin, w = h.w;
        std::vector<std::vector<int32_t>> codes((size_t)n * n);
        std::vector<int> wv(nin);
        for (int t = 0; t < H; ++t) {
            for (int d = 0; d < nin; ++d) wv[d] = window_var(H, nx, nu, h.w, h.rev, t, d);
            for (int pp = 0; pp < nin; ++pp)
                for (int qq = 0; qq < nin; ++qq)
                    if (wv[pp] >= 0 && wv[qq] >= 0) codes[(size_t)wv[pp] * n + wv[qq]].push_back(t * nin * nin + pp * nin + qq);
        }
        h.hess_rows.clear();
        h.hess_cols.clear();
        std::vector<int32_t> hmap;
        auto emit = [&](int r, int c) {
            const auto& cs = codes[(size_t)r * n + c];
            for (int k = 0; k < w; ++k) hmap.push_back(k < (int)cs.size() ? cs[k] : -1);
        };
        for (int r = 0; r < n; ++r)
            for (int c = 0; c <= r; ++c) {
                bool st;
                (void)obj_const(r, c, &st);
                if (st || !codes[(size_t)r * n + c].empty()) {
                    emit(r, c);
                    h.hess_rows.push_back(r);
                    h.hess_cols.push_back(c);
                }
            }
        for (int r = 0; r < n; ++r)
            for (int c = 0; c < n; ++c) emit(r, c);

        if ((rc = upload_map(h.d_hess_map, hmap, "Hessian map"))) return rc;
        // scatter form of the tril map for the Hessian kernel's fused assembly (plain models: one block element per entry)
        h.d_hess_smap.reset();
        h.hess_n_orph = -1;
        if (w == 1) {
            const int nnz_t = (int)h.hess_rows.size(), be = H * nin * nin;
            std::vector<int32_t> smap((size_t)be, -1), orph;
            for (int e = 0; e < nnz_t; ++e) {
                if (hmap[e] >= 0) smap[hmap[e]] = e;
                else orph.push_back(e);
            }
            if ((int)orph.size() <= nin * nin) {
                smap.insert(smap.end(), orph.begin(), orph.end());
                if ((rc = upload_map(h.d_hess_smap, smap, "Hessian scatter map"))) return rc;
                h.hess_n_orph = (int)orph.size();
            }
        }
        h.hess_maps_built = true;
    }

    // parameter block: the family's parameters, then the objective constant of every tril entry and of the dense matrix
    const size_t nnz_t = h.hess_rows.size();
    std::vector<double> all((size_t)off.total + nnz_t + (size_t)n * n);
    std::copy(o.Q.begin(), o.Q.end(), all.begin() + off.Q);
    std::copy(Qs.begin(), Qs.end(), all.begin() + off.Qs);
    std::copy(QT.begin(), QT.end(), all.begin() + off.QT);
    std::copy(QTs.begin(), QTs.end(), all.begin() + off.QTs);
    std::copy(o.R.begin(), o.R.end(), all.begin() + off.R);
    std::copy(Rs.begin(), Rs.end(), all.begin() + off.Rs);
    std::copy(o.xref.begin(), o.xref.end(), all.begin() + off.xref);
    std::copy(o.uref.begin(), o.uref.end(), all.begin() + off.uref);
    std::copy(o.cx.begin(), o.cx.end(), all.begin() + off.cx);
    std::copy(o.cu.begin(), o.cu.end(), all.begin() + off.cu);
    {
        bool st;
        double* oc = all.data() + off.total;
        for (size_t e = 0; e < nnz_t; ++e) oc[e] = obj_const(h.hess_rows[e], h.hess_cols[e], &st);
        oc += nnz_t;
        for (int r = 0; r < n; ++r)
            for (int c = 0; c < n; ++c) oc[(size_t)r * n + c] = obj_const(r, c, &st);
    }
    if (!h.d_obj || h.d_obj.bytes() != all.size() * h.esz)
        if ((rc = h.d_obj.alloc(all.size() * h.esz, "objective table"))) return rc;
    if ((rc = upload(h, all, h.d_obj.get()))) return rc;
    h.have_objective = true;
    return NEMPC_OK;
}

// The variable bounds nempc_kkt_residual and nempc_sensitivity see -- the caller's lb / ub (n host doubles each, null =
// unbounded) intersected with the box rows, as doubles on the device (+-inf kept) -- uploaded when they differ from the
// previous call's (a stream synchronisation then).  dlb / dub stay null when there is no bound at all.
int cached_bounds(Handle& h, const double* lb, const double* ub, const char* who, hipStream_t s, const double*& dlb,
                  const double*& dub) {
    dlb = dub = nullptr;
    if (!lb && !ub && !h.box) return NEMPC_OK;
    std::vector<double> both, hi;
    if (int rc = intersect_bounds(h, lb, ub, false, who, both, hi)) return rc;
    both.insert(both.end(), hi.begin(), hi.end());
    DeviceGuard dgb(h.cfg.device);
    if (!dgb.ok) return fail(NEMPC_EHIP, std::string(who) + ": hipSetDevice failed");
    // (bit-wise comparison: -inf / inf compare equal to themselves either way, and a NaN is uploaded every time)
    if (h.kkt_bounds_host.size() != both.size() ||
        std::memcmp(h.kkt_bounds_host.data(), both.data(), both.size() * sizeof(double)) != 0) {
        NEMPC_HIP(hipMemcpyAsync(h.d_kkt_bounds.get(), both.data(), both.size() * sizeof(double), hipMemcpyHostToDevice, s));
        NEMPC_HIP(hipStreamSynchronize(s));   // `both` is stack-owned
        h.kkt_bounds_host = both;
    }
    dlb = h.d_kkt_bounds.get(); dub = dlb + h.n;
    return NEMPC_OK;
}

// d_g_ws, (Bmax, m): sized with the batch workspaces below and again when the row count changes (nempc_set_box_rows)
size_t g_ws_bytes(const Handle& h) { return (size_t)h.cfg.max_batch * h.m * h.esz; }

// The buffers sized by cfg.max_batch that nempc_reserve replaces, named once, with their bytes at the current max_batch.
// what == nullptr: not sized here -- its first user does that (d_valu_ws: ensure_valu_ws; the RK4 Hessian pipeline's three;
// d_sens_ws of a rolling-window handle is never needed: nempc_sensitivity refuses those).  Not on the list: the layered path's
// chunk workspaces (layered_prepare replaces them when the chunk length changes) and the ones a call grows (DevBuf::ensure).
struct BatchWs {
    DevBuf<>& buf;
    size_t bytes;
    const char* what;
};
std::vector<BatchWs> batch_workspaces(Handle& h) {
    const size_t Bm = (size_t)h.cfg.max_batch, rows = Bm * h.cfg.H;
    return {
        {h.d_tiles_ws, rows * h.cfg.nx * h.nin * h.esz, "tiles workspace"},
        {h.d_hess_ws, rows * h.nin * h.nin * h.esz, "Lagrangian blocks workspace"},
        {h.d_kkt_grad, Bm * h.n * h.esz, "nempc_kkt_residual gradient"},
        {h.d_sens_ws, h.w == 1 ? sens_ws_doubles(h, Bm) * sizeof(double) : 0, h.w == 1 ? "nempc_sensitivity workspace" : nullptr},
        {h.d_g_ws, g_ws_bytes(h), "defect workspace"},
        {h.d_valu_ws, 0, nullptr},
        {h.d_rk4_stage, 0, nullptr}, {h.d_rk4_nu, 0, nullptr}, {h.d_rk4_ht, 0, nullptr},
    };
}

// nempc_create / nempc_reserve: the listed workspaces (all empty on entry), then the row kernels' own.  Sized and allocated
// here, not inside the first callback: an allocation is a synchronising call, is not stream-capture safe, and an
// out-of-memory belongs to create / reserve, not to the middle of a solve.
int alloc_batch_workspaces(Handle& h) {
    for (const BatchWs& w : batch_workspaces(h))
        if (w.what)
            if (int rc = w.buf.alloc(w.bytes, w.what)) return rc;
    if (h.layered) return layered_reserve(h);
    if (int rc = ensure_valu_ws(h)) return rc;
    return h.layered_hess ? layered_reserve(h) : NEMPC_OK;
}

// nempc_set_objective; every null argument is its default (Q = I, R = 0.1 I, zero references and linear costs)
int set_objective(Handle& h, const double* Q, const double* R, const double* xref, const double* uref, const double* cx,
                  const double* cu) {
    const int nx = h.cfg.nx, nu = h.cfg.nu, H = h.cfg.H;
    ObjHost o;
    o.Q.assign(nx * nx, 0.0);
    o.R.assign(nu * nu, 0.0);
    if (Q) o.Q.assign(Q, Q + nx * nx); else for (int i = 0; i < nx; ++i) o.Q[i * nx + i] = 1.0;
    if (R) o.R.assign(R, R + nu * nu); else for (int i = 0; i < nu; ++i) o.R[i * nu + i] = 0.1;
    o.xref.assign(H * nx, 0.0); o.cx.assign(H * nx, 0.0);
    o.uref.assign(H * nu, 0.0); o.cu.assign(H * nu, 0.0);
    if (xref) o.xref.assign(xref, xref + H * nx);
    if (uref) o.uref.assign(uref, uref + H * nu);
    if (cx) o.cx.assign(cx, cx + H * nx);
    if (cu) o.cu.assign(cu, cu + H * nu);
    return upload_objective(h, o);
}

// nempc_bind_tracking / nempc_bind_bounds: xs / us = one of the two arrays of state / control rows is given
int check_bind(const Handle& h, const char* who, bool xs, bool us, int32_t B, int64_t ld_x, int64_t ld_u) {
    if ((xs || us) && B < 1) return fail(NEMPC_EINVAL, who, ": B (problems the arrays cover) must be >= 1");
    if (xs && ld_x < (int64_t)h.cfg.H * h.cfg.nx) return fail(NEMPC_EINVAL, who, ": ld_x must be at least H * nx");
    if (us && ld_u < (int64_t)h.cfg.H * h.cfg.nu) return fail(NEMPC_EINVAL, who, ": ld_u must be at least H * nu");
    return NEMPC_OK;
}

// The network can run for B problems (nempc_eval, nempc_hess, nempc_hess_gn, nempc_rollout): weights set, extras and
// history bound and covering the batch.  nempc_solve words two of these differently and keeps its own.
int check_network_inputs(const Handle& h, int B, const char* who) {
    if (!h.have_weights) return fail(NEMPC_ESTATE, who, ": call nempc_set_weights first");
    if (h.ne > 0 && !h.d_extra) return fail(NEMPC_ESTATE, who, ": n_extra > 0 but nempc_bind_extra was not called");
    if (h.w > 1 && !h.d_hist_x) return fail(NEMPC_ESTATE, who, ": rolling_window > 1 but nempc_bind_history was not called");
    if ((h.ne > 0 && B > h.extra_B) || (h.w > 1 && B > h.hist_B))
        return fail(NEMPC_EINVAL, who, ": B exceeds the batch the bound extras / history cover");
    return NEMPC_OK;
}

// ---- the post-solve point calls (nempc_kkt_residual, nempc_sensitivity, nempc_kkt_solve): a primal-dual point
// (Z, X0, lam, zl, zu, lb, ub) on a plain-model handle.  Each entry point runs point_enter, then its own argument checks
// (outputs, nrhs, the empty batch, null pointers: their order against each other differs), then point_prepare, then its launch.
int point_enter(nempc_handle hh, int32_t B, const char* who, const char* rolling_refusal) {
    if (!hh) return fail(NEMPC_EINVAL, who, ": null handle");
    const Handle& h = *reinterpret_cast<Handle*>(hh);
    if (h.w > 1) return fail(NEMPC_EUNSUPPORTED, who, rolling_refusal);
    if (B < 0 || B > h.cfg.max_batch) return fail(NEMPC_EINVAL, who, ": B outside [0, max_batch]");
    return NEMPC_OK;
}

// nempc_kkt_residual, nempc_sensitivity, nempc_kkt_solve under a rate or stage-rows binding: they would certify or
// differentiate the problem WITHOUT the penalty, the limits and the rows
int refuse_rate(nempc_handle hh, const char* who) {
    if (reinterpret_cast<Handle*>(hh)->rows.on())
        return fail(NEMPC_EUNSUPPORTED, who, ": a stage-rows binding (nempc_bind_stage_rows) is on: the multipliers of the rows are "
                                             "not mapped back to the caller's problem; unbind it to evaluate the plain problem");
    if (!reinterpret_cast<Handle*>(hh)->rate.on()) return NEMPC_OK;
    return fail(NEMPC_EUNSUPPORTED, who, ": a rate binding (nempc_bind_rate) is on: the multipliers of the augmented problem are not "
                                         "mapped back to the caller's rows; unbind it to evaluate the plain problem");
}

enum : unsigned {
    POINT_TRACKING = 1,   // check the tracking binding's coverage here (without it only an evaluation with grad does)
    POINT_GRAD = 2,       // the objective gradient into d_kkt_grad
    POINT_BLOCKS = 4,     // the Lagrangian blocks into d_hess_ws, and the sweeps' d_sens_ws
};
struct PointCall {
    const double *dlb = nullptr, *dub = nullptr;   // lb / ub on the device (cached_bounds)
    hipStream_t s = nullptr;
    DeviceGuard dg;                                // the handle's device, for the entry point's launch
};
// Coverage of the bindings, the handle's workspaces, the bounds, then the point's tiles and g from one ordinary evaluation --
// whatever nempc_eval launches at this shape, its checks too -- and its blocks from nempc_hess's dispatch, both into buffers
// the handle owns (not the solver's).
int point_prepare(nempc_handle hh, const char* who, unsigned needs, int32_t B, const void* Z, const void* X0,
                  const void* lam, const double* lb, const double* ub, void* stream, PointCall& pc) {
    Handle& h = *reinterpret_cast<Handle*>(hh);
    if ((needs & POINT_TRACKING) && h.track.on() && B > h.track.B)
        return fail(NEMPC_EINVAL, who, ": B exceeds the batch the bound tracking data cover");
    if (h.bbind.on() && B > h.bbind.B) return fail(NEMPC_EINVAL, who, ": B exceeds the batch the bound per-problem bounds cover");
    if (((needs & POINT_GRAD) && !h.d_kkt_grad) || ((needs & POINT_BLOCKS) && (!h.d_sens_ws || !h.d_hess_ws)) ||
        !h.d_kkt_bounds || !h.d_g_ws || !h.d_tiles_ws)
        return fail(NEMPC_ESTATE, who, ": the handle's workspaces are gone (a failed nempc_reserve)");
    pc.s = reinterpret_cast<hipStream_t>(stream);
    if (int rc = cached_bounds(h, lb, ub, who, pc.s, pc.dlb, pc.dub)) return rc;
    void* const grad = (needs & POINT_GRAD) ? h.d_kkt_grad.get() : nullptr;
    if (int rc = nempc_eval(hh, B, Z, X0, nullptr, grad, h.d_g_ws.get(), nullptr, h.d_tiles_ws.get(), nullptr, stream)) return rc;
    // (blocks only: the objective factor, which nempc_hess asks for and only its assembly reads, is not used -- any pointer)
    if (needs & POINT_BLOCKS)
        if (int rc = nempc_hess(hh, B, Z, X0, lam, lam, nullptr, nullptr, h.d_hess_ws.get(), stream)) return rc;
    pc.dg.set(h.cfg.device);
    if (!pc.dg.ok) return fail(NEMPC_EHIP, who, ": hipSetDevice failed");
    return NEMPC_OK;
}

}  // namespace
}  // namespace nempc

using namespace nempc;

extern "C" {

int nempc_abi_version(void) { return NEMPC_ABI_VERSION; }

const char* nempc_last_error(void) { return g_last_error.c_str(); }

int nempc_create(const nempc_config* cfg, nempc_handle* out) {
    if (!cfg || !out) return fail(NEMPC_EINVAL, "nempc_create: null argument");
    *out = nullptr;
    if (cfg->abi_version != NEMPC_ABI_VERSION) return fail(NEMPC_EINVAL, "nempc_create: abi_version mismatch");
    if (cfg->dtype != NEMPC_F64 && cfg->dtype != NEMPC_F32) return fail(NEMPC_EINVAL, "nempc_create: bad dtype");
    if (cfg->integrator < NEMPC_DISCRET || cfg->integrator > NEMPC_RK4)
        return fail(NEMPC_EINVAL, "nempc_create: bad integrator kind");
    if (cfg->H < 1 || cfg->nx < 1 || cfg->nu < 1) return fail(NEMPC_EINVAL, "nempc_create: H, nx, nu must be >= 1");
    if (cfg->n_layers < 1 || cfg->n_layers > NEMPC_MAX_LAYERS)
        return fail(NEMPC_EINVAL, "nempc_create: n_layers out of range");
    if (cfg->widths[cfg->n_layers - 1] != cfg->nx)
        return fail(NEMPC_EINVAL, "nempc_create: last layer width must equal nx (model output = state dim)");
    for (int l = 0; l < cfg->n_layers; ++l) {
        if (cfg->widths[l] < 1) return fail(NEMPC_EINVAL, "nempc_create: layer width must be >= 1");
        if (cfg->activations[l] < 0 || cfg->activations[l] >= NEMPC_ACT_COUNT)
            return fail(NEMPC_EINVAL, "nempc_create: unknown activation code (NEMPC_ACT_*)");
        if (cfg->activations[l] == NEMPC_ACT_ELU && !(cfg->act_param[l] > 0.0))
            return fail(NEMPC_EINVAL, "nempc_create: elu needs act_param (alpha) > 0");
        if (cfg->activations[l] == NEMPC_ACT_LEAKY_RELU && !(cfg->act_param[l] >= 0.0))
            return fail(NEMPC_EINVAL, "nempc_create: leaky_relu needs act_param (alpha) >= 0");
    }
    if (cfg->max_batch < 1) return fail(NEMPC_EINVAL, "nempc_create: max_batch must be >= 1");
    if (cfg->n_extra < 0) return fail(NEMPC_EINVAL, "nempc_create: n_extra must be >= 0");
    if (cfg->kernel < NEMPC_KERNEL_AUTO || cfg->kernel > NEMPC_KERNEL_LAYERED)
        return fail(NEMPC_EINVAL, "nempc_create: bad kernel selector");
    if (cfg->integrator == NEMPC_RK4 && !(cfg->DT > 0.0)) return fail(NEMPC_EINVAL, "nempc_create: RK4 needs DT > 0");
    if (cfg->rolling_window < 1) return fail(NEMPC_EINVAL, "nempc_create: rolling_window must be >= 1");
    if (cfg->rolling_window > 1 && cfg->integrator == NEMPC_RK4)
        return fail(NEMPC_EUNSUPPORTED, "nempc_create: rolling-window models need the DISCRET or UNITY integrator");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(NEMPC_EHIP, "nempc_create: no HIP device visible (this library has no CPU fallback)");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(NEMPC_EINVAL, "nempc_create: device ordinal out of range");
    DeviceGuard dg(cfg->device);
    if (!dg.ok) return fail(NEMPC_EHIP, "nempc_create: hipSetDevice failed");

    Handle* h = new (std::nothrow) Handle();
    if (!h) return fail(NEMPC_ENOMEM, "nempc_create: out of host memory");
    h->cfg = *cfg;
    h->esz = cfg->dtype == NEMPC_F64 ? 8 : 4;
    h->w = cfg->rolling_window;
    h->rev = cfg->rolling_reverse ? 1 : 0;
    h->nin = h->w * (cfg->nx + cfg->nu);
    h->ne = cfg->n_extra;
    h->n = cfg->H * (cfg->nx + cfg->nu);
    h->nl = cfg->n_layers;
    h->maxw = 1;
    for (int l = 0; l < h->nl; ++l) {
        h->din[l] = l == 0 ? h->nin + h->ne : cfg->widths[l - 1];
        h->dout[l] = cfg->widths[l];
        if (l < h->nl - 1 && h->dout[l] > h->maxw) h->maxw = h->dout[l];
        h->act[l] = cfg->activations[l];
        h->actp[l] = cfg->act_param[l];
    }
    // matrix-core kernels: one non-linear activation on every hidden layer, linear output
    h->mfma_act = -1;
    if (h->nl >= 2 && h->act[h->nl - 1] == NEMPC_ACT_LINEAR && h->act[0] != NEMPC_ACT_LINEAR) {
        h->mfma_act = h->act[0];
        for (int l = 1; l < h->nl - 1; ++l)
            if (h->act[l] != h->act[0]) h->mfma_act = -1;
        // (the register-resident kernels are instantiated for tanh, relu, sigmoid, softplus and elu with alpha = 1)
        if (h->mfma_act > NEMPC_ACT_ELU) h->mfma_act = -1;
        for (int l = 0; l < h->nl - 1; ++l)
            if (h->act[l] == NEMPC_ACT_ELU && h->actp[l] != 1.0) h->mfma_act = -1;
    }
    // ... or any per-layer mix of the activations written from the layer's output (linear .. selu; elu / leaky_relu with
    // any alpha): the same kernels with the hidden layers' codes as launch arguments (NEMPC_ACT_RUNTIME instantiations)
    if (h->mfma_act < 0 && h->nl >= 2 && h->act[h->nl - 1] == NEMPC_ACT_LINEAR) {
        bool ok = true;
        for (int l = 0; l < h->nl - 1; ++l) ok = ok && h->act[l] >= NEMPC_ACT_LINEAR && h->act[l] < NEMPC_ACT_FIRST_ZBASED;
        static const bool rt_off = !env_enabled("NEMPC_MFMA_RUNTIME_ACT");    // (A/B: the layered path instead)
        if (ok && !rt_off) h->mfma_act = NEMPC_ACT_RUNTIME;
    }
    {
        // compute units of the device: every "fill the chip" launch geometry is sized from this, never from a literal.
        // NEMPC_NUM_CUS overrides it (tests of the launch planning on the one device a box has).
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess) {
            if (prop.multiProcessorCount > 0) h->num_cus = prop.multiProcessorCount;
            // (the LDS a workgroup may ask for: the RK4 congruence kernel sizes its workgroups by it, kernels_rk4hess.hip)
            if (prop.sharedMemPerBlock > 0) h->lds_limit = prop.sharedMemPerBlock;
        }
        if (const int v = env_int("NEMPC_NUM_CUS", 0); v > 0) h->num_cus = v;
    }
    h->variant = NEMPC_KERNEL_VALU;
    // swish / gelu / softsign / mish / exponential / relu6 are written from the pre-activation: the layered path (any layer,
    // the output layer included: its output step has z) and the generic kernel (which keeps s', s'' of every unit from its
    // forward pass) take them; the register-resident matrix-core kernels do not (mfma_act stays -1 for such a network)
    if (cfg->kernel == NEMPC_KERNEL_MFMA || cfg->kernel == NEMPC_KERNEL_MFMA_TILE) {
        if (!mfma_supported(*h)) {
            delete h;
            return fail(NEMPC_EUNSUPPORTED, "nempc_create: MFMA row kernel does not cover these layer dims / activations");
        }
        h->variant = cfg->kernel;
    } else if (cfg->kernel == NEMPC_KERNEL_AUTO && mfma_supported(*h) && !mfma_slower_than_layered(*h)) {
        h->variant = NEMPC_KERNEL_MFMA;
        h->layered_hess = mfma_hess_on_layered(*h);
    } else if (cfg->kernel == NEMPC_KERNEL_LAYERED || cfg->kernel == NEMPC_KERNEL_AUTO) {
        // wide / deep / mixed-activation networks: rows through the layer-at-a-time GEMM pipeline (kernels_layered.hip).
        // Internally the handle stays on the generic variant -- Hessian blocks and everything else the pipeline does not
        // produce come from the generic kernels -- with launch_rows_valu handing the rows over
        if (layered_supported(*h)) {
            h->layered = true;
        } else if (cfg->kernel == NEMPC_KERNEL_LAYERED) {
            delete h;
            return fail(NEMPC_EUNSUPPORTED, "nempc_create: the layered matrix-core path needs >= 1 hidden layer, hidden widths <= 1024, "
                                            "w*(nx+nu) <= 128 and nx <= 64");
        }
    }

    int rc;
    if ((rc = rebuild_structure(*h)) ||                                          // (the row count: d_g_ws is sized by it)
        (rc = alloc_batch_workspaces(*h)) || (rc = h->d_kkt_bounds.alloc((size_t)2 * h->n * sizeof(double), "variable bounds")) ||
        (rc = set_objective(*h, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr))) {
        delete h;           // (frees set no error text: the failure's message stands)
        return rc;
    }
    *out = reinterpret_cast<nempc_handle>(h);
    return NEMPC_OK;
}

int nempc_destroy(nempc_handle hh) {
    if (!hh) return NEMPC_OK;
    Handle* h = reinterpret_cast<Handle*>(hh);
    DeviceGuard dg(h->cfg.device);
    h->jac_resident.drop_all();
    delete h;
    return NEMPC_OK;
}

int nempc_reserve(nempc_handle hh, int32_t max_batch) {
    if (!hh) return fail(NEMPC_EINVAL, "nempc_reserve: null handle");
    Handle& h = *reinterpret_cast<Handle*>(hh);
    if (max_batch < 1) return fail(NEMPC_EINVAL, "nempc_reserve: max_batch must be >= 1");
    if (max_batch <= h.cfg.max_batch) return NEMPC_OK;
    DeviceGuard dg(h.cfg.device);
    if (!dg.ok) return fail(NEMPC_EHIP, "nempc_reserve: hipSetDevice failed");
    // an evaluation may still be running out of the old workspaces on some stream
    NEMPC_HIP(hipDeviceSynchronize());
    h.cfg.max_batch = max_batch;
    solver_free(h);
    for (const BatchWs& w : batch_workspaces(h)) w.buf.reset();
    const int rc = alloc_batch_workspaces(h);
    if (rc) h.cfg.max_batch = 0;   // workspaces are gone: every evaluation is refused until a reserve succeeds
    return rc;
}

int nempc_set_weights(nempc_handle hh, const double* const* W, const double* const* b) {
    if (!hh || !W || !b) return fail(NEMPC_EINVAL, "nempc_set_weights: null argument");
    Handle& h = *reinterpret_cast<Handle*>(hh);
    DeviceGuard dg(h.cfg.device);
    if (!dg.ok) return fail(NEMPC_EHIP, "nempc_set_weights: hipSetDevice failed");
    // every layer into new buffers first, into the handle only when all of them are up: a failure leaves the previous network
    DevBuf<> nW[NEMPC_MAX_LAYERS], nWt[NEMPC_MAX_LAYERS], nb[NEMPC_MAX_LAYERS];
    for (int l = 0; l < h.nl; ++l) {
        if (!W[l] || !b[l]) return fail(NEMPC_EINVAL, "nempc_set_weights: null layer pointer");
        const int win = h.din[l], wout = h.dout[l];
        for (size_t i = 0; i < (size_t)win * wout; ++i)
            if (!std::isfinite(W[l][i])) return fail(NEMPC_EINVAL, "nempc_set_weights: non-finite weight");
        std::vector<double> w(W[l], W[l] + (size_t)win * wout), wt((size_t)win * wout), bb(b[l], b[l] + wout);
        for (int i = 0; i < win; ++i)
            for (int j = 0; j < wout; ++j) wt[(size_t)j * win + i] = w[(size_t)i * wout + j];
        int rc;
        if ((rc = nW[l].alloc(w.size() * h.esz, "layer weights"))) return rc;
        if ((rc = nWt[l].alloc(wt.size() * h.esz, "transposed layer weights"))) return rc;
        if ((rc = nb[l].alloc(bb.size() * h.esz, "layer biases"))) return rc;
        if ((rc = upload(h, w, nW[l].get()))) return rc;
        if ((rc = upload(h, wt, nWt[l].get()))) return rc;
        if ((rc = upload(h, bb, nb[l].get()))) return rc;
    }
    // (the packed copy of the matrix-core kernels likewise: it replaces the old one only once it is up, and nothing after it fails)
    if (h.variant != NEMPC_KERNEL_VALU)
        if (int rc = mfma_pack_weights(h, W, b)) return rc;
    for (int l = 0; l < h.nl; ++l) {
        h.d_W[l] = std::move(nW[l]); h.d_Wt[l] = std::move(nWt[l]); h.d_b[l] = std::move(nb[l]);
    }
    h.have_weights = true;
    h.layered_pairs_valid = false;      // (the layered Hessian's table of first-layer weight products follows the weights)
    return NEMPC_OK;
}

int nempc_set_objective(nempc_handle hh, const double* Q, const double* R, const double* xref, const double* uref,
                        const double* cx, const double* cu) {
    if (!hh) return fail(NEMPC_EINVAL, "nempc_set_objective: null handle");
    Handle& h = *reinterpret_cast<Handle*>(hh);
    DeviceGuard dg(h.cfg.device);
    if (!dg.ok) return fail(NEMPC_EHIP, "nempc_set_objective: hipSetDevice failed");
    return set_objective(h, Q, R, xref, uref, cx, cu);
}

int nempc_set_terminal_weight(nempc_handle hh, const double* QT) {
    if (!hh) return fail(NEMPC_EINVAL, "nempc_set_terminal_weight: null handle");
    Handle& h = *reinterpret_cast<Handle*>(hh);
    DeviceGuard dg(h.cfg.device);
    if (!dg.ok) return fail(NEMPC_EHIP, "nempc_set_terminal_weight: hipSetDevice failed");
    const int nx = h.cfg.nx;
    if (QT) h.obj_QT.assign(QT, QT + nx * nx); else h.obj_QT.clear();
    const ObjHost keep = h.obj_host;
    return upload_objective(h, keep);
}

int nempc_bind_extra(nempc_handle hh, const void* E, int32_t B) {
    if (!hh) return fail(NEMPC_EINVAL, "nempc_bind_extra: null handle");
    Handle& h = *reinterpret_cast<Handle*>(hh);
    if (h.ne == 0 && E) return fail(NEMPC_EINVAL, "nempc_bind_extra: the handle was created with n_extra = 0");
    if (E && B < 1) return fail(NEMPC_EINVAL, "nempc_bind_extra: B (problems the tensor covers) must be >= 1");
    h.d_extra = E;
    h.extra_B = E ? B : 0;
    return NEMPC_OK;
}

int nempc_bind_history(nempc_handle hh, const void* hist_x, const void* hist_u, int32_t B) {
    if (!hh) return fail(NEMPC_EINVAL, "nempc_bind_history: null handle");
    Handle& h = *reinterpret_cast<Handle*>(hh);
    if (h.w == 1 && (hist_x || hist_u))
        return fail(NEMPC_EINVAL, "nempc_bind_history: the handle was created with rolling_window = 1");
    if (h.w > 1 && (!hist_x != !hist_u)) return fail(NEMPC_EINVAL, "nempc_bind_history: bind both histories or neither");
    if (hist_x && B < 1) return fail(NEMPC_EINVAL, "nempc_bind_history: B (problems the tensors cover) must be >= 1");
    h.d_hist_x = hist_x;
    h.d_hist_u = hist_u;
    h.hist_B = hist_x ? B : 0;
    return NEMPC_OK;
}

int nempc_bind_tracking(nempc_handle hh, const void* xref, const void* uref, const void* cx, const void* cu, int32_t B,
                        int64_t ld_x, int64_t ld_u) {
    if (!hh) return fail(NEMPC_EINVAL, "nempc_bind_tracking: null handle");
    Handle& h = *reinterpret_cast<Handle*>(hh);
    const bool xs = xref || cx, us = uref || cu;
    if (int rc = check_bind(h, "nempc_bind_tracking", xs, us, B, ld_x, ld_u)) return rc;
    h.track = (xs || us) ? TrackBind{xref, uref, cx, cu, ld_x, ld_u, B} : TrackBind{};
    return NEMPC_OK;
}

int nempc_bind_bounds(nempc_handle hh, const void* xlb, const void* xub, const void* ulb, const void* uub, int32_t B,
                      int64_t ld_x, int64_t ld_u) {
    if (!hh) return fail(NEMPC_EINVAL, "nempc_bind_bounds: null handle");
    Handle& h = *reinterpret_cast<Handle*>(hh);
    const bool xs = xlb || xub, us = ulb || uub;
    if (int rc = check_bind(h, "nempc_bind_bounds", xs, us, B, ld_x, ld_u)) return rc;
    h.bbind = (xs || us) ? BoundBind{xlb, xub, ulb, uub, ld_x, ld_u, B} : BoundBind{};
    return NEMPC_OK;
}

int nempc_bind_rate(nempc_handle hh, const double* S, const double* dlo, const double* dhi, int32_t per_stage,
                    const void* u_prev, int32_t B) {
    if (!hh) return fail(NEMPC_EINVAL, "nempc_bind_rate: null handle");
    Handle& h = *reinterpret_cast<Handle*>(hh);
    if (!S && !dlo && !dhi && !u_prev) { h.rate = RateBind{}; return NEMPC_OK; }
    if (h.w > 1)
        return fail(NEMPC_EUNSUPPORTED, "nempc_bind_rate: rolling_window > 1 handles are not supported (the window state and the "
                                        "rate state are two augmentations of the stage; their combination is not built)");
    if (!u_prev) return fail(NEMPC_EINVAL, "nempc_bind_rate: u_prev is required whenever S, dlo or dhi is given");
    if (B < 1) return fail(NEMPC_EINVAL, "nempc_bind_rate: B (problems u_prev covers) must be >= 1");
    if (per_stage != 0 && per_stage != 1) return fail(NEMPC_EINVAL, "nempc_bind_rate: per_stage must be 0 or 1");
    const int H = h.cfg.H, nu = h.cfg.nu;
    RateBind rb;
    rb.u_prev = u_prev; rb.B = B;
    rb.S.assign((size_t)nu * nu, 0.0);
    if (S)
        for (int i = 0; i < nu * nu; ++i) {
            if (!std::isfinite(S[i])) return fail(NEMPC_EINVAL, "nempc_bind_rate: S has a non-finite entry");
            rb.S[i] = S[i];
        }
    rb.dlo.assign((size_t)H * nu, -INFINITY);
    rb.dhi.assign((size_t)H * nu, INFINITY);
    for (int t = 0; t < H; ++t)
        for (int j = 0; j < nu; ++j) {
            const int e = per_stage ? t * nu + j : j;
            const double lo = dlo ? dlo[e] : -INFINITY, hi = dhi ? dhi[e] : INFINITY;
            if (std::isnan(lo) || std::isnan(hi)) return fail(NEMPC_EINVAL, "nempc_bind_rate: a limit is NaN");
            if (lo >= hi)
                return fail(NEMPC_EINVAL, "nempc_bind_rate: dlo >= dhi (a fixed or empty move has no interior for the barrier)");
            rb.dlo[(size_t)t * nu + j] = lo; rb.dhi[(size_t)t * nu + j] = hi;
        }
    h.rate = std::move(rb);
    return NEMPC_OK;
}

int nempc_bind_stage_rows(nempc_handle hh, int32_t nc, const double* C, const double* rlo, const double* rhi, int32_t per_stage) {
    if (!hh) return fail(NEMPC_EINVAL, "nempc_bind_stage_rows: null handle");
    Handle& h = *reinterpret_cast<Handle*>(hh);
    if (nc < 0) return fail(NEMPC_EINVAL, "nempc_bind_stage_rows: nc must be >= 0");
    if (nc == 0 || !C) { h.rows = RowsBind{}; return NEMPC_OK; }      // (d_rows_C stays: a launch in flight may still read it)
    if (h.w > 1)
        return fail(NEMPC_EUNSUPPORTED, "nempc_bind_stage_rows: rolling_window > 1 handles are not supported (the window state and "
                                        "the row state are two augmentations of the stage; their combination is not built)");
    if (per_stage != 0 && per_stage != 1) return fail(NEMPC_EINVAL, "nempc_bind_stage_rows: per_stage must be 0 or 1");
    const int H = h.cfg.H, nio = h.cfg.nx + h.cfg.nu;
    RowsBind rb;
    rb.nc = nc;
    rb.C.assign(C, C + (size_t)nc * nio);
    for (double c : rb.C)
        if (!std::isfinite(c)) return fail(NEMPC_EINVAL, "nempc_bind_stage_rows: C has a non-finite entry");
    rb.lo.assign((size_t)H * nc, -INFINITY);
    rb.hi.assign((size_t)H * nc, INFINITY);
    const RowsDims d = rows_dims(H, h.cfg.nx, h.cfg.nu, nc);
    for (int t = 0; t < H; ++t)
        for (int k = 0; k < nc; ++k) {
            const int e = rows_limit_entry(d, t, k, per_stage);
            const double lo = rlo ? rlo[e] : -INFINITY, hi = rhi ? rhi[e] : INFINITY;
            if (std::isnan(lo) || std::isnan(hi)) return fail(NEMPC_EINVAL, "nempc_bind_stage_rows: a limit is NaN");
            if (lo >= hi)
                return fail(NEMPC_EINVAL, "nempc_bind_stage_rows: rlo >= rhi (an equality or empty row has no interior for the barrier)");
            rb.lo[(size_t)t * nc + k] = lo; rb.hi[(size_t)t * nc + k] = hi;
        }
    // C in the handle's dtype on the device, each element cast once
    DeviceGuard dg(h.cfg.device);
    if (!dg.ok) return fail(NEMPC_EHIP, "nempc_bind_stage_rows: hipSetDevice failed");
    const size_t ne = rb.C.size(), bytes = ne * h.esz;
    if (int rc = h.d_rows_C.ensure(bytes, "stage rows C")) return rc;
    if (h.cfg.dtype == NEMPC_F64) {
        NEMPC_HIP(hipMemcpy(h.d_rows_C.get(), rb.C.data(), bytes, hipMemcpyHostToDevice));
    } else {
        const std::vector<float> cf(rb.C.begin(), rb.C.end());
        NEMPC_HIP(hipMemcpy(h.d_rows_C.get(), cf.data(), bytes, hipMemcpyHostToDevice));
    }
    h.rows = std::move(rb);
    return NEMPC_OK;
}

int nempc_set_box_rows(nempc_handle hh, int enabled, const double* lo, const double* hi) {
    if (!hh) return fail(NEMPC_EINVAL, "nempc_set_box_rows: null handle");
    Handle& h = *reinterpret_cast<Handle*>(hh);
    DeviceGuard dg(h.cfg.device);
    if (!dg.ok) return fail(NEMPC_EHIP, "nempc_set_box_rows: hipSetDevice failed");
    if (enabled && (!lo || !hi)) return fail(NEMPC_EINVAL, "nempc_set_box_rows: lo/hi required when enabled");
    h.box = enabled != 0;
    h.box_lo.clear();
    h.box_hi.clear();
    if (h.box) {
        h.box_lo.assign(lo, lo + h.cfg.nx);
        h.box_hi.assign(hi, hi + h.cfg.nx);
    }
    h.d_g_ws.reset();       // (its row count changes: no buffer of the old one behind a failure)
    if (int rc = rebuild_structure(h)) return rc;
    return h.d_g_ws.alloc(g_ws_bytes(h), "defect workspace");
}

int nempc_jac_dense_resident(nempc_handle hh, void* jac, int32_t B) {
    if (!hh) return fail(NEMPC_EINVAL, "nempc_jac_dense_resident: null handle");
    Handle& h = *reinterpret_cast<Handle*>(hh);
    if (B < 0 || B > h.cfg.max_batch) return fail(NEMPC_EINVAL, "nempc_jac_dense_resident: B outside [0, max_batch]");
    if (B == 0) {                     // removal; a pointer the table does not hold is not an error
        h.jac_resident.remove(jac);
        return NEMPC_OK;
    }
    if (!jac) return fail(NEMPC_EINVAL, "nempc_jac_dense_resident: jac is null");
    if (!h.jac_resident.find(jac) && h.jac_resident.count() == kJacResidentSlots) return NEMPC_EFULL;   // (no message: not an error)
    DeviceGuard dg(h.cfg.device);
    if (!dg.ok) return fail(NEMPC_EHIP, "nempc_jac_dense_resident: hipSetDevice failed");
    // a set-up call: whatever still runs on any stream is over before the fill, and the fill before the call returns
    h.jac_resident.remove(jac);
    NEMPC_HIP(hipDeviceSynchronize());
    NEMPC_HIP(hipMemset(jac, 0, (size_t)B * h.m * h.n * h.esz));
    NEMPC_HIP(hipDeviceSynchronize());
    h.jac_resident.add(jac, B);
    return NEMPC_OK;
}

int nempc_dims(nempc_handle hh, int32_t* n, int32_t* m, int32_t* nnz_jac, int32_t* nnz_hess) {
    if (!hh) return fail(NEMPC_EINVAL, "nempc_dims: null handle");
    Handle& h = *reinterpret_cast<Handle*>(hh);
    if (n) *n = h.n;
    if (m) *m = h.m;
    if (nnz_jac) *nnz_jac = (int32_t)h.jac_rows.size();
    if (nnz_hess) *nnz_hess = (int32_t)h.hess_rows.size();
    return NEMPC_OK;
}

int nempc_constraint_bounds(nempc_handle hh, double* cl, double* cu) {
    if (!hh || !cl || !cu) return fail(NEMPC_EINVAL, "nempc_constraint_bounds: null argument");
    Handle& h = *reinterpret_cast<Handle*>(hh);
    const int hx = h.cfg.H * h.cfg.nx;
    for (int i = 0; i < hx; ++i) cl[i] = cu[i] = 0.0;
    if (h.box)
        for (int t = 0; t < h.cfg.H; ++t)
            for (int i = 0; i < h.cfg.nx; ++i) {
                cl[hx + t * h.cfg.nx + i] = h.box_lo[i];
                cu[hx + t * h.cfg.nx + i] = h.box_hi[i];
            }
    return NEMPC_OK;
}

int nempc_jac_structure(nempc_handle hh, int32_t* rows, int32_t* cols) {
    if (!hh || !rows || !cols) return fail(NEMPC_EINVAL, "nempc_jac_structure: null argument");
    Handle& h = *reinterpret_cast<Handle*>(hh);
    std::memcpy(rows, h.jac_rows.data(), h.jac_rows.size() * sizeof(int32_t));
    std::memcpy(cols, h.jac_cols.data(), h.jac_cols.size() * sizeof(int32_t));
    return NEMPC_OK;
}

int nempc_hess_structure(nempc_handle hh, int32_t* rows, int32_t* cols) {
    if (!hh || !rows || !cols) return fail(NEMPC_EINVAL, "nempc_hess_structure: null argument");
    Handle& h = *reinterpret_cast<Handle*>(hh);
    std::memcpy(rows, h.hess_rows.data(), h.hess_rows.size() * sizeof(int32_t));
    std::memcpy(cols, h.hess_cols.data(), h.hess_cols.size() * sizeof(int32_t));
    return NEMPC_OK;
}

int nempc_eval(nempc_handle hh, int32_t B, const void* Z, const void* X0, void* f, void* grad, void* g,
               void* jac_dense, void* jac_tiles, void* jac_sparse, void* stream) {
    if (!hh) return fail(NEMPC_EINVAL, "nempc_eval: null handle");
    Handle& h = *reinterpret_cast<Handle*>(hh);
    if (B < 0 || B > h.cfg.max_batch) return fail(NEMPC_EINVAL, "nempc_eval: B outside [0, max_batch]");
    if (B == 0) return NEMPC_OK;
    if (!Z) return fail(NEMPC_EINVAL, "nempc_eval: Z is null");
    const bool need_rows = g || jac_dense || jac_tiles || jac_sparse;
    if (need_rows && !X0) return fail(NEMPC_EINVAL, "nempc_eval: X0 is null");
    if (need_rows)
        if (int rc = check_network_inputs(h, B, "nempc_eval")) return rc;
    // per-problem tracking data (nempc_bind_tracking): the launches that fuse the shared objective get no f / grad (ff, gf)
    // and the binding's own kernel follows them (launch_objective below)
    const bool trk = (f || grad) && h.track.on();
    if (trk && B > h.track.B) return fail(NEMPC_EINVAL, "nempc_eval: B exceeds the batch the bound tracking data cover");
    void* const ff = trk ? nullptr : f;
    void* const gf = trk ? nullptr : grad;
    DeviceGuard dg(h.cfg.device);
    if (!dg.ok) return fail(NEMPC_EHIP, "nempc_eval: hipSetDevice failed");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // a resident dense Jacobian (nempc_jac_dense_resident) has its structural zeros in place: the writers below leave them
    static const int resident_on = env_int("NEMPC_JAC_RESIDENT", 1);
    bool jres = jac_dense && resident_on && h.jac_resident.resident(jac_dense, B);
    // ... and its constant -1 / +1 entries: problems that lack them get them here, once, in front of the launches that then
    // skip them (jac_resident.h).  A stream that is being captured would record the fill without running it: such a call
    // takes the full-matrix path and marks nothing.
    if (jres && h.jac_resident.const_count(jac_dense) < B) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (s) NEMPC_HIP(hipStreamIsCapturing(s, &cap));      // (the null stream cannot be captured)
        if (cap != hipStreamCaptureStatusNone) {
            jres = false;
        } else {
            const int b0 = h.jac_resident.const_count(jac_dense);
            if (int rc0 = launch_jac_constants(h, b0, B, jac_dense, s)) return rc0;
            h.jac_resident.const_filled(jac_dense, B);
        }
    }
    // which kernel writes the dense matrix (nempc_last_dense_writer): the row launch below, or the assembly launch itself
    h.last_dense_writer = DENSE_WRITER_NONE;
    int rc;
    if (need_rows && h.variant == NEMPC_KERNEL_VALU) {
        void* tiles = jac_tiles ? jac_tiles : h.d_tiles_ws.get();
        if ((rc = launch_rows_valu(h, B, Z, X0, g ? g : h.d_g_ws.get(), tiles, s))) return rc;
        // sparse contract with the objective and without the dense matrix: one fused launch
        if (jac_sparse && !jac_dense && (ff || gf)) return launch_post_sparse(h, B, tiles, jac_sparse, Z, ff, gf, s);
        if (jac_sparse && (rc = launch_assemble_sparse(h, B, tiles, jac_sparse, s))) return rc;
        if (jac_dense && (ff || gf)) return launch_post(h, B, tiles, jac_dense, Z, ff, gf, s, jres);
        if (jac_dense && (rc = launch_assemble_dense(h, B, tiles, jac_dense, s, jres))) return rc;
    } else if (need_rows) {
        // One plan (mfma_plan.h) says what the row launch writes itself.  Compiled shape: rows, objective and the dense rows
        // or the band values in ONE launch; without a derivative output (g with f / grad: what a line-search trial needs)
        // the same launch runs its forward passes only.  Any plain-model shape the cooperative kernel takes: the dense rows
        // or the band values in nempc_jac_structure order (what a real Ipopt run wants: SURVEY 8f-2; the reference hands
        // cyipopt the dense (m, n), optimizer/ipopt.py:88-96) AND the objective leave from the row launch -- no assembly
        // launch, no tile round trip through memory, no objective launch.  (A resident matrix gets its zeros from the
        // cooperative kernel all the same: correct, and measured not worth a flag in rows_coop_kernel -- DESIGN 5.2.)
        // Defects only (IpoptProblem.constraints on its own): the matrix-core kernel skips its reverse sweeps.
        RowsOut ro;
        ro.g = g ? g : h.d_g_ws.get(); ro.tiles = jac_tiles; ro.need_tiles = jac_dense || jac_sparse;
        ro.jac = jac_dense; ro.sparse = jac_sparse; ro.f = ff; ro.grad = gf; ro.jac_resident = jres;
        unsigned covers = 0;
        if ((rc = launch_rows_mfma(h, B, Z, X0, ro, s, &covers))) return rc;
        if (covers & COVERS_DENSE) h.last_dense_writer = DENSE_WRITER_ROWS;
        // what the launch left over: assembly, post, objective
        const void* tiles = jac_tiles ? jac_tiles : h.d_tiles_ws.get();
        const bool obj_left = (ff || gf) && !(covers & COVERS_OBJ);
        const bool dense_left = jac_dense && !(covers & COVERS_DENSE), sparse_left = jac_sparse && !(covers & COVERS_SPARSE);
        // sparse contract with the objective and without the dense matrix: one fused launch
        if (sparse_left && !dense_left && obj_left) return launch_post_sparse(h, B, tiles, jac_sparse, Z, ff, gf, s);
        if (sparse_left && (rc = launch_assemble_sparse(h, B, tiles, jac_sparse, s))) return rc;
        if (dense_left && obj_left) return launch_post(h, B, tiles, jac_dense, Z, ff, gf, s, jres);
        if (dense_left && (rc = launch_assemble_dense(h, B, tiles, jac_dense, s, jres))) return rc;
        if (covers & COVERS_OBJ) return NEMPC_OK;
    }
    if ((f || grad) && (rc = launch_objective(h, B, Z, f, grad, s))) return rc;
    return NEMPC_OK;
}

int nempc_hess(nempc_handle hh, int32_t B, const void* Z, const void* X0, const void* lambda, const void* sigma,
               void* hvals, void* hdense, void* hblocks, void* stream) {
    if (!hh) return fail(NEMPC_EINVAL, "nempc_hess: null handle");
    Handle& h = *reinterpret_cast<Handle*>(hh);
    if (B < 0 || B > h.cfg.max_batch) return fail(NEMPC_EINVAL, "nempc_hess: B outside [0, max_batch]");
    if (B == 0) return NEMPC_OK;
    if (!Z || !X0 || !lambda || !sigma) return fail(NEMPC_EINVAL, "nempc_hess: null input");
    if (int rc = check_network_inputs(h, B, "nempc_hess")) return rc;
    DeviceGuard dg(h.cfg.device);
    if (!dg.ok) return fail(NEMPC_EHIP, "nempc_hess: hipSetDevice failed");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int rc;
    void* blocks = hblocks ? hblocks : h.d_hess_ws.get();
    unsigned covers = 0;
    if (h.variant == NEMPC_KERNEL_VALU) rc = launch_rowhess_valu(h, B, Z, X0, lambda, blocks, s);
    else if (h.cfg.integrator == NEMPC_RK4) {
        // (a wave's slice of the congruence step does not fit the device's LDS: generic kernel)
        rc = rk4hess_supported(h) ? launch_rowhess_rk4_mfma(h, B, Z, X0, lambda, blocks, s) : launch_rowhess_valu(h, B, Z, X0, lambda, blocks, s);
    } else {
        // tril values only: the compiled-shape and cooperative Hessian kernels assemble them themselves (one launch)
        HessOut ho;
        ho.blocks = blocks; ho.sigma = sigma;
        if (hvals && !hdense && !hblocks) ho.hvals = hvals;
        rc = launch_rowhess_mfma(h, B, Z, X0, lambda, ho, s, &covers);
    }
    if (rc) return rc;
    if ((!hvals && !hdense) || (covers & COVERS_HVALS)) return NEMPC_OK;
    return launch_assemble_hess(h, B, blocks, sigma, hvals, hdense, s);
}

int nempc_hess_gn(nempc_handle hh, int32_t B, const void* Z, const void* X0, const void* w, const void* sigma,
                  void* hvals, void* hdense, void* hblocks, void* stream) {
    if (!hh) return fail(NEMPC_EINVAL, "nempc_hess_gn: null handle");
    Handle& h = *reinterpret_cast<Handle*>(hh);
    if (B < 0 || B > h.cfg.max_batch) return fail(NEMPC_EINVAL, "nempc_hess_gn: B outside [0, max_batch]");
    if (B == 0) return NEMPC_OK;
    if (!Z || !X0 || !sigma) return fail(NEMPC_EINVAL, "nempc_hess_gn: null input");
    if (int rc = check_network_inputs(h, B, "nempc_hess_gn")) return rc;
    DeviceGuard dg(h.cfg.device);
    if (!dg.ok) return fail(NEMPC_EHIP, "nempc_hess_gn: hipSetDevice failed");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // first-order model only: the row kernel's tiles (no second-order sweep), then the same assembly as nempc_hess.  Compiled
    // shape, tril values only: blocks and assembly in the row launch's epilogue (one launch)
    int rc;
    if (h.variant != NEMPC_KERNEL_VALU) {
        RowsOut ro;
        ro.g = h.d_g_ws.get(); ro.tiles = h.d_tiles_ws.get();
        if (hvals && !hdense && !hblocks) { ro.gn_hvals = hvals; ro.gn_w = w; ro.gn_sigma = sigma; }
        unsigned covers = 0;
        rc = launch_rows_mfma(h, B, Z, X0, ro, s, &covers);
        if (rc == NEMPC_OK && (covers & COVERS_GN)) return rc;
    } else rc = launch_rows_valu(h, B, Z, X0, h.d_g_ws.get(), h.d_tiles_ws.get(), s);
    if (rc) return rc;
    // the caller does not ask for the per-row blocks: the assembly forms their elements where it uses them
    if (!hblocks) return (hvals || hdense) ? launch_assemble_hess_gn(h, B, h.d_tiles_ws.get(), w, sigma, hvals, hdense, s) : NEMPC_OK;
    if ((rc = launch_gn_blocks(h, B, h.d_tiles_ws.get(), w, hblocks, s))) return rc;
    if (!hvals && !hdense) return NEMPC_OK;
    return launch_assemble_hess(h, B, hblocks, sigma, hvals, hdense, s);
}

int nempc_solve(nempc_handle hh, int32_t B, const void* X0, void* Z, const double* lb, const double* ub,
                const nempc_solver_opts* opts, int32_t* status, int32_t* iters, void* stream) {
    return nempc_solve_duals(hh, B, X0, Z, lb, ub, opts, status, iters, nullptr, nullptr, nullptr, stream);
}

int nempc_solve_duals(nempc_handle hh, int32_t B, const void* X0, void* Z, const double* lb, const double* ub,
                      const nempc_solver_opts* opts, int32_t* status, int32_t* iters, void* lam, void* zl, void* zu,
                      void* stream) {
    if (!hh) return fail(NEMPC_EINVAL, "nempc_solve: null handle");
    Handle& h = *reinterpret_cast<Handle*>(hh);
    if (B < 0 || B > h.cfg.max_batch) return fail(NEMPC_EINVAL, "nempc_solve: B outside [0, max_batch]");
    if (B == 0) { if (iters) *iters = 0; return NEMPC_OK; }
    if (!X0 || !Z || !opts || !status) return fail(NEMPC_EINVAL, "nempc_solve: null argument");
    if (!h.have_weights) return fail(NEMPC_ESTATE, "nempc_solve: call nempc_set_weights first");
    if (h.ne > 0 && !h.d_extra) return fail(NEMPC_ESTATE, "nempc_solve: n_extra > 0 but nempc_bind_extra was not called");
    if (h.ne > 0 && B > h.extra_B) return fail(NEMPC_EINVAL, "nempc_solve: B exceeds the batch the bound extras cover");
    if (h.w > 1 && !h.d_hist_x)
        return fail(NEMPC_ESTATE, "nempc_solve: rolling_window > 1 but nempc_bind_history was not called");
    if (h.w > 1 && B > h.hist_B) return fail(NEMPC_EINVAL, "nempc_solve: B exceeds the batch the bound history covers");
    if (h.track.on() && B > h.track.B) return fail(NEMPC_EINVAL, "nempc_solve: B exceeds the batch the bound tracking data cover");
    if (h.track.on() && h.w > 1)
        return fail(NEMPC_EUNSUPPORTED, "nempc_solve: per-problem tracking data (nempc_bind_tracking) on a rolling_window > 1 handle: "
                                        "the objective table over the window state is built on the host");
    if (h.bbind.on() && B > h.bbind.B) return fail(NEMPC_EINVAL, "nempc_solve: B exceeds the batch the bound per-problem bounds cover");
    if (h.bbind.on() && h.w > 1)
        return fail(NEMPC_EUNSUPPORTED, "nempc_solve: per-problem bounds (nempc_bind_bounds) on a rolling_window > 1 handle: "
                                        "the bounds of the window state are built on the host");
    if (h.rate.on()) {
        if (B > h.rate.B) return fail(NEMPC_EINVAL, "nempc_solve: B exceeds the batch the bound u_prev (nempc_bind_rate) covers");
        if (lam || zl || zu)
            return fail(NEMPC_EUNSUPPORTED, "nempc_solve_duals: multipliers under a rate binding (nempc_bind_rate) are not supported (the "
                                            "costates of the augmented state are not mapped back to the caller's rows); pass NULL for "
                                            "lam, zl and zu");
        if (h.w > 1)
            return fail(NEMPC_EUNSUPPORTED, "nempc_solve: a rate binding (nempc_bind_rate) on a rolling_window > 1 handle is not supported");
        if (h.track.on())
            return fail(NEMPC_EUNSUPPORTED, "nempc_solve: per-problem tracking data (nempc_bind_tracking) with a rate binding "
                                            "(nempc_bind_rate): the objective table over the augmented state is built on the host");
        if (h.bbind.on())
            return fail(NEMPC_EUNSUPPORTED, "nempc_solve: per-problem bounds (nempc_bind_bounds) with a rate binding (nempc_bind_rate): "
                                            "the bounds of the augmented state are built on the host");
    }
    if (h.rows.on()) {
        if (lam || zl || zu)
            return fail(NEMPC_EUNSUPPORTED, "nempc_solve_duals: multipliers under a stage-rows binding (nempc_bind_stage_rows) are not "
                                            "supported (the costates of the augmented state are not mapped back to the caller's rows); "
                                            "pass NULL for lam, zl and zu");
        if (h.w > 1)
            return fail(NEMPC_EUNSUPPORTED, "nempc_solve: a stage-rows binding (nempc_bind_stage_rows) on a rolling_window > 1 handle is "
                                            "not supported");
        if (h.rate.on())
            return fail(NEMPC_EUNSUPPORTED, "nempc_solve: a rate binding (nempc_bind_rate) with a stage-rows binding "
                                            "(nempc_bind_stage_rows): the two augmentations of the stage are not combined");
        if (h.track.on())
            return fail(NEMPC_EUNSUPPORTED, "nempc_solve: per-problem tracking data (nempc_bind_tracking) with a stage-rows binding "
                                            "(nempc_bind_stage_rows): the objective table over the augmented state is built on the host");
        if (h.bbind.on())
            return fail(NEMPC_EUNSUPPORTED, "nempc_solve: per-problem bounds (nempc_bind_bounds) with a stage-rows binding "
                                            "(nempc_bind_stage_rows): the bounds of the augmented state are built on the host");
    }
    if (opts->max_iter < 1 || opts->max_linesearch < 1 || !(opts->mu_factor > 0.0 && opts->mu_factor < 1.0) ||
        !(opts->mu_init > 0.0) || !(opts->mu_min > 0.0) || opts->lq_kernel < 0 || opts->lq_kernel > 3)
        return fail(NEMPC_EINVAL, "nempc_solve: bad options");
    DeviceGuard dg(h.cfg.device);
    if (!dg.ok) return fail(NEMPC_EHIP, "nempc_solve: hipSetDevice failed");
    SolverDuals duals;
    duals.lam = lam; duals.zl = zl; duals.zu = zu;
    return solver_run(h, B, X0, Z, lb, ub, *opts, status, iters, duals, reinterpret_cast<hipStream_t>(stream));
}

int nempc_kkt_residual(nempc_handle hh, int32_t B, const void* Z, const void* X0, const void* lam, const void* zl,
                       const void* zu, const double* lb, const double* ub, void* r, void* stat, void* stream) {
    const char* const who = "nempc_kkt_residual";
    if (int rc = point_enter(hh, B, who, ": rolling_window > 1 handles are not supported (the band product is built for the "
                                         "tiles of a plain model)")) return rc;
    if (int rc = refuse_rate(hh, who)) return rc;
    if (B == 0) return NEMPC_OK;
    if (!Z || !X0 || !lam || !r) return fail(NEMPC_EINVAL, "nempc_kkt_residual: null argument (Z, X0, lam and r are required)");
    // (no tracking check of its own: its evaluation asks for grad, and nempc_eval checks the binding then)
    PointCall pc;
    if (int rc = point_prepare(hh, who, POINT_GRAD, B, Z, X0, lam, lb, ub, stream, pc)) return rc;
    Handle& h = *reinterpret_cast<Handle*>(hh);
    return launch_kkt_residual(h, B, Z, h.d_kkt_grad.get(), h.d_g_ws.get(), h.d_tiles_ws.get(), lam, zl, zu, pc.dlb, pc.dub, r, stat, pc.s);
}

int nempc_sensitivity(nempc_handle hh, int32_t B, const void* Z, const void* X0, const void* lam, const void* zl,
                      const void* zu, const double* lb, const double* ub, void* dU0, void* dZ, void* dlam, void* gains,
                      int32_t* status, void* stream) {
    const char* const who = "nempc_sensitivity";
    if (int rc = point_enter(hh, B, who, ": rolling_window > 1 handles are not supported (the sweep is built for the stages "
                                         "of a plain model)")) return rc;
    if (int rc = refuse_rate(hh, who)) return rc;
    if (!dU0 && !dZ && !dlam && !gains) return fail(NEMPC_EINVAL, "nempc_sensitivity: no output asked for (dU0, dZ, dlam, gains all null)");
    if (B == 0) return NEMPC_OK;
    if (!Z || !X0 || !lam || !status)
        return fail(NEMPC_EINVAL, "nempc_sensitivity: null argument (Z, X0, lam and status are required)");
    // (a tracking binding changes no second-order term, but the batch it covers is checked as nempc_kkt_residual's evaluation does)
    PointCall pc;
    if (int rc = point_prepare(hh, who, POINT_TRACKING | POINT_BLOCKS, B, Z, X0, lam, lb, ub, stream, pc)) return rc;
    Handle& h = *reinterpret_cast<Handle*>(hh);
    return launch_sensitivity(h, B, Z, h.d_tiles_ws.get(), h.d_hess_ws.get(), zl, zu, pc.dlb, pc.dub, dU0, dZ, dlam, gains, status, pc.s);
}

int nempc_kkt_solve(nempc_handle hh, int32_t B, const void* Z, const void* X0, const void* lam, const void* zl,
                    const void* zu, const double* lb, const double* ub, int32_t nrhs, const void* rz, const void* rg, void* v,
                    void* w, void* gx0, int32_t* status, void* stream) {
    const char* const who = "nempc_kkt_solve";
    if (int rc = point_enter(hh, B, who, ": rolling_window > 1 handles are not supported (the sweep is built for the stages "
                                         "of a plain model)")) return rc;
    if (int rc = refuse_rate(hh, who)) return rc;
    if (nrhs < 1 || nrhs > 64) return fail(NEMPC_EINVAL, "nempc_kkt_solve: nrhs outside [1, 64]");
    if (!v && !w && !gx0) return fail(NEMPC_EINVAL, "nempc_kkt_solve: no output asked for (v, w, gx0 all null)");
    if (B == 0) return NEMPC_OK;
    if (!Z || !X0 || !lam || !rz || !status)
        return fail(NEMPC_EINVAL, "nempc_kkt_solve: null argument (Z, X0, lam, rz and status are required)");
    // tiles and Lagrangian blocks exactly as nempc_sensitivity gets them
    PointCall pc;
    if (int rc = point_prepare(hh, who, POINT_TRACKING | POINT_BLOCKS, B, Z, X0, lam, lb, ub, stream, pc)) return rc;
    Handle& h = *reinterpret_cast<Handle*>(hh);
    return launch_kkt_solve(h, B, Z, h.d_tiles_ws.get(), h.d_hess_ws.get(), zl, zu, pc.dlb, pc.dub, nrhs, rz, rg, v, w, gx0, status, pc.s);
}

int nempc_n_params(nempc_handle hh, int64_t* P) {
    if (!hh || !P) return fail(NEMPC_EINVAL, "nempc_n_params: null argument");
    *P = wgrad_n_params(*reinterpret_cast<Handle*>(hh));
    return NEMPC_OK;
}

int nempc_weight_grad(nempc_handle hh, int32_t B, const void* Z, const void* X0, const void* lam, const void* v, const void* w,
                      const int32_t* skip, void* gtheta, void* stream) {
    const char* const who = "nempc_weight_grad";
    if (int rc = point_enter(hh, B, who, ": rolling_window > 1 handles are not supported (the sweep is built for the rows of a "
                                         "plain model)")) return rc;
    if ((lam == nullptr) != (v == nullptr)) return fail(NEMPC_EINVAL, who, ": lam and v are given both or neither");
    if (!gtheta) return fail(NEMPC_EINVAL, who, ": gtheta is null");
    if (B > 0 && (!Z || !X0 || !w)) return fail(NEMPC_EINVAL, who, ": null argument (Z, X0 and w are required)");
    Handle& h = *reinterpret_cast<Handle*>(hh);
    if (int rc = check_network_inputs(h, B, who)) return rc;
    DeviceGuard dg(h.cfg.device);
    if (!dg.ok) return fail(NEMPC_EHIP, who, ": hipSetDevice failed");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (B == 0) {        // the empty sum
        NEMPC_HIP(hipMemsetAsync(gtheta, 0, (size_t)wgrad_n_params(h) * h.esz, s));
        return NEMPC_OK;
    }
    return launch_weight_grad(h, B, Z, X0, lam, v, w, skip, gtheta, s);
}

int nempc_extra_grad(nempc_handle hh, int32_t B, const void* Z, const void* X0, const void* lam, const void* v, const void* w,
                     void* gE, void* stream) {
    const char* const who = "nempc_extra_grad";
    if (int rc = point_enter(hh, B, who, ": rolling_window > 1 handles are not supported (the sweep is built for the rows of a "
                                         "plain model)")) return rc;
    Handle& h = *reinterpret_cast<Handle*>(hh);
    if (h.ne == 0) return fail(NEMPC_EINVAL, who, ": the handle was created with n_extra = 0");
    if ((lam == nullptr) != (v == nullptr)) return fail(NEMPC_EINVAL, who, ": lam and v are given both or neither");
    if (!gE) return fail(NEMPC_EINVAL, who, ": gE is null");
    if (B > 0 && (!Z || !X0 || !w)) return fail(NEMPC_EINVAL, who, ": null argument (Z, X0 and w are required)");
    if (int rc = check_network_inputs(h, B, who)) return rc;
    if (B == 0) return NEMPC_OK;
    DeviceGuard dg(h.cfg.device);
    if (!dg.ok) return fail(NEMPC_EHIP, who, ": hipSetDevice failed");
    return launch_extra_grad(h, B, Z, X0, lam, v, w, gE, reinterpret_cast<hipStream_t>(stream));
}

int nempc_last_extra_grad_kernel(nempc_handle hh) {
    if (!hh) return fail(NEMPC_EINVAL, "nempc_last_extra_grad_kernel: null handle");
    return reinterpret_cast<Handle*>(hh)->last_egrad_kernel;
}

int nempc_rollout(nempc_handle hh, int32_t B, const void* X0, void* Z, void* f, void* stream) {
    if (!hh) return fail(NEMPC_EINVAL, "nempc_rollout: null handle");
    Handle& h = *reinterpret_cast<Handle*>(hh);
    if (B < 0 || B > h.cfg.max_batch) return fail(NEMPC_EINVAL, "nempc_rollout: B outside [0, max_batch]");
    if (B == 0) return NEMPC_OK;
    if (!Z || !X0) return fail(NEMPC_EINVAL, "nempc_rollout: null argument");
    if (int rc = check_network_inputs(h, B, "nempc_rollout")) return rc;
    // (cannot fire on a live handle -- nempc_create uploads the default objective -- so its place among the checks is free)
    if (f && !h.have_objective) return fail(NEMPC_ESTATE, "nempc_rollout: f asked for but the handle has no objective");
    if (f && h.track.on() && B > h.track.B)
        return fail(NEMPC_EINVAL, "nempc_rollout: B exceeds the batch the bound tracking data cover");
    const int which = env_int("NEMPC_ROLLOUT_KERNEL", 0);
    if (which < 0 || which > 2) return fail(NEMPC_EINVAL, "nempc_rollout: NEMPC_ROLLOUT_KERNEL must be 1 (generic) or 2 (matrix-core)");
    DeviceGuard dg(h.cfg.device);
    if (!dg.ok) return fail(NEMPC_EHIP, "nempc_rollout: hipSetDevice failed");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (int rc = launch_rollout(h, B, X0, Z, which, s)) return rc;
    return f ? launch_objective(h, B, Z, f, nullptr, s) : NEMPC_OK;
}

int nempc_last_rollout_kernel(nempc_handle hh) {
    if (!hh) return fail(NEMPC_EINVAL, "nempc_last_rollout_kernel: null handle");
    return reinterpret_cast<Handle*>(hh)->last_rollout_kernel;
}

int nempc_sync(nempc_handle hh, void* stream) {
    if (!hh) return fail(NEMPC_EINVAL, "nempc_sync: null handle");
    Handle& h = *reinterpret_cast<Handle*>(hh);
    DeviceGuard dg(h.cfg.device);
    NEMPC_HIP(hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
    return NEMPC_OK;
}

#ifdef NEMPC_STAMPS
// diagnostic library only (tools/diag_stamps.py): allocate / read the stamp buffer: 16 waves x 64 phase stamps of
// workgroup 0, then 16 words per workgroup (timeline of every workgroup, 4096 workgroups at most)
#define NEMPC_DBG_WORDS (1024 + 4096 * 16)
int nempc_debug_stamps(nempc_handle hh, long long* host_out) {
    Handle& h = *reinterpret_cast<Handle*>(hh);
    DeviceGuard dg(h.cfg.device);
    if (!h.d_dbg) {
        if (int rc = h.d_dbg.alloc(sizeof(long long) * NEMPC_DBG_WORDS, "stamp buffer")) return rc;
        NEMPC_HIP(hipMemset(h.d_dbg.get(), 0, sizeof(long long) * NEMPC_DBG_WORDS));
        return NEMPC_OK;
    }
    NEMPC_HIP(hipDeviceSynchronize());
    NEMPC_HIP(hipMemcpy(host_out, h.d_dbg.get(), sizeof(long long) * NEMPC_DBG_WORDS, hipMemcpyDeviceToHost));
    return NEMPC_OK;
}
#endif

int nempc_plan_grid(int32_t ntiles, int32_t num_cus, int32_t per_cu, int32_t* grid, int32_t* tiles_per_wg,
                    int32_t* tiles_rem) {
    if (ntiles < 1 || num_cus < 1 || per_cu < 1 || !grid || !tiles_per_wg || !tiles_rem)
        return fail(NEMPC_EINVAL, "nempc_plan_grid: bad argument");
    const GridPlan g = plan_grid(ntiles, num_cus, per_cu);
    *grid = g.grid; *tiles_per_wg = g.tiles_per_wg; *tiles_rem = g.tiles_rem;
    return NEMPC_OK;
}

int nempc_num_cus(nempc_handle hh) {
    if (!hh) return fail(NEMPC_EINVAL, "nempc_num_cus: null handle");
    return reinterpret_cast<Handle*>(hh)->num_cus;
}

int nempc_last_hess_kernel(nempc_handle hh) {
    if (!hh) return fail(NEMPC_EINVAL, "nempc_last_hess_kernel: null handle");
    return reinterpret_cast<Handle*>(hh)->last_hess_kernel;
}

int nempc_last_lq_kernel(nempc_handle hh) {
    if (!hh) return fail(NEMPC_EINVAL, "nempc_last_lq_kernel: null handle");
    return reinterpret_cast<Handle*>(hh)->last_lq_kernel;
}

int nempc_last_dense_writer(nempc_handle hh) {
    if (!hh) return fail(NEMPC_EINVAL, "nempc_last_dense_writer: null handle");
    return reinterpret_cast<Handle*>(hh)->last_dense_writer;
}

int nempc_last_row_kernel(nempc_handle hh) {
    if (!hh) return fail(NEMPC_EINVAL, "nempc_last_row_kernel: null handle");
    return reinterpret_cast<Handle*>(hh)->last_row_kernel;
}

int nempc_kernel_variant(nempc_handle hh) {
    if (!hh) return fail(NEMPC_EINVAL, "nempc_kernel_variant: null handle");
    const Handle& h = *reinterpret_cast<Handle*>(hh);
    return h.layered ? NEMPC_KERNEL_LAYERED : h.variant;
}

}  // extern "C"
