// KKT solves with caller-supplied right-hand sides (nempc_kkt_solve; no reference counterpart): the adjoint of the solution
// map and the forward sensitivity with respect to any parameter.  One wave per problem, up to four problems per workgroup,
// as sens_kernel (kernels_sens.hip); the recursion is kernels_sens_impl.h's backward stage followed, stage by stage, by the
// affine part of kernels_kktsolve_impl.h, then a forward sweep over the right-hand sides.  The working set of a problem --
// sens_layout plus the right-hand-side dependent kktsolve_layout -- lives in LDS when a workgroup's share fits
// kLqLdsBudget, otherwise both live in a per-problem region of global memory behind the same pointer arithmetic.
// The staging of Sigma, the tiles, the blocks and the objective weights is a copy of sens_kernel's (that kernel's source
// and device code are left as they are); the gains, the value matrices and Sigma of the global plans use the handle's
// nempc_sensitivity workspace, which a call owns only while it runs on the stream.
#include <algorithm>
#include <limits>
#include <string>

#include "kernels_kktsolve_impl.h"
#include "bounds_bind_impl.h"
#include "nempc_internal.h"

namespace nempc {

namespace {

struct KktSolvePlan {
    int ppw;            // problems (= waves) per workgroup
    bool use_lds;       // both working sets in LDS
    bool staged;        // ... and between them Sigma, the gains, the tiles and the blocks of the problem and the objective weights
    size_t stride;      // doubles of sens_layout
    size_t aff;         // doubles of kktsolve_layout at this nrhs
    size_t base;        // LDS bytes in front of the right-hand-side dependent region (a multiple of 16)
    size_t per_problem; // LDS bytes per problem (a multiple of 16)
};

inline size_t even(size_t v) { return (v + 1) & ~(size_t)1; }

KktSolvePlan kktsolve_plan(const Handle& h, int nrhs) {
    KktSolvePlan p;
    const size_t H = (size_t)h.cfg.H, nx = (size_t)h.cfg.nx, nu = (size_t)h.cfg.nu, nin = nx + nu;
    p.stride = (size_t)sens_layout(h.cfg.nx, h.cfg.nu).total;
    p.aff = (size_t)kktsolve_layout(h.cfg.H, h.cfg.nx, h.cfg.nu, nrhs).total;
    const size_t aff_bytes = p.aff * sizeof(double);
    const size_t ws_bytes = p.stride * sizeof(double);
    const size_t staged_bytes = ws_bytes + (even(H * nin) + even(H * nu * nx)) * sizeof(double) +
                                ((H * nx * nin + H * nin * nin + 2 * nx * nx + nu * nu) * h.esz + 15) / 16 * 16;
    const size_t fit = std::min<size_t>(4, kLqLdsBudget / (ws_bytes + aff_bytes)),
                 fit_staged = std::min<size_t>(4, kLqLdsBudget / (staged_bytes + aff_bytes));
    p.use_lds = fit >= 1;
    // (sens_plan never stages at the price of fewer problems per workgroup; here the right-hand sides take LDS of their own
    //  and every one of them re-reads the tiles, so staging may cost up to half the problems of a workgroup)
    p.staged = p.use_lds && fit_staged >= 1 && 2 * fit_staged >= fit;
    p.ppw = p.use_lds ? (int)(p.staged ? fit_staged : fit) : 4;
    p.base = p.staged ? staged_bytes : ws_bytes;
    p.per_problem = p.base + aff_bytes;
    return p;
}

struct KktSolveArgs {
    int B, H, nx, nu, nrhs, ppw, use_lds, staged;
    size_t stride, aff, base, per_problem;
    const void *Z, *tiles, *blocks, *zl, *zu, *obj, *rz, *rg;
    ObjOffsets oo;
    const double *lb, *ub;
    BoundBind bb;
    double *Kst, *Pst, *sig, *scratch;
    void *v, *w, *gx0;
    int32_t* status;
};

template <typename T>
__global__ __launch_bounds__(256) void kktsolve_kernel(KktSolveArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
    const int b = (int)blockIdx.x * a.ppw + wv;
    if (b >= a.B) return;            // (the whole wave leaves; nothing below synchronises across waves)
    const int H = a.H, nx = a.nx, nu = a.nu, nin = nx + nu, n = H * nin, hx = H * nx, nrhs = a.nrhs;
    // the two barriers of sens_kernel: `wsync` also orders the stores to global memory, `lsync` is enough between phases
    // that exchange data through LDS
    auto wsync = [] {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    };
    auto lsync = [] {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };
    unsigned char* mine = lds_raw + (size_t)wv * a.per_problem;
    double* ws = a.use_lds ? reinterpret_cast<double*>(mine) : a.scratch + (size_t)b * (a.stride + a.aff);
    double* aff = a.use_lds ? reinterpret_cast<double*>(mine + a.base) : ws + a.stride;
    double* sig = a.staged ? ws + a.stride : a.sig + (size_t)b * n;
    const T* z = (const T*)a.Z + (size_t)b * n;
    const T* zl = a.zl ? (const T*)a.zl + (size_t)b * n : nullptr;
    const T* zu = a.zu ? (const T*)a.zu + (size_t)b * n : nullptr;
    bool bad = false;
    for (int i = lane; i < n; i += 64) {
        double lo = a.lb ? a.lb[i] : -std::numeric_limits<double>::infinity();
        double hi = a.ub ? a.ub[i] : std::numeric_limits<double>::infinity();
        if (a.bb.B > 0) bound_bind_intersect<T>(a.bb, b, i, hx, lo, hi);
        sig[i] = sens_sigma_entry((double)z[i], zl ? (double)zl[i] : 0.0, zu ? (double)zu[i] : 0.0, lo, hi, bad);
    }
    const bool undefined = __any(bad ? 1 : 0) != 0;
    wsync();
    const T* rz = (const T*)a.rz + (size_t)b * nrhs * n;
    const T* rg = a.rg ? (const T*)a.rg + (size_t)b * nrhs * hx : nullptr;
    T* v = a.v ? (T*)a.v + (size_t)b * nrhs * n : nullptr;
    T* w = a.w ? (T*)a.w + (size_t)b * nrhs * hx : nullptr;
    T* gx0 = a.gx0 ? (T*)a.gx0 + (size_t)b * nrhs * nx : nullptr;
    const T* obj = (const T*)a.obj;
    const T* tl = (const T*)a.tiles + (size_t)b * H * nx * nin;
    const T* bl = (const T*)a.blocks + (size_t)b * H * nin * nin;
    double* Kst = a.Kst + (size_t)b * H * nu * nx;
    const T *Qs = obj + a.oo.Qs, *QTs = obj + a.oo.QTs, *Rs = obj + a.oo.Rs;
    if (a.staged) {
        Kst = sig + ((n + 1) & ~1);
        T* tls = reinterpret_cast<T*>(Kst + ((H * nu * nx + 1) & ~1));
        T* bls = tls + H * nx * nin;
        for (int i = lane; i < H * nx * nin; i += 64) tls[i] = tl[i];
        for (int i = lane; i < H * nin * nin; i += 64) bls[i] = bl[i];
        T* ws_obj = bls + H * nin * nin;            // Qs | QTs | Rs
        for (int i = lane; i < nx * nx; i += 64) {
            ws_obj[i] = obj[a.oo.Qs + i];
            ws_obj[nx * nx + i] = obj[a.oo.QTs + i];
        }
        for (int i = lane; i < nu * nu; i += 64) ws_obj[2 * nx * nx + i] = obj[a.oo.Rs + i];
        tl = tls;
        bl = bls;
        Qs = ws_obj; QTs = ws_obj + nx * nx; Rs = ws_obj + 2 * nx * nx;
        wsync();
    }
    double* Pst = a.Pst + (size_t)b * H * nx * nx;
    int st = 2;
    if (!undefined)
        st = a.use_lds ? kktsolve_problem<T>(lane, 64, lsync, wsync, H, nx, nu, nrhs, tl, bl, Qs, QTs, Rs, sig, rz, rg,
                                             ws, aff, Kst, Pst, v, w, gx0)
                       : kktsolve_problem<T>(lane, 64, wsync, wsync, H, nx, nu, nrhs, tl, bl, Qs, QTs, Rs, sig, rz, rg,
                                             ws, aff, Kst, Pst, v, w, gx0);
    if (st != 0) {
        const T nan = std::numeric_limits<T>::quiet_NaN();
        if (v) for (int i = lane; i < nrhs * n; i += 64) v[i] = nan;
        if (w) for (int i = lane; i < nrhs * hx; i += 64) w[i] = nan;
        if (gx0) for (int i = lane; i < nrhs * nx; i += 64) gx0[i] = nan;
    }
    if (lane == 0) a.status[b] = st;
}

}  // namespace

size_t kktsolve_ws_doubles(const Handle& h, size_t Bmax, int nrhs) {
    const KktSolvePlan p = kktsolve_plan(h, nrhs);
    return p.use_lds ? 0 : Bmax * (p.stride + p.aff);
}

int launch_kkt_solve(Handle& h, int B, const void* Z, const void* tiles, const void* blocks, const void* zl, const void* zu,
                     const double* lb, const double* ub, int nrhs, const void* rz, const void* rg, void* v, void* w, void* gx0,
                     int32_t* status, hipStream_t s) {
    const KktSolvePlan p = kktsolve_plan(h, nrhs);
    const size_t Bm = (size_t)h.cfg.max_batch, H = (size_t)h.cfg.H, nx = (size_t)h.cfg.nx, nu = (size_t)h.cfg.nu;
    // the plan's global region: allocated on the first call that needs one, grown (never shrunk) with nrhs and max_batch
    const size_t need = kktsolve_ws_doubles(h, Bm, nrhs);
    if (int rc = h.d_kktsolve_ws.ensure(need * sizeof(double), "nempc_kkt_solve workspace")) return rc;
    KktSolveArgs a;
    a.B = B; a.H = h.cfg.H; a.nx = h.cfg.nx; a.nu = h.cfg.nu; a.nrhs = nrhs; a.ppw = p.ppw; a.use_lds = p.use_lds ? 1 : 0;
    a.staged = p.staged ? 1 : 0;
    a.stride = p.stride; a.aff = p.aff; a.base = p.base; a.per_problem = p.per_problem;
    a.Z = Z; a.tiles = tiles; a.blocks = blocks; a.zl = zl; a.zu = zu; a.obj = h.d_obj.get(); a.rz = rz; a.rg = rg;
    a.oo = obj_offsets(h.cfg.H, h.cfg.nx, h.cfg.nu);
    a.lb = lb; a.ub = ub; a.bb = h.bbind;
    a.Kst = h.d_sens_ws.as<double>();
    a.Pst = a.Kst + Bm * H * nu * nx;
    a.sig = a.Pst + Bm * H * nx * nx;
    a.scratch = h.d_kktsolve_ws.as<double>();
    a.v = v; a.w = w; a.gx0 = gx0; a.status = status;
    const size_t lds = p.use_lds ? (size_t)p.ppw * p.per_problem : 0;
    const dim3 grid((unsigned)((B + p.ppw - 1) / p.ppw)), block((unsigned)(64 * p.ppw));
    if (h.cfg.dtype == NEMPC_F64) {
        NEMPC_HIP(ensure_dynamic_lds(reinterpret_cast<const void*>(kktsolve_kernel<double>), lds));
        hipLaunchKernelGGL(kktsolve_kernel<double>, grid, block, lds, s, a);
    } else {
        NEMPC_HIP(ensure_dynamic_lds(reinterpret_cast<const void*>(kktsolve_kernel<float>), lds));
        hipLaunchKernelGGL(kktsolve_kernel<float>, grid, block, lds, s, a);
    }
    NEMPC_HIP(hipGetLastError());
    return NEMPC_OK;
}

}  // namespace nempc
