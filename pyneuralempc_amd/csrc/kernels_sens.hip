// Solution sensitivities dz*/dx0 and feedback gains (nempc_sensitivity; no reference counterpart: the reference never
// differentiates its solution).  One wave per problem, up to four problems per workgroup; the recursion itself is
// kernels_sens_impl.h (a gain-only backward Riccati sweep and a closed-loop propagation of nx columns, double whatever
// the handle's dtype), with the entries of each small matrix product dealt out over the 64 lanes and wave-level
// synchronisation between dependent phases, as in solver_lqw_kernel.  The per-problem working set lives in LDS when a
// workgroup's share fits the budget the solver's LQ kernels plan with, otherwise in a per-problem region of global memory
// behind the same pointer arithmetic (states up to 64, network inputs up to 128).  Small problems -- where a stage is a
// handful of entries and every load from global memory sits in the dependent chain of a lone wave -- also stage their
// tiles, blocks, Sigma and gains in LDS, so the sweeps touch global memory only to write results.
#include <algorithm>
#include <limits>

#include "kernels_sens_impl.h"
#include "bounds_bind_impl.h"
#include "nempc_internal.h"

namespace nempc {

namespace {

struct SensPlan {
    int ppw;            // problems (= waves) per workgroup
    bool use_lds;       // working set in LDS
    bool staged;        // ... and behind it Sigma, the gains, the tiles and the blocks of the problem and the objective weights
    size_t stride;      // doubles of one problem's working set
    size_t per_problem; // LDS bytes per problem (a multiple of 16)
};

inline size_t even(size_t v) { return (v + 1) & ~(size_t)1; }

SensPlan sens_plan(const Handle& h) {
    SensPlan p;
    const size_t H = (size_t)h.cfg.H, nx = (size_t)h.cfg.nx, nu = (size_t)h.cfg.nu, nin = nx + nu;
    p.stride = (size_t)sens_layout(h.cfg.nx, h.cfg.nu).total;
    const size_t ws_bytes = p.stride * sizeof(double);
    const size_t staged_bytes = ws_bytes + (even(H * nin) + even(H * nu * nx)) * sizeof(double) +
                                ((H * nx * nin + H * nin * nin + 2 * nx * nx + nu * nu) * h.esz + 15) / 16 * 16;
    const size_t fit = std::min<size_t>(4, kLqLdsBudget / ws_bytes), fit_staged = std::min<size_t>(4, kLqLdsBudget / staged_bytes);
    p.use_lds = fit >= 1;
    p.staged = p.use_lds && fit_staged == fit;     // (never at the price of fewer problems per workgroup)
    p.ppw = p.use_lds ? (int)fit : 4;
    p.per_problem = p.staged ? staged_bytes : ws_bytes;
    return p;
}

struct SensArgs {
    int B, H, nx, nu, ppw, use_lds, staged;
    size_t stride, per_problem;
    const void *Z, *tiles, *blocks, *zl, *zu, *obj;
    ObjOffsets oo;
    const double *lb, *ub;
    BoundBind bb;          // per-problem bounds (nempc_bind_bounds; bb.B == 0: none), intersected with lb / ub
    double *Kst, *Pst, *sig, *scratch;
    void *dU0, *dZ, *dlam, *gains;
    int32_t* status;
};

template <typename T>
__global__ __launch_bounds__(256) void sens_kernel(SensArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int lane = (int)threadIdx.x & 63, wv = (int)threadIdx.x >> 6;
    const int b = (int)blockIdx.x * a.ppw + wv;
    if (b >= a.B) return;            // (the whole wave leaves; nothing below synchronises across waves)
    const int H = a.H, nx = a.nx, nu = a.nu, nin = nx + nu, n = H * nin;
    // two barriers of the wave: `wsync` orders everything including the stores to global memory (the working set in the
    // global-scratch plan, the gains and value matrices between the sweeps); `lsync` is solver_lqw_kernel's, enough between
    // phases that exchange data through LDS and does not wait for the stage's global stores
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
    double* ws = a.use_lds ? reinterpret_cast<double*>(mine) : a.scratch + (size_t)b * a.stride;
    double* sig = a.staged ? ws + a.stride : a.sig + (size_t)b * n;
    const T* z = (const T*)a.Z + (size_t)b * n;
    const T* zl = a.zl ? (const T*)a.zl + (size_t)b * n : nullptr;
    const T* zu = a.zu ? (const T*)a.zu + (size_t)b * n : nullptr;
    bool bad = false;
    for (int i = lane; i < n; i += 64) {
        double lo = a.lb ? a.lb[i] : -std::numeric_limits<double>::infinity();
        double hi = a.ub ? a.ub[i] : std::numeric_limits<double>::infinity();
        if (a.bb.B > 0) bound_bind_intersect<T>(a.bb, b, i, H * nx, lo, hi);
        sig[i] = sens_sigma_entry((double)z[i], zl ? (double)zl[i] : 0.0, zu ? (double)zu[i] : 0.0, lo, hi, bad);
    }
    const bool undefined = __any(bad ? 1 : 0) != 0;
    wsync();
    T* dU0 = a.dU0 ? (T*)a.dU0 + (size_t)b * nu * nx : nullptr;
    T* dZ = a.dZ ? (T*)a.dZ + (size_t)b * n * nx : nullptr;
    T* dlam = a.dlam ? (T*)a.dlam + (size_t)b * H * nx * nx : nullptr;
    T* gains = a.gains ? (T*)a.gains + (size_t)b * H * nu * nx : nullptr;
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
        st = a.use_lds ? sens_problem<T>(lane, 64, lsync, wsync, H, nx, nu, tl, bl, Qs, QTs, Rs, sig,
                                         ws, Kst, Pst, dU0, dZ, dlam, gains)
                       : sens_problem<T>(lane, 64, wsync, wsync, H, nx, nu, tl, bl, Qs, QTs, Rs, sig,
                                         ws, Kst, Pst, dU0, dZ, dlam, gains);
    if (st != 0) {
        const T nan = std::numeric_limits<T>::quiet_NaN();
        if (dU0) for (int i = lane; i < nu * nx; i += 64) dU0[i] = nan;
        if (dZ) for (int i = lane; i < n * nx; i += 64) dZ[i] = nan;
        if (dlam) for (int i = lane; i < H * nx * nx; i += 64) dlam[i] = nan;
        if (gains) for (int i = lane; i < H * nu * nx; i += 64) gains[i] = nan;
    }
    if (lane == 0) a.status[b] = st;
}

}  // namespace

size_t sens_ws_doubles(const Handle& h, size_t Bmax) {
    const SensPlan p = sens_plan(h);
    const size_t H = (size_t)h.cfg.H, nx = (size_t)h.cfg.nx, nu = (size_t)h.cfg.nu;
    return Bmax * (H * nu * nx + H * nx * nx + (size_t)h.n + (p.use_lds ? 0 : p.stride));
}

int launch_sensitivity(Handle& h, int B, const void* Z, const void* tiles, const void* blocks, const void* zl, const void* zu,
                       const double* lb, const double* ub, void* dU0, void* dZ, void* dlam, void* gains, int32_t* status,
                       hipStream_t s) {
    const SensPlan p = sens_plan(h);
    const size_t Bm = (size_t)h.cfg.max_batch, H = (size_t)h.cfg.H, nx = (size_t)h.cfg.nx, nu = (size_t)h.cfg.nu;
    SensArgs a;
    a.B = B; a.H = h.cfg.H; a.nx = h.cfg.nx; a.nu = h.cfg.nu; a.ppw = p.ppw; a.use_lds = p.use_lds ? 1 : 0;
    a.staged = p.staged ? 1 : 0;
    a.stride = p.stride; a.per_problem = p.per_problem;
    a.Z = Z; a.tiles = tiles; a.blocks = blocks; a.zl = zl; a.zu = zu; a.obj = h.d_obj.get();
    a.oo = obj_offsets(h.cfg.H, h.cfg.nx, h.cfg.nu);
    a.lb = lb; a.ub = ub; a.bb = h.bbind;
    a.Kst = h.d_sens_ws.as<double>();
    a.Pst = a.Kst + Bm * H * nu * nx;
    a.sig = a.Pst + Bm * H * nx * nx;
    a.scratch = a.sig + Bm * (size_t)h.n;
    a.dU0 = dU0; a.dZ = dZ; a.dlam = dlam; a.gains = gains; a.status = status;
    const size_t lds = p.use_lds ? (size_t)p.ppw * p.per_problem : 0;
    const dim3 grid((unsigned)((B + p.ppw - 1) / p.ppw)), block((unsigned)(64 * p.ppw));
    if (h.cfg.dtype == NEMPC_F64) {
        NEMPC_HIP(ensure_dynamic_lds(reinterpret_cast<const void*>(sens_kernel<double>), lds));
        hipLaunchKernelGGL(sens_kernel<double>, grid, block, lds, s, a);
    } else {
        NEMPC_HIP(ensure_dynamic_lds(reinterpret_cast<const void*>(sens_kernel<float>), lds));
        hipLaunchKernelGGL(sens_kernel<float>, grid, block, lds, s, a);
    }
    NEMPC_HIP(hipGetLastError());
    return NEMPC_OK;
}

}  // namespace nempc
