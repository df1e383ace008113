// nempc_extra_grad: gE[b,t,:] = d/d e_{b,t} ( w_{b,t} . Phi_t + lam_{b,t} . (T_t v_{b,[t]}) ), e_{b,t} the row of the tensor
// bound by nempc_bind_extra (include/nempc.h).  No reference counterpart: the reference never differentiates through p / tvp.
//
// The same dual-number sweep as nempc_weight_grad's (kernels_wgrad.hip): S is the epsilon coefficient of
// (lam + eps w) . Phi(xi + eps v_[t]), eps^2 = 0; forward on (a, a.), backward on (abar, abar.), through the four weight-shared
// stages under RK4.  What leaves the kernel is the epsilon part of the layer-0 input cotangent at the extras' slots, summed
// over the stages -- no factor rows, no accumulation launch.  Without lam / v the value cotangent and every tangent are zero and
// the SECOND = false instantiation carries one number per unit instead of two.
//
// Mapping (egrad_plan.h): a group of LANES = 1 | 16 | 64 lanes owns a row, a workgroup is one wave.  The lanes of a group stride
// over the units of a layer -- unit j of a pass belongs to lane j % LANES, so a group reads LANES consecutive weights of row k of
// W (forward) or of W' (backward) --, the layer's input is read from LDS as a broadcast, and s'(z), s''(z) z. are written and
// read back by the lane that owns the unit (LDS, or the group's region of the workspace).  One fixed order of every sum; plain
// stores; nothing shared between workgroups.
#include "activations.h"
#include "egrad_plan.h"
#include "nempc_internal.h"

namespace nempc {

namespace {

struct EgNet {
    int nl, nin, nx, ne, nstage, m;
    int din[NEMPC_MAX_LAYERS], dout[NEMPC_MAX_LAYERS], act[NEMPC_MAX_LAYERS];
    int soff[NEMPC_MAX_LAYERS];       // first unit of layer l inside a stage's block of SAVE
    int souts;                        // units of a stage: sum_l out_l
    double actp[NEMPC_MAX_LAYERS];
    const void* W[NEMPC_MAX_LAYERS];
    const void* Wt[NEMPC_MAX_LAYERS];
    const void* b[NEMPC_MAX_LAYERS];
    const void* extra;
    RowGather gk;
};

constexpr int EG_U = 4;      // units a lane carries through one pass over a layer's inputs

// acc[q] += sum_k xa[k] M[k][col[q]] (and accd with xd), M row-major with leading dimension ld, k ascending
template <typename T, int NQ, bool SECOND>
__device__ __forceinline__ void eg_dot(const T* __restrict__ M, int ld, int nk, const T* xa, const T* xd, int sl, const int (&col)[EG_U],
                                       T (&acc)[EG_U], T (&accd)[EG_U]) {
#pragma unroll 4
    for (int k = 0; k < nk; ++k) {
        const T a = xa[k * sl];
        T ad = T(0);
        if constexpr (SECOND) ad = xd[k * sl];
        const T* mr = M + (size_t)k * ld;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const T mv = mr[col[q]];
            acc[q] = fma(a, mv, acc[q]);
            if constexpr (SECOND) accd[q] = fma(ad, mv, accd[q]);
        }
    }
}

// columns c0 .. c0 + cnt - 1 of x' M, lane gl of the group taking columns gl, gl + LANES, ...; store(j, acc, accd) receives
// column c0 + j.  Every lane of the wave runs the same trips (cnt is uniform); lanes past the end compute the last column again
// and store nothing.
template <typename T, int LANES, bool SECOND, class Store>
__device__ __forceinline__ void eg_columns(const T* __restrict__ M, int ld, int nk, const T* xa, const T* xd, int sl, int c0, int cnt,
                                           int gl, Store&& store) {
    for (int jb = 0; jb < cnt; jb += LANES * EG_U) {
        int col[EG_U];
        T acc[EG_U], accd[EG_U];
#pragma unroll
        for (int q = 0; q < EG_U; ++q) {
            const int j = jb + q * LANES + gl;
            col[q] = c0 + (j < cnt ? j : cnt - 1);
            acc[q] = accd[q] = T(0);
        }
        const int nq = (cnt - jb + LANES - 1) / LANES;
        if (nq >= 4) eg_dot<T, 4, SECOND>(M, ld, nk, xa, xd, sl, col, acc, accd);
        else if (nq == 3) eg_dot<T, 3, SECOND>(M, ld, nk, xa, xd, sl, col, acc, accd);
        else if (nq == 2) eg_dot<T, 2, SECOND>(M, ld, nk, xa, xd, sl, col, acc, accd);
        else eg_dot<T, 1, SECOND>(M, ld, nk, xa, xd, sl, col, acc, accd);
#pragma unroll
        for (int q = 0; q < EG_U; ++q) {
            const int j = jb + q * LANES + gl;
            if (j < cnt) store(j, acc[q], accd[q]);
        }
    }
}

// Part 0 of a buffer is what both forms carry (forward: the value a; backward: the epsilon cotangent abar.), part 1 what only
// SECOND does (forward: the tangent a.; backward: the value cotangent abar).
template <typename T, int LANES, bool SECOND, bool SAVE_WS>
__global__ __launch_bounds__(64) void egrad_rows_kernel(EgNet net, T DT, int H, long long rows, int maxdim, long long stride,
                                                        long long save_elems, const T* __restrict__ Z, const T* __restrict__ X0,
                                                        const T* __restrict__ lam, const T* __restrict__ v, const T* __restrict__ w,
                                                        T* __restrict__ ws, T* __restrict__ gE) {
    extern __shared__ __align__(16) unsigned char eg_smem[];
    constexpr int RPW = 64 / LANES;
    constexpr int SL = LANES == 1 ? 64 : 1;
    const int lane = threadIdx.x, grp = lane / LANES, gl = lane % LANES;
    const int nl = net.nl, nx = net.nx, nin = net.nin, ne = net.ne, ns = net.nstage;
    T* const X = reinterpret_cast<T*>(eg_smem) + (LANES == 1 ? (long long)lane : grp * stride);
    T* const K = X + (size_t)4 * maxdim * SL;        // k | k. | kbar. | kbar
    T* const E = K + (size_t)4 * nx * SL;
    T* SV;
    if constexpr (SAVE_WS) SV = ws + (size_t)blockIdx.x * (size_t)(save_elems * RPW) + (LANES == 1 ? (long long)lane : grp * save_elems);
    else SV = E + (size_t)ne * SL;
    auto BUF = [&](int buf, int part) -> T* { return X + (size_t)((buf * 2 + part) * maxdim) * SL; };
    const T s6 = DT / T(6);

    for (long long blk = blockIdx.x; blk * RPW < rows; blk += gridDim.x) {
        const long long row = blk * RPW + grp;
        const long long r = row < rows ? row : rows - 1;       // (a group past the end repeats the last row and stores nothing)
        const int b = (int)(r / H), t = (int)(r % H);
        const T* z = Z + (size_t)b * net.gk.n;
        const T* wrow = w + ((size_t)b * H + t) * nx;
        const T* lrow = SECOND ? lam + (size_t)b * net.m + (size_t)t * nx : nullptr;
        const T* vrow = SECOND ? v + (size_t)b * net.gk.n : nullptr;
        const T* erow = (const T*)net.extra + ((size_t)b * H + t) * ne;

        // ---- forward, stage by stage
        for (int s = 0; s < ns; ++s) {
            const T c = s == 0 ? T(0) : (s == 3 ? DT : T(0.5) * DT);
            for (int d = gl; d < nin; d += LANES) {
                T x = gather_input<T>(net.gk, z, X0, b, t, d), xd = T(0);
                if constexpr (SECOND) xd = d < nx ? (t == 0 ? T(0) : vrow[(t - 1) * nx + d]) : vrow[H * nx + t * (nin - nx) + (d - nx)];
                if (s > 0 && d < nx) {
                    x += c * K[(size_t)d * SL];
                    if constexpr (SECOND) xd += c * K[(size_t)(nx + d) * SL];
                }
                BUF(0, 0)[(size_t)d * SL] = x;
                if constexpr (SECOND) BUF(0, 1)[(size_t)d * SL] = xd;
            }
            for (int j = gl; j < ne; j += LANES) {
                BUF(0, 0)[(size_t)(nin + j) * SL] = erow[j];
                if constexpr (SECOND) BUF(0, 1)[(size_t)(nin + j) * SL] = T(0);
            }
            __syncthreads();
            int cur = 0;
            for (int l = 0; l < nl; ++l) {
                const int win = net.din[l], wout = net.dout[l], code = net.act[l];
                const T par = (T)net.actp[l];
                const T* bias = (const T*)net.b[l];
                const bool last = l == nl - 1;
                T* on = last ? K : BUF(cur ^ 1, 0);
                T* ond = last ? K + (size_t)nx * SL : BUF(cur ^ 1, 1);
                T* sv = SV + (size_t)((s * net.souts + net.soff[l]) * 2) * SL;
                eg_columns<T, LANES, SECOND>((const T*)net.W[l], wout, win, BUF(cur, 0), BUF(cur, 1), SL, 0, wout, gl,
                                             [&](int j, T acc, T accd) {
                    const T zz = acc + bias[j];
                    T a, d1, d2;
                    if (act_zbased(code)) {
                        act_from_z<T>(code, zz, a, d1, d2);
                    } else {
                        a = act_f<T>(code, zz, par);
                        d1 = act_d1<T>(code, a, par);
                        d2 = act_r2<T>(code, a, par) * d1;
                    }
                    on[(size_t)j * SL] = a;
                    sv[(size_t)(2 * j) * SL] = d1;
                    if constexpr (SECOND) {
                        ond[(size_t)j * SL] = d1 * accd;
                        sv[(size_t)(2 * j + 1) * SL] = d2 * accd;
                    }
                });
                __syncthreads();
                cur ^= 1;
            }
        }

        // ---- backward, last stage first.  Cotangent of Phi: (lam, w); of the stage outputs k_s: DT/6 (1, 2, 2, 1) times it, plus
        // c_{s+1} times the state part of the next stage's input cotangent
        for (int s = ns - 1; s >= 0; --s) {
            for (int k = gl; k < nx; k += LANES) {
                T e = wrow[k], p = T(0);
                if constexpr (SECOND) p = lrow[k];
                if (ns > 1) {
                    const T wt = (s == 0 || s == 3) ? s6 : T(2) * s6;
                    e = wt * e + (s == 3 ? T(0) : K[(size_t)(2 * nx + k) * SL]);
                    if constexpr (SECOND) p = wt * p + (s == 3 ? T(0) : K[(size_t)(3 * nx + k) * SL]);
                }
                BUF(0, 0)[(size_t)k * SL] = e;
                if constexpr (SECOND) BUF(0, 1)[(size_t)k * SL] = p;
            }
            // (no barrier: the lane that wrote slot k is the one that scales it next)
            int cur = 0;
            for (int l = nl - 1; l >= 0; --l) {
                const int win = net.din[l], wout = net.dout[l];
                const T* sv = SV + (size_t)((s * net.souts + net.soff[l]) * 2) * SL;
                T* ce = BUF(cur, 0);
                T* cp = BUF(cur, 1);
                for (int j = gl; j < wout; j += LANES) {          // d = abar s',  d. = abar. s' + abar s'' z.
                    const T s1 = sv[(size_t)(2 * j) * SL];
                    const T abd = ce[(size_t)j * SL];
                    if constexpr (SECOND) {
                        const T q = sv[(size_t)(2 * j + 1) * SL], ab = cp[(size_t)j * SL];
                        ce[(size_t)j * SL] = fma(abd, s1, ab * q);
                        cp[(size_t)j * SL] = ab * s1;
                    } else {
                        ce[(size_t)j * SL] = abd * s1;
                    }
                }
                __syncthreads();
                const T* Wt = (const T*)net.Wt[l];      // (out, in) row-major
                if (l > 0) {
                    T* ne0 = BUF(cur ^ 1, 0);
                    T* np0 = BUF(cur ^ 1, 1);
                    eg_columns<T, LANES, SECOND>(Wt, win, wout, ce, cp, SL, 0, win, gl, [&](int i, T acc, T accd) {
                        ne0[(size_t)i * SL] = acc;
                        if constexpr (SECOND) np0[(size_t)i * SL] = accd;
                    });
                } else {
                    // of the first layer's input: the states when an earlier stage reads them, and the extras
                    if (s > 0) {
                        const T c = s == 3 ? DT : T(0.5) * DT;
                        eg_columns<T, LANES, SECOND>(Wt, win, wout, ce, cp, SL, 0, nx, gl, [&](int i, T acc, T accd) {
                            K[(size_t)(2 * nx + i) * SL] = c * acc;
                            if constexpr (SECOND) K[(size_t)(3 * nx + i) * SL] = c * accd;
                        });
                    }
                    eg_columns<T, LANES, SECOND>(Wt, win, wout, ce, cp, SL, nin, ne, gl, [&](int j, T acc, T) {
                        E[(size_t)j * SL] = s == ns - 1 ? acc : E[(size_t)j * SL] + acc;
                    });
                }
                __syncthreads();
                cur ^= 1;
            }
        }
        if (row < rows)
            for (int j = gl; j < ne; j += LANES) gE[(size_t)row * ne + j] = E[(size_t)j * SL];     // (the lane that summed slot j)
    }
}

EgradShape shape_of(const Handle& h) {
    EgradShape s{};
    s.nl = h.nl; s.nstage = h.cfg.integrator == NEMPC_RK4 ? 4 : 1; s.nx = h.cfg.nx; s.ne = h.ne; s.num_cus = h.num_cus; s.esz = h.esz;
    for (int l = 0; l < h.nl; ++l) { s.din[l] = h.din[l]; s.dout[l] = h.dout[l]; }
    return s;
}

template <typename T, int LANES, bool SECOND, bool SAVE_WS>
int launch_form(Handle& h, const EgradPlan& p, const EgNet& net, long long rows, const void* Z, const void* X0, const void* lam,
                const void* v, const void* w, void* gE, hipStream_t s) {
    auto kern = egrad_rows_kernel<T, LANES, SECOND, SAVE_WS>;
    if (p.lds_bytes > 65536) NEMPC_HIP(ensure_dynamic_lds(reinterpret_cast<const void*>(kern), p.lds_bytes));
    hipLaunchKernelGGL(kern, dim3((unsigned)egrad_grid(p, rows)), dim3(64), p.lds_bytes, s, net, (T)h.cfg.DT, h.cfg.H, rows, p.maxdim,
                       p.stride, p.save_elems, (const T*)Z, (const T*)X0, (const T*)lam, (const T*)v, (const T*)w, h.d_egrad_ws.as<T>(),
                       (T*)gE);
    NEMPC_HIP(hipGetLastError());
    return NEMPC_OK;
}

template <typename T, int LANES>
int launch_lanes(Handle& h, const EgradPlan& p, const EgNet& net, long long rows, const void* Z, const void* X0, const void* lam,
                 const void* v, const void* w, void* gE, hipStream_t s) {
    if (v) return p.save_in_lds ? launch_form<T, LANES, true, false>(h, p, net, rows, Z, X0, lam, v, w, gE, s)
                                : launch_form<T, LANES, true, true>(h, p, net, rows, Z, X0, lam, v, w, gE, s);
    return p.save_in_lds ? launch_form<T, LANES, false, false>(h, p, net, rows, Z, X0, lam, v, w, gE, s)
                         : launch_form<T, LANES, false, true>(h, p, net, rows, Z, X0, lam, v, w, gE, s);
}

template <typename T>
int run(Handle& h, const EgradPlan& p, const EgNet& net, long long rows, const void* Z, const void* X0, const void* lam, const void* v,
        const void* w, void* gE, hipStream_t s) {
    if (p.lanes == 1) return launch_lanes<T, 1>(h, p, net, rows, Z, X0, lam, v, w, gE, s);
    if (p.lanes == 16) return launch_lanes<T, 16>(h, p, net, rows, Z, X0, lam, v, w, gE, s);
    return launch_lanes<T, 64>(h, p, net, rows, Z, X0, lam, v, w, gE, s);
}

}  // namespace

// The checked call (nempc_api.hip).  A plan that keeps s', s'' z. in the workspace allocates it on the first call that needs it
// (sized for max_batch, so it never grows before nempc_reserve does): such a call synchronises the device.
int launch_extra_grad(Handle& h, int B, const void* Z, const void* X0, const void* lam, const void* v, const void* w, void* gE,
                      hipStream_t s) {
    const EgradPlan p = egrad_make_plan(shape_of(h));
    if (!p.fits) {
        set_error("nempc_extra_grad: a row's layer buffers do not fit the LDS of a workgroup (widths beyond 1024)");
        return NEMPC_EUNSUPPORTED;
    }
    const size_t bytes = (size_t)egrad_ws_elems(p, (long long)h.cfg.max_batch * h.cfg.H) * h.esz;
    if (int rc = h.d_egrad_ws.ensure(bytes, "nempc_extra_grad workspace")) return rc;
    EgNet net{};
    net.nl = h.nl; net.nin = h.nin; net.nx = h.cfg.nx; net.ne = h.ne; net.nstage = h.cfg.integrator == NEMPC_RK4 ? 4 : 1; net.m = h.m;
    net.extra = h.d_extra; net.gk = h.gather();
    for (int l = 0; l < h.nl; ++l) {
        net.din[l] = h.din[l]; net.dout[l] = h.dout[l]; net.act[l] = h.act[l]; net.actp[l] = h.actp[l];
        net.W[l] = h.d_W[l].get(); net.Wt[l] = h.d_Wt[l].get(); net.b[l] = h.d_b[l].get();
        net.soff[l] = net.souts; net.souts += h.dout[l];
    }
    const long long rows = (long long)B * h.cfg.H;
    const int rc = h.cfg.dtype == NEMPC_F64 ? run<double>(h, p, net, rows, Z, X0, lam, v, w, gE, s)
                                            : run<float>(h, p, net, rows, Z, X0, lam, v, w, gE, s);
    if (rc == NEMPC_OK) h.last_egrad_kernel = p.code;
    return rc;
}

}  // namespace nempc
