// Batched solver, input-rate penalty and rate limits (nempc_bind_rate) as a stage-wise problem in the state [x ; u] with the
// control move as the stage control: the kernels that move between the caller's variables and the augmented ones.  Included
// by solver.hip only; the index arithmetic is rate_index.h (host / device, checked by tests/rate_index_check.cpp).
#pragma once

#include "rate_index.h"

namespace nempc {

namespace {

// ---- the rate formulation:  min f(z) + sum_t dv_t' S dv_t,  dlo <= dv_t = u_t - u_{t-1} <= dhi,  u_{-1} = u_prev (data).
//     s_t = [x_{t+1} ; u_t],  v_t = dv_t,  s_{-1} = [x0 ; u_prev],   F(s, v) = [Phi(x, u + v) ; u + v]
// and the solver runs UNCHANGED on that plain problem with stage dimensions (nx + nu, nu), the construction of the rolling-
// window path (solver_roll_impl.h) with another augmentation.  The callbacks stay the handle's own kernels on the caller's
// variables: before an evaluation x_t and u_t := u_{t-1} + v_t are gathered out of the augmented iterate -- NOT the primary
// copy u_t: the network rows are then exact for F at the point the iterate stands on whatever the residual of the linear
// rows, which the start need not make zero (u and v are moved inside their bounds independently).  After it the defects,
// tiles and Lagrangian blocks are spread into augmented form: the u_{t-1} column and the v_t column of a stage both are the
// handle's u column, the linear rows are the constant rows [0 | I | I].  The objective is the host-built table over the
// augmented stage (Q_aug = blkdiag(Q, R) on s, R_aug = S on v): value and gradient are evaluated from it on the augmented
// iterate, with the arithmetic of objective_row_value, the very function the acceptance test scores a trial point with.
// Schedule: the window path's -- one trial per iteration, no compaction (the callbacks read x0 by problem index).

// augmented start: s slots = the caller's guess moved inside its bounds (what solver_init_kernel would do to them: it then
// leaves them alone), v_t = the difference of those controls moved inside the limits, s_{-1} = [x0 ; u_prev]
template <typename T>
__global__ __launch_bounds__(256) void rate_build_kernel(int B, RateDims d, const T* __restrict__ Zin, const T* __restrict__ X0,
                                                         const T* __restrict__ u_prev, const T* __restrict__ lb,
                                                         const T* __restrict__ ub, T mu0, int has_bounds,
                                                         T* __restrict__ Zaug, T* __restrict__ S0) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)B * d.ns) {
        const int b = (int)(i / d.ns), c = (int)(i % d.ns);
        S0[i] = rate_start_is_x0(d, c) ? X0[(size_t)b * d.nx + rate_start_entry(d, c)]
                                       : u_prev[(size_t)b * d.nu + rate_start_entry(d, c)];
    }
    if (i >= (size_t)B * d.n_s) return;
    const int b = (int)(i / d.n_s), k = (int)(i % d.n_s);
    const T* zin = Zin + (size_t)b * d.n_r;
    const int v = rate_source(d, k);
    if (v >= 0) { Zaug[i] = start_inside(zin[v], lb[k], ub[k], mu0, has_bounds); return; }
    const int t = (-1 - v) / d.nu, j = (-1 - v) % d.nu;
    auto u_inside = [&](int tt) -> T {
        const int ku = rate_slot_u(d, tt, j);
        return start_inside(zin[d.H * d.nx + tt * d.nu + j], lb[ku], ub[ku], mu0, has_bounds);
    };
    const T before = t == 0 ? u_prev[(size_t)b * d.nu + j] : u_inside(t - 1);
    Zaug[i] = start_inside(u_inside(t) - before, lb[k], ub[k], mu0, has_bounds);
}

// the caller's variables out of the augmented ones: x_t, and u_t := u_{t-1} + v_t (the point the network is evaluated at) or,
// for the returned solution (primary != 0), the u slots of s; with lam_r the multipliers of the network rows out of the
// augmented costates, for the Hessian callback
template <typename T>
__global__ __launch_bounds__(256) void rate_gather_kernel(int B, RateDims d, int m_r, int primary, const T* __restrict__ Zaug,
                                                          const T* __restrict__ S0, T* __restrict__ Zr,
                                                          const T* __restrict__ lam_aug, T* __restrict__ lam_r) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)B * d.n_r) {
        const int b = (int)(i / d.n_r), v = (int)(i % d.n_r);
        const T* za = Zaug + (size_t)b * d.n_s;
        T val;
        if (v < d.H * d.nx || primary) val = za[rate_bound_slot(d, v)];
        else {
            const int t = (v - d.H * d.nx) / d.nu, j = (v - d.H * d.nx) % d.nu;
            const T before = t == 0 ? S0[(size_t)b * d.ns + d.nx + j] : za[rate_slot_u(d, t - 1, j)];
            val = before + za[rate_slot_v(d, t, j)];
        }
        Zr[i] = val;
    }
    if (lam_r && i < (size_t)B * d.H * d.nx) {
        const int b = (int)(i / (d.H * d.nx)), r = (int)(i % (d.H * d.nx));
        lam_r[(size_t)b * m_r + r] = lam_aug[(size_t)b * d.m_s + (r / d.nx) * d.ns + (r % d.nx)];
    }
}

// step t's share of the gradient of an objective table over an augmented stage (P, ao: obj_offsets(H, ns, nu)), by the 256
// threads of a workgroup: the state block s_t (weights Q_aug, or QT_aug at the last step) and the stage-control block behind
// the H states; sums in objective_row_value's order.  za: the problem's augmented variables [s_0 .. s_{H-1} | controls]
template <typename T>
__device__ __forceinline__ void aug_stage_gradient(int b, int t, int H, int ns, int nu, const T* __restrict__ P, const ObjOffsets& ao,
                                                   const T* __restrict__ za, T* __restrict__ grad_aug) {
    const int nin_s = ns + nu;
    const size_t n_s = (size_t)H * nin_s;
    const T* Qs = P + (t == H - 1 ? ao.QTs : ao.Qs);
    const T* st = za + t * ns;
    const T* vt = za + H * ns + t * nu;
    for (int i = threadIdx.x; i < nin_s; i += 256) {
        T acc = T(0);
        if (i < ns) {
            for (int j = 0; j < ns; ++j) acc = fma(Qs[i * ns + j], st[j] - P[ao.xref + t * ns + j], acc);
            grad_aug[(size_t)b * n_s + t * ns + i] = acc + P[ao.cx + t * ns + i];
        } else {
            const int iu = i - ns;
            for (int j = 0; j < nu; ++j) acc = fma(P[ao.Rs + iu * nu + j], vt[j] - P[ao.uref + t * nu + j], acc);
            grad_aug[(size_t)b * n_s + H * ns + t * nu + iu] = acc + P[ao.cu + t * nu + iu];
        }
    }
}

// the evaluation spread into augmented form; one workgroup per (problem, step), its entries spread over the 256 threads.
// tiles / hblk / grad / f null: a trial point needs the defects only.  P, ao: the objective table over the augmented stage
template <typename T>
__global__ __launch_bounds__(256) void rate_spread_kernel(RateDims d, int m_r, const T* __restrict__ Zaug, const T* __restrict__ S0,
                                                          const T* __restrict__ g_r, const T* __restrict__ tiles_r,
                                                          const T* __restrict__ hblk_r, const T* __restrict__ P, ObjOffsets ao,
                                                          T* __restrict__ g_aug, T* __restrict__ tiles_aug,
                                                          T* __restrict__ hblk_aug, T* __restrict__ grad_aug, T* __restrict__ f) {
    const int H = d.H, nx = d.nx, nu = d.nu, ns = d.ns, nin_s = d.nin, nin_r = nx + nu;
    const int b = blockIdx.x / H, t = blockIdx.x % H;
    const T* za = Zaug + (size_t)b * d.n_s;
    for (int i = threadIdx.x; i < ns; i += 256) {
        T v;
        if (i < nx) v = g_r[(size_t)b * m_r + t * nx + i];
        else {      // u_{t-1} + v_t - u_t
            const int j = i - nx;
            const T before = t == 0 ? S0[(size_t)b * ns + i] : za[rate_slot_u(d, t - 1, j)];
            v = before + za[rate_slot_v(d, t, j)] - za[rate_slot_u(d, t, j)];
        }
        g_aug[(size_t)b * d.m_s + t * ns + i] = v;
    }
    if (tiles_aug) {
        T* ta = tiles_aug + ((size_t)b * H + t) * ns * nin_s;
        const T* tr = tiles_r + ((size_t)b * H + t) * nx * nin_r;
        for (int e = threadIdx.x; e < ns * nin_s; e += 256) {
            const int i = e / nin_s, c = e % nin_s;
            ta[e] = i < nx ? tr[i * nin_r + rate_handle_col(d, c)] : (T)rate_linear_entry(d, i, c);
        }
    }
    if (hblk_aug) {
        T* ha = hblk_aug + ((size_t)b * H + t) * nin_s * nin_s;
        const T* hr = hblk_r + ((size_t)b * H + t) * nin_r * nin_r;
        for (int e = threadIdx.x; e < nin_s * nin_s; e += 256)
            ha[e] = hr[rate_handle_col(d, e / nin_s) * nin_r + rate_handle_col(d, e % nin_s)];
    }
    if (grad_aug) aug_stage_gradient<T>(b, t, H, ns, nu, P, ao, za, grad_aug);
    // the objective value: the first wave of the problem's first workgroup, lanes over the horizon
    if (f && t == 0 && threadIdx.x < 64) {
        const double acc = objective_row_value<T>(b, (int)threadIdx.x, H, ns, nu, ao, P, za, (T*)nullptr);
        if (threadIdx.x == 0) f[b] = (T)acc;
    }
}

}  // namespace

}  // namespace nempc
