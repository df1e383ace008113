// Batched solver, linear stage inequality rows (nempc_bind_stage_rows) as a stage-wise problem in the state [x ; y] with y the
// value of the rows: the kernels that move between the caller's variables and the augmented ones.  Included by solver.hip
// only, after solver_rate_impl.h; the index arithmetic is rows_index.h (host / device, checked by tests/rows_index_check.cpp).
#pragma once

#include "rows_index.h"

namespace nempc {

namespace {

// ---- the rows formulation:  min f(z),  rlo_t <= Cx x_t + Cu u_t <= rhi_t  (x_t, u_t: row t of the state / control block of z).
//     s_t = [x_t ; y_t],  stage control u_t,  s_{-1} = [x0 ; 0],   F(s, u) = [Phi(x, u) ; Cx Phi(x, u) + Cu u]
// and the solver runs UNCHANGED on that plain problem with stage dimensions (nx + nc, nu), the construction of the rate path
// (solver_rate_impl.h) with another augmentation.  y_t feeds nothing and costs nothing: its variable bounds [rlo_t, rhi_t]
// are the rows.  The callbacks stay the handle's own kernels on the caller's variables, which are the x and u slots of the
// augmented iterate as they stand.  After an evaluation the defects, tiles and Lagrangian blocks are spread into augmented
// form: the y rows of a stage are Cx times the network's rows plus the constant Cu, evaluated without a second pass through
// the network (Phi = g_r + x_t); the y columns are zero.  The y rows are linear in Phi, so their second-order term is the
// network's, contracted with Cx' lam_y: the gather adds it to the multipliers the Hessian callback reads.  The objective is
// the host-built table over the augmented stage (zero on y), evaluated as on the rate path.
// C is (nc, nx + nu) row-major in the handle's dtype; every product with it is an fma chain in a fixed order (a solve is
// bitwise reproducible).  Schedule: the other augmentations' -- one trial per iteration, no compaction, no carry.

// augmented start: x and u slots = the caller's guess moved inside its bounds (what solver_init_kernel would do to them: it
// then leaves them alone), y_t = the rows at those values moved inside the limits, s_{-1} = [x0 ; 0]
template <typename T>
__global__ __launch_bounds__(256) void rows_build_kernel(int B, RowsDims d, const T* __restrict__ Zin, const T* __restrict__ X0,
                                                         const T* __restrict__ C, const T* __restrict__ lb,
                                                         const T* __restrict__ ub, T mu0, int has_bounds,
                                                         T* __restrict__ Zaug, T* __restrict__ S0) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)B * d.ns) {
        const int b = (int)(i / d.ns), c = (int)(i % d.ns);
        S0[i] = c < d.nx ? X0[(size_t)b * d.nx + c] : T(0);
    }
    if (i >= (size_t)B * d.n_s) return;
    const int b = (int)(i / d.n_s), k = (int)(i % d.n_s);
    const T* zin = Zin + (size_t)b * d.n_r;
    const int v = rows_source(d, k);
    if (v >= 0) { Zaug[i] = start_inside(zin[v], lb[k], ub[k], mu0, has_bounds); return; }
    const int t = (-1 - v) / d.nc, r = (-1 - v) % d.nc;
    const T* Ck = C + (size_t)r * (d.nx + d.nu);
    T acc = T(0);
    for (int c = 0; c < d.nx; ++c) {
        const int kx = rows_slot_x(d, t, c);
        acc = fma(Ck[c], start_inside(zin[t * d.nx + c], lb[kx], ub[kx], mu0, has_bounds), acc);
    }
    for (int j = 0; j < d.nu; ++j) {
        const int ku = rows_slot_u(d, t, j);
        acc = fma(Ck[d.nx + j], start_inside(zin[d.H * d.nx + t * d.nu + j], lb[ku], ub[ku], mu0, has_bounds), acc);
    }
    Zaug[i] = start_inside(acc, lb[k], ub[k], mu0, has_bounds);
}

// the caller's variables out of the augmented ones (the x and u slots); with lam_r the multipliers the Hessian callback
// contracts the network's second derivatives with, lam_x,t + Cx' lam_y,t
template <typename T>
__global__ __launch_bounds__(256) void rows_gather_kernel(int B, RowsDims d, int m_r, const T* __restrict__ C,
                                                          const T* __restrict__ Zaug, T* __restrict__ Zr,
                                                          const T* __restrict__ lam_aug, T* __restrict__ lam_r) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)B * d.n_r) {
        const int b = (int)(i / d.n_r), v = (int)(i % d.n_r);
        Zr[i] = Zaug[(size_t)b * d.n_s + rows_bound_slot(d, v)];
    }
    if (lam_r && i < (size_t)B * d.H * d.nx) {
        const int b = (int)(i / (d.H * d.nx)), r = (int)(i % (d.H * d.nx)), t = r / d.nx, c = r % d.nx;
        const T* la = lam_aug + (size_t)b * d.m_s + t * d.ns;
        T acc = la[c];
        for (int k = 0; k < d.nc; ++k) acc = fma(C[(size_t)k * (d.nx + d.nu) + c], la[d.nx + k], acc);
        lam_r[(size_t)b * m_r + r] = acc;
    }
}

// the evaluation spread into augmented form; one workgroup per (problem, step), its entries spread over the 256 threads.
// tiles / hblk / grad / f null: a trial point needs the defects only.  P, ao: the objective table over the augmented stage
template <typename T>
__global__ __launch_bounds__(256) void rows_spread_kernel(RowsDims d, int m_r, const T* __restrict__ C, const T* __restrict__ Zaug,
                                                          const T* __restrict__ g_r, const T* __restrict__ tiles_r,
                                                          const T* __restrict__ hblk_r, const T* __restrict__ P, ObjOffsets ao,
                                                          T* __restrict__ g_aug, T* __restrict__ tiles_aug,
                                                          T* __restrict__ hblk_aug, T* __restrict__ grad_aug, T* __restrict__ f) {
    const int H = d.H, nx = d.nx, nu = d.nu, ns = d.ns, nin_s = d.nin, nin_r = nx + nu;
    const int b = blockIdx.x / H, t = blockIdx.x % H;
    const T* za = Zaug + (size_t)b * d.n_s;
    const T* gr = g_r + (size_t)b * m_r + t * nx;
    for (int i = threadIdx.x; i < ns; i += 256) {
        T v;
        if (i < nx) v = gr[i];
        else {      // Cx Phi + Cu u_t - y_t,  Phi = g_r + x_t
            const T* Ck = C + (size_t)(i - nx) * nin_r;
            const T* xt = za + rows_slot_x(d, t, 0);
            T acc = T(0);
            for (int c = 0; c < nx; ++c) acc = fma(Ck[c], gr[c] + xt[c], acc);
            for (int j = 0; j < nu; ++j) acc = fma(Ck[nx + j], za[rows_slot_u(d, t, j)], acc);
            v = acc - za[rows_slot_y(d, t, i - nx)];
        }
        g_aug[(size_t)b * d.m_s + t * ns + i] = v;
    }
    if (tiles_aug) {
        T* ta = tiles_aug + ((size_t)b * H + t) * ns * nin_s;
        const T* tr = tiles_r + ((size_t)b * H + t) * nx * nin_r;
        for (int e = threadIdx.x; e < ns * nin_s; e += 256) {
            const int i = e / nin_s, hc = rows_handle_col(d, e % nin_s);
            T v = T(0);
            if (hc >= 0 && i < nx) v = tr[i * nin_r + hc];
            else if (hc >= 0) {      // [Cx T_x | Cx T_u + Cu]
                const T* Ck = C + (size_t)(i - nx) * nin_r;
                for (int c = 0; c < nx; ++c) v = fma(Ck[c], tr[c * nin_r + hc], v);
                if (hc >= nx) v += Ck[hc];
            }
            ta[e] = v;
        }
    }
    if (hblk_aug) {
        T* ha = hblk_aug + ((size_t)b * H + t) * nin_s * nin_s;
        const T* hr = hblk_r + ((size_t)b * H + t) * nin_r * nin_r;
        for (int e = threadIdx.x; e < nin_s * nin_s; e += 256) {
            const int r = rows_handle_col(d, e / nin_s), c = rows_handle_col(d, e % nin_s);
            ha[e] = (r >= 0 && c >= 0) ? hr[r * nin_r + c] : T(0);
        }
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
