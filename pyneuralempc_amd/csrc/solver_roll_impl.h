// Batched solver, rolling-window models as a stage-wise problem in the window state: the index tables and the kernels
// that move between the caller's variables and the augmented ones.  Included by solver.hip only.
#pragma once

namespace nempc {

namespace {

// ---- rolling-window models (model/tensorflow.py:132-340: the network of step t reads the last w states and controls).
// The Riccati sweeps need a STAGE-wise problem: the window is made the state,
//     s_tau = [x_tau, x_{tau-1}, .., x_{tau-w+1} | u_{tau-1}, .., u_{tau-w+1}]            (ns = w nx + (w-1) nu entries)
//     s_{t+1} = [Phi(window of step t) ; shifted copies of s_t and u_t]
// (x_tau indexes [x0 ; states], slots before the horizon are x0 and the bound history and make up s_0), and the solver
// runs UNCHANGED on that plain problem with stage dimensions (ns, nu).  The callbacks stay the handle's own window kernels
// on the caller's variables: before an evaluation the primary copies [x_tau | u_t] are gathered out of the augmented
// iterate; after it the defects, tiles, Lagrangian blocks and the objective gradient are spread into augmented form --
// a tile / block column of the window IS a column of (s_t, u_t), and the shift rows are constant 0/1 rows.  The shift
// rows are linear and hold at the start (the copies are built from the primaries), so every Newton step keeps them and
// the network is always evaluated at the point the augmented iterate stands on.
struct RollTables {        // device, int32; built once per workspace (they depend on the handle's shape only)
    int* src = nullptr;    // (n_s)  augmented variable -> caller's variable v >= 0, or -(1 + k): entry k of the problem's data
                           //        [x0 (nx) | hist_x (w-1, nx) | hist_u (w-1, nu)]
    int* src0 = nullptr;   // (ns)   the same for s_0 (data only)
    int* prim = nullptr;   // (n_r)  caller's variable -> its primary copy in the augmented vector
    int* isprim = nullptr; // (n_s)  1 where the augmented variable is a primary copy
    int* dcol = nullptr;   // (ns + nu) column of (s_t, u_t) -> window column of the handle's tiles / blocks
    int* shift = nullptr;  // (ns)   row i >= nx of a stage: column of (s_t, u_t) it copies
};

template <typename T>
__device__ __forceinline__ T roll_data(int k, int b, int nx, int nu, int back, const T* __restrict__ X0,
                                       const T* __restrict__ hx, const T* __restrict__ hu) {
    if (k < nx) return X0[(size_t)b * nx + k];
    k -= nx;
    if (k < back * nx) return hx[(size_t)b * back * nx + k];
    return hu[(size_t)b * back * nu + (k - back * nx)];
}

// augmented start: primaries = the caller's guess moved inside its bounds (what solver_init_kernel would do to them:
// it then leaves them alone), copies = those same values, s_0 from the data
template <typename T>
__global__ __launch_bounds__(256) void roll_build_kernel(int B, int n_s, int ns, int n_r, int nx, int nu, int back,
                                                         RollTables rt, const T* __restrict__ Zin, const T* __restrict__ X0,
                                                         const T* __restrict__ hx, const T* __restrict__ hu,
                                                         const T* __restrict__ lb, const T* __restrict__ ub, T mu0,
                                                         int has_bounds, T* __restrict__ Zaug, T* __restrict__ S0) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)B * ns) {
        const int b = (int)(i / ns), k = (int)(i % ns);
        S0[i] = roll_data(-1 - rt.src0[k], b, nx, nu, back, X0, hx, hu);
    }
    if (i >= (size_t)B * n_s) return;
    const int b = (int)(i / n_s), k = (int)(i % n_s);
    const int v = rt.src[k];
    if (v < 0) { Zaug[i] = roll_data(-1 - v, b, nx, nu, back, X0, hx, hu); return; }
    const int pk = rt.prim[v];
    Zaug[i] = start_inside(Zin[(size_t)b * n_r + v], lb[pk], ub[pk], mu0, has_bounds);
}

// caller's variables (and multipliers of the network rows) out of the augmented ones
template <typename T>
__global__ __launch_bounds__(256) void roll_in_kernel(int B, int n_s, int n_r, int H, int nx, int ns, int m_r, RollTables rt,
                                                      const T* __restrict__ Zaug, T* __restrict__ Zr,
                                                      const T* __restrict__ lam_aug, T* __restrict__ lam_r) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)B * n_r) {
        const int b = (int)(i / n_r), v = (int)(i % n_r);
        Zr[i] = Zaug[(size_t)b * n_s + rt.prim[v]];
    }
    if (lam_r && i < (size_t)B * H * nx) {
        const int b = (int)(i / (H * nx)), r = (int)(i % (H * nx));
        lam_r[(size_t)b * m_r + r] = lam_aug[(size_t)b * H * ns + (r / nx) * ns + (r % nx)];
    }
}

// the window evaluation spread into augmented form; one workgroup per (problem, step).  Any of tiles / hblk / grad may be
// null (a trial point needs the defects only)
template <typename T>
__global__ __launch_bounds__(256) void roll_out_kernel(int H, int nx, int nu, int ns, int nin_w, int n_r, int m_r, RollTables rt,
                                                       const T* __restrict__ Zaug, const T* __restrict__ S0,
                                                       const T* __restrict__ g_r, const T* __restrict__ tiles_r,
                                                       const T* __restrict__ hblk_r, const T* __restrict__ grad_r,
                                                       T* __restrict__ g_aug, T* __restrict__ tiles_aug,
                                                       T* __restrict__ hblk_aug, T* __restrict__ grad_aug) {
    const int b = blockIdx.x / H, t = blockIdx.x % H, nin_s = ns + nu, n_s = H * nin_s;
    const T* za = Zaug + (size_t)b * n_s;
    // value of column c of (s_t, u_t)
    auto col_value = [&](int c) -> T {
        if (c >= ns) return za[H * ns + t * nu + (c - ns)];
        return t == 0 ? S0[(size_t)b * ns + c] : za[(t - 1) * ns + c];
    };
    for (int i = threadIdx.x; i < ns; i += 256)
        g_aug[(size_t)b * H * ns + t * ns + i] =
            i < nx ? g_r[(size_t)b * m_r + t * nx + i] : col_value(rt.shift[i]) - za[t * ns + i];
    if (tiles_aug) {
        T* ta = tiles_aug + ((size_t)b * H + t) * ns * nin_s;
        const T* tr = tiles_r + ((size_t)b * H + t) * nx * nin_w;
        for (int e = threadIdx.x; e < ns * nin_s; e += 256) {
            const int i = e / nin_s, c = e % nin_s;
            T v;
            if (i < nx) { const int d = rt.dcol[c]; v = d >= 0 ? tr[i * nin_w + d] : T(0); }
            else v = rt.shift[i] == c ? T(1) : T(0);
            ta[e] = v;
        }
    }
    if (hblk_aug) {
        T* ha = hblk_aug + ((size_t)b * H + t) * nin_s * nin_s;
        const T* hr = hblk_r + ((size_t)b * H + t) * nin_w * nin_w;
        for (int e = threadIdx.x; e < nin_s * nin_s; e += 256) {
            const int dp = rt.dcol[e / nin_s], dq = rt.dcol[e % nin_s];
            ha[e] = (dp >= 0 && dq >= 0) ? hr[dp * nin_w + dq] : T(0);
        }
    }
    if (grad_aug) {
        // this step's share of the gradient: the state block s_{t+1} and the control block u_t
        for (int i = threadIdx.x; i < nin_s; i += 256) {
            const int k = i < ns ? t * ns + i : H * ns + t * nu + (i - ns);
            grad_aug[(size_t)b * n_s + k] = rt.isprim[k] ? grad_r[(size_t)b * n_r + rt.src[k]] : T(0);
        }
    }
}

}  // namespace

}  // namespace nempc
