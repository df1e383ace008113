// Index arithmetic of the input-rate formulation (nempc_bind_rate; solver_rate_impl.h, Solve<T> in solver.hip).  Like
// solver_soc_impl.h it includes nothing of the library and nothing of HIP, so that a host program checks every entry against
// a brute-force restatement (tests/rate_index_check.cpp).
//
// The caller's problem has the variables z = [x_1 .. x_H (H nx) | u_0 .. u_{H-1} (H nu)] (x_t: the state step t arrives at).
// The solver's problem is stage-wise in
//     s_t = [x_{t+1} ; u_t]  (ns = nx + nu),   v_t = u_t - u_{t-1}  (nu),   s_{-1} = [x0 ; u_prev]  (data),      t = 0 .. H-1
//     za  = [s_0 .. s_{H-1} (H ns) | v_0 .. v_{H-1} (H nu)]
// with the stage map F(s, v) = [Phi(x, u + v) ; u + v]: rows i < nx of a stage are the network's, rows i >= nx the linear
// rows  u_{t-1} + v_t - u_t.  A column of (s_{t-1}, v_t) is a column of the handle's tile / block [x_{t-1} | u_t]: the
// u_{t-1} column and the v_t column BOTH map to the handle's u column.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NEMPC_RATE_HD __host__ __device__
#else
#define NEMPC_RATE_HD
#endif

namespace nempc {

struct RateDims {
    int H, nx, nu;      // the caller's horizon, states, controls
    int ns;             // the solver's stage state: nx + nu
    int nin;            // columns of an augmented tile / block: ns + nu
    int n_s;            // augmented variables: H (ns + nu)
    int m_s;            // augmented defect rows: H ns
    int n_r;            // the caller's variables: H (nx + nu)
};

NEMPC_RATE_HD inline RateDims rate_dims(int H, int nx, int nu) {
    RateDims d;
    d.H = H; d.nx = nx; d.nu = nu; d.ns = nx + nu; d.nin = nx + 2 * nu;
    d.n_s = H * (nx + 2 * nu); d.m_s = H * (nx + nu); d.n_r = H * (nx + nu);
    return d;
}

// where the caller's x_{t+1}[i] / u_t[j] sit in the augmented vector, and v_t[j]
NEMPC_RATE_HD inline int rate_slot_x(const RateDims& d, int t, int i) { return t * d.ns + i; }
NEMPC_RATE_HD inline int rate_slot_u(const RateDims& d, int t, int j) { return t * d.ns + d.nx + j; }
NEMPC_RATE_HD inline int rate_slot_v(const RateDims& d, int t, int j) { return d.H * d.ns + t * d.nu + j; }

// augmented variable k -> the caller's variable it is a copy of (>= 0: the s slots), or -(1 + t nu + j) for v_t[j] (no
// caller variable: the difference of two)
NEMPC_RATE_HD inline int rate_source(const RateDims& d, int k) {
    if (k >= d.H * d.ns) return -(1 + (k - d.H * d.ns));
    const int t = k / d.ns, i = k % d.ns;
    return i < d.nx ? t * d.nx + i : d.H * d.nx + t * d.nu + (i - d.nx);
}

// entry c of the start state s_{-1} -> entry of the problem's data [x0 (nx) | u_prev (nu)]: the identity, spelled out
// because the two halves come from different arrays
NEMPC_RATE_HD inline bool rate_start_is_x0(const RateDims& d, int c) { return c < d.nx; }
NEMPC_RATE_HD inline int rate_start_entry(const RateDims& d, int c) { return c < d.nx ? c : c - d.nx; }

// column c of (s_{t-1}, v_t) -> column of the handle's tile / block [x_{t-1} (nx) | u_t (nu)]
NEMPC_RATE_HD inline int rate_handle_col(const RateDims& d, int c) { return c < d.ns ? c : c - d.nu; }

// linear row i >= nx of a stage, column c of (s_{t-1}, v_t): the constant tile entry (1 on the u_{t-1} and v_t columns of
// the row's control, 0 elsewhere)
NEMPC_RATE_HD inline int rate_linear_entry(const RateDims& d, int i, int c) {
    const int j = i - d.nx;
    return (c == d.nx + j || c == d.ns + j) ? 1 : 0;
}

// where the bounds land in the solver's bound vector (n_s): the caller's bound on variable v of z ...
NEMPC_RATE_HD inline int rate_bound_slot(const RateDims& d, int v) {
    if (v < d.H * d.nx) return rate_slot_x(d, v / d.nx, v % d.nx);
    const int r = v - d.H * d.nx;
    return rate_slot_u(d, r / d.nu, r % d.nu);
}
// ... and the limit on Delta u_t[j]; its entry in the caller's dlo / dhi array ((nu), or (H,nu) when per_stage)
NEMPC_RATE_HD inline int rate_limit_slot(const RateDims& d, int t, int j) { return rate_slot_v(d, t, j); }
NEMPC_RATE_HD inline int rate_limit_entry(const RateDims& d, int t, int j, int per_stage) { return per_stage ? t * d.nu + j : j; }

}  // namespace nempc
