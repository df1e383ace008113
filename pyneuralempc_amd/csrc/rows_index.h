// Index arithmetic of the linear stage rows (nempc_bind_stage_rows; solver_rows_impl.h, StageAug<T> in solver_aug.h).  Like
// rate_index.h it includes nothing of the library and nothing of HIP, so that a host program checks every entry against a
// brute-force restatement (tests/rows_index_check.cpp).
//
// The caller's problem has the variables z = [x_1 .. x_H (H nx) | u_0 .. u_{H-1} (H nu)]; below x_t is ROW t of the state
// block (the state step t arrives at) and u_t row t of the control block, t = 0 .. H-1.  The rows are
//     rlo_t <= Cx x_t + Cu u_t <= rhi_t,      C = [Cx (nc,nx) | Cu (nc,nu)]
// and the solver's problem is stage-wise in
//     s_t = [x_t ; y_t]  (ns = nx + nc),   the stage control is the caller's u_t,   s_{-1} = [x0 ; 0]  (data)
//     za  = [s_0 .. s_{H-1} (H ns) | u_0 .. u_{H-1} (H nu)]
// with the stage map F(s, u) = [Phi(x, u) ; Cx Phi(x, u) + Cu u]: rows i < nx of a stage are the network's, rows i >= nx the
// row values, whose variable bounds are the limits.  A column of (s_{t-1}, u_t) is a column of the handle's tile / block
// [x_{t-1} | u_t], or none: y feeds nothing.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NEMPC_ROWS_HD __host__ __device__
#else
#define NEMPC_ROWS_HD
#endif

namespace nempc {

struct RowsDims {
    int H, nx, nu, nc;  // the caller's horizon, states, controls; rows per stage
    int ns;             // the solver's stage state: nx + nc
    int nin;            // columns of an augmented tile / block: ns + nu
    int n_s;            // augmented variables: H (ns + nu)
    int m_s;            // augmented defect rows: H ns
    int n_r;            // the caller's variables: H (nx + nu)
};

NEMPC_ROWS_HD inline RowsDims rows_dims(int H, int nx, int nu, int nc) {
    RowsDims d;
    d.H = H; d.nx = nx; d.nu = nu; d.nc = nc; d.ns = nx + nc; d.nin = nx + nc + nu;
    d.n_s = H * (nx + nc + nu); d.m_s = H * (nx + nc); d.n_r = H * (nx + nu);
    return d;
}

// where the caller's x_t[i] / u_t[j] sit in the augmented vector, and the row value y_t[k]
NEMPC_ROWS_HD inline int rows_slot_x(const RowsDims& d, int t, int i) { return t * d.ns + i; }
NEMPC_ROWS_HD inline int rows_slot_y(const RowsDims& d, int t, int k) { return t * d.ns + d.nx + k; }
NEMPC_ROWS_HD inline int rows_slot_u(const RowsDims& d, int t, int j) { return d.H * d.ns + t * d.nu + j; }

// augmented variable k -> the caller's variable it is (>= 0), or -(1 + t nc + k) for y_t[k] (no caller variable)
NEMPC_ROWS_HD inline int rows_source(const RowsDims& d, int k) {
    if (k >= d.H * d.ns) return d.H * d.nx + (k - d.H * d.ns);
    const int t = k / d.ns, i = k % d.ns;
    return i < d.nx ? t * d.nx + i : -(1 + t * d.nc + (i - d.nx));
}

// column c of (s_{t-1}, u_t) -> column of the handle's tile / block [x_{t-1} (nx) | u_t (nu)], -1 for a y column
NEMPC_ROWS_HD inline int rows_handle_col(const RowsDims& d, int c) { return c < d.nx ? c : (c < d.ns ? -1 : c - d.nc); }

// where the bounds land in the solver's bound vector (n_s): the caller's bound on variable v of z ...
NEMPC_ROWS_HD inline int rows_bound_slot(const RowsDims& d, int v) {
    if (v < d.H * d.nx) return rows_slot_x(d, v / d.nx, v % d.nx);
    const int r = v - d.H * d.nx;
    return rows_slot_u(d, r / d.nu, r % d.nu);
}
// ... and the limit of row (t, k); its entry in the caller's rlo / rhi array ((nc), or (H,nc) when per_stage)
NEMPC_ROWS_HD inline int rows_limit_slot(const RowsDims& d, int t, int k) { return rows_slot_y(d, t, k); }
NEMPC_ROWS_HD inline int rows_limit_entry(const RowsDims& d, int t, int k, int per_stage) { return per_stage ? t * d.nc + k : k; }

}  // namespace nempc
