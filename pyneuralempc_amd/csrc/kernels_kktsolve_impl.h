// Arithmetic of KKT solves with caller-supplied right-hand sides (nempc_kkt_solve, kernels_kktsolve.hip): the affine part
// of the Riccati recursion whose matrix part is kernels_sens_impl.h.  Like that header it includes nothing of the library
// and nothing of HIP, so that a host program runs the very same recursion with one lane (tests/kkt_solve_check.cpp).
//
// At a primal-dual point the KKT matrix K = [[W + Sigma, J'], [J, 0]] is symmetric; K [v ; w] = [rz ; rg] reads, per stage t
// (notation of kernels_sens_impl.h; rz = (r^x_0..r^x_{H-1} | r^u_0..r^u_{H-1}) in z order, rg = (r^g_0..r^g_{H-1})):
//     (Rs + Sigma_u[t] + W_uu,t) v_u[t] + W_ux,t v_x[t-1] + B_t' w_t                              = r^u_t
//     (Qs|QTs + Sigma_x[t] + W_xx,t+1) v_x[t] + W_xu,t+1 v_u[t+1] - w_t + A_{t+1}' w_{t+1}         = r^x_t
//     A_t v_x[t-1] + B_t v_u[t] - v_x[t] = r^g_t,     v_x[-1] = 0
// With w_t = P_t v_x[t] - p_t the matrices P_t, K_t, Quu_t = L D L', Qux_t are those of sens_backward_stage, and per
// right-hand side (p_{H-1} = r^x_{H-1}):
//     backward  q_t = P_t r^g_t + p_t,   k_t = Quu_t^-1 (r^u_t + B_t' q_t),   p_{t-1} = r^x_{t-1} + A_t' q_t - Qux_t' k_t
//     forward   v_u[t] = K_t v_x[t-1] + k_t,   v_x[t] = A_t v_x[t-1] + B_t v_u[t] - r^g_t,   w_t = P_t v_x[t] - p_t
//     pull-back gx0 = -(W_ux,0' v_u[0] + A_0' w_0)
// gx0 is [v ; w]' (-d/dx0 [grad L ; g]): with rz the cotangent of z* it is the cotangent of x0, and with rz = e_i, rg = 0
// row i of nempc_sensitivity's dz/dx0.
// Everything is double; T appears at loads of the stage data and the right-hand sides and at stores of the results only.
// The arithmetic of one right-hand side does not depend on how many there are, nor on where the working sets live.
#pragma once

#include "kernels_sens_impl.h"

namespace nempc {

// The right-hand-side dependent working set of one problem (element offsets into `aff`, doubles): p_t and k_t of every
// stage and right-hand side, and the vectors one stage works on.
struct KktSolveLayout {
    int p, k, q, xa, xb, u, total;
};
NEMPC_SENS_HD inline KktSolveLayout kktsolve_layout(int H, int nx, int nu, int nrhs) {
    KktSolveLayout L;
    int o = 0;
    L.p = o; o += nrhs * H * nx;    // p_t       (nrhs, H, nx)
    L.k = o; o += nrhs * H * nu;    // k_t       (nrhs, H, nu)
    L.q = o; o += nrhs * nx;        // q_t backward, w_0 forward
    L.xa = o; o += nrhs * nx;       // v_x ping
    L.xb = o; o += nrhs * nx;       // v_x pong
    L.u = o; o += nrhs * nu;        // v_u[t]
    L.total = (o + 1) & ~1;
    return L;
}

// The affine part of one backward stage, right after sens_backward_stage(t) returned true: ws still holds the factor of
// Quu_t and Qux_t.  Pt = P_t (nx, nx) is read only when rg is given.  rz (nrhs, n), rg (nrhs, H nx) or null.
template <typename T, typename Sync>
NEMPC_SENS_HD inline void kktsolve_backward_stage(int lane, int nlanes, Sync sync, int t, int H, int nx, int nu, int nrhs,
                                                  const T* At, const double* Pt, const T* rz, const T* rg, const double* ws,
                                                  double* aff) {
    const SensLayout L = sens_layout(nx, nu);
    const KktSolveLayout A = kktsolve_layout(H, nx, nu, nrhs);
    const int nin = nx + nu, n = H * nin, hx = H * nx;
    const double *Quu = ws + L.Quu, *Qux = ws + L.Qux;
    double *p = aff + A.p, *kk = aff + A.k;
    // q = P r^g + p; without r^g it is p_t itself, read in place
    const double* q = p + t * nx;
    int qs = H * nx;
    if (rg) {
        double* qw = aff + A.q;
        for (int e = lane; e < nrhs * nx; e += nlanes) {
            const int c = e / nx, i = e - c * nx;
            double v = p[(c * H + t) * nx + i];
            for (int j = 0; j < nx; ++j) v += Pt[i * nx + j] * (double)rg[(size_t)c * hx + t * nx + j];
            qw[e] = v;
        }
        sync();
        q = qw;
        qs = nx;
    }
    // r^u + B' q
    for (int e = lane; e < nrhs * nu; e += nlanes) {
        const int c = e / nu, i = e - c * nu;
        double v = (double)rz[(size_t)c * n + hx + t * nu + i];
        for (int j = 0; j < nx; ++j) v += (double)At[j * nin + nx + i] * q[c * qs + j];
        kk[(c * H + t) * nu + i] = v;
    }
    sync();
    // k = Quu^-1 (.) in place: one right-hand side per lane
    for (int c = lane; c < nrhs; c += nlanes) {
        double* y = kk + (c * H + t) * nu;
        for (int i = 0; i < nu; ++i) {
            double v = y[i];
            for (int j = 0; j < i; ++j) v -= Quu[i * nu + j] * y[j];
            y[i] = v;
        }
        for (int i = 0; i < nu; ++i) y[i] /= Quu[i * nu + i];
        for (int i = nu - 1; i >= 0; --i) {
            double v = y[i];
            for (int j = i + 1; j < nu; ++j) v -= Quu[j * nu + i] * y[j];
            y[i] = v;
        }
    }
    sync();
    if (t > 0) {
        // p_{t-1} = r^x_{t-1} + A' q - Qux' k
        for (int e = lane; e < nrhs * nx; e += nlanes) {
            const int c = e / nx, i = e - c * nx;
            double v = (double)rz[(size_t)c * n + (t - 1) * nx + i];
            for (int j = 0; j < nx; ++j) v += (double)At[j * nin + i] * q[c * qs + j];
            for (int j = 0; j < nu; ++j) v -= Qux[j * nx + i] * kk[(c * H + t) * nu + j];
            p[(c * H + t - 1) * nx + i] = v;
        }
        sync();
    }
}

// One forward stage.  Kt (nu, nx), Pt (nx, nx; read when w or gx0 is asked for), W0 = Lagrangian block 0 (read at t = 0 for
// gx0).  v (nrhs, n), w (nrhs, H nx), gx0 (nrhs, nx): this problem's outputs, each may be null.
template <typename T, typename Sync>
NEMPC_SENS_HD inline void kktsolve_forward_stage(int lane, int nlanes, Sync sync, int t, int H, int nx, int nu, int nrhs,
                                                 const T* At, const T* W0, const double* Kt, const double* Pt, const T* rg,
                                                 double* aff, T* v, T* w, T* gx0) {
    const KktSolveLayout A = kktsolve_layout(H, nx, nu, nrhs);
    const int nin = nx + nu, n = H * nin, hx = H * nx;
    const double* xp = aff + ((t & 1) ? A.xb : A.xa);     // v_x[t-1] (nothing at t = 0: v_x[-1] = 0)
    double* xn = aff + ((t & 1) ? A.xa : A.xb);
    double *u = aff + A.u, *w0 = aff + A.q;
    const double *p = aff + A.p, *kk = aff + A.k;
    for (int e = lane; e < nrhs * nu; e += nlanes) {
        const int c = e / nu, i = e - c * nu;
        double s = kk[(c * H + t) * nu + i];
        if (t > 0)
            for (int j = 0; j < nx; ++j) s += Kt[i * nx + j] * xp[c * nx + j];
        u[e] = s;
        if (v) v[(size_t)c * n + hx + t * nu + i] = (T)s;
    }
    sync();
    for (int e = lane; e < nrhs * nx; e += nlanes) {
        const int c = e / nx, i = e - c * nx;
        double s = rg ? -(double)rg[(size_t)c * hx + t * nx + i] : 0.0;
        if (t > 0)
            for (int j = 0; j < nx; ++j) s += (double)At[i * nin + j] * xp[c * nx + j];
        for (int j = 0; j < nu; ++j) s += (double)At[i * nin + nx + j] * u[c * nu + j];
        xn[e] = s;
        if (v) v[(size_t)c * n + t * nx + i] = (T)s;
    }
    sync();
    if (!w && !(gx0 && t == 0)) return;
    for (int e = lane; e < nrhs * nx; e += nlanes) {
        const int c = e / nx, i = e - c * nx;
        double s = -p[(c * H + t) * nx + i];
        for (int j = 0; j < nx; ++j) s += Pt[i * nx + j] * xn[c * nx + j];
        if (t == 0) w0[e] = s;
        if (w) w[(size_t)c * hx + t * nx + i] = (T)s;
    }
    if (gx0 && t == 0) {
        sync();
        for (int e = lane; e < nrhs * nx; e += nlanes) {
            const int c = e / nx, i = e - c * nx;
            double s = 0.0;
            for (int j = 0; j < nu; ++j) s += (double)W0[(nx + j) * nin + i] * u[c * nu + j];
            for (int j = 0; j < nx; ++j) s += (double)At[j * nin + i] * w0[c * nx + j];
            gx0[(size_t)c * nx + i] = (T)(-s);
        }
        sync();     // (stage 1 overwrites v_u)
    }
}

// The whole solve of ONE problem: arguments as sens_problem, plus nrhs right-hand sides rz (nrhs, n), rg (nrhs, H nx) or null
// (zeros), the working set aff (kktsolve_layout(H, nx, nu, nrhs).total doubles) and the outputs.  Kst (H, nu, nx) and
// Pst (H, nx, nx) are both required (P_t is stored only for the stages where something reads it).  `sync_stored()` orders the stores to Kst / Pst before other lanes read them: between
// the sweeps, and -- when rg is given, so that q_t reads P_t -- after every backward stage.
// 0: done; 1: a pivot was not positive (no output has been written then).
template <typename T, typename Sync, typename SyncStored>
NEMPC_SENS_HD inline int kktsolve_problem(int lane, int nlanes, Sync sync, SyncStored sync_stored, int H, int nx, int nu,
                                          int nrhs, const T* tiles, const T* blocks, const T* Qs, const T* QTs, const T* Rs,
                                          const double* sig, const T* rz, const T* rg, double* ws, double* aff, double* Kst,
                                          double* Pst, T* v, T* w, T* gx0) {
    const SensLayout L = sens_layout(nx, nu);
    const KktSolveLayout A = kktsolve_layout(H, nx, nu, nrhs);
    const int nin = nx + nu, n = H * nin;
    const double* sig_u = sig + (size_t)H * nx;
    for (int e = lane; e < nx * nx; e += nlanes) {
        const int i = e / nx, j = e - i * nx;
        ws[L.P + e] = (double)QTs[e] + (i == j ? sig[(size_t)(H - 1) * nx + i] : 0.0);
    }
    for (int e = lane; e < nrhs * nx; e += nlanes) {
        const int c = e / nx, i = e - c * nx;
        aff[A.p + (c * H + H - 1) * nx + i] = (double)rz[(size_t)c * n + (H - 1) * nx + i];
    }
    sync();
    for (int t = H - 1; t >= 0; --t) {
        const T* At = tiles + (size_t)t * nx * nin;
        // (P_t is kept where something reads it: q_t with r^g, w_t, and w_0 for gx0)
        const bool keep_P = rg || w || (gx0 && t == 0);
        if (!sens_backward_stage<T>(lane, nlanes, sync, t, nx, nu, At, blocks + (size_t)t * nin * nin, Qs, Rs,
                                    t > 0 ? sig + (size_t)(t - 1) * nx : nullptr, sig_u + (size_t)t * nu, ws,
                                    Kst + (size_t)t * nu * nx, keep_P ? Pst + (size_t)t * nx * nx : nullptr))
            return 1;
        if (rg) sync_stored();
        kktsolve_backward_stage<T>(lane, nlanes, sync, t, H, nx, nu, nrhs, At, Pst + (size_t)t * nx * nx, rz, rg, ws, aff);
    }
    sync_stored();
    for (int t = 0; t < H; ++t)
        kktsolve_forward_stage<T>(lane, nlanes, sync, t, H, nx, nu, nrhs, tiles + (size_t)t * nx * nin, blocks,
                                  Kst + (size_t)t * nu * nx, Pst + (size_t)t * nx * nx, rg, aff, v, w, gx0);
    return 0;
}

}  // namespace nempc
