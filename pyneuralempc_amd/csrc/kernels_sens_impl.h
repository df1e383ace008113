// Arithmetic of the solution sensitivities dz*/dx0 (nempc_sensitivity, kernels_sens.hip), kept apart from the kernel's
// staging so that a host program can run the very same recursion with one lane (tests/sensitivity_check.cpp): this header
// includes nothing of the library and nothing of HIP.
//
// At a primal-dual point the perturbed KKT system [[W + Sigma, J'], [J, 0]] [dz ; dlam] = -d/dx0 [grad L ; g] is an LQ problem
// with zero linear terms and initial state dx_{-1} = I (include/nempc.h).  Stage t reads the Jacobian tile
// T_t = [A_t | B_t] (nx, nx+nu) and the Lagrangian block W_t (nx+nu, nx+nu) over (x_{t-1}, u_t):
//     backward, t = H-1 .. 0 (P_{H-1} = QTs + Sigma_x[H-1]):
//         PA = P A, PB = P B
//         Quu = Rs + Sigma_u[t] + W_uu + B' PB          Qux = W_ux + B' PA
//         Quu = L D L' (pivot test: every D_j > 0; no regularisation, ever)       K_t = -Quu^-1 Qux
//         t > 0:  P <- sym(Qs + Sigma_x[t-1] + W_xx + A' PA + Qux' K_t)
//     forward, t = 0 .. H-1 (D_{-1} = I):  dU_t = K_t D_{t-1},  D_t = A_t D_{t-1} + B_t dU_t,  dlam_t = P_t D_t
// Everything is double; T appears at loads of the stage data and at stores of the results only.
//
// Every function is called by `nlanes` cooperating lanes (lane = 0 .. nlanes-1) that share the working set `ws`; the
// entries of each small matrix are dealt out over the lanes and `sync()` separates dependent phases (a wave-level barrier
// on the device; nothing with nlanes = 1).
#pragma once

#include <stddef.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NEMPC_SENS_HD __host__ __device__
#else
#define NEMPC_SENS_HD
#endif

namespace nempc {

// |x| <= DBL_MAX without <cmath>: false for +-inf (and NaN)
NEMPC_SENS_HD inline bool sens_finite(double x) { return x >= -1.7976931348623157e308 && x <= 1.7976931348623157e308; }

// Sigma_i = zl/(z - lb) + zu/(ub - z) over the FINITE bounds.  A zero multiplier contributes 0 whatever the gap; a non-zero
// one on a gap <= 0 sets `bad` (Sigma is undefined there).
NEMPC_SENS_HD inline double sens_sigma_entry(double z, double vl, double vu, double lo, double hi, bool& bad) {
    double s = 0.0;
    if (sens_finite(lo) && vl != 0.0) {
        const double d = z - lo;
        if (d > 0.0) s += vl / d;
        else bad = true;
    }
    if (sens_finite(hi) && vu != 0.0) {
        const double d = hi - z;
        if (d > 0.0) s += vu / d;
        else bad = true;
    }
    return s;
}

// The working set of one problem (element offsets into ws, doubles).  The forward sweep reuses the backward sweep's
// regions: D ping-pongs between P and PA, dU lives in Qux.
struct SensLayout {
    int P, PA, Pn, PB, Qux, K, Quu, Y, flag, total;
};
NEMPC_SENS_HD inline SensLayout sens_layout(int nx, int nu) {
    SensLayout L;
    int p = 0;
    L.P = p; p += nx * nx;
    L.PA = p; p += nx * nx;
    L.Pn = p; p += nx * nx;
    L.PB = p; p += nx * nu;
    L.Qux = p; p += nu * nx;
    L.K = p; p += nu * nx;
    L.Quu = p; p += nu * nu;
    L.Y = p; p += nu * nx;      // one work vector (nu) per right-hand side of the gain solve
    L.flag = p; p += 1;         // factorisation verdict of the stage
    L.total = (p + 1) & ~1;     // (even: a problem's region stays 16-byte aligned behind another's)
    return L;
}

// One backward stage.  At (nx, nx+nu), Wt (nx+nu, nx+nu); Qs (nx, nx) and sig_xprev (nx) belong to x_{t-1} and are read
// for t > 0 only; sig_u (nu) belongs to u_t.  ws holds P_t on entry and P_{t-1} on return (t > 0).  K_t goes to Kt (nu, nx)
// and P_t to Pt (nx, nx; may be null).  false: a pivot of Quu was not positive (every lane returns the same verdict).
template <typename T, typename Sync>
NEMPC_SENS_HD inline bool sens_backward_stage(int lane, int nlanes, Sync sync, int t, int nx, int nu, const T* At, const T* Wt,
                                              const T* Qs, const T* Rs, const double* sig_xprev, const double* sig_u,
                                              double* ws, double* Kt, double* Pt) {
    const SensLayout L = sens_layout(nx, nu);
    const int nin = nx + nu;
    double *P = ws + L.P, *PA = ws + L.PA, *Pn = ws + L.Pn, *PB = ws + L.PB, *Qux = ws + L.Qux, *K = ws + L.K,
           *Quu = ws + L.Quu, *Y = ws + L.Y;
    // PA = P A, PB = P B; P_t for the multipliers' sensitivities
    for (int e = lane; e < nx * nx + nx * nu + (Pt ? nx * nx : 0); e += nlanes) {
        int r = e;
        if (r < nx * nx) {
            const int i = r / nx, j = r - i * nx;
            double v = 0.0;
            for (int k = 0; k < nx; ++k) v += P[i * nx + k] * (double)At[k * nin + j];
            PA[r] = v;
            continue;
        }
        r -= nx * nx;
        if (r < nx * nu) {
            const int i = r / nu, j = r - i * nu;
            double v = 0.0;
            for (int k = 0; k < nx; ++k) v += P[i * nx + k] * (double)At[k * nin + nx + j];
            PB[r] = v;
            continue;
        }
        r -= nx * nu;
        Pt[r] = P[r];
    }
    sync();
    // Quu = Rs + Sigma_u + W_uu + B' PB, Qux = W_ux + B' PA
    for (int e = lane; e < nu * nu + nu * nx; e += nlanes) {
        int r = e;
        if (r < nu * nu) {
            const int i = r / nu, j = r - i * nu;
            double v = (double)Rs[r] + (double)Wt[(nx + i) * nin + nx + j] + (i == j ? sig_u[i] : 0.0);
            for (int k = 0; k < nx; ++k) v += (double)At[k * nin + nx + i] * PB[k * nu + j];
            Quu[r] = v;
            continue;
        }
        r -= nu * nu;
        const int i = r / nx, j = r - i * nx;
        double v = (double)Wt[(nx + i) * nin + j];
        for (int k = 0; k < nx; ++k) v += (double)At[k * nin + nx + i] * PA[k * nx + j];
        Qux[r] = v;
    }
    sync();
    // Quu = L D L' in place from the lower triangle (unit L below the diagonal, D on it): small and serial, one lane.  The
    // pivots D_j are the squares of the Cholesky diagonal, so the verdict is the Cholesky verdict.
    if (lane == 0) {
        double ok = 1.0;
        for (int j = 0; j < nu; ++j) {
            double d = Quu[j * nu + j];
            for (int k = 0; k < j; ++k) d -= Quu[j * nu + k] * Quu[j * nu + k] * Quu[k * nu + k];
            if (!(d > 0.0)) { ok = 0.0; break; }
            Quu[j * nu + j] = d;
            for (int i = j + 1; i < nu; ++i) {
                double v = Quu[i * nu + j];
                for (int k = 0; k < j; ++k) v -= Quu[i * nu + k] * Quu[j * nu + k] * Quu[k * nu + k];
                Quu[i * nu + j] = v / d;
            }
        }
        ws[L.flag] = ok;
    }
    sync();
    if (!(ws[L.flag] > 0.0)) return false;
    // K = -Quu^-1 Qux: one right-hand side (column of Qux) per lane
    for (int col = lane; col < nx; col += nlanes) {
        double* y = Y + col * nu;
        for (int i = 0; i < nu; ++i) {
            double v = Qux[i * nx + col];
            for (int k = 0; k < i; ++k) v -= Quu[i * nu + k] * y[k];
            y[i] = v;
        }
        for (int i = 0; i < nu; ++i) y[i] /= Quu[i * nu + i];
        for (int i = nu - 1; i >= 0; --i) {
            double v = y[i];
            for (int k = i + 1; k < nu; ++k) v -= Quu[k * nu + i] * y[k];
            y[i] = v;
        }
        for (int i = 0; i < nu; ++i) {
            K[i * nx + col] = -y[i];
            Kt[i * nx + col] = -y[i];
        }
    }
    sync();
    if (t > 0) {
        for (int e = lane; e < nx * nx; e += nlanes) {
            const int i = e / nx, j = e - i * nx;
            double v = (double)Qs[e] + (double)Wt[i * nin + j] + (i == j ? sig_xprev[i] : 0.0);
            for (int k = 0; k < nx; ++k) v += (double)At[k * nin + i] * PA[k * nx + j];
            for (int k = 0; k < nu; ++k) v += Qux[k * nx + i] * K[k * nx + j];
            Pn[e] = v;
        }
        sync();
        for (int e = lane; e < nx * nx; e += nlanes) {
            const int i = e / nx, j = e - i * nx;
            P[e] = 0.5 * (Pn[i * nx + j] + Pn[j * nx + i]);
        }
        sync();
    }
    return true;
}

// One forward stage: ws holds D_{t-1} on entry (nothing at t = 0: D_{-1} = I is never formed, K_0 and A_0 are copied) and
// D_t on return.  Kt (nu, nx), Pt (nx, nx; read only when dlam is asked for).  dU0 (nu, nx), dZ (n, nx), dlam (H nx, nx),
// gains (H, nu, nx): this problem's outputs, each may be null.
template <typename T, typename Sync>
NEMPC_SENS_HD inline void sens_forward_stage(int lane, int nlanes, Sync sync, int t, int H, int nx, int nu, const T* At,
                                             const double* Kt, const double* Pt, double* ws, T* dU0, T* dZ, T* dlam, T* gains) {
    const SensLayout L = sens_layout(nx, nu);
    const int nin = nx + nu;
    const double* D = ws + ((t & 1) ? L.PA : L.P);
    double* Dn = ws + ((t & 1) ? L.P : L.PA);
    double* U = ws + L.Qux;
    for (int e = lane; e < nu * nx; e += nlanes) {
        const int i = e / nx, j = e - i * nx;
        double v = Kt[e];
        if (t > 0) {
            v = 0.0;
            for (int k = 0; k < nx; ++k) v += Kt[i * nx + k] * D[k * nx + j];
        }
        U[e] = v;
        if (dZ) dZ[(size_t)(H * nx + t * nu) * nx + e] = (T)v;
        if (dU0 && t == 0) dU0[e] = (T)v;
        if (gains) gains[(size_t)t * nu * nx + e] = (T)Kt[e];
    }
    sync();
    for (int e = lane; e < nx * nx; e += nlanes) {
        const int i = e / nx, j = e - i * nx;
        double v = (double)At[i * nin + j];
        if (t > 0) {
            v = 0.0;
            for (int k = 0; k < nx; ++k) v += (double)At[i * nin + k] * D[k * nx + j];
        }
        for (int k = 0; k < nu; ++k) v += (double)At[i * nin + nx + k] * U[k * nx + j];
        Dn[e] = v;
        if (dZ) dZ[(size_t)t * nx * nx + e] = (T)v;
    }
    sync();
    if (dlam) {
        for (int e = lane; e < nx * nx; e += nlanes) {
            const int i = e / nx, j = e - i * nx;
            double v = 0.0;
            for (int k = 0; k < nx; ++k) v += Pt[i * nx + k] * Dn[k * nx + j];
            dlam[(size_t)t * nx * nx + e] = (T)v;
        }
    }
}

// The whole recursion of ONE problem.  tiles (H, nx, nx+nu), blocks (H, nx+nu, nx+nu); Qs, QTs (nx, nx), Rs (nu, nu) the
// symmetrised objective weights; sig (n) Sigma in z order (states, then controls).  ws: sens_layout(nx, nu).total doubles;
// Kst (H, nu, nx) and Pst (H, nx, nx; required when dlam is asked for, else may be null) are written backward and read
// forward by other lanes than wrote them: `sync_stored()` between the two sweeps makes them visible (on the device a
// barrier that also orders the stores to Kst / Pst, which the per-phase `sync` need not when ws is on-chip memory).
// 0: done; 1: a pivot was not positive (no output has been written then).
template <typename T, typename Sync, typename SyncStored>
NEMPC_SENS_HD inline int sens_problem(int lane, int nlanes, Sync sync, SyncStored sync_stored, int H, int nx, int nu,
                                      const T* tiles, const T* blocks,
                                      const T* Qs, const T* QTs, const T* Rs, const double* sig, double* ws, double* Kst,
                                      double* Pst, T* dU0, T* dZ, T* dlam, T* gains) {
    const SensLayout L = sens_layout(nx, nu);
    const int nin = nx + nu;
    const double* sig_u = sig + (size_t)H * nx;
    if (!dlam) Pst = nullptr;
    for (int e = lane; e < nx * nx; e += nlanes) {
        const int i = e / nx, j = e - i * nx;
        ws[L.P + e] = (double)QTs[e] + (i == j ? sig[(size_t)(H - 1) * nx + i] : 0.0);
    }
    sync();
    for (int t = H - 1; t >= 0; --t) {
        if (!sens_backward_stage<T>(lane, nlanes, sync, t, nx, nu, tiles + (size_t)t * nx * nin, blocks + (size_t)t * nin * nin,
                                    Qs, Rs, t > 0 ? sig + (size_t)(t - 1) * nx : nullptr, sig_u + (size_t)t * nu, ws,
                                    Kst + (size_t)t * nu * nx, Pst ? Pst + (size_t)t * nx * nx : nullptr))
            return 1;
    }
    sync_stored();
    for (int t = 0; t < H; ++t)
        sens_forward_stage<T>(lane, nlanes, sync, t, H, nx, nu, tiles + (size_t)t * nx * nin, Kst + (size_t)t * nu * nx,
                              Pst ? Pst + (size_t)t * nx * nx : nullptr, ws, dU0, dZ, dlam, gains);
    return 0;
}

}  // namespace nempc
