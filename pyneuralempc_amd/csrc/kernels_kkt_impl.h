// Per-variable arithmetic of the KKT residual evaluator (nempc_kkt_residual, kernels_post.hip), kept apart from the kernel's
// indexing and reduction so that a host program can call the very same function (tests/kkt_residual_check.cpp): this
// header includes nothing of the library and nothing of HIP.
//
// Convention (include/nempc.h):  g = Phi - x,  L = f + lam.g - zl.(z - lb) + zu.(z - ub),  zl, zu >= 0, so that
//     s = grad f + J' lam - zl + zu.
// J' lam is formed straight from the compact tiles T_t = d Phi(x_{t-1}, u_t) / d[x_{t-1} | u_t]  (H, nx, nx+nu):
//     state   x_t[j]:  -lam_t[j] + sum_k T_{t+1}[k][j] lam_{t+1}[k]   (no second term at t = H-1)   [+ lam_box[t][j]]
//     control u_t[j]:   sum_k T_t[k][nx+j] lam_t[k]
// Sums run in double whatever T is.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NEMPC_KKT_HD __host__ __device__
#else
#define NEMPC_KKT_HD
#endif

namespace nempc {

struct KktTerms {
    double s;       // stationarity entry of the variable
    double pfeas;   // max((lb - z)+, (z - ub)+)
    double comp;    // max over the variable's FINITE bounds of |zl (z - lb)|, |zu (ub - z)|
    double dfeas;   // max(0, -zl, -zu)
};

// |x| <= DBL_MAX without <cmath>: false for +-inf (and NaN)
NEMPC_KKT_HD inline bool kkt_finite(double x) { return x >= -1.7976931348623157e308 && x <= 1.7976931348623157e308; }

// Variable i (< n = H (nx + nu)) of ONE problem.  z, grad (n), tiles (H, nx, nx+nu), lam (m: H nx defect multipliers, then
// H nx box-row multipliers when `box`) point at that problem's rows; zl / zu (n) may be null (= zeros); lb / ub (n) may be
// null (= unbounded) and hold +-infinity for a missing bound.  A multiplier on an infinite bound counts as zero.
// kkt_variable_terms_at takes the variable's two bounds by value (+-infinity for a missing one): the kernel hands it the
// problem's own effective bounds when per-problem bounds are bound (nempc_bind_bounds).
template <typename T>
NEMPC_KKT_HD inline KktTerms kkt_variable_terms_at(int i, int H, int nx, int nu, bool box, const T* z, const T* grad,
                                                   const T* tiles, const T* lam, const T* zl, const T* zu, double lo,
                                                   double hi) {
    const int nin = nx + nu, hx = H * nx;
    double s = (double)grad[i];
    if (i < hx) {
        const int t = i / nx, j = i - t * nx;
        s -= (double)lam[i];
        if (t + 1 < H) {
            const T* Tn = tiles + (t + 1) * nx * nin;
            const T* ln = lam + (t + 1) * nx;
            for (int k = 0; k < nx; ++k) s += (double)Tn[k * nin + j] * (double)ln[k];
        }
        if (box) s += (double)lam[hx + i];
    } else {
        const int c = i - hx, t = c / nu, j = c - t * nu;
        const T* Tt = tiles + t * nx * nin;
        const T* lt = lam + t * nx;
        for (int k = 0; k < nx; ++k) s += (double)Tt[k * nin + nx + j] * (double)lt[k];
    }
    const double zi = (double)z[i];
    const bool flo = kkt_finite(lo), fhi = kkt_finite(hi);
    const double vl = flo && zl ? (double)zl[i] : 0.0, vu = fhi && zu ? (double)zu[i] : 0.0;
    KktTerms r;
    r.s = s - vl + vu;
    r.pfeas = 0.0;
    r.comp = 0.0;
    r.dfeas = 0.0;
    if (flo) {
        const double d = zi - lo, c = vl * d;
        if (-d > r.pfeas) r.pfeas = -d;
        if (c > r.comp) r.comp = c;
        if (-c > r.comp) r.comp = -c;
        if (-vl > r.dfeas) r.dfeas = -vl;
    }
    if (fhi) {
        const double d = hi - zi, c = vu * d;
        if (-d > r.pfeas) r.pfeas = -d;
        if (c > r.comp) r.comp = c;
        if (-c > r.comp) r.comp = -c;
        if (-vu > r.dfeas) r.dfeas = -vu;
    }
    return r;
}

template <typename T>
NEMPC_KKT_HD inline KktTerms kkt_variable_terms(int i, int H, int nx, int nu, bool box, const T* z, const T* grad,
                                                const T* tiles, const T* lam, const T* zl, const T* zu, const double* lb,
                                                const double* ub) {
    return kkt_variable_terms_at<T>(i, H, nx, nu, box, z, grad, tiles, lam, zl, zu, lb ? lb[i] : -__builtin_huge_val(),
                                    ub ? ub[i] : __builtin_huge_val());
}

}  // namespace nempc
