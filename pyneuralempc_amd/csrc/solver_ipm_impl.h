// Batched solver, variable bounds by an interior point: barrier gradient and diagonal, dual steps, the log-barrier value
// and l1 norm the merit function sums, and the strictly interior start.  Included by solver.hip only.
#pragma once

namespace nempc {

namespace {

// ---- bounds by a PRIMAL-DUAL interior point (round 2; the first version was the primal log barrier, Hessian term
// mu/d^2).  With multipliers zl, zu of z >= lb, z <= ub the Newton system of the perturbed KKT conditions, reduced to
// the primal step, has  Hessian + diag(zl/dl + zu/du)  and gradient  grad f - mu/dl + mu/du  (dl = z-lb, du = ub-z);
// the dual steps follow from the primal one,  dzl = mu/dl - zl - (zl/dl) dz,  dzu = mu/du - zu + (zu/du) dz,  and are
// taken to their own fraction-to-the-boundary length.  The diagonal zl/dl stays moderate on a variable that sits at its
// bound with a small multiplier, where mu/dl^2 explodes -- the stragglers of the primal version were exactly the
// problems whose steps kept being cut by the boundary (NEMPC_SOLVER_TRACE).  Both terms keep the LQ structure.
// Runs before the LQ kernel: writes the diagonal bh and folds the barrier gradient into grad.
template <typename T>
__global__ __launch_bounds__(256) void solver_barrier_kernel(SolverArgs a) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx == 0) *a.n_active = 0;      // counter of the convergence test that follows the LQ solve (a memset launch before)
    if (idx >= (size_t)a.B * a.n) return;
    const int b = (int)(idx / a.n), i = (int)(idx - (size_t)b * a.n);
    T ga = T(0), ha = T(0);
    const T mu = ((const T*)a.mu)[b];
    if (mu > T(0) && a.status[b] < 0) {
        const T z = ((const T*)a.Z)[idx], lo = solver_lb<T>(a, b)[i], hi = solver_ub<T>(a, b)[i];
        if (lo > -std::numeric_limits<T>::max()) {
            const T d = z - lo;
            ga -= mu / d;
            ha += a.primal_dual ? ((const T*)a.zl)[idx] / d : mu / (d * d);
        }
        if (hi < std::numeric_limits<T>::max()) {
            const T d = hi - z;
            ga += mu / d;
            ha += a.primal_dual ? ((const T*)a.zu)[idx] / d : mu / (d * d);
        }
    }
    ((T*)a.bh)[idx] = ha;
    ((T*)a.grad)[idx] += ga;
}

// after the LQ solve: dual steps and their fraction-to-the-boundary length (one wave per problem)
template <typename T>
__device__ __forceinline__ void solver_dual_body(const SolverArgs& a, int b, int lane, const T* __restrict__ zp,
                                                 const T* __restrict__ dzp, T mu, int status, const T* lbp = nullptr,
                                                 const T* ubp = nullptr, const T* zlp = nullptr, const T* zup = nullptr) {
    // zp / dzp: the problem's iterate and step (global memory, or the Riccati kernel's LDS copies); lbp / ubp / zlp / zup:
    // staged copies of the bounds and of this problem's bound multipliers, when the caller has them
    if (!a.primal_dual) return;
    const T tau = T(0.995);
    T amax = T(1);
    const T* lbv = lbp ? lbp : solver_lb<T>(a, b);
    const T* ubv = ubp ? ubp : solver_ub<T>(a, b);
    const T* zlv = zlp ? zlp : (const T*)a.zl + (size_t)b * a.n;
    const T* zuv = zup ? zup : (const T*)a.zu + (size_t)b * a.n;
    if (mu > T(0) && status < 0)
        for (int i = lane; i < a.n; i += 64) {
            const size_t idx = (size_t)b * a.n + i;
            const T z = zp[i], d = dzp[i], lo = lbv[i], hi = ubv[i];
            T sl = T(0), su = T(0);
            if (lo > -std::numeric_limits<T>::max()) {
                const T dl = z - lo, zl = zlv[i];
                sl = mu / dl - zl - (zl / dl) * d;
                if (sl < T(0)) amax = fmin(amax, -tau * zl / sl);
            }
            if (hi < std::numeric_limits<T>::max()) {
                const T du = hi - z, zu = zuv[i];
                su = mu / du - zu + (zu / du) * d;
                if (su < T(0)) amax = fmin(amax, -tau * zu / su);
            }
            ((T*)a.dzl)[idx] = sl;
            ((T*)a.dzu)[idx] = su;
        }
    amax = (T)wave_min_lane0((double)amax);
    if (lane == 0) ((T*)a.alz)[b] = amax;
}

// The barrier terms of variable i of problem b at the iterate -- what solver_barrier_kernel writes, for the LQ kernels
// that stage their working set in LDS and fold it in while staging (one launch less per iteration): ga joins the
// gradient, ha is the diagonal of the LQ model
template <typename T>
__device__ __forceinline__ void barrier_terms_of(bool primal_dual, T mu, int status, T z, T lo, T hi, T zl, T zu, T& ga, T& ha) {
    ga = T(0); ha = T(0);
    if (mu > T(0) && status < 0) {
        if (lo > -std::numeric_limits<T>::max()) {
            const T d = z - lo;
            ga -= mu / d;
            ha += primal_dual ? zl / d : mu / (d * d);
        }
        if (hi < std::numeric_limits<T>::max()) {
            const T d = hi - z;
            ga += mu / d;
            ha += primal_dual ? zu / d : mu / (d * d);
        }
    }
}
template <typename T>
__device__ __forceinline__ void solver_barrier_terms(const SolverArgs& a, int b, int i, T& ga, T& ha) {
    ga = T(0); ha = T(0);
    const T mu = ((const T*)a.mu)[b];
    const int status = a.status[b];
    if (mu > T(0) && status < 0) {
        const size_t idx = (size_t)b * a.n + i;
        const T z = ((const T*)a.Z)[idx], lo = solver_lb<T>(a, b)[i], hi = solver_ub<T>(a, b)[i];
        const bool lof = lo > -std::numeric_limits<T>::max(), hif = hi < std::numeric_limits<T>::max();
        barrier_terms_of<T>(a.primal_dual, mu, status, z, lo, hi, a.primal_dual && lof ? ((const T*)a.zl)[idx] : T(0),
                            a.primal_dual && hif ? ((const T*)a.zu)[idx] : T(0), ga, ha);
    }
}

// log-barrier value of one problem's variables, summed by a wave
template <typename T>
__device__ __forceinline__ double barrier_value(const T* z, const T* lb, const T* ub, int n, T mu, int lane) {
    double acc = 0.0;
    if (mu > T(0))
        for (int i = lane; i < n; i += 64) {
            if (lb[i] > -std::numeric_limits<T>::max()) acc -= (double)mu * log((double)(z[i] - lb[i]));
            if (ub[i] < std::numeric_limits<T>::max()) acc -= (double)mu * log((double)(ub[i] - z[i]));
        }
    return wave_bcast_lane0(wave_sum_lane0(acc));
}

template <typename T>
__device__ __forceinline__ double l1_norm(const T* g, int m, int lane) {
    double acc = 0.0;
    for (int i = lane; i < m; i += 64) acc += fabs((double)g[i]);
    return wave_bcast_lane0(wave_sum_lane0(acc));
}

// strictly interior start + per-problem state
// the caller's initial guess, moved into the interior of its bounds.  Distance kept from a bound: 1e-2 for the default
// barrier parameter; a warm start (small mu_init) stays closer to the active bounds it was handed
template <typename T>
__device__ __forceinline__ T start_inside(T z, T lo, T hi, T mu0, int has_bounds) {
    const bool flo = lo > -std::numeric_limits<T>::max(), fhi = hi < std::numeric_limits<T>::max();
    T marg = has_bounds ? fmin(T(1e-2), fmax(T(10) * mu0, T(1e-6))) : T(1e-2);
    if (flo && fhi) marg = fmin(marg, T(0.25) * (hi - lo));
    if (flo) z = fmax(z, lo + marg);
    if (fhi) z = fmin(z, hi - marg);
    return z;
}

template <typename T>
__global__ __launch_bounds__(256) void solver_init_kernel(int B, int n, T* __restrict__ Z, const T* __restrict__ lb,
                                                          const T* __restrict__ ub, T* mu, T* nu, T* reg, int* status,
                                                          int* orig, int* iters_done, T* info, T* zl, T* zu, T mu0,
                                                          T reg0, int has_bounds, const T* __restrict__ Zin,
                                                          const T* __restrict__ X0in, T* __restrict__ X0c, int nx,
                                                          T* __restrict__ lam0, int m) {
    // (the working copies of the caller's Z and X0 and the zero multipliers come from this launch too: three copy / fill
    // launches less in a prologue that a single-problem closed loop pays every MPC step)
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (size_t)B * nx) X0c[i] = X0in[i];
    if (i < (size_t)B * m) lam0[i] = T(0);
    if (i < (size_t)B) {
        mu[i] = has_bounds ? mu0 : T(0); nu[i] = T(1); reg[i] = reg0; status[i] = -1;
        orig[i] = (int)i; iters_done[i] = 0;
        for (int k = 0; k < INFO_N; ++k) info[i * INFO_N + k] = std::numeric_limits<T>::max();   // "no previous step"
        info[i * INFO_N + INFO_LSK] = T(0);
        info[i * INFO_N + INFO_LSR] = T(0);
        info[i * INFO_N + INFO_PHN] = T(0);
        info[i * INFO_N + INFO_PHUP] = T(0);
    }
    if (i >= (size_t)B * n) return;
    const int k = (int)(i % n);
    const T lo = lb[k], hi = ub[k];
    const bool flo = lo > -std::numeric_limits<T>::max(), fhi = hi < std::numeric_limits<T>::max();
    const T z = start_inside(Zin[i], lo, hi, mu0, has_bounds);
    Z[i] = z;
    if (zl) {   // bound multipliers on the central path of the first barrier parameter
        zl[i] = flo ? mu0 / (z - lo) : T(0);
        zu[i] = fhi ? mu0 / (hi - z) : T(0);
    }
}

// The same start with per-problem bounds bound (nempc_bind_bounds): one workgroup per problem.  A first pass over the
// problem's n variables forms the effective bounds -- the shared vector (host lb / ub and box rows, already intersected)
// intersected with the problem's rows of the binding, +-inf and magnitudes at or above the dtype's max as +-max -- and
// decides two things for the whole problem: whether any bound is finite (none: mu = 0, the problem runs as an unbounded
// one and never walks the barrier schedule) and whether some variable has lo >= hi or a NaN bound.  Such a problem is
// finished from the start: status 1, Z as handed in, zero multipliers, and NO bounds in the working copy, so that no
// kernel forms a barrier term for it.  The second pass writes the working copy (lbw / ubw, (B,n), the caller's order: this
// launch runs before any compaction) and what solver_init_kernel writes.
template <typename T>
__global__ __launch_bounds__(256) void solver_init_bound_kernel(int B, int n, int hx, BoundBind bb, const T* __restrict__ lb,
                                                                const T* __restrict__ ub, T* __restrict__ lbw,
                                                                T* __restrict__ ubw, T* __restrict__ Z, T* mu, T* nu, T* reg,
                                                                int* status, int* orig, int* iters_done, T* info, T* zl, T* zu,
                                                                T mu0, T reg0, const T* __restrict__ Zin,
                                                                const T* __restrict__ X0in, T* __restrict__ X0c, int nx,
                                                                T* __restrict__ lam0, int m) {
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b >= B) return;
    const T big = std::numeric_limits<T>::max();
    auto effective = [&](int i, T& lo, T& hi, bool& nan) {
        T bl, bu;
        bound_bind_pair<T>(bb, b, i, hx, bl, bu);
        nan = bl != bl || bu != bu;
        lo = fmax(lb[i], fmax(bl, -big));       // (-inf -> -max; a NaN operand is dropped by fmax: `nan` has it)
        hi = fmin(ub[i], fmin(bu, big));
    };
    int any = 0, bad = 0;
    for (int i = tid; i < n; i += 256) {
        T lo, hi; bool nan;
        effective(i, lo, hi, nan);
        any |= (lo > -big || hi < big) ? 1 : 0;
        bad |= (nan || !(lo < hi)) ? 1 : 0;
    }
    bad = __syncthreads_or(bad);
    any = __syncthreads_or(any);
    for (int i = tid; i < nx; i += 256) X0c[(size_t)b * nx + i] = X0in[(size_t)b * nx + i];
    for (int i = tid; i < m; i += 256) lam0[(size_t)b * m + i] = T(0);
    if (tid == 0) {
        mu[b] = any && !bad ? mu0 : T(0); nu[b] = T(1); reg[b] = reg0; status[b] = bad ? 1 : -1;
        orig[b] = b; iters_done[b] = 0;
        for (int k = 0; k < INFO_N; ++k) info[(size_t)b * INFO_N + k] = big;   // "no previous step"
        info[(size_t)b * INFO_N + INFO_LSK] = T(0);
        info[(size_t)b * INFO_N + INFO_LSR] = T(0);
        info[(size_t)b * INFO_N + INFO_PHN] = T(0);
        info[(size_t)b * INFO_N + INFO_PHUP] = T(0);
    }
    for (int i = tid; i < n; i += 256) {
        const size_t k = (size_t)b * n + i;
        T lo, hi; bool nan;
        effective(i, lo, hi, nan);
        if (bad) { lo = -big; hi = big; }
        lbw[k] = lo; ubw[k] = hi;
        const bool flo = lo > -big, fhi = hi < big;
        const T z = bad ? Zin[k] : start_inside(Zin[k], lo, hi, mu0, 1);
        Z[k] = z;
        if (zl) {
            zl[k] = flo ? mu0 / (z - lo) : T(0);
            zu[k] = fhi ? mu0 / (hi - z) : T(0);
        }
    }
}

}  // namespace

}  // namespace nempc
