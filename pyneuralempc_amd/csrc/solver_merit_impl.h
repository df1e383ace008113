// Batched solver, globalisation: convergence test and merit at the iterate, the trial point, the acceptance test
// (deferred and inner-loop backtracking) and the second-order correction.  The bodies are called from the LQ kernels
// too, so solver.hip includes this header ahead of theirs.  Included by solver.hip only.
#pragma once

namespace nempc {

namespace {

// mode 0: after the LQ solve -- convergence / barrier update, penalty update, merit at the iterate, first step length
// mode 1: after evaluating the trial point -- Armijo test, accept (copy) or halve
// Convergence test, barrier update and merit at the iterate (after the LQ solve), one wave per problem.  Returns, the same
// in every lane, whether the problem takes no step this iteration (`lsd`) and the step length of its first trial (`al`).
template <typename T>
__device__ __forceinline__ StepInfo<T> step_info_from(const SolverArgs& a, int b, const T* __restrict__ f) {
    const T* info = (const T*)a.info + (size_t)b * INFO_N;
    return StepInfo<T>{info[INFO_GINF], info[INFO_STEP], info[INFO_ZINF], info[INFO_LAM], info[INFO_D0], info[INFO_AMAX],
                       info[INFO_LSK], info[INFO_LSA], info[INFO_RESTARTS], info[INFO_LSR],
                       ((const T*)a.mu)[b], ((const T*)a.pen)[b], f[b], a.status[b]};
}
// zp, gp: the problem's iterate and defects (global memory, or the Riccati kernel's LDS copies)
template <typename T>
__device__ __forceinline__ void solver_merit0_body(const SolverArgs& a, int b, int lane, const T* __restrict__ f,
                                                   const T* __restrict__ zp, const T* __restrict__ gp, const StepInfo<T>& si,
                                                   int& lsd, T& al, const T* lbp = nullptr, const T* ubp = nullptr) {
    T* mu = (T*)a.mu; T* nu = (T*)a.pen; T* alpha = (T*)a.alpha; T* phi0 = (T*)a.phi0; T* dir = (T*)a.dir;
    const T* lb = lbp ? lbp : solver_lb<T>(a, b);
    const T* ub = ubp ? ubp : solver_ub<T>(a, b);
    const int H = a.H, nx = a.nx;
    lsd = 1;
    al = T(0);
    if (si.status >= 0) { if (lane == 0) a.lsdone[b] = 1; return; }
    if (si.restarts < T(0)) {    // the Riccati sweep ran out of attempts: no step this iteration, still unconverged
        if (lane == 0) { a.lsdone[b] = 1; atomicAdd(a.n_active, 1); }
        return;
    }
    // converged for the current barrier parameter?  Sub-problems with mu above its floor are only solved to
    // an accuracy proportional to mu (kappa = 10); the last one to the requested tolerances.
    const T mub = si.mu;
    const bool last_mu = !(mub > (T)a.mu_min * T(1.0001));
    const T tg = last_mu ? (T)a.tol_g : fmax((T)a.tol_g, T(10) * mub);
    const T tsx = last_mu ? (T)a.tol_step * (T(1) + si.zinf) : fmax((T)a.tol_step, T(10) * mub) * (T(1) + si.zinf);
    const bool conv = si.ginf <= tg && si.step <= tsx;
    if (conv) {
        if (!last_mu) {
            // superlinear decrease: mu <- max(mu_min, min(mu_factor * mu, mu^1.5))
            if (lane == 0) mu[b] = fmax(fmin(mub * (T)a.mu_factor, mub * sqrt(mub)), (T)a.mu_min);
            // new sub-problem: skip this step (direction was computed for the old mu).  (Lowering mu one iteration
            // late instead, from the previous iteration's norms, so that no iteration is skipped, was measured:
            // same median iteration count, slightly fewer problems converged within 40 / 80 / 160 iterations.)
            if (lane == 0) { a.lsdone[b] = 1; atomicAdd(a.n_active, 1); }
        } else {
            if (lane == 0) { a.status[b] = 0; a.lsdone[b] = 1; a.iters_done[b] = a.cur_it + 1; }
        }
        return;
    }
    const double bar = barrier_value<T>(zp, lb, ub, a.n, mub, lane);
    const double g1 = l1_norm<T>(gp, H * nx, lane);
    // deferred backtracking: a problem whose last trial was rejected stands where it stood; this iteration
    // recomputed the same direction and tries it at half the rejected length
    lsd = 0;
    al = si.lsk > T(0) ? fmin(si.amax, si.lsa) : si.amax;
    if (lane == 0) {
        const T nun = fmax(si.nu, T(1.5) * si.lam + T(1e-3));
        nu[b] = nun;
        phi0[b] = (T)((double)si.f + bar + (double)nun * g1);
        dir[b] = si.d0 - nun * (T)g1;
        alpha[b] = al;
        // a retry iteration re-solves with the damping the opening iteration had to raise, so its own restart count
        // is zero: remember the opening one, or the accept below relaxes a term that was only just raised
        T* infw = (T*)a.info + (size_t)b * INFO_N;
        infw[INFO_LSR] = si.lsk > T(0) ? fmax(si.lsr, si.restarts) : si.restarts;
        a.lsdone[b] = 0;
        atomicAdd(a.n_active, 1);
    }
}

// After the LQ solve, ONE launch per iteration (three before: dual steps, merit at the iterate, first trial point): the
// dual steps of the bounds and their step length, the convergence test / barrier update / merit value, and the first
// trial point Zt = Z + alpha dz of the problems that take a step.  One wave per problem.
template <typename T>
__global__ __launch_bounds__(64) void solver_step_kernel(SolverArgs a, const T* __restrict__ f, const T* __restrict__ Zcur,
                                                         T* __restrict__ Zt) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b == 0 && lane == 0) *a.n_pending = 0;          // counted by the trial's acceptance test (solver_merit_kernel)
    if (b >= a.B) return;
    const T* z = Zcur + (size_t)b * a.n;
    const T* dz = (const T*)a.dz + (size_t)b * a.n;
    const StepInfo<T> si = step_info_from<T>(a, b, f);
    solver_dual_body<T>(a, b, lane, z, dz, si.mu, si.status);
    int lsd;
    T al;
    solver_merit0_body<T>(a, b, lane, f, z, (const T*)a.g + (size_t)b * a.m, si, lsd, al);
    for (int i = lane; i < a.n; i += 64) Zt[(size_t)b * a.n + i] = lsd ? z[i] : fma(al, dz[i], z[i]);
}

// Acceptance test of a trial point (Armijo on the l1 merit), one wave per problem
template <typename T>
__device__ __forceinline__ void solver_merit_body(const SolverArgs& a, const T* __restrict__ Zt, const T* __restrict__ gt,
                                                  const T* __restrict__ ft, T* __restrict__ Zcur, int last_ls,
                                                  const int* __restrict__ list_in, int* __restrict__ list_out,
                                                  int publish, int slot, int lane, int* n_active_word, int tag, int soc = 0) {
    // list_in: the trial buffers (Zt, gt, ft) hold only the problems that were still searching after the previous trial,
    // densely, in the order of that list (inner-loop backtracking); null: one slot per problem.  list_out: the problems
    // this trial rejects are appended for the next one.  slot / lane: the problem slot this wave works on; n_active_word /
    // tag: the convergence counter that is published (and cleared) and the iteration number it is published under.
    const int b = list_in ? list_in[slot] : slot;
    // the convergence counter of the NEXT iteration, when its test runs inside the Riccati kernel (the host's copy of this
    // iteration's count was issued before this launch)
    if (slot == 0 && lane == 0 && publish) {
        // first acceptance launch of the iteration: the iteration's convergence counter is complete (the Riccati / step
        // kernel that counts ran earlier in the stream).  It goes to pinned host memory by a plain store -- the host reads
        // it there whenever it likes: no copy launch, no event, no drained stream
        if (a.hpub) {
            const int v = *n_active_word;
            a.hpub[1] = v;
            if (v == 0 && a.hpub[2] == 0) a.hpub[2] = tag;
            __threadfence_system();
            a.hpub[0] = tag;
            __threadfence_system();
        }
        if (a.fuse_step) *n_active_word = 0;
    }
    if (b >= a.B) return;
    T* mu = (T*)a.mu; T* nu = (T*)a.pen; T* reg = (T*)a.reg; T* alpha = (T*)a.alpha; T* phi0 = (T*)a.phi0; T* dir = (T*)a.dir;
    const T* info = (const T*)a.info + (size_t)b * INFO_N;
    const T* lb = solver_lb<T>(a, b);
    const T* ub = solver_ub<T>(a, b);
    const int H = a.H, nx = a.nx;
    // objective value of the trial point, when no launch has left it in `ft` (shapes without the fused evaluation, and the
    // compiled shape whose trial launch computes the Lagrangian blocks instead): the wave has the point in hand, and a
    // launch of its own for one number per problem costs more than the number.  First in the kernel, before the problem's
    // scalars are waited for: its loads share their round trip.  (carry: the trial point's objective gradient is written too,
    // it is the next iterate's)
    // The kernel is a chain of global round trips of a lone wave (~1.5 us each): everything that does not depend on the
    // decision is requested HERE, before anything is waited for -- the problem's scalars, this lane's first element of every
    // array the merit value and the acceptance read (the loops below take it from registers in their first trip), the
    // first trips of the carried-over tiles / blocks -- and the objective's own loads follow in the same flight.
    const int done = a.lsdone[b];
    // (soc: the second-order-correction trial of a step that was just rejected -- its length is the one that trial had;
    //  alpha[b] was halved on the rejection)
    const T mub = mu[b], nub = nu[b], al = soc ? alpha[b] * T(2) : alpha[b], ph0 = phi0[b], drb = dir[b];
    T ftb = ft ? ft[slot] : T(0);
    const T az = a.primal_dual ? ((const T*)a.alz)[b] : T(0);
    const T lsr = info[INFO_LSR], lsk = info[INFO_LSK], regb = reg[b];
    const T* zt = Zt + (size_t)slot * a.n;
    const T* gtb = gt + (size_t)slot * a.m;
    const bool in0 = lane < a.n, isl0 = lane < H * nx, pdl = a.primal_dual != 0;
    const T zi_0 = in0 ? zt[lane] : T(0), lo_0 = in0 ? lb[lane] : T(0), hi_0 = in0 ? ub[lane] : T(0);
    const T gi_0 = isl0 ? gtb[lane] : T(0);
    const T l0_0 = isl0 ? ((const T*)a.lam)[(size_t)b * a.m + lane] : T(0), l1_0 = isl0 ? ((const T*)a.lamn)[(size_t)b * a.m + lane] : T(0);
    const T zl_0 = in0 && pdl ? ((const T*)a.zl)[(size_t)b * a.n + lane] : T(0), dl_0 = in0 && pdl ? ((const T*)a.dzl)[(size_t)b * a.n + lane] : T(0);
    const T zu_0 = in0 && pdl ? ((const T*)a.zu)[(size_t)b * a.n + lane] : T(0), du_0 = in0 && pdl ? ((const T*)a.dzu)[(size_t)b * a.n + lane] : T(0);
    constexpr int PRE_T = 2, PRE_H = 3;       // trips of the tile / block copies held in registers (2/1: 120 / 180 elements)
    const int ntl_c = H * nx * (nx + a.nu), nhb_c = H * (nx + a.nu) * (nx + a.nu);
    T tpre[PRE_T], hpre[PRE_H];
    if (a.carry) {
        #pragma unroll
        for (int k = 0; k < PRE_T; ++k) tpre[k] = lane + 64 * k < ntl_c ? ((const T*)a.tiles_t)[(size_t)b * ntl_c + lane + 64 * k] : T(0);
        #pragma unroll
        for (int k = 0; k < PRE_H; ++k) hpre[k] = a.hblk_t && lane + 64 * k < nhb_c ? ((const T*)a.hblk_t)[(size_t)b * nhb_c + lane + 64 * k] : T(0);
    }
    if (!ft && a.trk.B > 0)
        ftb = (T)wave_bcast_lane0(objective_row_value_tracking<T>(b, a.trk_prob[b], lane, H, nx, a.nu, a.oo, (const T*)a.obj, a.trk,
                                                                  zt, a.carry ? (T*)a.grad_t : (T*)nullptr));
    else if (!ft)
        ftb = (T)wave_bcast_lane0(objective_row_value<T>(b, lane, H, nx, a.nu, a.oo, (const T*)a.obj, zt,
                                                                 a.carry ? (T*)a.grad_t : (T*)nullptr));
    if (done) return;
    // log-barrier value and l1 norm of the defects at the trial point, one loop (the loads of both in flight together;
    // per-lane order and tree as barrier_value / l1_norm)
    double accb = 0.0, accg = 0.0;
    for (int i = lane; i < a.n; i += 64) {
        const bool first = i == lane;
        const T zi = first ? zi_0 : zt[i], lo = first ? lo_0 : lb[i], hi = first ? hi_0 : ub[i];
        const T gi = i < H * nx ? (first ? gi_0 : gtb[i]) : T(0);
        if (mub > T(0)) {
            if (lo > -std::numeric_limits<T>::max()) accb -= (double)mub * log((double)(zi - lo));
            if (hi < std::numeric_limits<T>::max()) accb -= (double)mub * log((double)(hi - zi));
        }
        if (i < H * nx) accg += fabs((double)gi);
    }
    const double bar = wave_bcast_lane0(wave_sum_lane0(accb));
    const double g1 = wave_bcast_lane0(wave_sum_lane0(accg));
    const T phit = (T)((double)ftb + bar + (double)nub * g1);
    // Armijo on the l1 merit; the directional derivative is negative for a descent direction
    // the slack absorbs the rounding of the merit value itself (f is a sum of ~n terms in T): without a dtype-sized one
    // an fp32 iterate close to its solution fails the test on noise, halves its step six times and gets damped
    const T slack = (T)a.armijo_slack;
    // Non-monotone reference (Grippo-Lampariello-Lucidi): the trial point has to improve on the LARGEST merit value of the
    // last iterates, not on the current one.  Near a feasible iterate a full SQP step moves along the constraint manifold
    // and raises the l1 merit through the second-order constraint violation times a penalty that tracks the multipliers
    // (order 250-700 at configs[2] dims): the monotone test cuts such steps to 2-5 % of their length for dozens of
    // iterations -- the Maratos effect (tools/c3_slow_trace.py).  History is only comparable under the same penalty and
    // barrier parameter; it starts over when either changes.
    T phref = ph0;
    const T phn = info[INFO_PHN];
    const bool hist_ok = a.nonmono > 0 && phn > T(0) && info[INFO_PHNU] == nub && info[INFO_PHMU] == mub;
    // Watchdog: after a step that was accepted UPHILL the next full step has to bring the merit below the value in front
    // of that step (a Maratos step is followed by one that restores feasibility and does; an iterate chattering across a
    // relu kink is not, and would otherwise be waved through forever), and a shortened one has to pass the monotone test.
    const bool up = info[INFO_PHUP] > T(0);
    if (hist_ok && !up) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (a.nonmono > k && phn > (T)k) phref = fmax(phref, info[INFO_PH1 + k]);
    } else if (hist_ok && up && al >= T(1)) {
        phref = info[INFO_PH1];
    }
    const bool ok = (phit == phit) && phit <= phref + T(1e-4) * al * fmin(drb, T(0)) + slack * fabs(phref);
    if (ok) {
        if (lane == 0 && a.nonmono > 0) {
            T* infw = (T*)a.info + (size_t)b * INFO_N;
            const T h1 = info[INFO_PH1], h2 = info[INFO_PH2], h3 = info[INFO_PH3];
            infw[INFO_PH4] = hist_ok ? h3 : ph0;
            infw[INFO_PH3] = hist_ok ? h2 : ph0;
            infw[INFO_PH2] = hist_ok ? h1 : ph0;
            infw[INFO_PH1] = ph0;
            infw[INFO_PHN] = hist_ok ? fmin(phn + T(1), T(4)) : T(1);
            infw[INFO_PHNU] = nub;
            infw[INFO_PHMU] = mub;
            infw[INFO_PHUP] = phit > ph0 ? T(1) : T(0);
        }
        T* lam = (T*)a.lam + (size_t)b * a.m;
        const T* lamn = (const T*)a.lamn + (size_t)b * a.m;
        // bound multipliers: their own step length, then kept within a factor kappa of mu / slack at the new point
        // (the safeguard of primal-dual interior-point codes: a multiplier far from the central path is pulled back)
        const bool duals = a.primal_dual && mub > T(0);
        const T kap = T(1e10);
        T* zl = (T*)a.zl + (size_t)b * a.n;
        T* zu = (T*)a.zu + (size_t)b * a.n;
        const T* dzl = (const T*)a.dzl + (size_t)b * a.n;
        const T* dzu = (const T*)a.dzu + (size_t)b * a.n;
        for (int i = lane; i < a.n; i += 64) {
            const bool first = i == lane;
            const T zi = first ? zi_0 : zt[i], lo = first ? lo_0 : lb[i], hi = first ? hi_0 : ub[i];
            const bool lof = duals && lo > -std::numeric_limits<T>::max(), hif = duals && hi < std::numeric_limits<T>::max();
            const bool isl = i < H * nx;
            const T l0 = isl ? (first ? l0_0 : lam[i]) : T(0), l1 = isl ? (first ? l1_0 : lamn[i]) : T(0);
            const T zl0 = lof ? (first ? zl_0 : zl[i]) : T(0), dl = lof ? (first ? dl_0 : dzl[i]) : T(0);
            const T zu0 = hif ? (first ? zu_0 : zu[i]) : T(0), du = hif ? (first ? du_0 : dzu[i]) : T(0);
            Zcur[(size_t)b * a.n + i] = zi;
            if (isl) lam[i] = fma(al, l1 - l0, l0);
            if (a.carry) {      // the accepted point's evaluation is the next iterate's: no launch for it
                ((T*)a.grad)[(size_t)b * a.n + i] = ((const T*)a.grad_t)[(size_t)b * a.n + i];
                if (i < a.m) ((T*)a.g)[(size_t)b * a.m + i] = gtb[i];
            }
            if (lof) {
                const T c = mub / (zi - lo);
                zl[i] = fmin(fmax(fma(az, dl, zl0), c / kap), c * kap);
            }
            if (hif) {
                const T c = mub / (hi - zi);
                zu[i] = fmin(fmax(fma(az, du, zu0), c / kap), c * kap);
            }
        }
        if (a.carry) {
            const int ntl = H * nx * (nx + a.nu);
            const T* ts = (const T*)a.tiles_t + (size_t)b * ntl;
            T* td = (T*)a.tiles + (size_t)b * ntl;
            #pragma unroll
            for (int k = 0; k < PRE_T; ++k)
                if (lane + 64 * k < ntl) td[lane + 64 * k] = tpre[k];
            for (int i = lane + 64 * PRE_T; i < ntl; i += 64) td[i] = ts[i];
            if (a.hblk_t) {
                const int nhb = nhb_c;
                const T* hs = (const T*)a.hblk_t + (size_t)b * nhb;
                T* hd = (T*)a.hblk + (size_t)b * nhb;
                #pragma unroll
                for (int k = 0; k < PRE_H; ++k)
                    if (lane + 64 * k < nhb) hd[lane + 64 * k] = hpre[k];
                for (int i = lane + 64 * PRE_H; i < nhb; i += 64) hd[i] = hs[i];
            }
            for (int i = a.n + lane; i < a.m; i += 64) ((T*)a.g)[(size_t)b * a.m + i] = gtb[i];      // (rows beyond n, if any)
            if (lane == 0) ((T*)a.f_it)[b] = ftb;
        }
        // relax the damping only after a sweep that went through at the first attempt: a term that had to be raised
        // this iteration would fail again right away and cost a full extra sweep
        if (lane == 0) {
            a.lsdone[b] = 1;
            // relax the damping only after a sweep that went through at the first attempt: a term that had to be raised
            // this iteration would fail again right away and cost a full extra sweep
            if (!(lsr > T(0))) reg[b] = fmax(regb * (T)a.reg_relax, T(1e-9));
            ((T*)a.info)[(size_t)b * INFO_N + INFO_LSK] = T(0);
        }
    } else if (lane == 0 && soc) {
        // the corrected point is no better: the backtracking goes on from the halved length the rejection left
        const int p = atomicAdd(a.n_pending, 1);
        if (list_out) list_out[p] = b;
    } else if (lane == 0) {
        alpha[b] = al * T(0.5);
        if (last_ls == 2) {
            // deferred backtracking (one trial per outer iteration): remember the halved length for the next iteration;
            // after max_ls rejections in a row the direction is given up and the next LQ solve is damped
            T* inf = (T*)a.info + (size_t)b * INFO_N;
            const T k = lsk + T(1);
            a.lsdone[b] = 1;
            if (k >= (T)a.max_ls) { inf[INFO_LSK] = T(0); reg[b] = fmin(fmax(regb * T(100), T(1e-6)), T(1e8)); }
            else { inf[INFO_LSK] = k; inf[INFO_LSA] = al * T(0.5); }
        } else {
            if (!last_ls) {     // still searching: the host polls the counter to stop the backtracking early
                const int p = atomicAdd(a.n_pending, 1);
                if (list_out) list_out[p] = b;
            }
            if (last_ls) {   // no progress: damp the next LQ solve
                a.lsdone[b] = 1;
                reg[b] = fmin(fmax(regb * T(100), T(1e-6)), T(1e8));
                ((T*)a.info)[(size_t)b * INFO_N + INFO_LSK] = T(0);
            }
        }
    }
}

// adaptive backtracking: the problems still searching after the first trial are a small minority -> they stand still this
// iteration and retry their (recomputed, identical) direction at the halved length in the next one
template <typename T>
__global__ __launch_bounds__(256) void solver_defer_kernel(SolverArgs a) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.B || a.lsdone[b]) return;
    T* inf = (T*)a.info + (size_t)b * INFO_N;
    T* reg = (T*)a.reg;
    const T k = inf[INFO_LSK] + T(1);
    a.lsdone[b] = 1;
    if (k >= (T)a.max_ls) { inf[INFO_LSK] = T(0); reg[b] = fmin(fmax(reg[b] * T(100), T(1e-6)), T(1e8)); }
    else { inf[INFO_LSK] = k; inf[INFO_LSA] = ((const T*)a.alpha)[b]; }
}

// seq > 0 (inner-loop backtracking): the block that finishes last publishes the number of problems still searching to
// pinned host memory under that sequence number -- the host reads it there instead of copying it behind a drained stream
template <typename T>
__global__ __launch_bounds__(64) void solver_merit_kernel(SolverArgs a, const T* __restrict__ Zt, const T* __restrict__ gt,
                                                          const T* __restrict__ ft, T* __restrict__ Zcur, int last_ls,
                                                          const int* __restrict__ list_in, int* __restrict__ list_out,
                                                          int publish, int seq, int soc = 0) {
    solver_merit_body<T>(a, Zt, gt, ft, Zcur, last_ls, list_in, list_out, publish, (int)blockIdx.x, (int)threadIdx.x, a.n_active,
                         a.cur_it + 1, soc);
    if (seq > 0 && threadIdx.x == 0) {
        __threadfence();                                    // this block's list entry and count are out
        const int t = atomicAdd(a.n_done, 1);
        if (t == (int)gridDim.x - 1) {
            __threadfence();
            const int v = atomicAdd(a.n_pending, 0);
            *a.n_done = 0;
            a.hpub[5] = v;
            __threadfence_system();
            a.hpub[4] = seq;
            __threadfence_system();
        }
    }
}

// Next trial point of the problems still searching (inner-loop backtracking), gathered densely in the order of `list`
// together with their initial states and per-problem extras: the trial evaluation then runs over those problems only
// (a trial over the whole active batch cost the same whether one problem or all of them were still searching)
template <typename T>
__global__ __launch_bounds__(64) void solver_trial_list_kernel(int n, int nx, int ex_per, const int* __restrict__ list,
                                                               const T* __restrict__ Z, const T* __restrict__ dz,
                                                               const T* __restrict__ alpha, const T* __restrict__ X0,
                                                               const T* __restrict__ ex, T* __restrict__ Zt,
                                                               T* __restrict__ X0p, T* __restrict__ exp_,
                                                               int* __restrict__ n_pending) {
    const int slot = blockIdx.x, lane = threadIdx.x;
    if (slot == 0 && lane == 0) *n_pending = 0;         // counter of the problems still searching after this trial
    const int b = list[slot];
    const T al = alpha[b];
    for (int i = lane; i < n; i += 64) Zt[(size_t)slot * n + i] = fma(al, dz[(size_t)b * n + i], Z[(size_t)b * n + i]);
    for (int i = lane; i < nx; i += 64) X0p[(size_t)slot * nx + i] = X0[(size_t)b * nx + i];
    for (int i = lane; i < ex_per; i += 64) exp_[(size_t)slot * ex_per + i] = ex[(size_t)b * ex_per + i];
}

// Second-order correction against the Maratos effect (inner-loop backtracking).  A full SQP step along a curved constraint
// manifold leaves defects c+ = c(z + alpha d) of second order in |d|; times the l1 merit's penalty (which tracks multipliers of
// order 250 - 700 at configs[2] dims) they outweigh the decrease of the objective and the step is cut to a few per cent for
// dozens of iterations (DESIGN "Batched solver", tools/c3_slow_trace.py).  The correction removes them to first order with the
// Jacobian of the ITERATE, which is already in hand: states only, dx_t = A_t dx_{t-1} + c+_t (dx_{-1} = 0: x0 is data) --
// a particular solution of  A delta = -c+  of the size of c+ itself -- one forward recursion per rejected problem, a wave each.
// The corrected points of the problems on `list` go to Zs densely (with their x0 / extras, like solver_trial_list_kernel),
// one defect-only row launch evaluates them, and the acceptance test takes them at the rejected trial's step length.  A
// corrected state that leaves its bounds makes the barrier term NaN and is rejected by the test itself.
template <typename T>
__global__ __launch_bounds__(64) void solver_soc_kernel(int n, int nx, int nu, int H, int m, int ex_per, const int* __restrict__ list,
                                                        const T* __restrict__ Zt, const T* __restrict__ gt,
                                                        const T* __restrict__ tiles, const T* __restrict__ X0,
                                                        const T* __restrict__ ex, T* __restrict__ Zs, T* __restrict__ X0p,
                                                        T* __restrict__ exp_, int* __restrict__ n_pending) {
    // dynamic LDS: dx_{t-1} and dx_t, 2 nx elements (soc_correct_row, solver_soc_impl.h: any nx, a lane walks the states
    // lane, lane + 64, ...)
    extern __shared__ __attribute__((aligned(16))) unsigned char soc_lds_raw[];
    const int slot = blockIdx.x, lane = threadIdx.x;
    if (slot == 0 && lane == 0) *n_pending = 0;
    const int b = list[slot];
    // (the rejected trial ran over every active problem: slot == problem)
    soc_correct_row<T>(lane, 64, [] { __syncthreads(); }, nx, nu, H, Zt + (size_t)b * n, gt + (size_t)b * m,
                       tiles + (size_t)b * H * nx * (nx + nu), Zs + (size_t)slot * n, reinterpret_cast<T*>(soc_lds_raw));
    for (int i = lane; i < nx; i += 64) X0p[(size_t)slot * nx + i] = X0[(size_t)b * nx + i];
    for (int i = lane; i < ex_per; i += 64) exp_[(size_t)slot * ex_per + i] = ex[(size_t)b * ex_per + i];
}

}  // namespace

}  // namespace nempc
