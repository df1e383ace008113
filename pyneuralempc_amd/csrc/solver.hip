// Batched on-device NMPC solver ("a lock-step batched iteration on device over the
// banded KKT system turns evals/sec into solved-MPC/sec").  The reference solves one problem at a time with a
// CPU solver (Ipopt via cyipopt, optimizer/ipopt.py:138-195, or SciPy SLSQP, optimizer/slsqp.py:143-197);
// this is the batched counterpart that consumes the same callbacks for B problems at once.
//
// Method: SQP with the exact Lagrangian Hessian on the multiple-shooting NLP
//     min f(z)  s.t.  Phi(x_{t-1},u_t) - x_t = 0,  lb <= z <= ub      (z as in optimizer/ipopt.py:20-28)
// * Hessian = objective blocks + the per-step Lagrangian blocks sum_k lambda_{t,k} d2 Phi_k / d[x_{t-1}|u_t]^2 of
//   the Hessian callback (a pure Gauss-Newton model was tried first: with multipliers of order 10 and a tanh
//   network it needs 50-200 iterations and damped steps; the exact blocks give 5-20 full steps).  The blocks
//   couple only (x_{t-1}, u_t), so every QP is still an LQ problem in the linearised dynamics
//   dx_t = A_t dx_{t-1} + B_t du_t + g_t, solved exactly by one backward Riccati sweep and one forward sweep per
//   problem (block-tridiagonal KKT, O(H (nx+nu)^3)).  Indefinite control Hessians Quu are handled the DDP way:
//   the sweep is repeated with a larger Levenberg term (half-decade steps from 1e-3, at most lq_attempts levels per
//   iteration, tried side by side on lanes of one wave in the per-thread kernel, the first level that goes through is
//   used: a problem still indefinite then keeps its damping and sits the iteration out, so that the launch does
//   not wait for it).  Multipliers = Riccati costates of the previous step;
// * variable bounds (DomainConstraint, constraints.py:3-33): primal-dual interior point -- the multipliers of the
//   bounds are iterates with their own step length; their diagonal terms keep the LQ structure (the primal log
//   barrier of round 1 stays as an option); mu is decreased per problem once its sub-problem has converged;
// * globalisation: l1 merit f_mu + nu |g|_1 with nu tracking the Riccati costates, backtracking from the
//   fraction-to-the-boundary step -- one trial per iteration for small stages (a rejected problem stands still and
//   retries the same direction at half the length next iteration), an inner loop for matrix-core-bound ones.
// Every problem carries its own mu, nu, step length, damping and status; the batch advances in lock step, the
// unconverged problems are compacted to the front as it converges.  All arithmetic is in kernels here; the callbacks
// are the handle's own row/objective kernels.  Per iteration on the compiled small shape (2 states, 1 control, fp64), TWO
// launches: (1) the LQ kernel -- acceptance test of the previous iteration's trial point (a wave per problem, before the
// staging; the accepted point's evaluation and Lagrangian blocks are carried over as the iterate's), barrier terms while
// staging, the LQ solve parallel in time (lq_scan_problem: a lane per stage), then step norms, dual steps, convergence test,
// merit and the trial point with its multipliers by a wave per problem; (2) ONE callback launch at the trial point:
// Lagrangian blocks, defects and tiles (rowhess_coopfx_kernel with evaluation outputs).  The accept phase publishes the
// convergence counter to pinned host memory, the host stays at most two iterations ahead of the device.  Other shapes: the
// Riccati sweep (thread or wave per problem), separate evaluation / block / acceptance launches; inner-loop backtracking
// (matrix-core-bound stages) evaluates a second and later trial for the still-searching problems only.
//
// Where the code is.  This file is the host side: workspace, knobs, Solve<T> (plan_lq and the steps of an iteration) and the
// entry points.  The device code sits in headers that only this file includes, one concern each, in this order:
//     solver_args.h          INFO_* columns, SolverArgs, StepInfo, LQ_STAMP: the contract between driver and kernels
//     bounds_bind_impl.h     per-problem bounds (nempc_bind_bounds): what the binding says about one variable (shared with kernels_post / kernels_sens)
//     solver_ipm_impl.h      bounds: barrier terms, dual steps, barrier value, interior start (solver_init_kernel, solver_init_bound_kernel)
//     solver_soc_impl.h      second-order correction: the state recursion (host / device, nothing of HIP: tests/soc_check.cpp)
//     solver_merit_impl.h    convergence test, merit, trial point, acceptance, second-order correction
//     solver_lq_scan_impl.h  LQ solve parallel in time (2/1 stages)
//     solver_lq_impl.h       LQ solve, thread per problem: staging, Riccati sweep, post-pass
//     solver_lqw_impl.h      LQ solve, wave per problem
//     solver_compact_impl.h  partition / gather of the unconverged problems, scatter of the results
//     solver_roll_impl.h     rolling-window models: RollTables and the roll_* kernels
//     solver_rate_impl.h     input-rate penalty and limits (nempc_bind_rate): the rate_* kernels (index arithmetic: rate_index.h)
//     solver_rows_impl.h     linear stage inequality rows (nempc_bind_stage_rows): the rows_* kernels (index arithmetic: rows_index.h)
//     solver_aug.h           StageAug<T>: what of a solve is specific to a stage augmentation (window, rate, rows) -- workspace, bounds,
//                            start, the callbacks in augmented form, the solution handed back; host side, launches the two above
//     stage_aug.h            ... and its host arithmetic (nothing of HIP: tests/stage_aug_check.cpp): stage dimensions, window_var,
//                            the window's tables, bound slots, the objective table over the augmented stage
// The merit and bound headers come first because the LQ kernels call their bodies.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "nempc_internal.h"
#include "activations.h"
#include "kernels_obj_impl.h"
#include "solver_args.h"
#include "bounds_bind_impl.h"
#include "solver_ipm_impl.h"
#include "solver_soc_impl.h"
#include "solver_merit_impl.h"
#include "solver_lq_scan_impl.h"
#include "solver_lq_impl.h"
#include "solver_lqw_impl.h"
#include "solver_compact_impl.h"
#include "solver_roll_impl.h"
#include "solver_rate_impl.h"
#include "solver_rows_impl.h"
#include "solver_aug.h"

namespace nempc {

namespace {

struct SolverWs {
    AugWs aug;                                // what a stage augmentation keeps (solver_aug.h); aug.kind: the one the buffers were sized for
    void *Zt = nullptr, *f = nullptr, *ft = nullptr, *grad = nullptr, *g = nullptr, *gt = nullptr, *tiles = nullptr;
    void *tiles_t = nullptr, *grad_t = nullptr;     // trial point's tiles and objective gradient (carried over on acceptance)
    void *lam_t = nullptr, *hblk_t = nullptr;       // ... its multipliers and Lagrangian blocks (blocks + evaluation in one launch)
    void *X0p = nullptr, *exp_ = nullptr;           // initial states / extras of the problems still backtracking, dense
    void *Zsoc = nullptr, *gsoc = nullptr;          // second-order-correction trial points and their defects, dense
    int* pend[2] = {nullptr, nullptr};              // ... and their indices (two lists: one read, one appended to)
    // (cap,n) effective bounds per problem: allocated by the first solve of this workspace that has bounds bound
    // (nempc_bind_bounds), so a handle that never binds any does not carry them
    void *lbw = nullptr, *ubw = nullptr;
    void *lb = nullptr, *ub = nullptr, *alpha = nullptr, *phi0 = nullptr, *dir = nullptr, *hblk = nullptr, *lamn = nullptr,
         *sig = nullptr, *dz = nullptr, *Kst = nullptr, *kst = nullptr, *Pst = nullptr, *pst = nullptr,
         *tmp = nullptr;   // (info lives in infoc: it is read across iterations)
    int *lsdone = nullptr, *n_active = nullptr;
    // state that lives across iterations, in two buffer sets (compaction gathers from one into the other)
    void *Zc[2] = {nullptr, nullptr}, *X0c[2] = {nullptr, nullptr}, *lamc[2] = {nullptr, nullptr}, *muc[2] = {nullptr, nullptr},
         *nuc[2] = {nullptr, nullptr}, *regc[2] = {nullptr, nullptr}, *exc[2] = {nullptr, nullptr}, *infoc[2] = {nullptr, nullptr},
         *zlc[2] = {nullptr, nullptr}, *zuc[2] = {nullptr, nullptr};
    void *dzl = nullptr, *dzu = nullptr, *alz = nullptr, *bh = nullptr;
    int *stc[2] = {nullptr, nullptr}, *orig[2] = {nullptr, nullptr}, *itc[2] = {nullptr, nullptr};
    int *perm = nullptr, *count = nullptr;
    int* hpoll = nullptr;                      // pinned host: [0] convergence counter (blocking polls), [2] backtracking poll
    int *hpub = nullptr, *hpub_dev = nullptr;  // pinned host memory the device publishes the convergence counter to
    int cap = 0;                              // problems the buffers hold; 0 until every allocation has succeeded
    int m = 0, n = 0;                         // row / variable counts the buffers were sized for (box rows change m)
    size_t ex_per = 0;
    std::vector<unsigned char> bounds_host;   // the bounds as last uploaded (lb | ub in the handle's dtype)

    // The workspace owns its memory: every buffer above comes from alloc(), which records what it hands out, and
    // release() walks the records.  A pointer is recorded once its allocation has succeeded, so a failure part-way leaves
    // a workspace that the next release frees completely.  Buffers stay allocations of their own.
    std::vector<void*> dev_allocs, host_allocs;
    int alloc(void** p, size_t bytes, int host_flags = -1) {     // device memory, or pinned host memory with these flags
        NEMPC_HIP(host_flags < 0 ? hipMalloc(p, bytes ? bytes : 16)      // (an empty array still has an address of its own)
                                 : hipHostMalloc(p, bytes, (unsigned)host_flags));
        (host_flags < 0 ? dev_allocs : host_allocs).push_back(*p);
        return NEMPC_OK;
    }
    void release() {
        for (void* p : dev_allocs) (void)hipFree(p);
        for (void* p : host_allocs) (void)hipHostFree(p);
    }
};

// polite busy-wait on a word the device writes (the waits are microseconds: no yield, no sleep)
inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#endif
}

int lq_tmp_elems(int nx, int nu) { return 3 * nx * nx + 3 * nx * nu + nu * nu + 5 * nx + 3 * nu + 1 + (nx + 1) * nu; }

}  // namespace

void solver_free(Handle& h) {
    SolverWs* w = static_cast<SolverWs*>(h.solver_ws);
    if (w) w->release();
    delete w;
    h.solver_ws = nullptr;
}

namespace {
// the handle's extras binding is pointed at the compacted copy while the solve runs; put back on every exit path
struct ExtraBindingGuard {
    Handle& h; const void* saved; int saved_B;
    explicit ExtraBindingGuard(Handle& hh) : h(hh), saved(hh.d_extra), saved_B(hh.extra_B) {}
    ~ExtraBindingGuard() { h.d_extra = saved; h.extra_B = saved_B; }
};

// The solver's environment knobs (README "Environment switches"), read where declared: ProcessKnobs once per process and dtype
// (the function-local static of Solve<T>::read_knobs), what SolverKnobs adds on every solve (tests flip these in one process).
struct ProcessKnobs {
    int lq_attempts = env_int("NEMPC_LQ_ATTEMPTS", 0);   // A/B knob (counts when positive)
    int lq_scan = env_int("NEMPC_LQ_SCAN", 1);   // A/B knob
    double slack_eps = env_double("NEMPC_SOLVER_SLACK_EPS", 0.0);
    // NEMPC_SOLVER_NONMONO: 0 monotone Armijo test (rounds 1-3), 1 .. 4 merit values of previous iterates the test may
    // refer to (default 4).  configs[2] dims, B = 1024, converged after 40 / 60 / 80 / 160 iterations
    // (profiles/r04_solver_nonmonotone.txt): 664 / 825 / 918 / 1008 monotone, 722 / 854 / 932 / 1014 (1), 747 / 881 / 966 /
    // 1020 (2), 766 / 906 / 974 / 1019 (3), 775 / 924 / 985 / 1021 (4); C2 dims 965 / 979 / 997 / 1015 -> 968 / 994 / 1011 / 1019
    int nonmono = env_int("NEMPC_SOLVER_NONMONO", 4);
    // The Levenberg term moves in half decades (round 5).  In whole decades -- x 10 when a sweep meets a pivot that is not
    // positive, x 0.1 after a clean one -- a problem whose reduced Hessian needs a term of, say, 2 alternates between 1
    // (fails, retried) and 10: it is damped five times harder than it has to be, and the slow problems of configs[2]'s dims
    // crawled through a dozen iterations of 4e-2 steps that way (tools/c3_slow_trace.py).  sqrt(10) each way: converged
    // after 40 / 60 / 80 iterations 994 / 1024 / 1024 of 1024 instead of 847 / 990 / 1021, the last problem through in
    // 81 ms instead of 123; C2 dims unchanged (968 / 991 / 1010 / 1021 against 968 / 993 / 1010 / 1019);
    // profiles/r05_solver_reg_steps.txt.  NEMPC_SOLVER_REG_RAISE / _RELAX are the A/B knobs.
    double reg_relax = env_double("NEMPC_SOLVER_REG_RELAX", 0.31622776601683794);
    double reg_raise = env_double("NEMPC_SOLVER_REG_RAISE", 3.1622776601683795);
    bool stats = env_set("NEMPC_SOLVER_STATS");   // Riccati restarts per iteration (diagnostic, synchronises)
    int trace_slot = env_int("NEMPC_SOLVER_TRACE", -1);   // one line per iteration for that slot (diagnostic, synchronises)
};
struct SolverKnobs : ProcessKnobs {
    int lq_spec = env_int("NEMPC_LQ_SPEC", 0);   // A/B knob (tests)
    int no_fuse_step = env_int("NEMPC_SOLVER_NO_FUSE_STEP", 0);   // (tests)
    int no_carry = env_int("NEMPC_SOLVER_NO_CARRY", 0);   // A/B knob (tests)
    int hess_trial = env_int("NEMPC_SOLVER_HESS_TRIAL", 1);   // A/B knob (tests)
    int fuse_accept = env_int("NEMPC_SOLVER_FUSE_ACCEPT", 1);   // A/B knob (tests)
    bool soc = env_enabled("NEMPC_SOLVER_SOC");      // (read per solve)
};

// One solve: handle, workspace, options, knobs, dimensions, what plan_lq decides, the kernels' arguments and the state the
// iteration carries from one step to the next.  run() is the algorithm; the members behind it are its steps.
template <typename T>
struct Solve {
    Handle& h; SolverWs& ws; const nempc_solver_opts& o; const int B; const void* const X0; const hipStream_t s;
    const SolverDuals duals;      // where the multipliers of the returned iterates go (nempc_solve_duals; all null: nowhere)
    // rolling-window models and rate bindings run as a plain problem in an augmented state (solver_aug.h): H, nx, nu, nin, n, m are
    // the SOLVER's stage dimensions
    StageAug<T> aug; const bool augmented;
    const int H, nu, nx, nin, n, m;
    const size_t ex_per; const unsigned gBn;      // grid of the element-wise kernels over the solver's variables
    const SolverKnobs kn = read_knobs();
    ExtraBindingGuard extra_guard; SolverArgs a{}; bool has_bounds = false;
    // plan_lq decides (besides fields of `a`): the kernel; stages wide enough to spread over a wave (matrix-core-bound
    // iterations); LDS elements per problem (odd); LDS of a workgroup: the problems' blocks + one copy of the bounds (2 n)
    void (*lqk)(SolverArgs) = nullptr; bool wave_wanted = false; int per_problem = 0; size_t wg_extra = 0, lds_budget = 0;
    volatile int* hp = nullptr;   // the words the device publishes (SolverArgs::hpub)
    int cur = 0;                  // buffer set of the working copies
    int Bact;                     // slots [0, Bact) may still be unconverged; compaction keeps them in front
    int last_nact;                // unconverged problems at the last convergence poll
    int it = 0, nact = -1;        // nact: unconverged problems as this iteration's poll has them (-1: it did not poll)
    bool finished = false;        // ... and the poll found none left (`it` is then the iteration at which that happened)
    int pend_seq = 0;             // sequence number of the inner loop's acceptance launches (published with their count)
    bool carry = false;           // deferred backtracking on a compiled shape: a trial evaluation is a full one, kept on acceptance
    bool hess_trial = false;      // ... with the trial point's Lagrangian blocks from the launch that evaluates it
    bool have_eval = false;       // the evaluation buffers hold every active problem's current iterate
    bool have_blocks = false;     // ... and so does the block buffer
    bool accept_pending = false;  // the last trial point has been evaluated, its acceptance test has not been launched
    bool published_polls = false, trace = false, compact = false;
    bool bound_rows = false;      // per-problem bounds are bound: every kernel reads the problem's row of the working copy
    bool tracking = false;        // per-problem tracking data are bound: no launch that fuses the shared objective; f and grad from
                                  // the binding's kernel at the iterate and from the acceptance test at a trial point
    static SolverKnobs read_knobs() { static const ProcessKnobs once; return SolverKnobs{once}; }
    static SolverWs& workspace(Handle& h) { return *static_cast<SolverWs*>(h.solver_ws ? h.solver_ws : (h.solver_ws = new SolverWs())); }
    Solve(Handle& hh, int BB, const void* X0_, const nempc_solver_opts& oo, const SolverDuals& dd, hipStream_t ss)
        : h(hh), ws(workspace(hh)), o(oo), B(BB), X0(X0_), s(ss), duals(dd),
          aug(hh, ws.aug, BB, ss), augmented(aug.on()), H(h.cfg.H), nu(h.cfg.nu), nx(aug.d.nx), nin(aug.d.nin), n(aug.d.n),
          m(augmented ? aug.d.m : h.m),      // (plain: the handle's rows, box rows included)
          ex_per((size_t)H * h.ne), gBn((unsigned)(((size_t)BB * std::max(n, std::max(m, nx)) + 255) / 256)),
          extra_guard(hh), Bact(BB), last_nact(BB) {}
    int run(void* Z, const double* lb, const double* ub, int32_t* status_dev, int32_t* iters_host) {
        int rc;
        if ((rc = ensure_workspace()) || (rc = upload_bounds(lb, ub)) || (rc = start(Z))) return rc;
        for (; it < o.max_iter; ++it) {
            a.B = Bact; a.cur_it = it; nact = -1;
            if ((rc = evaluate_iterate())) return rc;       // defects, tiles, f, gradient, Lagrangian blocks
            launch_lq();                                    // [acceptance of the last trial,] LQ solve, step, first trial point
            if (!published_polls && (rc = poll_blocking())) return rc;
            if (!finished && (rc = line_search())) return rc;            // trial evaluation(s) and their acceptance test
            if (!finished && published_polls && (rc = poll_published())) return rc;
            if (finished) break;            // (`it` is the iteration at which the last problem converged)
            if ((rc = diagnostics())) return rc;
            // once a quarter of the active slots has finished, shrink every launch to the unconverged problems
            if (compact && nact >= 0 && nact < Bact - Bact / 4 && Bact > 64 && (rc = compact_batch())) return rc;
        }
        return finish(Z, status_dev, iters_host);
    }
    // a workspace that holds B problems of these dimensions: kept when the handle has one, rebuilt otherwise
    int ensure_workspace() {
        if (ws.cap >= B && ws.ex_per == ex_per && ws.m == m && ws.n == n && ws.aug.kind == aug.kind) return NEMPC_OK;
        ws.release(); ws = SolverWs();
        SolverWs& w = ws;
        const size_t e = sizeof(T), Bn = (size_t)B;
        std::vector<BufReq> al = {
            {&w.Zt, Bn * n * e}, {&w.f, Bn * e}, {&w.ft, Bn * e}, {&w.grad, Bn * n * e}, {&w.g, Bn * m * e},
            {&w.gt, Bn * m * e}, {&w.tiles, Bn * H * nx * nin * e}, {&w.lb, (size_t)n * e}, {&w.ub, (size_t)n * e},
            {&w.alpha, Bn * e}, {&w.phi0, Bn * e},
            {&w.dir, Bn * e}, {&w.hblk, Bn * H * nin * nin * e}, {&w.lamn, Bn * m * e},
            {&w.sig, Bn * e}, {&w.dz, Bn * n * e}, {&w.Kst, Bn * H * nu * nx * e},
            {&w.kst, Bn * H * nu * e}, {&w.Pst, Bn * H * nx * nx * e}, {&w.pst, Bn * H * nx * e},
            {&w.tmp, Bn * lq_tmp_elems(nx, nu) * e}, {&w.dzl, Bn * n * e}, {&w.dzu, Bn * n * e}, {&w.alz, Bn * e},
            {&w.bh, Bn * n * e}, {&w.tiles_t, Bn * H * nx * nin * e}, {&w.grad_t, Bn * n * e},
            {&w.X0p, Bn * nx * e}, {&w.exp_, Bn * ex_per * e}, {&w.lam_t, Bn * m * e}, {&w.hblk_t, Bn * H * nin * nin * e},
            {&w.Zsoc, Bn * n * e}, {&w.gsoc, Bn * m * e}};
        for (int k = 0; k < 2; ++k)
            al.insert(al.end(), {
                {&w.Zc[k], Bn * n * e}, {&w.X0c[k], Bn * nx * e}, {&w.lamc[k], Bn * m * e}, {&w.muc[k], Bn * e},
                {&w.nuc[k], Bn * e}, {&w.regc[k], Bn * e}, {&w.exc[k], Bn * ex_per * e}, {&w.infoc[k], Bn * INFO_N * e},
                {&w.zlc[k], Bn * n * e}, {&w.zuc[k], Bn * n * e},
                {(void**)&w.stc[k], Bn * sizeof(int)}, {(void**)&w.orig[k], Bn * sizeof(int)},
                {(void**)&w.itc[k], Bn * sizeof(int)}});
        al.insert(al.end(), {{(void**)&w.lsdone, Bn * sizeof(int)}, {(void**)&w.pend[0], Bn * sizeof(int)},
                             {(void**)&w.pend[1], Bn * sizeof(int)},
                             {(void**)&w.n_active, 8 * sizeof(int)},   // [unconverged, still backtracking, blocks done, -, unconverged (odd iterations)]
                             {(void**)&w.perm, Bn * sizeof(int)}, {(void**)&w.count, sizeof(int)}});
        aug.buffers(al);
        for (const BufReq& x : al) if (int rc = w.alloc(x.p, x.bytes)) return rc;
        NEMPC_HIP(hipMemset(w.n_active, 0, 8 * sizeof(int)));
        if (int rc = w.alloc((void**)&w.hpoll, 4 * sizeof(int), hipHostMallocDefault)) return rc;
        if (int rc = w.alloc((void**)&w.hpub, 8 * sizeof(int), hipHostMallocMapped)) return rc;
        NEMPC_HIP(hipHostGetDevicePointer((void**)&w.hpub_dev, w.hpub, 0));
        if (int rc = aug.upload_tables()) return rc;
        w.cap = B; w.m = m; w.n = n; w.ex_per = ex_per;
        return NEMPC_OK;
    }
    // bounds -> device (dtype T); +-inf become +-max so that comparisons stay exact.  Box ROWS on the states
    // (nempc_set_box_rows; a Constraint's rows in the reference's glue, optimizer/ipopt.py:44-52) are bounds on the
    // state variables for this solver: intersected here, what controller.py:101-105 of this package does on the host.
    int upload_bounds(const double* lb, const double* ub) {
        const T big = std::numeric_limits<T>::max();
        std::vector<T> hl(n, -big), hu(n, big);      // (augmented: a slot that is nobody's carries no bound -- the copies inside a
                                                     //  window state)
        std::vector<double> blo, bhi;
        if (int rc = intersect_bounds(h, lb, ub, true, "nempc_solve", blo, bhi)) return rc;
        aug.append_bounds(blo, bhi);                 // (rate: the limits, behind the caller's bounds)
        for (size_t i = 0; i < blo.size(); ++i) {
            const double lo = blo[i], hi = bhi[i];
            const int k = ws.aug.bslot[i];
            hl[k] = std::isfinite(lo) ? (T)lo : -big;
            hu[k] = std::isfinite(hi) ? (T)hi : big;
            has_bounds = has_bounds || std::isfinite(lo) || std::isfinite(hi);
        }
        // per-problem bounds live on the device: whether a problem has a finite bound is decided there, per problem
        // (solver_init_bound_kernel: mu = 0 for one that has none); the host plans for the barrier
        bound_rows = h.bbind.on();
        has_bounds = has_bounds || bound_rows;
        // (an MPC loop solves with the same bounds every step: they are uploaded when they change)
        const size_t nb = (size_t)n * sizeof(T);
        if (ws.bounds_host.size() != 2 * nb || memcmp(ws.bounds_host.data(), hl.data(), nb) != 0 ||
            memcmp(ws.bounds_host.data() + nb, hu.data(), nb) != 0) {
            NEMPC_HIP(hipMemcpyAsync(ws.lb, hl.data(), nb, hipMemcpyHostToDevice, s));
            NEMPC_HIP(hipMemcpyAsync(ws.ub, hu.data(), nb, hipMemcpyHostToDevice, s));
            NEMPC_HIP(hipStreamSynchronize(s));   // hl / hu are stack-owned
            ws.bounds_host.resize(2 * nb);
            memcpy(ws.bounds_host.data(), hl.data(), nb);
            memcpy(ws.bounds_host.data() + nb, hu.data(), nb);
        }
        return NEMPC_OK;
    }
    int max_ppw() const { return (int)(lds_budget / ((size_t)per_problem * sizeof(T))); }
    size_t lds_bytes(int ppw) const { return (size_t)ppw * per_problem * sizeof(T) + wg_extra; }
    int pick_ppw(int nb) const {
        int ppw = std::min(max_ppw(), 16);
        if (ppw * a.spec > 64) ppw = 64 / a.spec;       // the sweeping lanes are one wave
        // the sweep is one latency chain per lane whatever the number of active lanes: spread the batch over the CUs
        const int spread = (nb + h.num_cus - 1) / h.num_cus;
        if (ppw > spread) ppw = spread < 1 ? 1 : spread;
        // the wave-per-problem kernel runs one problem per wave of a 256-thread workgroup
        if (wave_wanted && ppw > 4) ppw = 4;
        return ppw;
    }
    // the LQ solve of this shape: attempts and damping levels, LDS layout, problems per workgroup, the kernel
    int plan_lq() {
        a.lq_attempts = o.lq_attempts > 0 ? o.lq_attempts : (kn.lq_attempts > 0 ? kn.lq_attempts : 3);
        wave_wanted = o.lq_kernel != 1 && (o.lq_kernel == 2 || nx * (nx + nu) >= 12);
        // thread-per-problem sweep: up to three damping levels side by side (lanes and LDS regions per problem)
        a.spec = wave_wanted ? 1 : std::max(1, std::min(std::min(a.lq_attempts, kn.lq_spec > 0 ? kn.lq_spec : 3), 8));
        a.att_elems = H * nu * nx + H * nu + H * nx * nx + H * nx + lq_tmp_elems(nx, nu);
        // parallel-in-time solve (lq_scan_problem): 2/1 stages in double, a stage per lane
        const bool scan_fits = sizeof(T) == 8 && nx == 2 && nu == 1 && H + 1 <= 64;
        if (o.lq_kernel == 3 && !scan_fits) {
            set_error("nempc_solve: lq_kernel = 3 (scan) is built for 2-state / 1-control stages in fp64 with H <= 63");
            return NEMPC_EUNSUPPORTED;
        }
        const bool lq_scan = scan_fits && (o.lq_kernel == 3 || (o.lq_kernel == 0 && kn.lq_scan != 0));
        if (lq_scan) {
            a.spec = std::max(1, std::min(a.lq_attempts, 64 / (H + 1)));     // levels side by side: lane segments of H + 1
            a.att_elems = 0;                                                    // (no per-attempt region: the scan lives in registers)
        }
        wg_extra = (size_t)2 * n * sizeof(T);
        lds_budget = kLqLdsBudget > wg_extra ? kLqLdsBudget - wg_extra : 0;
        for (;; --a.spec) {
            per_problem = 2 * n + 2 * H * nx + H * nx * nin + H * nin * nin + n + n + H * nx + 2 * n + a.spec * a.att_elems;
            per_problem |= 1;   // odd stride: the ppw lanes of a sweep hit different LDS banks
            if (a.spec == 1 || (size_t)per_problem * sizeof(T) <= lds_budget) break;   // (levels one after the other if not)
        }
        a.ppw = pick_ppw(B);
        a.use_lds = a.ppw >= 1;
        a.lds_stride = per_problem;
        lqk = a.use_lds ? ((nx == 2 && nu == 1) ? solver_lq_kernel<T, 2, 1, true>
                                                      : ((nx == 6 && nu == 3) ? solver_lq_kernel<T, 6, 3, true> : solver_lq_kernel<T, 0, 0, true>))
                             : ((nx == 2 && nu == 1) ? solver_lq_kernel<T, 2, 1, false>
                                                      : ((nx == 6 && nu == 3) ? solver_lq_kernel<T, 6, 3, false> : solver_lq_kernel<T, 0, 0, false>));
        // wave-per-problem sweep when the working set is staged in LDS and a stage has enough entries to spread over a
        // wave: 6/3 stages 6.5 k vs 5.0 k MPC solves/s at C3; 2/1 stages are 4 entries wide and stay on the
        // thread-per-problem kernel (22.0 vs 23.1 ms per 40 iterations at C2).  nempc_solver_opts.lq_kernel forces one.
        const bool lq_wave = a.use_lds && wave_wanted;
        a.fuse_step = a.use_lds && !lq_wave && !kn.no_fuse_step;
        a.f_it = ws.f; a.Zt_it = ws.Zt;
        if (a.fuse_step) NEMPC_HIP(hipMemsetAsync(ws.n_active, 0, 8 * sizeof(int), s));
        if (lq_wave)
            lqk = (nx == 2 && nu == 1) ? solver_lqw_kernel<T, 2, 1>
                                            : ((nx == 6 && nu == 3) ? solver_lqw_kernel<T, 6, 3> : solver_lqw_kernel<T, 0, 0>);
        if constexpr (sizeof(T) == 8)
            if (lq_scan && a.use_lds && !lq_wave) lqk = solver_lq_kernel<T, 2, 1, true, true>;
        // what ran, for nempc_last_lq_kernel: a forced wave (or scan) kernel whose working set does not fit is plan 1
        h.last_lq_kernel = !a.use_lds ? LQ_THREAD_GLOBAL : (lq_wave ? LQ_WAVE_LDS : (sizeof(T) == 8 && lq_scan ? LQ_SCAN : LQ_THREAD_LDS));
        const size_t lds_max = a.use_lds ? lds_bytes(std::min(std::max(max_ppw(), 1), 16)) : 0;
        NEMPC_HIP(ensure_dynamic_lds(reinterpret_cast<const void*>(lqk), lds_max));
        return NEMPC_OK;
    }
    void point_at(int k) {
        a.Z = ws.Zc[k]; a.lam = ws.lamc[k]; a.mu = ws.muc[k]; a.pen = ws.nuc[k]; a.reg = ws.regc[k];
        a.status = ws.stc[k]; a.iters_done = ws.itc[k]; a.info = ws.infoc[k]; a.zl = ws.zlc[k]; a.zu = ws.zuc[k];
        if (ex_per) h.d_extra = ws.exc[k];
        a.trk_prob = ws.orig[k];
    }
    // ---- working copies in buffer set 0 (the caller's Z / status are written once, at the end, in the caller's order), the
    //      kernels' arguments, the LQ plan and the routes this solve takes
    int start(const void* Z) {
        int rc;
        if (ex_per) {
            NEMPC_HIP(hipMemcpyAsync(ws.exc[0], h.d_extra, (size_t)B * ex_per * sizeof(T), hipMemcpyDeviceToDevice, s));
            h.d_extra = ws.exc[0];
            h.extra_B = B;
        }
        const void *Zstart = Z, *X0start = X0, *obj_dev = h.d_obj.get();
        if (augmented) {
            if ((rc = aug.start(Z, X0, ws.lb, ws.ub, (T)o.mu_init, has_bounds ? 1 : 0, gBn))) return rc;
            Zstart = ws.aug.rZin; X0start = ws.aug.rS0; obj_dev = ws.aug.robj;
            aug.f = ws.f; aug.g = ws.g; aug.gt = ws.gt; aug.tiles = ws.tiles; aug.hblk = ws.hblk; aug.grad = ws.grad;
        }
        if (bound_rows && !ws.lbw) {     // (a rebuilt workspace starts without them; sized like its other buffers)
            const size_t nb = (size_t)ws.cap * n * sizeof(T);
            if ((rc = ws.alloc(&ws.lbw, nb)) || (rc = ws.alloc(&ws.ubw, nb))) return rc;
        }
        if (bound_rows)     // (plain models only, nempc_solve_duals: n, nx, m are the caller's)
            hipLaunchKernelGGL(solver_init_bound_kernel<T>, dim3(B), dim3(256), 0, s, B, n, H * nx, h.bbind, (const T*)ws.lb,
                               (const T*)ws.ub, (T*)ws.lbw, (T*)ws.ubw, (T*)ws.Zc[0], (T*)ws.muc[0], (T*)ws.nuc[0],
                               (T*)ws.regc[0], ws.stc[0], ws.orig[0], ws.itc[0], (T*)ws.infoc[0], (T*)ws.zlc[0], (T*)ws.zuc[0],
                               (T)o.mu_init, (T)o.reg, (const T*)Zstart, (const T*)X0start, (T*)ws.X0c[0], nx, (T*)ws.lamc[0], m);
        else
        hipLaunchKernelGGL(solver_init_kernel<T>, dim3(gBn), dim3(256), 0, s, B, n, (T*)ws.Zc[0], (const T*)ws.lb,
                           (const T*)ws.ub, (T*)ws.muc[0], (T*)ws.nuc[0], (T*)ws.regc[0], ws.stc[0], ws.orig[0], ws.itc[0],
                           (T*)ws.infoc[0], (T*)ws.zlc[0], (T*)ws.zuc[0], (T)o.mu_init, (T)o.reg, has_bounds ? 1 : 0,
                           (const T*)Zstart, (const T*)X0start, (T*)ws.X0c[0], nx, (T*)ws.lamc[0], m);
        a.H = H; a.nx = nx; a.nu = nu; a.nin = nin; a.n = n; a.m = m;
        a.grad = ws.grad; a.g = ws.g; a.tiles = ws.tiles;
        a.hblk = ws.hblk; a.lamn = ws.lamn;
        a.obj = obj_dev; a.oo = obj_offsets(H, nx, nu);
        tracking = h.track.on();
        a.trk = tracking ? h.track : TrackBind{};
        a.lb = bound_rows ? ws.lbw : ws.lb; a.ub = bound_rows ? ws.ubw : ws.ub; a.bstride = bound_rows ? n : 0;
        a.alpha = ws.alpha; a.phi0 = ws.phi0;
        a.dir = ws.dir; a.lsdone = ws.lsdone; a.n_active = ws.n_active; a.n_pending = ws.n_active + 1; a.n_done = ws.n_active + 2;
        a.dz = ws.dz; a.Kst = ws.Kst;
        a.dzl = ws.dzl; a.dzu = ws.dzu; a.alz = ws.alz; a.bh = ws.bh;
        a.primal_dual = (has_bounds && o.barrier != 1) ? 1 : 0; a.kst = ws.kst; a.Pst = ws.Pst; a.pst = ws.pst;
        a.tmp = ws.tmp; a.tmp_stride = (size_t)B;
        point_at(0);
        if ((rc = plan_lq())) return rc;
        a.tol_g = o.tol_constraint; a.tol_step = o.tol_step; a.mu_min = has_bounds ? o.mu_min : 0.0; a.mu_factor = o.mu_factor;
        a.armijo_slack = std::max(1e-12, kn.slack_eps * (double)std::numeric_limits<T>::epsilon());
        a.max_ls = o.max_linesearch;
        a.nonmono = kn.nonmono < 0 ? 0 : (kn.nonmono > 4 ? 4 : kn.nonmono);
        // Piecewise-linear networks (relu, leaky_relu, relu6) have no second-order constraint violation for the relaxed test
        // to forgive; what it does there is let an iterate chatter across a kink without its step ever shrinking.  A
        // network with such a layer keeps the monotone test.
        for (int l = 0; l < h.nl; ++l)
            if (act_is_piecewise_linear(h.act[l])) a.nonmono = 0;
        a.reg_relax = kn.reg_relax > 0.0 && kn.reg_relax < 1.0 ? kn.reg_relax : 0.31622776601683794;
        a.reg_raise = kn.reg_raise > 1.0 && kn.reg_raise <= 100.0 ? kn.reg_raise : 3.1622776601683795;
        const int lsm_carry = o.linesearch == 0 ? (wave_wanted ? 1 : 2) : o.linesearch;
        carry = lsm_carry == 2 && !kn.no_carry && a.use_lds && h.variant == NEMPC_KERNEL_MFMA && h.cfg.integrator != NEMPC_RK4 &&
                !augmented;
        // the trial point's Lagrangian blocks from the launch that evaluates it (compiled shape): an iteration is then the LQ
        // solve, ONE callback launch and the acceptance test
        hess_trial = carry && a.fuse_step && kn.hess_trial != 0;
        a.carry = 0; a.tiles_t = ws.tiles_t; a.grad_t = ws.grad_t; a.lam_t = nullptr; a.hblk_t = nullptr;
        // the acceptance test inside the next iteration's LQ kernel (see SolverArgs::accept_first): two launches per iteration
        a.accept_first = 0; a.n_active_prev = ws.n_active; a.gt_acc = ws.gt;
        a.hpub = ws.hpub_dev; hp = ws.hpub;
        for (int k = 0; k < 8; ++k) ws.hpub[k] = 0;       // (the previous solve on this handle ended with a synchronised stream)
        published_polls = !wave_wanted;  // small stages (chains of latency-bound launches): no blocking polls, the host
                                            // reads the counter the device publishes
        trace = kn.trace_slot >= 0 && kn.trace_slot < B;
        // augmented: the callbacks read the caller's x0 / history by problem index, so the batch keeps its order (a finished
        // problem is skipped by every solver kernel; its callback rows are evaluated and ignored)
        compact = o.compact != 0 && !trace && !augmented;
        return NEMPC_OK;
    }
    // ---- callbacks.  Plain models: the handle's launches on the solver's buffers (augmented: StageAug::eval)
    int launch_rows(int nb, const void* Zs, const void* X0s, void* g, void* tiles, void* tiles_scratch) {
        return callback_rows(h, nb, Zs, X0s, g, tiles, tiles_scratch, s);
    }
    int launch_blocks(int nb, const void* Zs, const void* X0s, const void* lam, void* blocks) {
        return callback_blocks(h, nb, Zs, X0s, lam, blocks, s);
    }
    // The launches a compiled shape has, asked of the plan (mfma_plan.h) at the call's batch size (several gates depend on it):
    // blocks + defects + tiles from one launch of the Hessian kernel ...
    HessOut blocks_eval_out(void* blocks, void* g, void* tiles) const { HessOut ho; ho.blocks = blocks; ho.ev_g = g; ho.ev_tiles = tiles; return ho; }
    bool has_blocks_eval(int nb, const HessOut& ho) const {
        return h.variant != NEMPC_KERNEL_VALU && h.mfma.blob && (mfma_plan_hess(h, nb, ho).covers & COVERS_EVAL);
    }
    // ... and defects, tiles (or neither: forward passes only), f and grad from one launch of the row kernel
    RowsOut fused_eval_out(void* g, void* tiles, void* f, void* grad) const { RowsOut ro; ro.g = g; ro.tiles = tiles; ro.f = f; ro.grad = grad; return ro; }
    bool has_fused_eval(int nb, const RowsOut& ro) const {
        return h.variant != NEMPC_KERNEL_VALU && h.mfma.blob && (mfma_plan_rows(h, nb, ro).covers & COVERS_OBJ);
    }
    // (A block-wise mirrored convexification of the stage Hessians, for the problems whose sweep needed damping, was built and
    // measured in round 4 -- profiles/r04_solver_convexify_c3.txt: +3 - 5 % problems converged at 1.5 ms per iteration; removed
    // in round 5: indefiniteness is not what holds the configs[2] solves back, DESIGN "Batched solver".)
    // callbacks at the iterate: defects + tiles (row kernel), f + grad (objective kernel)
    // and the per-step Lagrangian blocks with the current multipliers (all zero on the first iterate:
    // Gauss-Newton step).  The RK4 matrix-core pipeline produces defects, tiles and blocks from one row launch.
    int evaluate_iterate() {
        void* Zc = ws.Zc[cur];
        const void *X0c = ws.X0c[cur], *lam = ws.lamc[cur];
        const bool rk4_pipeline = h.variant != NEMPC_KERNEL_VALU && h.cfg.integrator == NEMPC_RK4;
        bool fused_eval = false;
        int rc;
        if (augmented) {
            fused_eval = true;                  // (f and grad come with it)
            rc = aug.eval(Zc, lam);
        } else if (have_eval) {
            // deferred backtracking on a compiled shape: the trial evaluation of the last iteration was a full one and the
            // acceptance kernel kept, per problem, the evaluation of the point it stands on -- only the blocks are new, and
            // not even those when the trial launch computed them
            fused_eval = true;
            rc = have_blocks ? NEMPC_OK : launch_blocks(Bact, Zc, X0c, lam, ws.hblk);
        } else if (rk4_pipeline) {
            if (rk4hess_supported(h)) rc = launch_rowhess_rk4_mfma(h, Bact, Zc, X0c, lam, ws.hblk, s, ws.g, ws.tiles);
            else {
                // (a wave's slice of the congruence step does not fit the device's LDS: rows through the matrix-core entry
                //  point and the blocks from the generic kernel)
                if ((rc = launch_rows(Bact, Zc, X0c, ws.g, ws.tiles, nullptr))) return rc;
                rc = launch_rowhess_valu(h, Bact, Zc, X0c, lam, ws.hblk, s);
            }
        } else if (const HessOut ho = blocks_eval_out(ws.hblk, ws.g, ws.tiles); carry && hess_trial && has_blocks_eval(Bact, ho)) {
            // first iterate (and the one after a compaction) through the kernel the trial points go through -- the same
            // arithmetic whichever way an iterate's evaluation was obtained: blocks, defects, tiles; f and grad below
            rc = launch_rowhess_mfma(h, Bact, Zc, X0c, lam, ho, s);
        } else {
            // compiled shapes: defects, tiles, f and grad from one launch
            const RowsOut ro = fused_eval_out(ws.g, ws.tiles, ws.f, ws.grad);
            fused_eval = h.variant == NEMPC_KERNEL_MFMA && !tracking && has_fused_eval(Bact, ro);
            rc = fused_eval ? launch_rows_mfma(h, Bact, Zc, X0c, ro, s) : launch_rows(Bact, Zc, X0c, ws.g, ws.tiles, nullptr);
            if (rc) return rc;
            rc = launch_blocks(Bact, Zc, X0c, lam, ws.hblk);
        }
        if (rc) return rc;
        if (fused_eval) return NEMPC_OK;
        // (slot i of the working batch holds the caller's problem orig[i]: its own references and linear costs)
        return tracking ? launch_objective_tracking(h, Bact, Zc, ws.f, ws.grad, ws.orig[cur], s)
                        : launch_objective(h, Bact, Zc, ws.f, ws.grad, s);
    }
    void launch_lq() {
        // bounds: barrier diagonal for the LQ model, barrier gradient folded into grad
        if (!a.use_lds)
            hipLaunchKernelGGL(solver_barrier_kernel<T>, dim3((unsigned)(((size_t)Bact * n + 255) / 256)), dim3(256), 0, s, a);
        a.lam_t = carry && hess_trial ? ws.lam_t : nullptr;
        // this iteration's convergence counter; the pending acceptance (if any) publishes and clears the other word
        a.n_active = kn.fuse_accept != 0 && a.fuse_step ? ws.n_active + (it & 1) * 4 : ws.n_active;
        a.n_active_prev = ws.n_active + ((it & 1) ^ 1) * 4;
        a.accept_first = accept_pending ? 1 : 0;
        accept_pending = false;
        // LDS mode: four waves stage the working set, the first ppw lanes run the sweeps
        hipLaunchKernelGGL(lqk, dim3(a.use_lds ? (Bact + a.ppw - 1) / a.ppw : (Bact + 63) / 64), dim3(a.use_lds ? 256 : 64),
                           a.use_lds ? lds_bytes(a.ppw) : 0, s, a);
#ifdef NEMPC_LQ_STAMPS
        if (it == 3) {
            long long st[16];
            hipStreamSynchronize(s);
            hipMemcpyFromSymbol(st, HIP_SYMBOL(nempc_lq_stamps), sizeof(st));
            fprintf(stderr, "lq stamps (cycles since start):");
            for (int i = 1; i <= 9; ++i) fprintf(stderr, " %lld", st[i] - st[0]);
            fprintf(stderr, "\n");
        }
#endif
        if (!a.fuse_step)
            hipLaunchKernelGGL(solver_step_kernel<T>, dim3(Bact), dim3(64), 0, s, a, (const T*)ws.f, (const T*)ws.Zc[cur], (T*)ws.Zt);
    }
    // Convergence poll.  Matrix-core-bound stages: a blocking copy every `check` iterations (an iteration is milliseconds,
    // a drained stream costs nothing next to iterations at a stale batch size).  Small stages: poll_published, after the
    // backtracking launches.
    int poll_blocking() {
        if ((it + 1) % (o.check_every > 0 ? o.check_every : 4) != 0 && it + 1 != o.max_iter) return NEMPC_OK;
        NEMPC_HIP(hipMemcpyAsync(ws.hpoll, ws.n_active, sizeof(int), hipMemcpyDeviceToHost, s));
        NEMPC_HIP(hipStreamSynchronize(s));
        last_nact = nact = ws.hpoll[0];
        // (report the iteration at which the last problem converged, as the published counter has it, not the poll's)
        if (nact == 0) { it = ws.hpub[2] > 0 ? ws.hpub[2] : it + 1; finished = true; }
        return NEMPC_OK;
    }
    // wait until the device has published a value of hp[word] that satisfies `reached` (what, which: the error's words)
    template <typename F> int wait_published(int word, F reached, const char* what, int which) {
        const auto t0 = std::chrono::steady_clock::now();
        long spins = 0;
        while (!reached(hp[word])) {
            cpu_relax();
            if ((++spins & 0xfff) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(5)) {
                NEMPC_HIP(hipStreamSynchronize(s));      // a device fault surfaces here instead of a hang
                if (!reached(hp[word])) {
                    set_error("nempc_solve: iteration " + std::to_string(it) + ": " + what + std::to_string(which) +
                              " was never published (stream drained, word still " + std::to_string(hp[word]) + ")");
                    return NEMPC_EHIP;
                }
            }
        }
        return NEMPC_OK;
    }
    // the acceptance kernel publishes the number of problems still searching under a sequence number: wait for it
    int poll_pending(int seq, int* out) {
        const int rc = wait_published(4, [seq](int v) { return v == seq; }, "the backtracking counter of trial ", seq);
        if (!rc) *out = hp[5];
        return rc;
    }
    // Backtracking in a lock-step batch.  An inner loop makes every problem pay for the one that needs six halvings
    // (measured: 5.7 trial evaluations per iteration at B=1024, C2 dims, 70 % of the solve time).  DEFERRED (2): one
    // trial per iteration; a problem whose trial is rejected stands still and retries the same direction at half the
    // length next iteration.  ADAPTIVE (3): after the first trial, if fewer than a quarter of the active problems
    // are still searching they are deferred, otherwise the loop goes on.  auto: matrix-core-bound iterations (6/3
    // 3x128: a trial is 5 % of an iteration) keep the inner loop; small stages defer -- at equal wall time deferral
    // converges more problems at every budget measured (2/1 2x64, B=1024: 1014 converged in 24.8 ms against 1004 in
    // 24.9 ms), in the wide phase because a trial evaluation costs real time and among the stragglers because each
    // extra trial is a latency-bound launch chain plus a host poll.  It spends more ITERATIONS on a hard problem
    // (a retry is an iteration), so max_iter budgets are larger than with the inner loop.
    // (augmented: one trial per iteration whatever was asked for -- the dense trial lists of the inner loop would need the
    //  callbacks' x0 / history gathered per list)
    int line_search() {
        void* Zc = ws.Zc[cur];
        const void* X0c = ws.X0c[cur];
        const int lsm = augmented ? 2 : (o.linesearch == 0 ? (wave_wanted ? 1 : 2) : o.linesearch);
        // second-order correction of rejected full steps: inner-loop backtracking only (the deferred form accepts inside the
        // next LQ kernel); NEMPC_SOLVER_SOC=0 switches it off (A/B, tests)
        const bool soc_on = lsm != 2 && !augmented && kn.soc;
        int pending = 0, rc = NEMPC_OK;
        int pflip = 0;          // which of the two lists of searching problems is read next (the correction stage swaps them)
        const void* const extra_all = h.d_extra;      // (h.d_extra points at a dense list's extras around its launches only)
        for (int ls = 0; ls < o.max_linesearch; ++ls) {
            // the first trial point comes from solver_step_kernel (or the Riccati kernel), for every active problem; later
            // ones (inner-loop backtracking) are built here for the problems still searching ONLY, densely: their
            // evaluation and acceptance test run over `pending` problems instead of the whole active batch
            const int nb = ls > 0 ? pending : Bact;
            const void* X0t = X0c;
            if (ls > 0) {
                hipLaunchKernelGGL(solver_trial_list_kernel<T>, dim3(nb), dim3(64), 0, s, n, nx, (int)ex_per,
                                   (const int*)ws.pend[(ls + pflip) & 1], (const T*)Zc, (const T*)ws.dz, (const T*)ws.alpha, (const T*)X0c,
                                   (const T*)extra_all, (T*)ws.Zt, (T*)ws.X0p, (T*)ws.exp_, a.n_pending);
                X0t = ws.X0p;
                if (ex_per) h.d_extra = ws.exp_;
            }
            // the merit function needs the defects only: the matrix-core kernel skips its reverse sweeps (tiles = null)
            // (compiled shapes: defects and f of the trial point from one forward-only launch)
            bool fused_trial = false, trial_done = false;
            a.carry = 0; a.hblk_t = nullptr;
            if (carry && hess_trial) {
                // blocks, defects and tiles of the trial point from one launch (the acceptance kernel evaluates the objective)
                const HessOut ho = blocks_eval_out(ws.hblk_t, ws.gt, ws.tiles_t);
                if (!has_blocks_eval(nb, ho)) hess_trial = false;
                else {
                    rc = launch_rowhess_mfma(h, nb, ws.Zt, X0t, ws.lam_t, ho, s);
                    trial_done = true; a.carry = 1; a.hblk_t = ws.hblk_t;
                }
            }
            if (carry && !trial_done && tracking) carry = false;      // (that launch fuses the shared objective)
            if (carry && !trial_done) {
                // full evaluation of the trial point (tiles and gradient too): it is the next iterate's if accepted
                const RowsOut ro = fused_eval_out(ws.gt, ws.tiles_t, ws.ft, ws.grad_t);
                fused_trial = has_fused_eval(nb, ro);
                if (!fused_trial) carry = false;      // not a compiled shape
                else { rc = launch_rows_mfma(h, nb, ws.Zt, X0t, ro, s); a.carry = 1; }
            }
            if (trial_done) {
            } else if (augmented) {
                rc = aug.eval(ws.Zt, nullptr);
            } else {
                if (!fused_trial) {
                    const RowsOut ro = fused_eval_out(ws.gt, nullptr, ws.ft, nullptr);
                    fused_trial = h.variant == NEMPC_KERNEL_MFMA && !tracking && has_fused_eval(nb, ro);
                    rc = fused_trial ? launch_rows_mfma(h, nb, ws.Zt, X0t, ro, s) : launch_rows(nb, ws.Zt, X0t, ws.gt, nullptr, h.d_tiles_ws.get());
                }
            }
            h.d_extra = extra_all;
            if (rc) return rc;
            // (no fused evaluation: the acceptance kernel computes the trial point's objective value itself)
            // Deferred backtracking with the trial point's blocks in hand: the test runs at the start of the next LQ kernel,
            // unless this is the last iteration of the budget or somebody reads the iterate before that kernel (diagnostics;
            // a compaction launches it below)
            accept_pending = kn.fuse_accept != 0 && a.fuse_step && trial_done && lsm == 2 && published_polls && it + 1 < o.max_iter && !trace &&
                             !kn.stats;
            if (!accept_pending)
                hipLaunchKernelGGL(solver_merit_kernel<T>, dim3(nb), dim3(64), 0, s, a, (const T*)ws.Zt,
                                   (const T*)ws.gt, fused_trial ? (const T*)ws.ft : (const T*)nullptr, (T*)Zc,
                                   lsm == 2 ? 2 : (ls + 1 == o.max_linesearch ? 1 : 0),
                                   ls > 0 ? (const int*)ws.pend[(ls + pflip) & 1] : (const int*)nullptr, ws.pend[(ls + 1 + pflip) & 1],
                                   ls == 0 ? 1 : 0, lsm == 2 ? 0 : ++pend_seq);
            have_eval = a.carry != 0;
            have_blocks = have_eval && a.hblk_t != nullptr;
            if (lsm == 2) break;          // one trial per outer iteration: nothing to poll
            // most iterations accept the first trial for every problem: one small poll saves the remaining
            // max_linesearch-1 callback evaluations
            if ((rc = poll_pending(pend_seq, &pending))) return rc;
            if (pending > 0 && ls == 0 && soc_on && !a.carry) {
                // second-order correction of the rejected full steps (solver_soc_kernel): one defect-only launch over the
                // rejected problems, accepted at the rejected trial's step length; what is still rejected backtracks as before
                const int* lin = ws.pend[(1 + pflip) & 1];
                int* lout = ws.pend[pflip & 1];
                hipLaunchKernelGGL(solver_soc_kernel<T>, dim3(pending), dim3(64), (size_t)2 * nx * sizeof(T), s, n, nx, nu, H, m, (int)ex_per, lin, (const T*)ws.Zt,
                                   (const T*)ws.gt, (const T*)ws.tiles, (const T*)X0c, (const T*)extra_all, (T*)ws.Zsoc, (T*)ws.X0p,
                                   (T*)ws.exp_, a.n_pending);
                if (ex_per) h.d_extra = ws.exp_;
                rc = launch_rows(pending, ws.Zsoc, ws.X0p, ws.gsoc, nullptr, h.d_tiles_ws.get());
                h.d_extra = extra_all;
                if (rc) return rc;
                hipLaunchKernelGGL(solver_merit_kernel<T>, dim3(pending), dim3(64), 0, s, a, (const T*)ws.Zsoc, (const T*)ws.gsoc,
                                   (const T*)nullptr, (T*)Zc, 0, lin, lout, 0, ++pend_seq, 1);
                if ((rc = poll_pending(pend_seq, &pending))) return rc;
                pflip ^= 1;
            }
            if (pending == 0) break;
            if (lsm == 3 && ls == 0 && pending * 4 <= std::min(Bact, last_nact)) {
                hipLaunchKernelGGL(solver_defer_kernel<T>, dim3((Bact + 255) / 256), dim3(256), 0, s, a);
                break;
            }
        }
        return NEMPC_OK;
    }
    // Small stages: an iteration is a chain of latency-bound launches, and a blocking poll drains the stream (10
    // polls of ~25 us in a 5.5 ms solve).  The acceptance kernel PUBLISHES the iteration's counter to pinned host
    // memory; the host only makes sure it never runs more than two iterations ahead of the device (it would
    // otherwise queue its whole budget before the first problem converges) and takes whatever the slot holds:
    // a count a couple of iterations old is an upper bound of the unconverged problems (they only ever leave),
    // which is all compaction needs, and "none left" is reported with the iteration at which it happened.
    int poll_published() {
        const int want = it + 1 - 2;
        if (want > 0)
            if (const int rc = wait_published(0, [want](int v) { return v >= want; }, "the convergence counter of iteration ", want))
                return rc;
        if (hp[0] > 0) {
            if (hp[2] > 0) { it = hp[2]; finished = true; return NEMPC_OK; }      // every problem had converged at that iteration
            last_nact = nact = hp[1];
        }
        return NEMPC_OK;
    }
    int diagnostics() {
        if (kn.stats) {   // NEMPC_SOLVER_STATS=1: Riccati restarts per iteration over the active slots (diagnostic, synchronises)
            std::vector<T> inf((size_t)Bact * INFO_N), rg((size_t)Bact);
            NEMPC_HIP(hipStreamSynchronize(s));
            NEMPC_HIP(hipMemcpy(inf.data(), a.info, inf.size() * sizeof(T), hipMemcpyDeviceToHost));
            NEMPC_HIP(hipMemcpy(rg.data(), a.reg, rg.size() * sizeof(T), hipMemcpyDeviceToHost));
            double sum = 0, mx = 0, rmx = 0; int nz = 0;
            for (int i = 0; i < Bact; ++i) {
                const double r = std::fabs((double)inf[(size_t)i * INFO_N + INFO_RESTARTS]);
                sum += r; if (r > mx) mx = r; if (r > 0) ++nz; if ((double)rg[i] > rmx) rmx = (double)rg[i];
            }
            fprintf(stderr, "[solver it %3d] active slots %4d  restarts: max %.0f mean %.2f  problems restarting %d  max damping %.1e\n",
                    it, Bact, mx, sum / Bact, nz, rmx);
        }
        if (trace) {   // NEMPC_SOLVER_TRACE=<slot>: one line per iteration for that slot (diagnostic, synchronises)
            T inf[INFO_N], muv, alv, regv, penv; int st, lsd;
            NEMPC_HIP(hipStreamSynchronize(s));
            NEMPC_HIP(hipMemcpy(inf, (const T*)a.info + (size_t)kn.trace_slot * INFO_N, sizeof(inf), hipMemcpyDeviceToHost));
            NEMPC_HIP(hipMemcpy(&muv, (const T*)a.mu + kn.trace_slot, sizeof(T), hipMemcpyDeviceToHost));
            NEMPC_HIP(hipMemcpy(&alv, (const T*)a.alpha + kn.trace_slot, sizeof(T), hipMemcpyDeviceToHost));
            NEMPC_HIP(hipMemcpy(&regv, (const T*)a.reg + kn.trace_slot, sizeof(T), hipMemcpyDeviceToHost));
            NEMPC_HIP(hipMemcpy(&penv, (const T*)a.pen + kn.trace_slot, sizeof(T), hipMemcpyDeviceToHost));
            NEMPC_HIP(hipMemcpy(&st, a.status + kn.trace_slot, sizeof(int), hipMemcpyDeviceToHost));
            NEMPC_HIP(hipMemcpy(&lsd, a.lsdone + kn.trace_slot, sizeof(int), hipMemcpyDeviceToHost));
            fprintf(stderr, "[solver it %3d slot %d] mu %.2e step %.2e ginf %.2e lam %.2e amax %.2e alpha %.2e reg %.1e pen %.2e restarts %.0f status %d lsdone %d\n",
                    it, kn.trace_slot, (double)muv, (double)inf[INFO_STEP], (double)inf[INFO_GINF], (double)inf[INFO_LAM],
                    (double)inf[INFO_AMAX], (double)alv, (double)regv, (double)penv, (double)inf[INFO_RESTARTS], st, lsd);
        }
        return NEMPC_OK;
    }
    // the acceptance test of a trial point that was left to the next LQ kernel, in a launch of its own
    void accept_now() {
        hipLaunchKernelGGL(solver_merit_kernel<T>, dim3(a.B), dim3(64), 0, s, a, (const T*)ws.Zt, (const T*)ws.gt,
                           (const T*)nullptr, (T*)ws.Zc[cur], 2, (const int*)nullptr, ws.pend[1], 1, 0);
        accept_pending = false;
    }
    // ---- compaction: gather the unconverged problems to the front of the other buffer set
    int compact_batch() {
        if (accept_pending) accept_now();       // the gather below reads the iterate
        const int nxt = cur ^ 1;
        hipLaunchKernelGGL(solver_partition_kernel, dim3(1), dim3(1024), 0, s, Bact, (const int*)ws.stc[cur], ws.perm,
                           ws.count);
        CompactArrays ca{};
        int k = 0;
        auto add = [&](const void* src, void* dst, int per, int esz) { ca.src[k] = src; ca.dst[k] = dst; ca.per[k] = per; ca.esz[k] = esz; ++k; };
        add(ws.Zc[cur], ws.Zc[nxt], n, sizeof(T));
        add(ws.X0c[cur], ws.X0c[nxt], nx, sizeof(T));
        add(ws.lamc[cur], ws.lamc[nxt], m, sizeof(T));
        add(ws.muc[cur], ws.muc[nxt], 1, sizeof(T));
        add(ws.nuc[cur], ws.nuc[nxt], 1, sizeof(T));
        add(ws.regc[cur], ws.regc[nxt], 1, sizeof(T));
        add(ws.stc[cur], ws.stc[nxt], 1, sizeof(int));
        add(ws.orig[cur], ws.orig[nxt], 1, sizeof(int));
        add(ws.itc[cur], ws.itc[nxt], 1, sizeof(int));
        add(ws.infoc[cur], ws.infoc[nxt], INFO_N, sizeof(T));
        add(ws.zlc[cur], ws.zlc[nxt], n, sizeof(T));
        add(ws.zuc[cur], ws.zuc[nxt], n, sizeof(T));
        if (ex_per) add(ws.exc[cur], ws.exc[nxt], (int)ex_per, sizeof(T));
        ca.n = k;
        hipLaunchKernelGGL(solver_gather_kernel, dim3(Bact), dim3(256), 0, s, Bact, (const int*)ws.perm, ca);
        // slots [Bact, B) hold problems that finished before earlier compactions: carry them over unchanged
        if (Bact < B) {
            const size_t rest = (size_t)(B - Bact);
            NEMPC_HIP(hipMemcpyAsync((T*)ws.Zc[nxt] + (size_t)Bact * n, (const T*)ws.Zc[cur] + (size_t)Bact * n,
                                     rest * n * sizeof(T), hipMemcpyDeviceToDevice, s));
            NEMPC_HIP(hipMemcpyAsync(ws.stc[nxt] + Bact, ws.stc[cur] + Bact, rest * sizeof(int), hipMemcpyDeviceToDevice, s));
            NEMPC_HIP(hipMemcpyAsync(ws.orig[nxt] + Bact, ws.orig[cur] + Bact, rest * sizeof(int), hipMemcpyDeviceToDevice, s));
            NEMPC_HIP(hipMemcpyAsync(ws.itc[nxt] + Bact, ws.itc[cur] + Bact, rest * sizeof(int), hipMemcpyDeviceToDevice, s));
            // ... with the multipliers they finished with (and the barrier parameter the primal barrier reports them from),
            // when the caller takes them: nothing else reads those rows of a finished problem
            if (duals.any()) {
                const size_t e = sizeof(T);
                NEMPC_HIP(hipMemcpyAsync((T*)ws.lamc[nxt] + (size_t)Bact * m, (const T*)ws.lamc[cur] + (size_t)Bact * m, rest * m * e, hipMemcpyDeviceToDevice, s));
                NEMPC_HIP(hipMemcpyAsync((T*)ws.zlc[nxt] + (size_t)Bact * n, (const T*)ws.zlc[cur] + (size_t)Bact * n, rest * n * e, hipMemcpyDeviceToDevice, s));
                NEMPC_HIP(hipMemcpyAsync((T*)ws.zuc[nxt] + (size_t)Bact * n, (const T*)ws.zuc[cur] + (size_t)Bact * n, rest * n * e, hipMemcpyDeviceToDevice, s));
                NEMPC_HIP(hipMemcpyAsync((T*)ws.muc[nxt] + Bact, (const T*)ws.muc[cur] + Bact, rest * e, hipMemcpyDeviceToDevice, s));
            }
        }
        // the unconverged problems now sit in front.  Their exact number is on the device; the host shrinks the
        // launches to the counter it has just read -- taken a period earlier, so an upper bound (problems only ever
        // leave the active set): a few finished problems ride along in the active prefix and are skipped by every
        // kernel, and no stream synchronisation is needed to learn the exact count
        cur = nxt;
        point_at(cur);
        have_eval = have_blocks = false;            // (the evaluation buffers are not gathered: one launch after a compaction)
        if (published_polls) {
            Bact = nact > 0 ? (nact < Bact ? nact : Bact) : 1;
        } else {
            NEMPC_HIP(hipMemcpyAsync(ws.hpoll, ws.count, sizeof(int), hipMemcpyDeviceToHost, s));
            NEMPC_HIP(hipStreamSynchronize(s));
            Bact = ws.hpoll[0] > 0 ? ws.hpoll[0] : 1;
        }
        a.ppw = pick_ppw(Bact);
        return NEMPC_OK;
    }
    // results back in the caller's order
    int finish(void* Z, int32_t* status_dev, int32_t* iters_host) {
        if (accept_pending) accept_now();           // (the loop was left with a trial point evaluated and not yet tested)
        hipLaunchKernelGGL(solver_scatter_kernel<T>, dim3(B), dim3(256), 0, s, B, n, (const T*)ws.Zc[cur],
                           (const int*)ws.stc[cur], (const int*)ws.orig[cur], (const int*)ws.itc[cur],
                           (T*)aug.solution_buffer(Z), status_dev, (int*)o.iters_out);
        aug.hand_back(Z);     // (augmented: the caller's variables out of the augmented solution)
        if (duals.any())  // (plain models only, solver_run: n, m are the caller's)
            hipLaunchKernelGGL(solver_scatter_duals_kernel<T>, dim3(B), dim3(256), 0, s, B, n, m, H * nx, (const T*)ws.Zc[cur],
                               (const T*)ws.lamc[cur], (const T*)ws.zlc[cur], (const T*)ws.zuc[cur], (const T*)ws.muc[cur],
                               (const T*)a.lb, (const T*)a.ub, (const int*)ws.orig[cur], a.bstride,
                               has_bounds && o.barrier == 1 ? 1 : 0,
                               (T*)duals.lam, (T*)duals.zl, (T*)duals.zu);
        NEMPC_HIP(hipGetLastError());
        NEMPC_HIP(hipStreamSynchronize(s));
        if (iters_host) *iters_host = it;
        return NEMPC_OK;
    }
};
}  // namespace

// Every exit of a failed solve leaves the handle as a finished one does: kernels that still write the published words
// (hpub) and the device counters may be queued when an error return is taken from inside the iteration loop, and the
// next solve zeroes those words on the assumption that nothing is in flight.  Drain the stream, reset the counters.
template <typename T>
static int solve_typed(Handle& h, int B, const void* X0, void* Z, const double* lb, const double* ub,
                       const nempc_solver_opts& o, int32_t* status_dev, int32_t* iters_host, const SolverDuals& duals, hipStream_t s) {
    const int rc = Solve<T>(h, B, X0, o, duals, s).run(Z, lb, ub, status_dev, iters_host);
    if (rc != NEMPC_OK) {
        (void)hipStreamSynchronize(s);
        if (SolverWs* w = static_cast<SolverWs*>(h.solver_ws)) {
            if (w->n_active) (void)hipMemset(w->n_active, 0, 8 * sizeof(int));
            if (w->hpub) for (int k = 0; k < 8; ++k) w->hpub[k] = 0;
        }
        (void)hipGetLastError();
    }
    return rc;
}

int intersect_bounds(const Handle& h, const double* lb, const double* ub, bool need_interior, const char* who,
                     std::vector<double>& lo_out, std::vector<double>& hi_out) {
    const int hx = h.cfg.H * h.cfg.nx, nx = h.cfg.nx;
    lo_out.assign(h.n, -INFINITY);
    hi_out.assign(h.n, INFINITY);
    for (int i = 0; i < h.n; ++i) {
        double lo = lb ? lb[i] : -INFINITY, hi = ub ? ub[i] : INFINITY;
        if (h.box && i < hx) {
            lo = std::max(lo, h.box_lo[i % nx]);
            hi = std::min(hi, h.box_hi[i % nx]);
        }
        if (lo > hi) { set_error(std::string(who) + ": lb > ub"); return NEMPC_EINVAL; }
        if (need_interior && lo == hi) {
            set_error(std::string(who) + ": lb == ub (a fixed variable has no interior for the barrier); eliminate it from the problem");
            return NEMPC_EINVAL;
        }
        lo_out[i] = lo; hi_out[i] = hi;
    }
    return NEMPC_OK;
}

int solver_run(Handle& h, int B, const void* X0, void* Z, const double* lb, const double* ub,
               const nempc_solver_opts& o, int32_t* status_dev, int32_t* iters_host, const SolverDuals& duals, hipStream_t s) {
    if (duals.any() && h.w > 1) {
        set_error("nempc_solve_duals: multipliers of a rolling_window > 1 handle are not supported (the costates of the window "
                  "state are not mapped back to the caller's rows); pass NULL for lam, zl and zu");
        return NEMPC_EUNSUPPORTED;
    }
    if (duals.any() && h.rate.on()) {
        set_error("nempc_solve_duals: multipliers under a rate binding (nempc_bind_rate) are not supported (the costates of the "
                  "augmented state are not mapped back to the caller's rows); pass NULL for lam, zl and zu");
        return NEMPC_EUNSUPPORTED;
    }
    return h.cfg.dtype == NEMPC_F64 ? solve_typed<double>(h, B, X0, Z, lb, ub, o, status_dev, iters_host, duals, s)
                                    : solve_typed<float>(h, B, X0, Z, lb, ub, o, status_dev, iters_host, duals, s);
}

}  // namespace nempc
