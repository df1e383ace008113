// The contract between the batched solver's host driver (Solve<T>, solver.hip) and its kernels: the info row's columns,
// the kernels' argument block, what the LQ kernels hand the acceptance code, the first damping level and the diagnostic
// cycle stamps.  Included by solver.hip only, ahead of the solver_*_impl.h headers.
#pragma once

#include "nempc_internal.h"

#ifndef NEMPC_REG_FLOOR
#define NEMPC_REG_FLOOR 1e-3      // first damping level of a restarted Riccati sweep (see solver_lq_kernel)
#endif

namespace nempc {

namespace {

constexpr int INFO_LAM = 0, INFO_STEP = 1, INFO_AMAX = 2, INFO_G1 = 3, INFO_GINF = 4, INFO_D0 = 5, INFO_ZINF = 6,
              INFO_RESTARTS = 7,
              INFO_LSK = 8, INFO_LSA = 9,   // deferred backtracking: rejected trials in a row, step length to retry with,
              INFO_LSR = 10,                // Riccati restarts of the iteration that opened the search (sticky over retries)
              // non-monotone acceptance: the merit values of the last two accepted iterates, the penalty / barrier parameter
              // they were computed under, how many of them are valid
              INFO_PH1 = 11, INFO_PH2 = 12, INFO_PH3 = 13, INFO_PH4 = 14, INFO_PHNU = 15, INFO_PHMU = 16, INFO_PHN = 17,
              INFO_PHUP = 18,               // 1: the last accepted step went uphill in the merit (watchdog, see solver_merit_body)
              INFO_N = 19;

struct SolverArgs {
    int B, H, nx, nu, nin, n, m;
    const void* Z; const void* grad; const void* g; const void* tiles;   // at the current iterate
    const void* hblk;                                                    // (B,H,nin,nin) Lagrangian blocks
    void* lam; void* lamn;                                               // (B,m) multipliers: current, LQ costates
    const void* obj;  ObjOffsets oo;                                     // Qs, Rs live in the objective block
    // per-problem tracking data (nempc_bind_tracking; trk.B == 0: none) and, per slot of the working batch, the caller's
    // index of the problem that sits there (the buffer set's orig[]): the data are the CALLER's problem's, wherever
    // compaction or a trial list has moved it
    TrackBind trk; const int* trk_prob;
    const void* lb; const void* ub;                                      // (n) device, dtype T, +-max for no bound
    // ... or, with per-problem bounds bound (nempc_bind_bounds), the (B,n) working copy of every problem's effective bounds
    // in the CALLER's order (solver_init_bound_kernel writes it): bstride = n, and the bounds of the problem in slot b are
    // row trk_prob[b].  bstride = 0: the one shared vector
    int bstride;
    void* mu; void* pen; void* reg; void* alpha; void* phi0; void* dir;  // (B) per problem (pen = l1 penalty)
    int lq_attempts;      // Riccati sweeps a problem may try per iteration before it sits the iteration out
    int* hpub;            // pinned host memory the acceptance kernel publishes the convergence counter to: [0] iteration
                          // tag, [1] unconverged problems at that iteration, [2] first iteration at which none was left;
                          // inner-loop backtracking: [4] sequence number of the trial, [5] problems still searching after it
    int* n_done;          // acceptance launches of the inner loop: blocks finished (the last one publishes)
    int carry;            // the trial evaluation is a full one and becomes the next iterate's on acceptance (tiles_t, grad_t)
    const void *tiles_t, *grad_t;
    // ... with the Lagrangian blocks of the trial point too (one launch: blocks + evaluation, HessOut::ev_g): the
    // step kernel writes the multipliers the trial point would have, lam + alpha (lamn - lam); hblk_t is carried over on
    // acceptance like the tiles
    void* lam_t; const void* hblk_t;
    // ... and the acceptance test of that trial point at the START of the next iteration's LQ kernel instead of in a launch
    // of its own (two launches per iteration): the LQ kernel's waves run solver_merit_body for their problems before they
    // stage.  The convergence counter alternates between two words by iteration parity -- the accept phase publishes and
    // clears the PREVIOUS iteration's word while this kernel's post-pass counts into its own
    int accept_first; int* n_active_prev; const void* gt_acc;
    int fuse_step;        // thread-per-problem Riccati kernel in LDS mode: it also does solver_step_kernel's work
    void* f_it; void* Zt_it;   // ... with the iterate's objective values (B) and the trial-point buffer (B,n)
    int* status; int* lsdone; int* n_active; int* n_pending;   // counters the host polls: unconverged problems / problems still backtracking
    int* iters_done; int cur_it;                                         // per problem: iteration at which it converged
    // bounds, primal-dual: zl / zu (B,n) multipliers of z >= lb / z <= ub, their steps, and the barrier diagonal the LQ
    // model adds to the Hessian (zl/(z-lb) + zu/(ub-z)); the barrier gradient -mu/(z-lb) + mu/(ub-z) is folded into grad
    void* zl; void* zu; void* dzl; void* dzu; void* alz; void* bh;
    int primal_dual;
    void* dz; void* info;                                                // (B,n), (B,INFO_N)
    void* Kst; void* kst; void* Pst; void* pst;                          // Riccati storage per problem
    void* tmp; size_t tmp_stride;                                        // global temporaries when LDS is too small
    int use_lds;                                                         // 1: per-problem working set staged in LDS
    int ppw;                                                             // problems per workgroup (LDS mode)
    int lds_stride;                                                      // elements per problem in LDS (odd)
    int spec, att_elems;   // thread-per-problem sweep: damping levels tried side by side (lanes per problem), elements of
                           // one attempt's region (gains, value function, temporaries) in the problem's LDS block
    double tol_g, tol_step, mu_min, mu_factor;
    double armijo_slack;                                                 // relative slack of the Armijo test (see merit kernel)
    int nonmono;                                                         // merit values of previous iterates the test may refer to (0: monotone)
    double reg_relax;                                                    // factor by which the Levenberg term is relaxed after a clean sweep
    double reg_raise;                                                    // ... and by which it is raised when a sweep meets a pivot that is not positive
    int max_ls;                                                          // halvings before the next LQ solve is damped
};

// the bounds of the problem in slot b of the working batch (SolverArgs::bstride; wave-uniform)
template <typename T>
__device__ __forceinline__ const T* solver_lb(const SolverArgs& a, int b) {
    return a.bstride ? (const T*)a.lb + (size_t)a.trk_prob[b] * a.bstride : (const T*)a.lb;
}
template <typename T>
__device__ __forceinline__ const T* solver_ub(const SolverArgs& a, int b) {
    return a.bstride ? (const T*)a.ub + (size_t)a.trk_prob[b] * a.bstride : (const T*)a.ub;
}

template <typename T>
struct StepInfo {   // what the Riccati kernel leaves in the info row (read from there, or handed over in registers) ...
    T ginf, step, zinf, lam, d0, amax, lsk, lsa, restarts;
    // ... and the problem's scalars, loaded in one go ahead of their use (each was a dependent global round trip)
    T lsr, mu, nu, f;
    int status;
};

#ifdef NEMPC_LQ_STAMPS
__device__ long long nempc_lq_stamps[16];
#define LQ_STAMP(i) do { if (blockIdx.x == 0 && threadIdx.x == 0) nempc_lq_stamps[i] = (long long)__builtin_readcyclecounter(); } while (0)
#else
#define LQ_STAMP(i) do { } while (0)
#endif

}  // namespace

}  // namespace nempc
