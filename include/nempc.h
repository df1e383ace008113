/*
 * nempc.h -- C ABI of the MI355X-native NMPC callback engine (libnempc.so).
 *
 * The reference (Enderdead/pyNeuralEMPC) is pure Python and has no FFI of its own; what this
 * library replaces is the arithmetic behind the five solver callbacks of
 *     pyNeuralEMPC/optimizer/ipopt.py:30-96   (objective / gradient / constraints / jacobian / hessian)
 * i.e.   integrator/{discret,unity,rk4}.py  forward + jacobian (+ hessian),
 *        model/tensorflow.py:49-109         network forward / per-row jacobian / hessian,
 *        objective/jax.py:28-57             f, grad f, hess f   (quadratic + linear family),
 *        constraints.py:36-96               extra constraint rows (box rows on the states),
 * evaluated for a BATCH of B independent problems per call (the reference solves one).
 *
 * Conventions
 *  - every `const void*` / `void*` named Z, X0, f, grad, g, jac_*, lambda, sigma, hvals is a
 *    DEVICE pointer owned by the caller, holding elements of the handle's dtype
 *    (NEMPC_F64 -> double, NEMPC_F32 -> float), dense row-major, no padding;
 *  - weights / objective / bounds setters take HOST pointers to double;
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls enqueue work and
 *    return; use nempc_sync or your own stream/event to wait;
 *  - every function returns 0 (NEMPC_OK) or a negative NEMPC_E* code and never throws;
 *    nempc_last_error() gives the message of the calling thread's last failure;
 *  - a handle is not re-entrant: one in-flight evaluation per handle (use one handle per stream).
 *
 * Layouts (identical to the reference, optimizer/ipopt.py:20-28):
 *    z  (n)      n = H*(nx+nu): z[0:H*nx] states (H,nx) row-major, z[H*nx:] controls (H,nu)
 *    g  (m)      m = H*nx defects [+ H*nx box rows = states.ravel() when enabled]
 *    jac_dense   (m,n) row-major -- what IpoptProblem.jacobian returns (ipopt.py:88-96)
 *    jac_tiles   (H,nx,nx+nu): row t = d Phi(x_{t-1},u_t) / d [x_{t-1} | u_t]  (compact contract)
 *
 * Rolling-window models (KerasTFModelRollingInput model/tensorflow.py:132-340, DiffDiscretJaxModelRollingWindow
 * model/jax.py:93-259): with rolling_window = w > 1 the network of step t reads the last w states and controls,
 *    xi_t = [ x_{t-w} .. x_{t-1} | u_{t-w+1} .. u_t | extras_t ]      (oldest first; newest first when
 *                                                                      rolling_reverse, tensorflow.py:120-127)
 * entries reaching before the horizon come from x0 and the history bound by nempc_bind_history.  The tile width
 * becomes w*(nx+nu) (window columns in the network's input order); the dense Jacobian / Hessian get the band the
 * reference builds with its projection matrices (jax.py:8-21, tensorflow.py:253-262, 312-340).
 */
#ifndef NEMPC_H
#define NEMPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NEMPC_ABI_VERSION 8
#define NEMPC_MAX_LAYERS 8 /* dense layers incl. the linear output layer */

/* status codes */
#define NEMPC_OK 0
#define NEMPC_EINVAL (-1)   /* bad argument / dims */
#define NEMPC_ENOMEM (-2)   /* device allocation failed */
#define NEMPC_EHIP (-3)     /* a HIP runtime call failed */
#define NEMPC_ESTATE (-4)   /* call order: weights / objective not set yet */
#define NEMPC_EUNSUPPORTED (-5)
#define NEMPC_EFULL (-6)    /* nempc_jac_dense_resident: the handle's table is full; not fatal, nothing changed */

/* dtype */
#define NEMPC_F64 0
#define NEMPC_F32 1

/* integrator kind -- integrator/discret.py, unity.py, rk4.py */
#define NEMPC_DISCRET 0 /* Phi = x + f(x,u) */
#define NEMPC_UNITY 1   /* Phi = f(x,u) */
#define NEMPC_RK4 2     /* Phi = x + DT/6 (k1 + 2k2 + 2k3 + k4) */

/* activation of a dense layer -- what the Keras Dense layers of the model KerasTFModel wraps are built with
 * (model/tensorflow.py:8-29 takes ANY feed-forward Keras model; tensorflow.py:49-109 differentiates it by autodiff).
 * Derivatives are evaluated from the layer's output a = s(z): s' = 1 (linear), 1 - a^2 (tanh), [a > 0] (relu: the
 * gradient at 0 is 0, as TensorFlow's), a(1-a) (sigmoid), 1 - e^-a (softplus), 1 | a + alpha (elu), 1 | alpha (leaky_relu),
 * lambda | a + lambda alpha (selu, Keras' fixed constants) -- the MONOTONE activations, whose derivatives follow from the
 * output alone.  swish (= silu, z sigmoid(z)), gelu (z Phi(z), Keras' approximate=False), softsign, mish, exponential and relu6
 * are written from the pre-activation (the first two and mish are not monotone; for the others it is simply the form at
 * hand), which the layer-at-a-time matrix-core path and the generic kernel keep (NEMPC_KERNEL_LAYERED / AUTO / VALU; any
 * layer, the output layer included) -- asking for the register-resident kernels (NEMPC_KERNEL_MFMA*) with them is refused.
 * Per-layer MIXES of the monotone family under a linear output layer run on the register-resident kernels, too (hidden
 * widths <= 128, <= 3 hidden layers, 4 up to width 64): the layers' codes are launch arguments there.
 * elu and leaky_relu read their alpha from nempc_config.act_param (elu: > 0, leaky_relu: >= 0). */
#define NEMPC_ACT_LINEAR 0
#define NEMPC_ACT_TANH 1
#define NEMPC_ACT_RELU 2
#define NEMPC_ACT_SIGMOID 3
#define NEMPC_ACT_SOFTPLUS 4
#define NEMPC_ACT_ELU 5
#define NEMPC_ACT_LEAKY_RELU 6
#define NEMPC_ACT_SELU 7
#define NEMPC_ACT_SWISH 8
#define NEMPC_ACT_GELU 9
#define NEMPC_ACT_SOFTSIGN 10    /* z / (1 + |z|)                    -- these four, like swish / gelu, from the pre-activation: */
#define NEMPC_ACT_MISH 11        /* z tanh(softplus(z))                  the layered path and the generic kernel */
#define NEMPC_ACT_EXPONENTIAL 12 /* e^z */
#define NEMPC_ACT_RELU6 13       /* min(max(z, 0), 6): Keras' ReLU(max_value=6) */
#define NEMPC_ACT_COUNT 14
#define NEMPC_ACT_FIRST_ZBASED NEMPC_ACT_SWISH /* codes >= this one are written from the pre-activation */

/* row-kernel implementation */
#define NEMPC_KERNEL_AUTO 0
#define NEMPC_KERNEL_VALU 1 /* generic thread-per-row kernel, any dims */
#define NEMPC_KERNEL_MFMA 2 /* matrix-core kernels, padded hidden width in {32,64,128}, <=3 hidden layers, nx <= 16,
                               network inputs w*(nx+nu)+n_extra <= 32, ONE non-linear activation on every hidden layer
                               and a linear output layer: CU-cooperative kernel when the weight slices fit the
                               registers and the inputs <= 16, else wave-per-tile */
#define NEMPC_KERNEL_MFMA_TILE 3 /* force the wave-per-tile matrix-core kernel (A/B measurements) */
#define NEMPC_KERNEL_LAYERED 4 /* layer-at-a-time matrix-core path: one GEMM launch per dense layer over all B*H rows, any
                                  activation per layer (output layer included), hidden widths <= 1024, up to 8 layers,
                                  w*(nx+nu) <= 128 decision inputs (extra inputs do not count), nx <= 64 -- what any
                                  feed-forward Keras model the reference wraps (model/tensorflow.py:8-29) that
                                  NEMPC_KERNEL_MFMA does not take runs on under AUTO.  Rows and Lagrangian blocks (Discret /
                                  Unity / RK4), hence the batched solver too.  One exception: the RK4 Lagrangian blocks of a
                                  shape whose congruence step (8 nin^2 + 3 nx nin elements per row, nin = nx+nu) does not
                                  fit the device's LDS -- fp64 beyond about 45 inputs at 160 KB -- come from the generic
                                  kernel (nempc_last_hess_kernel: 1); the rows of such a model stay on this path */

typedef struct nempc_handle_s* nempc_handle;

typedef struct nempc_config {
    int32_t abi_version;              /* = NEMPC_ABI_VERSION */
    int32_t device;                   /* HIP device ordinal */
    int32_t dtype;                    /* NEMPC_F64 | NEMPC_F32 */
    int32_t integrator;               /* NEMPC_DISCRET | NEMPC_UNITY | NEMPC_RK4 */
    int32_t H, nx, nu;                /* Integrator.H, Model.x_dim, Model.u_dim */
    int32_t n_layers;                 /* dense layers, >= 1; layer l applies activations[l] (below) */
    int32_t widths[NEMPC_MAX_LAYERS]; /* output width of each layer; widths[n_layers-1] == nx */
    int32_t max_batch;                /* capacity B_max of the workspaces */
    int32_t kernel;                   /* NEMPC_KERNEL_* */
    int32_t n_extra;                  /* extra per-step network inputs after [x | u]: tvp_dim + p_dim of the reference's
                                         Model (model/tensorflow.py:39-47); they feed the network but are not decision
                                         variables: no Jacobian / Hessian columns (tensorflow.py:65-66). 0 = none */
    int32_t rolling_window;           /* w >= 1: steps of history the network reads (1 = plain model).  w > 1 needs
                                         DISCRET or UNITY (the reference has no RK4 for rolling models) */
    int32_t rolling_reverse;          /* 0: window rows oldest -> newest (forward_rolling=True); 1: newest first */
    double DT;                        /* RK4 step (RK4Integrator.DT, rk4.py:49) */
    int32_t activations[NEMPC_MAX_LAYERS]; /* NEMPC_ACT_* of each layer, the output layer included (the reference's
                                         nn_model.h5: tanh, tanh, linear).  Any mix runs on the generic kernel; the
                                         matrix-core kernels take one non-linear activation on all hidden layers and
                                         a linear output layer (NEMPC_KERNEL_AUTO picks accordingly) */
    double act_param[NEMPC_MAX_LAYERS];    /* alpha of an elu / leaky_relu layer (Keras: ELU(alpha), LeakyReLU(negative_slope));
                                         ignored for the other activations.  The register-resident matrix-core kernels take
                                         elu with alpha = 1 only; leaky_relu, selu and elu(alpha != 1) run on the layered
                                         matrix-core path and the generic kernel */
} nempc_config;

/* lifetime ------------------------------------------------------------------------------- */
int nempc_create(const nempc_config* cfg, nempc_handle* out);
int nempc_destroy(nempc_handle h);

/* grow the workspaces to hold max_batch problems per call (no-op when they already do).  Everything else the handle
 * owns -- weights, objective, structure, bindings, communicator -- is kept.  Synchronises the device. */
int nempc_reserve(nempc_handle h, int32_t max_batch);

/* network weights: W[l] is (in_l, out_l) row-major -- the Keras `kernel` layout used by
 * KerasTFModel (model/tensorflow.py:8-51); b[l] is (out_l). Host doubles. */
int nempc_set_weights(nempc_handle h, const double* const* W, const double* const* b);

/* objective family standing in for JAXObjectifFunc (objective/jax.py:16-57):
 *   f = sum_t (x_t-xref_t)^T Q (x_t-xref_t) + (u_t-uref_t)^T R (u_t-uref_t) + cx_t.x_t + cu_t.u_t
 * Q (nx,nx), R (nu,nu), xref/cx (H,nx), uref/cu (H,nu); any pointer may be NULL (= zeros;
 * Q NULL = identity, R NULL = 0.1*identity, the SURVEY 8(d) defaults). Host doubles.
 * Ordering: the values overwrite the handle's parameter block in place with a copy on the NULL stream (no re-allocation, no
 * device synchronisation -- a tracking MPC moves xref / uref every step).  The NULL stream orders the copy against work on
 * blocking streams only: a caller that queues nempc_eval / nempc_hess / nempc_solve on a NON-BLOCKING stream must
 * nempc_sync that stream before changing the objective (same for nempc_set_terminal_weight), or the queued kernels may
 * read a half-updated block. */
int nempc_set_objective(nempc_handle h, const double* Q, const double* R, const double* xref,
                        const double* uref, const double* cx, const double* cu);

/* terminal cost: the last step's state term uses QT (nx,nx) instead of Q,
 *   ... + (x_{H-1}-xref_{H-1})^T QT (x_{H-1}-xref_{H-1});   NULL = back to Q.  Kept across nempc_set_objective calls.
 * (A member of the same family: JAXObjectifFunc takes any function of the whole trajectory, objective/jax.py:28-33.) */
int nempc_set_terminal_weight(nempc_handle h, const double* QT);

/* bind the extra network inputs for subsequent nempc_eval / nempc_hess / nempc_solve calls: E (B,H,n_extra) device,
 * dtype of the handle, row t of problem b = [tvp_t ; p] (time-varying parameters then constant parameters, the
 * concatenation order of KerasTFModel._gather_input).  The pointer is stored, not copied; required when
 * n_extra > 0.  B = problems the tensor covers: a later evaluation of more problems than that is refused
 * (NEMPC_EINVAL) instead of reading past the end.  */
int nempc_bind_extra(nempc_handle h, const void* E, int32_t B);

/* history of a rolling-window model for subsequent calls (set_prev_data, model/tensorflow.py:178-189):
 * hist_x (B, w-1, nx) = the w-1 states BEFORE x0, oldest first; hist_u (B, w-1, nu) = the w-1 controls before u_0.
 * Device pointers of the handle's dtype, stored not copied; required when rolling_window > 1.  B = problems the
 * tensors cover (evaluations of more problems are refused). */
int nempc_bind_history(nempc_handle h, const void* hist_x, const void* hist_u, int32_t B);

/* per-problem tracking references and linear costs for subsequent nempc_eval / nempc_rollout / nempc_solve calls.  The
 * weights Q, R, QT stay the handle's; each of xref, uref, cx, cu that is given replaces the matching array of
 * nempc_set_objective for problem b by that problem's own block, an array left NULL keeps the shared values:
 *    f_b = sum_t (x_t - xref_{b,t})' Q|QT (x_t - xref_{b,t}) + (u_t - uref_{b,t})' R (u_t - uref_{b,t})
 *                + cx_{b,t} . x_t + cu_{b,t} . u_t
 * (evaluated in this form, subtraction first: the arithmetic of the shared objective, to the bit when the data are equal).
 *   xref, cx  B blocks of (H,nx), ld_x elements from one problem's block to the next (ld_x >= H*nx);
 *   uref, cu  B blocks of (H,nu), ld_u elements apart (ld_u >= H*nu).
 * A leading dimension larger than one block lets a window slide over a longer per-problem reference without a copy: bind
 * base + k*nx (base + k*nu) for the window that starts at row k.  Device pointers of the handle's dtype, stored not copied,
 * read in stream order by the launches that follow.  B = problems the arrays cover: an evaluation of more problems is
 * NEMPC_EINVAL.  All four NULL removes the binding.  nempc_hess / nempc_hess_gn do not read these arrays (the Hessian of
 * the objective is the weights').  nempc_solve with a binding on a rolling_window > 1 handle is NEMPC_EUNSUPPORTED (the
 * objective table over the window state is built on the host). */
int nempc_bind_tracking(nempc_handle h, const void* xref, const void* uref, const void* cx, const void* cu,
                        int32_t B, int64_t ld_x, int64_t ld_u);

/* per-problem, per-stage lower and upper bounds on the states and controls for subsequent nempc_solve / nempc_solve_duals /
 * nempc_kkt_residual / nempc_sensitivity calls.  The host lb / ub of those calls stay one vector for the whole batch; each
 * of xlb, xub, ulb, uub that is given adds problem b's own rows, an array left NULL adds nothing.  The effective bounds of
 * problem b are the intersection of the host lb / ub of the call (NULL = unbounded), the box rows and that problem's rows:
 *    max(lb_i, box_lo, xlb_{b,t,j}) <= x_{t,j} = z[t*nx + j] <= min(ub_i, box_hi, xub_{b,t,j}),   likewise u_t with ulb, uub
 * (x0 is data, not a variable: row t of the x arrays bounds x_t, the state the t-th step arrives at).
 *   xlb, xub  B blocks of (H,nx), ld_x elements from one problem's block to the next (ld_x >= H*nx);
 *   ulb, uub  B blocks of (H,nu), ld_u elements apart (ld_u >= H*nu).
 * A leading dimension larger than one block lets a window slide over a longer per-problem schedule without a copy: bind
 * base + k*nx (base + k*nu) for the window that starts at row k.  Device pointers of the handle's dtype, stored not copied,
 * read in stream order by the launches that follow.  +-inf means "no bound there", and so does a value of magnitude at or
 * above the dtype's max.  B = problems the arrays cover: a solve / KKT / sensitivity call over more problems is
 * NEMPC_EINVAL.  All four NULL removes the binding.  nempc_eval, nempc_hess / nempc_hess_gn and nempc_rollout do not read
 * these arrays.  The arrays live on the device, so the host check of lb / ub (lb > ub, lb == ub) cannot see them: a problem
 * whose effective bounds have a variable with lo >= hi or a NaN fails alone, decided on the device -- nempc_solve returns it
 * with status 1, 0 iterations and its Z exactly as handed in, the other problems of the batch are not affected; a problem
 * with no finite effective bound is solved as an unbounded one (zl = zu = 0).  nempc_kkt_residual and nempc_sensitivity do
 * not validate: an empty interval shows up as r[1] > 0.  nempc_solve with a binding on a rolling_window > 1 handle is
 * NEMPC_EUNSUPPORTED (the bounds of the window state are built on the host). */
int nempc_bind_bounds(nempc_handle h, const void* xlb, const void* xub, const void* ulb, const void* uub,
                      int32_t B, int64_t ld_x, int64_t ld_u);

/* input-rate penalty and rate limits for subsequent nempc_solve calls.  With du_t = u_t - u_{t-1} and u_{-1} = u_prev_b (the
 * control applied before problem b's first step, data), the solve becomes
 *    min f(z) + sum_{t=0..H-1} du_t' S du_t    s.t. defects = 0,  lb <= z <= ub (as without the binding),  dlo_t <= du_t <= dhi_t
 *   S         (nu,nu) host doubles, used as given like R (the gradient uses S + S'); NULL = no penalty;
 *   dlo, dhi  host doubles, (nu) when per_stage == 0 (every step), (H,nu) when per_stage == 1; NULL or -+INFINITY = no limit.
 *             dlo >= dhi on any entry, or a NaN, is NEMPC_EINVAL (the barrier needs an interior: the rule of lb == ub);
 *   u_prev    (B,nu) device pointer of the handle's dtype, stored not copied, read in stream order by the solves that
 *             follow; required whenever S, dlo or dhi is given.  B = problems it covers: a solve over more is NEMPC_EINVAL.
 * S, dlo, dhi are copied.  All of S, dlo, dhi, u_prev NULL removes the binding.
 * The solver runs the problem stage-wise in the state [x_t ; u_t] with du_t as the stage control; the returned
 * u are the u slots of that state, and u_t - u_{t-1} = du_t holds to tol_constraint at convergence.  The Levenberg term of
 * nempc_solver_opts.reg sits on du.
 * nempc_eval, nempc_hess / nempc_hess_gn and nempc_rollout do not read the binding: they evaluate the plain problem.
 * While a binding is on: nempc_solve_duals with a non-NULL lam, zl or zu, nempc_kkt_residual, nempc_sensitivity and
 * nempc_kkt_solve are NEMPC_EUNSUPPORTED (they would certify or differentiate a different problem; mapping the multipliers of
 * the augmented problem back to the caller's rows is left to a later change); nempc_solve with a tracking binding
 * (nempc_bind_tracking) or per-problem bounds (nempc_bind_bounds) is NEMPC_EUNSUPPORTED (the objective table and the bounds of
 * the augmented state are built on the host, as for rolling windows).  On a rolling_window > 1 handle the call itself is
 * NEMPC_EUNSUPPORTED. */
int nempc_bind_rate(nempc_handle h, const double* S, const double* dlo, const double* dhi, int32_t per_stage,
                    const void* u_prev, int32_t B);

/* linear stage inequality rows for subsequent nempc_solve calls.  With C = [Cx (nc,nx) | Cu (nc,nu)] shared by every problem
 * and every step, the solve becomes
 *    min f(z)    s.t. defects = 0,  lb <= z <= ub (as without the binding),  rlo_t <= Cx x_t + Cu u_t <= rhi_t,  t = 0 .. H-1
 * Pairing: row block t pairs ROW t of the state block of z with ROW t of its control block -- z = [x rows (H,nx) | u rows
 * (H,nu)], state row t being the state the t-th step arrives at, Phi(state row t-1, control row t).  It is the pairing of the
 * reference's Constraint.forward(x, u) on its (H,nx) and (H,nu) arguments and of nempc_bind_bounds (row t of the x arrays
 * bounds x_t): state-only rows (Cu = 0) cover every state variable, control-only rows (Cx = 0) every control; x0 is data and
 * no row reads it.
 *   nc        rows per stage; nc == 0 or C == NULL removes the binding; nc < 0 is NEMPC_EINVAL;
 *   C         (nc, nx+nu) host doubles, row-major, copied (a non-finite entry is NEMPC_EINVAL);
 *   rlo, rhi  host doubles, copied: (nc) when per_stage == 0 (every step), (H,nc) when per_stage == 1; NULL or -+INFINITY = no
 *             limit on that side.  rlo >= rhi on any entry, or a NaN, is NEMPC_EINVAL (the barrier needs an interior: the rule
 *             of lb == ub; equality rows are not built).
 * The solver runs the problem stage-wise in the state [x_t ; y_t], y_t = Cx x_t + Cu u_t, with the rows as variable bounds of
 * y; the returned Z is the x and u of that problem.  Feasibility: at convergence (status 0) every row holds to
 * tol_constraint * (1 + |Cx row|_1) -- y is strictly inside its limits and both defect families, x_t - Phi and y_t - Cx Phi -
 * Cu u_t, are below tol_constraint.  The Levenberg term of nempc_solver_opts.reg stays on u.  The products with C accumulate
 * in the handle's dtype in a fixed order: a solve is bitwise reproducible.
 * nempc_eval, nempc_hess / nempc_hess_gn and nempc_rollout do not read the binding: they evaluate the plain problem, their
 * outputs unchanged to the bit.
 * While a binding is on, these are NEMPC_EUNSUPPORTED, each with a nempc_last_error text that names the call, and the handle
 * stays usable: nempc_solve_duals with a non-NULL lam, zl or zu; nempc_kkt_residual, nempc_sensitivity and nempc_kkt_solve (they
 * would certify or differentiate a different problem; the multipliers of the rows are left to a later change); nempc_solve
 * together with a rate binding (nempc_bind_rate), a tracking binding (nempc_bind_tracking) or per-problem bounds
 * (nempc_bind_bounds).  On a rolling_window > 1 handle the call itself is NEMPC_EUNSUPPORTED. */
int nempc_bind_stage_rows(nempc_handle h, int32_t nc, const double* C, const double* rlo, const double* rhi, int32_t per_stage);

/* extra constraint rows g_box = states.ravel() (a Constraint in the sense of constraints.py:36-63
 * with constant selector Jacobian); lo/hi (nx) host doubles are only reported back through
 * nempc_constraint_bounds. enabled=0 removes the rows. */
int nempc_set_box_rows(nempc_handle h, int enabled, const double* lo, const double* hi);

/* sizes: n, m, structural nnz of jac, nnz of the lower-triangular Lagrangian Hessian */
int nempc_dims(nempc_handle h, int32_t* n, int32_t* m, int32_t* nnz_jac, int32_t* nnz_hess);

/* cl, cu (m) host doubles -- IpoptProblem.get_constraint_{lower,upper}_bounds, ipopt.py:104-108 */
int nempc_constraint_bounds(nempc_handle h, double* cl, double* cu);

/* sparsity patterns, host int32, row-major sorted (the order of np.nonzero):
 * jacobian pattern (nnz_jac) and lower-triangular Hessian pattern (nnz_hess) -- replaces the
 * random-sampling probe of integrator/base.py:89-115 + ipopt.py:55-62 by the exact band pattern */
int nempc_jac_structure(nempc_handle h, int32_t* rows, int32_t* cols);
int nempc_hess_structure(nempc_handle h, int32_t* rows, int32_t* cols);

/* one batched evaluation of the hessian-free callbacks for B <= max_batch problems.
 *   Z (B,n), X0 (B,nx) inputs.  Outputs, each may be NULL to skip:
 *   f (B)            IpoptProblem.objective    ipopt.py:30-35
 *   grad (B,n)       IpoptProblem.gradient     ipopt.py:37-42
 *   g (B,m)          IpoptProblem.constraints  ipopt.py:44-52
 *   jac_dense (B,m,n)IpoptProblem.jacobian     ipopt.py:88-96
 *   jac_tiles (B,H,nx,w*(nx+nu))  compact per-step tiles (rk4.py:85-92 shape; w = rolling_window)
 *   jac_sparse (B,nnz_jac)    values in nempc_jac_structure order */
int nempc_eval(nempc_handle h, int32_t B, const void* Z, const void* X0, void* f, void* grad,
               void* g, void* jac_dense, void* jac_tiles, void* jac_sparse, void* stream);

/* Declares jac -- (B,m,n) of the handle's dtype, device memory -- a RESIDENT dense-Jacobian buffer of this handle.
 * Which entries of the dense Jacobian are structural zeros (98 % of them at H = 20, 2 states, 1 control) depends on the
 * shape and the box rows only, and callers re-evaluate into the same buffer: the zeros need to be written once.
 *   The call fills the buffer with zeros and returns when the fill is complete: it synchronises the device (a set-up
 *   call, not for a captured stream); evaluations on any stream may follow without further ordering.
 *   From then on nempc_eval(..., jac_dense == jac, ...) with at most B problems may write ONLY THE STRUCTURAL NON-ZEROS
 *   (problems beyond the evaluated ones are not touched).  The results are those of the full-matrix path, bit for bit.
 *   The constant non-zeros -- the -1 of every defect row, the +1 of every box row -- are as fixed as the zeros: the first
 *   evaluation that reaches a problem of the buffer writes them (one small launch in front of its own, on its stream),
 *   later ones leave them alone.  (An evaluation on a stream that is being captured before that has happened takes the
 *   full-matrix path.)
 *   ORDERING: that fill runs on the stream of the evaluation that issues it.  An evaluation of the same buffer on ANOTHER
 *   stream skips the constants from then on, so it -- and whoever reads its result -- must be ordered behind that first
 *   evaluation (an event, or a synchronisation), not only behind the registration.
 *   GRAPHS: a graph captured from an evaluation into a registered buffer records the launches of that moment -- without
 *   the zeros, and without the constants once they are in place.  Registering the pointer again (a fresh zero fill),
 *   nempc_set_box_rows and an unregistration followed by foreign writes invalidate such a graph: a replay would leave the
 *   buffer without its zeros / constants.  Capture again after any of them.
 *   The one-launch evaluation of the compiled shapes and the assembly launch behind the generic, layered and
 *   wave-per-tile rows do so; a writer that does not (the cooperative kernel's one-launch dense form) writes the full
 *   matrix into a resident buffer as into any other.
 *   CONTRACT: while the buffer is registered, nobody but nempc_eval of this handle writes it.  The caller may read it.
 *   Unregister it (below) before freeing it or handing it to anyone who writes: the address may come back from the
 *   allocator as somebody else's buffer.
 *   B == 0 removes the registration of jac (a pointer that is not registered: NEMPC_OK, nothing happens).
 *   The table holds 8 buffers per handle.  A ninth registration returns NEMPC_EFULL and changes nothing: not an error
 *   (nempc_last_error is not set), the buffer simply stays on the full-matrix path.
 *   nempc_set_box_rows (m and the pattern change) and nempc_destroy drop every registration of the handle.
 *   A pointer that is not registered behaves as ever: the full matrix is written by every call.
 *   NEMPC_JAC_RESIDENT=0 in the environment (read once per process) makes nempc_eval ignore the table (A/B switch).
 * The ABI version stays 8: nothing existing changed. */
int nempc_jac_dense_resident(nempc_handle h, void* jac, int32_t B);

/* Lagrangian Hessian values, IpoptProblem.hessian ipopt.py:66-86:
 *   hvals (B,nnz_hess) = (sigma_b * d2f + sum_i lambda_{b,i} d2g_i)[rows, cols]
 *   lambda (B,m), sigma (B).  Optional outputs (may be NULL): hdense (B,n,n) full symmetric matrix;
 *   hblocks (B,H,w*(nx+nu),w*(nx+nu)) the per-step blocks sum_k lambda_{t,k} d2 Phi_k / d[x_{t-1}|u_t]^2
 *   (the lambda-contracted form of Model.hessian, model/tensorflow.py:77-109). */
int nempc_hess(nempc_handle h, int32_t B, const void* Z, const void* X0, const void* lambda,
               const void* sigma, void* hvals, void* hdense, void* hblocks, void* stream);

/* Gauss-Newton Hessian callback (BASELINE.json north_star; no reference counterpart -- the reference's Hessian,
 * ipopt.py:66-86, is the exact one above):
 *   hvals (B,nnz_hess) = (sigma_b * d2f + sum_t T_t^T diag(w_{b,t}) T_t)[rows, cols],   T_t = jac tile of step t
 * in the SAME pattern as nempc_hess (nempc_hess_structure): the per-step blocks take the place of the Lagrangian
 * blocks, built from the row kernel's first-order tiles alone (no second-order sweep: one row-kernel launch, one block
 * kernel, one assembly).  w (B, H*nx) positive weights per defect row, NULL = ones; sigma (B).  Positive semidefinite
 * for w >= 0 and a convex objective.  Optional hdense (B,n,n), hblocks (B,H,w*(nx+nu),w*(nx+nu)) as in nempc_hess. */
int nempc_hess_gn(nempc_handle h, int32_t B, const void* Z, const void* X0, const void* w, const void* sigma,
                  void* hvals, void* hdense, void* hblocks, void* stream);

/* Batched on-device solver (no reference counterpart: the reference hands ONE problem at a time to Ipopt /
 * SLSQP on the CPU, optimizer/ipopt.py:138-195, slsqp.py:143-197).  Solves the B problems
 *     min f(z)  s.t.  integrator defects = 0,  lb <= z <= ub
 * in lock step by SQP with the exact per-step Lagrangian blocks (Gauss-Newton on the first iterate): per iterate one
 * callback + Hessian-block evaluation, one regularised Riccati (block-tridiagonal KKT) solve per problem, l1-merit
 * backtracking on defect-only evaluations; finite variable bounds by a primal-dual interior point (barrier parameter
 * mu, multipliers of the bounds updated with their own step length).
 *   X0 (B,nx) device; Z (B,n) device: initial guess in, solution out; lb/ub (n) HOST doubles (NULL = unbounded,
 *   +-INFINITY allowed; the vectors DomainConstraint.get_lower/upper_bounds produce, constraints.py:26-30);
 *   status (B) device int32 out: 0 converged (Optimizer.SUCCESS), 1 not converged (Optimizer.FAIL);
 *   *iters (host, optional) outer iterations run.  Synchronises the stream internally (convergence polls).
 *   Box ROWS (nempc_set_box_rows) are state limits: they are intersected with lb / ub on the state variables (what the
 *   reference's glue would hand Ipopt as constraint rows, optimizer/ipopt.py:44-52, is a bound here).
 *   lb[i] == ub[i] (a fixed variable) is NEMPC_EINVAL: the log barrier needs an interior.
 *   rolling_window > 1: needs nempc_bind_history.  The window is made the state (s_t = the last w states and w-1
 *   controls, w*nx + (w-1)*nu entries) and the same solver runs on that stage-wise problem, the callbacks staying the
 *   window kernels on the caller's variables; one trial step per iteration and no compaction whatever the options say. */
typedef struct nempc_solver_opts {
    int32_t max_iter;        /* outer iterations, e.g. 200 */
    int32_t max_linesearch;  /* halvings of a step before the direction is given up and the next LQ solve damped, e.g. 6 */
    int32_t check_every;     /* period, in iterations, of the BLOCKING convergence poll used for matrix-core-bound stages
                              * (e.g. 4); small stages do not poll: the device publishes the counter every iteration */
    int32_t lq_kernel;       /* LQ solve: 0 auto (by stage size), 1 sweep, one thread per problem, 2 sweep, one wave per problem,
                              * 3 parallel-in-time scan, one lane per stage (2-state / 1-control stages, fp64, H <= 63:
                              * what auto picks there; NEMPC_EUNSUPPORTED elsewhere) */
    double tol_constraint;   /* max |defect| at convergence, e.g. 1e-8 */
    double tol_step;         /* max |dz| <= tol_step * (1 + max |z|), e.g. 1e-8 */
    double mu_init, mu_min, mu_factor; /* barrier schedule, e.g. 1e-1, 1e-9, 0.2 */
    double reg;              /* initial Levenberg term on the control Hessian, e.g. 1e-9 */
    int32_t compact;         /* 1: whenever a quarter of the still-active problems has converged (looked at whenever the
                                convergence counter is read) gather the unconverged ones to the front and launch only over them -- the
                                stragglers then stop costing batch-wide launches; 0: lock step over all B to the end.
                                Results are identical either way (per-problem arithmetic does not depend on the slot). */
    int32_t barrier;         /* bounds: 0 primal-dual interior point (multipliers of the bounds carried along; default),
                                1 primal log barrier (the round-1 method; kept for A/B) */
    int32_t* iters_out;      /* optional device int32 (B): iteration at which each problem converged (0 = did not) */
    int32_t linesearch;      /* 0 auto (deferred for small stages, nx*(nx+nu) < 12, inner loop otherwise), 2 deferred
                                backtracking: ONE trial evaluation per outer iteration for the whole
                                batch; a problem whose trial is rejected stays where it is and retries the same direction at
                                half the length in the next iteration.  In a lock-step batch an inner backtracking loop makes
                                every problem pay for the one that needs six halvings (measured: 5.7 trial evaluations per
                                iteration at B=1024, 70 % of the solve time; at configs[2] dims a trial is 5 % of an iteration and
                                the inner loop converges more problems per second).  1: inner backtracking loop (round 1). */
    int32_t lq_attempts;     /* Riccati sweeps a problem may try per iteration (each restart damps ten times harder) before it
                                keeps its damping and sits the iteration out; 0 = default (3) */
} nempc_solver_opts;

int nempc_solve(nempc_handle h, int32_t B, const void* X0, void* Z, const double* lb, const double* ub,
                const nempc_solver_opts* opts, int32_t* status, int32_t* iters, void* stream);

/* nempc_solve, plus the multipliers the returned iterate carries (Ipopt's mult_g, mult_x_L, mult_x_U; the reference reads
 * none of them back).  lam (B,m), zl (B,n), zu (B,n): device pointers of the handle's dtype, each may be NULL;
 * nempc_solve is this call with three NULLs -- same launches, same results.
 *   Sign convention: g = Phi - x,  L = f + lam.g - zl.(z - lb) + zu.(z - ub),  zl, zu >= 0; stationarity reads
 *       grad f + J' lam - zl + zu = 0.
 *   Which multipliers: those of the RETURNED iterate, lam + alpha (lamn - lam) of the last accepted step (lamn the Riccati
 *   costates of that step's LQ solve) and zl / zu advanced by their own step length -- after max_iter = k full steps they
 *   are the multipliers of Newton step k exactly as Z is the iterate after k steps.  A trial point whose acceptance test
 *   was still outstanding when the loop ended is tested first and counts.  lam is zero when no step was accepted (zl / zu
 *   of a bounded problem then still hold the values the interior point starts from, mu_init / slack at the start).
 *   lam: the first H*nx entries are the defect multipliers in g order; with box rows enabled the H*nx box-row entries
 *   are written as zeros (those limits are bounds for this solver: their multipliers are zl / zu of the state variables),
 *   so lam is what nempc_hess takes.  An infinite bound has multiplier exactly 0.  opts->barrier == 1 (primal barrier, no
 *   bound multipliers carried): zl = mu/(z - lb), zu = mu/(ub - z) with the problem's final mu.  Problems that did not
 *   converge (status 1) return what they hold.  Identical to the bit with compact 0 or 1.
 *   rolling_window > 1 with a non-NULL multiplier pointer: NEMPC_EUNSUPPORTED (the costates of the window state are not
 *   mapped back). */
int nempc_solve_duals(nempc_handle h, int32_t B, const void* X0, void* Z, const double* lb, const double* ub,
                      const nempc_solver_opts* opts, int32_t* status, int32_t* iters, void* lam, void* zl, void* zu,
                      void* stream);

/* KKT residuals of B primal-dual points (any points: a solver's result or not), in the convention above.
 *   Z (B,n), X0 (B,nx), lam (B,m) device, required; zl, zu (B,n) device, NULL = zeros; lb, ub (n) HOST doubles as in
 *   nempc_solve (NULL = unbounded, +-INFINITY allowed), intersected with the box rows on the state variables.
 *   r (B,4) device out, per problem, with T_t = [A_t | B_t] the Jacobian tile of step t:
 *     s_x[t] = grad f_x[t] - lam_t + A_{t+1}' lam_{t+1} (no last term at t = H-1) [+ lam_box[t]] - zl + zu
 *     s_u[t] = grad f_u[t] + B_t' lam_t - zl + zu
 *     r[0] = |s|_inf                                                     stationarity
 *     r[1] = max(|defects|_inf, max_i (lb_i - z_i)+, (z_i - ub_i)+)      primal feasibility
 *     r[2] = max_i over FINITE bounds |zl_i (z_i - lb_i)|, |zu_i (ub_i - z_i)|   complementarity
 *     r[3] = max(0, max_i -zl_i, max_i -zu_i)                            dual feasibility
 *   stat (B,n) device out, optional: s.  Entries of zl / zu on an infinite bound count as zero everywhere.
 * One evaluation by the handle's own kernels (what nempc_eval launches for grad, g, jac_tiles: every kernel family, the
 * extras and tracking bindings, both dtypes) into buffers the handle owns, then one kernel that forms J' lam from the
 * compact tiles and reduces the four norms in double.  Asynchronous on `stream`, except that bounds that differ from the
 * previous call's are uploaded with a stream synchronisation.  Argument checks and codes as nempc_eval (a batch larger
 * than a binding covers: NEMPC_EINVAL); rolling_window > 1: NEMPC_EUNSUPPORTED. */
int nempc_kkt_residual(nempc_handle h, int32_t B, const void* Z, const void* X0, const void* lam, const void* zl,
                       const void* zu, const double* lb, const double* ub, void* r, void* stat, void* stream);

/* Solution sensitivities with respect to the initial state (reference counterpart: none -- the reference never
 * differentiates its solution).  At a primal-dual point (z, lam, zl, zu) the perturbed KKT system
 *     [[W + Sigma, J'], [J, 0]] [dz ; dlam] = -d/dx0 [grad L ; g],   Sigma_i = zl_i/(z_i - lb_i) + zu_i/(ub_i - z_i)
 * (finite bounds only; this also serves the primal barrier's zl = mu/d) is an LQ problem with zero linear terms and initial
 * state dx_{-1} = I: one gain-only backward Riccati sweep (K_t = -Quu_t^-1 Qux_t) and a closed-loop propagation of nx
 * columns (D_{-1} = I, dU_t = K_t D_{t-1}, D_t = A_t D_{t-1} + B_t dU_t, dlam_t = P_t D_t).  Objective second-order
 * terms: Q+Q', QT+QT' at t = H-1, R+R'; a tracking binding changes none of them; extras feed the tiles and blocks only.
 *   Inputs, conventions and bound handling exactly as nempc_kkt_residual: Z (B,n), X0 (B,nx), lam (B,m) device, required
 *   (box-row entries of lam are not read: those limits are bounds here, as in nempc_solve); zl, zu (B,n) device, NULL =
 *   zeros; lb, ub (n) HOST doubles, intersected with the box rows, +-INFINITY allowed.
 *   Outputs: device, dtype of the handle, row-major; each may be NULL, at least one must be given:
 *     dU0   (B,nu,nx)     du_0* / dx0 = K_0
 *     dZ    (B,n,nx)      row i = dz_i / dx0, in z order (states, then controls)
 *     dlam  (B,H*nx,nx)   dlam_t / dx0 = P_t D_t
 *     gains (B,H,nu,nx)   K_t, with du_t = K_t dx_{t-1}
 *   status (B) device int32, required: 0 ok; 1 a pivot of some Quu_t was not positive (the point is not a strict local
 *   minimiser of the barrier problem; NO Levenberg term is ever added: the sensitivity of a regularised problem is a
 *   different number); 2 a finite bound with a non-zero multiplier has gap <= 0 (Sigma is undefined there; a zero
 *   multiplier contributes 0 whatever the gap); 2 takes precedence over 1.  On status != 0 every requested output of that
 *   problem is NaN.
 * One evaluation by the handle's own kernels for the tiles, the Lagrangian blocks from the dispatch nempc_hess uses, then
 * one kernel (one wave per problem) whose arithmetic is double whatever the handle's dtype: with an active bound on a
 * state Sigma reaches 1e11 inside P and single precision loses every digit.  Asynchronous on `stream` apart from the
 * bound upload; checks and codes as nempc_kkt_residual (rolling_window > 1: NEMPC_EUNSUPPORTED; a batch larger than a
 * binding covers: NEMPC_EINVAL). */
int nempc_sensitivity(nempc_handle h, int32_t B, const void* Z, const void* X0, const void* lam, const void* zl,
                      const void* zu, const double* lb, const double* ub, void* dU0, void* dZ, void* dlam, void* gains,
                      int32_t* status, void* stream);

/* KKT solves with caller-supplied right-hand sides (reference counterpart: none).  At a primal-dual point the matrix
 * K = [[W + Sigma, J'], [J, 0]] of nempc_sensitivity is symmetric, so one solve
 *     K [v ; w] = [rz ; rg]
 * is the vector-Jacobian product of the solution map (rz = the cotangent of z*, rg = 0: the cotangent of a parameter theta is
 * -[v ; w]' d/dtheta [grad L ; g]) as well as the forward sensitivity with respect to any parameter
 * (right-hand side -d/dtheta [grad L ; g]).  Per right-hand side, on top of the matrices P_t, K_t, Quu_t = L D L', Qux_t of
 * nempc_sensitivity's backward sweep and with w_t = P_t v_x[t] - p_t, p_{H-1} = r^x_{H-1}:
 *     backward  q_t = P_t r^g_t + p_t,  k_t = Quu_t^-1 (r^u_t + B_t' q_t),  p_{t-1} = r^x_{t-1} + A_t' q_t - Qux_t' k_t
 *     forward   v_u[t] = K_t v_x[t-1] + k_t,  v_x[t] = A_t v_x[t-1] + B_t v_u[t] - r^g_t  (v_x[-1] = 0)
 *     pull-back gx0 = -(W_ux,0' v_u[0] + A_0' w_0) = -[v ; w]' d/dx0 [grad L ; g]
 * nempc_sensitivity is the special case rz = e_i, rg = 0: gx0 is then row i of its dZ.
 *   Z, X0, lam, zl, zu, lb, ub: exactly as nempc_sensitivity (bound handling, box rows, nempc_bind_bounds, the evaluation of
 *   tiles and blocks, argument checks and codes included: rolling_window > 1 NEMPC_EUNSUPPORTED; a batch larger than a
 *   binding covers NEMPC_EINVAL).
 *   nrhs: right-hand sides per problem, 1 <= nrhs <= 64 (else NEMPC_EINVAL; callers chunk larger sets).
 *   rz (B,nrhs,n) device, required: each right-hand side one contiguous row in z order (states, then controls);
 *   rg (B,nrhs,H*nx) device, defect order, NULL = zeros.
 *   Outputs: device, dtype of the handle; each may be NULL, at least one must be given:
 *     v   (B,nrhs,n)      in z order
 *     w   (B,nrhs,H*nx)   in defect order
 *     gx0 (B,nrhs,nx)
 *   status (B) device int32, required: the codes of nempc_sensitivity (0 / 1 / 2, 2 first).  On status != 0 every requested
 *   output of that problem is NaN.  NO Levenberg term is ever added.
 * One evaluation and one Lagrangian-block launch as nempc_sensitivity, then one kernel (one wave per problem, double
 * arithmetic whatever the handle's dtype).  The working sets live in LDS when they fit; when they do not, the call keeps
 * a per-problem region of device memory on the handle, allocated by the first call that needs it and grown when nrhs or
 * max_batch grow: such a call allocates and SYNCHRONISES THE DEVICE, every other call is asynchronous on `stream` apart
 * from the bound upload.  A handle that never calls this function allocates nothing for it.  The call uses
 * nempc_sensitivity's workspaces while it runs: issue both on one stream. */
int nempc_kkt_solve(nempc_handle h, int32_t B, const void* Z, const void* X0, const void* lam, const void* zl,
                    const void* zu, const double* lb, const double* ub, int32_t nrhs, const void* rz, const void* rg, void* v,
                    void* w, void* gx0, int32_t* status, void* stream);

/* Gradient with respect to the network's weights and biases (reference counterpart: none -- the reference never
 * differentiates anything with respect to its model's parameters).  With theta = all weights and biases, xi_{b,t} =
 * [x_{t-1} | u_t | extras_t] the network input of row (b,t), Phi_t the integrator map of the handle, T_t its Jacobian tile
 * and v_[t] = [v_x[t-1] | v_u[t]] (v_x[-1] = 0):
 *     S(theta) = sum_b keep_b sum_t ( w_{b,t} . Phi_t(xi_{b,t}; theta) + lam_{b,t} . ( T_t(xi_{b,t}; theta) v_{b,[t]} ) )
 *     gtheta   = dS / dtheta          (Z, X0, lam, v, w held fixed)
 * g = Phi - x and neither the objective nor the bound terms depend on theta, so gtheta = [v ; w]' d/dtheta [grad L ; g]: with
 * (v, w) from nempc_kkt_solve the cotangent of theta behind the solution map is -gtheta.  With lam = v = NULL the second term
 * drops and gtheta is the gradient of any defect-weighted loss (w = 2 (Phi - x_next): one-step prediction training).
 *   nempc_n_params: P = sum_l (in_l + 1) * out_l.
 *   Z (B,n), X0 (B,nx) device, required; w (B,H*nx) device, defect order, required;
 *   lam (B,m), v (B,n) device, both or neither (one without the other: NEMPC_EINVAL); box-row entries of lam are not read;
 *   skip (B) device int32, optional: a problem with skip[b] != 0 contributes exact zeros -- nothing of it is read, its
 *   lam / v / w may hold NaN, and the result is, to the bit, that of the batch without it;
 *   gtheta (P) device, dtype of the handle, OVERWRITTEN (not accumulated into): [W_0 (in_0,out_0) row-major | b_0 | W_1 | b_1
 *   | ...], the layout of nempc_set_weights.
 * Any network the generic row kernel takes (any widths up to 1024, up to 8 layers, any activation on any layer, extras: inputs
 * of zero tangent whose rows of W_0 receive gradient all the same), Discret / Unity / RK4 (cfg.DT; u and the extras held over
 * the four stages), both dtypes, whatever the handle's row-kernel variant.  One thread-per-row sweep in dual numbers leaves
 * per layer the inputs (a, a.) and pre-activation cotangents (d, d.); dW_l = sum_r a_r (x) d._r + a._r (x) d_r is then a product
 * over all rows on the matrix cores, split over the chip by rows, the partial sums added in a fixed order: no atomics, the
 * result is the same to the bit from call to call.  Rows go in chunks of NEMPC_WGRAD_CHUNK_ROWS (environment, read per
 * call; default: as many as 256 MiB of factors hold), rounded up to whole K slices.
 * Asynchronous on `stream`, except a call that has to allocate or grow the handle's workspace for it: that call
 * SYNCHRONISES THE DEVICE (the first call, and one after max_batch or the chunk size grew).  A handle that never calls this
 * function allocates nothing for it.  Reads the extras binding (B beyond what it covers: NEMPC_EINVAL); rolling_window > 1:
 * NEMPC_EUNSUPPORTED; argument checks and codes otherwise as nempc_eval.  The ABI version stays 8: nothing existing changed. */
int nempc_n_params(nempc_handle h, int64_t* P);
int nempc_weight_grad(nempc_handle h, int32_t B, const void* Z, const void* X0, const void* lam, const void* v,
                      const void* w, const int32_t* skip, void* gtheta, void* stream);

/* Gradient with respect to the extra network inputs p / tvp (reference counterpart: none -- the reference passes p and tvp
 * through its model, Model(p_dim, tvp_dim), NMPC.next(x0, p=, tvp=), and never differentiates with respect to them).  In the
 * notation of nempc_weight_grad, with e_{b,t} row (b,t) of the tensor bound by nempc_bind_extra ([tvp_t ; p]) and
 * xi_{b,t} = [x_{t-1} | u_t | e_{b,t}]:
 *     S_b(E)    = sum_t ( w_{b,t} . Phi_t(xi_{b,t}) + lam_{b,t} . ( T_t(xi_{b,t}) v_{b,[t]} ) )
 *     gE[b,t,:] = dS_b / d e_{b,t}          (Z, X0, lam, v, w, theta held fixed)
 * per row: no sum over t, no sum over b.  A constant parameter p occupies the same slots of every row and its gradient is the
 * caller's sum over t.  g = Phi - x depends on E, the objective and the bound terms do not: with (v, w) from nempc_kkt_solve
 * the cotangent of E behind the solution map is -gE.  With lam = v = NULL the second term drops and gE = w' dPhi/de is the
 * gradient of a defect-weighted loss (one-step-prediction fitting of p).  Under RK4 the extras are held over the four stages,
 * like u, and row (b,t) collects the contributions of all four.
 *   Z (B,n), X0 (B,nx) device, required; w (B,H*nx) device, defect order, required;
 *   lam (B,m), v (B,n) device, both or neither (one without the other: NEMPC_EINVAL); box-row entries of lam are not read;
 *   gE (B,H,n_extra) device, dtype of the handle, OVERWRITTEN.
 * n_extra == 0: NEMPC_EINVAL; rolling_window > 1: NEMPC_EUNSUPPORTED; a missing extras binding or one that covers fewer than
 * B problems: the codes of nempc_eval (NEMPC_ESTATE, NEMPC_EINVAL).  Every refusal names the function in nempc_last_error and
 * leaves the handle usable.  Problems are independent: the rows of a problem do not depend on B nor on what the other
 * problems hold (NaN included), to the bit, and a call is bitwise reproducible (no atomics, one summation order per row).
 * Any network the generic row kernel takes (widths up to 1024, up to 8 layers, any activation on any layer), Discret / Unity
 * / RK4, both dtypes, whatever the handle's row-kernel variant.  One launch: the dual-number sweep of nempc_weight_grad with a
 * row split over 1, 16 or 64 lanes (from the widest layer), s'(z) and s''(z) z. of the backward pass in LDS while they fit and
 * otherwise in a per-workgroup region of a workspace the handle owns.  Asynchronous on `stream`; only the first call of a
 * handle whose plan needs that workspace (and one after max_batch grew) allocates it and SYNCHRONISES THE DEVICE.  A handle
 * that never calls this function allocates nothing for it.  The ABI version stays 8: nothing existing changed. */
int nempc_extra_grad(nempc_handle h, int32_t B, const void* Z, const void* X0, const void* lam, const void* v, const void* w,
                     void* gE, void* stream);

/* launch form of the handle's most recent nempc_extra_grad: lanes per row 1 -> 1, 16 -> 2, 64 -> 3, plus 4 when the saved
 * activation derivatives went to the workspace instead of LDS (5, 6, 7); 0 = none yet */
int nempc_last_extra_grad_kernel(nempc_handle h);

/* Forward simulation of the handle's model (no reference counterpart: the reference never integrates its model over the
 * horizon on its own -- its cold start tiles x0, optimizer/ipopt.py:149, and its examples step the plant outside the library).
 *   Z (B,n) device, in/out: the controls are read from Z[:, H*nx:] and are not written; the states Z[:, :H*nx] are
 *   overwritten with x_t = Phi(x_{t-1}, u_t), x_{-1} = X0, t = 0..H-1, and are NOT read (they may hold anything, NaN included);
 *   X0 (B,nx) device;  f (B) optional: the handle's objective at the rolled-out point (NEMPC_ESTATE without an objective).
 * Phi is the row kernels' map: Discret / Unity / RK4 (u and the extra inputs held over the four stages, cfg.DT), the extra
 * inputs bound by nempc_bind_extra, rolling windows reaching into X0 and the history bound by nempc_bind_history (both
 * orders), any of the NEMPC_ACT_* activations on any layer, both dtypes.  Serial in t, parallel in B: ONE launch, step t
 * reading the states steps < t of the same call produced (they travel in registers / LDS, not through Z).
 * Two kernels: generic (one wave per problem, any dims the handle takes) and matrix-core (one wave per 16 problems for all
 * H steps; hidden widths <= 128, <= 4 hidden layers, any activation mix, nx <= 16, network inputs w*(nx+nu)+n_extra <= 32).
 * By shape the library launches the one that measured faster: the matrix-core kernel when the shape fits it, the hidden
 * widths are <= 64, its weight fragments fit the LDS and the batch gives at least 2.5 tiles per compute unit (its time
 * does not grow with B up to 4 tiles per unit, the generic kernel's does), else the generic kernel.
 * NEMPC_ROLLOUT_KERNEL=1|2 in the environment forces one (read per call); forcing 2 on a shape it does not take is
 * NEMPC_EUNSUPPORTED.  Argument checks and codes as nempc_eval.  Asynchronous on `stream`; does not synchronise the device. */
int nempc_rollout(nempc_handle h, int32_t B, const void* X0, void* Z, void* f, void* stream);

/* kernel the handle's most recent nempc_rollout launched: 1 generic (rollout_wave_kernel), 2 matrix-core
 * (rollout_mfma_kernel); 0 = none yet */
int nempc_last_rollout_kernel(nempc_handle h);

int nempc_sync(nempc_handle h, void* stream);

/* Multi-GPU (no reference counterpart -- the reference has no distributed code).  Ranks own disjoint
 * shards of the problem batch, one process per GPU; nothing on the callback path communicates.  The single exchange
 * is an all-gather of the solved first controls u0 = z[H*nx : H*nx+nu] of every problem, once per MPC step, issued on
 * RCCL (ncclAllGather over xGMI) by the library itself:
 *   nempc_comm_unique_id   rank 0 only: fills id (NEMPC_COMM_ID_BYTES host bytes = an ncclUniqueId); the host side
 *                          hands it to the other ranks (torch.distributed broadcast in pyneuralempc_amd/parallel.py)
 *   nempc_comm_init        every rank, collectively: builds the handle's communicator on the handle's device
 *   nempc_allgather_u0     every rank, collectively, asynchronous on `stream`: packs this rank's u0 -- taken from
 *                          Z (B,n) (what nempc_solve returns), or from u0 (B,nu) when Z is NULL -- into its slot of
 *                          gathered (nranks*rows_per_rank, nu) and all-gathers in place.  rows_per_rank >= B is the
 *                          common slot size (the largest shard when shards are ragged; the pad rows are zero).
 *   nempc_comm_size        nranks / rank of the handle's communicator (0 / -1 when there is none)
 * RCCL is bound at run time on the first of these calls (dlopen librccl.so.1; NEMPC_EUNSUPPORTED when absent). */
#define NEMPC_COMM_ID_BYTES 128
int nempc_comm_unique_id(void* id);
int nempc_comm_init(nempc_handle h, int32_t nranks, int32_t rank, const void* id);
int nempc_allgather_u0(nempc_handle h, int32_t B, int32_t rows_per_rank, const void* Z, const void* u0,
                       void* gathered, void* stream);
int nempc_comm_size(nempc_handle h, int32_t* nranks, int32_t* rank);
int nempc_comm_destroy(nempc_handle h);

/* Launch planning of the cooperative kernels (host arithmetic only, no device needed): ntiles 16-row tiles over
 * per_cu co-resident workgroups on each of num_cus compute units -> grid workgroups, workgroup i owning
 * tiles_per_wg + (i < tiles_rem) consecutive tiles.  The library sizes every chip-filling launch this way from
 * hipDeviceProp_t::multiProcessorCount of the handle's device (nempc_num_cus), never from a literal CU count. */
int nempc_plan_grid(int32_t ntiles, int32_t num_cus, int32_t per_cu, int32_t* grid, int32_t* tiles_per_wg,
                    int32_t* tiles_rem);
int nempc_num_cus(nempc_handle h);

/* which row kernel the handle resolved to (NEMPC_KERNEL_VALU | NEMPC_KERNEL_MFMA | NEMPC_KERNEL_MFMA_TILE |
 * NEMPC_KERNEL_LAYERED) */
int nempc_kernel_variant(nempc_handle h);

/* row kernel the handle's most recent evaluation actually launched: 1 generic (rows_valu_kernel),
 * 2 cooperative matrix-core (rows_coop_kernel), 3 wave-per-tile matrix-core (rows_mfma_kernel), 4 cooperative
 * matrix-core compiled for the problem's shape (rows_coopfx_kernel), 5 rows_coop_kernel writing the dense Jacobian
 * rows itself (no assembly launch), 6 / 7 rows_coopfx_kernel / rows_coop_kernel writing the band-pattern values of the
 * sparse contract itself (no tile round trip, no assembly launch), 8 the layer-at-a-time GEMM pipeline
 * (NEMPC_KERNEL_LAYERED); 0 = none yet */
int nempc_last_row_kernel(nempc_handle h);

/* which kernel wrote the dense Jacobian of the handle's most recent nempc_eval: 0 no dense matrix asked for, 1 the row launch
 * itself (the fused fixed-shape launch, rows_coop_kernel writing the dense rows), 2 assemble_dense_kernel (per-problem
 * grid), 3 post_kernel (the same with the objective blocks), 4 post_flat_kernel (one flat stream of 16-byte vectors, with or
 * without the objective blocks), 5 post_scatter_kernel (a resident matrix: the structural non-zeros alone) */
int nempc_last_dense_writer(nempc_handle h);

/* network kernel the handle's most recent nempc_hess (or solver iteration) launched for the Lagrangian blocks: 1 generic
 * (rowhess_valu_kernel), 2 cooperative matrix-core, forward-over-reverse (rowhess_coop_kernel), 3 wave-per-tile
 * matrix-core (rowhess_mfma_kernel), 4 compiled for the problem's shape, layer-wise contraction (rowhess_coopfx_kernel);
 * 5 the layer-at-a-time GEMM sweeps of wide / deep networks (layered_gemm_kernel + layered_hcontract_kernel);
 * + 10 when it ran inside the RK4 pipeline (stage records, stage multipliers, that kernel in direct mode, congruence
 * sum: integrator/rk4.py:181-285); 0 = none yet */
int nempc_last_hess_kernel(nempc_handle h);

/* LQ kernel the handle's most recent nempc_solve planned for its iterations: 1 thread per problem, working set in global
 * memory (it does not fit the LDS budget; a requested wave or scan kernel ends here too), 2 thread per problem, working set
 * staged in LDS, 3 wave per problem in LDS, 4 parallel-in-time scan (2-state / 1-control stages, fp64); 0 = none yet */
int nempc_last_lq_kernel(nempc_handle h);

const char* nempc_last_error(void);
int nempc_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* NEMPC_H */
