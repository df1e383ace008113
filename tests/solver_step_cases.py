"""Shapes, networks, objectives and starts of the per-step solver checks  --  TEST INFRASTRUCTURE, not a test.

Shared by tests/test_kkt_reference_cpu.py (the reference checks itself on these shapes) and tests/test_gpu_solver_steps.py
(the solver against the reference).  Everything is seeded; references are computed once per case and cached.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import nempc_oracle as orc
import kkt_reference as kkt

REG = 1e-9          # the Levenberg term every solve here passes (fp64: the solver's default, and its floor)
BMAX = 16
REF_SCALE = 0.1     # standard deviation of the per-stage xref, uref, cx, cu
KINDS = {"discret": orc.DISCRET, "unity": orc.UNITY, "rk4": orc.RK4}

# The smallest horizon at which plan_lq (csrc/solver.hip) no longer stages a 2/1 fp64 problem in LDS with lq_kernel =
# "thread": per problem (48 H + 37) doubles at one damping level (39 H of iterate / tiles / blocks / steps, 9 H + 36 of one
# attempt's gains and temporaries, made odd) against a budget of 150 KiB (kLqLdsBudget, csrc/nempc_internal.h; counted
# here on its own) minus 2 n doubles:
#     8 (48 H + 37) <= 153600 - 48 H   <=>   H <= 354
H_GLOBAL = 355


def lds_bytes(nx, nu, H, dtype="float64", levels=1):
    """(bytes one problem needs, budget of a workgroup) of the LQ sweep with `levels` damping levels side by side --
    plan_lq's sizes (csrc/solver.hip): the working set is staged in LDS when the first is at most the second."""
    nin = nx + nu
    n = H * nin
    size = {"float64": 8, "float32": 4}[dtype]
    tmp = 3 * nx * nx + 3 * nx * nu + nu * nu + 5 * nx + 3 * nu + 1 + (nx + 1) * nu
    att = H * nu * nx + H * nu + H * nx * nx + H * nx + tmp
    per = (2 * n + 2 * H * nx + H * nx * nin + H * nin * nin + n + n + H * nx + 2 * n + levels * att) | 1
    return size * per, 150 * 1024 - 2 * n * size


def lds_bytes_2x1_thread(H):
    """(bytes one problem needs, budget) of the 2/1 fp64 thread-per-problem sweep at one damping level -- plan_lq's sizes."""
    return lds_bytes(2, 1, H, "float64", 1)


def expected_lq_plan(nx, nu, H, dtype, kernel, scan_default=True):
    """The plan (CallbackEngine.last_lq_kernel: "thread_global" | "thread_lds" | "wave_lds" | "scan") the size formula
    predicts for a requested lq_kernel -- plan_lq's decision restated: the wave kernel is
    wanted when forced, or under "auto" at nx (nx + nu) >= 12, and then sweeps one damping level; the thread kernel asks for
    three levels side by side and gives them up one by one until the problem fits; whatever was asked for, a working set
    over the budget runs thread per problem from global memory.  The scan is built for 2/1 fp64 stages with H <= 63 and is
    what "auto" takes there (scan_default: the solver's NEMPC_LQ_SCAN knob, on unless the environment says otherwise)."""
    wave = kernel == "wave" or (kernel in ("auto", "scan") and nx * (nx + nu) >= 12)
    scan_fits = dtype == "float64" and (nx, nu) == (2, 1) and H + 1 <= 64
    scan = scan_fits and (kernel == "scan" or (kernel == "auto" and scan_default))
    need, budget = lds_bytes(nx, nu, H, dtype, 0 if scan else 1)
    if need > budget:
        return "thread_global"
    return "wave_lds" if wave else ("scan" if scan else "thread_lds")


# ---- (a) one Newton step on an equality-constrained convex QP: linear networks.
# name: (nx, nu, hidden, integrator, DT, horizons, lq kernels, dtype, window, forward_rolling, n_extra)
QP_ROWS = {
    "2x1_discret":   (2, 1, [32], "discret", 1.0, (1, 2, 3, 20, 63), ("thread", "wave", "scan", "auto"), "float64", 1, True, 0),
    "2x1_global":    (2, 1, [32], "discret", 1.0, (H_GLOBAL,), ("thread",), "float64", 1, True, 0),
    "6x3_rk4":       (6, 3, [16, 16], "rk4", 0.1, (8,), ("thread", "wave", "auto"), "float64", 1, True, 0),
    "3x2_unity":     (3, 2, [8], "unity", 1.0, (7,), ("thread", "wave"), "float64", 1, True, 0),
    "5x2_one_layer": (5, 2, [], "rk4", 0.1, (9,), ("auto",), "float64", 1, True, 0),
    "roll3_fwd":     (2, 1, [8], "discret", 1.0, (10,), ("auto",), "float64", 3, True, 0),
    "roll3_rev":     (2, 1, [8], "discret", 1.0, (10,), ("auto",), "float64", 3, False, 0),
    "2x1_extras":    (2, 1, [8], "discret", 1.0, (10,), ("auto",), "float64", 1, True, 2),
    "2x1_fp32":      (2, 1, [32], "discret", 1.0, (20,), ("thread", "wave"), "float32", 1, True, 0),
    # wide stages: more matrix entries than lanes, every LQ plan (lds_bytes: fp64 bytes per problem against ~150 KiB)
    "12x5_discret":  (12, 5, [16], "discret", 1.0, (4,), ("thread", "wave", "auto"), "float64", 1, True, 0),    # 33 KB: several per workgroup
    "3x8_discret":   (3, 8, [8], "discret", 1.0, (5,), ("thread", "wave", "auto"), "float64", 1, True, 0),      # nu > nx: 8 x 8 Quu
    "16x4_rk4":      (16, 4, [8], "rk4", 0.1, (4,), ("thread", "wave", "auto"), "float64", 1, True, 0),         # 48 KB
    "20x4_discret":  (20, 4, [8], "discret", 1.0, (6,), ("thread", "wave", "auto"), "float64", 1, True, 0),     # 98 KB: one per workgroup, > 64 KiB
    "33x3_unity":    (33, 3, [8], "unity", 1.0, (3,), ("thread", "wave"), "float64", 1, True, 0),               # 127 KB, nx > 32
    "40x10_discret": (40, 10, [8], "discret", 1.0, (3,), ("thread", "auto"), "float64", 1, True, 0),            # 221 KB: global memory
    "40x10_fp32":    (40, 10, [8], "discret", 1.0, (3,), ("thread", "wave"), "float32", 1, True, 0),            # 111 KB: the same shape in LDS
    "64x8_discret":  (64, 8, [8], "discret", 1.0, (1, 3), ("auto",), "float64", 1, True, 0),                    # global memory (H = 3)
    "64x8_fp32":     (64, 8, [8], "discret", 1.0, (1,), ("thread", "wave"), "float32", 1, True, 0),             # 119 KB: LDS at 64 states
    "70x3_discret":  (70, 3, [8], "discret", 1.0, (2,), ("auto",), "float64", 1, True, 0),                      # more states than lanes
}
# (one seed for every row.  It matters at H = 355 only: of the seeds 0..11 this one gives the 2/1 Discret dynamics I + 0.1 W the
#  smallest spectral radius, 1.0007 -- a mode of 1.015 grows 200-fold over 355 stages and takes the conditioning with it)
QP_SEED = 1
QP_CASES = [(name, H) for name, row in QP_ROWS.items() for H in row[5]]
QP_RANDOM_START = {("2x1_discret", 20), ("6x3_rk4", 8), ("12x5_discret", 4), ("20x4_discret", 6)}      # also run from a random Z_init

# ---- (b) three steps of a nonlinear solve: tanh networks, output layer scaled by 0.1, X0 in +-0.5, 8 problems
# name: (nx, nu, hidden, integrator, DT, H, lq kernels, dtype, steps)
NL_ROWS = {
    "2x1_h20":   (2, 1, [64, 64], "discret", 1.0, 20, ("thread", "wave", "scan", "auto"), "float64", 3),
    "2x1_h63":   (2, 1, [64, 64], "discret", 1.0, 63, ("thread", "wave", "scan", "auto"), "float64", 3),
    "6x3_rk4":   (6, 3, [32, 32], "rk4", 0.1, 8, ("thread", "wave", "auto"), "float64", 3),
    "3x2_unity": (3, 2, [24], "unity", 1.0, 7, ("thread", "wave", "auto"), "float64", 3),
    "5x2_h9":    (5, 2, [16, 16], "discret", 1.0, 9, ("thread", "wave", "auto"), "float64", 3),
    "6x3_fp32":  (6, 3, [32, 32], "rk4", 0.1, 8, ("thread", "wave", "auto"), "float32", 2),
    # wide stages (seed 0).  16x4_rk4 and 70x3_h2: some reference steps are below STOP_STEP by the third step
    "12x5_h4":   (12, 5, [16], "discret", 1.0, 4, ("thread", "wave", "auto"), "float64", 3),
    "20x4_h6":   (20, 4, [24], "discret", 1.0, 6, ("thread", "wave", "auto"), "float64", 3),
    "16x4_rk4":  (16, 4, [16, 16], "rk4", 0.1, 4, ("wave", "auto"), "float64", 3),
    "40x10_h3":  (40, 10, [16], "discret", 1.0, 3, ("auto",), "float64", 3),
    "70x3_h2":   (70, 3, [16], "discret", 1.0, 2, ("auto",), "float64", 3),
}
NL_B = 8
# Problems (of NL_B) whose reference steps 1..3 are all at least STOP_STEP, i.e. that are still compared at the third step,
# where that is not at least 5 (the bar of the multiplier test): wide stages converge faster than the small ones
# (asserted from the reference in tests/test_kkt_reference_cpu.py; steps 1 and 2 compare every problem on every row)
NL_STEP3_COMPARED = {"16x4_rk4": 2}
GATE_EIG = 0.05          # reduced-Hessian eigenvalue below which the sweep could restart with damping
STOP_STEP = 1e-6         # a reference step below this is at the convergence test: the solver rightly stands still


def _round(a, dtype):
    """Values as the handle holds them: an fp32 handle solves the problem with fp32-rounded data."""
    return np.asarray(a, dtype=np.float64) if dtype == "float64" else np.asarray(a, dtype=np.float32).astype(np.float64)


def objective(nx, nu, H, seed, dtype="float64", r_diag=0.3):
    """Non-symmetric Q = I + 0.1 N, R = r_diag I + 0.03 N (0.3; negative in the damped cases), QT = 2 I + 0.1 N (N seeded
    standard normal), random per-stage xref, uref, cx, cu."""
    rng = np.random.default_rng(seed)
    ob = dict(Q=np.eye(nx) + 0.1 * rng.normal(size=(nx, nx)), R=r_diag * np.eye(nu) + 0.03 * rng.normal(size=(nu, nu)),
              QT=2.0 * np.eye(nx) + 0.1 * rng.normal(size=(nx, nx)), xref=REF_SCALE * rng.normal(size=(H, nx)),
              uref=REF_SCALE * rng.normal(size=(H, nu)), cx=REF_SCALE * rng.normal(size=(H, nx)), cu=REF_SCALE * rng.normal(size=(H, nu)))
    return {k: _round(v, dtype) for k, v in ob.items()}


class Case:
    """One shape: the network, the objective, BMAX starts and per-problem oracle Problems."""

    def __init__(self, name, nx, nu, hidden, integ, DT, H, kernels, dtype, window=1, forward=True, n_extra=0,
                 act="linear", seed=0, B=BMAX, scale_b=False, x0_range=0.5, out_scale=0.1, r_diag=0.3):
        self.name, self.nx, self.nu, self.H, self.integ, self.DT = name, nx, nu, H, integ, DT
        self.kernels, self.dtype, self.window, self.forward, self.n_extra, self.B = kernels, dtype, window, forward, n_extra, B
        n_in = window * (nx + nu) + n_extra
        net = orc.MLP.random(n_in, hidden, nx, seed=seed, activations=act)
        if integ == "discret" or act != "linear":
            net.W[-1] *= out_scale
            if scale_b:
                net.b[-1] *= out_scale
        net.W = [_round(w, dtype) for w in net.W]
        net.b = [_round(b, dtype) for b in net.b]
        self.net = net
        self.obj = objective(nx, nu, H, seed + 100, dtype, r_diag)
        rng = np.random.default_rng(seed + 200)
        self.X0 = _round(rng.uniform(-x0_range, x0_range, size=(B, nx)), dtype)
        self.extra = _round(0.5 * rng.normal(size=(B, H, n_extra)), dtype) if n_extra else None
        self.hist_x = _round(rng.uniform(-0.5, 0.5, size=(B, window - 1, nx)), dtype) if window > 1 else None
        self.hist_u = _round(rng.uniform(-0.5, 0.5, size=(B, window - 1, nu)), dtype) if window > 1 else None
        self.n = H * (nx + nu)
        self.Zrand = _round(np.concatenate([rng.uniform(-0.5, 0.5, size=(B, H * nx)), rng.uniform(-0.5, 0.5, size=(B, H * nu))],
                                           axis=1), dtype)

    def problem(self, b):
        roll = {} if self.window == 1 else dict(window=self.window, forward_rolling=self.forward, hist_x=self.hist_x[b],
                                                hist_u=self.hist_u[b])
        return orc.Problem(self.net, self.H, self.nx, self.nu, KINDS[self.integ], self.DT,
                           extra=None if self.extra is None else self.extra[b], **self.obj, **roll)

    def start(self, b, random_start=False):
        return self.Zrand[b].copy() if random_start else orc.cold_start(self.X0[b], self.H, self.nu)

    def engine(self, **kw):
        """The device handle of this case (GPU tests only)."""
        import torch
        from pyneuralempc_amd import CallbackEngine
        dt = {"float64": torch.float64, "float32": torch.float32}[self.dtype]
        eng = CallbackEngine(self.net.W, self.net.b, self.H, self.nx, self.nu, integrator=self.integ, DT=self.DT, dtype=dt,
                             device="cuda:0", max_batch=self.B, n_extra=self.n_extra, rolling_window=self.window,
                             forward_rolling=self.forward, activations=self.net.act, **kw)
        eng.set_objective(**self.obj)
        return eng

    def bind(self, eng, B):
        """Per-problem data of the first B problems: extras / history bound on the handle; returns X0 on the device."""
        if self.n_extra:
            eng.bind_extra(eng.to_device(self.extra[:B]))
        if self.window > 1:
            eng.bind_history(eng.to_device(self.hist_x[:B]), eng.to_device(self.hist_u[:B]))
        return eng.to_device(self.X0[:B])


@functools.lru_cache(maxsize=None)
def qp_case(name, H):
    nx, nu, hidden, integ, DT, _, kernels, dtype, window, forward, n_extra = QP_ROWS[name]
    return Case(name, nx, nu, hidden, integ, DT, H, kernels, dtype, window, forward, n_extra, act="linear",
                seed=QP_SEED)


@functools.lru_cache(maxsize=None)
def nl_case(name):
    nx, nu, hidden, integ, DT, H, kernels, dtype, _ = NL_ROWS[name]
    return Case(name, nx, nu, hidden, integ, DT, H, kernels, dtype, act="tanh", seed=NL_SEEDS.get(name, 0), B=NL_B, scale_b=True)


# (seeds at which the REFERENCE clears both gates of (b) for all 8 problems and all three steps; of the seeds 0..7 the 2/1
#  Discret network clears them at 1, 2 and 6 -- at the others a reference step meets an indefinite reduced Hessian or raises
#  the merit, which is the damped / shortened territory test (b) leaves out; the damped part is cases (e), (f), (g) below)
NL_SEEDS = {"2x1_h20": 1, "2x1_h63": 1}


def np_dtype(case):
    return np.float64 if case.dtype == "float64" else np.float32


def step_tolerance(e, z):
    """Ten times what a correct sweep in the handle's precision loses on this system, floored at
    1e-12 (1 + |z|inf)."""
    return max(10.0 * e, 1e-12 * (1.0 + float(np.abs(z).max())))


@functools.lru_cache(maxsize=None)
def qp_reference(name, H, random_start=False):
    """Per problem of the case: (z0, dz_ref, lam_ref, tolerance, e) -- float64 dense Newton step from the start, and the
    tolerance from the Riccati sweep in the handle's precision."""
    case = qp_case(name, H)
    out = []
    for b in range(case.B):
        prob, x0 = case.problem(b), case.X0[b]
        z0 = case.start(b, random_start)
        dz, lam, _, _ = kkt.newton_step(prob, z0, x0, np.zeros(H * case.nx), REG, diagnostics=False)
        dzr, _ = kkt.riccati_step(prob, z0, x0, np.zeros(H * case.nx), REG, np_dtype(case))
        e = float(np.abs(dzr - dz).max())
        out.append((z0, dz, lam, step_tolerance(e, z0 + dz), e))
    return out


@functools.lru_cache(maxsize=None)
def nl_reference(name):
    """Per problem: the replayed steps (kkt.replay) and the cumulative sweep error in the handle's precision."""
    case = nl_case(name)
    steps = NL_ROWS[name][8]
    out = []
    for b in range(case.B):
        prob, x0 = case.problem(b), case.X0[b]
        z0 = case.start(b)
        out.append((kkt.replay(prob, x0, z0, steps, REG), kkt.sweep_error(prob, x0, z0, steps, REG, np_dtype(case))))
    return out


# ---- (c) bounded convex QP: linear networks, tight control bounds, wide state bounds, one state limit from the box rows
# name: (nx, nu, hidden, integrator, DT, H, seed)
BOUNDED_ROWS = {
    "2x1_h12": (2, 1, [32], "discret", 1.0, 12, 1),
    "3x2_h7":  (3, 2, [8], "unity", 1.0, 7, 1),
    "20x4_h6": (20, 4, [8], "discret", 1.0, 6, 1),
    "40x10_h3": (40, 10, [8], "discret", 1.0, 3, 1),
}
# The rows the central-path consumers keep (tests/test_sensitivity_reference_cpu.py, tests/test_kkt_solve_reference_cpu.py and
# the bounded test of test_gpu_sensitivity.py): they place a synthetic point at mu = 2.5e-9 next to
# the exact solution and hold the float64 references to absolute bars there (riccati - dense <= 1e-5, dense - active set <=
# 1e-4).  On the wide rows the float64 references alone miss those bars -- 15 .. 17 active bounds with multipliers down to
# 1.2e-3 put Sigma up to 2.5e11 into P: dense - active set is 3.5e-4 (20x4_h6) and 5.3e-3 (40x10_h3), the affine recursion is
# 1.6e-5 from the dense solve on 20x4_h6 problem 2 -- so those constructions cannot form the wide cases; the wide rows'
# end points, multipliers and certificates are checked in test_gpu_solver_steps.py and test_gpu_duals.py.
BOUNDED_SMALL = ("2x1_h12", "3x2_h7")
BOUNDED_B = 4
STATE_WIDE = 5.0
NU_MIN = 1e-3            # smallest active bound multiplier the reference must show (strict complementarity with a margin)


def slsqp(prob, x0, lb, ub):
    """SciPy SLSQP on the oracle's callbacks (defect rows as equalities, lb / ub as bounds)."""
    import warnings
    from scipy.optimize import Bounds, minimize
    m = prob.H * prob.nx
    zi = np.clip(orc.cold_start(x0, prob.H, prob.nu), lb, ub)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return minimize(prob.objective, zi, method="SLSQP", jac=prob.gradient, bounds=Bounds(lb, ub),
                        constraints=[{"type": "eq", "fun": lambda z: prob.constraints(z, x0)[:m],
                                      "jac": lambda z: prob.jacobian(z, x0)[:m]}],
                        options={"maxiter": 500, "ftol": 1e-14})


@functools.lru_cache(maxsize=None)
def bounded_case(name):
    """(case of BOUNDED_B problems, lb, ub as the solver ends up with them, what the handle is given: dict(lb, ub, box_lo,
    box_hi)).  The control limit is 40 % of the largest unconstrained control of problem 0; the box rows cap state 0 a tenth of its range
    under the highest value it reaches in problem 0's control-bounded solution; of a seeded pool of starts the first
    BOUNDED_B are kept whose REFERENCE solution has at least two controls on a bound and no active multiplier under NU_MIN
    (problem 0, which the limits were cut for, among them)."""
    nx, nu, hidden, integ, DT, H, seed = BOUNDED_ROWS[name]
    pool = Case(name, nx, nu, hidden, integ, DT, H, ("auto",), "float64", act="linear", seed=seed, B=32)
    n = pool.n
    p0, x00 = pool.problem(0), pool.X0[0]
    dz, _, _, _ = kkt.newton_step(p0, pool.start(0), x00, np.zeros(H * nx), REG, diagnostics=False)
    umax = float(np.abs((pool.start(0) + dz)[H * nx:]).max())
    c = round(0.4 * umax, 3)
    lb = np.concatenate([np.full(H * nx, -STATE_WIDE), np.full(H * nu, -c)])
    ub = -lb
    z1, _, _, _ = kkt.qp_solution(p0, x00, lb, ub)
    xs = z1[:H * nx].reshape(H, nx)
    cap = round(float(xs[:, 0].max()) - 0.1 * float(np.ptp(xs[:, 0])), 3)
    box_lo, box_hi = np.full(nx, -STATE_WIDE), np.full(nx, STATE_WIDE)
    box_hi[0] = cap
    lbe, ube = lb.copy(), ub.copy()
    ube[:H * nx] = np.minimum(ube[:H * nx], np.tile(box_hi, H))
    keep = []
    for b in range(pool.B):
        try:
            z, lam, nlo, nhi = kkt.qp_solution(pool.problem(b), pool.X0[b], lbe, ube)
        except (RuntimeError, AssertionError, np.linalg.LinAlgError):
            continue                              # (infeasible under the cap from this start)
        act = np.concatenate([nlo[nlo > 0], nhi[nhi > 0]])
        if ((nlo + nhi)[H * nx:] > 0).sum() >= 2 and act.min() >= NU_MIN:
            keep.append(b)
        if len(keep) == BOUNDED_B:
            break
    assert len(keep) == BOUNDED_B and keep[0] == 0, keep
    case = Case(name, nx, nu, hidden, integ, DT, H, ("auto",), "float64", act="linear", seed=seed, B=32)
    case.X0, case.B = pool.X0[keep].copy(), BOUNDED_B
    return case, lbe, ube, dict(lb=lb, ub=ub, box_lo=box_lo, box_hi=box_hi)


@functools.lru_cache(maxsize=None)
def bounded_reference(name):
    case, lbe, ube, _ = bounded_case(name)
    return [kkt.qp_solution(case.problem(b), case.X0[b], lbe, ube) for b in range(case.B)]


# ---- (d) second-order correction of a rejected full step (solver_soc_kernel): tanh networks, output layer NOT scaled down,
# 8 problems, X0 in +-SOC_X0_RANGE, start = the roll-out of seeded controls in +-SOC_U_RANGE.
# The start is feasible on purpose.  From the cold start the first full step removes defects of order one and lowers the l1
# merit for every problem at every scale tried on the CPU (output layer x 1, 2, 4; X0 in +-0.5 .. +-30; seeds 0, 1); the
# correction is for the Maratos setting: at a feasible point a full step along the curved constraints leaves second-order
# defects, the penalty 1.5 |lam+|inf (13 .. 43 here) times them outweighs the objective's decrease and the step is rejected.
# name: (nx, nu, hidden, integrator, DT, H)
SOC_ROWS = {
    "6x3_rk4": (6, 3, [32, 32], "rk4", 0.1, 8),
    "64x8_h3": (64, 8, [16], "discret", 1.0, 3),
    "70x3_h2": (70, 3, [16], "discret", 1.0, 2),
}
SOC_B, SOC_SEED, SOC_X0_RANGE, SOC_U_RANGE = 8, 0, 1.0, 0.5
MAX_LINESEARCH = 6       # CallbackEngine.solve's default: trial lengths 1, 1/2, .., 2^-5


@functools.lru_cache(maxsize=None)
def soc_case(name):
    nx, nu, hidden, integ, DT, H = SOC_ROWS[name]
    return Case(name, nx, nu, hidden, integ, DT, H, ("auto",), "float64", act="tanh", seed=SOC_SEED, B=SOC_B,
                x0_range=SOC_X0_RANGE, out_scale=1.0)


def rollout(prob, x0, U):
    """z = [x_1 .. x_H ; U] with x_t = Phi(x_{t-1}, u_t): zero defects."""
    H, nx = prob.H, prob.nx
    z = np.concatenate([np.zeros(H * nx), np.asarray(U, dtype=np.float64).ravel()])
    for t in range(H):
        z[t * nx:(t + 1) * nx] = prob.tiles(z, x0)[1][t]
    return z


def soc_correction(prob, z0, zt, x0):
    """The state-only recursion dx_t = A_t dx_{t-1} + c+_t with the Jacobian tiles at z0 and the defects at the trial point
    zt, as a z-shaped vector (zero on the controls)."""
    H, nx = prob.H, prob.nx
    dphi = prob.tiles(z0, x0)[2]
    c = prob.constraints(zt, x0)[:H * nx].reshape(H, nx)
    out, dx = np.zeros(prob.n), np.zeros(nx)
    for t in range(H):
        dx = dphi[t][:, :nx] @ dx + c[t]
        out[t * nx:(t + 1) * nx] = dx
    return out


@functools.lru_cache(maxsize=None)
def soc_reference(name):
    """Per problem: z0 (the feasible start), dz (the dense Newton step from it), tol (step_tolerance of that step), raises
    (the full step raises the l1 merit under the solver's penalty max(1, 1.5 |lam+|inf + 1e-3)) and cands: the finite set of
    points one iteration with inner-loop backtracking can return, [(label, point)] -- the full step, the corrected point,
    z0 + 2^-k dz for k = 1 .. MAX_LINESEARCH, and z0 itself."""
    case = soc_case(name)
    H, nx, nu = case.H, case.nx, case.nu
    rng = np.random.default_rng(SOC_SEED + 300)
    out = []
    for b in range(case.B):
        prob, x0 = case.problem(b), case.X0[b]
        z0 = rollout(prob, x0, rng.uniform(-SOC_U_RANGE, SOC_U_RANGE, size=(H, nu)))
        dz, lam, _, eig = kkt.newton_step(prob, z0, x0, np.zeros(H * nx), REG)
        dzr, _ = kkt.riccati_step(prob, z0, x0, np.zeros(H * nx), REG, np.float64)
        pen = max(1.0, 1.5 * float(np.abs(lam).max()) + 1e-3)
        cands = [("full", z0 + dz), ("corrected", z0 + dz + soc_correction(prob, z0, z0 + dz, x0))]
        cands += [(f"half^{k}", z0 + 2.0 ** -k * dz) for k in range(1, MAX_LINESEARCH + 1)] + [("start", z0)]
        out.append(dict(z0=z0, dz=dz, eig=eig, pen=pen, cands=cands, tol=step_tolerance(float(np.abs(dzr - dz).max()), z0 + dz),
                        raises=kkt.l1_merit(prob, z0 + dz, x0, pen) > kkt.l1_merit(prob, z0, x0, pen)))
    return out


# ---- (e) one damped step of an indefinite QP: the rows of QP_ROWS below with R = DAMPED_R_DIAG I + 0.03 N.  With lam0 = 0 and a
# linear network Quu_t does not depend on the problem: lambda, the smallest reg at which the sweep goes through (bisection
# on the reference, problem 0, the handle's precision), is one number per row, and reg0 = lambda sqrt(10)^(0.5 - k*) puts level
# k* half a rung above it and level k* - 1 half a rung below.  lambda per row, from the CPU (the horizons of a row agree to
# five digits):
#   2x1_discret H=20, 31, 63  0.3177    6x3_rk4 0.4880     3x2_unity 0.3822     roll3_fwd 0.3186    12x5_discret 0.4188
#   20x4_discret 0.4188       40x10_discret 0.5001         70x3_discret 0.5479  2x1_fp32 0.3177     40x10_fp32 0.5001
#   64x8_fp32 0.3692
# (name, H): the lq kernels taken there -- those of the row's QP_ROWS entry; at 2/1 H = 31 and 63 thread and scan, where the
# scan fits 2 and 1 levels side by side (3 at H = 20).
DAMPED_R_DIAG = -0.15
DAMPED_QP = {
    ("2x1_discret", 20): QP_ROWS["2x1_discret"][6], ("2x1_discret", 31): ("thread", "scan"), ("2x1_discret", 63): ("thread", "scan"),
    ("6x3_rk4", 8): QP_ROWS["6x3_rk4"][6], ("3x2_unity", 7): QP_ROWS["3x2_unity"][6], ("roll3_fwd", 10): QP_ROWS["roll3_fwd"][6],
    ("12x5_discret", 4): QP_ROWS["12x5_discret"][6], ("20x4_discret", 6): QP_ROWS["20x4_discret"][6],
    ("40x10_discret", 3): QP_ROWS["40x10_discret"][6], ("70x3_discret", 2): QP_ROWS["70x3_discret"][6],
    ("2x1_fp32", 20): QP_ROWS["2x1_fp32"][6], ("40x10_fp32", 3): QP_ROWS["40x10_fp32"][6], ("64x8_fp32", 1): QP_ROWS["64x8_fp32"][6],
}
DAMPED_KSTAR = (1, 2, 4)            # the level that wins, counted from the reg the solve is given
DAMPED_ATTEMPTS = (1, 3, 5)         # lq_attempts; with 5 and three levels side by side k* = 4 wins in the second round
DAMPED_SMALL_B = (1, 2, 3)          # at (k* = 2, lq_attempts = 3); every other combination at B = BMAX


def iterations_needed(kstar, attempts):
    """The iteration at which level k* of the ladder is reached when every iteration tries `attempts` levels."""
    return kstar // attempts + 1


@functools.lru_cache(maxsize=None)
def damped_qp_case(name, H):
    nx, nu, hidden, integ, DT, _, _, dtype, window, forward, n_extra = QP_ROWS[name]
    return Case(name, nx, nu, hidden, integ, DT, H, DAMPED_QP[(name, H)], dtype, window, forward, n_extra, act="linear",
                seed=QP_SEED, r_diag=DAMPED_R_DIAG)


@functools.lru_cache(maxsize=None)
def damped_qp_lambda(name, H):
    case = damped_qp_case(name, H)
    return kkt.min_passing_reg(case.problem(0), case.start(0), case.X0[0], np.zeros(H * case.nx), np_dtype(case))


@functools.lru_cache(maxsize=None)
def damped_qp_reference(name, H, kstar):
    """dict(reg0: what the solve is given, reg_k: level k* of its ladder, probs: per problem (z0, dz at reg_k, lam+,
    tolerance, sweep error e at reg_k in the handle's precision, dmerit of the full step))."""
    case = damped_qp_case(name, H)
    reg0 = damped_qp_lambda(name, H) * kkt.REG_RAISE ** (0.5 - kstar)
    reg_k = kkt.damping_levels(reg0, kstar)[kstar]
    lam0 = np.zeros(H * case.nx)
    probs = []
    for b in range(case.B):
        prob, x0, z0 = case.problem(b), case.X0[b], case.start(b)
        dz, lam, _, _ = kkt.newton_step(prob, z0, x0, lam0, reg_k, diagnostics=False)
        dzr, _ = kkt.riccati_step(prob, z0, x0, lam0, reg_k, np_dtype(case))
        e = float(np.abs(dzr - dz).max())
        pen = max(1.0, 1.5 * float(np.abs(lam).max()) + 1e-3)
        dmerit = kkt.l1_merit(prob, z0 + dz, x0, pen) - kkt.l1_merit(prob, z0, x0, pen)
        probs.append((z0, dz, lam, step_tolerance(e, z0 + dz), e, dmerit))
    return dict(reg0=reg0, reg_k=reg_k, probs=probs)


# the relaxation rule: (e) rows and kernels at lq_attempts = 1 (sit, sit, step, sit, step from k* = 2) ...
RELAX_ROWS = {("2x1_discret", 20): ("thread", "scan"), ("6x3_rk4", 8): ("wave",), ("12x5_discret", 4): ("thread",),
              ("2x1_fp32", 20): ("wave",)}
RELAX_KSTAR, RELAX_BUDGETS, RELAX_B = 2, 5, 4


@functools.lru_cache(maxsize=None)
def relax_reference(name, H, attempts=1, kstar=RELAX_KSTAR, budgets=RELAX_BUDGETS):
    """Per problem (of the first RELAX_B): (damped_replay over `budgets` iterations from reg0 of (e) at k*, cumulative sweep
    error)."""
    case = damped_qp_case(name, H)
    reg0 = damped_qp_reference(name, H, kstar)["reg0"]
    out = []
    for b in range(RELAX_B):
        prob, x0 = case.problem(b), case.X0[b]
        rp = kkt.damped_replay(prob, x0, case.start(b), budgets, reg0, attempts, np_dtype(case))
        out.append((rp, kkt.sweep_error_damped(prob, x0, rp, np_dtype(case))))
    return reg0, out


# ---- (f) mixed levels inside one launch: tanh networks at the first step (lam0 = 0: the blocks are zero and Quu_t = R + R' + reg
# + B_t' P B_t varies with the problem through B_t), output layer not scaled down, X0 in +-1, B = 16, seed 0, fp64.
# name: (nx, nu, hidden, integrator, DT, H, lq kernels, diagonal of R, reg0)
MIXED_ROWS = {
    "2x1_h20": (2, 1, [64, 64], "discret", 1.0, 20, ("thread", "wave", "scan", "auto"), -0.15, 0.012),
    "12x5_h4": (12, 5, [16], "discret", 1.0, 4, ("thread", "wave"), -0.3, 0.0658),
    "20x4_h6": (20, 4, [24], "discret", 1.0, 6, ("thread", "wave"), -0.3, 0.0475),
}
MIXED_ATTEMPTS = (5, 3)


@functools.lru_cache(maxsize=None)
def mixed_case(name):
    nx, nu, hidden, integ, DT, H, kernels, r_diag, _ = MIXED_ROWS[name]
    return Case(name, nx, nu, hidden, integ, DT, H, kernels, "float64", act="tanh", seed=0, B=BMAX, x0_range=1.0, out_scale=1.0,
                r_diag=r_diag)


@functools.lru_cache(maxsize=None)
def mixed_reference(name):
    """Per problem: z0, level (the first of MIXED_ATTEMPTS[0] = 5 levels from reg0 that sweeps through, None if none),
    robust, reg_k, dz (the dense step at reg_k), tol, raises (the full step raises the l1 merit), cands: [(label, point)] --
    the full step, z0 + 2^-j dz for j = 1 .. MAX_LINESEARCH, and z0; all from the problem's own winning level."""
    case = mixed_case(name)
    reg0 = MIXED_ROWS[name][8]
    lam0 = np.zeros(case.H * case.nx)
    out = []
    for b in range(case.B):
        prob, x0, z0 = case.problem(b), case.X0[b], case.start(b)
        sp = kkt.stage_problem(prob, z0, x0, lam0)
        level = kkt.winning_level(prob, z0, x0, lam0, reg0, MIXED_ATTEMPTS[0], sp=sp)
        robust = kkt.winning_level_is_robust(prob, z0, x0, lam0, reg0, MIXED_ATTEMPTS[0], sp=sp)
        r = dict(z0=z0, level=level, robust=robust, lam_min=kkt.min_passing_reg(prob, z0, x0, lam0))
        if level is not None:
            reg_k = kkt.damping_levels(reg0, level)[level]
            dz, lam, _, _ = kkt.newton_step(prob, z0, x0, lam0, reg_k, diagnostics=False)
            dzr, _ = kkt.riccati_step(prob, z0, x0, lam0, reg_k, np.float64, sp=sp)
            pen = max(1.0, 1.5 * float(np.abs(lam).max()) + 1e-3)
            cands = [("full", z0 + dz)] + [(f"half^{j}", z0 + 2.0 ** -j * dz) for j in range(1, MAX_LINESEARCH + 1)] + [("start", z0)]
            r.update(reg_k=reg_k, dz=dz, tol=step_tolerance(float(np.abs(dzr - dz).max()), z0 + dz), cands=cands,
                     raises=kkt.l1_merit(prob, z0 + dz, x0, pen) >= kkt.l1_merit(prob, z0, x0, pen))
        out.append(r)
    return out


# ---- (g) several iterations with the real state machine: the tanh 2/1 network of (b) (output layer times 0.1, X0 in +-0.5),
# default reg, default 3 attempts, 4 iterations, at seeds where the multipliers of the first step make a control Hessian
# indefinite: the problem then sits out while reg climbs 1e-9 -> 1e-2 -> 0.316 through the floor and takes a damped step.
CLIMB_SEEDS = (5, 7)
CLIMB_ITERATIONS, CLIMB_B, CLIMB_POOL = 4, 8, 32
CLIMB_KERNELS = ("thread", "wave", "scan", "auto")


@functools.lru_cache(maxsize=None)
def climb_case(seed):
    """(case of CLIMB_B problems, per problem (damped_replay, cumulative sweep error)): of a seeded pool of CLIMB_POOL starts
    the first CLIMB_B whose replay is robust at every iteration and whose every taken step lowers the l1 merit -- of which
    at most CLIMB_B - 2 may be problems that restart: at seed 5 the first eight such starts all sit out after their first
    step (the pool's 18 and 21 are its first that never restart), at seed 7 the cap changes nothing."""
    nx, nu, hidden, integ, DT, H = 2, 1, [64, 64], "discret", 1.0, 20
    pool = Case(f"climb{seed}", nx, nu, hidden, integ, DT, H, CLIMB_KERNELS, "float64", act="tanh", seed=seed, B=CLIMB_POOL,
                scale_b=True)
    keep, ref, n_restarting = [], [], 0
    for b in range(pool.B):
        prob, x0 = pool.problem(b), pool.X0[b]
        rp = kkt.damped_replay(prob, x0, pool.start(b), CLIMB_ITERATIONS, REG, kkt.LQ_ATTEMPTS)
        restarts = any(s["level"] != 0 for s in rp)
        if restarts and n_restarting == CLIMB_B - 2:
            continue
        if all(s["robust"] for s in rp) and all(s["dmerit"] < 0.0 for s in rp if s["level"] is not None):
            n_restarting += restarts
            keep.append(b)
            ref.append((rp, kkt.sweep_error_damped(prob, x0, rp, np.float64)))
        if len(keep) == CLIMB_B:
            break
    assert len(keep) == CLIMB_B, keep
    pool.X0, pool.B, pool.kept = pool.X0[keep].copy(), CLIMB_B, tuple(keep)
    return pool, ref


def climbed(rp):
    """The replay sat out at least once and later took a damped step."""
    sat = [i for i, s in enumerate(rp) if s["level"] is None]
    return bool(sat) and any(s["level"] is not None and s["reg_used"] >= kkt.REG_FLOOR for s in rp[sat[0] + 1:])


# ... and the guard of the rule: the tanh 2/1 network of (f) with lq_attempts = 2.  At GUARD_REG0 the first step of problems
# 4, 5, 7, 8, 9, 13 and 14 goes through at level 1, and with that step's multipliers in the blocks their second sweep needs level
# 1 again from the reg the first step stored.  Had the acceptance of the first step relaxed the reg (it must not: the
# opening sweep restarted), both levels of the second iteration would fail and the problem would sit out.
GUARD_REG0, GUARD_ATTEMPTS = 0.0783, 2


@functools.lru_cache(maxsize=None)
def guard_reference():
    case = mixed_case("2x1_h20")
    out = []
    for b in range(case.B):
        prob, x0 = case.problem(b), case.X0[b]
        rp = kkt.damped_replay(prob, x0, case.start(b), 2, GUARD_REG0, GUARD_ATTEMPTS)
        out.append((rp, kkt.sweep_error_damped(prob, x0, rp, np.float64)))
    return out
