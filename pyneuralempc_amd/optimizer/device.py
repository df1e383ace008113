"""``DeviceSqp``: the batched on-device solver (csrc/solver.hip, ``CallbackEngine.solve``) behind the reference's
``Optimizer`` interface, for ``NMPC.next`` on ONE problem.  The reference has no counterpart -- its optimizers are Ipopt
(optimizer/ipopt.py:138-195) and SciPy SLSQP (optimizer/slsqp.py:143-197), both on the CPU, calling back into the model
once per iterate; here the whole iteration (callbacks, Riccati solve, line search) stays on the GPU and the host gets the
solution.  Same plumbing as ``Slsqp``: problem object from the factory, cold start / shifted warm start
(``init_with_last_result``), ``prev_result`` for ``NMPC.next`` to split.

Needs the fused device path: a device integrator, a ``QuadraticObjective`` and no extra constraint rows other than one
``BoxStateConstraint`` (which the solver turns into state bounds) and any number of ``LinearStageConstraint`` (bound as the
solver's stage rows for the call); anything else raises ``NotImplementedError`` -- there is no CPU fallback."""
import numpy as np

from ..constraints import BoxStateConstraint, LinearStageConstraint
from .base import Optimizer, fused_evaluator
from .slsqp import Slsqp, SlsqpProblemFactory


class DeviceSqp(Slsqp):
    def __init__(self, max_iteration=200, tolerance=None, verbose=0, init_with_last_result=False, warm_mu=1e-4,
                 certificate=False, gain=False, du_weight=None, du_lb=None, du_ub=None, **solver_opts):
        """tolerance: max |defect| and relative step at convergence (tol_constraint = tol_step); None = what an iterate
        of the model's precision can reach (CallbackEngine.solve: 1e-8 for fp64, 1e-4 for fp32 -- an fp32 iterate stalls
        near 1e-5 and would never report success against 1e-8); warm_mu: initial barrier
        parameter of a warm-started solve (a cold start uses the solver's default of 0.1); solver_opts: further keyword
        arguments of CallbackEngine.solve (linesearch, lq_kernel, mu_min, ...).  certificate=True: every solve also takes
        the multipliers of its result (``last_duals``: {"lam", "zl", "zu"} as NumPy vectors of the one problem) and scores
        the point on the device (``last_kkt``: stationarity, primal feasibility, complementarity, dual feasibility --
        CallbackEngine.kkt_residual); without it nothing more than the solve is launched and both stay None.  gain=True:
        every solve also keeps the feedback gain of its result, ``last_gain`` (nu,nx) = du_0*/dx0 for
        u = u0* + K0 (x_measured - x0), and ``last_gain_status`` (CallbackEngine.sensitivity: 0 ok, else the gain is NaN).
        du_weight (nu,nu), du_lb / du_ub (nu,) or (H,nu): an input-rate penalty sum_t du_t' du_weight du_t and rate limits on
        du_t = u_t - u_{t-1} (CallbackEngine.bind_rate).  u_{-1} is the first control of the last successful solve -- the one
        NMPC.next's caller applied --, zeros on the first call, or what ``NMPC.next(u_prev=)`` / ``set_u_prev`` gave for the
        next solve.  Not together with certificate or gain (the library refuses multipliers under a rate binding).
        A problem whose constraint list holds LinearStageConstraints is solved inside their rows
        (CallbackEngine.bind_rows); a ValueError when the optimizer has rate terms, certificate or gain."""
        if (du_weight is not None or du_lb is not None or du_ub is not None) and (certificate or gain):
            raise ValueError("DeviceSqp: du_weight / du_lb / du_ub cannot be combined with certificate=True or gain=True")
        super().__init__(max_iteration=max_iteration, tolerance=tolerance, verbose=verbose,
                         init_with_last_result=init_with_last_result)
        self.warm_mu = warm_mu
        self.solver_opts = dict(solver_opts)
        self.last_iterations = None
        self.certificate = bool(certificate)
        self.last_duals = None
        self.last_kkt = None
        self.gain = bool(gain)
        self.last_gain = None
        self.last_gain_status = None
        self.rate = None if du_weight is None and du_lb is None and du_ub is None else dict(S=du_weight, du_lb=du_lb, du_ub=du_ub)
        self._u_prev = None

    def set_u_prev(self, u_prev, nu=None):
        """The control applied before the next solve (nu,), for the rate terms."""
        if self.rate is None:
            raise ValueError("DeviceSqp: u_prev needs rate terms (du_weight, du_lb or du_ub)")
        v = np.asarray(u_prev, dtype=np.float64).reshape(-1)
        if nu is not None and v.shape != (int(nu),):
            raise ValueError(f"u_prev must have shape {(int(nu),)}, got {tuple(np.shape(u_prev))}")
        self._u_prev = v

    def _fused_with_rows(self, problem):
        """(the problem's fused evaluator, None), or -- its constraint list holding LinearStageConstraints next to at most one
        BoxStateConstraint, which keeps the host glue off the fused path -- (the evaluator of the problem without them, the rows
        stacked as (C, lo, hi)).  (None, None) when there is no fused path."""
        fused = getattr(problem, "_fused", None)
        cons = list(getattr(problem, "constraints_list", None) or [])
        rows = [c for c in cons if isinstance(c, LinearStageConstraint)]
        if fused is not None or not rows:
            return fused, None
        boxes = [c for c in cons if isinstance(c, BoxStateConstraint)]
        integ = problem.integrator
        if len(boxes) + len(rows) != len(cons) or len(boxes) > 1 or not getattr(integ, "on_device", False):
            return None, None
        if self.rate is not None or self.certificate or self.gain:
            raise ValueError("DeviceSqp: a LinearStageConstraint cannot be combined with rate terms, certificate=True or gain=True")
        from ..objective.quadratic import QuadraticObjective
        if not isinstance(problem.objective_func, QuadraticObjective):
            return None, None
        fused = fused_evaluator(integ, problem.objective_func, boxes[0] if boxes else None)
        fused.set_parameters(problem.p, problem.tvp)
        return fused, LinearStageConstraint.stack(rows, int(integ.H), int(integ.model.x_dim) + int(integ.model.u_dim))

    def get_factory(self):
        return SlsqpProblemFactory()      # the same problem object: x0, parameters, fused evaluator, initial values

    def solve(self, problem, domain_constraint):
        fused, rows = self._fused_with_rows(problem)
        if fused is None:
            raise NotImplementedError("DeviceSqp needs the fused device path: a device integrator, a QuadraticObjective and "
                                      "no extra constraint rows other than one BoxStateConstraint")
        eng = fused.engine
        H = problem.integrator.H
        warm = (problem.get_init_variables()[0] is not None) or (self.init_with_last_result and self.prev_result is not None)
        z0 = np.asarray(self.initial_point(problem), dtype=np.float64).reshape(1, -1)
        lb = np.asarray(domain_constraint.get_lower_bounds(H), dtype=np.float64)
        ub = np.asarray(domain_constraint.get_upper_bounds(H), dtype=np.float64)
        opts = dict(max_iter=self.max_iteration)
        if self.tolerance is not None:
            opts.update(tol_constraint=self.tolerance, tol_step=self.tolerance)
        if warm:
            opts["mu_init"] = self.warm_mu
        opts.update(self.solver_opts)
        X0 = eng.to_device(np.asarray(problem.get_init_value(), dtype=np.float64).reshape(1, -1))
        if rows is not None:
            eng.bind_rows(*rows)
            try:
                Z, status, iters = eng.solve(X0, eng.to_device(z0), lb, ub, **opts)
            finally:
                eng.bind_rows()
            self.last_iterations = iters
            if int(status[0].item()) != 0:
                return Optimizer.FAIL
            self.prev_result = Z[0].to("cpu").double().numpy()
            return Optimizer.SUCCESS
        if self.rate is not None:
            up = np.zeros(eng.nu) if self._u_prev is None else self._u_prev
            eng.bind_rate(u_prev=eng.to_device(up.reshape(1, -1)), **self.rate)
            try:
                Z, status, iters = eng.solve(X0, eng.to_device(z0), lb, ub, **opts)
            finally:
                eng.bind_rate()
            self.last_iterations = iters
            if int(status[0].item()) != 0:
                return Optimizer.FAIL
            self.prev_result = Z[0].to("cpu").double().numpy()
            self._u_prev = self.prev_result[H * eng.nx:H * eng.nx + eng.nu].copy()
            return Optimizer.SUCCESS
        if self.certificate or self.gain:
            Z, status, iters, duals = eng.solve(X0, eng.to_device(z0), lb, ub, return_duals=True, **opts)
            if self.certificate:
                r = eng.kkt_residual(Z, X0, duals["lam"], duals["zl"], duals["zu"], lb, ub)
                self.last_duals = {k: v[0].to("cpu").double().numpy() for k, v in duals.items()}
                self.last_kkt = r[0].to("cpu").double().numpy()
            if self.gain:
                sens = eng.sensitivity(Z, X0, duals["lam"], duals["zl"], duals["zu"], lb, ub, want=("du0",))
                self.last_gain = sens["du0"][0].to("cpu").double().numpy()
                self.last_gain_status = int(sens["status"][0].item())
        else:
            Z, status, iters = eng.solve(X0, eng.to_device(z0), lb, ub, **opts)
        self.last_iterations = iters
        if int(status[0].item()) != 0:
            return Optimizer.FAIL
        self.prev_result = Z[0].to("cpu").double().numpy()
        return Optimizer.SUCCESS
