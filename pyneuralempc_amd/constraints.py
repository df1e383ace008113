"""Variable bounds and extra constraint rows (reference: pyNeuralEMPC/constraints.py:3-96)."""
import numpy as np


def _bound_column(pairs, which, H):
    """[b[which] for every (lower, upper) pair] repeated for the H steps of the horizon"""
    return [pair[which] for pair in pairs] * H


class DomainConstraint:
    """Box bounds on the decision variables z = [states | controls]; consumed by the optimizer as lb / ub
    (optimizer/ipopt.py:153-154), they add no rows to g."""

    def __init__(self, states_constraint: list, control_constraint: list):
        for pairs, empty_msg, label in ((states_constraint, "States constraint empty !", "states"),
                                        (control_constraint, "Control constraint empty !", "control")):
            if len(pairs) == 0:
                raise ValueError(empty_msg)
            if any(len(pair) != 2 for pair in pairs):
                raise ValueError(f"Your {label} constraint must be a list of bound couple  ! "
                                 "[(lower_bound, upper_bound), ...]")
        self.states_constraint, self.control_constraint = states_constraint, control_constraint

    def get_dim(self, H):
        return len(self.states_constraint), len(self.control_constraint)

    def get_lower_bounds(self, H):
        return _bound_column(self.states_constraint, 0, H) + _bound_column(self.control_constraint, 0, H)

    def get_upper_bounds(self, H):
        return _bound_column(self.states_constraint, 1, H) + _bound_column(self.control_constraint, 1, H)

    def get_type(self):
        return Constraint.EQ_TYPE     # meaningless for bounds and unused, as in the reference (constraints.py:32-33)


class Constraint:
    """Extra rows appended to g after the integrator defects (optimizer/ipopt.py:47-52,91-96).  A subclass gives
    forward (k,), jacobian (k, n), get_dim(H) and the two bound vectors; the row type follows from the bounds."""
    EQ_TYPE, INEQ_TYPE, INTER_TYPE = 0, 1, 2

    def forward(self, x, u, p=None, tvp=None):
        pass

    def jacobian(self, x, u, p=None, tvp=None):
        pass

    def hessian(self, x, u, p=None, tvp=None):
        """(k, n, n); called by the solver glue (ipopt.py:75) although the reference's base class does not declare
        it.  Default: linear rows, all zeros."""
        H, nx = np.asarray(x).shape
        n = H * (nx + np.asarray(u).shape[1])
        return np.zeros((int(self.get_dim(H)), n, n))

    def get_dim(self, H):
        raise NotImplementedError()

    def get_lower_bounds(self, H):
        raise NotImplementedError()

    def get_upper_bounds(self, H):
        raise NotImplementedError()

    def get_type(self, H=None):
        lo, hi = (np.asarray(v) for v in (self.get_lower_bounds(H), self.get_upper_bounds(H)))
        if not (lo == 0).all():
            return Constraint.INTER_TYPE
        if (hi == 0).all():
            return Constraint.EQ_TYPE
        return Constraint.INEQ_TYPE if (hi == np.inf).all() else Constraint.INTER_TYPE


class _ZeroLowerBound(Constraint):
    """rows bounded below by zero; the two public flavours differ in the upper bound only"""
    _upper = 0.0

    def forward(self, x, u, p=None, tvp=None):
        raise NotImplementedError()

    def jacobian(self, x, u, p=None, tvp=None):
        raise NotImplementedError()

    def get_lower_bounds(self, H):
        return np.zeros(int(self.get_dim(H)))

    def get_upper_bounds(self, H):
        return np.full(int(self.get_dim(H)), self._upper)


class EqualityConstraint(_ZeroLowerBound):       # g(z) = 0
    _upper = 0.0


class InequalityConstraint(_ZeroLowerBound):     # g(z) >= 0
    _upper = np.inf


class BoxStateConstraint(Constraint):
    """rows = states.ravel() kept in [lo, hi] (BASELINE config 5: box state constraints as rows of g,
    dense selector Jacobian).  The reference declares the interface but ships no concrete row
    constraint; this one is recognised by the solver glue and evaluated inside the fused device call.
    The NumPy methods below are the interface's contract for third-party glue."""

    def __init__(self, lo, hi, x_dim=None):
        lo, hi = np.atleast_1d(np.asarray(lo, dtype=np.float64)), np.atleast_1d(np.asarray(hi, dtype=np.float64))
        if x_dim is not None:
            lo, hi = np.broadcast_to(lo, (x_dim,)).copy(), np.broadcast_to(hi, (x_dim,)).copy()
        elif lo.size == 1 or hi.size == 1:
            raise ValueError("give one (lo, hi) per state, or scalars together with x_dim")
        if lo.shape != hi.shape:
            raise ValueError("lo and hi must have the same shape")
        self.lo, self.hi = lo, hi

    def _bounds(self, nx):
        return np.broadcast_to(self.lo, (nx,)), np.broadcast_to(self.hi, (nx,))

    def forward(self, x, u, p=None, tvp=None):
        return np.asarray(x, dtype=np.float64).reshape(-1).copy()

    def jacobian(self, x, u, p=None, tvp=None):
        H, nx = np.asarray(x).shape
        nu = np.asarray(u).shape[1]
        return np.concatenate([np.eye(H * nx), np.zeros((H * nx, H * nu))], axis=1)

    def get_dim(self, H):
        return H * len(self.lo)

    def get_lower_bounds(self, H):
        return np.tile(self.lo, H)

    def get_upper_bounds(self, H):
        return np.tile(self.hi, H)


class LinearStageConstraint(Constraint):
    """Linear stage rows lo <= Cx x_t + Cu u_t <= hi for every step t of the horizon, C = [Cx (nc,nx) | Cu (nc,nu)]: a shared
    actuator budget, a polytopic state set, a mixed limit.  Row block t pairs row t of the (H,nx) states with row t of the (H,nu)
    controls -- the arguments of forward -- so state row t is the state the t-th step arrives at (x0 is data and no row reads
    it).  lo / hi: (nc,) for every step or (H,nc) per step, a scalar for all rows, None or -+inf = no limit on that side;
    lo < hi on every entry (equality rows are not built).  A full Constraint for the host glue (Ipopt, SLSQP); the batched
    device solver takes it as it is (NMPC.next_batch, NMPC.closed_loop_batch, DeviceSqp; CallbackEngine.bind_rows)."""

    def __init__(self, C, lo=None, hi=None):
        C = np.asarray(C, dtype=np.float64)
        if C.ndim != 2 or C.shape[0] < 1 or not np.isfinite(C).all():
            raise ValueError(f"C must be a finite (nc, nx+nu) matrix with nc >= 1, got shape {C.shape}")
        nc = C.shape[0]
        lims = []
        for name, v, fill in (("lo", lo, -np.inf), ("hi", hi, np.inf)):
            a = np.full(nc, fill) if v is None else np.asarray(v, dtype=np.float64)
            if a.ndim == 0:
                a = np.full(nc, float(a))
            if a.ndim not in (1, 2) or a.shape[-1] != nc:
                raise ValueError(f"{name} must have shape {(nc,)} (every step) or (H, {nc}) (per step), got {a.shape}")
            if np.isnan(a).any():
                raise ValueError(f"{name} has a NaN")
            lims.append(a)
        lo, hi = lims
        if lo.ndim != hi.ndim:      # one form
            lo, hi = np.broadcast_arrays(lo, hi)
        if lo.shape != hi.shape:
            raise ValueError(f"lo {lo.shape} and hi {hi.shape} do not cover the same steps")
        if (lo >= hi).any():
            raise ValueError("lo >= hi on some entry (equality or empty rows are not supported: the solver's barrier needs an interior)")
        self.C, self.lo, self.hi = np.ascontiguousarray(C), np.ascontiguousarray(lo), np.ascontiguousarray(hi)

    @property
    def nc(self):
        return self.C.shape[0]

    def _split_C(self, x, u):
        x, u = np.asarray(x, dtype=np.float64), np.asarray(u, dtype=np.float64)
        if x.ndim != 2 or u.ndim != 2 or x.shape[0] != u.shape[0] or x.shape[1] + u.shape[1] != self.C.shape[1]:
            raise ValueError(f"C has {self.C.shape[1]} columns: x (H,nx) and u (H,nu) must have nx + nu of them, "
                             f"got {x.shape} and {u.shape}")
        return x, u, self.C[:, :x.shape[1]], self.C[:, x.shape[1]:]

    def forward(self, x, u, p=None, tvp=None):
        x, u, Cx, Cu = self._split_C(x, u)
        return (x @ Cx.T + u @ Cu.T).reshape(-1)

    def jacobian(self, x, u, p=None, tvp=None):
        x, u, Cx, Cu = self._split_C(x, u)
        (H, nx), nu, nc = x.shape, u.shape[1], self.nc
        J = np.zeros((H * nc, H * (nx + nu)))
        for t in range(H):
            J[t * nc:(t + 1) * nc, t * nx:(t + 1) * nx] = Cx
            J[t * nc:(t + 1) * nc, H * nx + t * nu:H * nx + (t + 1) * nu] = Cu
        return J

    def get_dim(self, H):
        return int(H) * self.nc

    def limits(self, H):
        """(lo, hi) as (H,nc) arrays"""
        if self.lo.ndim == 2 and self.lo.shape[0] != int(H):
            raise ValueError(f"the limits were given per step for H = {self.lo.shape[0]}, the horizon is {int(H)}")
        return tuple(np.ascontiguousarray(np.broadcast_to(a, (int(H), self.nc))) for a in (self.lo, self.hi))

    def get_lower_bounds(self, H):
        return self.limits(self.lo.shape[0] if H is None and self.lo.ndim == 2 else (1 if H is None else H))[0].reshape(-1)

    def get_upper_bounds(self, H):
        return self.limits(self.hi.shape[0] if H is None and self.hi.ndim == 2 else (1 if H is None else H))[1].reshape(-1)

    @staticmethod
    def stack(constraints, H, n_cols):
        """Several constraints as one: (C (sum nc, n_cols), lo (H, sum nc), hi (H, sum nc)), rows in list order."""
        for c in constraints:
            if c.C.shape[1] != n_cols:
                raise ValueError(f"LinearStageConstraint: C has {c.C.shape[1]} columns, the model has nx + nu = {n_cols}")
        lims = [c.limits(H) for c in constraints]
        return (np.concatenate([c.C for c in constraints], axis=0), np.concatenate([l[0] for l in lims], axis=1),
                np.concatenate([l[1] for l in lims], axis=1))
