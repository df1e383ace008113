"""NMPC facade (reference: pyNeuralEMPC/controller.py:7-113): argument checks, problem assembly
through the optimizer's factory, solve, reshape."""
import numpy as np

from .constraints import DomainConstraint
from .optimizer import Ipopt, Optimizer


class NMPC:
    def __init__(self, integrator, objective_func, constraint_list, H, DT, optimizer=None, use_hessian=True):
        self.integrator = integrator
        self.objective_func = objective_func
        self.constraint_list = constraint_list
        domains = [c for c in constraint_list if isinstance(c, DomainConstraint)]
        if not domains:
            raise IndexError("constraint_list must contain a DomainConstraint")
        # like the reference (controller.py:13-14) the first DomainConstraint is taken OUT of the caller's list
        self.domain_constraint = domains[0]
        self.constraint_list.remove(self.domain_constraint)
        self.H = H
        self.DT = DT
        # the reference's default argument `optimizer=Ipopt()` is one instance shared by every NMPC
        # (controller.py:8); a fresh one per controller is used here
        self.optimizer = Ipopt() if optimizer is None else optimizer
        # stored and, as in the reference, NOT forwarded to the problem factory (controller.py:18,
        # optimizer/base.py:78): the solve runs hessian-free unless the optimizer opts in
        self.use_hessian = use_hessian

    def _check(self, x0, p, tvp, init_x, init_u):
        model = self.integrator.model
        assert len(x0.shape) == 1, "x0 must be a vector"
        assert x0.shape[0] == model.x_dim, "x0 dim must set according to your model !"
        if p is not None:
            assert len(p.shape) == 1, "p must be a vector"
            assert p.shape[0] == model.p_dim, "p dim must set according to your model !"
        if tvp is not None:
            assert len(tvp.shape) == 2, "tvp must be a vector"
            assert tvp.shape[1] == model.tvp_dim, "tvp dim must set according to your model !"
            assert tvp.shape[0] == self.H, "tvp first dim must set according to the horizon size !"
        assert (init_x is None) == (init_u is None), "you must give both init values"
        if init_x is not None:
            assert init_x.shape[1] == model.x_dim, ("init_x dim must have the good feature size "
                                                    f"(expected {model.x_dim})")
            assert init_u.shape[1] == model.u_dim, ("init_u dim mist have the good feature size "
                                                    f"(expected {model.u_dim})")

    def get_pb(self, x0: np.array, p=None, tvp=None, init_x=None, init_u=None):
        self._check(x0, p, tvp, init_x, init_u)
        factory = self.optimizer.get_factory()
        factory.set_x0(x0)
        factory.set_objective(self.objective_func)
        factory.set_integrator(self.integrator)
        factory.set_constraints(self.constraint_list)
        if init_x is not None:
            factory.set_init_values(init_x, init_u)
        if tvp is not None:
            factory.set_tvp(tvp)
        if p is not None:
            factory.set_p(p)
        if getattr(self.optimizer, "exact_hessian", False):
            factory.set_use_hessian(bool(self.use_hessian))
        return factory.getProblemInterface()

    def next(self, x0: np.array, p=None, tvp=None, init_x=None, init_u=None, u_prev=None):
        """Solve one MPC problem; returns (states (H,nx), u (H,nu)) or (None, None) on solver failure.  u_prev (nu,): the
        control applied before this step, for an optimizer with an input-rate penalty or rate limits (DeviceSqp(du_weight=,
        du_lb=, du_ub=)); left out, such an optimizer takes the first control of its last result (zeros on the first call)."""
        pb = self.get_pb(x0, p=p, tvp=tvp, init_x=init_x, init_u=init_u)
        if u_prev is not None:
            if not hasattr(self.optimizer, "set_u_prev"):
                raise ValueError("next: u_prev is for an optimizer with rate terms (DeviceSqp(du_weight=, du_lb=, du_ub=))")
            self.optimizer.set_u_prev(u_prev, self.integrator.model.u_dim)
        status = self.optimizer.solve(pb, self.domain_constraint)
        if status != Optimizer.SUCCESS:
            return None, None
        model = self.integrator.model
        z = self.optimizer.prev_result
        nxh = model.x_dim * self.integrator.H
        return z[:nxh].reshape(self.integrator.H, -1), z[nxh:].reshape(self.integrator.H, -1)


    def _batch_engine(self, X0, p, tvp, prev_x, prev_u, prev_tvp, who):
        """What next_batch and closed_loop_batch share: the precondition check, the fused device engine with the extra inputs
        and the histories of the B problems bound, X0 on the device, and the variable bounds (box rows folded in)."""
        import torch
        from .optimizer.base import fused_evaluator
        from .objective.quadratic import QuadraticObjective
        from .integrator.base import DeviceIntegrator
        from .constraints import BoxStateConstraint, LinearStageConstraint
        boxes = [c for c in self.constraint_list if isinstance(c, BoxStateConstraint)]
        n_rows = sum(isinstance(c, LinearStageConstraint) for c in self.constraint_list)
        if not (isinstance(self.integrator, DeviceIntegrator) and self.integrator.on_device and isinstance(self.objective_func, QuadraticObjective)
                and len(boxes) + n_rows == len(self.constraint_list)):
            raise NotImplementedError(f"{who} needs a device integrator, a QuadraticObjective and no extra "
                                      "constraint rows other than BoxStateConstraint and LinearStageConstraint")
        eng = fused_evaluator(self.integrator, self.objective_func, None).engine
        H = self.integrator.H
        X0t = X0 if isinstance(X0, torch.Tensor) else eng.to_device(np.atleast_2d(np.asarray(X0, dtype=np.float64)))
        B = int(X0t.shape[0])
        model = self.integrator.model
        w = int(getattr(model, "rolling_window", 1))

        def history(given, stored, d, name):
            v = stored if given is None else given
            if v is None:
                raise ValueError(f"rolling-window model: pass {name} or call set_prev_data first")
            v = np.asarray(v, dtype=np.float64)
            if v.shape[-2:] != (w - 1, d) or v.ndim not in (2, 3) or (v.ndim == 3 and v.shape[0] != B):
                raise ValueError(f"{name} must have shape {(w - 1, d)} or {(B, w - 1, d)} (received : {v.shape})")
            return np.ascontiguousarray(np.broadcast_to(v if v.ndim == 3 else v[None], (B, w - 1, d)))

        if w > 1:
            eng.bind_history(eng.to_device(history(prev_x, model.prev_x, model.x_dim, "prev_x")),
                             eng.to_device(history(prev_u, model.prev_u, model.u_dim, "prev_u")))
        elif prev_x is not None or prev_u is not None or prev_tvp is not None:
            raise ValueError("this model has no rolling window: it takes no prev_x / prev_u / prev_tvp")
        if model.p_dim + model.tvp_dim:
            # extra network inputs of every problem: (B, H, tvp_dim + p_dim) = [tvp_t | p], the reference's
            # concatenation order (model/tensorflow.py:39-47); a (1, ...) binding left by NMPC.next never serves B > 1
            parts = []
            if model.tvp_dim:
                if tvp is None:
                    raise ValueError("this model has tvp_dim > 0: pass tvp (H, tvp_dim) or (B, H, tvp_dim)")
                tv = np.asarray(tvp, dtype=np.float64)
                tv = np.broadcast_to(tv if tv.ndim == 3 else tv[None], (B, H, model.tvp_dim))
                if w > 1:      # rolled like the states: (B, H, w * tvp_dim)  (_gather_input_V2, model/tensorflow.py:218-233)
                    ptv = history(prev_tvp, model.prev_tvp, model.tvp_dim, "prev_tvp")
                    tv = np.stack([model._roll(ptv[b], tv[b]) for b in range(B)], axis=0)
                parts.append(tv)
            if model.p_dim:
                if p is None:
                    raise ValueError("this model has p_dim > 0: pass p (p_dim,) or (B, p_dim)")
                pv = np.asarray(p, dtype=np.float64)
                pv = np.broadcast_to(pv if pv.ndim == 2 else pv[None], (B, model.p_dim))
                parts.append(np.broadcast_to(pv[:, None, :], (B, H, model.p_dim)))
            eng.bind_extra(eng.to_device(np.concatenate(parts, axis=2)))
        elif p is not None or tvp is not None:
            raise ValueError("this model takes no p / tvp")
        lb = np.asarray(self.domain_constraint.get_lower_bounds(H), dtype=np.float64).copy()
        ub = np.asarray(self.domain_constraint.get_upper_bounds(H), dtype=np.float64).copy()
        # box rows on the states are bounds on the state variables: intersect them with the domain
        for box in boxes:
            lo, hi = box._bounds(eng.nx)
            lb[:H * eng.nx] = np.maximum(lb[:H * eng.nx], np.tile(lo, H))
            ub[:H * eng.nx] = np.minimum(ub[:H * eng.nx], np.tile(hi, H))
        return eng, X0t.contiguous(), lb, ub

    def _tracking_check(self, X0, L, who, **arrays):
        """Shapes of the per-problem references / linear costs / bounds, checked before anything touches a device: (B,L,d), or
        (L,d) for one set shared by all problems.  Returns the arrays that were given."""
        model = self.integrator.model
        B = 1 if len(np.shape(X0)) < 2 else int(np.shape(X0)[0])
        given = {}
        for name, v in arrays.items():
            if v is None:
                continue
            d = int(model.x_dim if name in ("xref", "cx", "xlb", "xub") else model.u_dim)
            shape = tuple(int(k) for k in np.shape(v))
            if shape not in ((B, L, d), (L, d)):
                raise ValueError(f"{who}: {name} must have shape {(B, L, d)} (one per problem) or {(L, d)} (shared), got {shape}")
            given[name] = v
        return given

    def _rate_check(self, X0, who, u_prev, du_weight, du_lb, du_ub):
        """Shapes of the rate arguments, checked before anything touches a device.  -> None when none is given, else
        dict(u_prev (B,nu) float64 array or a tensor, S, du_lb, du_ub)."""
        if u_prev is None and du_weight is None and du_lb is None and du_ub is None:
            return None
        model = self.integrator.model
        nu, H = int(model.u_dim), int(self.integrator.H)
        B = 1 if len(np.shape(X0)) < 2 else int(np.shape(X0)[0])
        if u_prev is None:
            raise ValueError(f"{who}: u_prev (the control applied before the first step) is required with du_weight, du_lb or du_ub")
        shape = tuple(int(k) for k in np.shape(u_prev))
        if shape not in ((B, nu), (nu,)):
            raise ValueError(f"{who}: u_prev must have shape {(B, nu)} (one per problem) or {(nu,)} (shared), got {shape}")
        if du_weight is not None and tuple(np.shape(du_weight)) != (nu, nu):
            raise ValueError(f"{who}: du_weight must have shape {(nu, nu)}, got {tuple(np.shape(du_weight))}")
        for name, v in (("du_lb", du_lb), ("du_ub", du_ub)):
            if v is not None and tuple(np.shape(v)) not in ((nu,), (H, nu)):
                raise ValueError(f"{who}: {name} must have shape {(nu,)} (every step) or {(H, nu)} (per step), got {tuple(np.shape(v))}")
        if du_lb is not None and du_ub is not None and \
                (np.broadcast_to(np.asarray(du_lb, dtype=np.float64), (H, nu)) >= np.broadcast_to(np.asarray(du_ub, dtype=np.float64), (H, nu))).any():
            raise ValueError(f"{who}: du_lb >= du_ub on some entry (the solver's barrier needs an interior)")
        if int(getattr(model, "rolling_window", 1)) > 1:
            raise ValueError(f"{who}: rate terms are not supported with rolling-window models")
        return dict(u_prev=u_prev, S=du_weight, du_lb=du_lb, du_ub=du_ub)

    def _stage_rows(self, who, **refused):
        """The LinearStageConstraints of the constraint list stacked into one (C, lo (H,nc), hi (H,nc)), checked before anything
        touches a device; None when there is none.  refused: what the device solver does not combine with rows, by name."""
        from .constraints import LinearStageConstraint
        rows = [c for c in self.constraint_list if isinstance(c, LinearStageConstraint)]
        if not rows:
            return None
        bad = [name for name, on in refused.items() if on]
        if bad:
            raise ValueError(f"{who}: a LinearStageConstraint cannot be combined with {', '.join(bad)} (the device solver refuses "
                             "those combinations)")
        model = self.integrator.model
        if int(getattr(model, "rolling_window", 1)) > 1:
            raise ValueError(f"{who}: a LinearStageConstraint is not supported with rolling-window models")
        return LinearStageConstraint.stack(rows, int(self.integrator.H), int(model.x_dim) + int(model.u_dim))

    @staticmethod
    def _rate_bind(eng, B, rate):
        """The rate terms bound on the engine (CallbackEngine.bind_rate); returns the (B,nu) device tensor of u_prev, which
        the engine reads in stream order at every solve."""
        import torch
        v = rate["u_prev"]
        t = v.to(device=eng.device, dtype=eng.dtype) if isinstance(v, torch.Tensor) else \
            torch.as_tensor(np.asarray(v, dtype=np.float64), dtype=eng.dtype, device=eng.device)
        t = (t if t.dim() == 2 else t[None].expand(B, -1)).contiguous().clone()
        eng.bind_rate(u_prev=t, S=rate["S"], du_lb=rate["du_lb"], du_ub=rate["du_ub"])
        return t

    @staticmethod
    def _tracking_bind(eng, B, given, offset=0, bind=None):
        """Device tensors (B,L,d) of the engine's dtype for the given arrays, bound at `offset` (by eng.bind_tracking, or by
        `bind`: eng.bind_bounds); returns them."""
        import torch
        dev = {}
        for name, v in given.items():
            t = v.to(device=eng.device, dtype=eng.dtype) if isinstance(v, torch.Tensor) else \
                torch.as_tensor(np.asarray(v, dtype=np.float64), dtype=eng.dtype, device=eng.device)
            dev[name] = (t if t.dim() == 3 else t[None].expand(B, -1, -1)).contiguous()
        (bind or eng.bind_tracking)(**dev, offset=offset)
        return dev

    def next_batch(self, X0, init_z=None, p=None, tvp=None, prev_x=None, prev_u=None, prev_tvp=None, xref=None, uref=None,
                   cx=None, cu=None, xlb=None, xub=None, ulb=None, uub=None, return_duals=False, return_gain=False,
                   u_prev=None, du_weight=None, du_lb=None, du_ub=None, **solver_opts):
        """Solve B MPC problems at once on the device (no reference counterpart).  X0 (B,nx) NumPy
        array or device tensor.  Needs the fused device path (device integrator + QuadraticObjective; the only
        extra rows accepted are BoxStateConstraint, which become bounds on the state variables).  Models with
        parameters take p (p_dim,) or (B,p_dim) and tvp (H,tvp_dim) or (B,H,tvp_dim) -- one set for all problems or one
        per problem (the batched form of NMPC.next's p / tvp, controller.py:65).  Rolling-window models take the histories
        prev_x (w-1, nx) or (B, w-1, nx), prev_u, prev_tvp -- the batched form of set_prev_data (model/tensorflow.py:178-189);
        left out, what set_prev_data stored serves every problem.  solver_opts go to CallbackEngine.solve; init="rollout"
        among them starts from the roll-out of the start's controls (of zero controls without init_z) instead of the
        reference's tiled x0.  xref / cx (B,H,nx) and uref / cu (B,H,nu), NumPy arrays or device tensors, give every problem
        its own tracking reference / linear cost in place of the QuadraticObjective's (whose weights stay shared); an (H,d)
        value serves all problems; an array left out keeps the objective's.  They are bound for this call only (not with
        rolling-window models: the device solver refuses that combination).  xlb / xub (B,H,nx) and ulb / uub (B,H,nu) in the
        same forms give every problem its own, per-stage bounds on x_1 .. x_H and u_0 .. u_{H-1}: problem b is solved inside
        the intersection of the DomainConstraint, the box rows and its own rows (+-inf: no bound there); bound for this call
        only (CallbackEngine.bind_bounds), and the duals / the gain are those under the same bounds.  A problem whose own
        bounds leave a variable no interior (lo >= hi) or hold a NaN fails alone: FAIL, its start returned.  Returns (states (B,H,nx), u (B,H,nu),
        status (B,) with Optimizer.SUCCESS / FAIL per problem) as NumPy arrays.  return_duals=True appends the multipliers the
        returned iterates carry, as CallbackEngine.solve hands them back: a dict of device tensors {"lam": (B,m), "zl": (B,n),
        "zu": (B,n)} for the bounds the controller builds from its DomainConstraint (box rows folded in).  return_gain=True
        appends (after the duals when both are asked for) the feedback gain K0 = du_0*/dx0 (B,nu,nx) as a NumPy array, for
        u = u0* + K0 (x_measured - x0) between solves (CallbackEngine.sensitivity at the returned point, from the duals of
        the same solve and the controller's own bounds); entries are NaN where the sensitivity status, kept in
        ``self.last_gain_status`` (B,), is non-zero.  u_prev (B,nu) or (nu,), du_weight (nu,nu), du_lb / du_ub (nu,) or (H,nu)
        add an input-rate penalty sum_t du_t' du_weight du_t and rate limits du_lb <= du_t <= du_ub on du_t = u_t - u_{t-1},
        u_{-1} = u_prev (CallbackEngine.bind_rate, for this call only); not together with per-problem references or bounds,
        return_duals or return_gain (the device solver refuses those combinations).  Every LinearStageConstraint of the
        constraint list is a set of rows lo <= Cx x_t + Cu u_t <= hi of every problem (CallbackEngine.bind_rows, stacked, for
        this call only); not together with rate arguments, per-problem references or bounds, return_duals or return_gain."""
        import torch
        H = self.integrator.H
        rate = self._rate_check(X0, "next_batch", u_prev, du_weight, du_lb, du_ub)
        given = self._tracking_check(X0, H, "next_batch", xref=xref, uref=uref, cx=cx, cu=cu)
        bounds = self._tracking_check(X0, H, "next_batch", xlb=xlb, xub=xub, ulb=ulb, uub=uub)
        rows = self._stage_rows("next_batch", **{"rate arguments": rate, "per-problem references": given, "per-problem bounds": bounds,
                                                 "return_duals": return_duals, "return_gain": return_gain})
        eng, X0t, lb, ub = self._batch_engine(X0, p, tvp, prev_x, prev_u, prev_tvp, "next_batch")
        Zi = None if init_z is None else (init_z if isinstance(init_z, torch.Tensor) else eng.to_device(init_z))
        try:
            if given:
                self._tracking_bind(eng, int(X0t.shape[0]), given)
            if bounds:
                self._tracking_bind(eng, int(X0t.shape[0]), bounds, bind=eng.bind_bounds)
            if rate:
                self._rate_bind(eng, int(X0t.shape[0]), rate)
            if rows:
                eng.bind_rows(*rows)
            duals = gain = None
            if return_duals or return_gain:
                Z, status, iters, duals = eng.solve(X0t, Zi, lb, ub, return_duals=True, **solver_opts)
            else:
                Z, status, iters = eng.solve(X0t, Zi, lb, ub, **solver_opts)
            if return_gain:
                sens = eng.sensitivity(Z, X0t, duals["lam"], duals["zl"], duals["zu"], lb, ub, want=("du0",))
                gain = sens["du0"].to("cpu", torch.float64).numpy()
                self.last_gain_status = sens["status"].cpu().numpy()
        finally:
            if given:       # the engine is NMPC.next's too: back to the shared objective
                eng.bind_tracking()
            if bounds:
                eng.bind_bounds()
            if rate:
                eng.bind_rate()
            if rows:
                eng.bind_rows()
        self.last_batch_iterations = iters
        z = Z.to("cpu", torch.float64).numpy()
        B, nx, nu = z.shape[0], eng.nx, eng.nu
        res = (z[:, :H * nx].reshape(B, H, nx), z[:, H * nx:].reshape(B, H, nu), status.cpu().numpy())
        return res + ((duals,) if return_duals else ()) + ((gain,) if return_gain else ())

    def closed_loop_batch(self, X0, steps, p=None, prev_x=None, prev_u=None, disturbance=None, xref=None, uref=None, cx=None,
                          cu=None, xlb=None, xub=None, ulb=None, uub=None, u_prev=None, du_weight=None, du_lb=None, du_ub=None,
                          **solver_opts):
        """B closed loops of `steps` MPC steps on the device, the plant being the model itself (no reference counterpart:
        the reference's examples step their plant on the host between NMPC.next calls).  Preconditions as next_batch.  Per
        step, on device tensors only: (1) solve -- step 0 from solver_opts' init ("tile" by default), later steps from the
        warm start below with mu_init = 1e-4; (2) apply u_0: x+ = Phi(x0, u0) exactly, the first state of the roll-out of the
        solved controls (not the solver's state, which satisfies the dynamics to tol_constraint), plus disturbance[:, k]
        (B, steps, nx) when given; (3) warm start: the controls shifted by one stage, the last repeated, and their roll-out
        from the new x0, so the start satisfies the dynamics also after a disturbance; (4) rolling-window models: the histories
        take in x0 / u0 and are bound again.  The host waits in the solver's own convergence polls and in the final copy only.
        xref / cx (B, steps+H-1, nx) and uref / cu (B, steps+H-1, nu) (or one (steps+H-1, d) schedule for all problems) are
        per-problem references / linear costs over the whole run: step k scores its horizon against rows k .. k+H-1, bound
        by offset into the same device tensor (no copy, no synchronisation per step); left out, the QuadraticObjective's
        (H,d) values serve every step.  xlb / xub (B, steps+H-1, nx) and ulb / uub (B, steps+H-1, nu) (or one (steps+H-1, d)
        schedule) are per-problem, time-varying bounds over the whole run in the same way: step k solves inside rows
        k .. k+H-1 (row 0 of a u schedule bounds the control applied at step 0, row 0 of an x schedule the state it leads to),
        intersected with the DomainConstraint and the box rows.  u_prev (B,nu) or (nu,) (the control applied before step 0),
        du_weight (nu,nu), du_lb / du_ub (nu,) or (H,nu) add an input-rate penalty and rate limits to every solve
        (next_batch): after each step the applied u_0 becomes u_prev of the next solve, on the device; the shifted warm start
        is unchanged.  LinearStageConstraints of the constraint list hold in every solve (next_batch; not together with rate
        arguments, per-problem references or bounds).  Returns (X (B,steps+1,nx), U (B,steps,nu), status (steps,B)) as NumPy arrays."""
        import torch
        model = self.integrator.model
        steps = int(steps)
        if steps < 1:
            raise ValueError("steps must be >= 1")
        given = self._tracking_check(X0, steps + int(self.integrator.H) - 1, "closed_loop_batch", xref=xref, uref=uref, cx=cx, cu=cu)
        bounds = self._tracking_check(X0, steps + int(self.integrator.H) - 1, "closed_loop_batch", xlb=xlb, xub=xub, ulb=ulb, uub=uub)
        rate = self._rate_check(X0, "closed_loop_batch", u_prev, du_weight, du_lb, du_ub)
        rows = self._stage_rows("closed_loop_batch", **{"rate arguments": rate, "per-problem references": given,
                                                        "per-problem bounds": bounds})
        if int(getattr(model, "tvp_dim", 0)) > 0:
            raise NotImplementedError("closed_loop_batch: models with time-varying parameters (tvp_dim > 0) are not supported -- "
                                      "a closed loop of `steps` steps needs a tvp schedule of H + steps - 1 rows, longer than the "
                                      "horizon NMPC takes")
        eng, X, lb, ub = self._batch_engine(X0, p, None, prev_x, prev_u, None, "closed_loop_batch")
        B, H, nx, nu = int(X.shape[0]), eng.H, eng.nx, eng.nu
        D = None
        if disturbance is not None:
            D = disturbance if isinstance(disturbance, torch.Tensor) else eng.to_device(np.asarray(disturbance, dtype=np.float64))
            if tuple(D.shape) != (B, steps, nx):
                raise ValueError(f"disturbance must have shape {(B, steps, nx)}, got {tuple(D.shape)}")
        w = eng.rolling_window
        hx, hu = eng._history if w > 1 else (None, None)
        warm_opts = {k: v for k, v in solver_opts.items() if k != "init"}
        warm_opts["mu_init"] = 1e-4
        Xs, Us, Ss, iters, Zi = [X], [], [], [], None
        try:
            track = self._tracking_bind(eng, B, given) if given else None
            bnd = self._tracking_bind(eng, B, bounds, bind=eng.bind_bounds) if bounds else None
            up = self._rate_bind(eng, B, rate) if rate else None
            if rows:
                eng.bind_rows(*rows)
            for k in range(steps):
                if track and k > 0:                               # the horizon's window of the schedules: rows k .. k+H-1
                    eng.bind_tracking(**track, offset=k)
                if bnd and k > 0:
                    eng.bind_bounds(**bnd, offset=k)
                Z, status, it = eng.solve(X, Zi, lb, ub, **(solver_opts if k == 0 else warm_opts))[:3]
                iters.append(it)
                U = Z[:, H * nx:].reshape(B, H, nu).clone()
                eng.rollout(X, Z=Z)                               # the plant is the model: x+ = Phi(x0, u0)
                Xn = Z[:, :nx].clone()
                if D is not None:
                    Xn = Xn + D[:, k]
                if w > 1:                                         # the window moves on by one step
                    hx = torch.cat([hx[:, 1:], X[:, None, :]], dim=1).contiguous()
                    hu = torch.cat([hu[:, 1:], U[:, :1]], dim=1).contiguous()
                    eng.bind_history(hx, hu)
                X = Xn.contiguous()
                Zi = eng.rollout(X, U=torch.cat([U[:, 1:], U[:, -1:]], dim=1))
                Xs.append(X)
                Us.append(U[:, 0])
                if up is not None:                                # the applied control is the next solve's u_prev (bound tensor, in place)
                    up.copy_(U[:, 0])
                Ss.append(status)
        finally:
            if given:       # the engine is NMPC.next's too: back to the shared objective
                eng.bind_tracking()
            if bounds:
                eng.bind_bounds()
            if rate:
                eng.bind_rate()
            if rows:
                eng.bind_rows()
        self.last_closed_loop_iterations = iters      # outer iterations of every step's solve (a list; next_batch's int is last_batch_iterations)
        return (torch.stack(Xs, dim=1).to("cpu", torch.float64).numpy(), torch.stack(Us, dim=1).to("cpu", torch.float64).numpy(),
                torch.stack(Ss, dim=0).cpu().numpy())

MPC = NMPC  # BASELINE.json's north_star calls the entry point controller.MPC
