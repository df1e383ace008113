"""torch.autograd through the batched solver: `solve(eng, X0, xref=..., cu=...)` returns the solver's Z as a tensor that
`loss.backward()` differentiates with respect to the initial states, the per-problem tracking data, the extra network inputs
p / tvp (`extra=`), the cost weights (`Q=`, `R=`, `QT=`) and -- with `weights=` -- the weights and biases of the network.

The backward pass is one adjoint KKT solve (CallbackEngine.kkt_solve, nempc_kkt_solve): at the returned primal-dual point the
KKT matrix K = [[W + Sigma, J'], [J, 0]] is symmetric, so with K [v ; w] = [Zbar ; 0] the cotangent of a parameter theta is
-[v ; w]' d/dtheta [grad L ; g]:

    X0bar      = gx0                      (the solve's own pull-back)
    xrefbar[t] = Qs_t v_x[t]              Qs = Q + Q', QT + QT' at t = H-1
    urefbar[t] = Rs v_u[t]                Rs = R + R'
    cxbar      = -v_x,      cubar = -v_u
    thetabar   = -gtheta                  gtheta = [v ; w]' d/dtheta [grad L ; g]   (CallbackEngine.weight_grad, nempc_weight_grad:
                                          the objective and the bound terms do not depend on theta, g = Phi - x does)
    extrabar   = -gE                      gE[b,t] = d/d e_{b,t} of the same form    (CallbackEngine.extra_grad, nempc_extra_grad:
                                          per row; again only g depends on the extras)
    Qbar       = -sum_b sum_t ( v_x[t] dx_t' + dx_t v_x[t]' )     dx_t = x_t - xref_{b,t}; over the steps Q weighs: every t when
    QTbar      = the same term at t = H-1                          the handle has no terminal weight, else t < H-1
    Rbar       = -sum_b sum_t ( v_u[t] du_t' + du_t v_u[t]' )     du_t = u_t - uref_{b,t}
                                          (d/dQ_kl [(Q + Q') dx]_i = delta_ik dx_l + delta_il dx_k; xref_{b,t} is the bound
                                          tracking row where one is bound, else the shared one)

The network's weights and Q, R, QT are SHARED by the batch, so their cotangents are sums over the problems.  A failed problem
(solver status 1, or a KKT solve that reports status != 0) is always left out of those sums -- one NaN would poison every
parameter --, whatever `on_fail` says: `on_fail` keeps its meaning for the per-problem inputs only (X0, the tracking data,
the extras).

NOT differentiated: the bounds lb / ub and the rows of bind_bounds (on the central path the gradients with respect to a lower
/ an upper bound are Sigma_l * v and Sigma_u * v, Sigma_l = zl / (z - lb), Sigma_u = zu / (ub - z): a Sigma of up to 1e11 times
a v that vanishes there, which needs an error study of its own; a caller who needs them forms them from `kkt_solve`'s v and the
duals of `eng.solve`), and the histories of rolling-window models (the library's post-solve calls refuse such handles).

The module uses torch and four members of the engine only -- `solve(X0, lb=, ub=, return_duals=True, ...)`,
`kkt_solve(...)`, `bind_tracking(...)` and `objective_weights()`; with `weights=` also `set_weights(weights, biases)` and
`weight_grad(Z, X0, w, lam=, v=, skip=, flat=True)`; with `extra=` also `bind_extra(E)` and `extra_grad(Z, X0, w, lam=, v=)`;
with `Q=` / `R=` / `QT=` also `set_objective_weights(Q=, R=, QT=)`, `objective_refs()` and `has_terminal_weight` -- and assumes
nothing about the device: any object that offers them works (tests/test_autograd_cpu.py,
tests/test_weight_grad_autograd_cpu.py and tests/test_extra_grad_autograd_cpu.py run it on float64 CPU stubs).
"""
import torch

_NAMES = ("xref", "uref", "cx", "cu")
_NFIXED = 11          # arguments of _Solve.forward in front of the network's weights


class _Solve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, eng, opts, X0, xref, uref, cx, cu, extra, Q, R, QT, *weights):
        cost = {k: t.detach().to(device="cpu", dtype=torch.float64).numpy() for k, t in (("Q", Q), ("R", R), ("QT", QT)) if t is not None}
        if cost:
            eng.set_objective_weights(**cost)
        extra_d = None if extra is None else extra.detach().contiguous()
        if extra_d is not None:
            eng.bind_extra(extra_d)
        if weights:
            host = [t.detach().to(device="cpu", dtype=torch.float64).numpy() for t in weights]
            eng.set_weights(host[0::2], host[1::2])
        given = {k: t.detach().contiguous() for k, t in zip(_NAMES, (xref, uref, cx, cu)) if t is not None}
        X0d = X0.detach().contiguous()
        if given:
            eng.bind_tracking(**given)
        res = eng.solve(X0d, lb=opts["lb"], ub=opts["ub"], return_duals=True, **opts["solve_kw"])
        Z, status, duals = res[0], res[1], res[-1]
        # (clones: the point must survive whatever the engine does with its tensors until backward)
        ctx.eng, ctx.opts, ctx.given, ctx.extra = eng, opts, given, extra_d
        ctx.cmeta = {k: (t.device, t.dtype) for k, t in (("Q", Q), ("R", R), ("QT", QT)) if t is not None}
        ctx.wmeta = [(tuple(t.shape), t.device, t.dtype) for t in weights]
        ctx.saved = (Z.detach().clone(), X0d, duals["lam"].clone(), duals["zl"].clone(), duals["zu"].clone(), status.clone())
        ctx.mark_non_differentiable(status)
        return Z, status

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gZ, _gstatus):
        eng, opts = ctx.eng, ctx.opts
        Z, X0, lam, zl, zu, status = ctx.saved
        if ctx.given:
            eng.bind_tracking(**ctx.given)
        if ctx.extra is not None:
            eng.bind_extra(ctx.extra)
        need = ctx.needs_input_grad
        need_theta = any(need[_NFIXED:])
        out = eng.kkt_solve(Z, X0, lam, zl, zu, opts["lb"], opts["ub"], rz=gZ.contiguous(),
                            want=("v", "gx0", "w") if need_theta or need[7] else ("v", "gx0"))
        v, gx0 = out["v"], out["gx0"]
        B, nx = X0.shape
        Q, R, QT = (torch.as_tensor(a, dtype=torch.float64).to(device=v.device, dtype=v.dtype) for a in eng.objective_weights())
        nu = R.shape[0]
        H = v.shape[1] // (nx + nu)
        vx, vu = v[:, :H * nx].reshape(B, H, nx), v[:, H * nx:].reshape(B, H, nu)
        failed = (status != 0) | (out["status"] != 0)
        fill = float("nan") if opts["on_fail"] == "nan" else 0.0

        def done(g):
            return torch.where(failed.reshape((B,) + (1,) * (g.dim() - 1)), torch.full_like(g, fill), g)

        grads = [None, None, done(gx0) if need[2] else None] + [None] * (_NFIXED - 3 + len(ctx.wmeta))
        if need[3]:
            g = vx @ (Q + Q.T)
            g[:, H - 1] = vx[:, H - 1] @ (QT + QT.T)
            grads[3] = done(g)
        if need[4]:
            grads[4] = done(vu @ (R + R.T))
        if need[5]:
            grads[5] = done(-vx)
        if need[6]:
            grads[6] = done(-vu)
        if need[7]:
            gE = eng.extra_grad(Z, X0, out["w"].contiguous(), lam=lam, v=v.contiguous())
            grads[7] = done(-gE)
        if need[8] or need[9] or need[10]:
            # (failed problems are skipped, as in the weight gradient: Q, R, QT are shared by the batch.  The kept problems are
            # gathered first, so that the sums are those of the batch without the failed ones)
            kept = (~failed).nonzero().reshape(-1)
            xs, us = Z[:, :H * nx].reshape(B, H, nx), Z[:, H * nx:].reshape(B, H, nu)
            refs = eng.objective_refs()
            bound = dict(getattr(eng, "tracking_refs", dict)())
            bound.update(ctx.given)

            def ref_of(name, shared):
                if name in bound:
                    return bound[name].to(device=v.device, dtype=v.dtype)[:B, :H]
                return torch.as_tensor(shared, dtype=torch.float64).to(device=v.device, dtype=v.dtype)[None]

            def bar(vv, dd, ts, key):
                a, d = vv.index_select(0, kept)[:, ts], dd.index_select(0, kept)[:, ts]
                g = -(torch.einsum("btk,btl->kl", a, d) + torch.einsum("btk,btl->kl", d, a))
                return g.to(device=ctx.cmeta[key][0], dtype=ctx.cmeta[key][1])

            dx, du = xs - ref_of("xref", refs[0]), us - ref_of("uref", refs[1])
            term = "QT" in ctx.cmeta or bool(getattr(eng, "has_terminal_weight", False))
            if need[8]:
                grads[8] = bar(vx, dx, slice(0, H - 1) if term else slice(0, H), "Q")
            if need[9]:
                grads[9] = bar(vu, du, slice(0, H), "R")
            if need[10]:
                grads[10] = bar(vx, dx, slice(H - 1, H), "QT")
        if need_theta:
            # (failed problems are skipped, not filled: the sum over the batch is shared by every parameter)
            gtheta = eng.weight_grad(Z, X0, out["w"].contiguous(), lam=lam, v=v.contiguous(), skip=failed, flat=True)
            at = 0
            for i, (shape, dev, dt) in enumerate(ctx.wmeta):
                k = 1
                for d in shape:
                    k *= int(d)
                if need[_NFIXED + i]:
                    grads[_NFIXED + i] = (-gtheta[at:at + k]).reshape(shape).to(device=dev, dtype=dt)
                at += k
        return tuple(grads)


def solve(eng, X0, *, xref=None, uref=None, cx=None, cu=None, lb=None, ub=None, on_fail="nan", weights=None, extra=None,
          Q=None, R=None, QT=None, **solve_kw):
    """Batched solve whose result is differentiable: returns (Z (B,n), status (B,) int32) of `eng.solve(X0, lb=lb, ub=ub,
    **solve_kw)` with the per-problem tracking data xref, cx (B,H,nx), uref, cu (B,H,nu) bound (those given; the others keep
    the shared values of set_objective).  Z carries a gradient with respect to those of X0, xref, uref, cx, cu that require
    one; status does not.  Backward is one `eng.kkt_solve` at the returned point with the returned multipliers (module
    docstring); a problem whose solver status is 1 or whose KKT solve reports status != 0 (not a strict minimiser, undefined
    barrier term) gets NaN gradients, or zeros with on_fail="zero".

    The function binds the tracking tensors it is given with `eng.bind_tracking` in forward AND again in backward, and
    leaves that binding on the engine: a later plain `eng.solve` sees it until the caller binds something else or removes
    it with `eng.bind_tracking()`.  History bindings -- and the extras binding and the objective weights when they are not
    passed here -- are the caller's and must be the same at backward as at forward.  Not differentiated: lb / ub and the rows
    of bind_bounds, histories of rolling-window models (module docstring).

    extra: None, or the extra network inputs as a (B,H,n_extra) tensor on the engine's device and dtype.  Forward binds its
    detached value with `eng.bind_extra` -- the binding stays on the engine, like the tracking binding --, backward re-binds it
    and Z carries a gradient with respect to it: one `eng.extra_grad` call on top of the adjoint solve, per row.  It is a
    per-problem input: a failed problem gets the `on_fail` fill.  p and tvp are written in torch,
        extra = torch.cat([tvp, p[:, None, :].expand(-1, H, -1)], -1)
    and torch's own autograd then does the sum over t for p (and over b for a p shared by the batch).

    Q, R, QT: None, or the cost weights as torch tensors (nx,nx), (nu,nu), (nx,nx) on any device and dtype.  Forward uploads
    the detached values with `eng.set_objective_weights` (xref / uref / cx / cu and the weights not given stay as last set;
    they stay on the engine) and Z carries a gradient with respect to those that require one, formed in torch from the adjoint
    solve's v (module docstring).  They are shared by the batch: FAILED PROBLEMS ARE ALWAYS SKIPPED in their gradients.

    weights: None, or the network's parameters as a flat list [W_0, b_0, W_1, b_1, ...] of torch tensors (any device and
    dtype; W_l (in_l,out_l), b_l (out_l,)).  Forward uploads their detached values with `eng.set_weights` -- they stay on the
    engine -- and Z then carries a gradient with respect to those that require one: one `eng.weight_grad` call on top of the
    adjoint solve, returned on each tensor's device and dtype.  The weights are shared by the batch: FAILED PROBLEMS ARE ALWAYS
    SKIPPED in their gradient (a NaN would poison every parameter); `on_fail` decides about the per-problem inputs only.
    solve_kw goes to `eng.solve` (Z_init, max_iter, barrier, ...; return_duals is set here)."""
    if on_fail not in ("nan", "zero"):
        raise ValueError("on_fail must be 'nan' or 'zero'")
    if "return_duals" in solve_kw or "return_iterations" in solve_kw:
        raise ValueError("return_duals / return_iterations are not options of autograd.solve")
    opts = dict(lb=lb, ub=ub, on_fail=on_fail, solve_kw=solve_kw)
    weights = () if weights is None else tuple(weights)
    if len(weights) % 2 or any(not isinstance(t, torch.Tensor) for t in weights):
        raise ValueError("weights must be a flat list [W_0, b_0, W_1, b_1, ...] of torch tensors")
    for name, t in (("extra", extra), ("Q", Q), ("R", R), ("QT", QT)):
        if t is not None and not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor")
    return _Solve.apply(eng, opts, X0, xref, uref, cx, cu, extra, Q, R, QT, *weights)
