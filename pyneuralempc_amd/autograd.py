"""torch.autograd through the batched solver: `solve(eng, X0, xref=..., cu=...)` returns the solver's Z as a tensor that
`loss.backward()` differentiates with respect to the initial states and the per-problem tracking data.

The backward pass is one adjoint KKT solve (CallbackEngine.kkt_solve, nempc_kkt_solve): at the returned primal-dual point the
KKT matrix K = [[W + Sigma, J'], [J, 0]] is symmetric, so with K [v ; w] = [Zbar ; 0] the cotangent of a parameter theta is
-[v ; w]' d/dtheta [grad L ; g]:

    X0bar      = gx0                      (the solve's own pull-back)
    xrefbar[t] = Qs_t v_x[t]              Qs = Q + Q', QT + QT' at t = H-1
    urefbar[t] = Rs v_u[t]                Rs = R + R'
    cxbar      = -v_x,      cubar = -v_u

NOT differentiated: the network's weights, the extra inputs p / tvp, the weights Q / R / QT, and the bounds lb / ub (on the
central path the gradients with respect to a lower / an upper bound are Sigma_l * v and Sigma_u * v, Sigma_l = zl / (z - lb),
Sigma_u = zu / (ub - z): a caller who needs them forms them from `kkt_solve`'s v and the duals of `eng.solve`).

The module uses torch and four members of the engine only -- `solve(X0, lb=, ub=, return_duals=True, ...)`,
`kkt_solve(...)`, `bind_tracking(...)` and `objective_weights()` -- and assumes nothing about the device: any object that
offers them works (tests/test_autograd_cpu.py runs it on a float64 CPU stub).
"""
import torch

_NAMES = ("xref", "uref", "cx", "cu")


class _Solve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, eng, opts, X0, xref, uref, cx, cu):
        given = {k: t.detach().contiguous() for k, t in zip(_NAMES, (xref, uref, cx, cu)) if t is not None}
        X0d = X0.detach().contiguous()
        if given:
            eng.bind_tracking(**given)
        res = eng.solve(X0d, lb=opts["lb"], ub=opts["ub"], return_duals=True, **opts["solve_kw"])
        Z, status, duals = res[0], res[1], res[-1]
        # (clones: the point must survive whatever the engine does with its tensors until backward)
        ctx.eng, ctx.opts, ctx.given = eng, opts, given
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
        out = eng.kkt_solve(Z, X0, lam, zl, zu, opts["lb"], opts["ub"], rz=gZ.contiguous(), want=("v", "gx0"))
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

        need = ctx.needs_input_grad
        grads = [None, None, done(gx0) if need[2] else None, None, None, None, None]
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
        return tuple(grads)


def solve(eng, X0, *, xref=None, uref=None, cx=None, cu=None, lb=None, ub=None, on_fail="nan", **solve_kw):
    """Batched solve whose result is differentiable: returns (Z (B,n), status (B,) int32) of `eng.solve(X0, lb=lb, ub=ub,
    **solve_kw)` with the per-problem tracking data xref, cx (B,H,nx), uref, cu (B,H,nu) bound (those given; the others keep
    the shared values of set_objective).  Z carries a gradient with respect to those of X0, xref, uref, cx, cu that require
    one; status does not.  Backward is one `eng.kkt_solve` at the returned point with the returned multipliers (module
    docstring); a problem whose solver status is 1 or whose KKT solve reports status != 0 (not a strict minimiser, undefined
    barrier term) gets NaN gradients, or zeros with on_fail="zero".

    The function binds the tracking tensors it is given with `eng.bind_tracking` in forward AND again in backward, and
    leaves that binding on the engine: a later plain `eng.solve` sees it until the caller binds something else or removes
    it with `eng.bind_tracking()`.  Extras / history bindings and the objective weights are the caller's and must be the
    same at backward as at forward.  Not differentiated: network weights, p / tvp, Q / R / QT, lb / ub (module docstring).
    solve_kw goes to `eng.solve` (Z_init, max_iter, barrier, ...; return_duals is set here)."""
    if on_fail not in ("nan", "zero"):
        raise ValueError("on_fail must be 'nan' or 'zero'")
    if "return_duals" in solve_kw or "return_iterations" in solve_kw:
        raise ValueError("return_duals / return_iterations are not options of autograd.solve")
    opts = dict(lb=lb, ub=ub, on_fail=on_fail, solve_kw=solve_kw)
    return _Solve.apply(eng, opts, X0, xref, uref, cx, cu)
