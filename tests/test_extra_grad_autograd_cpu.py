"""CPU: pyneuralempc_amd.autograd.solve(..., extra=, Q=, R=, QT=) on a float64 stub engine whose solve / kkt_solve are the
reference (exact on the linear networks of the QP rows: one Newton step solves the problem) and whose extra_grad is
tests/extra_grad_reference.py's formula."""
import numpy as np
import pytest
import torch

from oracle import nempc_oracle as orc
from pyneuralempc_amd import autograd as nag
import kkt_reference as kkt
import kkt_solve_reference as kref
import sensitivity_reference as sref
import solver_step_cases as sc
from weight_grad_reference import TorchPhi

H, NE = 3, 2


class ExtraStub:
    """What autograd.solve uses of CallbackEngine, on the CPU in float64, unbounded problems: solve, kkt_solve (v, w, gx0),
    bind_tracking, bind_extra, extra_grad, objective_weights, set_objective_weights, objective_refs, has_terminal_weight.
    mode "flipped" returns -gE from extra_grad: the broken stub the gradcheck must reject."""

    def __init__(self, case, failed=(), terminal=True, mode="ok"):
        self.case, self.failed, self.mode, self.binding, self.extra, self.calls = case, set(failed), mode, {}, None, []
        self.obj = dict(case.obj)
        if not terminal:
            self.obj["QT"] = None

    has_terminal_weight = property(lambda self: self.obj["QT"] is not None)

    def bind_tracking(self, xref=None, uref=None, cx=None, cu=None, offset=0):
        self.binding = {k: v.detach().numpy().copy() for k, v in (("xref", xref), ("uref", uref), ("cx", cx), ("cu", cu)) if v is not None}
        self.calls.append(("bind", tuple(sorted(self.binding))))

    def bind_extra(self, E):
        assert E.shape[1:] == (self.case.H, self.case.n_extra) and E.is_contiguous() and not E.requires_grad
        self.extra = E.numpy().copy()
        self.calls.append(("bind_extra",))

    def set_objective_weights(self, Q=None, R=None, QT=None):
        for k, a in (("Q", Q), ("R", R), ("QT", QT)):
            if a is not None:
                self.obj[k] = np.array(a, dtype=np.float64)
        self.calls.append(("set_objective_weights", tuple(k for k, a in (("Q", Q), ("R", R), ("QT", QT)) if a is not None)))

    def objective_weights(self):
        return self.obj["Q"], self.obj["R"], self.obj["Q"] if self.obj["QT"] is None else self.obj["QT"]

    def objective_refs(self):
        return self.obj["xref"], self.obj["uref"]

    def _problem(self, b):
        c = self.case
        ob = dict(self.obj)
        ob.update({k: v[b] for k, v in self.binding.items()})
        return orc.Problem(c.net, c.H, c.nx, c.nu, sc.KINDS[c.integ], c.DT, extra=self.extra[b], **ob)

    def solve(self, X0, lb=None, ub=None, return_duals=False):
        assert lb is None and ub is None and return_duals
        c, B = self.case, X0.shape[0]
        Z, lam = np.zeros((B, c.n)), np.zeros((B, c.H * c.nx))
        for b in range(B):
            x0 = X0[b].numpy()
            z0 = orc.cold_start(x0, c.H, c.nu)
            dz, lam[b], _, _ = kkt.newton_step(self._problem(b), z0, x0, np.zeros(c.H * c.nx), 0.0, diagnostics=False)
            Z[b] = z0 + dz
        status = torch.tensor([1 if b in self.failed else 0 for b in range(B)], dtype=torch.int32)
        duals = {"lam": torch.from_numpy(lam), "zl": torch.zeros(B, c.n, dtype=torch.float64), "zu": torch.zeros(B, c.n, dtype=torch.float64)}
        self.calls.append(("solve",))
        return torch.from_numpy(Z), status, 1, duals

    def kkt_solve(self, Z, X0, lam, zl=None, zu=None, lb=None, ub=None, rz=None, rg=None, want=("v",)):
        c, B = self.case, Z.shape[0]
        assert rg is None and rz.shape == (B, c.n) and rz.is_contiguous()
        out = {"v": np.zeros((B, c.n)), "w": np.zeros((B, c.H * c.nx)), "gx0": np.zeros((B, c.nx))}
        for b in range(B):
            stage = sref.stage_data(self._problem(b), Z[b].numpy(), X0[b].numpy(), lam[b].numpy())
            s = kref.dense_solve(stage, c.H, c.nx, c.nu, None, rz[b].numpy())
            for k in out:
                out[k][b] = s[k][0]
        for b in self.failed:            # what the library hands back for a failed problem
            for k in out:
                out[k][b] = float("nan")
        self.calls.append(("kkt_solve",))
        res = {k: torch.from_numpy(out[k]) for k in want}
        res["status"] = torch.zeros(B, dtype=torch.int32)
        return res

    def extra_grad(self, Z, X0, w, lam=None, v=None):
        c = self.case
        assert w.is_contiguous() and v.is_contiguous()
        p = TorchPhi(c.net, c.H, c.nx, c.nu, sc.KINDS[c.integ], c.DT)
        e = torch.from_numpy(self.extra[:Z.shape[0]]).clone().requires_grad_(True)
        with torch.enable_grad():
            (g,) = torch.autograd.grad(p.S(p.theta0, Z, X0, w, lam, v, e), e)
        self.calls.append(("extra_grad",))
        return -g if self.mode == "flipped" else g


def _case(integ="discret"):
    return sc.Case("extras_" + integ, 2, 1, [8], integ, 0.1 if integ == "rk4" else 1.0, H, ("auto",), "float64", n_extra=NE, act="linear",
                   seed=sc.QP_SEED)


def _t(a):
    return torch.tensor(np.asarray(a), dtype=torch.float64, requires_grad=True)


def _inputs(case, B):
    return _t(case.X0[:B]), _t(case.extra[:B]), _t(case.obj["Q"]), _t(case.obj["R"]), _t(case.obj["QT"])


@pytest.mark.parametrize("with_x0", [False, True], ids=["alone", "with_X0"])
@pytest.mark.parametrize("which", ["extra", "Q", "R", "QT"])
@pytest.mark.parametrize("integ", ["discret", "rk4"])
def test_gradcheck_of_each_new_input(integ, which, with_x0):
    """torch.autograd.gradcheck (float64, its default tolerances) of Z over one of extra, Q, R, QT, alone and together with X0;
    two problems, per-problem xref bound (dx_t is measured from the bound row)"""
    case = _case(integ)
    eng = ExtraStub(case)
    X0, extra, Q, R, QT = _inputs(case, 2)
    xref = torch.tensor(0.1 * np.random.default_rng(2).normal(size=(2, H, case.nx)))
    args = dict(extra=extra, Q=Q, R=R, QT=QT)

    def fn(a, x0=None):
        kw = {k: v.detach() for k, v in args.items()}
        kw[which] = a
        return nag.solve(eng, X0.detach() if x0 is None else x0, xref=xref, **kw)[0]

    inputs = (args[which], X0) if with_x0 else (args[which],)
    assert torch.autograd.gradcheck(fn, inputs)
    names = [c[0] for c in eng.calls]
    assert "bind_extra" in names and "set_objective_weights" in names and (which != "extra" or "extra_grad" in names)


def test_gradcheck_of_all_of_them_together_and_a_flipped_extra_grad_is_caught():
    case = _case()
    X0, extra, Q, R, QT = _inputs(case, 2)
    for mode, expect in (("ok", True), ("flipped", False)):
        eng = ExtraStub(case, mode=mode)
        fn = lambda x0, e, q, r, qt: nag.solve(eng, x0, extra=e, Q=q, R=r, QT=qt)[0]
        assert torch.autograd.gradcheck(fn, (X0, extra, Q, R, QT), raise_exception=False) is expect


def test_Q_weighs_every_step_on_a_handle_without_a_terminal_weight():
    """no QT anywhere: Qbar collects t = H-1 too (gradcheck), and the shared xref is what dx_t is measured from"""
    case = _case()
    eng = ExtraStub(case, terminal=False)
    X0, extra, Q, R, _ = _inputs(case, 2)
    assert not eng.has_terminal_weight
    assert torch.autograd.gradcheck(lambda q, r: nag.solve(eng, X0.detach(), extra=extra.detach(), Q=q, R=r)[0], (Q, R))


def test_a_shared_p_expanded_into_the_extras_receives_the_sum_over_b_and_t():
    """extra = cat([tvp, p expanded]): gradcheck over tvp and p, and p.grad is the sum of its slots of the per-row gradient"""
    case = _case()
    eng = ExtraStub(case)
    B = 3
    X0 = torch.tensor(case.X0[:B])
    tvp, p = _t(case.extra[:B, :, :1]), _t(case.extra[0, 0, 1:])

    def fn(tvp, p):
        extra = torch.cat([tvp, p[None, None, :].expand(B, H, -1)], -1)
        return nag.solve(eng, X0, extra=extra)[0]

    assert torch.autograd.gradcheck(fn, (tvp, p))
    C = torch.tensor(np.random.default_rng(4).normal(size=(B, case.n)))
    (C * fn(tvp, p)).sum().backward()
    full = torch.cat([tvp, p[None, None, :].expand(B, H, -1)], -1).detach().requires_grad_(True)
    (C * nag.solve(eng, X0, extra=full)[0]).sum().backward()
    assert torch.allclose(p.grad, full.grad[:, :, 1:].sum((0, 1)), rtol=1e-13, atol=0) and torch.equal(tvp.grad, full.grad[:, :, :1])


@pytest.mark.parametrize("on_fail", ["nan", "zero"])
def test_a_failed_problem_is_skipped_in_the_cost_weights_and_filled_in_the_extras(on_fail):
    case = _case()
    eng = ExtraStub(case, failed=(1,))
    X0, extra, Q, R, QT = _inputs(case, 3)
    Z, status = nag.solve(eng, X0, extra=extra, Q=Q, R=R, QT=QT, on_fail=on_fail)
    assert status.tolist() == [0, 1, 0]
    C = torch.tensor(np.random.default_rng(3).normal(size=Z.shape))
    (C * Z).sum().backward()
    bad = extra.grad[1]
    assert bool(torch.isnan(bad).all()) if on_fail == "nan" else bool((bad == 0).all())
    assert bool(torch.isfinite(extra.grad[[0, 2]]).all()) and float(extra.grad[0].abs().max()) > 0.0
    # the batch without the failed problem
    eng2 = ExtraStub(case)
    sel = torch.tensor([0, 2])
    X02, extra2, Q2, R2, QT2 = _inputs(case, 3)
    Z2, _ = nag.solve(eng2, X02.detach()[sel], extra=extra2.detach()[sel].contiguous(), Q=Q2, R=R2, QT=QT2)
    (C[sel] * Z2).sum().backward()
    for a, b in ((Q, Q2), (R, R2), (QT, QT2)):
        assert bool(torch.isfinite(a.grad).all()) and float(a.grad.abs().max()) > 0.0
        assert float((a.grad - b.grad).abs().max()) <= 1e-12 * (1.0 + float(b.grad.abs().max()))


def test_inputs_that_need_no_gradient_cost_no_extra_grad_call():
    case = _case()
    eng = ExtraStub(case)
    X0, extra, Q, _, _ = _inputs(case, 2)
    Z, _ = nag.solve(eng, X0, extra=extra.detach(), Q=Q.detach())
    Z.sum().backward()
    names = [c[0] for c in eng.calls]
    assert names.count("bind_extra") == 2 and "extra_grad" not in names and X0.grad is not None
    assert ("set_objective_weights", ("Q",)) in eng.calls
    with pytest.raises(ValueError):
        nag.solve(eng, X0, extra=case.extra[:2])
