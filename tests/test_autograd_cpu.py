"""CPU: pyneuralempc_amd.autograd on a stub engine whose solve / kkt_solve are the float64 reference (exact on the linear
networks of the QP rows: one Newton step solves the problem)."""
import numpy as np
import pytest
import torch

from oracle import nempc_oracle as orc
from pyneuralempc_amd import autograd as nag
import kkt_reference as kkt
import kkt_solve_reference as kref
import sensitivity_reference as sref
import solver_step_cases as sc


class StubEngine:
    """solve / kkt_solve / bind_tracking / objective_weights of CallbackEngine on the CPU in float64, unbounded problems."""

    def __init__(self, case, failed=()):
        self.case, self.failed, self.binding, self.calls = case, set(failed), {}, []

    def bind_tracking(self, xref=None, uref=None, cx=None, cu=None, offset=0):
        self.binding = {k: v.detach().numpy().copy() for k, v in (("xref", xref), ("uref", uref), ("cx", cx), ("cu", cu)) if v is not None}
        self.calls.append(("bind", tuple(sorted(self.binding))))

    def objective_weights(self):
        ob = self.case.obj
        return ob["Q"], ob["R"], ob["QT"]

    def _problem(self, b):
        c = self.case
        ob = dict(c.obj)
        ob.update({k: v[b] for k, v in self.binding.items()})
        return orc.Problem(c.net, c.H, c.nx, c.nu, sc.KINDS[c.integ], c.DT, **ob)

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
        v, gx0 = np.zeros((B, c.n)), np.zeros((B, c.nx))
        for b in range(B):
            stage = sref.stage_data(self._problem(b), Z[b].numpy(), X0[b].numpy(), lam[b].numpy())
            s = kref.dense_solve(stage, c.H, c.nx, c.nu, None, rz[b].numpy())
            v[b], gx0[b] = s["v"][0], s["gx0"][0]
        self.calls.append(("kkt_solve",))
        out = {"v": torch.from_numpy(v), "gx0": torch.from_numpy(gx0), "status": torch.zeros(B, dtype=torch.int32)}
        return {k: out[k] for k in tuple(want) + ("status",)}


def _inputs(case, B, seed=5):
    rng = np.random.default_rng(seed)
    t = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)
    X0 = t(case.X0[:B])
    per = {k: t(sc.REF_SCALE * rng.normal(size=(B, case.H, d))) for k, d in (("xref", case.nx), ("uref", case.nu), ("cx", case.nx), ("cu", case.nu))}
    return X0, per


@pytest.mark.parametrize("row,H", [("2x1_discret", 3), ("3x2_unity", 7)])
def test_gradcheck_over_every_differentiable_input(row, H):
    """torch.autograd.gradcheck (float64, its default tolerances) of Z over X0, xref, uref, cx, cu, two problems."""
    case = sc.qp_case(row, H)
    eng = StubEngine(case)
    X0, per = _inputs(case, 2)

    def fn(X0, xref, uref, cx, cu):
        Z, status = nag.solve(eng, X0, xref=xref, uref=uref, cx=cx, cu=cu)
        assert not status.requires_grad and status.dtype == torch.int32
        return Z

    assert torch.autograd.gradcheck(fn, (X0, per["xref"], per["uref"], per["cx"], per["cu"]))
    # the tracking binding is put back before the adjoint solve and stays on the engine
    i = max(k for k, c in enumerate(eng.calls) if c[0] == "kkt_solve")
    assert eng.calls[i - 1] == ("bind", ("cu", "cx", "uref", "xref")) and set(eng.binding) == {"xref", "uref", "cx", "cu"}


def test_only_inputs_that_require_grad_get_one():
    case = sc.qp_case("2x1_discret", 3)
    eng = StubEngine(case)
    X0, per = _inputs(case, 2)
    X0 = X0.detach()
    cx = per["cx"].detach()
    Z, status = nag.solve(eng, X0, xref=per["xref"], cx=cx, cu=per["cu"])
    assert Z.requires_grad and not status.requires_grad and set(eng.binding) == {"xref", "cx", "cu"}
    c = torch.tensor(np.random.default_rng(1).normal(size=Z.shape))
    (c * Z).sum().backward()
    assert X0.grad is None and cx.grad is None and per["uref"].grad is None
    assert per["xref"].grad.shape == per["xref"].shape and per["cu"].grad.shape == per["cu"].shape
    # against the reference's vjp of problem 1
    g = kref.vjp(eng._problem(1), Z[1].detach().numpy(), X0[1].numpy(), eng.solve(X0, return_duals=True)[3]["lam"][1].numpy(), None,
                 c[1].numpy())
    assert np.abs(per["xref"].grad[1].numpy() - g["xref"]).max() <= 1e-12 * (1.0 + np.abs(g["xref"]).max())
    assert np.abs(per["cu"].grad[1].numpy() - g["cu"]).max() <= 1e-12 * (1.0 + np.abs(g["cu"]).max())
    # nothing requires grad: no graph, no adjoint solve
    n_before = len(eng.calls)
    Z2, _ = nag.solve(eng, X0, cx=cx)
    assert not Z2.requires_grad and [c[0] for c in eng.calls[n_before:]] == ["bind", "solve"]
    with pytest.raises(ValueError):
        nag.solve(eng, X0, on_fail="ignore")
    with pytest.raises(ValueError):
        nag.solve(eng, X0, return_duals=True)


@pytest.mark.parametrize("on_fail", ["nan", "zero"])
def test_failed_problems_get_nan_or_zero_gradients(on_fail):
    case = sc.qp_case("2x1_discret", 3)
    eng = StubEngine(case, failed=(1,))
    X0, per = _inputs(case, 3)
    Z, status = nag.solve(eng, X0, xref=per["xref"], cu=per["cu"], on_fail=on_fail)
    assert status.tolist() == [0, 1, 0]
    Z.sum().backward()
    for g in (X0.grad, per["xref"].grad, per["cu"].grad):
        bad = g[1]
        assert bool(torch.isnan(bad).all()) if on_fail == "nan" else bool((bad == 0).all())
        assert bool(torch.isfinite(g[0]).all()) and bool(torch.isfinite(g[2]).all()) and float(g[0].abs().max()) > 0.0
