"""CPU: pyneuralempc_amd.autograd.solve(..., weights=...) on the stub engine of tests/test_autograd_cpu.py extended with
`set_weights` / `weight_grad` backed by tests/weight_grad_reference.py (float64)."""
import numpy as np
import pytest
import torch

from oracle import nempc_oracle as orc
from pyneuralempc_amd import autograd as nag
import kkt_solve_reference as kref
import sensitivity_reference as sref
import solver_step_cases as sc
import weight_grad_reference as wref
from test_autograd_cpu import StubEngine, _inputs


class _CaseView:
    """a solver_step_cases.Case with its network replaced (the stub's _problem reads .net)"""

    def __init__(self, case, net):
        self.__dict__.update(case.__dict__)
        self.net = net


class WeightStub(StubEngine):
    """+ set_weights / weight_grad; kkt_solve also returns w.  mode: "ok", "no_second_order" (drops lam . T v) or "flipped"
    (returns -gtheta): the two broken stubs the gradcheck must reject."""

    def __init__(self, case, failed=(), mode="ok"):
        super().__init__(case, failed)
        self.mode = mode

    def set_weights(self, weights, biases):
        c = self.case
        assert [w.shape for w in weights] == [w.shape for w in c.net.W] and [b.shape for b in biases] == [b.shape for b in c.net.b]
        self.case = _CaseView(c, orc.MLP([np.array(w) for w in weights], [np.array(b) for b in biases], c.net.act))
        self.calls.append(("set_weights",))

    def kkt_solve(self, Z, X0, lam, zl=None, zu=None, lb=None, ub=None, rz=None, rg=None, want=("v",)):
        c, B = self.case, Z.shape[0]
        out = super().kkt_solve(Z, X0, lam, zl, zu, lb, ub, rz, rg, want=tuple(k for k in want if k != "w"))
        if "w" in want:
            w = np.zeros((B, c.H * c.nx))
            for b in range(B):
                stage = sref.stage_data(self._problem(b), Z[b].numpy(), X0[b].numpy(), lam[b].numpy())
                w[b] = kref.dense_solve(stage, c.H, c.nx, c.nu, None, rz[b].numpy())["w"][0]
            out["w"] = torch.from_numpy(w)
        for b in self.failed:            # what the library hands back for a failed problem
            for k in ("v", "w", "gx0"):
                if k in out:
                    out[k][b] = float("nan")
        return out

    def weight_grad(self, Z, X0, w, lam=None, v=None, skip=None, flat=False):
        c = self.case
        assert flat and w.is_contiguous() and v.is_contiguous()
        p = wref.TorchPhi(c.net, c.H, c.nx, c.nu, sc.KINDS[c.integ], c.DT)
        keep = None if skip is None else (~skip.bool()).numpy().astype(np.int64)
        if self.mode == "no_second_order":
            lam = v = None
        g = p.gtheta(Z.numpy(), X0.numpy(), w.numpy(), None if lam is None else lam.numpy(), None if v is None else v.numpy(), keep=keep)
        self.calls.append(("weight_grad",))
        return torch.from_numpy(-g if self.mode == "flipped" else g)


def _theta(case):
    out = []
    for W, b in zip(case.net.W, case.net.b):
        out += [torch.tensor(W, dtype=torch.float64, requires_grad=True), torch.tensor(b, dtype=torch.float64, requires_grad=True)]
    return out


def _gradcheck(row, H, mode):
    case = sc.qp_case(row, H)
    eng = WeightStub(case, mode=mode)
    X0, per = _inputs(case, 2)
    X0 = X0.detach()

    def fn(*theta):
        Z, _ = nag.solve(eng, X0, xref=per["xref"].detach(), cu=per["cu"].detach(), weights=list(theta))
        return Z

    return torch.autograd.gradcheck(fn, tuple(_theta(case)), raise_exception=False), eng


@pytest.mark.parametrize("row,H", [("2x1_discret", 3), ("3x2_unity", 7)])
def test_gradcheck_over_the_weights(row, H):
    """torch.autograd.gradcheck (float64, its default tolerances) of Z over every weight and bias, two problems.  Verified
    once that the check has teeth: with the stub's weight_grad dropping the lam . T v term (mode "no_second_order") and with
    its sign flipped (mode "flipped") gradcheck returns False on both rows -- asserted below, so it stays verified."""
    ok, eng = _gradcheck(row, H, "ok")
    assert ok
    names = [c[0] for c in eng.calls]
    assert "set_weights" in names and "weight_grad" in names
    assert not _gradcheck(row, H, "no_second_order")[0]
    assert not _gradcheck(row, H, "flipped")[0]


def test_failed_problems_are_skipped_in_the_weight_gradient_whatever_on_fail_says():
    case = sc.qp_case("2x1_discret", 3)
    grads = {}
    for on_fail in ("nan", "zero"):
        eng = WeightStub(case, failed=(1,))
        X0, _ = _inputs(case, 3)
        theta = _theta(case)
        Z, status = nag.solve(eng, X0, weights=theta, on_fail=on_fail)
        assert status.tolist() == [0, 1, 0]
        C = torch.tensor(np.random.default_rng(3).normal(size=Z.shape))
        (C * Z).sum().backward()
        assert all(bool(torch.isfinite(t.grad).all()) for t in theta) and float(theta[0].grad.abs().max()) > 0.0
        bad = X0.grad[1]
        assert bool(torch.isnan(bad).all()) if on_fail == "nan" else bool((bad == 0).all())
        grads[on_fail] = [t.grad.clone() for t in theta]
        # the batch without the failed problem
        eng2 = WeightStub(case)
        sel = torch.tensor([0, 2])
        theta2 = _theta(case)
        Z2, _ = nag.solve(eng2, X0.detach()[sel], weights=theta2)
        (C[sel] * Z2).sum().backward()
        for t, t2 in zip(theta, theta2):
            assert float((t.grad - t2.grad).abs().max()) <= 1e-12 * (1.0 + float(t2.grad.abs().max()))
    assert all(torch.equal(a, b) for a, b in zip(grads["nan"], grads["zero"]))


def test_weights_that_need_no_gradient_cost_no_weight_grad_call():
    case = sc.qp_case("2x1_discret", 3)
    eng = WeightStub(case)
    X0, _ = _inputs(case, 2)
    theta = [t.detach() for t in _theta(case)]
    Z, _ = nag.solve(eng, X0, weights=theta)
    Z.sum().backward()
    names = [c[0] for c in eng.calls]
    assert names.count("set_weights") == 1 and "weight_grad" not in names and X0.grad is not None
    with pytest.raises(ValueError):
        nag.solve(eng, X0, weights=theta[:-1])
