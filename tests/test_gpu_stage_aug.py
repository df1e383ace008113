"""GPU: what a stage augmentation of the batched solver keeps between solves on one handle (csrc/solver_aug.h: the objective
table over the augmented stage and the bound vector are uploaded when they change).  A handle that has solved with one
objective, or one set of bounds, and is then given another must solve as a fresh handle given the second from the outset:
Z, status and the per-problem iteration counts bit for bit (the solver has integer atomics only; tests/test_gpu_rate.py
relies on the same run-to-run equality).

2 states, 1 control, one hidden layer of 8, H = 4, B = 3, fp64; once as a rolling-window model (w = 2), once under a rate
binding (S = 0.2, |du| <= 0.1)."""
import numpy as np
import pytest
import torch

from oracle import nempc_oracle as orc

pytestmark = pytest.mark.gpu

NX, NU, H, B = 2, 1, 4, 3
N = H * (NX + NU)
_RNG = np.random.default_rng(33)
X0 = _RNG.uniform(-1.0, 1.0, size=(B, NX))
HX, HU = _RNG.uniform(-1.0, 1.0, size=(B, 1, NX)), _RNG.uniform(-0.3, 0.3, size=(B, 1, NU))
U_PREV = _RNG.uniform(-0.1, 0.1, size=(B, NU))
OBJECTIVES = [dict(Q=np.eye(NX), R=0.1 * np.eye(NU), xref=np.zeros((H, NX)), QT=None),
              dict(Q=np.array([[2.0, 0.3], [0.1, 0.5]]), R=np.array([[0.4]]), xref=np.full((H, NX), 0.25),
                   QT=np.array([[3.0, 0.0], [0.2, 1.5]]))]


def _bounds(umax):
    lb, ub = np.full(N, -np.inf), np.full(N, np.inf)
    lb[H * NX:], ub[H * NX:] = -umax, umax
    return lb, ub


BOUNDS = [_bounds(0.5), _bounds(0.05)]      # (|u_prev| <= 0.1 and |du| <= 0.1: a first control inside +-0.05 exists)


def _engine(kind):
    from pyneuralempc_amd import CallbackEngine
    w = 2 if kind == "window" else 1
    net = orc.MLP.random(w * (NX + NU), [8], NX, seed=4)
    net.W[-1] *= 0.2
    net.b[-1] *= 0.2
    eng = CallbackEngine(net.W, net.b, H, NX, NU, dtype=torch.float64, device="cuda:0", max_batch=B, rolling_window=w)
    if kind == "window":
        eng.bind_history(eng.to_device(HX), eng.to_device(HU))
    else:
        eng.bind_rate(u_prev=eng.to_device(U_PREV), S=0.2 * np.eye(NU), du_lb=np.full(NU, -0.1), du_ub=np.full(NU, 0.1))
    return eng


def _solve(eng, objective, bounds):
    eng.set_objective(**objective)      # (Q, R, xref, and the terminal weight: nempc_set_objective, nempc_set_terminal_weight)
    Z, st, _, per = eng.solve(eng.to_device(X0), None, bounds[0], bounds[1], max_iter=60, return_iterations=True)
    return Z.cpu().numpy(), st.cpu().numpy(), per.cpu().numpy()


@pytest.mark.parametrize("changed", ["objective", "bounds"])
@pytest.mark.parametrize("kind", ["window", "rate"])
def test_a_second_solve_on_one_handle_is_the_solve_of_a_fresh_handle(kind, changed):
    first = (OBJECTIVES[0], BOUNDS[0])
    second = (OBJECTIVES[1], BOUNDS[0]) if changed == "objective" else (OBJECTIVES[0], BOUNDS[1])
    eng = _engine(kind)
    Z1, st1, per1 = _solve(eng, *first)
    Z2, st2, per2 = _solve(eng, *second)           # the same start (the cold start from X0), the handle's workspace kept
    Zf, stf, perf = _solve(_engine(kind), *second)
    print(f"[stage aug {kind}, {changed} changed] status {st1.tolist()} -> {st2.tolist()} (fresh {stf.tolist()}), iterations "
          f"{per1.tolist()} -> {per2.tolist()} (fresh {perf.tolist()}), |Z2 - Z1| = {np.abs(Z2 - Z1).max():.3e}, "
          f"|Z2 - Zfresh| = {np.abs(Z2 - Zf).max():.3e}")
    assert (st1 == 0).all() and (stf == 0).all(), (st1.tolist(), stf.tolist())
    assert np.abs(Z2 - Z1).max() > 1e-3            # (the change is in effect: a table that stayed would pass the rest)
    assert Z2.tobytes() == Zf.tobytes() and st2.tobytes() == stf.tobytes() and per2.tobytes() == perf.tobytes()
    Z3, st3, per3 = _solve(eng, *first)            # ... and back: the first solve again
    assert Z3.tobytes() == Z1.tobytes() and st3.tobytes() == st1.tobytes() and per3.tobytes() == per1.tobytes()
