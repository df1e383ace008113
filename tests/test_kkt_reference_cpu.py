"""The dense KKT reference of the per-step solver checks (tests/kkt_reference.py) checks itself: no GPU.

The GPU tests in tests/test_gpu_solver_steps.py hold the solver's steps against `newton_step` / `replay` / `qp_solution`
to a tolerance derived from `riccati_step`; here those four agree with each other, with the KKT conditions and with SciPy
SLSQP on the oracle's callbacks, on the very shapes the GPU tests use."""
import numpy as np
import pytest

import kkt_reference as kkt
import solver_step_cases as sc

EPS = np.finfo(np.float64).eps


def _agree(prob, z, x0, lam, small_steps=False):
    """small_steps: along a replay the steps shrink to 1e-6 while the right-hand side [grad f ; g] is still evaluated at
    |z| of order one, with a rounding error of a few eps (1 + |z|inf) that the solve amplifies by cond(K) whatever |dz| is:
    that floor, 10 eps cond(K) (1 + |z|inf), is added to the bound."""
    dz, lamn, cond, eig = kkt.newton_step(prob, z, x0, lam, sc.REG)
    dzr, lamr = kkt.riccati_step(prob, z, x0, lam, sc.REG, np.float64)
    bound = 1e3 * EPS * cond * np.abs(dz).max() + (10 * EPS * cond * (1.0 + np.abs(z).max()) if small_steps else 0.0)
    assert np.abs(dzr - dz).max() <= bound, (np.abs(dzr - dz).max(), bound)
    assert np.abs(lamr - lamn).max() <= 1e3 * EPS * cond * max(1.0, np.abs(lamn).max())
    return dz, lamn, eig


@pytest.mark.parametrize("name,H", sc.QP_CASES)
def test_dense_and_riccati_steps_agree_on_the_qp_shapes(name, H):
    """Dense solve against the float64 sweep, to 1e3 eps cond(K) |dz|inf, cold and random start; the rolling shapes go
    through the window-as-state stages.  (H = 355: the condition number of a 1775-square matrix, one problem.)"""
    case = sc.qp_case(name, H)
    for b in ((0,) if H > 100 else (0, case.B - 1)):
        prob = case.problem(b)
        for rnd in (False, True):
            _, _, eig = _agree(prob, case.start(b, rnd), case.X0[b], np.zeros(H * case.nx))
            assert eig > 0.1          # the objective Hessian is positive definite with the non-symmetric weights


@pytest.mark.parametrize("name", list(sc.NL_ROWS))
def test_dense_and_riccati_steps_agree_along_the_nonlinear_replays(name):
    """... and with non-zero multipliers: the Lagrangian blocks enter both the same way."""
    case = sc.nl_case(name)
    for b in (0, case.B - 1):
        prob = case.problem(b)
        for st in kkt.replay(prob, case.X0[b], case.start(b), sc.NL_ROWS[name][8], sc.REG):
            if np.abs(st["dz"]).max() < sc.STOP_STEP:
                break       # (not compared on the GPU either: the error is that of the defects, eps |z|, not eps |dz|)
            _agree(prob, st["z_before"], case.X0[b], st["lam_before"], small_steps=True)


@pytest.mark.parametrize("name", list(sc.NL_ROWS))
def test_every_nonlinear_problem_clears_both_gates(name):
    """What tests/test_gpu_solver_steps.py asserts before it compares: no damping restart (reduced Hessian eigenvalue >=
    0.05) and a strictly decreasing l1 merit under the full step, for all 8 problems at every compared step."""
    for rp, _ in sc.nl_reference(name):
        for st in rp:
            assert st["eig"] >= sc.GATE_EIG and st["dmerit"] < 0.0


@pytest.mark.parametrize("name,H", [("2x1_discret", 20), ("6x3_rk4", 8), ("roll3_rev", 10), ("2x1_extras", 10)])
def test_one_step_solves_the_equality_constrained_qp(name, H):
    """Linear network: the Newton point has zero defect and zero KKT residual (up to the Levenberg term reg |du|), and a
    second step from it is zero."""
    case = sc.qp_case(name, H)
    prob, x0 = case.problem(1), case.X0[1]
    z0 = case.start(1, True)
    dz, lam, _, _ = kkt.newton_step(prob, z0, x0, np.zeros(H * case.nx), sc.REG)
    z = z0 + dz
    assert np.abs(prob.constraints(z, x0)).max() < 1e-12
    assert np.abs(prob.gradient(z) + prob.jacobian(z, x0).T @ lam).max() < 10 * sc.REG * max(1.0, np.abs(dz).max())
    dz2, lam2, _, _ = kkt.newton_step(prob, z, x0, lam, sc.REG)
    assert np.abs(dz2).max() < 1e-7 and np.abs(lam2 - lam).max() < 1e-6


def test_replay_converges_to_the_slsqp_minimum_on_a_tanh_case():
    from scipy.optimize import minimize
    case = sc.nl_case("6x3_rk4")
    prob, x0 = case.problem(0), case.X0[0]
    rp = kkt.replay(prob, x0, case.start(0), 8, sc.REG)
    z = rp[-1]["z"]
    assert np.abs(rp[-1]["dz"]).max() < 1e-10            # quadratic convergence: long since at the solution
    res = minimize(prob.objective, case.start(0), method="SLSQP", jac=prob.gradient,
                   constraints=[{"type": "eq", "fun": lambda v: prob.constraints(v, x0), "jac": lambda v: prob.jacobian(v, x0)}],
                   options={"maxiter": 500, "ftol": 1e-14})
    assert res.success
    np.testing.assert_allclose(z, res.x, rtol=0, atol=1e-5)
    assert abs(prob.objective(z) - res.fun) < 1e-9
    # the replayed multipliers are those of the minimum
    assert np.abs(prob.gradient(z) + prob.jacobian(z, x0).T @ rp[-1]["lam"]).max() < 1e-8


def test_fp32_sweep_loses_what_fp32_can_lose():
    """riccati_step in float32 is the same sweep at single precision: its distance from the dense step is a few thousand eps
    of the step, not zero and not garbage -- the yardstick of the fp32 GPU cases."""
    case = sc.qp_case("2x1_fp32", 20)
    prob, x0 = case.problem(0), case.X0[0]
    z0 = case.start(0)
    dz, _, cond, _ = kkt.newton_step(prob, z0, x0, np.zeros(20 * 2), sc.REG)
    d32, _ = kkt.riccati_step(prob, z0, x0, np.zeros(20 * 2), sc.REG, np.float32)
    e = np.abs(d32 - dz).max()
    assert 0.0 < e <= np.finfo(np.float32).eps * cond * np.abs(dz).max()


@pytest.mark.parametrize("name", list(sc.BOUNDED_ROWS))
def test_qp_solution_satisfies_the_kkt_conditions(name):
    """Bounded convex QP: feasibility, stationarity with the bound multipliers, complementarity, signs; several controls
    and at least one state (the box row's limit) end on their bounds; and SLSQP lands on the same point."""
    case, lb, ub, _ = sc.bounded_case(name)
    H, nx = case.H, case.nx
    box_active = 0
    for b in range(case.B):
        prob, x0 = case.problem(b), case.X0[b]
        z, lam, nlo, nhi = kkt.qp_solution(prob, x0, lb, ub)
        assert np.abs(prob.constraints(z, x0)).max() < 1e-12
        assert (z >= lb).all() and (z <= ub).all()
        assert np.abs(prob.gradient(z) + prob.jacobian(z, x0).T @ lam - nlo + nhi).max() < 1e-10
        assert (nlo >= 0).all() and (nhi >= 0).all()
        assert np.abs(nlo * (z - lb)).max() == 0.0 and np.abs(nhi * (ub - z)).max() == 0.0
        act = (nlo > 0) | (nhi > 0)
        assert act[H * nx:].sum() >= 2
        box_active += int(act[:H * nx].sum())
        assert min(nlo[nlo > 0].min(initial=np.inf), nhi[nhi > 0].min(initial=np.inf)) >= 1e-3
        res = sc.slsqp(prob, x0, lb, ub)
        np.testing.assert_allclose(z, res.x, rtol=0, atol=1e-6)
    assert box_active >= 1


def test_global_memory_horizon_is_the_first_past_the_lds_budget():
    need, budget = sc.lds_bytes_2x1_thread(sc.H_GLOBAL)
    assert need > budget
    need, budget = sc.lds_bytes_2x1_thread(sc.H_GLOBAL - 1)
    assert need <= budget
