"""The dense KKT reference of the per-step solver checks (tests/kkt_reference.py) checks itself: no GPU.

The GPU tests in tests/test_gpu_solver_steps.py hold the solver's steps against `newton_step` / `replay` / `qp_solution`
to a tolerance derived from `riccati_step`; here those four agree with each other, with the KKT conditions and with SciPy
SLSQP on the oracle's callbacks, on the very shapes the GPU tests use.  The size formula that predicts the solver's LQ plan
(solver_step_cases.lds_bytes) is held against the figures the wide rows were chosen by, and the recursion of the
second-order correction (csrc/solver_soc_impl.h) passes a sanitized stand-alone host program."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

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


@pytest.mark.parametrize("name", list(sc.NL_ROWS))
def test_every_nonlinear_problem_is_compared_at_the_first_two_steps(name):
    """A problem leaves the GPU comparison once a reference step is below STOP_STEP (the solver rightly stands still there).
    On every row that happens at the third step at the earliest: every problem is compared after one and after two steps."""
    for rp, _ in sc.nl_reference(name):
        assert all(np.abs(st["dz"]).max() >= sc.STOP_STEP for st in rp[:2]), [float(np.abs(st["dz"]).max()) for st in rp]
    steps = sc.NL_ROWS[name][8]
    if steps >= 3:      # ... and at the third step at least 5 of the 8, except where NL_STEP3_COMPARED says how many
        left = sum(all(np.abs(st["dz"]).max() >= sc.STOP_STEP for st in rp[:3]) for rp, _ in sc.nl_reference(name))
        assert left >= 5 if name not in sc.NL_STEP3_COMPARED else left == sc.NL_STEP3_COMPARED[name], left


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
    assert sc.lds_bytes_2x1_thread(20) == sc.lds_bytes(2, 1, 20, "float64", 1) == (8 * (48 * 20 + 37), 150 * 1024 - 48 * 20)


# fp64 (fp32 where the row is) KB per problem at one damping level, as the wide rows were chosen
WIDE_KB = {("12x5_discret", 4): 33, ("16x4_rk4", 4): 48, ("20x4_discret", 6): 98, ("33x3_unity", 3): 127, ("40x10_discret", 3): 221,
           ("40x10_fp32", 3): 111, ("64x8_fp32", 1): 119}


def test_wide_rows_land_on_every_lq_plan():
    """lds_bytes restates plan_lq's count (csrc/solver.hip).  The wide QP rows' working sets are the sizes they were chosen by,
    20x4 needs more dynamic LDS than the 64 KiB a kernel gets by default, and over the rows with more matrix entries than
    lanes (nx nx > 64) the requested kernels reach thread-from-global-memory, thread-in-LDS and wave-in-LDS; a wave kernel
    requested for a working set over the budget would be the thread kernel from global memory."""
    for (name, H), kb in WIDE_KB.items():
        nx, nu, _, _, _, _, _, dtype = sc.QP_ROWS[name][:8]
        assert round(sc.lds_bytes(nx, nu, H, dtype)[0] / 1000) == kb, (name, sc.lds_bytes(nx, nu, H, dtype))
    need, budget = sc.lds_bytes(20, 4, 6)
    assert 64 * 1024 < need <= budget < 2 * need          # one problem per workgroup
    plans = set()
    for name, H in sc.QP_CASES:
        nx, nu, _, _, _, _, kernels, dtype = sc.QP_ROWS[name][:8]
        if nx * nx > 64:
            plans.update(sc.expected_lq_plan(nx, nu, H, dtype, k) for k in kernels)
    assert plans == {"thread_global", "thread_lds", "wave_lds"}
    assert sc.expected_lq_plan(40, 10, 3, "float64", "wave") == "thread_global"
    assert sc.expected_lq_plan(40, 10, 3, "float32", "wave") == "wave_lds"
    assert sc.expected_lq_plan(2, 1, 63, "float64", "auto") == "scan" and sc.expected_lq_plan(2, 1, 64, "float64", "auto") == "thread_lds"
    assert sc.expected_lq_plan(6, 3, 8, "float64", "auto") == "wave_lds" and sc.expected_lq_plan(3, 2, 7, "float64", "auto") == "wave_lds"
    assert sc.expected_lq_plan(2, 1, sc.H_GLOBAL, "float64", "thread") == "thread_global"


def test_second_order_correction_passes_the_sanitized_host_program(tmp_path):
    """tests/soc_check.cpp: the host / device recursion of csrc/solver_soc_impl.h with one lane and with 64 simulated lanes
    (threads, `sync` a barrier), compiled for the host with AddressSanitizer and UndefinedBehaviorSanitizer and run on its
    own, against a dense forward substitution in long double: nx in {1, 3, 63, 64, 65, 130} x nu in {1, 4} x H in {1, 2, 5}
    x {double, float}, every array at its exact size; bound 64 u (1 + |dx|inf) H (observed: 0.04 of it); every output
    element written, controls copied, 64 lanes == 1 lane bit for bit."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "soc_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(REPO, "pyneuralempc_amd", "csrc"), "-o", exe, os.path.join(REPO, "tests", "soc_check.cpp")]
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-400:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    m = re.search(r"(\d+) cases, (\d+) entries checked, 0 failures", r.stdout)
    assert m and int(m.group(1)) == 144 and int(m.group(2)) > 20000, r.stdout


@pytest.mark.parametrize("name", list(sc.SOC_ROWS))
def test_the_correction_cases_reject_the_full_step_and_keep_their_candidates_apart(name):
    """What the candidate-set test of tests/test_gpu_solver_steps.py stands on, from the reference alone: the starts are
    feasible, no damping restart (reduced Hessian eigenvalue >= 0.05), the full step RAISES the l1 merit for at least half
    of the problems while the corrected point lowers it for at least one of those, the corrected point has smaller defects
    than the full step, and any two candidates of a problem are more than a thousand tolerances apart."""
    case = sc.soc_case(name)
    ref = sc.soc_reference(name)
    assert sum(r["raises"] for r in ref) >= case.B / 2
    helped = 0
    for b, r in enumerate(ref):
        prob, x0 = case.problem(b), case.X0[b]
        hx = case.H * case.nx
        assert np.abs(prob.constraints(r["z0"], x0)[:hx]).max() <= 1e-13 * (1.0 + np.abs(r["z0"]).max())
        assert r["eig"] >= sc.GATE_EIG
        pts = dict(r["cands"])
        g_full, g_corr = (np.abs(prob.constraints(pts[k], x0)[:hx]).sum() for k in ("full", "corrected"))
        assert g_corr < g_full, (b, g_corr, g_full)
        helped += r["raises"] and kkt.l1_merit(prob, pts["corrected"], x0, r["pen"]) < kkt.l1_merit(prob, r["z0"], x0, r["pen"])
        P = np.stack([p for _, p in r["cands"]])
        d = np.abs(P[:, None, :] - P[None, :, :]).max(axis=2) + np.eye(len(P)) * 1e300
        assert d.min() > 1e3 * r["tol"], (b, d.min(), r["tol"])
    assert helped >= 1
