"""Per-problem, time-varying bounds of the bounded convex QPs  --  TEST INFRASTRUCTURE, not a test.

Shared by tests/test_bounds_cpu.py (the fixture checks itself) and tests/test_gpu_bounds.py (nempc_bind_bounds against the
exact active-set solutions).  The two small rows of solver_step_cases.BOUNDED_ROWS (ROWS below) keep their networks, objectives and starts
(solver_step_cases.bounded_case); what changes is where the limits come from: every problem gets a SCHEDULE of L = H + 3 rows
of its own, handed over through the binding alone -- no box rows, no host lb / ub:

    control limits of problem b, row t:   +- c s_b (1 + 0.25 sin(0.9 (t + b))),   s = (1.0, 0.8, 1.25, 0.6)
    upper limit of state 0:               cap + 0.05 b                            (every row)
    every other state limit:              +- STATE_WIDE

with c the case's control limit and cap its state cap.  A solve over the window that starts at row k of the schedule has
rows k .. k + H - 1 as its bounds; the references are kkt_reference.qp_solution with exactly those, at k = 0 and k = 3.
"""
from __future__ import annotations

import functools

import numpy as np

import kkt_reference as kkt
import solver_step_cases as sc

# The rows this construction serves: the two bounded rows of small stages.  The wide rows of BOUNDED_ROWS (20x4_h6,
# 40x10_h3) are not formed here: the schedule's moving control limits leave inactive controls so close to a limit in their
# references that the inactive bounds' pull on the last barrier sub-problem (inactive_pull, below) exceeds the end-point
# bound itself at the tests' MU_MIN -- 20x4_h6, offset 3, problem 3: 2.7e-6 against a bound of 4.3e-7 -- so condition C of
# tests/test_bounds_cpu.py fails on the reference alone, before any solver runs.  Their shared-bounds form is checked in
# tests/test_gpu_solver_steps.py and tests/test_gpu_duals.py.
ROWS = ("2x1_h12", "3x2_h7")
EXTRA_ROWS = 3
OFFSETS = (0, EXTRA_ROWS)
SCALES = (1.0, 0.8, 1.25, 0.6)
# The solver settings of the end-point tests.  The end-point bound below models two things: the distance mu_min / nu the last
# barrier sub-problem keeps from an ACTIVE bound, and the stopping test.  It leaves out the pull of the INACTIVE bounds: the
# barrier's gradient there, p_i = -mu_min / (z*_i - lo_i) + mu_min / (hi_i - z*_i), moves the minimiser of the last
# sub-problem, to first order, by the solution of the KKT system of the QP on its active set with -p on the right-hand
# side (inactive_pull).  A schedule that moves by one row per step puts some inactive control close to its limit: the
# smallest inactive gap of these 16 solutions is 1.4e-3 (3x2_h7, problem 2, offset 3), and at mu_min = 1e-9 -- the setting
# of test_interior_point_ends_at_the_solution_of_the_bounded_qp, whose fixture has no such gap -- that problem's central-path
# point lies 2.76e-7 from z*, 1.34 times the bound, before any solver error.  The bound's tenfold margin is meant for the
# solver: the tests use the largest decade of mu_min at which the pull stays under a quarter of the bound for every
# reference (asserted in tests/test_bounds_cpu.py): 1e-10, where it is at most 0.18 of it.
MU_MIN, TOL_STEP = 1e-10, 1e-8


def end_point_tolerance(nu_min, zs):
    """The bound of test_interior_point_ends_at_the_solution_of_the_bounded_qp: the distance the barrier's last sub-problem
    keeps from an active bound plus the stopping test, with a tenfold margin."""
    return 10.0 * (MU_MIN / nu_min + TOL_STEP * (1.0 + float(np.abs(zs).max())))


@functools.lru_cache(maxsize=None)
def schedule(name):
    """(case, dict(xlb, xub (B, L, nx), ulb, uub (B, L, nu)) float64 schedules of the BOUNDED_B problems)."""
    case, _, _, given = sc.bounded_case(name)
    H, nx, nu, B = case.H, case.nx, case.nu, case.B
    assert B == len(SCALES)
    L = H + EXTRA_ROWS
    c, cap = float(given["ub"][-1]), float(given["box_hi"][0])
    t = np.arange(L, dtype=np.float64)
    xlb = np.full((B, L, nx), -sc.STATE_WIDE)
    xub = np.full((B, L, nx), sc.STATE_WIDE)
    uub = np.empty((B, L, nu))
    for b in range(B):
        xub[b, :, 0] = cap + 0.05 * b
        uub[b] = (c * SCALES[b] * (1.0 + 0.25 * np.sin(0.9 * (t + b))))[:, None]
    return case, dict(xlb=xlb, xub=xub, ulb=-uub, uub=uub)


def window(name, b, offset):
    """(lb, ub) (n,) of problem b for the horizon that starts at row `offset` of its schedule, in z order."""
    case, s = schedule(name)
    rows = slice(offset, offset + case.H)
    return (np.concatenate([s["xlb"][b, rows].ravel(), s["ulb"][b, rows].ravel()]),
            np.concatenate([s["xub"][b, rows].ravel(), s["uub"][b, rows].ravel()]))


@functools.lru_cache(maxsize=None)
def reference(name, offset):
    """Per problem: (z*, lam, nu_lo, nu_hi) of kkt.qp_solution under that problem's own window."""
    case, _ = schedule(name)
    return [kkt.qp_solution(case.problem(b), case.X0[b], *window(name, b, offset)) for b in range(case.B)]


def inactive_pull(name, offset, b, mu=None):
    """|dz|inf the barrier terms of the INACTIVE bounds move the last sub-problem's minimiser by, to first order, at
    mu (default MU_MIN): the equality-constrained QP on the reference's active set with their gradient as linear term."""
    mu = MU_MIN if mu is None else mu
    case, _ = schedule(name)
    z, _, nlo, nhi = reference(name, offset)[b]
    lo, hi = window(name, b, offset)
    p = np.zeros_like(z)
    p[nlo == 0] -= mu / (z - lo)[nlo == 0]
    p[nhi == 0] += mu / (hi - z)[nhi == 0]
    prob = case.problem(b)
    Hm = prob.objective_hessian()
    C = np.vstack([prob.jacobian(z, case.X0[b])[:case.H * case.nx], np.eye(z.size)[(nlo > 0) | (nhi > 0)]])
    K = np.block([[0.5 * (Hm + Hm.T), C.T], [C, np.zeros((C.shape[0], C.shape[0]))]])
    sol = np.linalg.lstsq(K, np.concatenate([-p, np.zeros(C.shape[0])]), rcond=None)[0]
    return float(np.abs(sol[:z.size]).max())


def smallest_active_multiplier(ref_b):
    _, _, nlo, nhi = ref_b
    return float(np.concatenate([nlo[nlo > 0], nhi[nhi > 0]]).min())
