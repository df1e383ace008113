"""Shapes and data of the linear-stage-row tests (nempc_bind_stage_rows)  --  TEST INFRASTRUCTURE, not a test.

Shared by tests/test_stage_rows_cpu.py (the references check themselves, and that the limit cases cannot pass vacuously) and
tests/test_gpu_stage_rows.py.  Everything is seeded; references are computed once per case and cached.
"""
from __future__ import annotations

import functools

import numpy as np

import kkt_reference as kkt
import rows_reference as wr
import solver_step_cases as sc

# ---- (1) a binding with nothing in effect: linear networks, no bounds, rows with infinite limits
# name: (nx, nu, nc, hidden, integrator, DT, horizons, lq kernels, dtype).  The solver plans over the AUGMENTED stage (nx + nc, nu):
# 3/1 for the 2/1 rows -- 3 (3 + 1) = 12 entries, the threshold at which "auto" takes the wave plan, so the thread plan is asked
# for by name --, 8/3 for 6/3.
QP_ROWS = {
    "2x1_discret": (2, 1, 1, [32], "discret", 1.0, (1, 2, 6), ("thread", "wave", "auto"), "float64"),
    "6x3_rk4":     (6, 3, 2, [16, 16], "rk4", 0.1, (4,), ("thread", "auto"), "float64"),
    "2x1_fp32":    (2, 1, 1, [32], "discret", 1.0, (6,), ("thread", "wave"), "float32"),
}
QP_CASES = [(name, H) for name, row in QP_ROWS.items() for H in row[6]]
QP_BATCHES = (1, 3, 16)
QP_SEED = 1


def row_data(case, nc, seed):
    """C (nc, nx+nu): mixed rows, entries standard normal, as the handle holds them."""
    rng = np.random.default_rng(seed + 500)
    return sc._round(rng.normal(size=(nc, case.nx + case.nu)), case.dtype)


@functools.lru_cache(maxsize=None)
def qp_case(name, H):
    nx, nu, nc, hidden, integ, DT, _, kernels, dtype = QP_ROWS[name]
    case = sc.Case(name, nx, nu, hidden, integ, DT, H, kernels, dtype, act="linear", seed=QP_SEED)
    case.nc, case.C = nc, row_data(case, nc, QP_SEED)
    return case


def augmented_plan(case, kernel):
    """The LQ plan the size formula predicts for the augmented stage."""
    return sc.expected_lq_plan(case.nx + case.nc, case.nu, case.H, case.dtype, kernel)


@functools.lru_cache(maxsize=None)
def qp_reference(name, H):
    """Per problem: (z0, dz_ref, tolerance, e) -- the dense float64 step of the PLAIN QP from the cold start (rows without
    limits change nothing), and the tolerance from the Riccati sweep over the augmented stages in the handle's precision
    (sc.step_tolerance)."""
    case = qp_case(name, H)
    out = []
    for b in range(case.B):
        prob, x0 = case.problem(b), case.X0[b]
        z0 = case.start(b)
        lam0 = np.zeros(H * case.nx)
        dz = kkt.newton_step(prob, z0, x0, lam0, sc.REG, diagnostics=False)[0]
        dzr = wr.riccati_step(prob, z0, x0, lam0, sc.REG, case.C, sc.np_dtype(case))
        e = float(np.abs(dzr - dz).max())
        out.append((z0, dz, sc.step_tolerance(e, z0 + dz), e))
    return out


# ---- (3), (4), (6) the nonlinear network: 2/1, 2 x 64 tanh, H = 8;  (5) the same with two controls
NL_H, NL_SEED = 8, 1


@functools.lru_cache(maxsize=None)
def nl_case(B, nu=1, x0_range=0.5):
    return sc.Case(f"2x{nu}_h8", 2, nu, [64, 64], "discret", 1.0, NL_H, ("auto",), "float64", act="tanh", seed=NL_SEED, B=B, scale_b=True,
                   x0_range=x0_range)


# ---- (2) limits: linear networks, bounds on u, limits on the rows
# name: (nx, nu, hidden, integrator, DT, H, seed, C rows as (state part, control part), per_stage)
LIMIT_ROWS = {
    "2x1_h8": (2, 1, [32], "discret", 1.0, 8, 1, "mixed", 0),
    "6x3_h4": (6, 3, [16, 16], "rk4", 0.1, 4, 1, "state+mixed", 1),
}
LIMIT_B = 4
LIMIT_FRACTION = 0.4     # limits as a fraction of what the unconstrained solution reaches
NU_MIN = 1e-3            # smallest active multiplier the reference must show (strict complementarity with a margin)


def _limit_rows(kind, nx, nu, seed):
    rng = np.random.default_rng(seed + 600)
    mixed = rng.normal(size=(1, nx + nu))
    if kind == "mixed":
        return mixed
    state = np.concatenate([rng.normal(size=(1, nx)), np.zeros((1, nu))], axis=1)       # state-only: Cu = 0
    return np.concatenate([state, mixed])


def unconstrained(prob, z0, x0):
    """The solution without bounds and without rows (linear networks: one Newton step, reg = 0)."""
    return z0 + kkt.newton_step(prob, z0, x0, np.zeros(prob.H * prob.nx), 0.0, diagnostics=False)[0]


@functools.lru_cache(maxsize=None)
def limit_case(name):
    """(case of LIMIT_B problems with .C, lb, ub (n), rlo, rhi ((nc,), or (H,nc) for the per_stage row)).  The control limit c
    is LIMIT_FRACTION of the largest control of problem 0's unconstrained solution, the limit of row k LIMIT_FRACTION of the
    largest |value| that row reaches there (per_stage: widened by 5 % per step, so every step has its own number); of a seeded
    pool of 48 starts the first LIMIT_B are kept whose REFERENCE solution has at least one row active, at least one control
    on a bound and no active multiplier under NU_MIN."""
    nx, nu, hidden, integ, DT, H, seed, kind, per_stage = LIMIT_ROWS[name]
    pool = sc.Case(name, nx, nu, hidden, integ, DT, H, ("auto",), "float64", act="linear", seed=seed, B=48)
    C = _limit_rows(kind, nx, nu, seed)
    p0 = pool.problem(0)
    zs = unconstrained(p0, pool.start(0), pool.X0[0])
    c = round(LIMIT_FRACTION * float(np.abs(zs[H * nx:]).max()), 3)
    L = np.round(LIMIT_FRACTION * np.abs(wr.row_values(p0, zs, C)).max(axis=0), 3)
    lb = np.concatenate([np.full(H * nx, -sc.STATE_WIDE), np.full(H * nu, -c)])
    ub = -lb
    rhi = L * (1.0 + 0.05 * np.arange(H))[:, None] if per_stage else L
    rlo = -rhi
    keep = []
    for b in range(pool.B):
        try:
            z, lam, nlo, nhi, qlo, qhi = wr.qp_solution(pool.problem(b), pool.X0[b], lb, ub, C, rlo, rhi)
        except (RuntimeError, AssertionError, np.linalg.LinAlgError):
            continue
        act = np.concatenate([v[v > 0] for v in (nlo, nhi, qlo, qhi)])
        if ((qlo + qhi) > 0).sum() >= 1 and ((nlo + nhi)[H * nx:] > 0).sum() >= 1 and act.min() >= NU_MIN:
            keep.append(b)
        if len(keep) == LIMIT_B:
            break
    assert len(keep) == LIMIT_B, keep
    case = sc.Case(name, nx, nu, hidden, integ, DT, H, ("auto",), "float64", act="linear", seed=seed, B=48)
    case.X0, case.B = pool.X0[keep].copy(), LIMIT_B
    case.C, case.nc = C, C.shape[0]
    return case, lb, ub, rlo, rhi


@functools.lru_cache(maxsize=None)
def limit_reference(name):
    case, lb, ub, rlo, rhi = limit_case(name)
    return [wr.qp_solution(case.problem(b), case.X0[b], lb, ub, case.C, rlo, rhi) for b in range(case.B)]
