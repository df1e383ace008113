"""Shapes and data of the input-rate tests (nempc_bind_rate)  --  TEST INFRASTRUCTURE, not a test.

Shared by tests/test_rate_cpu.py (the references check themselves, and that the limit cases cannot pass vacuously) and
tests/test_gpu_rate.py.  Everything is seeded; references are computed once per case and cached.
"""
from __future__ import annotations

import functools

import numpy as np

import kkt_reference as kkt
import rate_reference as rr
import solver_step_cases as sc

# ---- (1) one Newton step on the rate QP: linear networks, no bounds, no limits
# name: (nx, nu, hidden, integrator, DT, horizons, lq kernels, dtype).  The solver plans over the AUGMENTED stage (nx + nu, nu):
# 3/1 for the 2/1 rows -- 3 (3 + 1) = 12 entries, the threshold at which "auto" takes the wave plan, so the thread plan is asked
# for by name --, 9/3 for 6/3.
QP_ROWS = {
    "2x1_discret": (2, 1, [32], "discret", 1.0, (1, 2, 6), ("thread", "wave", "auto"), "float64"),
    "6x3_rk4":     (6, 3, [16, 16], "rk4", 0.1, (4,), ("thread", "auto"), "float64"),
    "2x1_fp32":    (2, 1, [32], "discret", 1.0, (6,), ("thread", "wave"), "float32"),
}
QP_CASES = [(name, H) for name, row in QP_ROWS.items() for H in row[5]]
QP_BATCHES = (1, 3, 16)
QP_SEED = 1


def rate_data(case, seed):
    """S = 0.5 I + 0.05 N (not symmetric, symmetric part positive definite) and u_prev (B,nu) uniform in +-0.5, as the handle
    holds them."""
    rng = np.random.default_rng(seed + 400)
    S = sc._round(0.5 * np.eye(case.nu) + 0.05 * rng.normal(size=(case.nu, case.nu)), case.dtype)
    u_prev = sc._round(rng.uniform(-0.5, 0.5, size=(case.B, case.nu)), case.dtype)
    assert np.linalg.eigvalsh(S + S.T).min() > 0.5
    return S, u_prev


@functools.lru_cache(maxsize=None)
def qp_case(name, H):
    nx, nu, hidden, integ, DT, _, kernels, dtype = QP_ROWS[name]
    case = sc.Case(name, nx, nu, hidden, integ, DT, H, kernels, dtype, act="linear", seed=QP_SEED)
    case.S, case.u_prev = rate_data(case, QP_SEED)
    return case


def augmented_plan(case, kernel):
    """The LQ plan the size formula predicts for the augmented stage."""
    return sc.expected_lq_plan(case.nx + case.nu, case.nu, case.H, case.dtype, kernel)


@functools.lru_cache(maxsize=None)
def qp_reference(name, H):
    """Per problem: (z0, dz_ref, tolerance, e) -- the dense float64 step of the rate QP from the cold start, and the
    tolerance from the Riccati sweep over the augmented stages in the handle's precision (sc.step_tolerance)."""
    case = qp_case(name, H)
    out = []
    for b in range(case.B):
        prob, x0 = case.problem(b), case.X0[b]
        z0 = case.start(b)
        lam0 = np.zeros(H * case.nx)
        dz, _ = rr.newton_step(prob, z0, x0, lam0, sc.REG, case.S, case.u_prev[b])
        dzr = rr.riccati_step(prob, z0, x0, lam0, sc.REG, case.S, case.u_prev[b], sc.np_dtype(case))
        e = float(np.abs(dzr - dz).max())
        out.append((z0, dz, sc.step_tolerance(e, z0 + dz), e))
    return out


# ---- (2), (3), (5) the nonlinear network: 2/1, 2 x 64 tanh, H = 8
NL_H, NL_SEED = 8, 1


@functools.lru_cache(maxsize=None)
def nl_case(B):
    case = sc.Case("2x1_h8", 2, 1, [64, 64], "discret", 1.0, NL_H, ("auto",), "float64", act="tanh", seed=NL_SEED, B=B, scale_b=True)
    case.S, case.u_prev = rate_data(case, NL_SEED)
    return case


# ---- (4) limits: linear networks, bounds on u, limits on du
# name: (nx, nu, hidden, integrator, DT, H, seed)
LIMIT_ROWS = {
    "2x1_h8": (2, 1, [32], "discret", 1.0, 8, 1),
    "6x3_h4": (6, 3, [16, 16], "rk4", 0.1, 4, 1),
}
LIMIT_B = 4
NU_MIN = 1e-3            # smallest active multiplier the reference must show (strict complementarity with a margin)


@functools.lru_cache(maxsize=None)
def limit_case(name):
    """(case of LIMIT_B problems with .S / .u_prev, lb, ub (n), dlo, dhi (nu,)).  The control limit c is 40 % of the largest
    control of problem 0's unconstrained rate solution, the rate limit d 30 % of its largest move (the move against u_prev
    included); of a seeded pool of starts and previous controls the first LIMIT_B are kept whose REFERENCE solution has the
    limit on du_0 active, at least one control on a bound and no active multiplier under NU_MIN."""
    nx, nu, hidden, integ, DT, H, seed = LIMIT_ROWS[name]
    pool = sc.Case(name, nx, nu, hidden, integ, DT, H, ("auto",), "float64", act="linear", seed=seed, B=48)
    pool.S, pool.u_prev = rate_data(pool, seed)
    p0, x00 = pool.problem(0), pool.X0[0]
    dz, _ = rr.newton_step(p0, pool.start(0), x00, np.zeros(H * nx), 0.0, pool.S, pool.u_prev[0])
    zs = pool.start(0) + dz
    c = round(0.4 * float(np.abs(zs[H * nx:]).max()), 3)
    d = round(0.3 * float(np.abs(rr.moves(p0, zs, pool.u_prev[0])).max()), 3)
    lb = np.concatenate([np.full(H * nx, -sc.STATE_WIDE), np.full(H * nu, -c)])
    ub = -lb
    dlo, dhi = np.full(nu, -d), np.full(nu, d)
    keep = []
    for b in range(pool.B):
        # (u_prev inside the control bounds: a previous control the same actuator could have applied)
        pool.u_prev[b] = np.clip(pool.u_prev[b], -0.9 * c, 0.9 * c)
        try:
            z, lam, nlo, nhi, rlo, rhi = rr.qp_solution(pool.problem(b), pool.X0[b], lb, ub, pool.S, pool.u_prev[b], dlo, dhi)
        except (RuntimeError, AssertionError, np.linalg.LinAlgError):
            continue
        act = np.concatenate([v[v > 0] for v in (nlo, nhi, rlo, rhi)])
        if (rlo + rhi)[:nu].max() > 0 and ((nlo + nhi)[H * nx:] > 0).sum() >= 1 and act.min() >= NU_MIN:
            keep.append(b)
        if len(keep) == LIMIT_B:
            break
    assert len(keep) == LIMIT_B, keep
    case = sc.Case(name, nx, nu, hidden, integ, DT, H, ("auto",), "float64", act="linear", seed=seed, B=48)
    case.X0, case.B = pool.X0[keep].copy(), LIMIT_B
    case.S, case.u_prev = pool.S, pool.u_prev[keep].copy()
    return case, lb, ub, dlo, dhi


@functools.lru_cache(maxsize=None)
def limit_reference(name):
    case, lb, ub, dlo, dhi = limit_case(name)
    return [rr.qp_solution(case.problem(b), case.X0[b], lb, ub, case.S, case.u_prev[b], dlo, dhi) for b in range(case.B)]
