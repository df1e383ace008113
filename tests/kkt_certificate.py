"""KKT residuals of a primal-dual point in NumPy float64  --  TEST INFRASTRUCTURE, not a test.

Built on `oracle.nempc_oracle.Problem` (dense jacobian, gradient, constraints) and tests/kkt_reference.py.  Conventions are
theirs and the library's (include/nempc.h, nempc_solve_duals / nempc_kkt_residual):

    g = Phi - x,   L = f + lam.g - zl.(z - lb) + zu.(z - ub),   zl, zu >= 0
    s    = grad f + J' lam - zl + zu                       (lam (m): defect rows, then the box rows of a Problem with box)
    r[0] = |s|inf                                                            stationarity
    r[1] = max(|defects|inf, max_i (lb_i - z_i)+, max_i (z_i - ub_i)+)       primal feasibility
    r[2] = max over FINITE bounds of |zl_i (z_i - lb_i)|, |zu_i (ub_i - z_i)| complementarity
    r[3] = max(0, max_i -zl_i, max_i -zu_i)                                  dual feasibility

Entries of zl / zu on an infinite bound count as zero everywhere.  A Problem with box rows has its limits intersected with
lb / ub on the state variables (they are bounds for the solver), exactly as the library does.
"""
from __future__ import annotations

import numpy as np

import kkt_reference as kkt


def effective_bounds(prob, lb, ub):
    """lb / ub (n) or None, intersected with the Problem's box rows on the state variables; +-inf for a missing bound."""
    n, hx = prob.n, prob.H * prob.nx
    lo = np.full(n, -np.inf) if lb is None else np.array(np.broadcast_to(np.asarray(lb, dtype=np.float64), (n,)))
    hi = np.full(n, np.inf) if ub is None else np.array(np.broadcast_to(np.asarray(ub, dtype=np.float64), (n,)))
    if prob.box is not None:
        lo[:hx] = np.maximum(lo[:hx], np.tile(prob.box[0], prob.H))
        hi[:hx] = np.minimum(hi[:hx], np.tile(prob.box[1], prob.H))
    return lo, hi


def residuals(prob, z, x0, lam, zl=None, zu=None, lb=None, ub=None):
    """(r (4,), s (n,)) by the formulas of the module docstring, from the oracle's dense callbacks."""
    z = np.asarray(z, dtype=np.float64)
    n, hx = prob.n, prob.H * prob.nx
    lam = np.asarray(lam, dtype=np.float64)
    assert lam.shape == (prob.m,), (lam.shape, prob.m)
    lo, hi = effective_bounds(prob, lb, ub)
    flo, fhi = np.isfinite(lo), np.isfinite(hi)
    vl = np.where(flo, 0.0 if zl is None else np.asarray(zl, dtype=np.float64), 0.0)
    vu = np.where(fhi, 0.0 if zu is None else np.asarray(zu, dtype=np.float64), 0.0)
    s = prob.gradient(z) + prob.jacobian(z, x0).T @ lam - vl + vu
    dl = np.where(flo, z - np.where(flo, lo, 0.0), np.inf)
    du = np.where(fhi, np.where(fhi, hi, 0.0) - z, np.inf)
    defect = prob.constraints(z, x0)[:hx]
    r = np.zeros(4)
    r[0] = np.abs(s).max()
    r[1] = max(np.abs(defect).max(), np.maximum(-dl, 0.0).max(), np.maximum(-du, 0.0).max())
    r[2] = max(np.abs(vl[flo] * dl[flo]).max(initial=0.0), np.abs(vu[fhi] * du[fhi]).max(initial=0.0))
    r[3] = max(0.0, (-vl).max(), (-vu).max())
    return r, s


def lam_sweep_error(prob, x0, z0, steps, reg, dtype):
    """The analogue of kkt_reference.sweep_error for the multipliers: what a correct sweep in `dtype` loses on lam+ over
    the systems of a replay -- sum over the replayed steps (each taken at the float64 reference iterate and multipliers) of
    |riccati_step(dtype) lam+ - newton_step(float64) lam+|inf, cumulative per step."""
    acc, out = 0.0, []
    for st in kkt.replay(prob, x0, z0, steps, reg):
        _, lamn = kkt.riccati_step(prob, st["z_before"], x0, st["lam_before"], reg, dtype)
        acc += float(np.abs(lamn - st["lam"]).max())
        out.append(acc)
    return out


def lam_tolerance(e, lam_ref, factor=10.0):
    """`factor` times what a correct sweep in the handle's precision loses, floored at 1e-12 (1 + |lam_ref|inf)."""
    return max(factor * e, 1e-12 * (1.0 + float(np.abs(lam_ref).max())))
