"""Dense float64 reference of the linear stage rows (nempc_bind_stage_rows)  --  TEST INFRASTRUCTURE, not a test.

Built on `oracle.nempc_oracle.Problem` and tests/kkt_reference.py, in the CALLER's variables z = [states (H,nx) ; controls
(H,nu)].  With C = [Cx (nc,nx) | Cu (nc,nu)] the rows are  rlo_t <= Cx x_t + Cu u_t <= rhi_t,  x_t / u_t row t of the state /
control block, i.e. rows = G z with G = row_matrix.  The solver runs the problem stage-wise in s_t = [x_t ; y_t], y_t the row
values, with the caller's u_t as the stage control: y costs nothing and feeds nothing, so the Newton step of a problem without
limits is the plain one (kkt.newton_step) and the Levenberg term stays reg I on the controls.
"""
from __future__ import annotations

import warnings

import numpy as np

from oracle import nempc_oracle as orc
import kkt_reference as kkt


def row_matrix(prob, C):
    """G (H nc, n): (G z)[t nc + k] = Cx[k] . x_t + Cu[k] . u_t."""
    H, nx, nu = prob.H, prob.nx, prob.nu
    C = np.asarray(C, dtype=np.float64)
    nc = C.shape[0]
    assert C.shape == (nc, nx + nu)
    G = np.zeros((H * nc, prob.n))
    for t in range(H):
        G[t * nc:(t + 1) * nc, t * nx:(t + 1) * nx] = C[:, :nx]
        G[t * nc:(t + 1) * nc, H * nx + t * nu:H * nx + (t + 1) * nu] = C[:, nx:]
    return G


def row_values(prob, z, C):
    """(H,nc) row values of the point z."""
    return (row_matrix(prob, C) @ np.asarray(z, dtype=np.float64)).reshape(prob.H, -1)


def row_tolerance(C, nx, tol_constraint):
    """(nc,) what a converged solve may exceed a limit by: tol_constraint (1 + |Cx row|_1) -- y is strictly inside its limits,
    |y - Cx Phi - Cu u| and |x - Phi| are below tol_constraint."""
    return tol_constraint * (1.0 + np.abs(np.asarray(C, dtype=np.float64)[:, :nx]).sum(axis=1))


def augmented_stage_problem(prob, z, x0, lam, C):
    """The LQ sub-problem over the augmented stages s = [x ; y] (ns = nx + nc) with the caller's u as the stage control, at the
    augmented point of z with y = the row values (what the solver's start is without limits): the y defects are then Cx times
    the network's.  Same keys as kkt.stage_problem."""
    H, nx, nu = prob.H, prob.nx, prob.nu
    C = np.asarray(C, dtype=np.float64)
    nc, Cx, Cu = C.shape[0], C[:, :nx], C[:, nx:]
    ns = nx + nc
    sp = kkt.stage_problem(prob, z, x0, lam)
    A = np.zeros((H, ns, ns)); B = np.zeros((H, ns, nu)); c = np.zeros((H, ns)); W = np.zeros((H, ns + nu, ns + nu))
    Qs = np.zeros((H, ns, ns)); gx = np.zeros((H, ns))
    col = np.concatenate([np.arange(nx), ns + np.arange(nu)])      # column of the handle's [x | u] -> column of (s, u)
    for t in range(H):
        A[t, :nx, :nx], A[t, nx:, :nx] = sp["A"][t], Cx @ sp["A"][t]
        B[t, :nx], B[t, nx:] = sp["B"][t], Cx @ sp["B"][t] + Cu
        c[t, :nx], c[t, nx:] = sp["c"][t], Cx @ sp["c"][t]
        W[t][np.ix_(col, col)] = sp["W"][t]
        Qs[t, :nx, :nx] = sp["Qs"][t]
        gx[t, :nx] = sp["gx"][t]
    return dict(A=A, B=B, c=c, W=W, Qs=Qs, Rs=sp["Rs"], gx=gx, gu=sp["gu"], ns=ns)


def riccati_step(prob, z, x0, lam, reg, C, dtype=np.float64):
    """dz (caller's variables) of the plain Newton step by a Riccati sweep over the AUGMENTED stages carried out in `dtype`
    (the recursion of kkt.riccati_step)."""
    dtype = np.dtype(dtype).type
    sp = augmented_stage_problem(prob, z, x0, lam, C)
    H, nx, nu, ns = prob.H, prob.nx, prob.nu, sp["ns"]
    A, B, c, W, Qs, Rs, gx, gu = (np.asarray(sp[k], dtype=dtype) for k in ("A", "B", "c", "W", "Qs", "Rs", "gx", "gu"))
    regI = (dtype(reg) * np.eye(nu)).astype(dtype)
    P, p = Qs[H - 1].copy(), gx[H - 1].copy()
    Ks, ks = [None] * H, [None] * H
    for t in range(H - 1, -1, -1):
        PA, PB, Pc = P @ A[t], P @ B[t], P @ c[t] + p
        Quu = Rs + W[t][ns:, ns:] + regI + B[t].T @ PB
        qu = gu[t] + B[t].T @ Pc
        Qux = W[t][ns:, :ns] + B[t].T @ PA
        L = np.linalg.cholesky(Quu)
        Ks[t] = -np.linalg.solve(L.T, np.linalg.solve(L, Qux)).astype(dtype)
        ks[t] = -np.linalg.solve(L.T, np.linalg.solve(L, qu)).astype(dtype)
        if t > 0:
            Pn = Qs[t - 1] + W[t][:ns, :ns] + A[t].T @ PA + Qux.T @ Ks[t]
            p = gx[t - 1] + A[t].T @ Pc + Qux.T @ ks[t]
            P = dtype(0.5) * (Pn + Pn.T)
    ds = np.zeros(ns, dtype=dtype)
    dz = np.zeros(prob.n, dtype=dtype)
    for t in range(H):
        du = ks[t] + Ks[t] @ ds
        ds = c[t] + A[t] @ ds + B[t] @ du
        dz[t * nx:(t + 1) * nx] = ds[:nx]
        dz[H * nx + t * nu:H * nx + (t + 1) * nu] = du
    assert dz.dtype == dtype
    return dz.astype(np.float64)


def qp_solution(prob, x0, lb, ub, C, rlo, rhi):
    """Linear networks only: kkt.qp_solution extended by the linear inequality rows rlo <= G z <= rhi (rlo, rhi (nc,) or (H,nc),
    +-inf = none) as a SciPy LinearConstraint.  SLSQP with those rows proposes the active set; one KKT solve with that set
    fixed gives the point; the multiplier signs and the inactive rows are verified.  Returns (z*, lam, nu_lo, nu_hi (n,
    bounds), r_lo, r_hi (H nc, rows)), multipliers >= 0 and zero off the active set."""
    from scipy.optimize import Bounds, LinearConstraint, minimize
    assert prob.box is None and all(a == "linear" for a in prob.net.act)
    H, nx = prob.H, prob.nx
    n, m = prob.n, H * nx
    G = row_matrix(prob, C)
    nc = G.shape[0] // H
    lb, ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    rlo, rhi = (np.broadcast_to(np.asarray(v, dtype=np.float64), (H, nc)).ravel() for v in (rlo, rhi))
    z00 = np.zeros(n)
    Hm, c0 = prob.objective_hessian(), prob.gradient(z00)
    J, g0 = kkt._jac(prob, z00, x0), kkt._defects(prob, z00, x0)
    zi = np.clip(orc.cold_start(x0, H, prob.nu), lb, ub)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = minimize(prob.objective, zi, method="SLSQP", jac=prob.gradient, bounds=Bounds(lb, ub),
                       constraints=[{"type": "eq", "fun": lambda z: kkt._defects(prob, z, x0), "jac": lambda z: kkt._jac(prob, z, x0)},
                                    LinearConstraint(G, rlo, rhi)],
                       options={"maxiter": 1000, "ftol": 1e-14})
    # every inequality as a row a.z <= h (sign -1: lower side)
    rows = np.concatenate([-np.eye(n), np.eye(n), -G, G])
    h = np.concatenate([-lb, ub, -rlo, rhi])
    fin = np.isfinite(h)
    act = fin & (rows @ res.x >= np.where(fin, h, 0.0) - 1e-7)
    for _ in range(30):
        Ga, ha = rows[act], h[act]
        na = int(act.sum())
        K = np.zeros((n + m + na, n + m + na))
        K[:n, :n] = Hm
        K[:n, n:n + m], K[n:n + m, :n] = J.T, J
        K[:n, n + m:], K[n + m:, :n] = Ga.T, Ga
        sol = np.linalg.solve(K, np.concatenate([-c0, -g0, ha]))
        z, lam, mult = sol[:n], sol[n:n + m], sol[n + m:]
        idx = np.flatnonzero(act)
        drop = idx[mult < 0.0]
        viol = fin & ~act & (rows @ z > np.where(fin, h, 0.0) + 1e-12)
        if drop.size == 0 and not viol.any():
            break
        act[drop] = False
        act |= viol
    else:
        raise RuntimeError("rows qp_solution: the active set did not settle")
    full = np.zeros(rows.shape[0])
    full[idx] = mult
    nu_lo, nu_hi, r_lo, r_hi = full[:n], full[n:2 * n], full[2 * n:2 * n + H * nc], full[2 * n + H * nc:]
    assert (full >= 0.0).all() and (z >= lb - 1e-12).all() and (z <= ub + 1e-12).all()
    rv = G @ z
    assert (rv >= rlo - 1e-12).all() and (rv <= rhi + 1e-12).all()
    return z, lam, nu_lo, nu_hi, r_lo, r_hi


def stationarity(prob, z, x0, C=None, rlo=None, rhi=None, lb=None, ub=None, act_tol=1e-6):
    """First-order optimality of the point z for the caller's problem, by the oracle: with A the defect Jacobian stacked with
    the ACTIVE rows and bounds (within act_tol of a limit; as rows a.z <= h),
      red    |Zn' grad f|inf over an orthonormal null-space basis Zn of A,
      defect |defects|inf,
      mult   the smallest least-squares multiplier of the active inequalities (grad f + A' [lam ; mult] ~ 0; +inf when none is
             active): a minimiser has mult >= 0,
      n_act  how many inequalities are active."""
    z = np.asarray(z, dtype=np.float64)
    n = prob.n
    g = prob.gradient(z)
    J = kkt._jac(prob, z, x0)
    ineq, h = [], []
    if lb is not None:
        ineq += [-np.eye(n), np.eye(n)]
        h += [-np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)]
    if C is not None:
        G = row_matrix(prob, C)
        nc = G.shape[0] // prob.H
        lo, hi = (np.broadcast_to(np.asarray(v, dtype=np.float64), (prob.H, nc)).ravel() for v in (rlo, rhi))
        ineq += [-G, G]
        h += [-lo, hi]
    if ineq:
        rows, h = np.concatenate(ineq), np.concatenate(h)
        fin = np.isfinite(h)
        act = fin & (rows @ z >= np.where(fin, h, 0.0) - act_tol)
        Aact = rows[act]
    else:
        Aact = np.zeros((0, n))
    A = np.concatenate([J, Aact])
    _, s, Vt = np.linalg.svd(A, full_matrices=True)
    rank = int((s > s.max() * 1e-13).sum())
    Zn = Vt[rank:].T
    mult = np.linalg.lstsq(A.T, -g, rcond=None)[0][J.shape[0]:]
    return dict(red=float(np.abs(Zn.T @ g).max()) if Zn.shape[1] else 0.0, defect=float(np.abs(kkt._defects(prob, z, x0)).max()),
                mult=float(mult.min()) if mult.size else np.inf, n_act=int(Aact.shape[0]))
