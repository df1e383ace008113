"""Dense float64 reference of the input-rate formulation (nempc_bind_rate)  --  TEST INFRASTRUCTURE, not a test.

Built on `oracle.nempc_oracle.Problem` and tests/kkt_reference.py, in the CALLER's variables z = [states (H,nx) ; controls
(H,nu)].  With D the block difference operator on the controls, du = D u - e_0 (x) u_prev, the problem is
    min f(z) + du' (I (x) S) du    s.t. defects = 0,  lb <= z <= ub,  dlo <= du <= dhi
so the Hessian gains D' (I (x) (S + S')) D on the control block and the gradient the matching linear term.  The solver runs
the problem stage-wise in s_t = [x_{t+1} ; u_t] with the move v_t = du_t as the stage control, and its Levenberg term sits on
v: eliminating v through the linear rows gives reg D'D on the control block here, not reg I.
"""
from __future__ import annotations

import warnings

import numpy as np

from oracle import nempc_oracle as orc
import kkt_reference as kkt


def diff_operator(H, nu):
    """D (H nu, H nu): (D u)_t = u_t - u_{t-1}, u_{-1} = 0."""
    D = np.eye(H * nu)
    for t in range(1, H):
        D[t * nu:(t + 1) * nu, (t - 1) * nu:t * nu] = -np.eye(nu)
    return D


def moves(prob, z, u_prev):
    """du (H,nu) of the point z."""
    U = np.asarray(z, dtype=np.float64)[prob.H * prob.nx:].reshape(prob.H, prob.nu)
    return np.diff(np.concatenate([np.asarray(u_prev, dtype=np.float64).reshape(1, prob.nu), U], axis=0), axis=0)


def rate_value(prob, z, S, u_prev):
    dv = moves(prob, z, u_prev)
    return float(np.einsum("ti,ij,tj->", dv, np.asarray(S, dtype=np.float64), dv))


def rate_gradient(prob, z, S, u_prev):
    """Gradient of rate_value with respect to z (zero on the states)."""
    S = np.asarray(S, dtype=np.float64)
    w = moves(prob, z, u_prev) @ (S + S.T).T          # (S + S') du_t per step
    gu = w.copy()
    gu[:-1] -= w[1:]                                   # D' w
    return np.concatenate([np.zeros(prob.H * prob.nx), gu.ravel()])


def rate_hessian(prob, S, reg=0.0):
    """(n,n): D' (I (x) (S + S' + reg I)) D on the control block."""
    H, nx, nu = prob.H, prob.nx, prob.nu
    S = np.asarray(S, dtype=np.float64)
    D = diff_operator(H, nu)
    Hr = np.zeros((prob.n, prob.n))
    Hr[H * nx:, H * nx:] = D.T @ np.kron(np.eye(H), S + S.T + reg * np.eye(nu)) @ D
    return Hr


def newton_step(prob, z, x0, lam, reg, S, u_prev):
    """One SQP step of the rate problem by a dense solve in the caller's variables: (dz, lam+)."""
    assert prob.box is None
    z = np.asarray(z, dtype=np.float64)
    n, m = prob.n, prob.H * prob.nx
    Hm = prob.lagrangian_hessian(z, x0, lam, 1.0) + rate_hessian(prob, S, reg)
    J = kkt._jac(prob, z, x0)
    K = np.zeros((n + m, n + m))
    K[:n, :n], K[:n, n:], K[n:, :n] = Hm, J.T, J
    rhs = -np.concatenate([prob.gradient(z) + rate_gradient(prob, z, S, u_prev), kkt._defects(prob, z, x0)])
    sol = np.linalg.solve(K, rhs)
    return sol[:n], sol[n:]


def augmented_stage_problem(prob, z, x0, lam, S, u_prev):
    """The LQ sub-problem over the augmented stages s = [x ; u] (ns = nx + nu), v = du, at the augmented point of z (u slots =
    z's controls, v = their differences: the linear rows hold).  Same keys as kkt.stage_problem."""
    H, nx, nu = prob.H, prob.nx, prob.nu
    ns = nx + nu
    sp = kkt.stage_problem(prob, z, x0, lam)
    S = np.asarray(S, dtype=np.float64)
    A = np.zeros((H, ns, ns)); B = np.zeros((H, ns, nu)); c = np.zeros((H, ns)); W = np.zeros((H, ns + nu, ns + nu))
    Qs = np.zeros((H, ns, ns)); gx = np.zeros((H, ns))
    col = np.concatenate([np.arange(nx + nu), nx + np.arange(nu)])      # column of (s, v) -> column of the handle's [x | u]
    for t in range(H):
        A[t, :nx, :nx], A[t, :nx, nx:] = sp["A"][t], sp["B"][t]
        A[t, nx:, nx:] = np.eye(nu)
        B[t, :nx], B[t, nx:] = sp["B"][t], np.eye(nu)
        c[t, :nx] = sp["c"][t]
        W[t] = sp["W"][t][np.ix_(col, col)]
        Qs[t, :nx, :nx], Qs[t, nx:, nx:] = sp["Qs"][t], sp["Rs"]
        gx[t, :nx], gx[t, nx:] = sp["gx"][t], sp["gu"][t]
    gu = moves(prob, z, u_prev) @ (S + S.T).T
    return dict(A=A, B=B, c=c, W=W, Qs=Qs, Rs=S + S.T, gx=gx, gu=gu, ns=ns)


def riccati_step(prob, z, x0, lam, reg, S, u_prev, dtype=np.float64):
    """dz (caller's variables) of the same Newton step by a Riccati sweep over the AUGMENTED stages carried out in `dtype`
    (the recursion of kkt.riccati_step)."""
    dtype = np.dtype(dtype).type
    sp = augmented_stage_problem(prob, z, x0, lam, S, u_prev)
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
        dv = ks[t] + Ks[t] @ ds
        ds = c[t] + A[t] @ ds + B[t] @ dv
        dz[t * nx:(t + 1) * nx] = ds[:nx]
        dz[H * nx + t * nu:H * nx + (t + 1) * nu] = ds[nx:]
    assert dz.dtype == dtype
    return dz.astype(np.float64)


def reduced_gradient(prob, z, x0, S=None, u_prev=None):
    """|Zn' (grad f + rate gradient)|inf with Zn an orthonormal null-space basis of the defect Jacobian at z (the basis of
    kkt.reduced_min_eig), and |defects|inf."""
    g = prob.gradient(z) + (0.0 if S is None else rate_gradient(prob, z, S, u_prev))
    J = kkt._jac(prob, z, x0)
    _, s, Vt = np.linalg.svd(J, full_matrices=True)
    rank = int((s > s.max() * 1e-13).sum())
    Zn = Vt[rank:].T
    return float(np.abs(Zn.T @ g).max()), float(np.abs(kkt._defects(prob, z, x0)).max())


def qp_solution(prob, x0, lb, ub, S, u_prev, dlo, dhi):
    """Linear networks only: kkt.qp_solution extended by the rate penalty and the linear inequality rows dlo <= du <= dhi
    (dlo, dhi (H,nu), +-inf = none).  SLSQP with those rows proposes the active set; one KKT solve with that set fixed gives
    the point; the multiplier signs and the inactive rows are verified.  Returns (z*, lam, nu_lo, nu_hi (n, bounds), r_lo,
    r_hi (H nu, rate limits)), multipliers >= 0 and zero off the active set."""
    from scipy.optimize import Bounds, LinearConstraint, minimize
    assert prob.box is None and all(a == "linear" for a in prob.net.act)
    H, nx, nu = prob.H, prob.nx, prob.nu
    n, m = prob.n, H * nx
    lb, ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    dlo, dhi = (np.broadcast_to(np.asarray(v, dtype=np.float64), (H, nu)).ravel() for v in (dlo, dhi))
    e0 = np.concatenate([np.asarray(u_prev, dtype=np.float64).ravel(), np.zeros((H - 1) * nu)])
    G = np.zeros((H * nu, n))
    G[:, m:] = diff_operator(H, nu)                        # du = G z - e0
    z00 = np.zeros(n)
    Hm = prob.objective_hessian() + rate_hessian(prob, S)
    c0 = prob.gradient(z00) + rate_gradient(prob, z00, S, u_prev)
    J, g0 = kkt._jac(prob, z00, x0), kkt._defects(prob, z00, x0)
    fun = lambda z: prob.objective(z) + rate_value(prob, z, S, u_prev)
    jac = lambda z: prob.gradient(z) + rate_gradient(prob, z, S, u_prev)
    zi = np.clip(orc.cold_start(x0, H, nu), lb, ub)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = minimize(fun, zi, method="SLSQP", jac=jac, bounds=Bounds(lb, ub),
                       constraints=[{"type": "eq", "fun": lambda z: kkt._defects(prob, z, x0), "jac": lambda z: kkt._jac(prob, z, x0)},
                                    LinearConstraint(G, dlo + e0, dhi + e0)],
                       options={"maxiter": 1000, "ftol": 1e-14})
    # every inequality as a row a.z <= h (sign -1: lower side)
    rows = np.concatenate([-np.eye(n), np.eye(n), -G, G])
    h = np.concatenate([-lb, ub, -(dlo + e0), dhi + e0])
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
        raise RuntimeError("rate qp_solution: the active set did not settle")
    full = np.zeros(rows.shape[0])
    full[idx] = mult
    nu_lo, nu_hi, r_lo, r_hi = full[:n], full[n:2 * n], full[2 * n:2 * n + H * nu], full[2 * n + H * nu:]
    assert (full >= 0.0).all() and (z >= lb - 1e-12).all() and (z <= ub + 1e-12).all()
    dv = G @ z - e0
    assert (dv >= dlo - 1e-12).all() and (dv <= dhi + 1e-12).all()
    return z, lam, nu_lo, nu_hi, r_lo, r_hi
