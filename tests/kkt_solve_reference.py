"""Float64 reference for KKT solves with caller-supplied right-hand sides  --  TEST INFRASTRUCTURE, not a test.

NumPy on stage data (`sensitivity_reference.stage_data` / `stage_data_from_tiles`).  At a primal-dual point with barrier
diagonal `sigma` (n; None = zeros) the symmetric KKT matrix K = [[W + diag(sigma), J'], [J, 0]] is solved for columns

    K [v ; w] = [rz ; rg],      rz (k, n) in z order, rg (k, H nx) in defect order (None = zeros)

`dense_solve` assembles K and calls np.linalg.solve; `affine_riccati` is the recursion the device kernel runs (the gain-only
backward sweep of `sensitivity_reference.riccati` plus its affine part); both also return the pull-back
gx0 = -(W_ux,0' v_u[0] + A_0' w_0) = -[v ; w]' d/dx0 [grad L ; g].  `vjp` turns one cotangent of z* into the cotangents of
x0, xref, uref, cx, cu.
"""
from __future__ import annotations

import numpy as np

import sensitivity_reference as sref


def kkt_matrix(stage, H, nx, nu, sigma=None):
    """K (n + H nx, n + H nx) from stage data, unknowns [x_0..x_{H-1} | u_0..u_{H-1} | w_0..w_{H-1}]."""
    A, B, W, Qs, Rs = (np.asarray(stage[k], dtype=np.float64) for k in ("A", "B", "W", "Qs", "Rs"))
    n, m = H * (nx + nu), H * nx
    K = np.zeros((n + m, n + m))
    for t in range(H):
        xs, us, ls = slice(t * nx, (t + 1) * nx), slice(m + t * nu, m + (t + 1) * nu), slice(n + t * nx, n + (t + 1) * nx)
        K[xs, xs] = Qs[t] + (W[t + 1][:nx, :nx] if t + 1 < H else 0.0)
        K[us, us] = Rs + W[t][nx:, nx:]
        K[ls, xs] = -np.eye(nx)
        K[ls, us] = B[t]
        if t > 0:
            xp = slice((t - 1) * nx, t * nx)
            K[us, xp] = W[t][nx:, :nx]
            K[xp, us] = W[t][nx:, :nx].T
            K[ls, xp] = A[t]
    K[:n, n:] = K[n:, :n].T
    if sigma is not None:
        K[np.arange(n), np.arange(n)] += np.asarray(sigma, dtype=np.float64)
    return K


def _pull_back(stage, H, nx, nu, v, w):
    W0, A0 = np.asarray(stage["W"][0], dtype=np.float64), np.asarray(stage["A"][0], dtype=np.float64)
    return -(v[:, H * nx:H * nx + nu] @ W0[nx:, :nx] + w[:, :nx] @ A0)


def _rhs(H, nx, nu, rz, rg):
    rz = np.atleast_2d(np.asarray(rz, dtype=np.float64))
    rg = np.zeros((rz.shape[0], H * nx)) if rg is None else np.atleast_2d(np.asarray(rg, dtype=np.float64))
    assert rz.shape[1] == H * (nx + nu) and rg.shape == (rz.shape[0], H * nx)
    return rz, rg


def dense_solve(stage, H, nx, nu, sigma, rz, rg=None):
    """dict(v (k,n), w (k,H nx), gx0 (k,nx)) by one dense solve."""
    rz, rg = _rhs(H, nx, nu, rz, rg)
    n = H * (nx + nu)
    sol = np.linalg.solve(kkt_matrix(stage, H, nx, nu, sigma), np.concatenate([rz, rg], axis=1).T).T
    v, w = sol[:, :n], sol[:, n:]
    return dict(v=v, w=w, gx0=_pull_back(stage, H, nx, nu, v, w))


def affine_riccati(stage, H, nx, nu, sigma, rz, rg=None):
    """The device kernel's recursion.  dict(v, w, gx0, pd, margin): pd / margin as `sensitivity_reference.riccati`; v, w, gx0
    are NaN when not pd."""
    rz, rg = _rhs(H, nx, nu, rz, rg)
    k, n, hx = rz.shape[0], H * (nx + nu), H * nx
    A, B, W, Qs, Rs = (np.asarray(stage[key], dtype=np.float64) for key in ("A", "B", "W", "Qs", "Rs"))
    sg = np.zeros(n) if sigma is None else np.asarray(sigma, dtype=np.float64)
    sx, su = sg[:hx].reshape(H, nx), sg[hx:].reshape(H, nu)
    rx, ru, rgs = rz[:, :hx].reshape(k, H, nx), rz[:, hx:].reshape(k, H, nu), rg.reshape(k, H, nx)
    nan = dict(v=np.full((k, n), np.nan), w=np.full((k, hx), np.nan), gx0=np.full((k, nx), np.nan))
    P = Qs[H - 1] + np.diag(sx[H - 1])
    p = rx[:, H - 1].copy()
    Ks, Ps, ps, ks, margin = [None] * H, [None] * H, [None] * H, [None] * H, np.inf
    for t in range(H - 1, -1, -1):
        Ps[t], ps[t] = P, p
        PA, PB = P @ A[t], P @ B[t]
        Quu = Rs + np.diag(su[t]) + W[t][nx:, nx:] + B[t].T @ PB
        Qux = W[t][nx:, :nx] + B[t].T @ PA
        piv, fac = sref._pivots(Quu)
        margin = min(margin, float(np.abs(piv).min() / np.abs(Quu).max()))
        if fac is None:
            return dict(nan, pd=False, margin=margin)
        Lf, d = fac
        solve = lambda Y: np.linalg.solve(Lf.T, np.linalg.solve(Lf, Y) / d[:, None])
        Ks[t] = -solve(Qux)
        q = rgs[:, t] @ P.T + p
        ks[t] = solve((ru[:, t] + q @ B[t]).T).T
        if t > 0:
            p = rx[:, t - 1] + q @ A[t] - ks[t] @ Qux
            Pn = Qs[t - 1] + np.diag(sx[t - 1]) + W[t][:nx, :nx] + A[t].T @ PA + Qux.T @ Ks[t]
            P = 0.5 * (Pn + Pn.T)
    vx = np.zeros((k, nx))
    v, w = np.zeros((k, n)), np.zeros((k, hx))
    for t in range(H):
        vu = vx @ Ks[t].T + ks[t]
        vx = vx @ A[t].T + vu @ B[t].T - rgs[:, t]
        v[:, t * nx:(t + 1) * nx], v[:, hx + t * nu:hx + (t + 1) * nu] = vx, vu
        w[:, t * nx:(t + 1) * nx] = vx @ Ps[t].T - ps[t]
    return dict(v=v, w=w, gx0=_pull_back(stage, H, nx, nu, v, w), pd=True, margin=margin)


def param_grads(v, gx0, Qs, Rs, H, nx, nu):
    """Cotangents of (x0, xref, uref, cx, cu) from v = K^-1 [zbar ; 0] and its pull-back; v (..., n), gx0 (..., nx);
    Qs (H,nx,nx) the symmetrised state weights per stage, Rs (nu,nu)."""
    vx = v[..., :H * nx].reshape(v.shape[:-1] + (H, nx))
    vu = v[..., H * nx:].reshape(v.shape[:-1] + (H, nu))
    return dict(X0=gx0, xref=np.einsum("tij,...tj->...ti", Qs, vx), uref=vu @ np.asarray(Rs).T, cx=-vx, cu=-vu)


def vjp(prob, z, x0, lam, sigma, zbar):
    """Cotangents dict(X0 (nx), xref (H,nx), uref (H,nu), cx (H,nx), cu (H,nu)) of the solution map at the primal-dual point
    (z, lam) of `prob` for the cotangent zbar (n) of z*, by the dense solve on the oracle's own stage data."""
    stage = sref.stage_data(prob, z, x0, lam)
    H, nx, nu = prob.H, prob.nx, prob.nu
    s = dense_solve(stage, H, nx, nu, sigma, zbar)
    return param_grads(s["v"][0], s["gx0"][0], stage["Qs"], stage["Rs"], H, nx, nu)
