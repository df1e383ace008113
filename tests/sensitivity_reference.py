"""Float64 reference for the solution sensitivities dz*/dx0  --  TEST INFRASTRUCTURE, not a test.

NumPy on `oracle.nempc_oracle.Problem` and `kkt_reference.stage_problem` (plain models, defect rows only: box rows are
bounds).  At a primal-dual point (z, lam) with barrier diagonal `sigma` (n; None = zeros) the sensitivities solve

    [[W + diag(sigma), J'], [J, 0]] [S ; dlam] = -d/dx0 [grad f + J' lam ; g]

where only stage 0 carries a right-hand side: A_0 in its defect rows and the (u, x) part of Lagrangian block 0 in the rows
of u_0.  `dense` solves that system, `dense_fd_rhs` forms its right-hand side by central differences instead (independent
of the stage form), `riccati` is the gain-only backward sweep and closed-loop propagation the device kernel runs.
"""
from __future__ import annotations

import numpy as np

import kkt_reference as kkt


def _kkt_matrix(prob, z, x0, lam, sigma):
    n, m = prob.n, prob.H * prob.nx
    Hm = prob.lagrangian_hessian(z, x0, lam, 1.0)
    if sigma is not None:
        Hm = Hm + np.diag(np.asarray(sigma, dtype=np.float64))
    J = prob.jacobian(z, x0)[:m]
    K = np.zeros((n + m, n + m))
    K[:n, :n] = Hm
    K[:n, n:] = J.T
    K[n:, :n] = J
    return K


def _analytic_rhs(prob, z, x0, lam):
    n, m, nx, nu, H = prob.n, prob.H * prob.nx, prob.nx, prob.nu, prob.H
    sp = kkt.stage_problem(prob, z, x0, lam)
    R = np.zeros((n + m, nx))
    R[H * nx:H * nx + nu] = sp["W"][0][nx:, :nx]
    R[n:n + nx] = sp["A"][0][:nx, :nx]
    return R


def dense(prob, z, x0, lam, sigma=None):
    """(S (n,nx), dlam (H nx,nx)) by one dense solve with the analytic stage-0 right-hand side."""
    assert prob.box is None and prob.window == 1
    z = np.asarray(z, dtype=np.float64)
    sol = np.linalg.solve(_kkt_matrix(prob, z, x0, lam, sigma), -_analytic_rhs(prob, z, x0, lam))
    return sol[:prob.n], sol[prob.n:]


def dense_fd_rhs(prob, z, x0, lam, sigma=None, h=1e-6):
    """The same solve with the right-hand side by central differences of [grad f + J' lam ; defects] over x0."""
    assert prob.box is None and prob.window == 1
    z = np.asarray(z, dtype=np.float64)
    n, m, nx = prob.n, prob.H * prob.nx, prob.nx

    def F(x):
        return np.concatenate([prob.gradient(z) + prob.jacobian(z, x)[:m].T @ lam, prob.constraints(z, x)[:m]])

    R = np.zeros((n + m, nx))
    for j in range(nx):
        e = np.zeros(nx)
        e[j] = h
        R[:, j] = (F(x0 + e) - F(x0 - e)) / (2.0 * h)
    sol = np.linalg.solve(_kkt_matrix(prob, z, x0, lam, sigma), -R)
    return sol[:n], sol[n:]


def stage_data(prob, z, x0, lam):
    """A, B, W, Qs, Rs of the stage form (kkt_reference.stage_problem)."""
    sp = kkt.stage_problem(prob, np.asarray(z, dtype=np.float64), x0, lam)
    return {k: sp[k] for k in ("A", "B", "W", "Qs", "Rs")}


def stage_data_from_tiles(prob, tiles, blocks):
    """The stage form from compact Jacobian tiles (H,nx,nx+nu) and Lagrangian blocks (H,nx+nu,nx+nu) -- a device's own
    `jac_tiles` / `hblocks` -- with the objective weights of `prob`."""
    nx = prob.nx
    tiles = np.asarray(tiles, dtype=np.float64)
    Qs = np.repeat((prob.Q + prob.Q.T)[None], prob.H, axis=0)
    Qs[prob.H - 1] = prob.QT + prob.QT.T
    return dict(A=tiles[:, :, :nx].copy(), B=tiles[:, :, nx:].copy(), W=np.asarray(blocks, dtype=np.float64), Qs=Qs,
                Rs=prob.R + prob.R.T)


def dense_stage(stage, H, nx, nu, sigma=None):
    """`dense` assembled from stage data instead of the oracle's callbacks (the same inputs `riccati` takes): (S, dlam)."""
    A, B, W, Qs, Rs = (np.asarray(stage[k], dtype=np.float64) for k in ("A", "B", "W", "Qs", "Rs"))
    n, m = H * (nx + nu), H * nx
    K = np.zeros((n + m, n + m))
    R = np.zeros((n + m, nx))
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
    R[m:m + nu] = W[0][nx:, :nx]
    R[n:n + nx] = A[0]
    sol = np.linalg.solve(K, -R)
    return sol[:n], sol[n:]


def perturbed(stage, rel, seed=0):
    """The stage data with every entry of A, B, W moved relatively by rel N(0,1) (seeded)."""
    rng = np.random.default_rng(seed)
    out = dict(stage)
    for k in ("A", "B", "W"):
        v = np.asarray(stage[k], dtype=np.float64)
        out[k] = v * (1.0 + rel * rng.normal(size=v.shape))
    return out


def _pivots(Quu):
    """Pivots of the Cholesky factorisation from the lower triangle (squares of its diagonal), up to and including the first
    non-positive one; and the factor L D L' when all are positive."""
    nu = Quu.shape[0]
    L = np.eye(nu)
    d = np.zeros(nu)
    for j in range(nu):
        d[j] = Quu[j, j] - (L[j, :j] ** 2) @ d[:j]
        if not d[j] > 0.0:
            return d[:j + 1], None
        for i in range(j + 1, nu):
            L[i, j] = (Quu[i, j] - (L[i, :j] * L[j, :j]) @ d[:j]) / d[j]
    return d, (L, d)


def riccati(stage, H, nx, nu, sigma=None, dtype=np.float64):
    """Gain-only backward Riccati sweep and closed-loop propagation of nx columns on stage data (stage_data /
    stage_data_from_tiles), carried out in `dtype`.  Returns dict(S (n,nx), dlam (H nx,nx), gains (H,nu,nx), pd (every pivot of
    every Quu_t positive; S, dlam and gains are NaN when not), margin (the smallest |pivot| / |Quu_t|inf met: how far the
    verdict is from flipping))."""
    dtype = np.dtype(dtype).type
    A, B, W, Qs, Rs = (np.asarray(stage[k], dtype=dtype) for k in ("A", "B", "W", "Qs", "Rs"))
    n = H * (nx + nu)
    sg = np.zeros(n, dtype=dtype) if sigma is None else np.asarray(sigma, dtype=dtype)
    sx, su = sg[:H * nx].reshape(H, nx), sg[H * nx:].reshape(H, nu)
    nan = dict(S=np.full((n, nx), np.nan), dlam=np.full((H * nx, nx), np.nan), gains=np.full((H, nu, nx), np.nan))
    P = Qs[H - 1] + np.diag(sx[H - 1])
    Ks, Ps, margin = [None] * H, [None] * H, np.inf
    for t in range(H - 1, -1, -1):
        Ps[t] = P
        PA, PB = P @ A[t], P @ B[t]
        Quu = Rs + np.diag(su[t]) + W[t][nx:, nx:] + B[t].T @ PB
        Qux = W[t][nx:, :nx] + B[t].T @ PA
        piv, fac = _pivots(Quu)
        margin = min(margin, float(np.abs(piv).min() / np.abs(Quu).max()))
        if fac is None:
            return dict(nan, pd=False, margin=margin)
        Lf, d = fac
        K = -np.linalg.solve(Lf.T, np.linalg.solve(Lf, Qux) / d[:, None]).astype(dtype)
        Ks[t] = K
        if t > 0:
            Pn = Qs[t - 1] + np.diag(sx[t - 1]) + W[t][:nx, :nx] + A[t].T @ PA + Qux.T @ K
            P = dtype(0.5) * (Pn + Pn.T)
    D = np.eye(nx, dtype=dtype)
    S = np.zeros((n, nx), dtype=dtype)
    Lm = np.zeros((H * nx, nx), dtype=dtype)
    for t in range(H):
        U = Ks[t] @ D
        D = A[t] @ D + B[t] @ U
        S[t * nx:(t + 1) * nx] = D
        S[H * nx + t * nu:H * nx + (t + 1) * nu] = U
        Lm[t * nx:(t + 1) * nx] = Ps[t] @ D
    return dict(S=S.astype(np.float64), dlam=Lm.astype(np.float64), gains=np.stack(Ks).astype(np.float64), pd=True,
                margin=margin)


def riccati_at(prob, z, x0, lam, sigma=None, dtype=np.float64):
    """`riccati` on the oracle's own stage data at (z, lam)."""
    return riccati(stage_data(prob, z, x0, lam), prob.H, prob.nx, prob.nu, sigma, dtype)


def active_set(prob, z, x0, lam, active):
    """Sensitivities of the solution with the variables flagged in `active` (n, bool) held on their bounds (dz_i = 0 there):
    the limit of `dense` along the central path under strict complementarity.  (S, dlam)."""
    n, m = prob.n, prob.H * prob.nx
    active = np.asarray(active, dtype=bool)
    K = _kkt_matrix(prob, z, x0, lam, None)
    R = _analytic_rhs(prob, z, x0, lam)
    idx = np.concatenate([np.where(~active)[0], n + np.arange(m)])
    sol = np.linalg.solve(K[np.ix_(idx, idx)], -R[idx])
    nf = int((~active).sum())
    S = np.zeros((n, prob.nx))
    S[~active] = sol[:nf]
    return S, sol[nf:]


def sigma_of(z, zl, zu, lb, ub):
    """sigma_i = zl_i / (z_i - lb_i) + zu_i / (ub_i - z_i) over the finite bounds (a zero multiplier contributes 0)."""
    z, zl, zu = (np.asarray(a, dtype=np.float64) for a in (z, zl, zu))
    lb = np.broadcast_to(np.asarray(lb, dtype=np.float64), z.shape)
    ub = np.broadcast_to(np.asarray(ub, dtype=np.float64), z.shape)
    s = np.zeros_like(z)
    lo = np.isfinite(lb) & (zl != 0.0)
    hi = np.isfinite(ub) & (zu != 0.0)
    s[lo] += zl[lo] / (z[lo] - lb[lo])
    s[hi] += zu[hi] / (ub[hi] - z[hi])
    return s


def central_path_point(ref, lb, ub, mu):
    """A synthetic point on the central path of a bounded QP next to its exact solution `ref` = (z*, lam, nu_lo, nu_hi)
    (kkt_reference.qp_solution): active variables sit mu / nu inside their bound with the exact multiplier, every other
    finite bound carries mu / gap.  Returns (z, lam, zl, zu); each finite bound has zl (z - lb) = mu."""
    z, lam, nlo, nhi = ref
    lb, ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    zc, zl, zu = np.array(z, dtype=np.float64), np.zeros(z.size), np.zeros(z.size)
    lo, hi = nlo > 0, nhi > 0
    zc[lo] = lb[lo] + mu / nlo[lo]
    zl[lo] = nlo[lo]
    zc[hi] = ub[hi] - mu / nhi[hi]
    zu[hi] = nhi[hi]
    fl = np.isfinite(lb) & ~lo
    zl[fl] = mu / (zc[fl] - lb[fl])
    fh = np.isfinite(ub) & ~hi
    zu[fh] = mu / (ub[fh] - zc[fh])
    return zc, np.array(lam, dtype=np.float64), zl, zu


def converge(prob, x0, z0, steps=12):
    """Full Newton steps from z0 with lam_0 = 0 (kkt.replay's iteration without its diagnostics): (z, lam)."""
    z, lam = np.array(z0, dtype=np.float64), np.zeros(prob.H * prob.nx)
    for _ in range(steps):
        dz, lam, _, _ = kkt.newton_step(prob, z, x0, lam, 0.0, diagnostics=False)
        z = z + dz
    return z, lam
