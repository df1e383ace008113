"""Dense float64 KKT reference for single steps of the batched solver  --  TEST INFRASTRUCTURE, not a test.

Built on `oracle.nempc_oracle.Problem` alone (constraints, jacobian, gradient, objective_hessian, lagrangian_hessian and,
for the Riccati restatement, the per-row tiles those are assembled from).  Defect rows only: box rows are bounds for the
solver, so every Problem handed in here has `box=None`.

Conventions (the oracle's): z = [states (H,nx) ; controls (H,nu)], g = Phi - x, Lagrangian L = f + lam.g, so a Newton
step of the equality-constrained NLP solves
    [[H, J'], [J, 0]] [dz ; lam+] = -[grad f ; g],      H = d2f + sum_k lam_k d2g_k + reg I on the control block
(csrc/solver_lq_impl.h: Quu = Rs + barrier + reg + B'PB -- the Levenberg term sits on the controls only).
"""
from __future__ import annotations

import warnings

import numpy as np

from oracle import nempc_oracle as orc


def _hessian(prob, z, x0, lam, reg):
    Hm = prob.lagrangian_hessian(z, x0, lam, 1.0)
    uo = prob.H * prob.nx
    Hm[np.arange(uo, prob.n), np.arange(uo, prob.n)] += reg
    return Hm


def _defects(prob, z, x0):
    return prob.constraints(z, x0)[:prob.H * prob.nx]


def _jac(prob, z, x0):
    return prob.jacobian(z, x0)[:prob.H * prob.nx]


def reduced_min_eig(Hm, J):
    """Smallest eigenvalue of H restricted to the null space of J (orthonormal basis from the SVD of J)."""
    _, s, Vt = np.linalg.svd(J, full_matrices=True)
    rank = int((s > s.max() * 1e-13).sum())
    Zn = Vt[rank:].T
    if Zn.shape[1] == 0:
        return np.inf
    Hr = Zn.T @ (0.5 * (Hm + Hm.T)) @ Zn
    return float(np.linalg.eigvalsh(Hr).min())


def newton_step(prob, z, x0, lam, reg, diagnostics=True):
    """One SQP step by a dense solve: (dz, lam+, cond(K), smallest eigenvalue of the reduced Hessian); diagnostics=False
    leaves the last two None (two SVDs of a 1775-square matrix per problem at H = 355 are seconds)."""
    assert prob.box is None
    z = np.asarray(z, dtype=np.float64)
    n, m = prob.n, prob.H * prob.nx
    Hm = _hessian(prob, z, x0, lam, reg)
    J = _jac(prob, z, x0)
    K = np.zeros((n + m, n + m))
    K[:n, :n] = Hm
    K[:n, n:] = J.T
    K[n:, :n] = J
    rhs = -np.concatenate([prob.gradient(z), _defects(prob, z, x0)])
    sol = np.linalg.solve(K, rhs)
    if not diagnostics:
        return sol[:n], sol[n:], None, None
    return sol[:n], sol[n:], float(np.linalg.cond(K)), reduced_min_eig(Hm, J)


def l1_merit(prob, z, x0, pen):
    return prob.objective(z) + pen * float(np.abs(_defects(prob, z, x0)).sum())


def replay(prob, x0, z0, steps, reg):
    """Full-step SQP from z0 with lam_0 = 0 and lam <- lam+ (the solver's update at alpha = 1).  One dict per step:
    z (the iterate after it), dz, lam (= lam+), cond, eig (reduced-Hessian gate), dmerit (l1-merit gate: merit after the full
    step minus merit before it, penalty pen = max(pen, 1.5 |lam+|inf + 1e-3) from 1 as in solver_merit0_body), z_before,
    lam_before."""
    z = np.array(z0, dtype=np.float64)
    lam = np.zeros(prob.H * prob.nx)
    pen = 1.0
    out = []
    for _ in range(steps):
        dz, lamn, cond, eig = newton_step(prob, z, x0, lam, reg)
        pen = max(pen, 1.5 * float(np.abs(lamn).max()) + 1e-3)
        dmerit = l1_merit(prob, z + dz, x0, pen) - l1_merit(prob, z, x0, pen)
        out.append(dict(z=z + dz, dz=dz, lam=lamn, cond=cond, eig=eig, dmerit=dmerit, pen=pen, z_before=z, lam_before=lam))
        z, lam = z + dz, lamn
    return out


# --------------------------------------------------------------------------------------
# The same step by a Riccati sweep (recursion of tools/lq_scan_proto.py `seq`), in a chosen precision.
# Rolling-window models (window w > 1) are made stage-wise the way the solver does it: the window is the state,
#     s_t = (x_t, x_{t-1}, .., x_{t-w+1}, u_t, .., u_{t-w+2}),    ns = w nx + (w-1) nu
# with copy rows of zero defect below the network's rows; the multipliers of the defect rows are the first nx entries of
# the augmented costate.  w = 1 gives the plain (x_{t-1}, u_t) stages.
# --------------------------------------------------------------------------------------
def _stage_maps(prob):
    """For every tile column: (is_control_of_this_stage, index into s_{t-1} or into u_t)."""
    nx, nu, w = prob.nx, prob.nu, prob.window
    to_u = np.zeros(prob.tw, dtype=bool)
    idx = np.zeros(prob.tw, dtype=np.int64)
    for j in range(w):
        lag = (w - 1 - j) if prob.forward_rolling else j
        idx[j * nx:(j + 1) * nx] = lag * nx + np.arange(nx)
        cu = slice(w * nx + j * nu, w * nx + (j + 1) * nu)
        if lag == 0:
            to_u[cu] = True
            idx[cu] = np.arange(nu)
        else:
            idx[cu] = w * nx + (lag - 1) * nu + np.arange(nu)
    return to_u, idx


def stage_problem(prob, z, x0, lam):
    """The LQ sub-problem in stage form, float64: A (H,ns,ns), B (H,ns,nu), c (H,ns), W (H,ns+nu,ns+nu) Lagrangian blocks
    over (s_{t-1}, u_t), Qs (H,ns,ns) state weights (2 sym Q on the primary block, terminal weight at H-1), Rs (nu,nu),
    gx (H,ns), gu (H,nu) objective gradient."""
    H, nx, nu, w = prob.H, prob.nx, prob.nu, prob.window
    ns = w * nx + (w - 1) * nu
    z = np.asarray(z, dtype=np.float64)
    x, phi, dphi, d2phi = prob.tiles(z, x0, want_hess=True)
    to_u, idx = _stage_maps(prob)
    col = np.where(to_u, ns + idx, idx)          # position in (s_{t-1}, u_t)
    A = np.zeros((H, ns, ns)); B = np.zeros((H, ns, nu)); c = np.zeros((H, ns)); W = np.zeros((H, ns + nu, ns + nu))
    lam = np.asarray(lam, dtype=np.float64).reshape(H, nx)
    for t in range(H):
        T = np.zeros((nx, ns + nu))
        T[:, col] = dphi[t]
        A[t, :nx], B[t, :nx] = T[:, :ns], T[:, ns:]
        for l in range(1, w):                    # x_{t-l} of s_t is x_{t-1-(l-1)} of s_{t-1}
            A[t, l * nx:(l + 1) * nx, (l - 1) * nx:l * nx] = np.eye(nx)
        if w > 1:
            B[t, w * nx:w * nx + nu] = np.eye(nu)
            for l in range(2, w):
                A[t, w * nx + (l - 1) * nu:w * nx + l * nu, w * nx + (l - 2) * nu:w * nx + (l - 1) * nu] = np.eye(nu)
        c[t, :nx] = phi[t] - x[t]
        W[t][np.ix_(col, col)] = np.einsum("k,kpq->pq", lam[t], d2phi[t])
    Qs = np.zeros((H, ns, ns))
    Qs[:, :nx, :nx] = prob.Q + prob.Q.T
    Qs[H - 1, :nx, :nx] = prob.QT + prob.QT.T
    gr = prob.gradient(z)
    gx = np.zeros((H, ns))
    gx[:, :nx] = gr[:H * nx].reshape(H, nx)
    gu = gr[H * nx:].reshape(H, nu)
    return dict(A=A, B=B, c=c, W=W, Qs=Qs, Rs=prob.R + prob.R.T, gx=gx, gu=gu, ns=ns)


def riccati_step(prob, z, x0, lam, reg, dtype=np.float64, sp=None):
    """(dz, lam+) of the same Newton step by one backward and one forward Riccati sweep carried out in `dtype`.  Raises
    numpy.linalg.LinAlgError at a pivot of a control Hessian that is not above PIVOT_MIN.  sp: stage_problem(prob, z, x0, lam)
    where the caller already has it (the damping ladder sweeps the same stages at several reg)."""
    assert prob.box is None
    dtype = np.dtype(dtype).type
    if sp is None:
        sp = stage_problem(prob, z, x0, lam)
    H, nx, nu, ns = prob.H, prob.nx, prob.nu, sp["ns"]
    A, B, c, W, Qs, Rs, gx, gu = (np.asarray(sp[k], dtype=dtype) for k in ("A", "B", "c", "W", "Qs", "Rs", "gx", "gu"))
    regI = (dtype(reg) * np.eye(nu)).astype(dtype)
    P, p = Qs[H - 1].copy(), gx[H - 1].copy()
    Ps, ps, Ks, ks = [None] * H, [None] * H, [None] * H, [None] * H
    for t in range(H - 1, -1, -1):
        Ps[t], ps[t] = P, p
        PA, PB, Pc = P @ A[t], P @ B[t], P @ c[t] + p
        Quu = Rs + W[t][ns:, ns:] + regI + B[t].T @ PB
        qu = gu[t] + B[t].T @ Pc
        Qux = W[t][ns:, :ns] + B[t].T @ PA
        L = np.linalg.cholesky(Quu)              # (raises where the solver would restart with more damping)
        if not (np.diag(L) ** 2 > PIVOT_MIN).all():
            raise np.linalg.LinAlgError("pivot not above PIVOT_MIN")
        K = -np.linalg.solve(L.T, np.linalg.solve(L, Qux)).astype(dtype)
        kv = -np.linalg.solve(L.T, np.linalg.solve(L, qu)).astype(dtype)
        Ks[t], ks[t] = K, kv
        if t > 0:
            Pn = Qs[t - 1] + W[t][:ns, :ns] + A[t].T @ PA + Qux.T @ K
            p = gx[t - 1] + A[t].T @ Pc + Qux.T @ kv
            P = dtype(0.5) * (Pn + Pn.T)
    ds = np.zeros(ns, dtype=dtype)               # x0 and the history are data
    dz = np.zeros(prob.n, dtype=dtype)
    lamn = np.zeros(H * nx, dtype=dtype)
    for t in range(H):
        du = ks[t] + Ks[t] @ ds
        ds = c[t] + A[t] @ ds + B[t] @ du
        lamn[t * nx:(t + 1) * nx] = (ps[t] + Ps[t] @ ds)[:nx]
        dz[t * nx:(t + 1) * nx] = ds[:nx]
        dz[H * nx + t * nu:H * nx + (t + 1) * nu] = du
    assert dz.dtype == dtype
    return dz.astype(np.float64), lamn.astype(np.float64)


def sweep_error(prob, x0, z0, steps, reg, dtype):
    """What a correct sweep in `dtype` loses on the systems of a replay: sum over the replayed steps (each taken at the
    float64 reference iterate and multipliers) of |riccati_step(dtype) - newton_step(float64)|inf, cumulative per step."""
    acc, out = 0.0, []
    for st in replay(prob, x0, z0, steps, reg):
        dz, _ = riccati_step(prob, st["z_before"], x0, st["lam_before"], reg, dtype)
        acc += float(np.abs(dz - st["dz"]).max())
        out.append(acc)
    return out


# --------------------------------------------------------------------------------------
# The damping state machine: what the solver does when a control Hessian Quu_t is not positive definite.  The same ladder is
# written three times on the device (csrc/solver_lq_impl.h, solver_lqw_impl.h, solver_lq_scan_impl.h); this is its
# restatement.  The constants are the code's:
#   REG_RAISE, REG_RELAX   csrc/solver.hip, ProcessKnobs::reg_raise / reg_relax (half decades)
#   REG_FLOOR              csrc/solver_args.h, NEMPC_REG_FLOOR: the first damping level of a restarted sweep
#   REG_RELAX_FLOOR        csrc/solver_merit_impl.h, solver_merit_body: reg <- max(reg * reg_relax, 1e-9)
#   PIVOT_MIN              csrc/solver_lq_impl.h: a sweep fails at a Cholesky pivot that is not > 1e-12
#   LQ_ATTEMPTS            csrc/solver.hip, plan_lq: levels tried per iteration when the caller passes lq_attempts = 0
# --------------------------------------------------------------------------------------
REG_RAISE = 3.1622776601683795
REG_RELAX = 0.31622776601683794
REG_FLOOR = 1e-3
REG_RELAX_FLOOR = 1e-9
PIVOT_MIN = 1e-12
LQ_ATTEMPTS = 3
ROBUST_D = {np.float64: 1e-3, np.float32: 5e-2}     # relative move of every level's reg that must not change the winner


def damping_levels(reg, attempts, raise_=REG_RAISE, floor=REG_FLOOR):
    """attempts + 1 values: entry j is the stored `reg` raised j times by reg <- max(reg raise_, floor).  Entries 0 ..
    attempts - 1 are the levels an iteration may sweep at; the last is what is stored when none of them goes through."""
    out = [float(reg)]
    for _ in range(attempts):
        out.append(max(out[-1] * raise_, floor))
    return out


def winning_level(prob, z, x0, lam, reg, attempts, dtype=np.float64, scale=1.0, sp=None):
    """The first of `attempts` levels from the stored `reg` whose sweep in `dtype` goes through (riccati_step does not
    raise), or None.  scale: every level's reg times this (winning_level_is_robust)."""
    if sp is None:
        sp = stage_problem(prob, z, x0, lam)
    for j, r in enumerate(damping_levels(reg, attempts)[:attempts]):
        try:
            riccati_step(prob, z, x0, lam, r * scale, dtype, sp=sp)
        except np.linalg.LinAlgError:
            continue
        return j
    return None


def winning_level_is_robust(prob, z, x0, lam, reg, attempts, dtype=np.float64, sp=None):
    """The same winner with every level's reg scaled by 1 - d and by 1 + d (d = ROBUST_D of the handle's precision).  A pivot
    moves one for one with reg, so the deciding pivots are about d reg away from zero: the device's rounding cannot
    decide otherwise."""
    if sp is None:
        sp = stage_problem(prob, z, x0, lam)
    d = ROBUST_D[np.dtype(dtype).type]
    w = winning_level(prob, z, x0, lam, reg, attempts, dtype, 1.0, sp)
    return all(winning_level(prob, z, x0, lam, reg, attempts, dtype, s, sp) == w for s in (1.0 - d, 1.0 + d))


def damped_replay(prob, x0, z0, iterations, reg0, attempts=LQ_ATTEMPTS, dtype=np.float64):
    """The solver's iteration with full steps and the damping state machine, from z0 with lam_0 = 0 and the stored reg = reg0.
    Per iteration: the first of `attempts` levels from the stored reg that sweeps through in `dtype` (the handle's precision;
    the step itself is the dense float64 one at that level's reg) is taken, that level's reg is stored, and only a step whose
    level is 0 relaxes it, reg <- max(reg REG_RELAX, REG_RELAX_FLOOR); where none goes through the problem sits the iteration
    out: z, lam unchanged, stored reg = raised `attempts` times.  One dict per iteration: z, lam (after it), level (None =
    sat out), reg_used (None = sat out), reg_after, dz (zero where sat out), dmerit (l1-merit change of the full step under
    pen, 0 where sat out), pen (as in `replay`), robust (winning_level_is_robust), z_before, lam_before."""
    z = np.array(z0, dtype=np.float64)
    lam = np.zeros(prob.H * prob.nx)
    pen, reg = 1.0, float(reg0)
    out = []
    for _ in range(iterations):
        sp = stage_problem(prob, z, x0, lam)
        levels = damping_levels(reg, attempts)
        level = winning_level(prob, z, x0, lam, reg, attempts, dtype, 1.0, sp)
        robust = winning_level_is_robust(prob, z, x0, lam, reg, attempts, dtype, sp)
        if level is None:
            reg = levels[attempts]
            out.append(dict(z=z, lam=lam, level=None, reg_used=None, reg_after=reg, dz=np.zeros(prob.n), dmerit=0.0, pen=pen,
                            robust=robust, z_before=z, lam_before=lam))
            continue
        used = levels[level]
        dz, lamn, _, _ = newton_step(prob, z, x0, lam, used, diagnostics=False)
        pen = max(pen, 1.5 * float(np.abs(lamn).max()) + 1e-3)
        dmerit = l1_merit(prob, z + dz, x0, pen) - l1_merit(prob, z, x0, pen)
        reg = used if level > 0 else max(used * REG_RELAX, REG_RELAX_FLOOR)
        out.append(dict(z=z + dz, lam=lamn, level=level, reg_used=used, reg_after=reg, dz=dz, dmerit=dmerit, pen=pen,
                        robust=robust, z_before=z, lam_before=lam))
        z, lam = z + dz, lamn
    return out


def sweep_error_damped(prob, x0, rp, dtype):
    """sweep_error for a damped_replay `rp`: cumulative |riccati_step(dtype) - newton_step(float64)|inf over the steps taken,
    each at the replay's own iterate, multipliers and reg; an iteration that sat out adds nothing."""
    acc, out = 0.0, []
    for st in rp:
        if st["level"] is not None:
            dz, _ = riccati_step(prob, st["z_before"], x0, st["lam_before"], st["reg_used"], dtype)
            acc += float(np.abs(dz - st["dz"]).max())
        out.append(acc)
    return out


def min_passing_reg(prob, z, x0, lam, dtype=np.float64, rel=1e-9):
    """The smallest reg at which the sweep in `dtype` goes through, by bisection (0.0 where it does undamped).  Going through
    is monotone in reg: more damping makes every P_t, and with it every Quu_t, larger in the positive semi-definite order."""
    sp = stage_problem(prob, z, x0, lam)

    def ok(r):
        try:
            riccati_step(prob, z, x0, lam, r, dtype, sp=sp)
            return True
        except np.linalg.LinAlgError:
            return False
    if ok(0.0):
        return 0.0
    hi = 1e-6
    while not ok(hi):
        hi *= 10.0
        assert hi < 1e12
    lo = hi / 10.0 if hi > 1e-6 else 0.0
    while hi - lo > rel * hi:
        mid = 0.5 * (lo + hi)
        lo, hi = (lo, mid) if ok(mid) else (mid, hi)
    return hi


# --------------------------------------------------------------------------------------
# Bounded convex QP (linear dynamics): the unique minimiser by an exact active-set KKT solve
# --------------------------------------------------------------------------------------
def qp_solution(prob, x0, lb, ub):
    """Linear networks only.  Returns (z*, lam (defect multipliers), nu_lo, nu_hi (bound multipliers, >= 0, zero off the
    active set)).  SciPy SLSQP on the oracle's callbacks proposes the active set; one KKT system with those variables fixed
    gives the point, and the signs of the bound multipliers and the bounds of the free variables are verified."""
    from scipy.optimize import Bounds, minimize
    assert prob.box is None and all(a == "linear" for a in prob.net.act)
    n, m = prob.n, prob.H * prob.nx
    lb, ub = np.asarray(lb, dtype=np.float64), np.asarray(ub, dtype=np.float64)
    z00 = np.zeros(n)
    Hm, c0 = prob.objective_hessian(), prob.gradient(z00)
    J, g0 = _jac(prob, z00, x0), _defects(prob, z00, x0)
    zi = np.clip(orc.cold_start(x0, prob.H, prob.nu), np.where(np.isfinite(lb), lb, -np.inf), np.where(np.isfinite(ub), ub, np.inf))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = minimize(prob.objective, zi, method="SLSQP", jac=prob.gradient, bounds=Bounds(lb, ub),
                       constraints=[{"type": "eq", "fun": lambda z: _defects(prob, z, x0), "jac": lambda z: _jac(prob, z, x0)}],
                       options={"maxiter": 500, "ftol": 1e-14})
    at_lo = res.x <= lb + 1e-7
    at_hi = res.x >= ub - 1e-7
    for _ in range(20):                          # (SLSQP's set is almost always right; repair it if not)
        act = at_lo | at_hi
        free = ~act
        zA = np.where(at_lo, lb, ub)[act]
        nf = int(free.sum())
        K = np.zeros((nf + m, nf + m))
        K[:nf, :nf] = Hm[np.ix_(free, free)]
        K[:nf, nf:] = J[:, free].T
        K[nf:, :nf] = J[:, free]
        rhs = np.concatenate([-c0[free] - Hm[np.ix_(free, act)] @ zA, -g0 - J[:, act] @ zA])
        sol = np.linalg.solve(K, rhs)
        z = np.empty(n)
        z[free], z[act] = sol[:nf], zA
        lam = sol[nf:]
        r = Hm @ z + c0 + J.T @ lam              # = nu_lo - nu_hi
        drop = (at_lo & (r < 0.0)) | (at_hi & (r > 0.0))
        add_lo, add_hi = free & (z < lb), free & (z > ub)
        if not (drop.any() or add_lo.any() or add_hi.any()):
            break
        at_lo = (at_lo & ~drop) | add_lo
        at_hi = (at_hi & ~drop) | add_hi
    else:
        raise RuntimeError("qp_solution: the active set did not settle")
    nu_lo, nu_hi = np.where(at_lo, r, 0.0), np.where(at_hi, -r, 0.0)
    assert (nu_lo >= 0.0).all() and (nu_hi >= 0.0).all() and (z >= lb).all() and (z <= ub).all()
    return z, lam, nu_lo, nu_hi
