"""GPU: per-problem, time-varying bounds (nempc_bind_bounds) in nempc_solve / nempc_solve_duals, nempc_kkt_residual,
nempc_sensitivity and the controller's batched calls.

References: for the bounded convex QPs the exact active-set solutions of tests/bounds_cases.py (one per problem and window)
and the NumPy certificate tests/kkt_certificate.py with the problem's own bounds; for nonlinear problems the library itself,
one problem at a time with that problem's bounds as the host lb / ub of the call.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import nempc_oracle as orc
import bounds_cases as bc
import kkt_certificate as cert
import solver_step_cases as sc

pytestmark = pytest.mark.gpu

PARITY_TOL = {"float64": 1e-11, "float32": 3e-4}     # tests/test_gpu_parity.py (as tests/test_gpu_duals.py has it)
NAMES = ("xlb", "xub", "ulb", "uub")
TOL_CONSTRAINT = 1e-8
# The certificate test's barrier floor is the one of test_bounded_qp_solution_carries_a_kkt_certificate: its bound on the
# complementarity, 10 mu_min, is a statement about the barrier and can only hold while mu_min is not below what the stopping
# test leaves of zl (z - lb) at an active bound, nu tol_step (1 + |z|inf) ~ 2.5e-9 here.  (The end-point test compares with z*
# and needs the smaller bounds_cases.MU_MIN; see there.)
MU_MIN_DUALS = 1e-9


def _np(t):
    return t.detach().cpu().double().numpy()


def _inf_norm(M):
    return float(np.abs(M).sum(axis=1).max())


def _stationarity_bound(prob, z, zl, zu, lb, ub, tol_step):
    """10 |W|inf tol_step (1 + |z|inf), W = objective Hessian + diag(zl / (z - lb) + zu / (ub - z)) of the returned values:
    the largest change of the stationarity residual a last step admitted by the stopping test can leave behind
    (tests/test_gpu_duals.py, restated)."""
    flo, fhi = np.isfinite(lb), np.isfinite(ub)
    dg = np.zeros(prob.n)
    dg[flo] += zl[flo] / (z[flo] - lb[flo])
    dg[fhi] += zu[fhi] / (ub[fhi] - z[fhi])
    return 10.0 * _inf_norm(prob.objective_hessian() + np.diag(dg)) * tol_step * (1.0 + np.abs(z).max())


def _dev(eng, arrays, B=None):
    return {k: eng.to_device(v if B is None else v[:B]) for k, v in arrays.items()}


def _flat(arrays, b, rows):
    """(lb, ub) (n,) of problem b from (B,L,d) schedules, rows `rows`, in z order."""
    return (np.concatenate([arrays["xlb"][b, rows].ravel(), arrays["ulb"][b, rows].ravel()]),
            np.concatenate([arrays["xub"][b, rows].ravel(), arrays["uub"][b, rows].ravel()]))


# --------------------------------------------------------------------------------------------------------------------
# 4. / 5. bounded convex QPs: exact end points per problem, duals and certificate
# --------------------------------------------------------------------------------------------------------------------
QP_KERNELS = {"2x1_h12": ("thread", "wave", "scan"), "3x2_h7": ("thread", "wave")}
QP_CASES = [(n, k) for n in bc.ROWS for k in QP_KERNELS[n]]


@functools.lru_cache(maxsize=None)
def _qp_engine(name):
    return bc.schedule(name)[0].engine()


def _qp_solve(name, sched, offset, barrier, linesearch, lq, mu_min=bc.MU_MIN):
    """The BOUNDED_B problems of the row under rows offset .. offset+H-1 of `sched`, bound; no box rows, no host lb / ub."""
    case, eng = bc.schedule(name)[0], _qp_engine(name)
    X0 = case.bind(eng, case.B)
    try:
        eng.bind_bounds(**_dev(eng, sched), offset=offset)
        Z, st, it, per, d = eng.solve(X0, None, reg=sc.REG, max_iter=400, barrier=barrier, linesearch=linesearch, lq_kernel=lq,
                                      mu_min=mu_min, tol_step=bc.TOL_STEP, tol_constraint=TOL_CONSTRAINT,
                                      return_iterations=True, return_duals=True)
        r, s = eng.kkt_residual(Z, X0, d["lam"], d["zl"], d["zu"], want_stat=True)
        return dict(Z=_np(Z), st=st.cpu().numpy(), it=it, per=per.cpu().numpy(), lam=_np(d["lam"]), zl=_np(d["zl"]),
                    zu=_np(d["zu"]), r=_np(r), s=_np(s))
    finally:
        eng.bind_bounds()


@pytest.mark.parametrize("linesearch", ["loop", "deferred"])
@pytest.mark.parametrize("barrier", ["primal-dual", "primal"])
@pytest.mark.parametrize("name,lq", QP_CASES)
def test_every_problem_ends_at_the_solution_under_its_own_window(name, lq, barrier, linesearch):
    """Item 4.  B = 4 problems, each with a schedule of control limits and a state cap of its own (bounds_cases), bound at
    rows 0 and 3 of the L = H + 3 row tensors: every problem converges, ends within
    10 (mu_min / nu_min_b + tol_step (1 + |z*_b|inf)) of ITS exact solution and lies inside ITS bounds to 1e-12.  The
    fixture keeps every solution more than 100 tolerances away from the one under shared bounds
    (tests/test_bounds_cpu.py), so bounds of another problem or another row cannot pass.  mu_min is bounds_cases.MU_MIN
    (1e-10; why, there).  Observed on an MI355X: every problem of the 160 solves converges in 15 .. 34 iterations, the
    largest error is 0.27 of its tolerance; at mu_min = 1e-9 problem 2 of 3x2_h7 at offset 3 ended 2.759e-07 from z*
    against 2.062e-07 -- the central-path point itself, bounds_cases.inactive_pull gives 2.76e-07."""
    case, sched = bc.schedule(name)
    for offset in bc.OFFSETS:
        out, ref = _qp_solve(name, sched, offset, barrier, linesearch, lq), bc.reference(name, offset)
        assert (out["st"] == 0).all(), (offset, out["st"].tolist(), out["it"])
        for b in range(case.B):
            zs = ref[b][0]
            nu_min = bc.smallest_active_multiplier(ref[b])
            assert nu_min >= sc.NU_MIN
            tol = bc.end_point_tolerance(nu_min, zs)
            e = np.abs(out["Z"][b] - zs).max()
            lo, hi = bc.window(name, b, offset)
            print(f"[bounds end point {name} {lq} {barrier} {linesearch} offset {offset}] b={b}: |Z - z*| = {e:.3e}, tolerance "
                  f"{tol:.3e}, iterations {out['per'][b]}")
            assert e <= tol, (offset, b, e, tol)
            assert (out["Z"][b] >= lo - 1e-12).all() and (out["Z"][b] <= hi + 1e-12).all(), (offset, b)


@pytest.mark.parametrize("linesearch", ["loop", "deferred"])
@pytest.mark.parametrize("barrier", ["primal-dual", "primal"])
@pytest.mark.parametrize("name,lq", QP_CASES)
def test_the_duals_certify_every_problem_against_its_own_bounds(name, lq, barrier, linesearch):
    """Item 5.  The same solves with problem 2's lower control limit removed (-inf) on the last three stages of the window.
    From the RETURNED Z, lam, zl, zu the NumPy certificate with the problem's own bounds gives r[3] == 0,
    r[1] <= tol_constraint, r[2] <= 10 mu_min, r[0] <= 10 |W|inf tol_step (1 + |z|inf); nempc_kkt_residual under the binding
    agrees with it to the fp64 parity tolerance; the multipliers on the removed limits are exactly 0."""
    case, base = bc.schedule(name)
    H, nx, hx = case.H, case.nx, case.H * case.nx
    fails = []
    for offset in bc.OFFSETS:
        sched = {k: v.copy() for k, v in base.items()}
        sched["ulb"][2, offset + H - 3:offset + H] = -np.inf
        out = _qp_solve(name, sched, offset, barrier, linesearch, lq, MU_MIN_DUALS)
        assert (out["st"] == 0).all(), (offset, out["st"].tolist(), out["it"])
        for b in range(case.B):
            prob = case.problem(b)
            lo, hi = _flat(sched, b, slice(offset, offset + H))
            Z, lam, zl, zu = out["Z"][b], out["lam"][b], out["zl"][b], out["zu"][b]
            r, s = cert.residuals(prob, Z, case.X0[b], lam[:hx], zl, zu, lo, hi)
            r0_bound = _stationarity_bound(prob, Z, zl, zu, lo, hi, bc.TOL_STEP)
            tag = f"[bounds duals {name} {lq} {barrier} {linesearch} offset {offset}] b={b}:"
            print(f"{tag} stationarity {r[0]:.3e} (bound {r0_bound:.3e}), primal {r[1]:.3e}, complementarity {r[2]:.3e} "
                  f"(bound {10 * MU_MIN_DUALS:.1e}), dual {r[3]:.3e}")
            for ok, what in ((r[3] == 0.0, f"r[3] = {r[3]}"), (r[1] <= TOL_CONSTRAINT, f"r[1] = {r[1]:.3e}"),
                             (r[2] <= 10.0 * MU_MIN_DUALS, f"r[2] = {r[2]:.3e}"), (r[0] <= r0_bound, f"r[0] = {r[0]:.3e} > {r0_bound:.3e}"),
                             ((zl[~np.isfinite(lo)] == 0).all() and (zu[~np.isfinite(hi)] == 0).all(), "multiplier on an infinite bound")):
                if not ok:
                    fails.append(f"{tag} {what}")
            scale = 1.0 + np.abs(prob.gradient(Z)).max() + np.abs(prob.jacobian(Z, case.X0[b])).max() * np.abs(lam).max()
            rd, sd = out["r"][b], out["s"][b]
            e_dev = max(np.abs(sd - s).max() / scale, abs(rd[0] - r[0]) / scale, abs(rd[1] - r[1]), abs(rd[2] - r[2]), abs(rd[3] - r[3]))
            print(f"{tag} device evaluator {rd.tolist()}, largest scaled difference {e_dev:.3e}")
            if not e_dev <= PARITY_TOL["float64"]:
                fails.append(f"{tag} device evaluator differs by {e_dev:.3e}")
        assert not np.isfinite(_flat(sched, 2, slice(offset, offset + H))[0]).all()
    assert not fails, "\n".join(fails)


# --------------------------------------------------------------------------------------------------------------------
# 6. / 7. / 8. / 9. nonlinear problems: the library one problem at a time is the reference
# --------------------------------------------------------------------------------------------------------------------
class Setup:
    """One nonlinear (or fp32) shape with BMAX starts; the engine is built on first use."""

    def __init__(self, net, H, nx, nu, integ, DT, dtype, obj, X0, bmax, kw=None):
        self.net, self.H, self.nx, self.nu, self.integ, self.DT, self.dtype, self.obj = net, H, nx, nu, integ, DT, dtype, obj
        self.X0, self.bmax, self.n, self.kw = X0, bmax, H * (nx + nu), kw or {}

    @functools.cached_property
    def eng(self):
        from pyneuralempc_amd import CallbackEngine
        eng = CallbackEngine(self.net.W, self.net.b, self.H, self.nx, self.nu, integrator=self.integ, DT=self.DT,
                             dtype={"float64": torch.float64, "float32": torch.float32}[self.dtype], device="cuda:0",
                             max_batch=self.bmax, activations=self.net.act)
        eng.set_objective(**self.obj)
        return eng

    def problem(self, b):
        return orc.Problem(self.net, self.H, self.nx, self.nu, sc.KINDS[self.integ], self.DT, **self.obj)

    def start(self, B):
        return np.concatenate([np.tile(self.X0[:B], (1, self.H)), np.zeros((B, self.H * self.nu))], axis=1)


@functools.lru_cache(maxsize=None)
def _setup(shape):
    if shape == "2x1_fused":      # the setting of test_gpu_tracking's _nl_solver: the compiled fused shape
        nx, nu, H, B = 2, 1, 20, 160
        net = orc.MLP.random(nx + nu, [64, 64], nx, seed=3)
        net.W[-1] *= 0.2
        net.b[-1] *= 0.2
        obj = dict(Q=np.eye(nx), R=0.1 * np.eye(nu), xref=np.zeros((H, nx)), uref=np.zeros((H, nu)), cx=np.zeros((H, nx)),
                   cu=np.zeros((H, nu)))
        X0 = np.random.default_rng(4).uniform(-0.8, 0.8, size=(B, nx))
        return Setup(net, H, nx, nu, "discret", 1.0, "float64", obj, X0, B)
    case = {"6x3_rk4": lambda: sc.nl_case("6x3_rk4"), "2x1_fp32": lambda: sc.qp_case("2x1_fp32", 20),
            "2x1_global": lambda: sc.qp_case("2x1_global", sc.H_GLOBAL)}[shape]()
    return Setup(case.net, case.H, case.nx, case.nu, case.integ, case.DT, case.dtype, case.obj, case.X0, case.B)


def _limits(s, B, seed=21):
    """(B,H,d) bounds: control limits +- U(0.3, 0.7) drawn per problem (one value per problem, every stage), states +- 3;
    values as the handle's dtype holds them."""
    c = sc._round(np.random.default_rng(seed).uniform(0.3, 0.7, size=B), s.dtype)
    xub = np.full((B, s.H, s.nx), 3.0)
    uub = np.broadcast_to(c[:, None, None], (B, s.H, s.nu)).copy()
    return dict(xlb=-xub, xub=xub, ulb=-uub, uub=uub)


def _solve_kw():
    return dict(max_iter=150, return_iterations=True, return_duals=True)


def _batch(s, lim, B, Zi=None, X0=None, **kw):
    eng = s.eng
    X0 = eng.to_device(s.X0[:B]) if X0 is None else X0
    Zi = eng.to_device(s.start(B)) if Zi is None else Zi
    try:
        eng.bind_bounds(**_dev(eng, lim))
        return eng.solve(X0, Zi, **{**_solve_kw(), **kw})
    finally:
        eng.bind_bounds()


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("shape", ["2x1_fused", "6x3_rk4", "2x1_fp32"])
def test_a_batch_under_the_binding_against_one_problem_at_a_time(shape):
    """Item 6.  B = 6: problems 0 - 3 have control limits of their own (states +- 3), problem 4 has every bound infinite,
    problem 5 has uub < ulb on one stage.  solve, kkt_residual and sensitivity (du0, dz) under the binding against B calls of
    one problem each with that problem's bounds as host lb / ub: equal status, Z within 10 tol_step (1 + |Z|inf), residuals
    and sensitivities (at the batch's points) within the dtype's parity tolerance.  Problem 4 takes the iterations of its
    unbounded single solve and has zero bound multipliers; problem 5 returns status 1, its start and 0 iterations, and shows
    as r[1] > 0; problems 0 - 4 are bit-identical to the same batch with problem 5's bounds repaired.
    On an MI355X batch and single solves are bit-identical at all three shapes (Z, multipliers, iterations, du0, dz): asserted
    too, as test_solver_uniform_binding_against_the_shared_objective does for the tracking binding."""
    from pyneuralempc_amd._lib import NempcError
    s = _setup(shape)
    eng, B, H, nx, nu, n = s.eng, 6, s.H, s.nx, s.nu, s.n
    tol_step = 1e-8 if s.dtype == "float64" else 1e-4
    lim = _limits(s, B)
    for k in NAMES:
        lim[k][4] = -np.inf if k in ("xlb", "ulb") else np.inf
    good = {k: v.copy() for k, v in lim.items()}
    lim["uub"][5, H // 2] = lim["ulb"][5, H // 2] - 0.1
    X0, Zi = eng.to_device(s.X0[:B]), eng.to_device(s.start(B))
    Z, st, it, per, d = _batch(s, lim, B, Zi, X0)
    Zg, stg, _, perg, dg = _batch(s, good, B, Zi, X0)
    st_h, per_h = st.cpu().numpy(), per.cpu().numpy()
    # problem 5 fails alone, decided on the device; the others do not see it
    assert st_h[5] == 1 and per_h[5] == 0 and torch.equal(Z[5], Zi[5]), (st_h.tolist(), per_h.tolist())
    assert (_np(d["zl"])[5] == 0).all() and (_np(d["zu"])[5] == 0).all()
    for a, b in ((Z, Zg), (st, stg), (per, perg), (d["lam"], dg["lam"]), (d["zl"], dg["zl"]), (d["zu"], dg["zu"])):
        assert torch.equal(a[:5], b[:5]), "problems 0 - 4 differ when problem 5's bounds are repaired"
    assert st_h[4] == 0, st_h.tolist()
    assert (_np(d["zl"])[4] == 0).all() and (_np(d["zu"])[4] == 0).all()
    try:
        eng.bind_bounds(**_dev(eng, lim))
        r = _np(eng.kkt_residual(Z, X0, d["lam"], d["zl"], d["zu"]))
        sens = eng.sensitivity(Z, X0, d["lam"], d["zl"], d["zu"], want=("du0", "dz"))
    finally:
        eng.bind_bounds()
    assert r[5, 1] > 0.0
    ptol, identical = PARITY_TOL[s.dtype], True
    for b in range(5):
        lo, hi = _flat(lim, b, slice(0, H))
        lo, hi = (None, None) if b == 4 else (lo, hi)
        sl = slice(b, b + 1)
        Z1, st1, _, per1, d1 = eng.solve(X0[sl].contiguous(), Zi[sl].contiguous(), lo, hi, **_solve_kw())
        assert st1.cpu().numpy()[0] == st_h[b]
        z, z1 = _np(Z)[b], _np(Z1)[0]
        e = np.abs(z - z1).max()
        same = all(torch.equal(a[b], c[0]) for a, c in ((Z, Z1), (d["lam"], d1["lam"]), (d["zl"], d1["zl"]), (d["zu"], d1["zu"])))
        identical = identical and same and per_h[b] == per1.cpu().numpy()[0]
        assert e <= 10.0 * tol_step * (1.0 + np.abs(z1).max()), (b, e)
        if b == 4:
            assert per_h[4] == per1.cpu().numpy()[0], (per_h[4], per1.tolist())
        pt = [t[sl].contiguous() for t in (Z, X0, d["lam"], d["zl"], d["zu"])]
        r1 = _np(eng.kkt_residual(*pt, lo, hi))[0]
        s1 = eng.sensitivity(*pt, lo, hi, want=("du0", "dz"))
        assert np.abs(r[b] - r1).max() <= ptol * (1.0 + np.abs(r1).max()), (b, r[b], r1)
        assert sens["status"].cpu().numpy()[b] == s1["status"].cpu().numpy()[0]
        for k in ("du0", "dz"):
            a, c = _np(sens[k])[b], _np(s1[k])[0]
            assert np.isfinite(c).all() and np.abs(a - c).max() <= ptol * (1.0 + np.abs(c).max()), (b, k)
            identical = identical and _same(a, c)
        print(f"[bounds one-at-a-time {shape}] b={b}: |Z - Z_single| = {e:.3e}, iterations {per_h[b]} / {per1.tolist()[0]}, "
              f"bit-identical {same}")
    print(f"[bounds one-at-a-time {shape}] batch under the binding bit-identical to the single solves: {identical}")
    assert identical
    with pytest.raises(NempcError):       # (the host check sees what the device decided: the reference for problem 5)
        eng.solve(X0[5:6].contiguous(), Zi[5:6].contiguous(), *_flat(lim, 5, slice(0, H)), max_iter=2)


@pytest.mark.parametrize("shape,kw", [("2x1_fused", {}), ("6x3_rk4", {}), ("2x1_global", dict(max_iter=5, lq_kernel="thread"))])
def test_a_uniform_binding_equals_shared_bounds(shape, kw):
    """Item 7.  Copies of the shared lb / ub bound per problem, no host vector, against the unbound call with the host
    vector: equal status, Z within 10 tol_step (1 + |Z|inf); on an MI355X the results are bit-identical at all three shapes (Z,
    iterations, multipliers), which is asserted too.  2/1 at H = 355 is the sweep that
    leaves the LDS (solver_step_cases.H_GLOBAL): the bounds are not staged there."""
    s = _setup(shape)
    eng, B, H = s.eng, min(8, s.bmax), s.H
    lim = _limits(s, B)
    for k in NAMES:
        lim[k][:] = lim[k][0]
    lo, hi = _flat(lim, 0, slice(0, H))
    X0, Zi = eng.to_device(s.X0[:B]), eng.to_device(s.start(B))
    opts = {**_solve_kw(), **kw}
    Zs, sts, _, pers, ds = eng.solve(X0, Zi, lo, hi, **opts)
    Zb, stb, _, perb, db = _batch(s, lim, B, Zi, X0, **kw)
    assert torch.equal(sts, stb)
    zs, zb = _np(Zs), _np(Zb)
    assert np.abs(zs - zb).max() <= 10.0 * 1e-8 * (1.0 + np.abs(zs).max())
    same = all(torch.equal(a, b) for a, b in ((Zs, Zb), (pers, perb), (ds["lam"], db["lam"]), (ds["zl"], db["zl"]), (ds["zu"], db["zu"])))
    print(f"[bounds uniform {shape}] status {sts.tolist()}, iterations {pers.tolist()}, |Z - Z_shared| = {np.abs(zs - zb).max():.3e}, "
          f"bit-identical {same}")
    assert same
    assert (np.abs(zb[:, H * s.nx:]) <= hi[H * s.nx:] + 1e-12).all()


def _certify(s, lim, b, Z, d, tol_step):
    """The NumPy certificate of problem b's returned point with its own bounds, and item 5's bound of its r[0]."""
    lo, hi = _flat(lim, b, slice(0, s.H))
    z, lam, zl, zu = _np(Z)[b], _np(d["lam"])[b], _np(d["zl"])[b], _np(d["zu"])[b]
    prob = s.problem(b)
    return cert.residuals(prob, z, s.X0[b], lam[:s.H * s.nx], zl, zu, lo, hi)[0], _stationarity_bound(prob, z, zl, zu, lo, hi, tol_step)


@pytest.mark.parametrize("linesearch", ["loop", "deferred"])
@pytest.mark.parametrize("B", [48, 160])
def test_slots_compaction_and_permutation(B, linesearch):
    """Item 8.  2/1 tanh 2 x 64, H = 20, per-problem control limits: compact 0 and 1 give bit-identical status, iterations, Z
    and duals; permuting the problems (X0, start and bound tensors together) permutes the results bit for bit; every
    converged problem lies inside its own bounds, and six sampled converged problems pass the NumPy certificate with
    their own bounds, all four assertions of item 5 (r[3] == 0, r[1] <= tol_constraint, r[2] <= 10 mu_min,
    r[0] <= 10 |W|inf tol_step (1 + |z|inf); solver defaults: tol_step = tol_constraint = 1e-8, mu_min = 1e-9).  No converged
    share is asserted.  Observed on an MI355X over the 24 sampled problems: r[0] at most 3.8e-10, at most 1.2e-3 of its bound
    (smallest bound 2.7e-7)."""
    s = _setup("2x1_fused")
    eng, H, nx = s.eng, s.H, s.nx
    lim = _limits(s, B, seed=22)
    X0, Zi = eng.to_device(s.X0[:B]), eng.to_device(s.start(B))
    kw = dict(linesearch=linesearch, max_iter=120)
    a = _batch(s, lim, B, Zi, X0, compact=True, **kw)
    b = _batch(s, lim, B, Zi, X0, compact=False, **kw)

    def equal(p, q, idx=None):
        pairs = ((p[0], q[0]), (p[1], q[1]), (p[3], q[3]), (p[4]["lam"], q[4]["lam"]), (p[4]["zl"], q[4]["zl"]), (p[4]["zu"], q[4]["zu"]))
        return all(torch.equal(x if idx is None else x[idx], y) for x, y in pairs)

    assert equal(a, b), "compact = 0 / 1 differ"
    perm = np.random.default_rng(5).permutation(B)
    pt = torch.as_tensor(perm, device=X0.device)
    c = _batch(s, {k: v[perm] for k, v in lim.items()}, B, Zi[pt].contiguous(), X0[pt].contiguous(), **kw)
    assert equal(a, c, pt), "a permutation of the problems does not permute the results"
    Z, st = _np(a[0]), a[1].cpu().numpy()
    conv = np.flatnonzero(st == 0)
    print(f"[bounds slots B={B} {linesearch}] converged {len(conv)} of {B}, iterations {a[2]}")
    for i in conv:
        lo, hi = _flat(lim, i, slice(0, H))
        assert (Z[i] >= lo).all() and (Z[i] <= hi).all(), i
    for i in conv[:: max(1, len(conv) // 6)][:6]:
        r, r0_bound = _certify(s, lim, i, a[0], a[4], 1e-8)
        print(f"[bounds slots B={B} {linesearch}] b={i}: certificate {r.tolist()}, stationarity bound {r0_bound:.3e}")
        assert r[3] == 0.0 and r[1] <= TOL_CONSTRAINT and r[2] <= 10.0 * MU_MIN_DUALS and r[0] <= r0_bound, (i, r, r0_bound)


def test_permutation_where_the_sweep_leaves_the_lds():
    """Item 8, at H = 355 (2/1, thread per problem, B = 3, max_iter = 5): the kernels read the bounds from the working copy
    in global memory; a permutation of the problems permutes the results bit for bit."""
    s = _setup("2x1_global")
    eng, B = s.eng, 3
    lim = _limits(s, B, seed=23)
    X0, Zi = eng.to_device(s.X0[:B]), eng.to_device(s.start(B))
    kw = dict(max_iter=5, lq_kernel="thread")
    a = _batch(s, lim, B, Zi, X0, **kw)
    perm = np.array([2, 0, 1])
    pt = torch.as_tensor(perm, device=X0.device)
    c = _batch(s, {k: v[perm] for k, v in lim.items()}, B, Zi[pt].contiguous(), X0[pt].contiguous(), **kw)
    for x, y in ((a[0], c[0]), (a[1], c[1]), (a[3], c[3]), (a[4]["lam"], c[4]["lam"]), (a[4]["zl"], c[4]["zl"]), (a[4]["zu"], c[4]["zu"])):
        assert torch.equal(x[pt], y)
    # ... and the limits were read: the controls of every problem lie inside its own
    U = _np(a[0])[:, s.H * s.nx:]
    assert (np.abs(U) <= lim["uub"][:, :, 0] + 1e-12).all()
    assert not torch.equal(a[0][0], a[0][1])


def test_coverage_and_lifetime():
    """Item 9.  A batch larger than the binding is NEMPC_EINVAL for solve, kkt_residual and sensitivity; eval and rollout do
    not read the binding (bit-identical outputs, no refusal); the binding survives nempc_reserve and a rebuilt handle;
    unbinding restores the shared result bit for bit."""
    from pyneuralempc_amd import CallbackEngine
    from pyneuralempc_amd._lib import NempcError
    s = _setup("2x1_fused")
    eng = CallbackEngine(s.net.W, s.net.b, s.H, s.nx, s.nu, integrator=s.integ, DT=s.DT, dtype=torch.float64, device="cuda:0",
                         max_batch=8, activations=s.net.act)
    eng.set_objective(**s.obj)
    B, H = 9, s.H
    lim = _limits(s, B, seed=24)
    X0, Zi = eng.to_device(s.X0[:B]), eng.to_device(s.start(B))
    lo, hi = _flat(_limits(s, 1, seed=25), 0, slice(0, H))
    kw = dict(max_iter=60, return_iterations=True, return_duals=True)
    plain = eng.solve(X0, Zi, lo, hi, **kw)                      # (B > max_batch: reserve)
    ev, ro = {k: v.clone() for k, v in eng.eval(Zi, X0).items()}, eng.rollout(X0).clone()
    eng.bind_bounds(**_dev(eng, lim, 8))
    d = plain[4]
    for call, who in ((lambda: eng.solve(X0, Zi, max_iter=1), "nempc_solve"),
                      (lambda: eng.kkt_residual(plain[0], X0, d["lam"], d["zl"], d["zu"]), "nempc_kkt_residual"),
                      (lambda: eng.sensitivity(plain[0], X0, d["lam"], d["zl"], d["zu"]), "nempc_sensitivity")):
        with pytest.raises(NempcError) as ei:
            call()
        assert ei.value.code == -1 and who in str(ei.value) and "bounds" in str(ei.value)
    ev2 = eng.eval(Zi, X0)
    assert all(torch.equal(ev2[k], ev[k]) for k in ev) and torch.equal(eng.rollout(X0), ro)
    eng.bind_bounds(**_dev(eng, lim))
    first = eng.solve(X0, Zi, **kw)
    assert not torch.equal(first[0], plain[0])
    B2 = 12
    eng.reserve(B2)
    assert eng.max_batch == B2
    again = eng.solve(X0, Zi, **kw)
    eng._create(16)
    rebuilt = eng.solve(X0, Zi, **kw)
    for other in (again, rebuilt):
        for x, y in ((first[0], other[0]), (first[1], other[1]), (first[3], other[3]), (first[4]["zl"], other[4]["zl"])):
            assert torch.equal(x, y)
    eng.bind_bounds()
    assert eng._bounds is None
    back = eng.solve(X0, Zi, lo, hi, **kw)
    for x, y in ((plain[0], back[0]), (plain[1], back[1]), (plain[3], back[3]), (plain[4]["lam"], back[4]["lam"]),
                 (plain[4]["zl"], back[4]["zl"]), (plain[4]["zu"], back[4]["zu"])):
        assert torch.equal(x, y)


def test_solver_refuses_a_binding_on_a_rolling_window_model():
    """Item 9.  nempc_solve with a bounds binding on a rolling_window > 1 handle is NEMPC_EUNSUPPORTED."""
    from pyneuralempc_amd._lib import NempcError
    case = sc.qp_case("roll3_fwd", 10)
    eng = case.engine()
    X0 = case.bind(eng, 4)
    try:
        eng.bind_bounds(uub=eng.to_device(np.full((4, case.H, case.nu), 0.5)))
        with pytest.raises(NempcError) as ei:
            eng.solve(X0, max_iter=2)
        assert ei.value.code == -5 and "rolling" in str(ei.value) and "nempc_bind_bounds" in str(ei.value)
    finally:
        eng.bind_bounds()
    eng.solve(X0, max_iter=2)         # unbound, the rolling solve runs


# --------------------------------------------------------------------------------------------------------------------
# 10. controller
# --------------------------------------------------------------------------------------------------------------------
def _controller(H=20, ulim=1.0):
    import pyneuralempc_amd as nEMPC
    s = _setup("2x1_fused")
    model = nEMPC.model.MLPModel(s.net.W, s.net.b, s.nx, s.nu, device="cuda:0")
    integ = nEMPC.integrator.DiscretIntegrator(model, H)
    obj = nEMPC.objective.QuadraticObjective(device="cuda:0", Q=np.eye(s.nx), R=0.1 * np.eye(s.nu))
    dom = nEMPC.constraints.DomainConstraint(states_constraint=[[-3.0, 3.0]] * s.nx, control_constraint=[[-ulim, ulim]] * s.nu)
    return s, nEMPC.controller.NMPC(integ, obj, [dom], H, 1.0, optimizer=nEMPC.optimizer.DeviceSqp())


def test_the_controller_passes_the_bounds_through():
    """Item 10.  next_batch with (B,H,d) limits equals eng.solve under the same binding; a shared (H,d) value equals the same
    limits written into the DomainConstraint's host vector (item 7's tolerance); closed_loop_batch with a control schedule
    (B, steps+H-1, nu) that tightens halfway keeps every applied control inside the limit of its own row, step k equals a
    next_batch from the same state and warm start with rows k .. k+H-1, and the engine is unbound afterwards."""
    from pyneuralempc_amd.optimizer.base import fused_evaluator
    s, mpc = _controller()
    H, nx, nu, B, steps = s.H, s.nx, s.nu, 5, 4
    X0 = s.X0[:B]
    lim = _limits(s, B, seed=26)
    xs, us, st = mpc.next_batch(X0, ulb=lim["ulb"], uub=lim["uub"], max_iter=150)
    eng = fused_evaluator(mpc.integrator, mpc.objective_func, None).engine
    assert eng._bounds is None
    lb = np.asarray(mpc.domain_constraint.get_lower_bounds(H), dtype=np.float64)
    ub = np.asarray(mpc.domain_constraint.get_upper_bounds(H), dtype=np.float64)
    try:
        eng.bind_bounds(ulb=eng.to_device(lim["ulb"]), uub=eng.to_device(lim["uub"]))
        Z, st2, _ = eng.solve(eng.to_device(X0), None, lb, ub, max_iter=150)
    finally:
        eng.bind_bounds()
    assert np.array_equal(_np(Z), np.concatenate([xs.reshape(B, -1), us.reshape(B, -1)], axis=1)) and (st2.cpu().numpy() == 0).all()
    assert (st == 0).all() and (np.abs(us) <= lim["uub"] + 1e-12).all()
    # one (H,d) value for all problems against the same limits in the host vector
    shared = lim["uub"][0]
    xs1, us1, st1 = mpc.next_batch(X0, ulb=-shared, uub=shared, max_iter=150)
    lb2, ub2 = lb.copy(), ub.copy()
    lb2[H * nx:], ub2[H * nx:] = -shared.ravel(), shared.ravel()
    Z2, st3, _ = eng.solve(eng.to_device(X0), None, lb2, ub2, max_iter=150)
    z1 = np.concatenate([xs1.reshape(B, -1), us1.reshape(B, -1)], axis=1)
    assert (st1 == 0).all() and (st3.cpu().numpy() == 0).all()
    assert np.abs(z1 - _np(Z2)).max() <= 10.0 * 1e-8 * (1.0 + np.abs(z1).max())
    # closed loop: a schedule that tightens halfway
    L = steps + H - 1
    sched = np.broadcast_to(lim["uub"][:, :1], (B, L, nu)).copy()
    sched[:, steps // 2:] *= 0.5
    X, U, S = mpc.closed_loop_batch(X0, steps, ulb=-sched, uub=sched, max_iter=150)
    assert eng._bounds is None
    print(f"[bounds controller] closed loop status per step {S.tolist()}")
    assert (np.abs(U) <= sched[:, :steps] + 1e-12).all()      # (an unconverged iterate is interior too)
    assert (np.abs(U[:, steps // 2:]) <= 0.5 * lim["uub"][:, :1] + 1e-12).all()
    # every step again through next_batch: the same state, the same warm start, rows k .. k+H-1 of the schedule
    Zi = None
    for k in range(steps):
        opts = dict(max_iter=150) if k == 0 else dict(max_iter=150, mu_init=1e-4)
        _, uk, sk = mpc.next_batch(X[:, k], init_z=Zi, ulb=-sched[:, k:k + H], uub=sched[:, k:k + H], **opts)
        assert np.array_equal(sk, S[k]) and np.array_equal(uk[:, 0], U[:, k]), k
        Uk = eng.to_device(uk)
        Zi = eng.rollout(eng.to_device(X[:, k + 1]), U=torch.cat([Uk[:, 1:], Uk[:, -1:]], dim=1)).clone()
