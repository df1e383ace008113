"""GPU: the linear stage inequality rows of the batched solver (nempc_bind_stage_rows; csrc/solver_rows_impl.h, the AUG_ROWS
branches of StageAug<T> in csrc/solver_aug.h) against dense float64 references in the caller's variables
(tests/rows_reference.py, shapes and data in tests/rows_cases.py, both checked on the CPU by tests/test_stage_rows_cpu.py).

With C = [Cx | Cu] the bound solve minimises f(z) inside rlo_t <= Cx x_t + Cu u_t <= rhi_t, x_t / u_t row t of the state / control
block of z.  The solver runs it stage-wise in s = [x ; y], y the row values, whose variable bounds are the limits.
"""
import numpy as np
import pytest
import torch

import rows_cases as wc
import rows_reference as wr
import solver_step_cases as sc

pytestmark = pytest.mark.gpu

EUNSUPPORTED, EINVAL = -5, -1
TOL_C = 1e-8


def _solve(eng, X0, Zi, **kw):
    Z, st, it, per = eng.solve(X0, Zi, reg=sc.REG, return_iterations=True, **kw)
    return Z.cpu().double().numpy(), st.cpu().numpy(), it, per.cpu().numpy()


@pytest.mark.parametrize("name,H", wc.QP_CASES)
def test_a_binding_with_nothing_in_effect_takes_the_plain_newton_step(name, H):
    """Linear networks, no bounds, mixed rows with infinite limits, non-symmetric Q, R, QT and per-stage xref, uref, cx, cu: the
    problem is the plain equality-constrained convex QP, solved over the augmented stages.  After max_iter = 1 the iterate is
    z0 + dz of kkt.newton_step for the plain QP; a full solve ends there too with status 0 and every problem converges by
    iteration 3.  B in {1, 3, 16}, every lq_kernel the row names; the LQ plan is held against the size formula at the
    AUGMENTED stage (3/1 for the 2/1 rows, 8/3 for 6/3).  Tolerance: solver_step_cases.step_tolerance of what a NumPy Riccati
    sweep over the augmented stages in the handle's precision loses against the dense solve.

    Observed on an MI355X (LQ plans per requested kernel in the row's order; largest error over tolerance, one step / full
    solve; convergence iterations):
      2x1_discret H=1   thread_lds wave_lds wave_lds   0.000 / 0.000   {2}     (tolerances 1.2e-12 .. 1.8e-12)
      2x1_discret H=2   thread_lds wave_lds wave_lds   0.000 / 0.000   {2}     (1.5e-12 .. 2.1e-12)
      2x1_discret H=6   thread_lds wave_lds wave_lds   0.001 / 0.001   {2}     (2.3e-12 .. 3.1e-12)
      6x3_rk4     H=4   thread_lds wave_lds            0.001 / 0.001   {2}     (1.4e-12 .. 1.7e-12)
      2x1_fp32    H=6   thread_lds wave_lds            0.240 / 0.240   {2}     (6.1e-07 .. 2.5e-06)
    (handle variant mfma, rows rows_coop_kernel, blocks rowhess_coop_kernel on every row)"""
    case = wc.qp_case(name, H)
    ref = wc.qp_reference(name, H)
    eng = case.engine()
    bad, plans, its = [], [], set()
    worst1 = worstf = 0.0
    for B in wc.QP_BATCHES:
        X0 = case.bind(eng, B)
        eng.bind_rows(case.C)
        for k in case.kernels:
            Z1, _, _, _ = _solve(eng, X0, None, max_iter=1, lq_kernel=k)
            want = wc.augmented_plan(case, k)
            if B == wc.QP_BATCHES[0]:
                plans.append(eng.last_lq_kernel)
            if eng.last_lq_kernel != want:
                bad.append(f"{k} B={B}: LQ plan {eng.last_lq_kernel}, the size formula says {want} at the augmented stage")
            Zf, st, _, per = _solve(eng, X0, None, max_iter=30, lq_kernel=k)
            its.update(per.tolist())
            if not (st == 0).all() or per.max() > 3 or per.min() < 1:
                bad.append(f"{k} B={B}: status {st.tolist()} convergence iterations {per.tolist()}")
            for b in range(B):
                z0, dz, tol, _ = ref[b]
                e1, ef = np.abs(Z1[b] - (z0 + dz)).max(), np.abs(Zf[b] - (z0 + dz)).max()
                worst1, worstf = max(worst1, e1 / tol), max(worstf, ef / tol)
                if e1 > tol:
                    bad.append(f"{k} B={B} b={b}: one step |Z - (z0 + dz)| = {e1:.3e} > {tol:.3e} (ratio {e1 / tol:.2f})")
                if ef > tol:
                    bad.append(f"{k} B={B} b={b}: full solve |Z - (z0 + dz)| = {ef:.3e} > {tol:.3e} (ratio {ef / tol:.2f})")
    print(f"[rows qp {name} H={H}] variant {eng.kernel_variant}, rows {eng.last_row_kernel}, blocks {eng.last_hess_kernel}; plans "
          f"{plans}; error / tolerance: one step {worst1:.3f}, full solve {worstf:.3f}; convergence iterations {sorted(its)}; "
          f"tolerances {min(r[2] for r in ref):.1e} .. {max(r[2] for r in ref):.1e}")
    assert not bad, "\n".join(bad)


def _rows_inside(prob, z, C, rlo, rhi, tol_c=TOL_C):
    """every row of the point inside its limits within tol_constraint (1 + |Cx row|_1); -> the largest excess over a limit"""
    rv = wr.row_values(prob, z, C)
    slack = wr.row_tolerance(C, prob.nx, tol_c)
    lo, hi = (np.broadcast_to(np.asarray(v, dtype=np.float64), rv.shape) for v in (rlo, rhi))
    assert (rv >= lo - slack).all() and (rv <= hi + slack).all(), (float((lo - rv).max()), float((rv - hi).max()), slack)
    return float(max((lo - rv).max(), (rv - hi).max()))


@pytest.mark.parametrize("barrier", ["primal-dual", "primal"])
@pytest.mark.parametrize("name", list(wc.LIMIT_ROWS))
def test_limits_bind_where_the_reference_says(name, barrier):
    """Linear networks, 2/1 at H = 8 with one mixed row and 6/3 RK4 at H = 4 with one state-only and one mixed row under per_stage
    limits, bounds on u, B = 4: the converged iterate against the exact active-set solution of the inequality-constrained QP
    (rows_reference.qp_solution).  In every problem the reference has at least one row active and at least one control on
    a bound (asserted here and, with the KKT conditions of the reference, in tests/test_stage_rows_cpu.py).  Tolerance, the
    rule of test_interior_point_ends_at_the_solution_of_the_bounded_qp: 10 (mu_min / nu_min + tol_step (1 + |z*|inf)) with
    nu_min the reference's smallest active multiplier (bounds and rows).  Every returned row lies inside its limits within
    tol_constraint (1 + |Cx row|_1), every z inside lb, ub.

    Observed on an MI355X (active bounds / active rows per problem; largest error over tolerance; iterations):
      2x1_h8  primal-dual  6/1 7/1 7/1 6/1   0.068   16 .. 20        primal  0.072   21 .. 26
      6x3_h4  primal-dual  5/3 4/4 3/4 7/4   0.606   18 .. 27        primal  0.604   26 .. 43"""
    mu_min, tol_step = 1e-9, 1e-8
    case, lb, ub, rlo, rhi = wc.limit_case(name)
    ref = wc.limit_reference(name)
    eng = case.engine()
    X0 = case.bind(eng, case.B)
    eng.bind_rows(case.C, rlo, rhi)
    Z, st, it, per = _solve(eng, X0, None, lb=lb, ub=ub, max_iter=400, barrier=barrier, mu_min=mu_min, tol_step=tol_step,
                            tol_constraint=TOL_C)
    assert (st == 0).all(), (st.tolist(), it)
    H, nx = case.H, case.nx
    n_rows = n_ctrl = 0
    for b, (zs, _, nlo, nhi, qlo, qhi) in enumerate(ref):
        act = np.concatenate([v[v > 0] for v in (nlo, nhi, qlo, qhi)])
        assert ((qlo + qhi) > 0).sum() >= 1 and ((nlo + nhi)[H * nx:] > 0).sum() >= 1
        n_rows += int(((qlo + qhi) > 0).sum())
        n_ctrl += int(((nlo + nhi)[H * nx:] > 0).sum())
        tol = 10.0 * (mu_min / act.min() + tol_step * (1.0 + np.abs(zs).max()))
        e = np.abs(Z[b] - zs).max()
        print(f"[rows limits {name} {barrier}] b={b}: {int(((nlo + nhi) > 0).sum())} active bounds, {int(((qlo + qhi) > 0).sum())} active "
              f"rows, nu_min {act.min():.3e}, |Z - z*| = {e:.3e}, tolerance {tol:.3e} (ratio {e / tol:.3f}), iterations {per[b]}")
        assert e <= tol, (b, e, tol)
        _rows_inside(case.problem(b), Z[b], case.C, rlo, rhi)
        assert (Z[b] >= lb - 1e-12).all() and (Z[b] <= ub + 1e-12).all()
    assert n_rows >= case.B and n_ctrl >= case.B


WIDE = 5.0
# what: (column of C = variable of the stage, L, range of X0).  The state limit needs starts it can be kept from: the
# network moves a state by about a tenth of its output per step, so a start outside +-L makes the problem infeasible (X0 in
# +-0.5 with x_0 held to +-0.3: 4 of 16 problems end with status 1 on both paths); X0 in +-0.1 with L = 0.1 is feasible for all.
SELECTOR_LIMITS = {"state": (0, 0.10, 0.1), "control": (2, 0.25, 0.5)}


@pytest.mark.parametrize("what", list(SELECTOR_LIMITS))
def test_a_selector_row_is_a_bound(what):
    """2/1, 2 x 64 tanh, H = 8, B = 16: a row C = e_j with limits [-L, L], every variable bounded at +-5 (wide), against the plain
    solve with that variable bounded at +-L (the existing path).  L is such that the limit is active -- a multiplier of the
    plain solve above its slack -- in at least half the problems (asserted).  The statuses are equal and
    |Z_rows - Z_bound|inf <= 10 (mu_min / nu_min + tol_step (1 + |Z|inf)), nu_min the smallest active multiplier of the plain
    solve's returned zl / zu; problems where it is under 1e-3 are skipped, at most a quarter of the batch.  Iteration counts
    are printed, not asserted.

    Observed on an MI355X (error over tolerance below 0.0005 on both: the two paths end within 1e-10 of each other):
      state   x_0 at +-0.10, X0 in +-0.1: active in  9 of 16 problems, 0 skipped, error / tolerance 0.000; iterations bound 14 .. 23, rows 14 .. 23
      control u_0 at +-0.25, X0 in +-0.5: active in 14 of 16 problems, 0 skipped, error / tolerance 0.000; iterations bound 14 .. 19, rows 14 .. 19"""
    B, mu_min, tol_step = 16, 1e-9, 1e-8
    col, L, x0_range = SELECTOR_LIMITS[what]
    case = wc.nl_case(B, x0_range=x0_range)
    eng = case.engine()
    X0 = case.bind(eng, B)
    H, nx, nu = case.H, case.nx, case.nu
    lbw, ubw = np.full(case.n, -WIDE), np.full(case.n, WIDE)
    lbb, ubb = lbw.copy(), ubw.copy()
    idx = np.arange(H) * nx + col if col < nx else H * nx + np.arange(H) * nu + (col - nx)
    lbb[idx], ubb[idx] = -L, L
    kw = dict(reg=sc.REG, max_iter=200, mu_min=mu_min, tol_step=tol_step, tol_constraint=TOL_C, return_iterations=True)
    Zb, stb, _, perb, duals = eng.solve(X0, None, lbb, ubb, return_duals=True, **kw)
    C = np.zeros((1, nx + nu))
    C[0, col] = 1.0
    eng.bind_rows(C, [-L], [L])
    Zr, str_, _, perr = eng.solve(X0, None, lbw, ubw, **kw)
    eng.bind_rows()
    Zb, Zr = Zb.cpu().numpy(), Zr.cpu().numpy()
    zl, zu = duals["zl"].cpu().numpy(), duals["zu"].cpu().numpy()
    assert np.array_equal(stb.cpu().numpy(), str_.cpu().numpy())
    assert (stb.cpu().numpy() == 0).all()             # (the comparison below is between two converged iterates)
    n_act = skipped = 0
    worst = 0.0
    for b in range(B):
        active = np.concatenate([zl[b][zl[b] > Zb[b] - lbb], zu[b][zu[b] > ubb - Zb[b]]])
        on_limit = bool((zl[b][idx] > (Zb[b] - lbb)[idx]).any() or (zu[b][idx] > (ubb - Zb[b])[idx]).any())
        n_act += on_limit
        nu_min = active.min() if active.size else np.inf
        if nu_min < 1e-3:
            skipped += 1
            continue
        tol = 10.0 * (mu_min / nu_min + tol_step * (1.0 + np.abs(Zb[b]).max()))
        e = np.abs(Zr[b] - Zb[b]).max()
        worst = max(worst, e / tol)
        assert e <= tol, (b, e, tol, nu_min)
        assert np.abs(Zr[b][idx]).max() <= L + TOL_C
    print(f"[rows selector {what}] L = {L}: active in {n_act} of {B} problems, {skipped} skipped, largest error over tolerance {worst:.3f}; "
          f"iterations bound {perb.min().item()} .. {perb.max().item()}, rows {perr.min().item()} .. {perr.max().item()}")
    assert n_act >= B // 2
    assert skipped <= B // 4


MIXED_ROW = np.array([[1.0, -0.5, 2.0]])
MIXED_LIMIT = 0.25


def test_a_nonlinear_solve_under_an_active_row_is_stationary_for_the_callers_problem():
    """The same network, B = 16, no bounds on z, the mixed row x_t[0] - 0.5 x_t[1] + 2 u_t <= 0.25.  The plain solution's
    largest row value is at least twice the limit (asserted), and the row ends up active in at least half the problems.  At
    the returned point the oracle computes: the defects (<= tol_constraint); the rows (inside the limit within tol_constraint
    (1 + |Cx row|_1)); the reduced gradient |Zn' grad f|inf over the null space of the defect Jacobian stacked with the active
    rows -- at most ten times the same quantity at the PLAIN solve of the same problems, the bar of
    test_a_nonlinear_solve_with_a_penalty_is_stationary_for_the_callers_problem (the unbounded solve, which runs no barrier)
    --; and the least-squares multipliers of the active rows, which have the right sign down to minus that bar.

    mu_min = 1e-11, and a row counts as active within sqrt(mu_min) of its limit.  An interior-point solution keeps the barrier
    multiplier mu_min / slack on every INACTIVE row, and that is what the reduced gradient over the active set's null space
    still sees: |C row| mu_min / slack.  The closest inactive row here has a slack of 1.8e-2 (problem 14), so the solver's default
    mu_min = 1e-9 leaves 1.1e-7 there by construction -- measured, against a bar of 8.6e-8 -- and 1e-11 leaves 1.4e-9.

    Observed on an MI355X: plain solve largest row value 2.265 (limit 0.25), largest reduced gradient 8.6e-09; rows solve
    1.4e-09 (bar 8.6e-08), defects 7.9e-14, smallest multiplier 6.7e-04, the row active in 11 of 16 problems (at all 8 steps
    in 7 of them), 13 .. 24 iterations.  Recorded in profiles/stage_rows.txt."""
    B, mu_min = 16, 1e-11
    case = wc.nl_case(B)
    eng = case.engine()
    X0 = case.bind(eng, B)
    Zp, stp, _, _ = _solve(eng, X0, None, max_iter=200, tol_constraint=TOL_C)
    eng.bind_rows(MIXED_ROW, None, [MIXED_LIMIT])
    Z, st, _, per = _solve(eng, X0, None, max_iter=200, tol_constraint=TOL_C, mu_min=mu_min)
    assert (stp == 0).all() and (st == 0).all(), (stp.tolist(), st.tolist())
    free = max(float(wr.row_values(case.problem(b), Zp[b], MIXED_ROW).max()) for b in range(B))
    assert free >= 2.0 * MIXED_LIMIT, free
    plain = [wr.stationarity(case.problem(b), Zp[b], case.X0[b]) for b in range(B)]
    rows = [wr.stationarity(case.problem(b), Z[b], case.X0[b], MIXED_ROW, -np.inf, MIXED_LIMIT, act_tol=np.sqrt(mu_min)) for b in range(B)]
    bar = 10.0 * max(r["red"] for r in plain)
    print(f"[rows nonlinear] plain solve: largest row value {free:.3f} (limit {MIXED_LIMIT}), reduced gradient max {max(r['red'] for r in plain):.3e}; "
          f"rows solve: reduced gradient max {max(r['red'] for r in rows):.3e} (bar {bar:.3e}), defects {max(r['defect'] for r in rows):.3e}, "
          f"smallest multiplier {min(r['mult'] for r in rows):.3e}, active rows {[r['n_act'] for r in rows]}; iterations {per.tolist()}")
    assert max(r["defect"] for r in rows) <= TOL_C
    for b in range(B):
        _rows_inside(case.problem(b), Z[b], MIXED_ROW, -np.inf, MIXED_LIMIT)
    assert sum(r["n_act"] >= 1 for r in rows) >= B // 2       # (the row is active in at least half the problems)
    assert max(r["red"] for r in rows) <= bar
    assert min(r["mult"] for r in rows) >= -bar


BUDGET = 0.4


def test_closed_loop_under_a_shared_budget():
    """closed_loop_batch, 2 states, 2 controls, 2 x 64 tanh, H = 8, B = 8, 6 steps, LinearStageConstraint([[0,0,1,1]], -inf, P):
    a shared actuator budget u_1 + u_2 <= P.  Q = I, R = 0.5 I and a control reference of 0.8 for each actuator -- both want
    twice the whole budget --, X0 in +-0.1, controls bounded at +-1.  Without the row the largest applied u_1 + u_2 is at least
    2 P (asserted: otherwise the budget would show nothing); with it every applied sum is <= P + tol_constraint and every
    solve converges.  The engine is left without a binding.

    Observed on an MI355X: largest applied sum without the row 1.6238, with it 0.39999999 (P = 0.4); all statuses 0 in both
    runs, 12 then 7 iterations per step of the constrained run."""
    import pyneuralempc_amd as nEMPC
    from pyneuralempc_amd.optimizer.base import fused_evaluator
    B, H, steps = 8, wc.NL_H, 6
    case = wc.nl_case(B, nu=2)
    model = nEMPC.model.MLPModel(case.net.W, case.net.b, 2, 2, device="cuda:0")
    integ = nEMPC.integrator.DiscretIntegrator(model, H)
    obj = nEMPC.objective.QuadraticObjective(Q=np.eye(2), R=0.5 * np.eye(2), uref=np.tile([0.8, 0.8], (H, 1)), device="cuda:0")
    dom = nEMPC.constraints.DomainConstraint(states_constraint=[[-5.0, 5.0]] * 2, control_constraint=[[-1.0, 1.0]] * 2)
    row = nEMPC.constraints.LinearStageConstraint([[0.0, 0.0, 1.0, 1.0]], -np.inf, BUDGET)
    X0 = np.random.default_rng(7).uniform(-0.1, 0.1, size=(B, 2))
    free_mpc = nEMPC.controller.NMPC(integ, obj, [dom], H, 1.0, optimizer=nEMPC.optimizer.DeviceSqp())
    _, U_free, st_free = free_mpc.closed_loop_batch(X0, steps, max_iter=200, tol_constraint=TOL_C)
    mpc = nEMPC.controller.NMPC(integ, obj, [dom, row], H, 1.0, optimizer=nEMPC.optimizer.DeviceSqp())
    _, U, st = mpc.closed_loop_batch(X0, steps, max_iter=200, tol_constraint=TOL_C)
    free, lim = float(U_free.sum(axis=2).max()), float(U.sum(axis=2).max())
    print(f"[rows closed loop] largest applied u_1 + u_2: without the row {free:.4f}, with it {lim:.8f} (P = {BUDGET}); "
          f"converged per step {(st_free == 0).sum(axis=1).tolist()} / {(st == 0).sum(axis=1).tolist()} of {B}; "
          f"iterations {mpc.last_closed_loop_iterations}")
    assert (st_free == 0).all()
    assert free >= 2.0 * BUDGET
    assert (st == 0).all()
    assert lim <= BUDGET + TOL_C
    assert fused_evaluator(integ, obj, None).engine._rows is None


def _refused(code, word, fn, *a, **kw):
    from pyneuralempc_amd._lib import NempcError
    with pytest.raises(NempcError) as ei:
        fn(*a, **kw)
    assert ei.value.code == code and word in str(ei.value), (ei.value.code, str(ei.value))


def test_refusals_and_the_way_back():
    """Each refusal returns its code and leaves a nempc_last_error text naming the call, and the handle stays usable; a bound
    binding changes no bit of eval, hess or rollout; a second solve under the same binding equals the first bit for bit;
    after bind_rows() with nothing a plain solve returns the bits it returned before any binding (Z, status, iteration
    counts)."""
    import ctypes
    B = 4
    case = wc.nl_case(B)
    eng = case.engine()
    X0 = case.bind(eng, B)
    lb, ub = np.full(case.n, -WIDE), np.full(case.n, WIDE)
    kw = dict(reg=sc.REG, max_iter=100, return_iterations=True)
    Z0, st0, it0, per0 = eng.solve(X0, None, lb, ub, **kw)
    Z0d, st0d, _, duals = eng.solve(X0, None, lb, ub, reg=sc.REG, max_iter=100, return_duals=True)
    lam = duals["lam"]
    sig = torch.ones(B, dtype=eng.dtype, device=eng.device)
    before = dict(ev={k: v.clone() for k, v in eng.eval(Z0, X0, want=("f", "grad", "g", "jac_tiles")).items()},
                  he=eng.hess(Z0, X0, lam, sig, want=("hvals",))["hvals"].clone(), ro=eng.rollout(X0, Z=Z0.clone()).clone())
    eng.bind_rows(MIXED_ROW, None, [MIXED_LIMIT])
    # eval / hess / rollout ignore the binding
    after = dict(ev=eng.eval(Z0, X0, want=("f", "grad", "g", "jac_tiles")), he=eng.hess(Z0, X0, lam, sig, want=("hvals",))["hvals"],
                 ro=eng.rollout(X0, Z=Z0.clone()))
    assert all(torch.equal(before["ev"][k], after["ev"][k]) for k in before["ev"])
    assert torch.equal(before["he"], after["he"]) and torch.equal(before["ro"], after["ro"])
    # the refusals
    _refused(EUNSUPPORTED, "nempc_solve_duals", eng.solve, X0, None, lb, ub, reg=sc.REG, max_iter=5, return_duals=True)
    _refused(EUNSUPPORTED, "nempc_kkt_residual", eng.kkt_residual, Z0d, X0, lam, duals["zl"], duals["zu"], lb, ub)
    _refused(EUNSUPPORTED, "nempc_sensitivity", eng.sensitivity, Z0d, X0, lam, duals["zl"], duals["zu"], lb, ub)
    _refused(EUNSUPPORTED, "nempc_kkt_solve", eng.kkt_solve, Z0d, X0, lam, duals["zl"], duals["zu"], lb, ub,
             rz=torch.ones(B, case.n, dtype=eng.dtype, device=eng.device))
    ref_x = torch.zeros(B, case.H, case.nx, dtype=eng.dtype, device=eng.device)
    eng.bind_tracking(xref=ref_x)
    _refused(EUNSUPPORTED, "nempc_solve", eng.solve, X0, None, lb, ub, reg=sc.REG, max_iter=5)
    eng.bind_tracking()
    eng.bind_bounds(xub=ref_x + 4.0)
    _refused(EUNSUPPORTED, "nempc_solve", eng.solve, X0, None, lb, ub, reg=sc.REG, max_iter=5)
    eng.bind_bounds()
    eng.bind_rate(u_prev=eng.to_device(np.zeros((B, case.nu))), du_lb=[-0.3], du_ub=[0.3])
    _refused(EUNSUPPORTED, "nempc_solve", eng.solve, X0, None, lb, ub, reg=sc.REG, max_iter=5)
    eng.bind_rate()
    # rlo >= rhi, a NaN and nc < 0 reach the library only past the Python check: ask it directly
    dp = ctypes.POINTER(ctypes.c_double)
    Cc = (ctypes.c_double * 3)(1.0, 0.0, 1.0)
    one, nan = (ctypes.c_double * 1)(0.1), (ctypes.c_double * 1)(float("nan"))
    fn = eng.lib.nempc_bind_stage_rows
    for args in ((1, Cc, one, one, 0), (1, Cc, nan, None, 0), (-1, Cc, None, None, 0), (1, Cc, None, None, 2)):
        assert fn(eng._handle, *args) == EINVAL, args
        assert b"nempc_bind_stage_rows" in eng.lib.nempc_last_error()
    assert eng._rows is not None      # (a refused call leaves the binding as it was)
    # a rolling-window handle refuses the binding
    roll = sc.qp_case("roll3_fwd", 10)
    reng = roll.engine()
    assert reng.lib.nempc_bind_stage_rows(reng._handle, 1, Cc, None, one, 0) == EUNSUPPORTED
    assert b"nempc_bind_stage_rows" in reng.lib.nempc_last_error()
    # two solves under the binding: the same bits; then the way back: the plain solve's bits
    Zr, str_, itr, perr = eng.solve(X0, None, lb, ub, **kw)
    Zr2, str2, itr2, perr2 = eng.solve(X0, None, lb, ub, **kw)
    assert (str_.cpu().numpy() == 0).all() and not torch.equal(Zr, Z0)
    assert torch.equal(Zr, Zr2) and torch.equal(str_, str2) and torch.equal(perr, perr2) and itr == itr2
    eng.bind_rows()
    Z1, st1, it1, per1 = eng.solve(X0, None, lb, ub, **kw)
    assert torch.equal(Z1, Z0) and torch.equal(st1, st0) and torch.equal(per1, per0) and it1 == it0


def test_next_batch_and_device_sqp_honour_the_row():
    """NMPC.next_batch with two LinearStageConstraints (stacked: the mixed row and a state-only one with (H,1) limits) and a
    BoxStateConstraint gives what the engine gives with the same binding and bounds (bit for bit) and leaves no binding
    behind; NMPC.next with DeviceSqp honours the rows; any other Constraint subclass is refused as before."""
    import pyneuralempc_amd as nEMPC
    from pyneuralempc_amd.optimizer.base import fused_evaluator
    B, H = 4, wc.NL_H
    case = wc.nl_case(B)
    model = nEMPC.model.MLPModel(case.net.W, case.net.b, 2, 1, device="cuda:0")
    integ = nEMPC.integrator.DiscretIntegrator(model, H)
    obj = nEMPC.objective.QuadraticObjective(Q=np.eye(2), R=0.01 * np.eye(1), xref=np.tile([0.8, -0.4], (H, 1)), device="cuda:0")
    dom = nEMPC.constraints.DomainConstraint(states_constraint=[[-5.0, 5.0]] * 2, control_constraint=[[-1.0, 1.0]])
    hi2 = 0.5 + 0.05 * np.arange(H)[:, None]
    rows = [nEMPC.constraints.LinearStageConstraint(MIXED_ROW, None, MIXED_LIMIT),
            nEMPC.constraints.LinearStageConstraint([[1.0, 0.0, 0.0]], -hi2, hi2)]
    box = nEMPC.constraints.BoxStateConstraint([-4.0, -3.0], [4.0, 3.0])
    mpc = nEMPC.controller.NMPC(integ, obj, [dom, box] + rows, H, 1.0, optimizer=nEMPC.optimizer.DeviceSqp())
    X0 = case.X0[:B] * 0.2
    xs, us, st = mpc.next_batch(X0, max_iter=200)
    eng = fused_evaluator(integ, obj, None).engine
    assert eng._rows is None and (st == nEMPC.optimizer.Optimizer.SUCCESS).all()

    def inside(x, u):
        return (x[:, 0] - 0.5 * x[:, 1] + 2.0 * u[:, 0]).max() <= MIXED_LIMIT + 2.5 * TOL_C and (np.abs(x[:, 0]) <= hi2[:, 0] + 2 * TOL_C).all()
    assert all(inside(xs[b], us[b]) for b in range(B))
    C, lo, hi = nEMPC.constraints.LinearStageConstraint.stack(rows, H, 3)
    eng.bind_rows(C, lo, hi)
    lb, ub = np.asarray(dom.get_lower_bounds(H), dtype=np.float64), np.asarray(dom.get_upper_bounds(H), dtype=np.float64)
    lb[:H * 2], ub[:H * 2] = np.maximum(lb[:H * 2], np.tile([-4.0, -3.0], H)), np.minimum(ub[:H * 2], np.tile([4.0, 3.0], H))
    Z, _, _ = eng.solve(eng.to_device(X0), None, lb, ub, max_iter=200)
    eng.bind_rows()
    assert np.array_equal(Z.cpu().numpy()[:, H * 2:].reshape(B, H, 1), us) and np.array_equal(Z.cpu().numpy()[:, :H * 2].reshape(B, H, 2), xs)
    x1, u1 = mpc.next(X0[0])
    assert u1 is not None and inside(x1, u1) and eng._rows is None
    xf, uf = nEMPC.controller.NMPC(integ, obj, [dom], H, 1.0, optimizer=nEMPC.optimizer.DeviceSqp()).next(X0[0])
    assert not inside(xf, uf)                                   # (without the rows the same problem leaves them)

    class Other(nEMPC.constraints.Constraint):
        def get_dim(self, H):
            return 0
    with pytest.raises(NotImplementedError):
        nEMPC.controller.NMPC(integ, obj, [dom, rows[0], Other()], H, 1.0, optimizer=nEMPC.optimizer.DeviceSqp()).next_batch(X0)
