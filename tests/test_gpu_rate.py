"""GPU: the input-rate penalty and rate limits of the batched solver (nempc_bind_rate; csrc/solver_rate_impl.h, the AUG_RATE
branches of Solve<T> in csrc/solver.hip) against dense float64 references in the caller's variables (tests/rate_reference.py,
shapes and data in tests/rate_cases.py, both checked on the CPU by tests/test_rate_cpu.py).

With du_t = u_t - u_{t-1}, u_{-1} = u_prev, the bound solve minimises f(z) + sum_t du_t' S du_t inside dlo <= du_t <= dhi.  The
solver runs it stage-wise in s = [x ; u] with du as the stage control; its Levenberg term sits on du, so the reference's is
reg D'D on the controls.
"""
import numpy as np
import pytest
import torch

import rate_cases as rc
import rate_reference as rr
import solver_step_cases as sc

pytestmark = pytest.mark.gpu

EUNSUPPORTED, EINVAL = -5, -1


def _solve(eng, X0, Zi, **kw):
    Z, st, it, per = eng.solve(X0, Zi, reg=sc.REG, return_iterations=True, **kw)
    return Z.cpu().double().numpy(), st.cpu().numpy(), it, per.cpu().numpy()


@pytest.mark.parametrize("name,H", rc.QP_CASES)
def test_one_newton_step_solves_the_rate_qp(name, H):
    """Linear networks, no bounds, no limits, S not symmetric, u_prev random per problem, non-symmetric Q, R, QT and per-stage
    xref, uref, cx, cu: the rate problem is an equality-constrained convex QP and the first step from the cold start is exact.
    After max_iter = 1 the iterate is z0 + dz_ref (rate_reference.newton_step, dense, in the caller's variables); a full solve
    ends there too with status 0 and every problem converges by iteration 3.  B in {1, 3, 16}, every lq_kernel the row names;
    the LQ plan is held against the size formula at the AUGMENTED stage (3/1 for the 2/1 rows, 9/3 for 6/3).  Tolerance:
    solver_step_cases.step_tolerance of what a NumPy Riccati sweep over the augmented stages in the handle's precision loses
    against the dense solve (largest over the problems: 2x1_discret H=1 1.8e-12, H=2 2.1e-12, H=6 3.1e-12; 6x3_rk4 1.6e-12;
    2x1_fp32 2.6e-06).

    Observed on an MI355X (LQ plans per requested kernel in the row's order; largest error over tolerance, one step / full
    solve; convergence iterations):
      2x1_discret H=1   thread_lds wave_lds wave_lds   0.000 / 0.000   {2}
      2x1_discret H=2   thread_lds wave_lds wave_lds   0.000 / 0.000   {2}
      2x1_discret H=6   thread_lds wave_lds wave_lds   0.002 / 0.002   {2}
      6x3_rk4     H=4   thread_lds wave_lds            0.002 / 0.002   {2}
      2x1_fp32    H=6   thread_lds wave_lds            0.231 / 0.231   {2}
    (handle variant mfma, rows rows_coop_kernel, blocks rowhess_coop_kernel on every row)"""
    case = rc.qp_case(name, H)
    ref = rc.qp_reference(name, H)
    eng = case.engine()
    bad, plans, its = [], [], set()
    worst1 = worstf = 0.0
    for B in rc.QP_BATCHES:
        X0 = case.bind(eng, B)
        eng.bind_rate(u_prev=eng.to_device(case.u_prev[:B]), S=case.S)
        for k in case.kernels:
            Z1, _, _, _ = _solve(eng, X0, None, max_iter=1, lq_kernel=k)
            want = rc.augmented_plan(case, k)
            if B == rc.QP_BATCHES[0]:
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
    print(f"[rate qp {name} H={H}] variant {eng.kernel_variant}, rows {eng.last_row_kernel}, blocks {eng.last_hess_kernel}; plans "
          f"{plans}; error / tolerance: one step {worst1:.3f}, full solve {worstf:.3f}; convergence iterations {sorted(its)}")
    assert not bad, "\n".join(bad)


NL_BOUND = 5.0


def _nl_engine(B):
    case = rc.nl_case(B)
    eng = case.engine()
    return case, eng, case.bind(eng, B)


def test_a_binding_with_nothing_in_effect_solves_the_plain_problem():
    """2/1, 2 x 64 tanh, H = 8, B = 16, states and controls bounded at +-5 (the barrier and its schedule run; no bound is
    active, asserted: a restart at mu_init would otherwise have to rebuild an active bound's multiplier, which is not a
    property of this binding).  The plain solve first; then S = 0, no limits, an arbitrary u_prev, from the plain solution
    with mu_init = 1e-6: status 0, at most 3 iterations, |Z - Z_plain|inf <= 10 tol_step (1 + |Z|inf) -- the stopping test
    allows a step of tol_step (1 + |z|), the factor 10 is for the three iterations and the different LQ path.

    Observed on an MI355X (LQ plan wave_lds): every problem converges at iteration 2 -- the first iteration finds the
    sub-problem of mu = 1e-6 converged and lowers mu to its floor, the second finds a step under the stopping test and takes
    none --, so |Z - Z_plain| = 0 against a bound of 2.1e-07: the plain solution is a stationary point of the augmented problem
    to the solver's own test."""
    B, tol_step = 16, 1e-8
    case, eng, X0 = _nl_engine(B)
    lb, ub = np.full(case.n, -NL_BOUND), np.full(case.n, NL_BOUND)
    Zp_dev, stp, _ = eng.solve(X0, None, lb, ub, reg=sc.REG, max_iter=80, tol_step=tol_step)
    Zp = Zp_dev.cpu().numpy()
    assert (stp.cpu().numpy() == 0).all()
    assert np.abs(Zp).max() <= NL_BOUND - 1.0
    eng.bind_rate(u_prev=eng.to_device(case.u_prev[:B]), S=np.zeros((case.nu, case.nu)))
    Z, st, it, per = _solve(eng, X0, Zp_dev, lb=lb, ub=ub, max_iter=80, tol_step=tol_step, mu_init=1e-6)
    e, bound = np.abs(Z - Zp).max(), 10.0 * tol_step * (1.0 + np.abs(Z).max())
    print(f"[rate none] iterations {per.tolist()} (launch budget used {it}), |Z - Z_plain| = {e:.3e}, bound {bound:.3e}, lq {eng.last_lq_kernel}")
    assert (st == 0).all() and per.max() <= 3, (st.tolist(), per.tolist())
    assert e <= bound


def test_a_nonlinear_solve_with_a_penalty_is_stationary_for_the_callers_problem():
    """The same network, S with a positive definite symmetric part, no bounds, B = 16.  At the returned point the oracle
    computes the defects and the reduced gradient |Zn' (grad f + rate gradient)|inf (Zn: orthonormal null-space basis of the
    defect Jacobian).  The bar is ten times the largest value of the same quantity (without the rate gradient) at the PLAIN
    solve of the same problems, the existing path -- the augmented stage is wider and the path differs; defects <=
    tol_constraint.

    Observed on an MI355X: plain solve largest reduced gradient 8.609e-09, rate solve 2.699e-09 (bar 8.609e-08); defects
    plain 9.0e-10, rate 3.1e-10; 4 .. 5 iterations; the penalty moves the solution by 0.48 (so it is a different problem that
    is stationary).  Recorded in profiles/rate_penalty.txt."""
    B, tol_c = 16, 1e-8
    case, eng, X0 = _nl_engine(B)
    Zp, stp, _, _ = _solve(eng, X0, None, max_iter=80, tol_constraint=tol_c)
    eng.bind_rate(u_prev=eng.to_device(case.u_prev[:B]), S=case.S)
    Z, st, _, per = _solve(eng, X0, None, max_iter=80, tol_constraint=tol_c)
    assert (stp == 0).all() and (st == 0).all(), (stp.tolist(), st.tolist())
    plain = [rr.reduced_gradient(case.problem(b), Zp[b], case.X0[b]) for b in range(B)]
    rate = [rr.reduced_gradient(case.problem(b), Z[b], case.X0[b], case.S, case.u_prev[b]) for b in range(B)]
    bar = 10.0 * max(r for r, _ in plain)
    print(f"[rate penalty] reduced gradient: plain solve max {max(r for r, _ in plain):.3e}, rate solve max {max(r for r, _ in rate):.3e} "
          f"(bar {bar:.3e}); defects plain {max(d for _, d in plain):.3e}, rate {max(d for _, d in rate):.3e}; iterations {per.tolist()}; "
          f"|Z - Z_plain| = {np.abs(Z - Zp).max():.3e}")
    assert max(d for _, d in rate) <= tol_c
    assert max(r for r, _ in rate) <= bar
    assert np.abs(Z - Zp).max() > 1e-3          # (the penalty is in effect)


@pytest.mark.parametrize("barrier", ["primal-dual", "primal"])
@pytest.mark.parametrize("name", list(rc.LIMIT_ROWS))
def test_limits_bind_where_the_reference_says(name, barrier):
    """Linear networks, 2/1 at H = 8 and 6/3 RK4 at H = 4, bounds on u, limits on du, B = 4: the converged iterate against the
    exact active-set solution of the inequality-constrained QP (rate_reference.qp_solution).  In every problem the
    reference has the limit on du_0 (against u_prev) active and at least one control on a bound (asserted here and, with the
    KKT conditions of the reference, in tests/test_rate_cpu.py).  Tolerance, the rule of
    test_interior_point_ends_at_the_solution_of_the_bounded_qp: 10 (mu_min / nu_min + tol_step (1 + |z*|inf)) with nu_min the
    reference's smallest active multiplier (bounds and limits).  Every returned du lies inside its limits.

    Observed on an MI355X (active bounds / active limits per problem; largest error over tolerance; iterations):
      2x1_h8  primal-dual  6/1 3/4 4/4 4/3   0.220   18 .. 20        primal  0.219   26 .. 28
      6x3_h4  primal-dual  4/2 2/2 7/2 4/2   0.764   19 .. 24        primal  0.759   27 .. 34"""
    mu_min, tol_step = 1e-9, 1e-8
    case, lb, ub, dlo, dhi = rc.limit_case(name)
    ref = rc.limit_reference(name)
    eng = case.engine()
    X0 = case.bind(eng, case.B)
    eng.bind_rate(u_prev=eng.to_device(case.u_prev), S=case.S, du_lb=dlo, du_ub=dhi)
    Z, st, it, per = _solve(eng, X0, None, lb=lb, ub=ub, max_iter=400, barrier=barrier, mu_min=mu_min, tol_step=tol_step)
    assert (st == 0).all(), (st.tolist(), it)
    H, nx, nu = case.H, case.nx, case.nu
    n_rate = n_ctrl = 0
    for b, (zs, _, nlo, nhi, rlo, rhi) in enumerate(ref):
        act = np.concatenate([v[v > 0] for v in (nlo, nhi, rlo, rhi)])
        assert (rlo + rhi)[:nu].max() > 0 and ((rlo + rhi) > 0).sum() >= 1 and ((nlo + nhi)[H * nx:] > 0).sum() >= 1
        n_rate += int(((rlo + rhi) > 0).sum())
        n_ctrl += int(((nlo + nhi)[H * nx:] > 0).sum())
        tol = 10.0 * (mu_min / act.min() + tol_step * (1.0 + np.abs(zs).max()))
        e = np.abs(Z[b] - zs).max()
        print(f"[rate limits {name} {barrier}] b={b}: {int(((nlo + nhi) > 0).sum())} active bounds, {int(((rlo + rhi) > 0).sum())} active "
              f"limits, nu_min {act.min():.3e}, |Z - z*| = {e:.3e}, tolerance {tol:.3e} (ratio {e / tol:.3f}), iterations {per[b]}")
        assert e <= tol, (b, e, tol)
        dv = rr.moves(case.problem(b), Z[b], case.u_prev[b])
        assert (dv >= dlo).all() and (dv <= dhi).all(), (b, dv.min(), dv.max())
        assert (Z[b] >= lb - 1e-12).all() and (Z[b] <= ub + 1e-12).all()
    assert n_rate >= case.B and n_ctrl >= case.B


def test_closed_loop_moves_stay_inside_the_limits():
    """closed_loop_batch, 2/1, 2 x 64 tanh, H = 8, B = 8, 6 steps; the objective's reference is a set point (0.8, -0.4) away
    from X0 in +-0.1 with R = 0.01 I -- a step change at time 0 --, controls bounded at +-1, u_prev = 0.  Without limits the
    largest applied move, step 0 against u_prev included, is at least twice the limit used next (asserted: otherwise the
    limits would show nothing); with du limited to +-0.05 every applied move, step 0 included, is within the limit plus
    tol_constraint, and every solve converges.

    Observed on an MI355X: largest move without limits 0.8296, with limits 0.05000000; all statuses 0 in both runs, 16 .. 22
    iterations per step of the limited run."""
    import pyneuralempc_amd as nEMPC
    B, H, steps, d, tol_c = 8, rc.NL_H, 6, 0.05, 1e-8
    case = rc.nl_case(B)
    model = nEMPC.model.MLPModel(case.net.W, case.net.b, 2, 1, device="cuda:0")
    integ = nEMPC.integrator.DiscretIntegrator(model, H)
    obj = nEMPC.objective.QuadraticObjective(Q=np.eye(2), R=0.01 * np.eye(1), xref=np.tile([0.8, -0.4], (H, 1)), device="cuda:0")
    dom = nEMPC.constraints.DomainConstraint(states_constraint=[[-5.0, 5.0]] * 2, control_constraint=[[-1.0, 1.0]])
    mpc = nEMPC.controller.NMPC(integ, obj, [dom], H, 1.0, optimizer=nEMPC.optimizer.DeviceSqp())
    X0 = np.random.default_rng(7).uniform(-0.1, 0.1, size=(B, 2))
    up = np.zeros((B, 1))

    def largest_move(U):
        return float(np.abs(np.diff(np.concatenate([up[:, None, :], U], axis=1), axis=1)).max())

    _, U_free, st_free = mpc.closed_loop_batch(X0, steps, max_iter=200, tol_constraint=tol_c)
    free = largest_move(U_free)
    _, U, st = mpc.closed_loop_batch(X0, steps, u_prev=up, du_lb=[-d], du_ub=[d], max_iter=200, tol_constraint=tol_c)
    lim = largest_move(U)
    print(f"[rate closed loop] largest applied move: without limits {free:.4f}, with limits {lim:.8f} (limit {d}); "
          f"converged per step {(st_free == 0).sum(axis=1).tolist()} / {(st == 0).sum(axis=1).tolist()} of {B}; "
          f"iterations {mpc.last_closed_loop_iterations}")
    assert (st_free == 0).all()
    assert free >= 2.0 * d
    assert (st == 0).all()
    assert lim <= d + tol_c
    # the engine is left without a binding
    from pyneuralempc_amd.optimizer.base import fused_evaluator
    assert fused_evaluator(integ, obj, None).engine._rate is None


def _refused(code, word, fn, *a, **kw):
    from pyneuralempc_amd._lib import NempcError
    with pytest.raises(NempcError) as ei:
        fn(*a, **kw)
    assert ei.value.code == code and word in str(ei.value), (ei.value.code, str(ei.value))


def test_refusals_and_the_way_back():
    """Each refusal returns its code and leaves a nempc_last_error text naming the call; a batch larger than u_prev covers is
    NEMPC_EINVAL; after bind_rate() with nothing a plain solve returns the bits it returned before any binding (Z, status,
    iteration counts); a bound but unused binding changes no bit of eval, hess or rollout."""
    B = 4
    case, eng, X0 = _nl_engine(B)
    lb, ub = np.full(case.n, -NL_BOUND), np.full(case.n, NL_BOUND)
    kw = dict(reg=sc.REG, max_iter=60, return_iterations=True)
    Z0, st0, it0, per0 = eng.solve(X0, None, lb, ub, **kw)
    Z0d, st0d, _, duals = eng.solve(X0, None, lb, ub, reg=sc.REG, max_iter=60, return_duals=True)
    lam = duals["lam"]
    sig = torch.ones(B, dtype=eng.dtype, device=eng.device)
    before = dict(ev={k: v.clone() for k, v in eng.eval(Z0, X0, want=("f", "grad", "g", "jac_tiles")).items()},
                  he=eng.hess(Z0, X0, lam, sig, want=("hvals",))["hvals"].clone(), ro=eng.rollout(X0, Z=Z0.clone()).clone())
    up = eng.to_device(case.u_prev[:B])
    eng.bind_rate(u_prev=up, S=case.S, du_lb=[-0.3], du_ub=[0.3])
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
    # a batch larger than u_prev covers
    eng.bind_rate(u_prev=up[:2].contiguous(), S=case.S)
    _refused(EINVAL, "nempc_solve", eng.solve, X0, None, lb, ub, reg=sc.REG, max_iter=5)
    # dlo >= dhi reaches the library only past the Python check: ask it directly
    from pyneuralempc_amd import _lib
    import ctypes
    one = (ctypes.c_double * 1)(0.1)
    assert eng.lib.nempc_bind_rate(eng._handle, None, one, one, 0, ctypes.c_void_p(up.data_ptr()), B) == EINVAL
    assert b"nempc_bind_rate" in eng.lib.nempc_last_error()
    assert eng.lib.nempc_bind_rate(eng._handle, None, one, None, 0, None, B) == EINVAL
    # a rolling-window handle refuses the binding
    roll = sc.qp_case("roll3_fwd", 10)
    reng = roll.engine()
    hu = reng.to_device(np.zeros((1, roll.nu)))
    assert reng.lib.nempc_bind_rate(reng._handle, None, None, one, 0, ctypes.c_void_p(hu.data_ptr()), 1) == EUNSUPPORTED
    assert b"nempc_bind_rate" in reng.lib.nempc_last_error()
    # a solve under the binding, then the way back: the plain solve's bits
    eng.bind_rate(u_prev=up, S=case.S, du_lb=[-0.3], du_ub=[0.3])
    Zr, str_, _ = eng.solve(X0, None, lb, ub, reg=sc.REG, max_iter=60)
    assert (str_.cpu().numpy() == 0).all() and not torch.equal(Zr, Z0)
    eng.bind_rate()
    Z1, st1, it1, per1 = eng.solve(X0, None, lb, ub, **kw)
    assert torch.equal(Z1, Z0) and torch.equal(st1, st0) and torch.equal(per1, per0) and it1 == it0


def test_next_batch_and_device_sqp_carry_the_previous_control():
    """NMPC.next_batch(u_prev=, du_weight=, du_lb=, du_ub=) gives what the engine gives with the same binding (bit for bit) and
    leaves no binding behind; NMPC.next with DeviceSqp(du_lb=, du_ub=) starts from u_prev = 0, then from the control it
    returned: both first moves are inside the limit."""
    import pyneuralempc_amd as nEMPC
    from pyneuralempc_amd.optimizer.base import fused_evaluator
    B, H, d = 4, rc.NL_H, 0.05
    case = rc.nl_case(B)
    model = nEMPC.model.MLPModel(case.net.W, case.net.b, 2, 1, device="cuda:0")
    integ = nEMPC.integrator.DiscretIntegrator(model, H)
    obj = nEMPC.objective.QuadraticObjective(Q=np.eye(2), R=0.01 * np.eye(1), xref=np.tile([0.8, -0.4], (H, 1)), device="cuda:0")
    dom = nEMPC.constraints.DomainConstraint(states_constraint=[[-5.0, 5.0]] * 2, control_constraint=[[-1.0, 1.0]])
    mpc = nEMPC.controller.NMPC(integ, obj, [dom], H, 1.0, optimizer=nEMPC.optimizer.DeviceSqp(du_lb=[-d], du_ub=[d]))
    X0 = case.X0[:B] * 0.2
    S = 0.2 * np.eye(1)
    xs, us, st = mpc.next_batch(X0, u_prev=case.u_prev[:B], du_weight=S, du_lb=[-d], du_ub=[d], max_iter=200)
    eng = fused_evaluator(integ, obj, None).engine
    assert eng._rate is None and (st == nEMPC.optimizer.Optimizer.SUCCESS).all()
    assert (np.abs(us[:, 0] - case.u_prev[:B]) <= d + 1e-8).all() and (np.abs(np.diff(us, axis=1)) <= d + 1e-8).all()
    eng.bind_rate(u_prev=eng.to_device(case.u_prev[:B]), S=S, du_lb=[-d], du_ub=[d])
    lb, ub = np.asarray(dom.get_lower_bounds(H), dtype=np.float64), np.asarray(dom.get_upper_bounds(H), dtype=np.float64)
    Z, _, _ = eng.solve(eng.to_device(X0), None, lb, ub, max_iter=200)
    eng.bind_rate()
    assert np.array_equal(Z.cpu().numpy()[:, H * 2:].reshape(B, H, 1), us)
    _, u1 = mpc.next(X0[0])
    assert u1 is not None and abs(u1[0, 0]) <= d + 1e-8
    _, u2 = mpc.next(X0[0])
    assert u2 is not None and abs(u2[0, 0] - u1[0, 0]) <= d + 1e-8 and abs(u2[0, 0]) > d      # (it keeps ramping)
    _, u3 = mpc.next(X0[0], u_prev=[0.0])
    assert u3 is not None and abs(u3[0, 0]) <= d + 1e-8
