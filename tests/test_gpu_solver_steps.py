"""GPU: single steps of the batched solver (csrc/solver.hip) against a dense float64 KKT reference.

`nempc_solve` with max_iter = k returns the iterate after k accepted steps (the last iteration of a budget runs its
acceptance test), and each step is the solution of a KKT system the oracle builds densely (tests/kkt_reference.py).  The
existing solver tests check where a solve ends; a globalised SQP method gets there with a wrong direction too -- these
check the direction: the Riccati recursion, the cross term Qux, the Lagrangian blocks, the costates, the terminal weight,
the off-diagonals of Q / R / QT and the linear cost terms.

Tolerances are not taken from the device: per case, e = |riccati_step(handle's dtype) - newton_step(float64)|inf on the
CPU is what a correct sweep in that precision loses on that system; 10 e is allowed, floored at 1e-12 (1 + |z|inf)
(solver_step_cases.step_tolerance).  Largest tolerance over the problems of each shape:

  (a) one Newton step, linear networks                       (b) cumulative over the steps, tanh networks
  2x1_discret  H=1 1.8e-12  H=2 2.1e-12  H=3 2.3e-12          2x1_h20    3.1e-13 3.3e-13 3.7e-13 -> floor ~3e-12
               H=20 5.9e-12  H=63 2.1e-11                     2x1_h63    1.0e-12 1.4e-12 1.6e-12
  2x1_global   H=355 1.3e-10                                  6x3_rk4    floor ~1.5e-12
  6x3_rk4 2.0e-12   3x2_unity 1.8e-12   5x2_one_layer 1.9e-12 3x2_unity  floor ~1.6e-12
  roll3_fwd 2.2e-12  roll3_rev 2.1e-12  2x1_extras 2.0e-12    5x2_h9     3.4e-13 3.7e-13 4.1e-13 -> floor ~3e-12
  2x1_fp32 H=20 2.4e-05                                       6x3_fp32   5.5e-07 8.5e-07
against steps of order 1 (up to 18 at H = 355) and multipliers up to 1100.  The wide rows (12 .. 70 states):
  12x5_discret 2.6e-12  3x8_discret 2.5e-12  16x4_rk4 2.4e-12       12x5_h4   floor ~1.8e-12    20x4_h6  floor ~2.6e-12
  20x4_discret 2.8e-12  33x3_unity 3.0e-12  40x10_discret 2.3e-12   16x4_rk4  floor ~1.5e-12    40x10_h3 floor ~1.9e-12
  64x8_discret H=1 1.9e-12  H=3 2.3e-12     70x3_discret 2.2e-12    70x3_h2   floor ~2.0e-12
  40x10_fp32 3.5e-06 (smallest over the problems 1.1e-06)  64x8_fp32 9.0e-07 (smallest 2.2e-07)
(cumulative sweep errors of the wide tanh rows are 3e-15 .. 3e-14: every tolerance there is the floor).

Every solve also reports which LQ plan ran (CallbackEngine.last_lq_kernel); tests (a) and (b) hold it against the plan the
size formula predicts for the row and the requested kernel (solver_step_cases.expected_lq_plan).

The last four tests are about the branch (a) and (b) keep out of: a control Hessian that is not positive definite, the
restarted sweep and the per-problem damping it stores (kkt_reference.damped_replay restates the rule; cases (e), (f), (g) of
solver_step_cases).  Their tolerance is the same step_tolerance, of the sweep error at the reg of the level that wins;
the largest per row is in each test's docstring.
"""
import numpy as np
import pytest

import solver_step_cases as sc

pytestmark = pytest.mark.gpu

BATCHES = (1, 2, 3, 16)     # solver_lq_kernel's staging splits its waves differently for 1, 2 and >= 3 problems per workgroup


def _solve(eng, X0, Zi, reg=sc.REG, **kw):
    Z, st, it, per = eng.solve(X0, Zi, reg=reg, return_iterations=True, **kw)
    return Z.cpu().double().numpy(), st.cpu().numpy(), it, per.cpu().numpy()


def _kernels(eng):
    return f"variant {eng.kernel_variant}, rows {eng.last_row_kernel}, blocks {eng.last_hess_kernel}, lq {eng.last_lq_kernel}"


@pytest.mark.parametrize("name,H", sc.QP_CASES)
def test_one_newton_step_solves_an_equality_constrained_qp(name, H):
    """Linear networks: the NLP is an equality-constrained convex QP, the Lagrangian blocks are zero and the first step is
    exact.  After max_iter = 1 the iterate is z0 + dz_ref; a full solve ends there too (status 0 everywhere) and every
    problem's convergence iteration is at most 3: the Newton step lands on the solution, the next iteration sees a zero step
    and passes the convergence test, one more is allowed for a deferred acceptance.  Every lq_kernel the row names, B in
    {1, 2, 3, 16}, cold start (and a random Z_init on two rows).

    Observed on an MI355X: every problem of every row, kernel and batch size converges at iteration 2.  Handle variant,
    last row kernel, last block kernel, and the largest error as a fraction of the tolerance (one step = full solve):
      2x1_discret H=1,2,3   mfma  rows_mfma_kernel  rowhess_coop_kernel       0.000
      2x1_discret H=20      mfma  rows_mfma_kernel  rowhess_coop_kernel       0.025 (random Z_init: 0.025)
      2x1_discret H=63      mfma  rows_mfma_kernel  rowhess_coop_kernel       0.100
      2x1_global  H=355     mfma  rows_mfma_kernel  rowhess_coop_kernel       0.100
      6x3_rk4     H=8       mfma  rows_coop_kernel  rk4:rowhess_coop_kernel   0.003 (random Z_init: 0.004)
      3x2_unity   H=7       mfma  rows_coop_kernel  rowhess_coop_kernel       0.000
      5x2_one_layer H=9     valu  rows_valu_kernel  rowhess_valu_kernel       0.006
      roll3_fwd / roll3_rev mfma  rows_coop_kernel  rowhess_coop_kernel       0.002 / 0.006
      2x1_extras  H=10      mfma  rows_mfma_kernel  rowhess_coop_kernel       0.003
      2x1_fp32    H=20      mfma  rows_coop_kernel  rowhess_coop_kernel       0.151
    The wide rows (LQ plan per requested kernel in the row's order; all problems converge at iteration 2):
      12x5_discret H=4      mfma     rows_mfma_kernel    rowhess_mfma_kernel       thread_lds wave_lds wave_lds   0.003 (random Z_init: 0.004)
      3x8_discret  H=5      mfma     rows_coop_kernel    rowhess_coop_kernel       thread_lds wave_lds wave_lds   0.002
      16x4_rk4     H=4      layered  layered_gemm_kernel rk4:layered_gemm_kernel   thread_lds wave_lds wave_lds   0.003
      20x4_discret H=6      layered  layered_gemm_kernel layered_gemm_kernel       thread_lds wave_lds wave_lds   0.014 (random Z_init: 0.013)
      33x3_unity   H=3      layered  layered_gemm_kernel layered_gemm_kernel       thread_lds wave_lds            0.002
      40x10_discret H=3     layered  layered_gemm_kernel layered_gemm_kernel       thread_global thread_global    0.006
      40x10_fp32   H=3      layered  layered_gemm_kernel layered_gemm_kernel       thread_lds wave_lds            0.234
      64x8_discret H=1, 3   layered  layered_gemm_kernel layered_gemm_kernel       thread_global                  0.001 / 0.007
      64x8_fp32    H=1      layered  layered_gemm_kernel layered_gemm_kernel       thread_lds wave_lds            0.821  (see below)
      70x3_discret H=2      valu     rows_valu_kernel    rowhess_valu_kernel       thread_global                  0.006
    16x4_rk4 first failed differently: as an fp64 RK4 stage of 16 states and 20 inputs it was given to the matrix-core row
    kernels, whose scratch of one wave (168.5 KiB) exceeds a CU's LDS, and every launch was refused (hipFuncSetAttribute:
    invalid argument).  mfma_supported (csrc/kernels_mfma.hip) now leaves such shapes to the layered path.
    64x8_fp32 first missed the one-step tolerance on problem 0: |Z - (z0 + dz)| = 2.764e-07 against 2.164e-07 (ratio 1.277),
    the same bits for both kernels and every batch size, all of it on the controls; its multipliers missed theirs by 1.108
    (tests/test_gpu_duals.py).  No term was wrong: a CPU float32 replay of the kernel's own order of operations on the
    device's evaluation reproduces the device's figures (multipliers 1.87e-06, to three digits; step 1.14 of the tolerance).
    It was the length of the sums: at 64 states every entry of P c, B' P c and P dx is a float32 sum of 64 terms of order
    one, while the tolerance of that problem is ten times 2.16e-08 -- at H = 1 the NumPy float32 sweep rounds almost exactly.
    The run-time-dimension LQ kernels now accumulate the sweeps' sums in double on fp32 handles (LqAcc,
    csrc/solver_lq_impl.h; the replay with those sums in double predicted 0.32 / 0.90): 0.821 here and 0.901 on the
    multipliers, 40x10_fp32 0.685 -> 0.234.  fp64 handles and the compiled 2/1 and 6/3 stages are untouched, bit for bit.
    (a linear network is not among the fused launch's compiled shapes -- the row kernel is rows_mfma_kernel, not
    rows_coopfx_kernel, also at 2 x 64 linear -- so the 2/1 rows run the deferred schedule with evaluation, block and
    acceptance launches of their own; the trial point's blocks from the evaluation launch and the acceptance test inside the
    next LQ kernel are reached by the tanh 2 x 64 shapes of the next test)"""
    case = sc.qp_case(name, H)
    eng = case.engine()
    bad, plans = [], set()
    for rnd in ((False, True) if (name, H) in sc.QP_RANDOM_START else (False,)):
        ref = sc.qp_reference(name, H, rnd)
        worst1 = worstf = 0.0
        its = set()
        for B in BATCHES:
            X0 = case.bind(eng, B)
            Zi = eng.to_device(case.Zrand[:B]) if rnd else None
            for k in case.kernels:
                Z1, _, _, _ = _solve(eng, X0, Zi, max_iter=1, lq_kernel=k)
                plans.add((k, eng.last_lq_kernel))
                if case.window == 1:        # (a rolling-window solve plans over the augmented state)
                    want = sc.expected_lq_plan(case.nx, case.nu, H, case.dtype, k)
                    if eng.last_lq_kernel != want:
                        bad.append(f"{k} B={B}: LQ plan {eng.last_lq_kernel}, the size formula says {want}")
                Zf, st, _, per = _solve(eng, X0, Zi, max_iter=30, lq_kernel=k)
                its.update(per.tolist())
                if not (st == 0).all() or per.max() > 3 or per.min() < 1:
                    bad.append(f"{k} B={B} random={rnd}: status {st.tolist()} convergence iterations {per.tolist()}")
                for b in range(B):
                    z0, dz, _, tol, _ = ref[b]
                    e1, ef = np.abs(Z1[b] - (z0 + dz)).max(), np.abs(Zf[b] - (z0 + dz)).max()
                    worst1, worstf = max(worst1, e1 / tol), max(worstf, ef / tol)
                    if not e1 <= tol:
                        bad.append(f"{k} B={B} b={b} random={rnd}: after one step |Z - (z0 + dz)| = {e1:.3e} > {tol:.3e}")
                    if not ef <= tol:
                        bad.append(f"{k} B={B} b={b} random={rnd}: full solve |Z - (z0 + dz)| = {ef:.3e} > {tol:.3e}")
        print(f"[qp {name} H={H} random={rnd}] {_kernels(eng)}; plans {sorted(plans)}; convergence iterations {sorted(its)}; "
              f"error / tolerance: one step {worst1:.3f}, full solve {worstf:.3f}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", list(sc.NL_ROWS))
def test_three_steps_of_a_nonlinear_solve_follow_the_newton_replay(name):
    """tanh networks: max_iter = 1, 2, 3 against the full-step SQP replay with lam <- lam+.  Step 2 is the first whose
    Hessian carries sum lam d2Phi with the costates of step 1 (wrong if the blocks' use in the sweep or the costates are);
    step 3 checks the costates of a step that had blocks.  Every problem must clear the reference's gates at every compared
    step (reduced Hessian eigenvalue >= 0.05: no damping restart; l1 merit strictly decreasing under the full step): a gate
    failure fails the test.  A problem is no longer compared once the reference step is below 1e-6.

    Observed on an MI355X (handle variant mfma everywhere; last row kernel, last block kernel, largest error as a fraction of
    the tolerance after 1 / 2 / 3 steps):
      2x1_h20    rows_coopfx_kernel  rowhess_coopfx_kernel    0.017 0.003 0.003   (auto: scan, fused accept path)
      2x1_h63    rows_coopfx_kernel  rowhess_coopfx_kernel    0.054 0.058 0.012
      6x3_rk4    rows_mfma_kernel    rk4:rowhess_coop_kernel  0.008 0.006 0.003   (auto: wave, inner-loop line search)
      3x2_unity  rows_mfma_kernel    rowhess_coop_kernel      0.000 0.000 0.000
      5x2_h9     rows_mfma_kernel    rowhess_coop_kernel      0.020 0.005 0.003
      6x3_fp32   rows_mfma_kernel    rk4:rowhess_coop_kernel  0.523 0.131
    The wide rows (every problem is compared after 1 and 2 steps -- asserted from the reference; after 3 steps 2 of 8 on
    16x4_rk4 and 6 of 8 on 70x3_h2, the others' reference steps are below STOP_STEP by then):
      12x5_h4    mfma     rows_mfma_kernel     rowhess_mfma_kernel      thread_lds wave_lds wave_lds  0.002 0.003 0.002
      20x4_h6    layered  layered_gemm_kernel  layered_gemm_kernel      thread_lds wave_lds wave_lds  0.009 0.007 0.004
      16x4_rk4   layered  layered_gemm_kernel  rk4:layered_gemm_kernel  wave_lds wave_lds             0.004 0.003 0.004
      40x10_h3   layered  layered_gemm_kernel  layered_gemm_kernel      thread_global                 0.004 0.003 0.004
      70x3_h2    valu     rows_valu_kernel     rowhess_valu_kernel      thread_global                 0.003 0.004 0.004
    Sharpness, checked once with a local edit: with the Lagrangian block's term of Qux negated in solver_lq_kernel
    (csrc/solver_lq_impl.h) every `thread` case here fails from step 2 on (errors 1e-9 ... 2e-1 against 2e-12) while the one-step QP test above passes."""
    case = sc.nl_case(name)
    steps = sc.NL_ROWS[name][8]
    ref = sc.nl_reference(name)
    for rp, _ in ref:
        for s in rp:
            assert s["eig"] >= sc.GATE_EIG and s["dmerit"] < 0.0, (s["eig"], s["dmerit"])
    # (every problem is compared after one and after two steps, on every row: from the reference, not from the device)
    assert all(np.abs(s["dz"]).max() >= sc.STOP_STEP for rp, _ in ref for s in rp[:2])
    eng = case.engine()
    X0 = case.bind(eng, case.B)
    bad, plans = [], set()
    worst = np.zeros(steps)
    for k in case.kernels:
        for it in range(1, steps + 1):
            Z, _, _, _ = _solve(eng, X0, None, max_iter=it, lq_kernel=k)
            plans.add((k, eng.last_lq_kernel))
            want = sc.expected_lq_plan(case.nx, case.nu, case.H, case.dtype, k)
            if eng.last_lq_kernel != want:
                bad.append(f"{k}: LQ plan {eng.last_lq_kernel}, the size formula says {want}")
            for b, (rp, cum_e) in enumerate(ref):
                if any(np.abs(s["dz"]).max() < sc.STOP_STEP for s in rp[:it]):
                    continue
                tol = sc.step_tolerance(cum_e[it - 1], rp[it - 1]["z"])
                e = np.abs(Z[b] - rp[it - 1]["z"]).max()
                worst[it - 1] = max(worst[it - 1], e / tol)
                if not e <= tol:
                    bad.append(f"{k} b={b} after {it} steps: |Z - z_ref| = {e:.3e} > {tol:.3e} (ratio {e / tol:.1f})")
    print(f"[nl {name}] {_kernels(eng)}; plans {sorted(plans)}; error / tolerance per step {np.round(worst, 3).tolist()}")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("linesearch", ["loop", "deferred"])
@pytest.mark.parametrize("barrier", ["primal-dual", "primal"])
@pytest.mark.parametrize("name", list(sc.BOUNDED_ROWS))
def test_interior_point_ends_at_the_solution_of_the_bounded_qp(name, barrier, linesearch):
    """Linear networks with tight control bounds, wide state bounds and one state limit set through the box rows: the
    converged iterate against the exact active-set solution (kkt.qp_solution).  The reference's smallest active bound
    multiplier nu_min is at least 1e-3 (asserted), and the tolerance is 10 (mu_min / nu_min + tol_step (1 + |z*|inf)): the
    distance the barrier's last sub-problem keeps from an active bound plus the stopping test, with a tenfold margin.

    Observed on an MI355X on the wide rows (B = 4, budget 400): 20x4_h6 (LQ plan wave_lds) converges in 19 .. 32 iterations
    with 4 .. 17 active bounds per problem and errors of 0.07 .. 0.22 of the tolerance; 40x10_h3 (thread_global) in 20 .. 40
    iterations, 14 .. 16 active bounds, errors of 0.09 .. 0.10 of the tolerance."""
    mu_min, tol_step = 1e-9, 1e-8
    case, lbe, ube, given = sc.bounded_case(name)
    ref = sc.bounded_reference(name)
    eng = case.engine()
    eng.set_box_rows(given["box_lo"], given["box_hi"])
    Z, st, it, per = _solve(eng, case.bind(eng, case.B), None, lb=given["lb"], ub=given["ub"], max_iter=400, barrier=barrier,
                            linesearch=linesearch, mu_min=mu_min, tol_step=tol_step)
    assert (st == 0).all(), (st.tolist(), it)
    H, nx = case.H, case.nx
    worst, box_active = 0.0, 0
    for b, (zs, _, nlo, nhi) in enumerate(ref):
        act = np.concatenate([nlo[nlo > 0], nhi[nhi > 0]])
        assert act.min() >= sc.NU_MIN and ((nlo + nhi)[H * nx:] > 0).sum() >= 2
        box_active += int(((nlo + nhi)[:H * nx] > 0).sum())
        tol = 10.0 * (mu_min / act.min() + tol_step * (1.0 + np.abs(zs).max()))
        e = np.abs(Z[b] - zs).max()
        worst = max(worst, e / tol)
        print(f"[bounded {name} {barrier} {linesearch}] b={b}: {len(act)} active bounds, nu_min {act.min():.3e}, "
              f"|Z - z*| = {e:.3e}, tolerance {tol:.3e}, iterations {per[b]}")
        assert e <= tol, (b, e, tol)
        assert (Z[b] >= lbe - 1e-12).all() and (Z[b] <= ube + 1e-12).all()
    assert box_active >= 1          # the state limit of the box rows binds


@pytest.mark.parametrize("name", list(sc.SOC_ROWS))
def test_a_rejected_full_step_ends_on_a_member_of_the_candidate_set(name, monkeypatch):
    """Second-order correction (solver_soc_kernel, csrc/solver_soc_impl.h) at 6, 64 and 70 states.  tanh networks with the
    output layer not scaled down, fp64, B = 8, no bounds, linesearch="loop", max_iter = 1, from feasible starts
    (solver_step_cases.soc_reference; why not the cold start, there): the reference full step raises the l1 merit for at
    least half of the problems (asserted from the reference), so the iteration goes through the correction and the
    backtracking.  Whatever it accepts, the returned iterate is one of finitely many points the oracle can name: z0 + dz,
    the corrected point z0 + dz + corr (corr: the state-only recursion with the Jacobian tiles at z0 and the defects at
    z0 + dz), z0 + 2^-k dz for k = 1 .. max_linesearch, or z0 itself.  Each problem must be within step_tolerance of one of
    them, with NEMPC_SOLVER_SOC unset and with NEMPC_SOLVER_SOC=0; with the correction on at least one problem lands on the
    corrected point, with it off none does.  A corrected point with states the kernel never wrote, or scored from them,
    matches no member.

    Observed on an MI355X (seed 0, the first tried; where the 8 problems land with the correction on / off; largest error
    as a fraction of the tolerance):
      6x3_rk4  mfma, wave_lds          full step raises the merit for 7 of 8; on: 7 corrected, 1 full;  off: 7 half^1, 1 full;   0.006 / 0.003
      64x8_h3  layered, thread_global  8 of 8; on: 3 corrected, half^2, half^3 x 2, half^4 x 2;  off: half^2 x 4, half^3 x 2, half^4 x 2;   0.010 / 0.003
      70x3_h2  valu, thread_global     8 of 8; on: 8 corrected;  off: half^1 .. half^4;   0.007 / 0.002
    -- as the CPU's Armijo test on the same candidates predicts, problem by problem.
    Sharpness, checked once against a library built with the one-state-per-lane kernel this replaces: 6x3_rk4 and 64x8_h3
    pass, 70x3_h2 fails -- states 64 .. 69 of the corrected points are never written, the merit test rejects all 8 of
    them and every problem backtracks (landing exactly where the run without the correction lands), so "at least one
    problem lands on the corrected point" does not hold.  With the kernel as it is now all three pass, and the 6x3_rk4 and
    64x8_h3 iterates after 1 and after 6 iterations are bit-identical to those of the commit before it."""
    case = sc.soc_case(name)
    ref = sc.soc_reference(name)
    assert sum(r["raises"] for r in ref) >= case.B / 2
    eng = case.engine()
    X0 = case.bind(eng, case.B)
    Zi = eng.to_device(np.stack([r["z0"] for r in ref]))
    bad, landed = [], {}
    for soc in (True, False):
        if soc:
            monkeypatch.delenv("NEMPC_SOLVER_SOC", raising=False)
        else:
            monkeypatch.setenv("NEMPC_SOLVER_SOC", "0")
        Z, _, _, _ = _solve(eng, X0, Zi, max_iter=1, linesearch="loop")
        landed[soc], worst = [], 0.0
        for b, r in enumerate(ref):
            e, label = min((float(np.abs(Z[b] - p).max()), lb) for lb, p in r["cands"])
            landed[soc].append(label)
            worst = max(worst, e / r["tol"])
            if not e <= r["tol"]:
                bad.append(f"correction {'on' if soc else 'off'} b={b}: nearest candidate {label} at {e:.3e} > {r['tol']:.3e}")
        print(f"[soc {name} correction {'on' if soc else 'off'}] {_kernels(eng)}; full step raises the merit for "
              f"{sum(r['raises'] for r in ref)} of {case.B}; landed on {landed[soc]}; error / tolerance {worst:.3f}")
    assert not bad, "\n".join(bad)
    assert "corrected" in landed[True], landed
    assert "corrected" not in landed[False], landed


# --------------------------------------------------------------------------------------
# The damping restarts: what every LQ kernel does when a control Hessian is not positive definite, against
# kkt_reference.damped_replay (the state machine restated) and the dense step at the reg of the level that wins.
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,H", list(sc.DAMPED_QP))
def test_a_restarted_sweep_takes_the_step_of_the_first_level_that_goes_through(name, H):
    """(e) Linear networks with R = -0.15 I + 0.03 N: Quu is indefinite below lambda (the smallest reg at which the sweep
    goes through, one number per row), and the solve is given reg0 = lambda sqrt(10)^(0.5 - k*): the levels below k* fail,
    level k* goes through half a rung above lambda.  k* in {1, 2, 4} x lq_attempts in {1, 3, 5} at B = 16, B in {1, 2, 3} at
    (2, 3), every lq_kernel of the row.  Level k* is reached in iteration it* = k* // lq_attempts + 1: with a smaller budget
    the problem has only sat out -- Z is the start bit for bit and the status is not 0 -- and with max_iter = it* the iterate
    is z0 + dz(reg_k*) of the dense solve, to step_tolerance of the sweep error at reg_k*.  Where the row has no window the
    LQ plan is the one the size formula predicts.

    Largest tolerance per row (step_tolerance of the sweep error at reg_k* in the handle's precision, from the CPU; fp64 sweep
    errors are 1e-16 .. 1.4e-12, every fp64 tolerance but H = 63's is the floor 1e-12 (1 + |z|inf)):
      2x1_discret H=20 7.9e-12  H=31 9.5e-12  H=63 1.5e-11    6x3_rk4 2.1e-12   3x2_unity 1.9e-12   roll3_fwd 2.9e-12
      12x5_discret 2.9e-12   20x4_discret 2.7e-12   40x10_discret 2.3e-12   70x3_discret 2.0e-12
      2x1_fp32 4.2e-05 (sweep error 2.1e-06 .. 4.2e-06)   40x10_fp32 3.0e-06 (9.5e-08 .. 3.0e-07)   64x8_fp32 1.7e-06 (4.5e-08 .. 1.7e-07)
    against steps of 0.5 .. 12.
    Observed on an MI355X: every budget below it* returns the start's bits and a status that is not 0, every kernel and batch
    size.  Handle variant, LQ plan per requested kernel in the row's order, largest error as a fraction of the tolerance at
    max_iter = it*:
      2x1_discret H=20   mfma     thread_lds wave_lds scan scan      0.024      H=31  thread_lds scan  0.034     H=63  thread_lds scan  0.100
      6x3_rk4            mfma     thread_lds wave_lds wave_lds       0.003      3x2_unity  mfma  thread_lds wave_lds  0.000
      roll3_fwd          mfma     wave_lds (the augmented stage)     0.001      12x5_discret  mfma  thread_lds wave_lds wave_lds  0.003
      20x4_discret       layered  thread_lds wave_lds wave_lds       0.013      40x10_discret  layered  thread_global thread_global  0.005
      70x3_discret       valu     thread_global                      0.006      2x1_fp32  mfma  thread_lds wave_lds  0.176
      40x10_fp32         layered  thread_lds wave_lds                0.219      64x8_fp32  layered  thread_lds wave_lds  0.429
    Sharpness, checked once with a local edit: with the winner of solver_lq_kernel's ballot taken as the LAST level of a round
    that goes through instead of the first, 8 of the 13 rows here fail (every row whose `thread` solve keeps levels side by
    side in LDS: the levels above k* go through as well, and the step of the most damped one of the round is taken); roll3_fwd,
    the global-memory rows, and 40x10_fp32 and 64x8_fp32, where one level fills the LDS, pass, as do all wave and scan solves."""
    case = sc.damped_qp_case(name, H)
    eng = case.engine()
    combos = [(ks, at, sc.BMAX) for ks in sc.DAMPED_KSTAR for at in sc.DAMPED_ATTEMPTS] + [(2, 3, B) for B in sc.DAMPED_SMALL_B]
    bad, plans, worst = [], set(), 0.0
    for ks, at, B in combos:
        ref = sc.damped_qp_reference(name, H, ks)
        assert all(p[5] < 0.0 for p in ref["probs"])            # the dense full step lowers the l1 merit
        X0 = case.bind(eng, B)
        need = sc.iterations_needed(ks, at)
        for k in case.kernels:
            for it in range(1, need + 1):
                Z, st, _, _ = _solve(eng, X0, None, reg=ref["reg0"], max_iter=it, lq_kernel=k, lq_attempts=at)
                plans.add((k, eng.last_lq_kernel))
                tag = f"k*={ks} attempts={at} B={B} {k} max_iter={it}"
                if case.window == 1:
                    want = sc.expected_lq_plan(case.nx, case.nu, H, case.dtype, k)
                    if eng.last_lq_kernel != want:
                        bad.append(f"{tag}: LQ plan {eng.last_lq_kernel}, the size formula says {want}")
                for b in range(B):
                    z0, dz, _, tol, _, _ = ref["probs"][b]
                    if it < need:
                        if not np.array_equal(Z[b], z0) or st[b] == 0:
                            bad.append(f"{tag} b={b}: sat out, but |Z - z0| = {np.abs(Z[b] - z0).max():.3e}, status {st[b]}")
                    else:
                        e = np.abs(Z[b] - (z0 + dz)).max()
                        worst = max(worst, e / tol)
                        if not e <= tol:
                            bad.append(f"{tag} b={b}: |Z - (z0 + dz(reg_k*))| = {e:.3e} > {tol:.3e} (|dz| = {np.abs(dz).max():.3g})")
    print(f"[damped qp {name} H={H}] {_kernels(eng)}; plans {sorted(plans)}; error / tolerance {worst:.3f}")
    assert not bad, "\n".join(bad[:40])


def _follow(eng, case, X0, ref, reg0, attempts, kernel, budgets, compare, bad, worst, duals=False, **kw):
    """max_iter = 1 .. budgets against a damped_replay per problem (ref: [(replay, cumulative sweep error)]): over an
    iteration the replay sits out Z (and lam, with duals) keeps its bits; after one it steps in Z is within step_tolerance
    of the cumulative sweep error.  compare(b, it): whether problem b is still compared after `it` iterations."""
    prev = np.stack([rp[0]["z_before"] for rp, _ in ref])
    prev_lam = None
    for it in range(1, budgets + 1):
        res = eng.solve(X0, None, reg=reg0, max_iter=it, lq_kernel=kernel, lq_attempts=attempts, return_duals=duals, **kw)
        Z = res[0].cpu().double().numpy()
        lam = res[-1]["lam"].cpu().double().numpy() if duals else None
        for b, (rp, cum_e) in enumerate(ref):
            if not compare(b, it):
                if not np.isfinite(Z[b]).all():
                    bad.append(f"{kernel} b={b} after {it} iterations: not finite")
                continue
            s = rp[it - 1]
            if s["level"] is None:
                if not np.array_equal(Z[b], prev[b]):
                    bad.append(f"{kernel} b={b} iteration {it}: the replay sits out, Z moved by {np.abs(Z[b] - prev[b]).max():.3e}")
                if duals and prev_lam is not None and not np.array_equal(lam[b], prev_lam[b]):
                    bad.append(f"{kernel} b={b} iteration {it}: the replay sits out, lam moved by {np.abs(lam[b] - prev_lam[b]).max():.3e}")
            else:
                tol = sc.step_tolerance(cum_e[it - 1], s["z"])
                e = np.abs(Z[b] - s["z"]).max()
                worst[it - 1] = max(worst[it - 1], e / tol)
                if not e <= tol:
                    bad.append(f"{kernel} b={b} after {it} iterations (level {s['level']}, reg {s['reg_used']:.3e}): |Z - z_ref| = "
                               f"{e:.3e} > {tol:.3e} (step {np.abs(s['dz']).max():.3g})")
        prev, prev_lam = Z, lam


RELAX_CASES = [f"{name}-{H}" for name, H in sc.RELAX_ROWS] + ["guard"]


@pytest.mark.parametrize("which", RELAX_CASES)
def test_the_damping_relaxes_only_after_a_sweep_that_needed_no_restart(which):
    """Two halves of one rule (csrc/solver_merit_impl.h, solver_merit_body): an accepted step relaxes the stored reg by
    sqrt(10), but only if its opening sweep went through at level 0.

    The (e) rows 2x1_discret H=20 (thread, scan), 6x3_rk4 (wave), 12x5_discret (thread), 2x1_fp32 (wave) with lq_attempts = 1
    from k* = 2, budgets 1 .. 5: the reference says sit, sit, step, sit, step -- the step of iteration 3 went through at
    level 0, so reg is relaxed to half a rung under lambda, iteration 4 fails there and sits out, iteration 5 steps.  Equal
    bits across a sat-out iteration, cumulative sweep error after a step; both steps lower the l1 merit on every row
    (asserted from the reference).  That half pins that the relaxation happens; with one attempt per iteration every step's
    level is 0 and the guard is never asked.

    "guard": the tanh 2/1 network of (f) with reg0 = GUARD_REG0 and lq_attempts = 2, budgets 1 and 2, thread / wave / scan /
    auto.  At least four problems take their first step at level 1 and, with the first step's multipliers in the blocks,
    need level 1 again from the reg that step stored (asserted from the reference).  Had the first step's acceptance
    relaxed reg, the second iteration's two levels would both lie below what goes through and the problem would sit out.
    Problems whose replay is not robust or whose step raises the merit are only required to be finite.
    Observed on an MI355X (largest error as a fraction of the tolerance after budgets 1 .. 5; 0 where every problem sat out):
      2x1_discret H=20  thread_lds, scan   0 0 0.023 0 0.014       6x3_rk4  wave_lds   0 0 0.002 0 0.001
      12x5_discret      thread_lds         0 0 0.003 0 0.004       2x1_fp32 wave_lds   0 0 0.136 0 0.170
      guard             thread_lds, wave_lds, scan, scan: 9 of 16 problems compared (7 of them level 1 twice), 0.003 0.007
    Sharpness, checked once with a local edit: with the `if (!(lsr > T(0)))` guard of the relaxation removed (every accepted
    step relaxes), the four (e) rows pass -- as argued above they cannot see the guard -- and "guard" fails on every kernel:
    problems 4, 5, 7, 8, 9, 13 and 14 sit out the second iteration, 1.8 .. 10.5 away from the replay's second step (tolerance
    4e-12 .. 1.6e-11); every other new test passes with that edit."""
    bad = []
    if which == "guard":
        case, reg0, attempts, budgets = sc.mixed_case("2x1_h20"), sc.GUARD_REG0, sc.GUARD_ATTEMPTS, 2
        ref = sc.guard_reference()
        kernels, B = case.kernels, case.B
        good = [all(s["robust"] for s in rp) and all(s["dmerit"] < 0.0 for s in rp if s["level"] is not None) for rp, _ in ref]
        assert sum(g and [s["level"] for s in rp] == [1, 1] for g, (rp, _) in zip(good, ref)) >= 4
    else:
        name, H = next(r for r in sc.RELAX_ROWS if f"{r[0]}-{r[1]}" == which)
        case, kernels, attempts, budgets, B = sc.damped_qp_case(name, H), sc.RELAX_ROWS[(name, H)], 1, sc.RELAX_BUDGETS, sc.RELAX_B
        reg0, ref = sc.relax_reference(name, H)
        for rp, _ in ref:
            assert [s["level"] for s in rp] == [None, None, 0, None, 0] and all(s["robust"] for s in rp)
            assert all(s["dmerit"] < 0.0 for s in rp if s["level"] is not None)
        good = [True] * B
    eng = case.engine()
    X0 = case.bind(eng, B)
    worst = np.zeros(budgets)
    for k in kernels:
        _follow(eng, case, X0, ref, reg0, attempts, k, budgets, lambda b, it: good[b], bad, worst)
    print(f"[relax {which}] {_kernels(eng)}; compared {sum(good)} of {B}; error / tolerance per budget {np.round(worst, 3).tolist()}")
    assert not bad, "\n".join(bad[:40])


@pytest.mark.parametrize("name", list(sc.MIXED_ROWS))
def test_problems_of_one_launch_win_at_different_levels(name, monkeypatch):
    """(f) tanh networks at the first step, output layer not scaled down, R with a negative diagonal, B = 16: the smallest reg
    that goes through varies with the problem (through B_t), so the problems of one launch -- of one wave, in the thread
    kernel -- win at different levels of the same ladder.  Asserted from the reference: at least two levels are each taken by
    at least two robust problems, at most 2 of 16 are not robust.  NEMPC_SOLVER_SOC=0, linesearch="loop", max_iter = 1, with
    lq_attempts = 5 and with 3; with 3 the problems whose level is 3 or more come back bit-identical to their start (status
    not 0) while their neighbours move.  A robust problem whose full step lowers the l1 merit is within step_tolerance of
    z0 + dz(reg of its own level); one whose full step raises it is within the tolerance of a member of {z0 + 2^-j dz, j = 0
    .. MAX_LINESEARCH} or z0; a problem that is not robust only has to be finite.

    From the reference (winning level: problems; full step raises the merit for; largest tolerance):
      2x1_h20  R -0.15 I + 0.03 N  reg0 0.012    lambda 0.020 .. 0.259  {1: 2, 2: 7, 3: 7}, all robust   7 of 16   3.3e-11
      12x5_h4  R -0.3 I + 0.03 N   reg0 0.0658   lambda 0.609 .. 0.686  {2: 10, 3: 6}, all robust        0 of 16   1.0e-11
      20x4_h6  R -0.3 I + 0.03 N   reg0 0.0475   lambda 0.439 .. 0.581  {2: 9, 3: 7}, problem 6 (level 2) not robust   6 of 16   8.0e-10
    (12x5_h4: reg0 moved from 0.0612, where 15 of 16 problems win at level 3, into the gap of the per-problem lambda between
    0.6515 and 0.6642.)
    Observed on an MI355X (handle variant; plans; where the 16 problems land with 5 attempts, the same for every kernel; with 3
    attempts the problems of level 3 sit out and the others land where they landed with 5; largest error / tolerance):
      2x1_h20  mfma     thread_lds wave_lds scan scan   9 full, half^1, half^2 x 2, half^3, half^4 x 2, half^5   0.005
      12x5_h4  mfma     thread_lds wave_lds             16 full                                                  0.044
      20x4_h6  layered  thread_lds wave_lds             9 full, half^1 x 3, half^2 x 2, problem 6 not compared   0.060
    -- every problem whose full step raises the merit lands on a shortened step of its own level's direction, none on z0.
    Sharpness, checked once with a local edit: with the winner of solver_lq_kernel's ballot taken as the LAST level of a round
    that goes through instead of the first, all three rows fail, in their `thread` solves only: with 5 attempts every
    problem of level 3 takes the step of level 4 (errors 0.45 .. 2.0 against 2e-12 .. 5e-12), the problems of level 1 on
    2x1_h20 and of level 2 on 20x4_h6 that of level 2 resp. a higher one; the wave and scan solves pass."""
    case = sc.mixed_case(name)
    ref = sc.mixed_reference(name)
    reg0 = sc.MIXED_ROWS[name][8]
    levels = [r["level"] for r in ref if r["robust"]]
    assert sum(levels.count(lv) >= 2 for lv in set(levels) if lv is not None) >= 2 and sum(not r["robust"] for r in ref) <= 2
    monkeypatch.setenv("NEMPC_SOLVER_SOC", "0")
    eng = case.engine()
    X0 = case.bind(eng, case.B)
    bad, plans, worst, landed = [], set(), 0.0, {}
    for at in sc.MIXED_ATTEMPTS:
        for k in case.kernels:
            Z, st, _, _ = _solve(eng, X0, None, reg=reg0, max_iter=1, lq_kernel=k, lq_attempts=at, linesearch="loop")
            plans.add((k, eng.last_lq_kernel))
            want = sc.expected_lq_plan(case.nx, case.nu, case.H, case.dtype, k)
            if eng.last_lq_kernel != want:
                bad.append(f"{k}: LQ plan {eng.last_lq_kernel}, the size formula says {want}")
            lands = []
            for b, r in enumerate(ref):
                tag = f"attempts={at} {k} b={b} (level {r['level']})"
                if not r["robust"]:
                    lands.append("?")
                    if not np.isfinite(Z[b]).all():
                        bad.append(f"{tag}: not finite")
                elif r["level"] is None or r["level"] >= at:
                    lands.append("sat")
                    if not np.array_equal(Z[b], r["z0"]) or st[b] == 0:
                        bad.append(f"{tag}: out of attempts, but |Z - z0| = {np.abs(Z[b] - r['z0']).max():.3e}, status {st[b]}")
                else:
                    cands = r["cands"] if r["raises"] else r["cands"][:1]
                    e, label = min((float(np.abs(Z[b] - p).max()), lb) for lb, p in cands)
                    lands.append(label)
                    worst = max(worst, e / r["tol"])
                    if not e <= r["tol"]:
                        bad.append(f"{tag}: nearest of {len(cands)} candidates {label} at {e:.3e} > {r['tol']:.3e} "
                                   f"(|dz| = {np.abs(r['dz']).max():.3g})")
            landed[(at, k)] = lands
    print(f"[mixed {name}] {_kernels(eng)}; plans {sorted(plans)}; levels {[r['level'] for r in ref]}; error / tolerance {worst:.3f}")
    for key, lands in landed.items():
        print(f"[mixed {name}] attempts, kernel {key}: {lands}")
    assert not bad, "\n".join(bad[:40])


@pytest.mark.parametrize("seed", sc.CLIMB_SEEDS)
def test_a_climbing_problem_resumes_with_the_multipliers_it_had(seed):
    """(g) The tanh 2/1 network of (b) at seeds where the first step's multipliers make a control Hessian indefinite; default
    reg (1e-9), default 3 attempts, budgets 1 .. 4 against damped_replay, thread / wave / scan / auto.  A climbing problem
    takes an undamped first step, sits out two iterations while reg goes 1e-9 -> 1e-2 -> 0.316 through the floor, and takes
    a damped fourth step at level 1 or 2 (reg 1 or 3.16) whose Hessian carries the first step's multipliers in its blocks --
    or sits out the fourth iteration as well ("out of attempts, keep climbing").  Z and, through return_duals=True, lam keep
    their bits over every sat-out iteration; after every iteration the replay steps in, Z is within step_tolerance of the
    cumulative sweep error.  A problem is no longer compared once a reference step is below STOP_STEP.  Asserted from the
    reference, per seed: at least 2 of the 8 problems sat out and then took a damped step, at least 2 never restarted.

    From the reference (levels per iteration, - = sat out):
      seed 5 (pool starts 0 1 6 7 9 12 18 21)   0--2  0---  0--2  0---  0--2  0---  0000  0000      largest tolerance 1.1e-11
      seed 7 (pool starts 0 1 2 3 4 5 7 8)      0--2  0000  0000  0000  0000  0--1  0--2  0--2      largest tolerance 2.5e-12
    Observed on an MI355X (plans thread_lds, wave_lds, scan, scan; handle variant mfma, rows_coopfx_kernel /
    rowhess_coopfx_kernel: the fused accept path under scan; largest error as a fraction of the tolerance after budgets 1 .. 4):
      seed 5   0.101 0.071 0.030 0.323        seed 7   0.062 0.006 0.004 0.095
    Z and lam keep their bits over every sat-out iteration on every kernel."""
    case, ref = sc.climb_case(seed)
    assert sum(sc.climbed(rp) for rp, _ in ref) >= 2 and sum(all(s["level"] == 0 for s in rp) for rp, _ in ref) >= 2
    eng = case.engine()
    X0 = case.bind(eng, case.B)
    bad, worst = [], np.zeros(sc.CLIMB_ITERATIONS)

    def compare(b, it):
        return not any(s["level"] is not None and np.abs(s["dz"]).max() < sc.STOP_STEP for s in ref[b][0][:it])
    for k in case.kernels:
        _follow(eng, case, X0, ref, sc.REG, 0, k, sc.CLIMB_ITERATIONS, compare, bad, worst, duals=True)
    print(f"[climb seed {seed}] {_kernels(eng)}; levels {[[s['level'] for s in rp] for rp, _ in ref]}; "
          f"error / tolerance per budget {np.round(worst, 3).tolist()}")
    assert not bad, "\n".join(bad[:40])
