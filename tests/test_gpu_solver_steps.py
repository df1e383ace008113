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
"""
import numpy as np
import pytest

import solver_step_cases as sc

pytestmark = pytest.mark.gpu

BATCHES = (1, 2, 3, 16)     # solver_lq_kernel's staging splits its waves differently for 1, 2 and >= 3 problems per workgroup


def _solve(eng, X0, Zi, **kw):
    Z, st, it, per = eng.solve(X0, Zi, reg=sc.REG, return_iterations=True, **kw)
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
