"""GPU: the multipliers nempc_solve_duals returns and the on-device KKT residual evaluator nempc_kkt_residual.

References are NumPy float64 on the oracle: tests/kkt_certificate.py (residuals of any primal-dual point) and
tests/kkt_reference.py (the multipliers lam+ of every Newton step, the exact solution of the bounded QPs).  Sign convention
everywhere: g = Phi - x, L = f + lam.g - zl.(z - lb) + zu.(z - ub), zl, zu >= 0.

Tolerances are not taken from the device:
  * evaluator parity: what tests/test_gpu_parity.py allows for grad / g / jac_tiles (fp64 1e-11, fp32 3e-4), relative to
    1 + |grad f|inf + |J|inf |lam|inf;
  * step multipliers: FACTOR times what a Riccati sweep in the handle's precision loses on lam+ (kkt_certificate's
    lam_sweep_error, the construction solver_step_cases.step_tolerance uses for Z), floored at 1e-12 (1 + |lam_ref|inf);
  * bounded QP: bounds that follow from mu_min, tol_step and the returned values themselves (derived in the test).
"""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import nempc_oracle as orc
from helpers import GOLDEN
import kkt_certificate as cert
import kkt_reference as kkt
import solver_step_cases as sc

pytestmark = pytest.mark.gpu

PARITY_TOL = {"float64": 1e-11, "float32": 3e-4}     # tests/test_gpu_parity.py, rows-and-objective parity of both dtypes
FACTOR = 10.0                                         # of the multiplier tolerance (step_tolerance's)
BATCHES = (1, 2, 3, 16)


def _np(t):
    return t.detach().cpu().double().numpy()


# --------------------------------------------------------------------------------------------------------------------
# 1. evaluator parity at arbitrary points
# --------------------------------------------------------------------------------------------------------------------
# id: (kind, row, H, handle keywords, box rows, tracking binding)
PARITY_ROWS = {
    "2x1_H1": ("qp", "2x1_discret", 1, {}, False, False),
    "2x1_H2": ("qp", "2x1_discret", 2, {}, False, False),
    "2x1_H3": ("qp", "2x1_discret", 3, {}, False, False),
    "2x1_H20": ("qp", "2x1_discret", 20, {}, False, False),
    "2x1_H63": ("qp", "2x1_discret", 63, {}, False, False),
    "6x3_rk4_H8": ("qp", "6x3_rk4", 8, {}, False, False),
    "3x2_unity_H7": ("qp", "3x2_unity", 7, {}, False, False),
    "5x2_one_layer": ("qp", "5x2_one_layer", 9, {}, False, False),
    "2x1_extras": ("qp", "2x1_extras", 10, {}, False, False),
    "2x1_fp32": ("qp", "2x1_fp32", 20, {}, False, False),
    "12x5_H4": ("qp", "12x5_discret", 4, {}, False, False),
    "3x8_H5": ("qp", "3x8_discret", 5, {}, False, False),
    "20x4_H6": ("qp", "20x4_discret", 6, {}, False, False),
    "40x10_fp32": ("qp", "40x10_fp32", 3, {}, False, False),
    "64x8_H3": ("qp", "64x8_discret", 3, {}, False, False),
    "70x3_H2": ("qp", "70x3_discret", 2, {}, False, False),
    "tanh_2x1_h20": ("nl", "2x1_h20", 20, {}, False, False),
    "tanh_6x3_rk4": ("nl", "6x3_rk4", 8, {}, False, False),
    "tanh_2x1_h20_box": ("nl", "2x1_h20", 20, {}, True, False),
    "tanh_6x3_rk4_box": ("nl", "6x3_rk4", 8, {}, True, False),
    "tanh_16x4_rk4": ("nl", "16x4_rk4", 4, {}, False, False),
    "tanh_40x10_h3_box": ("nl", "40x10_h3", 3, {}, True, False),
    "tanh_70x3_h2": ("nl", "70x3_h2", 2, {}, False, False),
    "tanh_2x1_h20_tracking": ("nl", "2x1_h20", 20, {}, False, True),
    "tanh_2x1_h20_valu": ("nl", "2x1_h20", 20, {"kernel": "valu"}, False, False),
    "tanh_2x1_h20_layered": ("nl", "2x1_h20", 20, {"kernel": "layered"}, False, False),
}
PARITY_B = (1, 3, 16, 17)
BOX = (-0.3, 0.4)


@pytest.mark.parametrize("rid", list(PARITY_ROWS))
def test_kkt_residual_matches_the_numpy_certificate_at_arbitrary_points(rid):
    """Random Z, lam, zl >= 0, zu >= 0 (no solutions), bounds finite on some variables and infinite on others and violated
    by some entries of Z; r (B,4) and stat (B,n) against kkt_certificate.residuals per problem, B in {1, 3, 16, 17} (17
    grows the handle's workspaces: nempc_reserve).  B = 1 runs without bounds (the multipliers given then count as zero),
    B = 3 with null zl / zu.  Rows: every shape of the step tests at window 1, box rows on, a tracking binding (each problem
    against its own references), and the generic and layered tile producers next to the matrix-core one."""
    kind, row, H, kw, box, track = PARITY_ROWS[rid]
    case = sc.qp_case(row, H) if kind == "qp" else sc.nl_case(row)
    nx, nu, n, hx, ne = case.nx, case.nu, case.n, H * case.nx, case.n_extra
    eng = case.engine(**kw)
    if box:
        eng.set_box_rows(*BOX)
    m = eng.m
    assert m == hx * (2 if box else 1)
    tol = PARITY_TOL[case.dtype]
    rnd = lambda a: sc._round(a, case.dtype)
    rng = np.random.default_rng(7)
    Bm = max(PARITY_B)
    X0, Z = rnd(rng.uniform(-0.5, 0.5, size=(Bm, nx))), rnd(rng.uniform(-0.5, 0.5, size=(Bm, n)))
    lam, zl, zu = rnd(3.0 * rng.normal(size=(Bm, m))), rnd(rng.uniform(0, 1, size=(Bm, n))), rnd(rng.uniform(0, 1, size=(Bm, n)))
    zl[Bm - 1] *= -1.0      # (the last problem, seen at B = 17 only: infeasible multipliers, so r[3] is exercised too)
    lb = np.where(rng.uniform(size=n) < 0.4, -np.inf, rng.uniform(-0.6, -0.2, size=n))
    ub = np.where(rng.uniform(size=n) < 0.4, np.inf, rng.uniform(0.2, 0.6, size=n))
    extra = rnd(0.5 * rng.normal(size=(Bm, H, ne))) if ne else None
    per = {k: rnd(sc.REF_SCALE * rng.normal(size=(Bm, H, d))) for k, d in (("xref", nx), ("uref", nu), ("cx", nx), ("cu", nu))}

    def problem(b):
        ob = dict(case.obj)
        if track:
            ob.update({k: v[b] for k, v in per.items()})
        return orc.Problem(case.net, H, nx, nu, sc.KINDS[case.integ], case.DT, extra=None if extra is None else extra[b],
                           box=BOX if box else None, **ob)

    worst = np.zeros(5)
    for B in PARITY_B:
        if ne:
            eng.bind_extra(eng.to_device(extra[:B]))
        if track:
            eng.bind_tracking(**{k: eng.to_device(v[:B]) for k, v in per.items()})
        use_lb, use_ub = (None, None) if B == 1 else (lb, ub)
        mult = B != 3
        dev = [eng.to_device(a[:B]) for a in (Z, X0, lam, zl, zu)]
        r, stat = eng.kkt_residual(dev[0], dev[1], dev[2], dev[3] if mult else None, dev[4] if mult else None, use_lb, use_ub,
                                   want_stat=True)
        r, stat = _np(r), _np(stat)
        assert r.shape == (B, 4) and stat.shape == (B, n) and np.isfinite(r).all()
        for b in range(B):
            prob = problem(b)
            r_ref, s_ref = cert.residuals(prob, Z[b], X0[b], lam[b], zl[b] if mult else None, zu[b] if mult else None, use_lb, use_ub)
            scale = 1.0 + np.abs(prob.gradient(Z[b])).max() + np.abs(prob.jacobian(Z[b], X0[b])).max() * np.abs(lam[b]).max()
            gscale = 1.0 + np.abs(prob.constraints(Z[b], X0[b])).max()
            errs = np.array([np.abs(stat[b] - s_ref).max() / (tol * scale), abs(r[b, 0] - r_ref[0]) / (tol * scale),
                             abs(r[b, 1] - r_ref[1]) / (tol * gscale), abs(r[b, 2] - r_ref[2]) / (tol * (1.0 + r_ref[2])),
                             abs(r[b, 3] - r_ref[3]) / (tol * (1.0 + r_ref[3]))])
            worst = np.maximum(worst, errs)
            assert (errs <= 1.0).all(), (rid, B, b, errs.tolist(), r[b].tolist(), r_ref.tolist())
        if B > 1:       # bounds are violated and multipliers sit on them: none of the four numbers is trivially zero
            assert (r[:, 0] > 0).all() and (r[:, 1] > 0).all()
            assert mult == bool((r[:, 2] > 0).any())
        if B == Bm:
            assert r[Bm - 1, 3] > 0 and (r[:Bm - 1, 3] == 0).all()
    print(f"[kkt parity {rid}] variant {eng.kernel_variant}, rows {eng.last_row_kernel}; error / tolerance: stat {worst[0]:.1e}, "
          f"r {[f'{w:.1e}' for w in worst[1:]]}")
    if track:
        eng.bind_tracking()


def test_rolling_window_handles_are_refused_by_both_calls_and_still_solve():
    from pyneuralempc_amd._lib import NempcError
    case = sc.qp_case("roll3_fwd", 10)
    eng = case.engine()
    B = 3
    X0 = case.bind(eng, B)
    Z = eng.to_device(case.Zrand[:B])
    lam = torch.zeros(B, eng.m, dtype=eng.dtype, device=eng.device)
    with pytest.raises(NempcError) as e1:
        eng.kkt_residual(Z, X0, lam)
    assert e1.value.code == -5 and "rolling_window" in str(e1.value)
    with pytest.raises(NempcError) as e2:
        eng.solve(X0, None, reg=sc.REG, max_iter=30, return_duals=True)
    assert e2.value.code == -5 and "rolling_window" in str(e2.value)
    Zs, st, _ = eng.solve(X0, None, reg=sc.REG, max_iter=30)
    assert (st == 0).all()
    ref = sc.qp_reference("roll3_fwd", 10)
    for b in range(B):
        z0, dz, _, tolz, _ = ref[b]
        assert np.abs(_np(Zs)[b] - (z0 + dz)).max() <= tolz


# --------------------------------------------------------------------------------------------------------------------
# 2. one Newton step on an equality-constrained QP: lam+ of that step
# --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _qp_lam_error(name, H):
    """Per problem: |riccati_step(handle's dtype) lam+ - newton_step(float64) lam+|inf from the cold start."""
    case = sc.qp_case(name, H)
    ref = sc.qp_reference(name, H)
    out = []
    for b in range(case.B):
        _, lamr = kkt.riccati_step(case.problem(b), ref[b][0], case.X0[b], np.zeros(H * case.nx), sc.REG, sc.np_dtype(case))
        out.append(float(np.abs(lamr - ref[b][2]).max()))
    return out


QP_W1 = [(name, H) for name, H in sc.QP_CASES if sc.QP_ROWS[name][8] == 1]


@pytest.mark.parametrize("name,H", QP_W1)
def test_one_newton_step_returns_the_multipliers_of_that_step(name, H):
    """Linear networks, max_iter = 1: lam[:, :H nx] is lam+ of the dense Newton step (qp_reference), for every lq kernel of
    the row and B in {1, 2, 3, 16}; zl, zu are exactly zero (no bounds); no problem is left out.

    Observed on an MI355X, largest error / tolerance on the wide rows: 12x5 0.006, 3x8 0.004, 16x4_rk4 0.006, 20x4 0.025,
    33x3 0.003, 40x10 0.011, 40x10_fp32 0.199, 64x8 H=1 0.001, H=3 0.013, 70x3 0.008, 64x8_fp32 0.901.  The last one was
    1.108 (problem 4: 1.865e-06 against 1.683e-06) while the run-time-dimension LQ kernels summed 64 float32 terms per
    multiplier in float32; they now accumulate in double on fp32 handles (the 64x8_fp32 note in
    tests/test_gpu_solver_steps.py).  What is left is the float32 objective gradient, which enters lam+ one to one at
    H = 1 and is within 1.1e-06 of the float64 one."""
    case = sc.qp_case(name, H)
    ref, e_lam = sc.qp_reference(name, H), _qp_lam_error(name, H)
    eng = case.engine()
    hx = H * case.nx
    bad, worst, count = [], 0.0, 0
    for B in BATCHES:
        X0 = case.bind(eng, B)
        for k in case.kernels:
            Z, st, it, d = eng.solve(X0, None, reg=sc.REG, max_iter=1, lq_kernel=k, return_duals=True)
            lam, zl, zu = _np(d["lam"]), _np(d["zl"]), _np(d["zu"])
            assert lam.shape == (B, eng.m) and zl.shape == zu.shape == (B, case.n)
            assert (zl == 0).all() and (zu == 0).all() and (lam[:, hx:] == 0).all()
            for b in range(B):
                lam_ref = ref[b][2]
                tol = cert.lam_tolerance(e_lam[b], lam_ref, FACTOR)
                e = np.abs(lam[b, :hx] - lam_ref).max()
                worst, count = max(worst, e / tol), count + 1
                if not e <= tol:
                    bad.append(f"{k} B={B} b={b}: |lam - lam+| = {e:.3e} > {tol:.3e} (|lam+| = {np.abs(lam_ref).max():.2e})")
    assert count == sum(BATCHES) * len(case.kernels)
    print(f"[qp duals {name} H={H}] {count} comparisons, error / tolerance {worst:.3f}, |lam+|inf up to "
          f"{max(np.abs(r[2]).max() for r in ref):.2e}")
    assert not bad, "\n".join(bad)


# --------------------------------------------------------------------------------------------------------------------
# 3. multipliers along a nonlinear solve
# --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _nl_lam_error(name):
    case = sc.nl_case(name)
    steps = sc.NL_ROWS[name][8]
    return [cert.lam_sweep_error(case.problem(b), case.X0[b], case.start(b), steps, sc.REG, sc.np_dtype(case)) for b in range(case.B)]


@pytest.mark.parametrize("name", list(sc.NL_ROWS))
def test_multipliers_along_a_nonlinear_solve_follow_the_newton_replay(name):
    """tanh networks, max_iter = 1, 2, 3: the returned lam is lam+ of replay step k, as Z is the iterate after it.  The 2 x 64
    rows run the fused-accept schedule (trial multipliers carried), the 6/3 rows the inner-loop line search.  A problem is
    no longer compared once a reference step is below STOP_STEP (the existing rule); steps 1 and 2 compare all 8 problems,
    step 3 at least 5 (16x4_rk4: the 2 that solver_step_cases.NL_STEP3_COMPARED counts from the reference).

    Observed on an MI355X at FACTOR = 10 (problems compared per step; largest error / tolerance after 1 / 2 / 3 steps; the
    test prints both per row):
      2x1_h20    8 8 8   0.057 0.009 0.007      3x2_unity  8 8 5   0.000 0.000 0.000
      2x1_h63    8 8 8   0.101 0.091 0.031      5x2_h9     8 8 8   0.035 0.010 0.011
      6x3_rk4    8 8 7   0.019 0.010 0.006      6x3_fp32   8 8     0.299 0.194
      12x5_h4    8 8 8   0.004 0.005 0.005      40x10_h3   8 8 8   0.007 0.006 0.007
      20x4_h6    8 8 8   0.024 0.012 0.011      70x3_h2    8 8 6   0.006 0.007 0.006
      16x4_rk4   8 8 2   0.006 0.007 0.007
    No ratio is above 1, so the factor stays 10."""
    case = sc.nl_case(name)
    steps = sc.NL_ROWS[name][8]
    ref, lam_e = sc.nl_reference(name), _nl_lam_error(name)
    eng = case.engine()
    X0 = case.bind(eng, case.B)
    hx = case.H * case.nx
    bad = []
    worst, lam_max = np.zeros(steps), 0.0
    compared = np.zeros(steps, dtype=int)
    for k in case.kernels:
        for it in range(1, steps + 1):
            Z, st, _, d = eng.solve(X0, None, reg=sc.REG, max_iter=it, lq_kernel=k, return_duals=True)
            lam = _np(d["lam"])
            assert (_np(d["zl"]) == 0).all() and (_np(d["zu"]) == 0).all()
            nb = 0
            for b, (rp, _) in enumerate(ref):
                if any(np.abs(s["dz"]).max() < sc.STOP_STEP for s in rp[:it]):
                    continue
                nb += 1
                lam_ref = rp[it - 1]["lam"]
                lam_max = max(lam_max, float(np.abs(lam_ref).max()))
                tol = cert.lam_tolerance(lam_e[b][it - 1], lam_ref, FACTOR)
                e = np.abs(lam[b, :hx] - lam_ref).max()
                worst[it - 1] = max(worst[it - 1], e / tol)
                if not e <= tol:
                    bad.append(f"{k} b={b} after {it} steps: |lam - lam+| = {e:.3e} > {tol:.3e} (ratio {e / tol:.1f})")
            compared[it - 1] = nb
            assert nb == case.B if it <= 2 else nb >= sc.NL_STEP3_COMPARED.get(name, 5), (name, it, nb)
    print(f"[nl duals {name}] problems compared per step {compared.tolist()}, |lam+|inf up to {lam_max:.1f}, "
          f"error / tolerance per step {np.round(worst, 3).tolist()} (factor {FACTOR:g})")
    assert not bad, "\n".join(bad)


# --------------------------------------------------------------------------------------------------------------------
# 4. bounded QP: the returned point under the NumPy certificate
# --------------------------------------------------------------------------------------------------------------------
def _inf_norm(M):
    return float(np.abs(M).sum(axis=1).max())


def _stationarity_bound(prob, z, zl, zu, lb, ub, tol_step):
    """10 |W|inf tol_step (1 + |z|inf), W = objective Hessian + diag(zl / (z - lb) + zu / (ub - z)) of the returned values:
    the largest change of the stationarity residual a last step admitted by the stopping test can leave behind."""
    flo, fhi = np.isfinite(lb), np.isfinite(ub)
    dg = np.zeros(prob.n)
    dg[flo] += zl[flo] / (z[flo] - lb[flo])
    dg[fhi] += zu[fhi] / (ub[fhi] - z[fhi])
    return 10.0 * _inf_norm(prob.objective_hessian() + np.diag(dg)) * tol_step * (1.0 + np.abs(z).max())


@pytest.mark.parametrize("linesearch", ["loop", "deferred"])
@pytest.mark.parametrize("barrier", ["primal-dual", "primal"])
@pytest.mark.parametrize("name", list(sc.BOUNDED_ROWS))
def test_bounded_qp_solution_carries_a_kkt_certificate(name, barrier, linesearch):
    """The set-up of test_interior_point_ends_at_the_solution_of_the_bounded_qp, with the multipliers: from the RETURNED
    Z, lam, zl, zu the NumPy certificate gives r[3] == 0, r[1] <= tol_constraint inside the bounds, r[2] <= 10 mu_min,
    r[0] <= 10 |W|inf tol_step (1 + |z|inf); every active bound of the exact solution is identified with its multiplier
    and every other finite bound has a multiplier <= 10 mu_min / gap; the device evaluator agrees with the certificate.

    Observed on an MI355X (both line searches alike).  primal-dual: stationarity 1e-16 .. 5e-14 (2x1_h12 problem 0: 1.3e-6)
    against bounds of 3e1 .. 2e5, complementarity 1.0e-9 .. 2.5e-9, active multipliers within 1.2e-6, device evaluator
    within 5e-17 of the certificate.  primal barrier: stationarity 0.2 .. 1.4 against bounds of 6e1 .. 1e4 -- mu / gap with
    gaps of the order of tol_step is that inaccurate, and |W|inf, which holds zl / gap, says so; complementarity exactly
    mu_min.  The stationarity and multiplier bounds are loose by construction (|W|inf of an active bound is nu / gap ~ 1e7)."""
    mu_min, tol_step, tol_constraint = 1e-9, 1e-8, 1e-8
    case, lbe, ube, given = sc.bounded_case(name)
    ref = sc.bounded_reference(name)
    eng = case.engine()
    eng.set_box_rows(given["box_lo"], given["box_hi"])
    X0 = case.bind(eng, case.B)
    Zt, st, it, d = eng.solve(X0, None, reg=sc.REG, lb=given["lb"], ub=given["ub"], max_iter=400, barrier=barrier,
                              linesearch=linesearch, mu_min=mu_min, tol_step=tol_step, tol_constraint=tol_constraint,
                              return_duals=True)
    assert (st == 0).all(), (st.tolist(), it)
    r_dev, s_dev = eng.kkt_residual(Zt, X0, d["lam"], d["zl"], d["zu"], given["lb"], given["ub"], want_stat=True)
    r_dev, s_dev = _np(r_dev), _np(s_dev)
    Z, lam, zl, zu = _np(Zt), _np(d["lam"]), _np(d["zl"]), _np(d["zu"])
    H, nx, n = case.H, case.nx, case.n
    hx = H * nx
    assert (lam[:, hx:] == 0).all() and lam.shape == (case.B, 2 * hx)
    fails = []

    def check(ok, what):
        if not ok:
            fails.append(what)

    for b, (zs, lams, nlo, nhi) in enumerate(ref):
        prob = case.problem(b)
        r, s = cert.residuals(prob, Z[b], case.X0[b], lam[b, :hx], zl[b], zu[b], lbe, ube)
        tag = f"[bounded duals {name} {barrier} {linesearch}] b={b}:"
        r0_bound = _stationarity_bound(prob, Z[b], zl[b], zu[b], lbe, ube, tol_step)
        print(f"{tag} stationarity {r[0]:.3e} (bound {r0_bound:.3e}), primal {r[1]:.3e} (bound {tol_constraint:.1e}), "
              f"complementarity {r[2]:.3e} (bound {10 * mu_min:.1e}), dual {r[3]:.3e} (bound 0)")
        check(r[3] == 0.0, f"{tag} r[3] = {r[3]}")
        check(r[1] <= tol_constraint and (Z[b] >= lbe).all() and (Z[b] <= ube).all(), f"{tag} r[1] = {r[1]:.3e}")
        check(r[2] <= 10.0 * mu_min, f"{tag} r[2] = {r[2]:.3e} > {10 * mu_min:.1e}")
        check(r[0] <= r0_bound, f"{tag} r[0] = {r[0]:.3e} > {r0_bound:.3e}")
        # active-set identification
        act = np.concatenate([nlo[nlo > 0], nhi[nhi > 0]])
        assert act.min() >= sc.NU_MIN
        tol_z = 10.0 * (mu_min / act.min() + tol_step * (1.0 + np.abs(zs).max()))
        HJ = np.concatenate([prob.objective_hessian(), prob.jacobian(zs, case.X0[b]).T], axis=1)
        tol_nu = 10.0 * (r0_bound + _inf_norm(HJ) * tol_z)
        worst_act = worst_in = 0.0
        for ours, nu_ref, gap, fin in ((zl[b], nlo, Z[b] - lbe, np.isfinite(lbe)), (zu[b], nhi, ube - Z[b], np.isfinite(ube))):
            on = nu_ref > 0
            e_act = np.abs(ours[on] - nu_ref[on])
            worst_act = max(worst_act, float(e_act.max(initial=0.0)) / tol_nu)
            check((e_act <= tol_nu).all(), f"{tag} active multiplier off by {e_act.max(initial=0.0):.3e} > {tol_nu:.3e}")
            off = fin & ~on
            ratio = ours[off] * gap[off] / (10.0 * mu_min)
            worst_in = max(worst_in, float(ratio.max(initial=0.0)))
            check((ratio <= 1.0).all(), f"{tag} inactive multiplier x gap = {(ours[off] * gap[off]).max(initial=0.0):.3e} > {10 * mu_min:.1e}")
            check((ours[~fin] == 0).all(), f"{tag} multiplier on an infinite bound")
        print(f"{tag} {len(act)} active bounds, nu_min {act.min():.3e}; active multiplier error / tolerance {worst_act:.3e} "
              f"(tolerance {tol_nu:.3e}), inactive multiplier x gap / (10 mu_min) {worst_in:.3e}")
        # the device evaluator on the same values (box rows on the handle: a Problem with those rows and the caller's bounds)
        pbox = orc.Problem(case.net, H, nx, case.nu, sc.KINDS[case.integ], case.DT, box=(given["box_lo"], given["box_hi"]), **case.obj)
        r2, s2 = cert.residuals(pbox, Z[b], case.X0[b], lam[b], zl[b], zu[b], given["lb"], given["ub"])
        assert np.abs(r2 - r).max() <= 1e-15 * (1 + np.abs(r).max()) and np.abs(s2 - s).max() == 0.0
        ptol = PARITY_TOL["float64"]
        scale = 1.0 + np.abs(prob.gradient(Z[b])).max() + np.abs(prob.jacobian(Z[b], case.X0[b])).max() * np.abs(lam[b]).max()
        e_dev = max(np.abs(s_dev[b] - s).max() / scale, abs(r_dev[b, 0] - r[0]) / scale, abs(r_dev[b, 1] - r[1]),
                    abs(r_dev[b, 2] - r[2]), abs(r_dev[b, 3] - r[3]))
        print(f"{tag} device evaluator {r_dev[b].tolist()}, largest scaled difference {e_dev:.3e} (tolerance {ptol:.0e})")
        check(e_dev <= ptol, f"{tag} device evaluator differs by {e_dev:.3e}")
    assert not fails, "\n".join(fails)


# --------------------------------------------------------------------------------------------------------------------
# 5. compaction and slots
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("barrier", ["primal-dual", "primal"])
def test_duals_are_identical_with_and_without_compaction(barrier):
    """2/1 tanh 2 x 64, H = 20, B = 96 (compaction needs more than 64 active slots), bounded controls: Z, lam, zl, zu and the
    status are the same bits whether the unconverged problems were gathered to the front along the way or not -- finished
    problems keep the multipliers they finished with across later compactions -- and asking for the multipliers does not
    change Z."""
    from pyneuralempc_amd import CallbackEngine
    nx, nu, H, B = 2, 1, 20, 96
    net = orc.MLP.random(nx + nu, [64, 64], nx, seed=0)
    net.W[-1] *= 0.2
    net.b[-1] *= 0.2
    eng = CallbackEngine(net.W, net.b, H, nx, nu, integrator="discret", dtype=torch.float64, device="cuda:0", max_batch=B)
    X0 = eng.to_device(np.random.default_rng(4).uniform(-0.8, 0.8, size=(B, nx)))
    lb = np.concatenate([np.full(H * nx, -np.inf), np.full(H * nu, -0.5)])
    kw = dict(lb=lb, ub=-lb, max_iter=60, barrier=barrier, return_iterations=True)
    Za, sa, ia, pa, da = eng.solve(X0, compact=False, return_duals=True, **kw)
    Zb, sb, ib, pb, db = eng.solve(X0, compact=True, return_duals=True, **kw)
    Zc, sc_, ic, pc = eng.solve(X0, compact=True, **kw)
    assert ia == ib == ic and torch.equal(sa, sb) and torch.equal(pa, pb) and torch.equal(sa, sc_)
    assert torch.equal(Za, Zb) and torch.equal(Zb, Zc)
    for k in ("lam", "zl", "zu"):
        assert torch.equal(da[k], db[k]), k
    ok = (sa == 0).cpu().numpy()
    its = np.sort(pa.cpu().numpy()[ok])
    assert ok.sum() >= 3 * B // 4
    # a quarter of the batch has converged several iterations before the last problem: the compacting run did compact,
    # and more than once when the spread is wide
    assert its[B // 4] + 3 < ia, (its.tolist(), ia)
    zl, zu, lam = _np(da["zl"]), _np(da["zu"]), _np(da["lam"])
    assert (zl[:, :H * nx] == 0).all() and (zu[:, :H * nx] == 0).all()            # infinite bounds: exactly zero
    assert (zl[:, H * nx:] > 0).all() and (zu[:, H * nx:] > 0).all() and np.abs(lam).max() > 1e-3
    # the converged problems are KKT points by the device's own evaluator
    r = _np(eng.kkt_residual(Za, X0, da["lam"], da["zl"], da["zu"], lb, -lb))
    print(f"[compaction {barrier}] iterations {ia}, converged {int(ok.sum())}/{B}, convergence iterations {its[0]}..{its[-1]}, "
          f"largest residuals of the converged problems {r[ok].max(axis=0).tolist()}")
    assert (r[ok, 3] == 0).all() and (r[ok, 1] <= 1e-8).all()


# --------------------------------------------------------------------------------------------------------------------
# 6. the returned lam feeds the Hessian callback
# --------------------------------------------------------------------------------------------------------------------
def test_returned_multipliers_feed_the_hessian_callback_on_a_box_row_handle():
    case = sc.nl_case("2x1_h20")
    eng = case.engine()
    box = (-0.45, 0.45)
    eng.set_box_rows(*box)
    B, H, nx, nu = case.B, case.H, case.nx, case.nu
    X0 = case.bind(eng, B)
    lb = np.concatenate([np.full(H * nx, -np.inf), np.full(H * nu, -0.3)])
    Z, st, it, d = eng.solve(X0, None, reg=sc.REG, lb=lb, ub=-lb, max_iter=4, return_duals=True)
    lam = d["lam"]
    assert tuple(lam.shape) == (B, eng.m) and eng.m == 2 * H * nx
    assert (lam[:, H * nx:] == 0).all() and float(lam.abs().max()) > 1e-2
    hd = _np(eng.hess(Z, X0, lam, torch.ones(B, dtype=eng.dtype, device=eng.device), want=("hdense",))["hdense"])
    prob = orc.Problem(case.net, H, nx, nu, sc.KINDS[case.integ], case.DT, box=box, **case.obj)
    Zh, lamh = _np(Z), _np(lam)
    for b in range(B):
        refh = prob.lagrangian_hessian(Zh[b], case.X0[b], lamh[b], 1.0)
        np.testing.assert_allclose(hd[b], refh, rtol=0, atol=1e-9 * max(1.0, np.abs(refh).max()))     # (test_gpu_parity's)


# --------------------------------------------------------------------------------------------------------------------
# 7. next_batch / DeviceSqp plumbing
# --------------------------------------------------------------------------------------------------------------------
def test_next_batch_and_device_sqp_hand_the_multipliers_through():
    import pyneuralempc_amd as nEMPC
    m = dict(np.load(os.path.join(GOLDEN, "misc.npz")))
    W = [m[f"W{i}"] for i in range(3)]
    bs = [m[f"b{i}"] for i in range(3)]
    H = int(m["nmpc_H"])
    nx, nu = 2, 1
    n, hx = H * (nx + nu), H * nx
    model = nEMPC.model.MLPModel(W, bs, nx, nu, device="cuda:0")
    integ = nEMPC.integrator.discret.DiscretIntegrator(model, H)
    obj = nEMPC.objective.QuadraticObjective(Q=np.eye(2), R=0.1 * np.eye(1), device="cuda:0")
    dom = nEMPC.constraints.DomainConstraint(states_constraint=[[-5.0, 5.0]] * 2, control_constraint=[[-1.0, 1.0]])
    mpc = nEMPC.controller.NMPC(integ, obj, [dom], H, 1.0, optimizer=nEMPC.optimizer.Slsqp())
    X0 = np.stack([m["nmpc_x0"], m["nmpc_x1"]])
    plain = mpc.next_batch(X0)
    assert len(plain) == 3
    xs, us, st, duals = mpc.next_batch(X0, return_duals=True)
    assert st.tolist() == [0, 0] and np.array_equal(xs, plain[0]) and np.array_equal(us, plain[1]) and np.array_equal(st, plain[2])
    assert set(duals) == {"lam", "zl", "zu"}
    assert tuple(duals["lam"].shape) == (2, hx) and tuple(duals["zl"].shape) == tuple(duals["zu"].shape) == (2, n)
    assert all(t.is_cuda and t.dtype == torch.float64 for t in duals.values())
    assert float(duals["zl"].min()) > 0 and float(duals["zu"].min()) > 0          # every variable is bounded here

    ref_opt = nEMPC.optimizer.DeviceSqp()
    s0, u0 = nEMPC.controller.NMPC(integ, obj, [dom], H, 1.0, optimizer=ref_opt).next(m["nmpc_x0"])
    assert ref_opt.last_duals is None and ref_opt.last_kkt is None
    opt = nEMPC.optimizer.DeviceSqp(certificate=True)
    s1, u1 = nEMPC.controller.NMPC(integ, obj, [dom], H, 1.0, optimizer=opt).next(m["nmpc_x0"])
    assert np.array_equal(s0, s1) and np.array_equal(u0, u1)
    r = np.asarray(opt.last_kkt)
    assert r.shape == (4,) and np.isfinite(r).all() and r[3] == 0.0 and r[1] <= 1e-8
    dl = opt.last_duals
    assert dl["lam"].shape == (hx,) and dl["zl"].shape == dl["zu"].shape == (n,)
    z = np.concatenate([s1.ravel(), u1.ravel()])
    lb, ub = np.asarray(dom.get_lower_bounds(H), dtype=np.float64), np.asarray(dom.get_upper_bounds(H), dtype=np.float64)
    net = orc.MLP(W, bs)
    prob = orc.Problem(net, H, nx, nu, orc.DISCRET, 1.0, Q=np.eye(2), R=0.1 * np.eye(1))
    bound = _stationarity_bound(prob, z, dl["zl"], dl["zu"], lb, ub, 1e-8)
    r_ref, _ = cert.residuals(prob, z, m["nmpc_x0"], dl["lam"], dl["zl"], dl["zu"], lb, ub)
    print(f"[DeviceSqp certificate] last_kkt {r.tolist()}, NumPy certificate {r_ref.tolist()}, stationarity bound {bound:.3e}")
    assert r[0] <= bound
    assert np.abs(r - r_ref).max() <= PARITY_TOL["float64"] * (1.0 + np.abs(dl["lam"]).max())
