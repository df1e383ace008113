"""GPU: solution sensitivities dz*/dx0 and feedback gains (nempc_sensitivity, CallbackEngine.sensitivity).

Reference: tests/sensitivity_reference.py (NumPy float64).  Tolerances are not taken from the device:
  * tier A isolates the sweep kernel: the reference recursion is fed the DEVICE's own jac_tiles and hblocks (outputs of
    eng.eval / eng.hess with their own parity tests); fp64: max(10 e, 1e-12 (1 + |S|inf)), fp32 handles add
    4 * 2^-23 (1 + |S|inf) (the rounding of the stored result), e = |riccati - dense|inf of the float64 reference on those same
    inputs: what a correct double sweep loses;
  * tier B is end to end, fp64 handles: against `dense` on the oracle's own data,
    max(10 e, PARITY_TOL (1 + |S|inf) cond_gate), cond_gate = |dS|inf / (1e-11 |S|inf) of the reference when its stage data move
    relatively by 1e-11 (measured per problem, printed).
dlam is held to the same expressions with |dlam|inf in place of |S|inf.
"""
import os

import numpy as np
import pytest
import torch

from oracle import nempc_oracle as orc
from helpers import GOLDEN
import kkt_certificate as cert
import sensitivity_reference as sref
import solver_step_cases as sc

pytestmark = pytest.mark.gpu

PARITY_TOL = {"float64": 1e-11, "float32": 3e-4}     # tests/test_gpu_parity.py
BATCHES = (1, 3, 16, 17)
BOX = (-0.3, 0.4)
UBOUND = 0.6          # control bounds of the arbitrary points: wider than the +-0.5 the points are drawn from
ALL = ("du0", "dz", "dlam", "gains")


def _np(t):
    return t.detach().cpu().double().numpy()


def _wide_case(dtype):
    """12 states, 5 controls: nx^2 = 144 entries of a value matrix against the 64 lanes of a wave."""
    return sc.Case("12x5_h4", 12, 5, [16], "discret", 1.0, 4, ("auto",), dtype, act="tanh", seed=3, B=16, scale_b=True)


def _large_case(dims):
    """Linear networks at the sizes where the sweep kernel changes its plan (csrc/kernels_sens.hip, sens_plan): the working
    set of a problem is 3 nx^2 + 4 nx nu + nu^2 + 2 doubles against an LDS budget of 150 KiB per workgroup --
    40/10: 52 KB, two problems per workgroup; 64/8: 115 KB, one (and more than the 64 KiB a kernel gets by default);
    64/32: 172 KB, the per-problem region in global memory (64/64 would do as well, but R + R' of the seeded objective is
    not positive definite at 64 controls)."""
    nx, nu, H = dims
    return sc.Case(f"{nx}x{nu}_h{H}", nx, nu, [8], "discret", 1.0, H, ("auto",), "float64", act="linear", seed=sc.QP_SEED, B=16)


# id: (kind, row, H, handle keywords, box rows, tracking binding)
ROWS = {
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
    "3x8_H5": ("qp", "3x8_discret", 5, {}, False, False),              # (wide rows of the step tables: nu > nx,
    "20x4_H6": ("qp", "20x4_discret", 6, {}, False, False),            #  a 98 KB solver working set,
    "70x3_H2": ("qp", "70x3_discret", 2, {}, False, False),            #  more states than lanes)
    "tanh_2x1_h20": ("nl", "2x1_h20", 20, {}, False, False),
    "tanh_2x1_h20_valu": ("nl", "2x1_h20", 20, {"kernel": "valu"}, False, False),
    "tanh_2x1_h20_layered": ("nl", "2x1_h20", 20, {"kernel": "layered"}, False, False),
    "tanh_6x3_rk4": ("nl", "6x3_rk4", 8, {}, False, False),
    "tanh_2x1_h20_box": ("nl", "2x1_h20", 20, {}, True, False),
    "tanh_2x1_h20_tracking": ("nl", "2x1_h20", 20, {}, False, True),
    "tanh_12x5_h4": ("wide", "float64", 4, {}, False, False),
    "tanh_12x5_h4_fp32": ("wide", "float32", 4, {}, False, False),
    "40x10_two_per_workgroup": ("large", (40, 10, 3), 3, {}, False, False),
    "64x8_one_per_workgroup": ("large", (64, 8, 3), 3, {}, False, False),
    "64x32_global_scratch": ("large", (64, 32, 2), 2, {}, False, False),
}


def _tolerance(e, scale, dtype, tier_b_gate=None):
    """The module docstring's expressions; scale = 1 + |reference|inf."""
    if tier_b_gate is not None:
        return max(10.0 * e, PARITY_TOL["float64"] * scale * tier_b_gate)
    tol = max(10.0 * e, 1e-12 * scale)
    return tol + (4.0 * 2.0 ** -23 * scale if dtype == "float32" else 0.0)


def _tier_a(res, b, stage, H, nx, nu, sigma, dtype):
    """Device outputs of problem b against the float64 recursion on the same stage data.  -> (largest error / tolerance,
    reference verdict, its margin)."""
    ric = sref.riccati(stage, H, nx, nu, sigma)
    if not ric["pd"]:
        return None, False, ric["margin"]
    S, dl = sref.dense_stage(stage, H, nx, nu, sigma)
    eS, eL = np.abs(ric["S"] - S).max(), np.abs(ric["dlam"] - dl).max()
    worst = 0.0
    hx = H * nx
    for key, ref, e in (("dz", ric["S"], eS), ("dlam", ric["dlam"], eL), ("gains", ric["gains"], eS),
                        ("du0", ric["S"][hx:hx + nu], eS)):
        if key in res:
            scale = 1.0 + np.abs(ric["dlam"] if key == "dlam" else ric["S"]).max()
            worst = max(worst, np.abs(res[key][b] - ref).max() / _tolerance(e, scale, dtype))
    return worst, True, ric["margin"]


def _tier_b(res, b, prob, z, x0, lam, sigma):
    """Device outputs of problem b against the dense solve on the oracle's own data.  -> (error / tolerance, cond_gate)."""
    S, dl = sref.dense(prob, z, x0, lam, sigma)
    stage = sref.stage_data(prob, z, x0, lam)
    ric = sref.riccati(stage, prob.H, prob.nx, prob.nu, sigma)
    assert ric["pd"]
    eS, eL = np.abs(ric["S"] - S).max(), np.abs(ric["dlam"] - dl).max()
    rp = sref.riccati(sref.perturbed(stage, 1e-11, seed=b), prob.H, prob.nx, prob.nu, sigma)
    gate = max(1.0, np.abs(rp["S"] - ric["S"]).max() / (1e-11 * np.abs(ric["S"]).max()))
    gate_l = max(1.0, np.abs(rp["dlam"] - ric["dlam"]).max() / (1e-11 * np.abs(ric["dlam"]).max()))
    worst = np.abs(res["dz"][b] - S).max() / _tolerance(eS, 1.0 + np.abs(S).max(), "float64", gate)
    if "dlam" in res:
        worst = max(worst, np.abs(res["dlam"][b] - dl).max() / _tolerance(eL, 1.0 + np.abs(dl).max(), "float64", gate_l))
    return worst, gate


def _sens(eng, dev, lb, ub, want=ALL, mult=True):
    out = eng.sensitivity(dev[0], dev[1], dev[2], dev[3] if mult else None, dev[4] if mult else None, lb, ub, want=want)
    return {k: (v.cpu().numpy() if k == "status" else _np(v)) for k, v in out.items()}, out


# --------------------------------------------------------------------------------------------------------------------
# 1. arbitrary points, every output
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid", list(ROWS))
def test_sensitivities_match_the_reference_at_arbitrary_points(rid):
    """Random points (Z in +-0.5 like Case.Zrand, lam = N(0,1)), B in {1, 3, 16, 17} (partial workgroups; 17 grows the
    handle's workspaces): du0, dz, dlam, gains under tier A at every batch and tier B (fp64) at B = 17.  B = 1 runs without
    bounds (the multipliers given then count as zero), B = 3 with bounds and null zl / zu, the others with random positive
    multipliers on control bounds of +-0.6 (and, on the box-row handle, on the state limits too); multipliers on the
    unbounded states are given and must be ignored.  du0, dz's u_0 rows and gains[:, 0] are the same bits; asking for one
    output gives the bits of asking for all."""
    kind, row, H, kw, box, track = ROWS[rid]
    case = {"qp": lambda: sc.qp_case(row, H), "nl": lambda: sc.nl_case(row), "wide": lambda: _wide_case(row),
            "large": lambda: _large_case(row)}[kind]()
    nx, nu, n, hx, ne = case.nx, case.nu, case.n, H * case.nx, case.n_extra
    eng = case.engine(**kw)
    if box:
        eng.set_box_rows(*BOX)
    m = eng.m
    rnd = lambda a: sc._round(a, case.dtype)
    rng = np.random.default_rng(11)
    Bm = max(BATCHES)
    X0, Z = rnd(rng.uniform(-0.5, 0.5, size=(Bm, nx))), rnd(rng.uniform(-0.5, 0.5, size=(Bm, n)))
    if box:      # inside the box rows: every gap of a multiplied bound is positive
        Z[:, :hx] = rnd(rng.uniform(BOX[0] + 0.05, BOX[1] - 0.05, size=(Bm, hx)))
    lam, zl, zu = rnd(rng.normal(size=(Bm, m))), rnd(rng.uniform(0, 1, size=(Bm, n))), rnd(rng.uniform(0, 1, size=(Bm, n)))
    lb = np.concatenate([np.full(hx, -np.inf), np.full(H * nu, -UBOUND)])
    ub = -lb
    # what the call ends up with: the box rows are intersected into the state bounds, with or without lb / ub
    box_lb, box_ub = np.full(n, -np.inf), np.full(n, np.inf)
    if box:
        box_lb[:hx], box_ub[:hx] = BOX
    lbe, ube = np.maximum(lb, box_lb), np.minimum(ub, box_ub)
    extra = rnd(0.5 * rng.normal(size=(Bm, H, ne))) if ne else None
    per = {k: rnd(sc.REF_SCALE * rng.normal(size=(Bm, H, d))) for k, d in (("xref", nx), ("uref", nu), ("cx", nx), ("cu", nu))}

    def problem(b):
        return orc.Problem(case.net, H, nx, nu, sc.KINDS[case.integ], case.DT, extra=None if extra is None else extra[b], **case.obj)

    worst_a = worst_b = gate_max = 0.0
    for B in BATCHES:
        if ne:
            eng.bind_extra(eng.to_device(extra[:B]))
        if track:
            eng.bind_tracking(**{k: eng.to_device(v[:B]) for k, v in per.items()})
        use_lb, use_ub = (None, None) if B == 1 else (lb, ub)
        mult = B != 3
        dev = [eng.to_device(a[:B]) for a in (Z, X0, lam, zl, zu)]
        res, raw = _sens(eng, dev, use_lb, use_ub, ALL, mult)
        assert res["du0"].shape == (B, nu, nx) and res["dz"].shape == (B, n, nx) and res["dlam"].shape == (B, hx, nx)
        assert res["gains"].shape == (B, H, nu, nx) and res["status"].shape == (B,)
        tiles = _np(eng.eval(dev[0], dev[1], want=("jac_tiles",))["jac_tiles"])
        blocks = _np(eng.hess(dev[0], dev[1], dev[2], torch.ones(B, dtype=eng.dtype, device=eng.device), want=("hblocks",))["hblocks"])
        # the three copies of K_0, bit for bit; single outputs, bit for bit
        assert np.array_equal(res["du0"], res["dz"][:, hx:hx + nu]) and np.array_equal(res["du0"], res["gains"][:, 0])
        for key in ("du0", "dlam"):
            one, _ = _sens(eng, dev, use_lb, use_ub, (key,), mult)
            assert set(one) == {key, "status"} and np.array_equal(one[key], res[key]) and np.array_equal(one["status"], res["status"])
        for b in range(B):
            prob = problem(b)
            sigma = sref.sigma_of(Z[b], zl[b], zu[b], box_lb if B == 1 else lbe, box_ub if B == 1 else ube) if mult else None
            stage = sref.stage_data_from_tiles(prob, tiles[b], blocks[b])
            wa, pd, margin = _tier_a(res, b, stage, H, nx, nu, sigma, case.dtype)
            assert pd and res["status"][b] == 0, (rid, B, b, res["status"][b], margin)
            worst_a = max(worst_a, wa)
            if B == Bm and case.dtype == "float64":
                wb, gate = _tier_b(res, b, prob, Z[b], X0[b], lam[b, :hx], sigma)
                worst_b, gate_max = max(worst_b, wb), max(gate_max, gate)
    if track:
        eng.bind_tracking()
    print(f"[sensitivity {rid}] tier A error / tolerance {worst_a:.3e}, tier B error / tolerance {worst_b:.3e} "
          f"(cond_gate up to {gate_max:.3g})")
    assert worst_a <= 1.0 and worst_b <= 1.0


# --------------------------------------------------------------------------------------------------------------------
# 2. verdicts
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["2x1_h20", "6x3_rk4"])
def test_status_is_the_cholesky_verdict_of_the_reference(name):
    """Case.Zrand with lam_b = s_b N(0,1), s_b = (0, 1, 30, 300)[b % 4]: status equals the reference's verdict on every problem
    whose smallest reference pivot is farther than 1e-8 |Quu|inf from zero (the reference gives both verdicts: 2/1 positive
    definite at s in {0, 1} and not at {30, 300}; 6/3 not at 300 only); status-1 problems are all NaN, the others pass tier
    A in the same launch.  Then: z_i = ub_i with zu_i > 0 gives status 2 (all NaN), the same point with zu_i = 0 status 0."""
    case = sc.nl_case(name)
    H, nx, nu, n, hx, B = case.H, case.nx, case.nu, case.n, case.H * case.nx, case.B
    eng = case.engine()
    rng = np.random.default_rng(7)
    lam = np.stack([(0.0, 1.0, 30.0, 300.0)[b % 4] * rng.normal(size=hx) for b in range(B)])
    Z, X0 = case.Zrand[:B], case.X0[:B]
    dev = [eng.to_device(a) for a in (Z, X0, lam)]
    res, _ = _sens(eng, dev + [None, None], None, None, ALL, False)
    tiles = _np(eng.eval(dev[0], dev[1], want=("jac_tiles",))["jac_tiles"])
    blocks = _np(eng.hess(dev[0], dev[1], dev[2], torch.ones(B, dtype=eng.dtype, device=eng.device), want=("hblocks",))["hblocks"])
    verdicts, worst, decided = [], 0.0, 0
    for b in range(B):
        stage = sref.stage_data_from_tiles(case.problem(b), tiles[b], blocks[b])
        wa, pd, margin = _tier_a(res, b, stage, H, nx, nu, None, case.dtype)
        verdicts.append(pd)
        if margin > 1e-8:
            decided += 1
            assert res["status"][b] == (0 if pd else 1), (b, res["status"][b], pd, margin)
        if res["status"][b] == 1:
            assert all(np.isnan(res[k][b]).all() for k in ALL), b
        elif pd:
            worst = max(worst, wa)
    print(f"[sensitivity verdicts {name}] reference verdicts {verdicts}, device status {res['status'].tolist()}, "
          f"{decided} decided, tier A error / tolerance {worst:.3e}")
    expect = [s < 30.0 for s in (0.0, 1.0, 30.0, 300.0)] if name == "2x1_h20" else [True, True, True, False]
    assert verdicts == [expect[b % 4] for b in range(B)] and decided == B and worst <= 1.0
    # an undefined Sigma
    lb = np.concatenate([np.full(hx, -np.inf), np.full(H * nu, -UBOUND)])
    Zb = Z.copy()
    Zb[1, hx + 3] = UBOUND
    zu = np.zeros((B, n))
    zu[1, hx + 3] = 0.5
    lam0 = np.zeros((B, hx))
    d2 = [eng.to_device(a) for a in (Zb, X0, lam0, np.zeros((B, n)), zu)]
    r2, _ = _sens(eng, d2, lb, -lb, ALL, True)
    assert r2["status"].tolist() == [0, 2] + [0] * (B - 2)
    assert all(np.isnan(r2[k][1]).all() for k in ALL) and all(np.isfinite(r2[k][0]).all() and np.isfinite(r2[k][2:]).all() for k in ALL)
    zu[1, hx + 3] = 0.0
    d3 = [eng.to_device(a) for a in (Zb, X0, lam0, np.zeros((B, n)), zu)]
    r3, _ = _sens(eng, d3, lb, -lb, ALL, True)
    assert (r3["status"] == 0).all() and all(np.isfinite(r3[k]).all() for k in ALL)


# --------------------------------------------------------------------------------------------------------------------
# 3. at solver solutions
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [k for k, v in sc.NL_ROWS.items() if v[7] == "float64"])
def test_sensitivities_at_solver_solutions(name):
    """Unbounded solves of the tanh rows (max_iter = 200, the library's fp64 tolerances): tier B at the returned point with
    the returned multipliers, statuses all 0."""
    case = sc.nl_case(name)
    H, nx, hx, B = case.H, case.nx, case.H * case.nx, case.B
    eng = case.engine()
    X0 = case.bind(eng, B)
    Zt, st, it, d = eng.solve(X0, None, reg=sc.REG, max_iter=200, return_duals=True)
    assert (st == 0).all(), (st.tolist(), it)
    out = eng.sensitivity(Zt, X0, d["lam"], d["zl"], d["zu"], want=("dz", "dlam", "du0"))
    res = {k: (v.cpu().numpy() if k == "status" else _np(v)) for k, v in out.items()}
    assert (res["status"] == 0).all(), res["status"].tolist()
    Z, lam = _np(Zt), _np(d["lam"])
    worst = gate_max = 0.0
    for b in range(B):
        wb, gate = _tier_b(res, b, case.problem(b), Z[b], case.X0[b], lam[b, :hx], None)
        worst, gate_max = max(worst, wb), max(gate_max, gate)
    print(f"[sensitivity at solutions {name}] {it} iterations, tier B error / tolerance {worst:.3e} (cond_gate up to {gate_max:.3g}), "
          f"|K0|inf {np.abs(res['du0']).max():.3g}")
    assert worst <= 1.0


# --------------------------------------------------------------------------------------------------------------------
# 4. bounded QP
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.BOUNDED_SMALL))      # (why not the wide rows: solver_step_cases.BOUNDED_SMALL)
def test_bounded_qp_sensitivities_approach_the_active_set_limit(name):
    """The set-up of test_bounded_qp_solution_carries_a_kkt_certificate (primal-dual, mu_min = 1e-9) at the returned
    (Z, lam, zl, zu): tier B with sigma_of(...); then the device result against `active_set` of the exact solution within
    10 gap + tier-B tolerance, gap = |dense(Sigma) - active_set|inf of the float64 reference at central_path_point(mu = r[2]),
    r[2] the problem's complementarity by the NumPy certificate (the solver's point is within a factor of the central
    path: each zl d <= 10 mu_min).  Rows of dZ of controls in the reference's active set are below that bound; 2x1_h12 has
    u_0 clamped in all four problems (K0 near zero), 3x2_h7 has a non-zero K0 -- both against the reference."""
    mu_min = 1e-9
    case, lbe, ube, given = sc.bounded_case(name)
    ref = sc.bounded_reference(name)
    H, nx, nu, hx = case.H, case.nx, case.nu, case.H * case.nx
    eng = case.engine()
    eng.set_box_rows(given["box_lo"], given["box_hi"])
    X0 = case.bind(eng, case.B)
    Zt, st, it, d = eng.solve(X0, None, reg=sc.REG, lb=given["lb"], ub=given["ub"], max_iter=400, barrier="primal-dual",
                              mu_min=mu_min, tol_step=1e-8, tol_constraint=1e-8, return_duals=True)
    assert (st == 0).all(), (st.tolist(), it)
    out = eng.sensitivity(Zt, X0, d["lam"], d["zl"], d["zu"], given["lb"], given["ub"], want=("dz", "du0"))
    res = {k: (v.cpu().numpy() if k == "status" else _np(v)) for k, v in out.items()}
    assert (res["status"] == 0).all(), res["status"].tolist()
    Z, lam, zl, zu = _np(Zt), _np(d["lam"]), _np(d["zl"]), _np(d["zu"])
    fails, k0 = [], []
    for b, rf in enumerate(ref):
        prob, x0 = case.problem(b), case.X0[b]
        sigma = sref.sigma_of(Z[b], zl[b], zu[b], lbe, ube)
        wb, gate = _tier_b(res, b, prob, Z[b], x0, lam[b, :hx], sigma)
        r, _ = cert.residuals(prob, Z[b], x0, lam[b, :hx], zl[b], zu[b], lbe, ube)
        act = (rf[2] > 0) | (rf[3] > 0)
        Sa, _ = sref.active_set(prob, rf[0], x0, rf[1], act)
        zc, lc, zlc, zuc = sref.central_path_point(rf, lbe, ube, r[2])
        Sc, _ = sref.dense(prob, zc, x0, lc, sref.sigma_of(zc, zlc, zuc, lbe, ube))
        gap = np.abs(Sc - Sa).max()
        Sd, _ = sref.dense(prob, Z[b], x0, lam[b, :hx], sigma)
        ric = sref.riccati_at(prob, Z[b], x0, lam[b, :hx], sigma)
        tol_b = _tolerance(np.abs(ric["S"] - Sd).max(), 1.0 + np.abs(Sd).max(), "float64", gate)
        bound = 10.0 * gap + tol_b
        err = np.abs(res["dz"][b] - Sa).max()
        rows = np.abs(res["dz"][b][act]).max()
        k0.append((np.abs(res["du0"][b]).max(), np.abs(Sa[hx:hx + nu]).max(), bool(act[hx:hx + nu].all()), bound))
        print(f"[sensitivity bounded {name}] b={b}: complementarity {r[2]:.2e}, tier B error / tolerance {wb:.3e} (cond_gate {gate:.3g}), "
              f"gap {gap:.2e}, bound {bound:.2e}, |device - active set| {err:.2e}, active rows {rows:.2e}, |K0| {k0[-1][0]:.3g}")
        if wb > 1.0:
            fails.append(f"b={b}: tier B {wb:.3e}")
        if err > bound:
            fails.append(f"b={b}: |device - active set| {err:.3e} > {bound:.3e}")
        if rows > bound:
            fails.append(f"b={b}: rows of active variables {rows:.3e} > {bound:.3e}")
    assert not fails, "\n".join(fails)
    if name == "2x1_h12":
        # u_0 is clamped in the reference's solution of all four problems: its K0 is exactly zero, the device's below the bound
        assert all(c and ref0 == 0.0 and dev0 <= bd for dev0, ref0, c, bd in k0), k0
    else:
        assert all(ref0 > 1e-2 and abs(dev0 - ref0) <= bd for dev0, ref0, _, bd in k0), k0


# --------------------------------------------------------------------------------------------------------------------
# 5. refusals and plumbing
# --------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from pyneuralempc_amd._lib import NempcError
    import ctypes
    case = sc.qp_case("roll3_fwd", 10)
    eng = case.engine()
    B = 3
    X0 = case.bind(eng, B)
    Z = eng.to_device(case.Zrand[:B])
    lam = torch.zeros(B, eng.m, dtype=eng.dtype, device=eng.device)
    with pytest.raises(NempcError) as e1:
        eng.sensitivity(Z, X0, lam)
    assert e1.value.code == -5 and "rolling_window" in str(e1.value)
    Zs, st, _ = eng.solve(X0, None, reg=sc.REG, max_iter=30)
    assert (st == 0).all()
    zref = sc.qp_reference("roll3_fwd", 10)
    for b in range(B):
        z0, dz, _, tolz, _ = zref[b]
        assert np.abs(_np(Zs)[b] - (z0 + dz)).max() <= tolz
    # a batch larger than a binding covers
    case = sc.qp_case("2x1_extras", 10)
    eng = case.engine()
    X0 = case.bind(eng, 4)
    Z = eng.to_device(case.Zrand[:4])
    lam = torch.zeros(4, eng.m, dtype=eng.dtype, device=eng.device)
    eng.bind_extra(eng.to_device(case.extra[:2]))
    status = torch.zeros(4, dtype=torch.int32, device=eng.device)
    du0 = torch.zeros(4, case.nu, case.nx, dtype=eng.dtype, device=eng.device)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = eng.lib.nempc_sensitivity(eng._handle, 4, vp(Z), vp(X0), vp(lam), None, None, None, None, vp(du0), None, None, None,
                                   vp(status), None)
    assert rc == -1 and b"exceeds the batch" in eng.lib.nempc_last_error()
    # no output asked for
    rc = eng.lib.nempc_sensitivity(eng._handle, 2, vp(Z), vp(X0), vp(lam), None, None, None, None, None, None, None, None,
                                   vp(status), None)
    assert rc == -1 and b"no output" in eng.lib.nempc_last_error()
    with pytest.raises(ValueError):
        eng.sensitivity(Z[:2], X0[:2], lam[:2], want=())
    torch.cuda.synchronize()


def test_a_solve_after_a_sensitivity_call_is_bit_identical():
    """The call's buffers are the handle's, not the solver's."""
    case = sc.nl_case("6x3_rk4")
    eng = case.engine()
    X0 = case.bind(eng, case.B)
    lb = np.concatenate([np.full(case.H * case.nx, -np.inf), np.full(case.H * case.nu, -0.3)])
    Za, sa, ia, da = eng.solve(X0, None, reg=sc.REG, lb=lb, ub=-lb, max_iter=40, return_duals=True)
    out = eng.sensitivity(Za, X0, da["lam"], da["zl"], da["zu"], lb, -lb, want=ALL)
    assert int(out["status"].max()) == 0
    Zb, sb, ib, db = eng.solve(X0, None, reg=sc.REG, lb=lb, ub=-lb, max_iter=40, return_duals=True)
    assert ia == ib and torch.equal(Za, Zb) and torch.equal(sa, sb) and all(torch.equal(da[k], db[k]) for k in da)


def test_next_batch_and_device_sqp_hand_the_gain_through():
    import pyneuralempc_amd as nEMPC
    from pyneuralempc_amd.optimizer.base import fused_evaluator
    m = dict(np.load(os.path.join(GOLDEN, "misc.npz")))
    W = [m[f"W{i}"] for i in range(3)]
    bs = [m[f"b{i}"] for i in range(3)]
    H = int(m["nmpc_H"])
    nx, nu = 2, 1
    model = nEMPC.model.MLPModel(W, bs, nx, nu, device="cuda:0")
    integ = nEMPC.integrator.discret.DiscretIntegrator(model, H)
    obj = nEMPC.objective.QuadraticObjective(Q=np.eye(2), R=0.1 * np.eye(1), device="cuda:0")
    dom = nEMPC.constraints.DomainConstraint(states_constraint=[[-5.0, 5.0]] * 2, control_constraint=[[-1.0, 1.0]])
    mpc = nEMPC.controller.NMPC(integ, obj, [dom], H, 1.0, optimizer=nEMPC.optimizer.Slsqp())
    X0 = np.stack([m["nmpc_x0"], m["nmpc_x1"]])
    plain = mpc.next_batch(X0)
    xs, us, st, K0 = mpc.next_batch(X0, return_gain=True)
    assert len(plain) == 3 and np.array_equal(xs, plain[0]) and np.array_equal(us, plain[1]) and st.tolist() == [0, 0]
    assert isinstance(K0, np.ndarray) and K0.shape == (2, nu, nx) and mpc.last_gain_status.tolist() == [0, 0]
    xs2, us2, st2, duals, K0b = mpc.next_batch(X0, return_duals=True, return_gain=True)
    assert np.array_equal(K0, K0b) and set(duals) == {"lam", "zl", "zu"}
    eng = fused_evaluator(integ, obj, None).engine
    lb, ub = np.asarray(dom.get_lower_bounds(H), dtype=np.float64), np.asarray(dom.get_upper_bounds(H), dtype=np.float64)
    Zd = eng.to_device(np.concatenate([xs2.reshape(2, -1), us2.reshape(2, -1)], axis=1))
    direct = eng.sensitivity(Zd, eng.to_device(X0), duals["lam"], duals["zl"], duals["zu"], lb, ub)
    assert np.array_equal(_np(direct["du0"]), K0)
    # the gain predicts the first control of a neighbouring solve to first order
    delta = 1e-3 * np.array([[1.0, -0.5], [0.3, 1.0]])
    _, us3, st3 = mpc.next_batch(X0 + delta)
    pred = us[:, 0] + np.einsum("bij,bj->bi", K0, delta)
    assert st3.tolist() == [0, 0] and np.abs(us3[:, 0] - pred).max() <= 1e-4 * (1.0 + np.abs(K0).max()), (us3[:, 0], pred)

    opt = nEMPC.optimizer.DeviceSqp()
    nEMPC.controller.NMPC(integ, obj, [dom], H, 1.0, optimizer=opt).next(m["nmpc_x0"])
    assert opt.last_gain is None and opt.last_gain_status is None
    opt = nEMPC.optimizer.DeviceSqp(gain=True)
    nEMPC.controller.NMPC(integ, obj, [dom], H, 1.0, optimizer=opt).next(m["nmpc_x0"])
    assert opt.last_gain.shape == (nu, nx) and opt.last_gain_status == 0 and np.isfinite(opt.last_gain).all()
    assert np.abs(opt.last_gain - K0[0]).max() <= 1e-6 * (1.0 + np.abs(K0[0]).max())
