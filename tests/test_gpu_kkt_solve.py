"""GPU: KKT solves with caller-supplied right-hand sides (nempc_kkt_solve, CallbackEngine.kkt_solve) and torch autograd through
the batched solver (pyneuralempc_amd.autograd).

Reference: tests/kkt_solve_reference.py (NumPy float64).  Tolerances are the tier-A / tier-B expressions of
tests/test_gpu_sensitivity.py with |v|inf, |w|inf in place of |S|inf, |dlam|inf; none is taken from the device:
  * tier A isolates the sweep kernel: the reference recursion is fed the DEVICE's own jac_tiles and hblocks;
    fp64: max(10 e, 1e-12 scale), fp32 handles add 4 * 2^-23 scale (the rounding of the stored result),
    e = |affine_riccati - dense_solve|inf of the float64 reference on those same inputs: what a correct double sweep loses;
  * tier B is end to end, fp64 handles: against `dense_solve` on the oracle's own data,
    max(10 e, PARITY_TOL scale cond_gate), cond_gate = |dv|inf / (1e-11 |v|inf) of the reference when its stage data move
    relatively by 1e-11 (measured per problem, printed).
scale is 1 + |v|inf for v and 1 + |w|inf for w.  gx0 = -(W_ux,0' v_u[0] + A_0' w_0) is formed from both, so its e is measured on
gx0 itself and its scale is 1 + |v|inf + |w|inf.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import nempc_oracle as orc
import kkt_solve_reference as kref
import sensitivity_reference as sref
import solver_step_cases as sc

pytestmark = pytest.mark.gpu

PARITY_TOL = {"float64": 1e-11, "float32": 3e-4}     # tests/test_gpu_parity.py
BATCHES = (1, 3, 16, 17)
NRHS = (1, 3, 64)
BOX = (-0.3, 0.4)
UBOUND = 0.6          # control bounds of the arbitrary points: wider than the +-0.5 the points are drawn from
ALL = ("v", "w", "gx0")


def _np(t):
    return t.detach().cpu().double().numpy()


def _wide_case(dtype):
    """12 states, 5 controls: nx^2 = 144 entries of a value matrix against the 64 lanes of a wave."""
    return sc.Case("12x5_h4", 12, 5, [16], "discret", 1.0, 4, ("auto",), dtype, act="tanh", seed=3, B=16, scale_b=True)


def _large_case(dims):
    """Linear networks at the sizes where the kernel changes its plan (the cases of tests/test_gpu_sensitivity.py)."""
    nx, nu, H = dims
    return sc.Case(f"{nx}x{nu}_h{H}", nx, nu, [8], "discret", 1.0, H, ("auto",), "float64", act="linear", seed=sc.QP_SEED, B=16)


# id: (kind, row, H, handle keywords, box rows, tracking binding)
ROWS = {
    "2x1_H1": ("qp", "2x1_discret", 1, {}, False, False),
    "2x1_H2": ("qp", "2x1_discret", 2, {}, False, False),
    "2x1_H3": ("qp", "2x1_discret", 3, {}, False, False),
    "2x1_H20": ("qp", "2x1_discret", 20, {}, False, False),
    "6x3_rk4_H8": ("qp", "6x3_rk4", 8, {}, False, False),
    "3x2_unity_H7": ("qp", "3x2_unity", 7, {}, False, False),
    "2x1_extras": ("qp", "2x1_extras", 10, {}, False, False),
    "2x1_fp32": ("qp", "2x1_fp32", 20, {}, False, False),
    "3x8_H5": ("qp", "3x8_discret", 5, {}, False, False),              # (wide rows of the step tables: nu > nx,
    "20x4_H6": ("qp", "20x4_discret", 6, {}, False, False),            #  a 98 KB solver working set,
    "70x3_H2": ("qp", "70x3_discret", 2, {}, False, False),            #  more states than lanes)
    "tanh_2x1_h20": ("nl", "2x1_h20", 20, {}, False, False),
    "tanh_2x1_h20_valu": ("nl", "2x1_h20", 20, {"kernel": "valu"}, False, False),
    "tanh_2x1_h20_layered": ("nl", "2x1_h20", 20, {"kernel": "layered"}, False, False),
    "tanh_2x1_h20_box": ("nl", "2x1_h20", 20, {}, True, False),
    "tanh_2x1_h20_tracking": ("nl", "2x1_h20", 20, {}, False, True),
    "tanh_12x5_h4": ("wide", "float64", 4, {}, False, False),
    "tanh_12x5_h4_fp32": ("wide", "float32", 4, {}, False, False),
}


def _tolerance(e, scale, dtype, tier_b_gate=None):
    """The module docstring's expressions."""
    if tier_b_gate is not None:
        return max(10.0 * e, PARITY_TOL["float64"] * scale * tier_b_gate)
    tol = max(10.0 * e, 1e-12 * scale)
    return tol + (4.0 * 2.0 ** -23 * scale if dtype == "float32" else 0.0)


def _scales(d):
    sv, sw = 1.0 + np.abs(d["v"]).max(), 1.0 + np.abs(d["w"]).max()
    return {"v": sv, "w": sw, "gx0": sv + sw - 1.0}


def _tier_a(res, b, stage, H, nx, nu, sigma, dtype, rz, rg):
    """Device outputs of problem b against the float64 recursion on the same stage data.  -> (largest error / tolerance,
    reference verdict, its margin, {key: tolerance})."""
    ric = kref.affine_riccati(stage, H, nx, nu, sigma, rz, rg)
    if not ric["pd"]:
        return None, False, ric["margin"], None
    d = kref.dense_solve(stage, H, nx, nu, sigma, rz, rg)
    scales = _scales(d)
    tols = {k: _tolerance(np.abs(ric[k] - d[k]).max(), scales[k], dtype) for k in ALL}
    worst = max(np.abs(res[k][b] - ric[k]).max() / tols[k] for k in ALL if k in res)
    return worst, True, ric["margin"], tols


def _tier_b(res, b, prob, z, x0, lam, sigma, rz, rg, keys=ALL):
    """Device outputs of problem b against the dense solve on the oracle's own data.  -> (error / tolerance, cond_gate)."""
    H, nx, nu = prob.H, prob.nx, prob.nu
    stage = sref.stage_data(prob, z, x0, lam)
    d = kref.dense_solve(stage, H, nx, nu, sigma, rz, rg)
    ric = kref.affine_riccati(stage, H, nx, nu, sigma, rz, rg)
    assert ric["pd"]
    rp = kref.affine_riccati(sref.perturbed(stage, 1e-11, seed=b), H, nx, nu, sigma, rz, rg)
    gates = {k: max(1.0, np.abs(rp[k] - ric[k]).max() / (1e-11 * np.abs(ric[k]).max())) for k in ALL}
    scales = _scales(d)
    worst = max(np.abs(res[k][b] - d[k]).max() / _tolerance(np.abs(ric[k] - d[k]).max(), scales[k], "float64", gates[k])
                for k in keys if k in res)
    return worst, max(gates.values())


def _solve(eng, dev, lb, ub, rz, rg, want=ALL, mult=True):
    out = eng.kkt_solve(dev[0], dev[1], dev[2], dev[3] if mult else None, dev[4] if mult else None, lb, ub,
                        rz=eng.to_device(rz), rg=None if rg is None else eng.to_device(rg), want=want)
    return {k: (v.cpu().numpy() if k == "status" else _np(v)) for k, v in out.items()}


def _stage_inputs(eng, dev, B):
    tiles = _np(eng.eval(dev[0], dev[1], want=("jac_tiles",))["jac_tiles"])
    blocks = _np(eng.hess(dev[0], dev[1], dev[2], torch.ones(B, dtype=eng.dtype, device=eng.device), want=("hblocks",))["hblocks"])
    return tiles, blocks


# --------------------------------------------------------------------------------------------------------------------
# 1. arbitrary points, every output
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid", list(ROWS))
def test_solves_match_the_reference_at_arbitrary_points(rid):
    """Random points (Z in +-0.5 like Case.Zrand, lam = N(0,1)), B in {1, 3, 16, 17} x nrhs in {1, 3, 64} with N(0,1) right-hand
    sides: v, w, gx0 under tier A at every batch and tier B (fp64) at B = 17.  Bounds and multipliers per batch as in the
    sensitivity test (B = 1 unbounded, B = 3 bounds with null zl / zu, the others random positive multipliers on control
    bounds of +-0.6 and, on the box-row handle, on the state limits); rg is NULL at B = 3 and random at the others.
    Asking for one output gives the bits of asking for all.  nrhs = 3 equals three nrhs = 1 calls TO THE BIT: the arithmetic
    of a right-hand side reads only its own column of the working set, the library is built without floating-point
    contraction, and all these shapes stay on the LDS plans (one instantiation of the recursion), so neither the number of
    right-hand sides nor the problems per workgroup can change a rounding."""
    kind, row, H, kw, box, track = ROWS[rid]
    case = {"qp": lambda: sc.qp_case(row, H), "nl": lambda: sc.nl_case(row), "wide": lambda: _wide_case(row)}[kind]()
    nx, nu, n, hx, ne = case.nx, case.nu, case.n, H * case.nx, case.n_extra
    eng = case.engine(**kw)
    if box:
        eng.set_box_rows(*BOX)
    m = eng.m
    rnd = lambda a: sc._round(a, case.dtype)
    rng = np.random.default_rng(11)
    Bm, km = max(BATCHES), max(NRHS)
    X0, Z = rnd(rng.uniform(-0.5, 0.5, size=(Bm, nx))), rnd(rng.uniform(-0.5, 0.5, size=(Bm, n)))
    if box:      # inside the box rows: every gap of a multiplied bound is positive
        Z[:, :hx] = rnd(rng.uniform(BOX[0] + 0.05, BOX[1] - 0.05, size=(Bm, hx)))
    lam, zl, zu = rnd(rng.normal(size=(Bm, m))), rnd(rng.uniform(0, 1, size=(Bm, n))), rnd(rng.uniform(0, 1, size=(Bm, n)))
    RZ, RG = rnd(rng.normal(size=(Bm, km, n))), rnd(rng.normal(size=(Bm, km, hx)))
    lb = np.concatenate([np.full(hx, -np.inf), np.full(H * nu, -UBOUND)])
    ub = -lb
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
        tiles, blocks = _stage_inputs(eng, dev, B)
        stages = [sref.stage_data_from_tiles(problem(b), tiles[b], blocks[b]) for b in range(B)]
        sigmas = [sref.sigma_of(Z[b], zl[b], zu[b], box_lb if B == 1 else lbe, box_ub if B == 1 else ube) if mult else None
                  for b in range(B)]
        by_k = {}
        for k in NRHS:
            rz, rg = RZ[:B, :k], (None if B == 3 else RG[:B, :k])
            res = _solve(eng, dev, use_lb, use_ub, rz, rg, ALL, mult)
            by_k[k] = res
            assert res["v"].shape == (B, k, n) and res["w"].shape == (B, k, hx) and res["gx0"].shape == (B, k, nx)
            assert res["status"].shape == (B,)
            for b in range(B):
                wa, pd, margin, _ = _tier_a(res, b, stages[b], H, nx, nu, sigmas[b], case.dtype, rz[b], None if rg is None else rg[b])
                assert pd and res["status"][b] == 0, (rid, B, k, b, res["status"][b], margin)
                worst_a = max(worst_a, wa)
                if B == Bm and case.dtype == "float64":
                    wb, gate = _tier_b(res, b, problem(b), Z[b], X0[b], lam[b, :hx], sigmas[b], rz[b], None if rg is None else rg[b])
                    worst_b, gate_max = max(worst_b, wb), max(gate_max, gate)
        # single outputs, bit for bit; one right-hand side at a time, bit for bit (a 2-D rz loses the axis)
        rz3, rg3 = RZ[:B, :3], (None if B == 3 else RG[:B, :3])
        for key in ("v", "gx0"):
            one = _solve(eng, dev, use_lb, use_ub, rz3, rg3, (key,), mult)
            assert set(one) == {key, "status"} and np.array_equal(one[key], by_k[3][key]) and np.array_equal(one["status"], by_k[3]["status"])
        for c in range(3):
            one = _solve(eng, dev, use_lb, use_ub, np.ascontiguousarray(rz3[:, c]), None if rg3 is None else np.ascontiguousarray(rg3[:, c]),
                         ALL, mult)
            assert one["v"].shape == (B, n) and all(np.array_equal(one[key], by_k[3][key][:, c]) for key in ALL), (rid, B, c)
        assert all(np.array_equal(by_k[3][key], by_k[64][key][:, :3]) and np.array_equal(by_k[1][key], by_k[64][key][:, :1]) for key in ALL)
    if track:
        eng.bind_tracking()
    print(f"[kkt_solve {rid}] tier A error / tolerance {worst_a:.3e}, tier B error / tolerance {worst_b:.3e} "
          f"(cond_gate up to {gate_max:.3g})")
    assert worst_a <= 1.0 and worst_b <= 1.0


def test_more_than_64_right_hand_sides_go_in_chunks():
    """k = 130 right-hand sides (64 + 64 + 2): the bits of the three calls made by hand."""
    case = sc.qp_case("2x1_discret", 3)
    eng = case.engine()
    B, rng = 3, np.random.default_rng(2)
    dev = [eng.to_device(a) for a in (case.Zrand[:B], case.X0[:B], rng.normal(size=(B, eng.m)), np.zeros((B, case.n)), np.zeros((B, case.n)))]
    rz, rg = rng.normal(size=(B, 130, case.n)), rng.normal(size=(B, 130, case.H * case.nx))
    res = _solve(eng, dev, None, None, rz, rg, ALL, False)
    assert res["v"].shape == (B, 130, case.n) and (res["status"] == 0).all()
    for c0, c1 in ((0, 64), (64, 128), (128, 130)):
        part = _solve(eng, dev, None, None, np.ascontiguousarray(rz[:, c0:c1]), np.ascontiguousarray(rg[:, c0:c1]), ALL, False)
        assert all(np.array_equal(part[k], res[k][:, c0:c1]) for k in ALL)


# --------------------------------------------------------------------------------------------------------------------
# 2. symmetry against the shipped kernel
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["2x1_h20", "6x3_rk4"])
def test_identity_right_hand_sides_give_the_rows_of_the_shipped_sensitivities(name):
    """rz = the n identity rows (chunks of 64 inside the engine), rg = 0, at Case.Zrand with lam = N(0,1): gx0[b, i, :] equals
    eng.sensitivity(want = dz)[b, i, :] within the SUM of the two kernels' tier-A tolerances on the device's own tiles and
    blocks (K is symmetric: row i of K^-1 applied to the x0 right-hand side)."""
    case = sc.nl_case(name)
    H, nx, nu, n, hx, B = case.H, case.nx, case.nu, case.n, case.H * case.nx, 4
    eng = case.engine()
    rng = np.random.default_rng(5)
    lam = rng.normal(size=(B, hx))
    dev = [eng.to_device(a) for a in (case.Zrand[:B], case.X0[:B], lam)]
    rz = np.repeat(np.eye(n)[None], B, axis=0)
    res = _solve(eng, dev + [None, None], None, None, rz, None, ("gx0",), False)
    dz = _np(eng.sensitivity(dev[0], dev[1], dev[2], want=("dz",))["dz"])
    assert (res["status"] == 0).all() and res["gx0"].shape == (B, n, nx) == dz.shape
    tiles, blocks = _stage_inputs(eng, dev, B)
    worst = 0.0
    for b in range(B):
        stage = sref.stage_data_from_tiles(case.problem(b), tiles[b], blocks[b])
        _, pd, _, tols = _tier_a(res, b, stage, H, nx, nu, None, case.dtype, rz[b], None)
        ric = sref.riccati(stage, H, nx, nu, None)
        S, _ = sref.dense_stage(stage, H, nx, nu, None)
        tol_s = _tolerance(np.abs(ric["S"] - S).max(), 1.0 + np.abs(ric["S"]).max(), case.dtype)
        assert pd and ric["pd"]
        worst = max(worst, np.abs(res["gx0"][b] - dz[b]).max() / (tols["gx0"] + tol_s))
    print(f"[kkt_solve symmetry {name}] |gx0(e_i) - dz_i/dx0| / (sum of the tier-A tolerances) {worst:.3e}")
    assert worst <= 1.0


# --------------------------------------------------------------------------------------------------------------------
# 3. plan boundaries
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,nrhs,plan", [((40, 10, 3), 1, "two per workgroup"), ((40, 10, 3), 16, "one per workgroup"),
                                            ((40, 10, 3), 64, "global"), ((64, 8, 3), 1, "one per workgroup"),
                                            ((64, 8, 3), 12, "global"), ((64, 32, 2), 1, "global"), ((64, 32, 2), 12, "global")])
def test_plan_boundaries(dims, nrhs, plan):
    """The linear cases of the sensitivity test where kktsolve_plan (csrc/kernels_kktsolve.hip) changes.  Per problem the plan
    counts 8 (3 nx^2 + 4 nx nu + nu^2 + 2) bytes of sens_layout plus 8 nrhs (H (nx + nu) + 3 nx + nu) bytes of kktsolve_layout
    against kLqLdsBudget = 153600 bytes per workgroup:
        40/10 H3:  52016 + 2240 nrhs   nrhs = 1: 54256, two problems per workgroup; nrhs = 16: 87856, one; nrhs = 64: 195376,
                                       both working sets in the per-problem region of global memory
        64/8  H3: 115216 + 3328 nrhs   nrhs = 1: 118544, one problem per workgroup (more LDS than the 64 KiB a kernel gets
                                       by default); nrhs = 12: 155152, global
        64/32 H2: 172048 + 3328 nrhs   global at every nrhs; nrhs = 12 after nrhs = 1 on one handle grows the region
    B = 3 (partial workgroups), bounds with multipliers on the controls, random rg: v, w, gx0 under tier A.  Where two plans
    of a shape run (the parameters above, fresh handles), each is held to the reference, not to the other."""
    nx, nu, H = dims
    case = _large_case(dims)
    n, hx, B = case.n, H * nx, 3
    eng = case.engine()
    rng = np.random.default_rng(13)
    X0, Z = rng.uniform(-0.5, 0.5, size=(B, nx)), rng.uniform(-0.5, 0.5, size=(B, n))
    lam, zl, zu = rng.normal(size=(B, eng.m)), rng.uniform(0, 1, size=(B, n)), rng.uniform(0, 1, size=(B, n))
    lb = np.concatenate([np.full(hx, -np.inf), np.full(H * nu, -UBOUND)])
    dev = [eng.to_device(a) for a in (Z, X0, lam, zl, zu)]
    tiles, blocks = _stage_inputs(eng, dev, B)
    worst = 0.0
    for k in ((1, nrhs) if (dims == (64, 32, 2) and nrhs > 1) else (nrhs,)):
        rz, rg = rng.normal(size=(B, k, n)), rng.normal(size=(B, k, hx))
        res = _solve(eng, dev, lb, -lb, rz, rg, ALL, True)
        for b in range(B):
            stage = sref.stage_data_from_tiles(case.problem(b), tiles[b], blocks[b])
            wa, pd, margin, _ = _tier_a(res, b, stage, H, nx, nu, sref.sigma_of(Z[b], zl[b], zu[b], lb, -lb), case.dtype, rz[b], rg[b])
            assert pd and res["status"][b] == 0, (dims, k, b, res["status"][b], margin)
            worst = max(worst, wa)
    print(f"[kkt_solve plan {nx}/{nu} H{H} nrhs={nrhs}: {plan}] tier A error / tolerance {worst:.3e}")
    assert worst <= 1.0


# --------------------------------------------------------------------------------------------------------------------
# 4. verdicts
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["2x1_h20", "6x3_rk4"])
def test_status_is_the_cholesky_verdict_of_the_reference(name):
    """Case.Zrand with lam_b = s_b N(0,1), s_b = (0, 1, 30, 300)[b % 4], two random right-hand sides: status equals the
    reference's verdict on every problem whose smallest reference pivot is farther than 1e-8 |Quu|inf from zero; status-1
    problems are all NaN, the others pass tier A in the same launch.  Then: z_i = ub_i with zu_i > 0 gives status 2 (all
    NaN), the same point with zu_i = 0 status 0."""
    case = sc.nl_case(name)
    H, nx, nu, n, hx, B = case.H, case.nx, case.nu, case.n, case.H * case.nx, case.B
    eng = case.engine()
    rng = np.random.default_rng(7)
    lam = np.stack([(0.0, 1.0, 30.0, 300.0)[b % 4] * rng.normal(size=hx) for b in range(B)])
    rz, rg = rng.normal(size=(B, 2, n)), rng.normal(size=(B, 2, hx))
    Z, X0 = case.Zrand[:B], case.X0[:B]
    dev = [eng.to_device(a) for a in (Z, X0, lam)]
    res = _solve(eng, dev + [None, None], None, None, rz, rg, ALL, False)
    tiles, blocks = _stage_inputs(eng, dev, B)
    verdicts, worst, decided = [], 0.0, 0
    for b in range(B):
        stage = sref.stage_data_from_tiles(case.problem(b), tiles[b], blocks[b])
        wa, pd, margin, _ = _tier_a(res, b, stage, H, nx, nu, None, case.dtype, rz[b], rg[b])
        verdicts.append(pd)
        if margin > 1e-8:
            decided += 1
            assert res["status"][b] == (0 if pd else 1), (b, res["status"][b], pd, margin)
        if res["status"][b] == 1:
            assert all(np.isnan(res[k][b]).all() for k in ALL), b
        elif pd:
            worst = max(worst, wa)
    print(f"[kkt_solve verdicts {name}] reference verdicts {verdicts}, device status {res['status'].tolist()}, "
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
    r2 = _solve(eng, d2, lb, -lb, rz, rg, ALL, True)
    assert r2["status"].tolist() == [0, 2] + [0] * (B - 2)
    assert all(np.isnan(r2[k][1]).all() for k in ALL) and all(np.isfinite(r2[k][0]).all() and np.isfinite(r2[k][2:]).all() for k in ALL)
    zu[1, hx + 3] = 0.0
    d3 = [eng.to_device(a) for a in (Zb, X0, lam0, np.zeros((B, n)), zu)]
    r3 = _solve(eng, d3, lb, -lb, rz, rg, ALL, True)
    assert (r3["status"] == 0).all() and all(np.isfinite(r3[k]).all() for k in ALL)


# --------------------------------------------------------------------------------------------------------------------
# 5. at solver solutions
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [k for k, v in sc.NL_ROWS.items() if v[7] == "float64"])
def test_adjoint_solves_at_solver_solutions(name):
    """Unbounded solves of the tanh rows (max_iter = 200, the library's fp64 tolerances), one random cotangent per problem:
    v and gx0 under tier B at the returned point with the returned multipliers, statuses all 0."""
    case = sc.nl_case(name)
    H, nx, hx, B = case.H, case.nx, case.H * case.nx, case.B
    eng = case.engine()
    X0 = case.bind(eng, B)
    Zt, st, it, d = eng.solve(X0, None, reg=sc.REG, max_iter=200, return_duals=True)
    assert (st == 0).all(), (st.tolist(), it)
    zbar = np.random.default_rng(9).normal(size=(B, case.n))
    out = eng.kkt_solve(Zt, X0, d["lam"], d["zl"], d["zu"], rz=eng.to_device(zbar), want=("v", "gx0"))
    res = {k: (v.cpu().numpy() if k == "status" else _np(v)[:, None]) for k, v in out.items()}
    assert (res["status"] == 0).all() and res["v"].shape == (B, 1, case.n) and res["gx0"].shape == (B, 1, nx)
    Z, lam = _np(Zt), _np(d["lam"])
    worst = gate_max = 0.0
    for b in range(B):
        wb, gate = _tier_b(res, b, case.problem(b), Z[b], case.X0[b], lam[b, :hx], None, zbar[b], None, ("v", "gx0"))
        worst, gate_max = max(worst, wb), max(gate_max, gate)
    print(f"[kkt_solve at solutions {name}] {it} iterations, tier B error / tolerance {worst:.3e} (cond_gate up to {gate_max:.3g})")
    assert worst <= 1.0


@pytest.mark.parametrize("name", list(sc.BOUNDED_ROWS))
def test_adjoint_solves_at_bounded_qp_solutions(name):
    """The set-up of test_bounded_qp_solution_carries_a_kkt_certificate (primal-dual, mu_min = 1e-9) at the returned
    (Z, lam, zl, zu), one random cotangent per problem: v and gx0 under tier B with sigma_of(...)."""
    case, lbe, ube, given = sc.bounded_case(name)
    H, nx, hx, B = case.H, case.nx, case.H * case.nx, case.B
    eng = case.engine()
    eng.set_box_rows(given["box_lo"], given["box_hi"])
    X0 = case.bind(eng, B)
    Zt, st, it, d = eng.solve(X0, None, reg=sc.REG, lb=given["lb"], ub=given["ub"], max_iter=400, barrier="primal-dual",
                              mu_min=1e-9, tol_step=1e-8, tol_constraint=1e-8, return_duals=True)
    assert (st == 0).all(), (st.tolist(), it)
    zbar = np.random.default_rng(9).normal(size=(B, case.n))
    out = eng.kkt_solve(Zt, X0, d["lam"], d["zl"], d["zu"], given["lb"], given["ub"], rz=eng.to_device(zbar), want=("v", "gx0"))
    res = {k: (v.cpu().numpy() if k == "status" else _np(v)[:, None]) for k, v in out.items()}
    assert (res["status"] == 0).all(), res["status"].tolist()
    Z, lam, zl, zu = _np(Zt), _np(d["lam"]), _np(d["zl"]), _np(d["zu"])
    fails = []
    for b in range(B):
        sigma = sref.sigma_of(Z[b], zl[b], zu[b], lbe, ube)
        wb, gate = _tier_b(res, b, case.problem(b), Z[b], case.X0[b], lam[b, :hx], sigma, zbar[b], None, ("v", "gx0"))
        print(f"[kkt_solve bounded {name}] b={b}: max Sigma {sigma.max():.2e}, tier B error / tolerance {wb:.3e} (cond_gate {gate:.3g})")
        if wb > 1.0:
            fails.append(f"b={b}: tier B {wb:.3e}")
    assert not fails, "\n".join(fails)


# --------------------------------------------------------------------------------------------------------------------
# 6. autograd end to end
# --------------------------------------------------------------------------------------------------------------------
def test_autograd_end_to_end():
    """nl_case("2x1_h20"), B = 4, unbounded, per-problem xref and cu bound, loss = sum(c . Z) with seeded c.  The gradients of
    X0, xref and cu equal the float64 reference `vjp` at the device's solution under tier B (X0: gx0's tolerance; xref:
    |Qs|_inf-row-sum times v's; cu: v's).  Then a neighbouring solve with cu + delta, |delta_i| = 1e-3: the loss changes by
    grad . delta within 1e-4 (1 + |grad|inf), the first-order bar of the gain test -- after the CPU check, with
    sref.converge on the same problems, that the reference's own second-order remainder is at most a tenth of that bar at
    this delta (it is: 1e-3 was not shrunk)."""
    from pyneuralempc_amd import autograd as nag
    case = sc.nl_case("2x1_h20")
    H, nx, nu, n, hx, B = case.H, case.nx, case.nu, case.n, case.H * case.nx, 4
    eng = case.engine()
    rng = np.random.default_rng(21)
    xref, cu = sc.REF_SCALE * rng.normal(size=(B, H, nx)), sc.REF_SCALE * rng.normal(size=(B, H, nu))
    c = rng.normal(size=(B, n))
    delta = 1e-3 * rng.choice([-1.0, 1.0], size=(B, H, nu))
    leaf = lambda a: eng.to_device(a).requires_grad_(True)
    X0t, xt, ct = leaf(case.X0[:B]), leaf(xref), leaf(cu)
    cdev = eng.to_device(c)
    Zt, st = nag.solve(eng, X0t, xref=xt, cu=ct, reg=sc.REG, max_iter=200)
    assert (st == 0).all() and not st.requires_grad
    loss = (cdev * Zt).sum()
    loss.backward()
    g = {"X0": _np(X0t.grad), "xref": _np(xt.grad), "cu": _np(ct.grad)}
    # the multipliers of the same solve (the binding is still on the engine)
    Z2, _, _, d = eng.solve(X0t.detach(), None, reg=sc.REG, max_iter=200, return_duals=True)
    assert torch.equal(Z2, Zt.detach())
    Z, lam = _np(Zt), _np(d["lam"])

    def problem(b, cub):
        ob = dict(case.obj)
        ob.update(xref=xref[b], cu=cub)
        return orc.Problem(case.net, H, nx, nu, sc.KINDS[case.integ], case.DT, **ob)

    worst = 0.0
    for b in range(B):
        prob = problem(b, cu[b])
        ref = kref.vjp(prob, Z[b], case.X0[b], lam[b, :hx], None, c[b])
        stage = sref.stage_data(prob, Z[b], case.X0[b], lam[b, :hx])
        dn, ric = kref.dense_solve(stage, H, nx, nu, None, c[b]), kref.affine_riccati(stage, H, nx, nu, None, c[b])
        rp = kref.affine_riccati(sref.perturbed(stage, 1e-11, seed=b), H, nx, nu, None, c[b])
        scales = _scales(dn)
        tol = {k: _tolerance(np.abs(ric[k] - dn[k]).max(), scales[k], "float64",
                             max(1.0, np.abs(rp[k] - ric[k]).max() / (1e-11 * np.abs(ric[k]).max()))) for k in ("v", "gx0")}
        qnorm = max(np.abs(stage["Qs"][t]).sum(axis=1).max() for t in range(H))
        for key, t in (("X0", tol["gx0"]), ("xref", qnorm * tol["v"]), ("cu", tol["v"])):
            worst = max(worst, np.abs(g[key][b] - ref[key]).max() / t)
        # the reference's own second-order remainder at this delta
        z0, _ = sref.converge(prob, case.X0[b], Z[b], 3)
        z1, _ = sref.converge(problem(b, cu[b] + delta[b]), case.X0[b], Z[b], 5)
        rem = abs(c[b] @ (z1 - z0) - (ref["cu"] * delta[b]).sum())
        assert rem <= 0.1 * 1e-4 * (1.0 + np.abs(ref["cu"]).max()), (b, rem)
    print(f"[kkt_solve autograd] gradient error / tier-B tolerance {worst:.3e}")
    assert worst <= 1.0
    with torch.no_grad():
        Zn, stn = nag.solve(eng, X0t.detach(), xref=xt.detach(), cu=eng.to_device(cu + delta), reg=sc.REG, max_iter=200)
    assert (stn == 0).all()
    for b in range(B):
        change = float((c[b] * (_np(Zn)[b] - Z[b])).sum())
        pred = float((g["cu"][b] * delta[b]).sum())
        assert abs(change - pred) <= 1e-4 * (1.0 + np.abs(g["cu"][b]).max()), (b, change, pred)
    eng.bind_tracking()


# --------------------------------------------------------------------------------------------------------------------
# 7. refusals and non-interference
# --------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from pyneuralempc_amd._lib import NempcError
    case = sc.qp_case("roll3_fwd", 10)
    eng = case.engine()
    B = 3
    X0 = case.bind(eng, B)
    Z = eng.to_device(case.Zrand[:B])
    lam = torch.zeros(B, eng.m, dtype=eng.dtype, device=eng.device)
    with pytest.raises(NempcError) as e1:
        eng.kkt_solve(Z, X0, lam, rz=torch.ones_like(Z))
    assert e1.value.code == -5 and "rolling_window" in str(e1.value)
    # a batch larger than a binding covers
    case = sc.qp_case("2x1_extras", 10)
    eng = case.engine()
    X0 = case.bind(eng, 4)
    Z = eng.to_device(case.Zrand[:4])
    lam = torch.zeros(4, eng.m, dtype=eng.dtype, device=eng.device)
    eng.bind_extra(eng.to_device(case.extra[:2]))
    status = torch.zeros(4, dtype=torch.int32, device=eng.device)
    rz = torch.ones(4, 1, case.n, dtype=eng.dtype, device=eng.device)
    v = torch.zeros(4, 1, case.n, dtype=eng.dtype, device=eng.device)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    call = lambda B, nrhs, rz_, v_: eng.lib.nempc_kkt_solve(eng._handle, B, vp(Z), vp(X0), vp(lam), None, None, None, None, nrhs, rz_, None,
                                                            v_, None, None, vp(status), None)
    assert call(4, 1, vp(rz), vp(v)) == -1 and b"exceeds the batch" in eng.lib.nempc_last_error()
    assert call(2, 0, vp(rz), vp(v)) == -1 and b"nrhs" in eng.lib.nempc_last_error()
    assert call(2, 65, vp(rz), vp(v)) == -1 and b"nrhs" in eng.lib.nempc_last_error()
    assert call(2, 1, vp(rz), None) == -1 and b"no output" in eng.lib.nempc_last_error()
    assert call(2, 1, None, vp(v)) == -1 and b"null argument" in eng.lib.nempc_last_error()
    assert call(2, 1, vp(rz), vp(v)) == 0
    with pytest.raises(ValueError):
        eng.kkt_solve(Z[:2], X0[:2], lam[:2], rz=rz[:2, 0].contiguous(), want=())
    with pytest.raises(ValueError):
        eng.kkt_solve(Z[:2], X0[:2], lam[:2])
    torch.cuda.synchronize()
    assert status[:2].tolist() == [0, 0]


def test_solve_and_sensitivity_are_bit_identical_around_a_kkt_solve_call():
    """The call's buffers are the handle's (and nempc_sensitivity's between calls), not the solver's."""
    case = sc.nl_case("6x3_rk4")
    eng = case.engine()
    X0 = case.bind(eng, case.B)
    lb = np.concatenate([np.full(case.H * case.nx, -np.inf), np.full(case.H * case.nu, -0.3)])
    Za, sa, ia, da = eng.solve(X0, None, reg=sc.REG, lb=lb, ub=-lb, max_iter=40, return_duals=True)
    want = ("du0", "dz", "dlam", "gains")
    s1 = eng.sensitivity(Za, X0, da["lam"], da["zl"], da["zu"], lb, -lb, want=want)
    rz = eng.to_device(np.random.default_rng(4).normal(size=(case.B, 5, case.n)))
    out = eng.kkt_solve(Za, X0, da["lam"], da["zl"], da["zu"], lb, -lb, rz=rz, want=ALL)
    assert int(out["status"].max()) == 0 and int(s1["status"].max()) == 0
    s2 = eng.sensitivity(Za, X0, da["lam"], da["zl"], da["zu"], lb, -lb, want=want)
    Zb, sb, ib, db = eng.solve(X0, None, reg=sc.REG, lb=lb, ub=-lb, max_iter=40, return_duals=True)
    assert ia == ib and torch.equal(Za, Zb) and torch.equal(sa, sb) and all(torch.equal(da[k], db[k]) for k in da)
    assert all(torch.equal(s1[k], s2[k]) for k in s1)
