"""Shapes of the input-gather parity sweep: extra network inputs and rolling windows through the register-resident
matrix-core kernels  --  TEST INFRASTRUCTURE, not a test.

Shared by tests/test_input_gather_cases_cpu.py (the table covers every path and each case can see a wrong index) and
tests/test_gpu_input_gather.py (the kernels against the oracle).  Small on purpose: B * H <= 300, H <= 9.  Everything is
seeded; the extras differ for every problem AND every stage, the histories for every problem, so a kernel that indexed
either by the wrong row would miss the oracle.

The second half restates, in plain Python, what decides which kernel and which staging path a case takes
(csrc/mfma_plan.h: plan_rows / plan_hess and what they call; kernels_mfma_typed.inc: the `early` predicate of
launch_coop), the way solver_step_cases.expected_lq_plan restates plan_lq.  tests/input_gather_plan_check.cpp asks the real
plan the same questions on the CPU.
"""
from __future__ import annotations

import functools
import os

import numpy as np

from oracle import nempc_oracle as orc

KINDS = {"discret": orc.DISCRET, "unity": orc.UNITY, "rk4": orc.RK4}
MAX_ROWS, MAX_H = 300, 9

# Bars relative to max(1, |ref|inf): those of the plain-input sweeps of test_gpu_parity.py
# (test_every_matrix_core_row_instantiation_against_the_oracle / ..._with_its_hessian_against_the_oracle)
BAR = {"f64": dict(first=1e-10, hess=1e-9, gn=1e-9), "f32": dict(first=2e-4, hess=2e-3, gn=2e-3)}
DETECT = 50.0        # a swapped row must move g by this many first-order bars (test_input_gather_cases_cpu.py)


# --------------------------------------------------------------------------------------------------------------------
# the table
# --------------------------------------------------------------------------------------------------------------------
def _c(id, nx, nu, hidden, *, act="tanh", kind="discret", window=1, fwd=True, ne=0, kernel="mfma", B=9, H=7, cus=0,
       gn=False, box=False, dtypes=("f64", "f32"), seed=0):
    # RK4 cases: DT = 0.1, and the extras (standard normal elsewhere) three times as large -- they reach the defects through
    # DT, and at unit scale a swapped row moved g of one case by 0.98 of what test_input_gather_cases_cpu.py asks for
    DT, ex_scale = (0.1, 3.0) if kind == "rk4" else (1.0, 1.0)
    return [dict(id=f"{id}-{dt}", shape=id, nx=nx, nu=nu, hidden=list(hidden), act=act, kind=kind, DT=DT, window=window,
                 fwd=fwd, ne=ne, dtype=dt, kernel=kernel, B=B, H=H, cus=cus, gn=gn, box=box, seed=seed, ex_scale=ex_scale)
            for dt in dtypes]


MIX = ["relu", "tanh", "linear"]     # per-layer codes at run time (NEMPC_ACT_RUNTIME instantiations)

CASES = (
    # ---- (a) cooperative rows, inputs staged through registers ("early"), extras
    _c("a-c2", 2, 1, [64, 64], ne=2, gn=True) +                                   # C2 dims: ne != 0 turns rows_coopfx_kernel off
    _c("a-w128", 2, 1, [128, 128], ne=2, B=5, H=6) +
    _c("a-c3dims", 6, 3, [128, 128, 128], ne=2, B=5, H=4) +                       # fp32: nx / nu compiled in; fp64: streamed tile kernel
    _c("a-6x3-w64", 6, 3, [64, 64], ne=2, B=9, H=5) +                             # 17 columns, one tile per pass (LDS): against 32
    _c("a-2x1-w32", 2, 1, [24, 24], ne=2, B=9, H=7, gn=True) +                    # width 32: one tile per pass (LDS), 7 columns against 16
    # ---- (b) the same with one compute unit: several passes per workgroup, the next pass's extras prefetched; 18 tiles, the
    #      last one holding 15 rows of three problems
    _c("b-c2-cus1", 2, 1, [64, 64], ne=2, B=41, H=7, cus=1) +
    _c("b-w128-cus1", 3, 2, [96, 96], ne=1, B=41, H=7, cus=1) +
    # ---- (c) cooperative rows, staged directly because of the column count, extras
    _c("c-6x3-w32", 6, 3, [32, 32], ne=2, B=9, H=5) +                             # 17 columns against 16
    _c("c-1x2-w64-ne8", 1, 2, [64, 64], ne=8, B=9, H=7, gn=True) +                # 12 columns: fp64 (2 tiles a pass) early, fp32 (3) direct
    _c("c-1x1-w64x1-ne8", 1, 1, [48], ne=8, B=9, H=7) +                           # 11 columns, 3 tiles a pass in both: against 10
    # ---- (d) cooperative rows with a window, with and without extras
    _c("d-w32-win2", 2, 1, [32, 32], window=2, B=9, H=6) +
    _c("d-w32-win4-ne2", 2, 1, [24], window=4, fwd=False, ne=2, B=9, H=7) +
    _c("d-w64-win2-ne1", 3, 2, [64, 48], window=2, ne=1, B=9, H=7, gn=True) +
    _c("d-w64-win4-short", 2, 1, [64, 64], window=4, B=40, H=2) +                 # H < w
    _c("d-w64-win2-rev", 2, 1, [48, 48, 48], window=2, fwd=False, ne=2, B=7, H=9) +
    _c("d-w128-win2-ne2", 2, 1, [128, 128], window=2, ne=2, B=7, H=5) +
    _c("d-w128-win4", 2, 1, [96], window=4, fwd=False, B=9, H=7) +
    _c("d-w64-win2-cus1", 2, 1, [64, 64], window=2, ne=2, B=41, H=7, cus=1) +
    # ---- (e) wave per tile: asked for by name, or "mfma" where the cooperative kernel is refused
    _c("e-res-ne2", 2, 1, [64, 64], ne=2, kernel="mfma_tile", B=11, H=7, gn=True) +
    _c("e-res-win2", 3, 2, [48], kind="unity", window=2, kernel="mfma_tile", B=11, H=7) +
    _c("e-res-win3-ne1", 2, 1, [32, 32, 32], window=3, ne=1, kernel="mfma_tile", B=9, H=6) +
    _c("e-str-128x2-ne2", 2, 1, [128, 128], ne=2, kernel="mfma_tile", B=11, H=7) +
    _c("e-str-128x3-ne3", 3, 1, [128, 96, 128], ne=3, kernel="mfma_tile", B=7, H=5) +
    _c("e-str-64x3-ne2", 2, 1, [64, 64, 64], ne=2, kernel="mfma_tile", B=11, H=7, dtypes=("f64",)) +
    _c("e-str-win2", 2, 1, [128, 128], window=2, kernel="mfma_tile", B=7, H=5) +
    _c("e-str-win2-ne2", 3, 2, [128, 128, 128], window=2, ne=2, kernel="mfma_tile", B=5, H=4) +
    _c("e-regs-128x3", 2, 1, [128, 128, 128], ne=2, B=7, H=5, dtypes=("f64",)) +  # "mfma": the weight slices do not fit the registers
    _c("e-ks5", 12, 4, [32, 32], ne=1, B=5, H=4) +                                # nin = 16: the extras alone make the fifth k-step
    _c("e-mb2", 14, 3, [64], ne=3, B=5, H=4) +                                    # nin = 17: two 16-row input blocks
    _c("e-lim32", 10, 4, [48, 48], window=2, ne=4, B=5, H=4) +                    # nin + ne = 32
    _c("e-lim32-plain", 16, 8, [32], ne=8, B=3, H=3) +
    # ---- (f) RK4 with extras (RK4 with a window is refused at creation)
    _c("f-coop", 2, 1, [64, 64], kind="rk4", ne=2) +
    _c("f-coop-3x2", 3, 2, [96, 96], kind="rk4", ne=1, B=5, H=6) +
    _c("f-coop-h3", 2, 1, [48, 48], kind="rk4", ne=2, B=7, H=3) +                 # a 16-record tile: three stages' rows of one problem, one of the next
    _c("f-tile-res", 2, 1, [64, 64], kind="rk4", ne=2, kernel="mfma_tile") +
    _c("f-tile-res-h3", 2, 1, [32, 32], kind="rk4", ne=2, kernel="mfma_tile", B=7, H=3) +
    _c("f-tile-str", 2, 1, [128, 128, 128], kind="rk4", ne=2, kernel="mfma_tile", B=7, H=5) +
    # ---- (i) activations, a run-time mix, box rows
    _c("i-relu", 2, 1, [64, 64], act="relu", ne=2) +
    _c("i-sigmoid", 3, 2, [32, 32], act="sigmoid", ne=1) +
    _c("i-softplus-tile", 2, 1, [64, 64], act="softplus", ne=2, kernel="mfma_tile") +
    _c("i-elu-win2", 2, 1, [128, 128], act="elu", window=2, ne=2, B=7, H=5) +
    _c("i-mix", 2, 1, [64, 64], act=MIX, ne=2, gn=True) +
    _c("i-mix-rk4-tile", 2, 1, [48, 48], act=MIX, kind="rk4", ne=2, kernel="mfma_tile", B=7, H=5) +
    _c("i-box", 2, 1, [64, 64], ne=2, box=True) +
    _c("i-box-win2", 2, 1, [32, 32], window=2, ne=1, box=True, B=9, H=6)
)
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)
BOX = (-2.0, 2.0)


# --------------------------------------------------------------------------------------------------------------------
# data
# --------------------------------------------------------------------------------------------------------------------
def _round(a, dtype):
    """Values as the handle holds them: an fp32 handle evaluates fp32-rounded data, and so does the oracle."""
    return np.asarray(a, dtype=np.float64) if dtype == "f64" else np.asarray(a, dtype=np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def data(case_id):
    """-> (oracle network, dict of host float64 arrays).  E / E2: two sets of extras (B, H, ne), the second for the in-place
    overwrite of the bound tensor."""
    c = BY_ID[case_id]
    nx, nu, H, B, w, ne, dt = c["nx"], c["nu"], c["H"], c["B"], c["window"], c["ne"], c["dtype"]
    net = orc.MLP.random(w * (nx + nu) + ne, c["hidden"], nx, seed=3 + c["seed"], activations=c["act"])
    net.W = [_round(a, dt) for a in net.W]
    net.b = [_round(a, dt) for a in net.b]
    rng = np.random.default_rng(11 + c["seed"])
    Z, X0 = orc.synthetic_inputs(B, H, nx, nu, seed=5 + c["seed"])
    m = H * nx * (2 if c["box"] else 1)
    d = dict(Z=Z, X0=X0, E=c["ex_scale"] * rng.normal(size=(B, H, ne)), E2=c["ex_scale"] * rng.normal(size=(B, H, ne)),
             hx=rng.normal(size=(B, w - 1, nx)), hu=rng.uniform(-1, 1, size=(B, w - 1, nu)),
             lam=rng.normal(size=(B, m)), sigma=rng.uniform(0.5, 1.5, size=B), w=rng.uniform(0.2, 1.5, size=(B, H * nx)))
    return net, {k: _round(v, dt) for k, v in d.items()}


def problem(case, net, d, b, extras="E", extra=None, hist_from=None):
    """The oracle's problem b.  `extra` (H, ne) / `hist_from` (a problem index) replace its own extras / history."""
    ne, w = case["ne"], case["window"]
    hb = b if hist_from is None else hist_from
    ex = (d[extras][b] if extra is None else extra) if ne else None
    roll = {} if w == 1 else dict(window=w, forward_rolling=case["fwd"], hist_x=d["hx"][hb], hist_u=d["hu"][hb])
    return orc.Problem(net, case["H"], case["nx"], case["nu"], KINDS[case["kind"]], case["DT"],
                       box=BOX if case["box"] else None, extra=ex, **roll)


def engine(case, net):
    """The device handle of the case (GPU tests only).  NEMPC_NUM_CUS is set around the handle's creation only."""
    import torch
    from pyneuralempc_amd import CallbackEngine
    old = os.environ.pop("NEMPC_NUM_CUS", None)
    if case["cus"]:
        os.environ["NEMPC_NUM_CUS"] = str(case["cus"])
    try:
        eng = CallbackEngine(net.W, net.b, case["H"], case["nx"], case["nu"], integrator=case["kind"], DT=case["DT"],
                             dtype={"f64": torch.float64, "f32": torch.float32}[case["dtype"]], device="cuda:0",
                             max_batch=case["B"], kernel=case["kernel"], n_extra=case["ne"], rolling_window=case["window"],
                             forward_rolling=case["fwd"], activations=net.act)
    finally:
        os.environ.pop("NEMPC_NUM_CUS", None)
        if old is not None:
            os.environ["NEMPC_NUM_CUS"] = old
    if case["box"]:
        eng.set_box_rows(*BOX)
    return eng


# --------------------------------------------------------------------------------------------------------------------
# what decides the path: csrc/mfma_plan.h restated
# --------------------------------------------------------------------------------------------------------------------
LDS_TILE, LDS_COOP, MAX_WAVES = 150 * 1024, 160 * 1024, 8       # kLdsBudget, kLdsBudgetCoop, kMaxWaves
HESS_TG = 3                                                      # kHessTG


def up16(v):
    return (v + 15) & ~15


def esz(case):
    return 8 if case["dtype"] == "f64" else 4


def padded_width(case):
    w = max(case["hidden"])
    return 32 if w <= 32 else (64 if w <= 64 else 128)


def nin(case):
    return case["window"] * (case["nx"] + case["nu"])


def ks(case):
    """First-layer k-steps: MfmaShape::ks()."""
    return (nin(case) + case["ne"] + 3) // 4


def mb(case):
    """16-row blocks of the input dimension: MfmaShape::mb()."""
    return (nin(case) + 15) // 16


def ntiles(case, vdiv=1):
    return (case["B"] * case["H"] * vdiv + 15) // 16


def coop_fits_registers(e, wp, nh):
    return ((nh - 1) * 2 * (wp // 16) * 4 + 8) * (e // 4) <= 144


def tile_weights_resident(e, wp, nh):
    return (nh - 1) * 2 * (wp // 16) ** 2 * 256 * e <= 96 * 1024


def coop_tpw_default(e, wp, nh):
    return 2 if (e == 8 and wp >= 64 and nh >= 2) else 3


def rows_scratch(case):
    """One wave's scratch of the row kernels in elements: MfmaShape::rows_scratch()."""
    njs = 4 if case["kind"] == "rk4" else 1
    return (16 * nin(case) + 2 * 16 * case["nx"] + njs * 16 * case["nx"] * nin(case) + 16 * case["nx"] + 16 * case["ne"] + 1) & ~1


def hess_scratch(case):
    return (16 * nin(case) + 16 * case["nx"] + 16 * nin(case) ** 2 + 16 * case["ne"] + 1) & ~1


def blob_offsets(case):
    """-> (total, seed, p0tab) of make_offsets: the packed network's element offsets the LDS sizes use."""
    MT, nh, nx, ni = padded_width(case) // 16, len(case["hidden"]), case["nx"], nin(case)
    p = ks(case) * MT * 64 + (nh - 1) * MT * MT * 256 + MT * 256 + (nh - 1) * MT * MT * 256 + MT * 256 * mb(case)
    p0tab = p
    p += ni * MT * 16 + ((nx + 3) // 4) * MT * 64
    seed = p
    p += nx * MT * 16 + nh * MT * 16 + 16
    return p, seed, p0tab


def _coop_kg(e, nt):
    return 2 if nt * e <= 8 else 1


def _coop_slots(e, tpw):
    return max(nt * _coop_kg(e, nt) for nt in range(1, tpw + 1))


def _coop_nr(e, ni):
    return (ni + 3) // 4 if e == 8 else 4


def coop_lds_bytes(case, tpw):
    """coop_layout(...).total * esz."""
    e, MT = esz(case), padded_width(case) // 16
    total, seed, _ = blob_offsets(case)
    q = ks(case) * MT * 64 + up16(total - seed) + 2 * _coop_slots(e, tpw) * MT * 256
    q += up16((1 + case["nx"]) * tpw * MT * _coop_nr(e, nin(case)) * 64)
    q += 2 * up16(tpw * rows_scratch(case)) + 2 * up16(tpw * 16 * 2 * 4 // e + 1)
    return q * e


def hess_coop_lds_bytes(case):
    """hess_coop_layout(...).total * esz."""
    e, MT, ni = esz(case), padded_width(case) // 16, nin(case)
    total, _, p0tab = blob_offsets(case)
    q = up16(ks(case) * MT * 64) + up16(total - p0tab) + 2 * HESS_TG * MT * 256 + up16(HESS_TG * MT * _coop_nr(e, ni) * 64)
    q += up16(16 * (ni + case["nx"] + case["ne"] + ni * ni))
    return q * e


def _coop_shape(case):
    return case["kernel"] == "mfma" and mb(case) == 1 and ks(case) <= 4 and case["B"] * case["H"] ** 2 < 2 ** 32


def coop_rows_plan(case, num_cus, stages=False):
    """-> (tiles per pass, workgroups per CU) of rows_coop_kernel, or None where plan_rows does not give the rows to it."""
    e, wp, nh = esz(case), padded_width(case), len(case["hidden"])
    by_regs = 8 // (wp // 16)

    def attempt(tpw):
        per_cu = LDS_COOP // coop_lds_bytes(case, tpw)
        if per_cu < 1 or (per_cu < by_regs and tpw > 1):
            return None
        return tpw, min(per_cu, by_regs)

    if not _coop_shape(case) or not coop_fits_registers(e, wp, nh):
        return None
    if stages:
        return attempt(1)
    if tile_weights_resident(e, wp, nh) and ntiles(case) > 32 * num_cus:
        return None
    if wp <= 64:
        for tpw in (3, 2):
            if coop_tpw_default(e, wp, nh) >= tpw and attempt(tpw):
                return attempt(tpw)
    return attempt(1)


def early(case, num_cus):
    """launch_coop's `early`: the pass's inputs (window columns, x_t, extras) travel through two registers per thread and
    the next pass's are prefetched; else they are staged directly.  None: the rows are not the cooperative kernel's.  The
    library does not report which of the two ran: this is the launcher's predicate restated."""
    plan = coop_rows_plan(case, num_cus)
    if plan is None:
        return None
    MT = padded_width(case) // 16
    return case["window"] == 1 and (nin(case) + case["nx"] + case["ne"]) * plan[0] * 16 <= 2 * MT * 64


def coop_first_wg_tiles(case, num_cus):
    """Tiles of the first workgroup of rows_coop_kernel (plan_grid: it owns tiles 0 .. this - 1, and no workgroup owns
    more), 0 where the kernel is not used."""
    plan = coop_rows_plan(case, num_cus)
    if plan is None:
        return 0
    nt = ntiles(case)
    grid = max(1, min(max(1, num_cus) * plan[1], nt))
    return nt // grid + (1 if nt % grid else 0)


def coop_passes(case, num_cus):
    """Most passes one workgroup of rows_coop_kernel makes, 0 where the kernel is not used."""
    plan = coop_rows_plan(case, num_cus)
    return 0 if plan is None else (coop_first_wg_tiles(case, num_cus) + plan[0] - 1) // plan[0]


def tile_resident(case, num_cus, hess=False):
    """set_tile_geom: the wave-per-tile kernel keeps the hidden-to-hidden fragments in LDS (else it streams them)."""
    e = esz(case)
    if not tile_weights_resident(e, padded_width(case), len(case["hidden"])):
        return False
    vdiv = 4 if hess and case["kind"] == "rk4" else 1
    waves = min(max((ntiles(case, vdiv) + num_cus - 1) // num_cus, 1), 4 if hess else MAX_WAVES)
    blob = ((blob_offsets(case)[0] + 1) & ~1) * e
    return blob + waves * (hess_scratch(case) if hess else rows_scratch(case)) * e <= LDS_TILE


def expected_kernels(case, num_cus=256):
    """What CallbackEngine.last_row_kernel / last_hess_kernel must name: `tiles` after an evaluation that asks for
    jac_tiles (with or without the dense matrix and the band values) and after the Gauss-Newton callback; `dense` after
    want=("g", "jac_dense") on the engine's own (16-byte aligned) matrix; `defect` after want=("g",); `hess` after
    hess(want=("hvals",)).  No case here has a compiled shape: every one has extras or a window."""
    assert case["ne"] > 0 or case["window"] > 1
    e, wp, nh = esz(case), padded_width(case), len(case["hidden"])
    coop = coop_rows_plan(case, num_cus) is not None
    n = case["H"] * (case["nx"] + case["nu"])
    blk = case["nx"] * n * e
    writes_dense = coop and case["window"] == 1 and blk % 16 == 0 and 4 * 16 * blk < 0x7fffffff
    tiles = "rows_coop_kernel" if coop else "rows_mfma_kernel"
    hess_coop = (case["kernel"] == "mfma" and mb(case) == 1 and ks(case) <= 4 and coop_fits_registers(e, wp, nh) and
                 LDS_COOP // hess_coop_lds_bytes(case) >= 1)
    hess = "rowhess_coop_kernel" if hess_coop else "rowhess_mfma_kernel"
    return dict(tiles=tiles, dense="rows_coop_kernel+dense" if writes_dense else tiles, defect="rows_mfma_kernel",
                hess=("rk4:" if case["kind"] == "rk4" else "") + hess)


# --------------------------------------------------------------------------------------------------------------------
# which problems a test compares
# --------------------------------------------------------------------------------------------------------------------
def compared_problems(case, num_cus=256):
    """Every problem where B <= 9; else problems 0 and 1, the last one, every problem with a row in the ragged last tile,
    and one whose rows lie in a middle pass of a workgroup of the cooperative kernel (pass 2 or later of the first
    workgroup where it makes more than two; else in the middle tile)."""
    B, H = case["B"], case["H"]
    if B <= 9:
        return list(range(B))
    nt = ntiles(case)
    keep = {0, 1, B - 1} | set(range((16 * (nt - 1)) // H, B))
    plan = coop_rows_plan(case, num_cus)
    mid_tile = nt // 2
    if plan is not None and coop_passes(case, num_cus) > 2:
        mid_tile = 2 * plan[0]                      # first tile of the first workgroup's third pass
    keep.add(min((16 * mid_tile + 8) // H, B - 1))
    return sorted(keep)


# --------------------------------------------------------------------------------------------------------------------
# the classes the table must cover (per dtype): name -> predicate(case, num_cus)
# --------------------------------------------------------------------------------------------------------------------
def _wp(c):
    return padded_width(c)


def _tile_rows(c, cus):
    return expected_kernels(c, cus)["tiles"] == "rows_mfma_kernel"


def _refused(c, cus):
    return c["kernel"] == "mfma" and _tile_rows(c, cus)


CLASSES = {
    "a: coop, early, extras, C2 dims": lambda c, cus: early(c, cus) is True and c["ne"] == 2 and (c["nx"], c["nu"], c["hidden"]) == (2, 1, [64, 64]),
    "a: coop, early, extras, width 128": lambda c, cus: early(c, cus) is True and c["ne"] > 0 and _wp(c) == 128,
    "b: coop, early, extras, > 2 passes, ragged": lambda c, cus: (early(c, cus) is True and c["ne"] > 0 and c["cus"] == 1 and
                                                                  coop_passes(c, 1) > 2 and (c["B"] * c["H"]) % 16 != 0 and ntiles(c) <= 32),
    "c: coop, direct by columns, extras": lambda c, cus: early(c, cus) is False and c["window"] == 1 and c["ne"] > 0,
    "d: coop, window 2, width 32": lambda c, cus: early(c, cus) is False and c["window"] == 2 and _wp(c) == 32,
    "d: coop, window 4, width 32": lambda c, cus: early(c, cus) is False and c["window"] == 4 and _wp(c) == 32,
    "d: coop, window, width 64, extras": lambda c, cus: early(c, cus) is False and c["window"] > 1 and _wp(c) == 64 and c["ne"] > 0,
    "d: coop, window, width 64, no extras": lambda c, cus: early(c, cus) is False and c["window"] > 1 and _wp(c) == 64 and c["ne"] == 0,
    "d: coop, window, width 128, extras": lambda c, cus: early(c, cus) is False and c["window"] > 1 and _wp(c) == 128 and c["ne"] > 0,
    "d: coop, window, width 128, no extras": lambda c, cus: early(c, cus) is False and c["window"] > 1 and _wp(c) == 128 and c["ne"] == 0,
    "d: coop, window, one compute unit": lambda c, cus: early(c, cus) is False and c["window"] > 1 and c["cus"] == 1 and coop_passes(c, 1) > 2,
    "e: tile by name, resident, extras": lambda c, cus: c["kernel"] == "mfma_tile" and tile_resident(c, cus) and c["ne"] > 0,
    "e: tile by name, resident, window": lambda c, cus: c["kernel"] == "mfma_tile" and tile_resident(c, cus) and c["window"] > 1,
    "e: tile, streamed, extras": lambda c, cus: _tile_rows(c, cus) and not tile_resident(c, cus) and c["ne"] > 0,
    "e: tile, streamed, window": lambda c, cus: _tile_rows(c, cus) and not tile_resident(c, cus) and c["window"] > 1,
    "e: mfma refused: fifth k-step from the extras": lambda c, cus: _refused(c, cus) and nin(c) == 16 and c["ne"] == 1 and ks(c) == 5,
    "e: mfma refused: two input blocks, extras": lambda c, cus: _refused(c, cus) and nin(c) == 17 and c["ne"] == 3 and mb(c) == 2,
    "e: nin + ne = 32": lambda c, cus: _tile_rows(c, cus) and nin(c) + c["ne"] == 32,
    "f: rk4, extras, coop, width 64, 2 layers": lambda c, cus: (c["kind"] == "rk4" and c["ne"] > 0 and _wp(c) == 64 and len(c["hidden"]) == 2 and
                                                                expected_kernels(c, cus)["tiles"] == "rows_coop_kernel"),
    "f: rk4, extras, tile, resident": lambda c, cus: c["kind"] == "rk4" and c["ne"] > 0 and _tile_rows(c, cus) and tile_resident(c, cus),
    "f: rk4, extras, tile, streamed, 128 x 3": lambda c, cus: (c["kind"] == "rk4" and c["ne"] > 0 and _tile_rows(c, cus) and not tile_resident(c, cus)
                                                               and _wp(c) == 128 and len(c["hidden"]) == 3),
    "g: rowhess_coop_kernel, extras": lambda c, cus: expected_kernels(c, cus)["hess"] == "rowhess_coop_kernel" and c["ne"] > 0,
    "g: rowhess_coop_kernel, window": lambda c, cus: expected_kernels(c, cus)["hess"] == "rowhess_coop_kernel" and c["window"] > 1,
    "g: rowhess_mfma_kernel, extras": lambda c, cus: expected_kernels(c, cus)["hess"] == "rowhess_mfma_kernel" and c["ne"] > 0,
    "g: rowhess_mfma_kernel, window": lambda c, cus: expected_kernels(c, cus)["hess"] == "rowhess_mfma_kernel" and c["window"] > 1,
    "g: rowhess_mfma_kernel, streamed, extras": lambda c, cus: (expected_kernels(c, cus)["hess"] == "rowhess_mfma_kernel" and c["ne"] > 0 and
                                                                not tile_resident(c, cus, hess=True)),
    # a 16-record tile of the direct mode holds four rows: three stages of one problem and the first of the next at H = 3
    "g: rk4 pipeline, coop, extras, two problems per tile": lambda c, cus: (expected_kernels(c, cus)["hess"] == "rk4:rowhess_coop_kernel" and
                                                                            c["ne"] > 0 and c["H"] == 3 and c["B"] >= 2),
    "g: rk4 pipeline, tile, extras, two problems per tile": lambda c, cus: (expected_kernels(c, cus)["hess"] == "rk4:rowhess_mfma_kernel" and
                                                                            c["ne"] > 0 and c["H"] == 3 and c["B"] >= 2),
    "h: Gauss-Newton, extras, width 64": lambda c, cus: c["gn"] and c["ne"] > 0 and c["window"] == 1 and _wp(c) == 64,
    "h: Gauss-Newton, window, width 64": lambda c, cus: c["gn"] and c["window"] > 1 and _wp(c) == 64,
    "i: tanh, extras": lambda c, cus: c["act"] == "tanh" and c["ne"] > 0,
    "i: relu, extras": lambda c, cus: c["act"] == "relu" and c["ne"] > 0,
    "i: sigmoid, extras": lambda c, cus: c["act"] == "sigmoid" and c["ne"] > 0,
    "i: softplus, extras": lambda c, cus: c["act"] == "softplus" and c["ne"] > 0,
    "i: elu, extras": lambda c, cus: c["act"] == "elu" and c["ne"] > 0,
    "i: run-time mix, extras": lambda c, cus: isinstance(c["act"], list) and c["ne"] > 0,
    "i: box rows": lambda c, cus: c["box"] and c["ne"] > 0,
}


def class_of(case):
    """The letter the docstring of the device test files the case under."""
    return case["shape"][0]
