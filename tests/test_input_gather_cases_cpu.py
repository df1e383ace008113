"""CPU: the table of the input-gather sweep (tests/input_gather_cases.py) covers every path it was written for, once per
dtype, by the module's own restatement of the plan; the restatement agrees with the real plan (csrc/mfma_plan.h, asked
through tests/input_gather_plan_check.cpp); and each case can SEE a wrong index: for problem 0 the oracle's defects move
by at least 50 first-order bars when it is given problem 1's extras, its own extras shifted by one stage, or problem
1's history.  A condition on the inputs, not a measurement: a case that misses it gets other seeds or scales.

Over the table the swaps move g by 1.3e-2 (i-sigmoid: the flattest activation, one extra input) to 0.88 and the dense
Jacobian by 4.6e-3 to 0.41, relative to max(1, |.|inf); 50 fp32 bars are 1e-2.  (With standard-normal extras one RK4 case
moved g by 9.8e-3 only -- the extras reach the defects through DT = 0.1 -- so the RK4 cases draw theirs three times as
large.)  No device call."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO
import input_gather_cases as ig

CUS = (256, 64, 1)          # an MI355X in SPX mode, a partitioned device, and what the cus = 1 cases set themselves


def _cus(case, num_cus):
    return case["cus"] or num_cus


def test_size_limits_and_ids():
    assert 60 <= len(ig.CASES) <= 90
    for c in ig.CASES:
        assert c["B"] * c["H"] <= ig.MAX_ROWS and c["H"] <= ig.MAX_H, c["id"]
        assert c["ne"] > 0 or c["window"] > 1, c["id"]
        assert c["kernel"] in ("mfma", "mfma_tile") and c["cus"] in (0, 1), c["id"]
        assert c["window"] == 1 or c["kind"] != "rk4", c["id"]
        assert ig.nin(c) <= 32 and ig.nin(c) + c["ne"] <= 32 and c["nx"] <= 16, c["id"]
        assert c["B"] >= 2 and set(ig.compared_problems(c)) >= {0, 1, c["B"] - 1}, c["id"]
    assert {c["fwd"] for c in ig.CASES if c["window"] > 1} == {True, False}
    assert any(c["H"] == 2 and c["window"] == 4 and ig.padded_width(c) >= 64 for c in ig.CASES)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("num_cus", CUS)
def test_table_covers_every_class(dtype, num_cus):
    cases = [c for c in ig.CASES if c["dtype"] == dtype]
    for name, pred in ig.CLASSES.items():
        hits = [c["id"] for c in cases if pred(c, _cus(c, num_cus))]
        assert hits, f"no {dtype} case for class '{name}' on {num_cus} compute units"
    # nothing may be expected from the generic or the layered path, and every case has a Hessian kernel to name
    for c in cases:
        k = ig.expected_kernels(c, _cus(c, num_cus))
        assert k["tiles"] in ("rows_coop_kernel", "rows_mfma_kernel") and k["dense"] in (k["tiles"], "rows_coop_kernel+dense")
        assert k["hess"].replace("rk4:", "") in ("rowhess_coop_kernel", "rowhess_mfma_kernel")
        assert k["hess"].startswith("rk4:") == (c["kind"] == "rk4")


def test_the_streamed_instantiations_all_run_with_extras():
    """fp64 64 x 3, 128 x 2, 128 x 3 and fp32 128 x 2, 128 x 3: the rows_mfma_kernel instantiations with streamed weights,
    the ones the build's repair (pyneuralempc_amd/_isa.py) sits in, each with ne > 0."""
    seen = {(c["dtype"], ig.padded_width(c), len(c["hidden"])) for c in ig.CASES
            if c["ne"] > 0 and ig.expected_kernels(c)["tiles"] == "rows_mfma_kernel" and not ig.tile_resident(c, 256)}
    assert seen >= {("f64", 64, 3), ("f64", 128, 2), ("f64", 128, 3), ("f32", 128, 2), ("f32", 128, 3)}, seen


def test_both_sides_of_the_register_staging_limit():
    """Two values per thread: 2 * MT * 64 / (16 * tiles per pass) columns.  One shape sits on either side by dtype alone (the
    fp32 pass has three tiles, the fp64 pass two), 17 columns against 16 at width 32 and 11 against 10 in both
    dtypes at width 64."""
    for cus in CUS:
        assert ig.early(ig.BY_ID["c-1x2-w64-ne8-f64"], cus) is True and ig.early(ig.BY_ID["c-1x2-w64-ne8-f32"], cus) is False
        assert ig.coop_rows_plan(ig.BY_ID["c-1x2-w64-ne8-f64"], cus)[0] == 2 and ig.coop_rows_plan(ig.BY_ID["c-1x2-w64-ne8-f32"], cus)[0] == 3
        for cid in ("c-6x3-w32-f64", "c-6x3-w32-f32"):
            c = ig.BY_ID[cid]
            assert ig.early(c, cus) is False and ig.coop_rows_plan(c, cus)[0] == 1 and ig.nin(c) + c["nx"] + c["ne"] == 17, cid
        for cid in ("c-1x1-w64x1-ne8-f64", "c-1x1-w64x1-ne8-f32"):
            assert ig.early(ig.BY_ID[cid], cus) is False and ig.coop_rows_plan(ig.BY_ID[cid], cus)[0] == 3, cid


def test_compared_problems_reach_the_middle_pass_and_the_ragged_tile():
    for c in ig.CASES:
        if c["B"] <= 9:
            assert ig.compared_problems(c) == list(range(c["B"]))
            continue
        cus = _cus(c, 256)
        keep, H = ig.compared_problems(c, cus), c["H"]
        last = 16 * (ig.ntiles(c) - 1)
        assert {last // H, c["B"] - 1} <= set(keep), c["id"]
        if c["cus"] == 1 and ig.coop_passes(c, 1) > 2:
            tpw = ig.coop_rows_plan(c, 1)[0]
            rows = [(b * H, b * H + H - 1) for b in keep]
            # all of its rows in the first workgroup's third or a later pass
            assert any(lo // 16 >= 2 * tpw and hi // 16 < ig.coop_first_wg_tiles(c, 1) for lo, hi in rows), c["id"]
    ragged = [c for c in ig.CASES if c["cus"] == 1]
    assert ragged and all(len(set(range((16 * (ig.ntiles(c) - 1)) // c["H"], c["B"]))) >= 2 for c in ragged)


def _moved(a, b):
    return float(np.abs(a - b).max() / max(1.0, np.abs(a).max()))


@pytest.mark.parametrize("case_id", [c["id"] for c in ig.CASES])
def test_each_case_can_see_a_wrong_index(case_id):
    c = ig.BY_ID[case_id]
    net, d = ig.data(case_id)
    need = ig.DETECT * ig.BAR[c["dtype"]]["first"]
    z, x0 = d["Z"][0], d["X0"][0]
    own = ig.problem(c, net, d, 0)
    g, J = own.constraints(z, x0), own.jacobian(z, x0)
    swaps = {}
    for extras in ("E", "E2") if c["ne"] else ():
        E = d[extras]
        assert len({E[b, t].tobytes() for b in range(c["B"]) for t in range(c["H"])}) == c["B"] * c["H"]     # every row its own
        base = ig.problem(c, net, d, 0, extras=extras)
        swaps[extras + ": problem 1's extras"] = (base, ig.problem(c, net, d, 0, extra=E[1]))
        swaps[extras + ": extras one stage late"] = (base, ig.problem(c, net, d, 0, extra=np.roll(E[0], 1, axis=0)))
    if c["ne"]:
        swaps["the overwrite changes the values"] = (own, ig.problem(c, net, d, 0, extras="E2"))
    if c["window"] > 1:
        swaps["problem 1's history"] = (own, ig.problem(c, net, d, 0, hist_from=1))
    assert swaps
    for what, (a, b) in swaps.items():
        dg = _moved(a.constraints(z, x0), b.constraints(z, x0))
        dJ = _moved(a.jacobian(z, x0), b.jacobian(z, x0))
        print(f"{case_id}: {what}: g moves {dg:.2e}, jacobian {dJ:.2e} (needed {need:.1e})")
        assert dg >= need, (case_id, what, dg, need)
        assert dJ > 0.0 or c["act"] == "relu", (case_id, what)
    assert np.isfinite(g).all() and np.isfinite(J).all()
    if c["dtype"] == "f32":       # the oracle sees what the handle holds
        for a in list(net.W) + list(net.b) + list(d.values()):
            assert np.array_equal(a, a.astype(np.float32).astype(np.float64))


@pytest.fixture(scope="module")
def real_plan(tmp_path_factory):
    """case id, compute units -> what plan_rows / plan_hess of csrc/mfma_plan.h answer for the case's calls."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    tmp = tmp_path_factory.mktemp("input_gather_plan")
    exe, qfile = str(tmp / "plan_check"), str(tmp / "queries.txt")
    act = {"tanh": 1, "relu": 2, "sigmoid": 3, "softplus": 4, "elu": 5}
    with open(qfile, "w") as fh:
        for c in ig.CASES:
            for cus in sorted({_cus(c, n) for n in CUS}):
                n = c["H"] * (c["nx"] + c["nu"])
                m = c["H"] * c["nx"] * (2 if c["box"] else 1)
                fh.write(" ".join(str(v) for v in (
                    c["id"], ig.esz(c), ig.padded_width(c), len(c["hidden"]), c["nx"], c["nu"], ig.nin(c), c["ne"], c["window"],
                    {"discret": 0, "unity": 1, "rk4": 2}[c["kind"]], {"mfma": 2, "mfma_tile": 3}[c["kernel"]],
                    act[c["act"]] if isinstance(c["act"], str) else 100, n, m, c["B"], c["H"], cus)) + "\n")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", os.path.join(REPO, "pyneuralempc_amd", "csrc"), "-I", os.path.join(REPO, "include"),
                    "-o", exe, os.path.join(REPO, "tests", "input_gather_plan_check.cpp")], check=True, capture_output=True)
    r = subprocess.run([exe, qfile], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = {}
    for line in r.stdout.splitlines():
        f = line.split()
        out[(f[0], int(f[1]))] = dict(zip(("tiles", "dense", "defect", "hess", "tpw", "per_cu", "rows_resident", "hess_resident", "passes"),
                                          [int(v) for v in f[2:]]))
    return out


def test_the_restated_predicates_agree_with_the_plan(real_plan):
    """Kernel codes (the enums of mfma_plan.h as CallbackEngine names them), tiles per pass, workgroups per compute unit,
    passes per workgroup and the resident / streamed choice, for every case on 256 and 64 compute units and on one."""
    from pyneuralempc_amd.engine import CallbackEngine as CE
    assert len(real_plan) >= len(ig.CASES)
    for (cid, cus), p in real_plan.items():
        c = ig.BY_ID[cid]
        k = ig.expected_kernels(c, cus)
        tag = (cid, cus)
        assert CE.ROW_KERNELS[p["tiles"]] == k["tiles"] and CE.ROW_KERNELS[p["dense"]] == k["dense"], tag
        assert CE.ROW_KERNELS[p["defect"]] == k["defect"], tag
        name = CE.HESS_KERNELS[p["hess"]]
        assert ("rk4:" if c["kind"] == "rk4" else "") + name == k["hess"], tag
        plan = ig.coop_rows_plan(c, cus)
        assert (p["tpw"], p["per_cu"]) == (plan if plan else (0, 0)), tag
        assert p["passes"] == ig.coop_passes(c, cus), tag
        if k["tiles"] == "rows_mfma_kernel":
            assert bool(p["rows_resident"]) == ig.tile_resident(c, cus), tag
        if name == "rowhess_mfma_kernel":
            assert bool(p["hess_resident"]) == ig.tile_resident(c, cus, hess=True), tag
