"""CPU: the plan of the register-resident matrix-core launches (csrc/mfma_plan.h, plain host code) passes its stand-alone
check (tests/plan_check.cpp) under the address and undefined-behaviour sanitizers: for every launch recorded on the device
(tests/golden/mfma_launches.json, tools/record_mfma_launches.py) the plan names the recorded kernel code, grid and workgroup
size; over a sweep of shapes it never names an instantiation outside the table of compiled shapes and stays inside the LDS
budgets; each refusal that used to happen inside a launcher has a case on each side; each environment switch flips the choice
its README line names.  The recorded table covers what the issue of the plan listed; engine.py's name tables equal the
enums the program prints.  No device call."""
import json
import os
import re
import shutil
import subprocess

import pytest

from conftest import GOLDEN, REPO
import mfma_plan_cases as mc

ACT_CODE = {None: 1, "relu": 2}                      # NEMPC_ACT_TANH, NEMPC_ACT_RELU; a list of names: per-layer codes (100)
WANT = dict(TILES=1, DENSE=2, SPARSE=4, F=8, GRAD=16, STAGES=32, GN=64)      # RowsWant bits
HWANT = dict(BLOCKS=1, HVALS=2, EVAL=4, DIRECT=8)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "mfma_launches.json")) as fh:
        return json.load(fh)


def _shape(case):
    nx, nu, hidden, acts, ne = mc.NETS[case["net"]]
    H, B = case["H"], case["B"]
    wp = 32 if max(hidden) <= 32 else (64 if max(hidden) <= 64 else 128)
    act = ACT_CODE[acts] if not isinstance(acts, list) else 100
    return [8 if case["dtype"] == "f64" else 4, wp, len(hidden), nx, nu, nx + nu, ne, 1, {"discret": 0, "unity": 1, "rk4": 2}[case["kind"]],
            {"mfma": 2, "mfma_tile": 3}[case["kernel"]], act, H * (nx + nu), H * nx, B, H, case["cus"] or 256,
            4 * nx * nx + 2 * nu * nu + 2 * H * (nx + nu), 1, 0]


def _launch(rec, prefix):
    hits = [l for l in rec["launches"] if re.match(r"(void )?nempc::(\(anonymous namespace\)::)?" + prefix, l["name"])]
    assert len(hits) == 1, (prefix, rec)
    return hits[0]


def queries(golden):
    """The plan queries the library makes for each case (nempc_eval / nempc_hess / nempc_hess_gn, kernels_rk4hess.hip), with
    what the device recorded for them."""
    out = []
    for case in mc.CASES:
        rec, sh, want = golden[case["id"]], _shape(case), case["want"]
        esz = sh[0]
        rows = hess = None
        if case["call"] == "eval":
            bits = sum(WANT[k] for k, name in (("DENSE", "jac_dense"), ("SPARSE", "jac_sparse"), ("F", "f"), ("GRAD", "grad")) if name in want)
            if any(k.startswith("jac") for k in want):
                bits |= WANT["TILES"]
            rows = (bits, esz if case["misalign"] else 0, 0, rec["row"])
        elif case["call"] == "hess_gn":
            rows = (WANT["TILES"] | (WANT["GN"] if want == ("hvals",) else 0), 0, 0, rec["row"])
        elif case["kind"] == "rk4":
            rows = (WANT["TILES"] | WANT["STAGES"], 0, 0, rec["row"])
            hess = (HWANT["BLOCKS"] | HWANT["DIRECT"], 4, rec["hess"] - 10)
        else:
            hess = (HWANT["HVALS"] if want == ("hvals",) else HWANT["BLOCKS"], 1, rec["hess"])
        if rows:
            l = _launch(rec, "rows_")
            out.append(["R", case["id"]] + sh + [rows[0], rows[1], rows[2], rows[3], l["grid"], l["wg"]])
        if hess:
            l = _launch(rec, "rowhess_")
            out.append(["H", case["id"]] + sh + [hess[0], hess[1], 0, hess[2], l["grid"], l["wg"]])
    return out


@pytest.fixture(scope="module")
def check_output(tmp_path_factory, golden):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    tmp = tmp_path_factory.mktemp("mfma_plan")
    exe, qfile = str(tmp / "plan_check"), str(tmp / "queries.txt")
    with open(qfile, "w") as fh:
        for q in queries(golden):
            fh.write(" ".join(str(v) for v in q) + "\n")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "pyneuralempc_amd", "csrc"), "-I", os.path.join(REPO, "include"), "-o", exe,
                    os.path.join(REPO, "tests", "plan_check.cpp")], check=True, capture_output=True)
    r = subprocess.run([exe, qfile], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_plan_stand_alone_under_sanitizers(check_output, golden):
    m = re.search(r"(\d+) checks, 0 failures", check_output)
    assert m and int(m.group(1)) >= 1000000, check_output[-2000:]
    n_queries = int(re.search(r"recorded: (\d+) queries", check_output).group(1))
    assert n_queries == len(queries(golden)) >= len(mc.CASES)


def test_recorded_table_covers_the_dispatch(golden):
    """Once per dtype that has it: every row code 2 - 7, Hessian codes 2, 3, 4 and their forms inside the RK4 pipeline; and
    the named cases."""
    assert set(golden) == set(mc.BY_ID)
    for dt in ("f64", "f32"):
        recs = {i: r for i, r in golden.items() if i.endswith(dt)}
        assert {r["row"] for r in recs.values()} >= {2, 3, 4, 5, 6, 7}
        hess = {r["hess"] for r in recs.values()}
        assert hess >= {2, 3, 4, 12, 13} and (14 in hess) == (dt == "f32")      # (6/3 3 x 128 Hessian dims: fp32 only)
        assert recs[f"cus1-under-{dt}"]["row"] == 2 and recs[f"cus1-over-{dt}"]["row"] == 3      # both sides of the tile-count rule
        assert mc.BY_ID[f"cus1-over-{dt}"]["B"] * mc.BY_ID[f"cus1-over-{dt}"]["H"] / 16 > 32
        assert mc.BY_ID[f"defect-only-{dt}"]["want"] == ("g",)
        nx, nu, _, _, ne = mc.NETS[mc.BY_ID[f"two-block-input-{dt}"]["net"]]
        assert 17 <= nx + nu <= 32
        nx, nu, _, _, ne = mc.NETS[mc.BY_ID[f"five-k-steps-{dt}"]["net"]]
        assert nx + nu + ne > 16
        assert mc.BY_ID[f"tile-variant-{dt}"]["kernel"] == "mfma_tile" and recs[f"tile-variant-{dt}"]["row"] == 3
        assert mc.NETS[mc.BY_ID[f"lv-dense-{dt}"]["net"]][:3] == (2, 1, [30, 30])
        assert "rows_coopfx_kernel<" in _launch(recs[f"gn-lv-{dt}"], "rows_")["name"]
        assert mc.BY_ID[f"misaligned-dense-{dt}"]["misalign"] and recs[f"misaligned-dense-{dt}"]["dense_writer"] == 3
    # 6/3 3 x 128: compiled dimensions in fp32, streamed weights in fp64
    assert "128, 3, 1, false, 2, 1, 6, 3>" in _launch(golden["c3-tiles-f32"], "rows_")["name"]
    assert "rows_mfma_kernel<double, 128, 3, false" in _launch(golden["c3-tiles-f64"], "rows_")["name"]


def test_engine_tables_equal_the_enums(check_output):
    from pyneuralempc_amd import CallbackEngine
    printed = {}
    for what, code, name in re.findall(r"^enum (\S+) (\d+) (\S+)$", check_output, re.M):
        printed.setdefault(what, {})[int(code)] = None if name == "-" else name
    assert printed["RowKernel"] == CallbackEngine.ROW_KERNELS and sorted(printed["RowKernel"]) == list(range(9))
    assert printed["HessKernel"] == CallbackEngine.HESS_KERNELS and sorted(printed["HessKernel"]) == list(range(6))
    assert printed["HessKernel+"] == {CallbackEngine.HESS_IN_RK4: "rk4:"}
    assert printed["LqKernel"] == CallbackEngine.LQ_KERNELS
    assert printed["RolloutKernel"] == CallbackEngine.ROLLOUT_KERNELS
