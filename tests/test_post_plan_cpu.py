"""CPU: the host arithmetic of the dense / sparse assembly launches (csrc/post_plan.h, plain host code) passes its stand-alone
check under the address and undefined-behaviour sanitizers; the Python restatement of its rule that test_gpu_jac_writers.py
takes its expectations from (tests/post_plan_rule.py) draws the same boundary; nempc_last_dense_writer is exported and
validates its handle.  No device call."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import REPO
import post_plan_rule as rule

TOP = (1 << 17) + 4096           # the stand-alone check's sweep: every mn up to here


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("post_plan") / "post_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "pyneuralempc_amd", "csrc"), "-o", exe,
                    os.path.join(REPO, "tests", "post_plan_check.cpp")], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout


def test_plan_stand_alone_under_sanitizers(check_output):
    """tests/post_plan_check.cpp over csrc/post_plan.h: the 32-bit reciprocal exact for every numerator of every admitted
    mn up to 2^17 and no vector across a problem boundary, every refusal for its stated reason, the B * mn < 2^32 limit and
    the guard of the last block under it, the block counts, the 64-bit reciprocal around problem boundaries, nnz < 2
    refused."""
    m = re.search(r"(\d+) checks, 0 failures", check_output)
    # two checks per admitted mn (73 511 of them in the two widths), one per refused or ragged mn, four per nnz up to 2^16
    assert m and int(m.group(1)) >= 500000, check_output
    for nv in (2, 4):
        assert re.search(rf"NV={nv}: \d+ admitted, \d+ refused by the error bound, first refused mn = \d+", check_output)


@pytest.mark.parametrize("esz", [8, 4])
def test_python_restatement_draws_the_same_boundary(check_output, esz):
    """The first mn the error bound refuses, and how many mn of the whole sweep are admitted / refused by it: the program's
    printed figures against post_plan_rule.flat_refusal."""
    nv = 16 // esz
    m = re.search(rf"NV={nv}: (\d+) admitted, (\d+) refused by the error bound, first refused mn = (\d+)", check_output)
    admitted, refused, first = (int(v) for v in m.groups())
    assert rule.first_inexact(esz, TOP) == first
    why = [rule.flat_refusal(mn, 1, esz, 0) for mn in range(nv, TOP + 1, nv)]
    assert why.count(None) == admitted and why.count(rule.INEXACT) == refused and admitted + refused == len(why)
    # the shapes test_gpu_jac_writers.py names: 15/2 at H = 16 is past the boundary, 10/6 at H = 20 the last reachable one before it
    assert first <= 65280 and rule.flat_refusal(65280, 2, esz, 0) == rule.INEXACT
    assert 64000 < first and rule.flat_refusal(64000, 2, esz, 0) is None


def test_restatement_reasons_and_writer_names():
    assert rule.flat_refusal(6, 700, 8, 0) is None and rule.flat_refusal(6, 700, 4, 0) == rule.RAGGED
    assert rule.flat_refusal(735, 3, 8, 0) == rule.RAGGED and rule.flat_refusal(735, 3, 4, 0) == rule.RAGGED
    assert rule.flat_refusal(2400, 5, 8, 8) == rule.MISALIGNED and rule.flat_refusal(2400, 5, 4, 12) == rule.MISALIGNED
    assert rule.flat_refusal(2401, 5, 8, 8) == rule.RAGGED              # (the order of the header's tests)
    assert rule.flat_refusal(2400, (1 << 32) // 2400 + 1, 8, 0) == rule.TOO_LARGE
    assert rule.flat_refusal(2400, (1 << 32) // 2400, 8, 0) is None
    assert rule.assembly_writer(2400, 5, 8, 0, True, True) == "post_scatter_kernel"
    assert rule.assembly_writer(2400, 5, 8, 0, False, False) == "post_flat_kernel"
    assert rule.assembly_writer(2400, 5, 8, 8, False, True) == "post_kernel"
    assert rule.assembly_writer(2400, 5, 8, 8, False, False) == "assemble_dense_kernel"
    from pyneuralempc_amd import CallbackEngine
    assert set(CallbackEngine.DENSE_WRITERS.values()) == {None, "row_launch", "assemble_dense_kernel", "post_kernel",
                                                         "post_flat_kernel", "post_scatter_kernel"}
    assert sorted(CallbackEngine.DENSE_WRITERS) == [0, 1, 2, 3, 4, 5]


def test_export_exists_and_a_null_handle_is_einval():
    from pyneuralempc_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "nempc_last_dense_writer") and "nempc_last_dense_writer" in _lib.EXPORTS
    assert lib.nempc_last_dense_writer(None) == _lib.EINVAL
    assert b"nempc_last_dense_writer" in lib.nempc_last_error()
    text = open(os.path.join(REPO, "include", "nempc.h")).read()
    assert re.search(r"#define NEMPC_ABI_VERSION 8\b", text) and "int nempc_last_dense_writer(nempc_handle h);" in text
