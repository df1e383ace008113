"""CPU: the reference of nempc_extra_grad (tests/extra_grad_reference.py) under torch's gradcheck, the planner of the lane
mapping (csrc/egrad_plan.h) as a stand-alone sanitized program, and the new symbols of the C ABI."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import REPO
import extra_grad_reference as eref

# measured on the CPU (float32 evaluation of the reference formula against float64, normalised by max |gE|): the floors the fp32
# device tolerance is 8 times of (tests/test_extra_grad_gpu.py); (with lam and v, first order)
F32_FLOOR = {"a": (4.3e-8, 7.6e-8), "b": (2.7e-7, 2.4e-7), "c": (2.3e-7, 2.1e-7), "d": (2.3e-7, 2.3e-7)}


@pytest.mark.parametrize("second", [False, True], ids=["first_order", "with_lam_v"])
@pytest.mark.parametrize("name", ["a", "c"])
def test_gradcheck_of_S_with_respect_to_the_extras(name, second):
    """torch.autograd.gradcheck (float64, its default tolerances): what reference() returns is the gradient of S"""
    c = eref.CASES[name]
    fn, e = eref.S_of_extra(c.phi(torch.float64), c.inputs(), second)
    assert torch.autograd.gradcheck(fn, (e.clone().requires_grad_(True),))


@pytest.mark.parametrize("name", sorted(eref.CASES))
def test_second_order_part_is_visible_and_fp32_floors_are_as_recorded(name):
    """the lam . T v term is at least a quarter of max |gE| on every case (a device result without it is off by that much);
    the float32 floors are those written down above, within a factor 4"""
    c, r = eref.CASES[name], eref.reference(name)
    assert r["g2"].shape == (c.B, c.H, c.ne) == r["g1"].shape
    part = np.abs(r["g2"] - r["g1"]).max() / np.abs(r["g2"]).max()
    print(f"case {name}: second-order part {part:.2e}, f32 floors {r['e2_f32']:.2e} {r['e1_f32']:.2e}")
    assert part >= 0.25
    for live, rec in zip((r["e2_f32"], r["e1_f32"]), F32_FLOOR[name]):
        assert rec / 4.0 <= live <= rec * 4.0


def test_the_gradient_is_per_row():
    """row (b,t) of gE depends on row (b,t) of the data only: one problem alone gives its rows of the batch"""
    c = eref.CASES["a"]
    d = c.inputs()
    one = {k: (None if a is None else a[2:3]) for k, a in d.items()}
    assert np.abs(eref.gE(c.phi(), one) - eref.reference("a")["g2"][2:3]).max() <= 1e-15


def test_egrad_plans_stay_inside_lds_and_their_workspace_regions_are_disjoint(tmp_path):
    """tests/egrad_plan_check.cpp over csrc/egrad_plan.h with -fsanitize=address,undefined: widths 1 .. 1024, both dtypes,
    1 .. 8 layers, RK4 or not"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "egrad_plan_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "pyneuralempc_amd", "csrc"), "-o", exe,
           os.path.join(REPO, "tests", "egrad_plan_check.cpp")]
    subprocess.run(cmd, check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) plans checked, 0 failures", r.stdout)
    assert m and int(m.group(1)) > 50_000, r.stdout


def test_new_symbols_are_declared_exported_and_the_abi_is_still_8():
    from pyneuralempc_amd import _lib
    text = open(os.path.join(REPO, "include", "nempc.h")).read()
    assert re.search(r"#define NEMPC_ABI_VERSION 8\b", text) and _lib.ABI_VERSION == 8
    lib = _lib.load()
    for s in ("nempc_extra_grad", "nempc_last_extra_grad_kernel"):
        assert s in _lib.EXPORTS and re.search(r"\bint " + s + r"\(", text) and hasattr(lib, s)
    assert lib.nempc_abi_version() == 8
    # argument checks that need no device
    assert lib.nempc_extra_grad(None, 1, None, None, None, None, None, None, None) == _lib.EINVAL
    assert b"nempc_extra_grad" in lib.nempc_last_error()
    assert lib.nempc_last_extra_grad_kernel(None) == _lib.EINVAL
