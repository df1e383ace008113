"""CPU: the reference of nempc_weight_grad (tests/weight_grad_reference.py) against the oracle, the planner of the accumulation
(csrc/wgrad_plan.h) as a stand-alone sanitized program, and the new symbols of the C ABI."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import REPO
from oracle import nempc_oracle as orc
import weight_grad_reference as wref

# measured on the CPU (float32 evaluation of the reference formula against float64, normalised by max |gtheta|): the floors
# the fp32 device tolerance is 8 times of (tests/test_weight_grad_gpu.py); (with lam and v, first order)
F32_FLOOR = {"a": (1.1e-7, 8.1e-8), "b": (1.1e-7, 1.2e-7), "c": (2.4e-7, 1.7e-7), "d": (2.9e-7, 2.0e-7), "e": (1.1e-7, 8.1e-8)}


@pytest.mark.parametrize("name", sorted(wref.CASES))
def test_restatement_equals_the_oracle_rows_and_tiles(name):
    """Phi and the tiles of the torch restatement equal orc.Problem.constraints / tiles to 1e-12 on every case"""
    c = wref.CASES[name]
    d = c.inputs()
    p = c.phi()
    Z, X0 = p.t(d["Z"]), p.t(d["X0"])
    Phi, T = p.phi_and_tiles(p.theta0, Z, X0, p.t(d["extra"]))
    for b in range(0, c.B, max(1, c.B // 5)):
        prob = c.problem(b)
        x, phi, dphi, _ = prob.tiles(d["Z"][b], d["X0"][b])
        assert np.abs(Phi[b].numpy() - phi).max() <= 1e-12
        assert np.abs(T[b].numpy() - dphi).max() <= 1e-12
        assert np.abs((Phi[b].numpy() - x).ravel() - prob.constraints(d["Z"][b], d["X0"][b])).max() <= 1e-12


def _oracle_S(c, net, d):
    """S of include/nempc.h with the oracle alone: w . Phi + lam . (T v_[t]) over all rows at once"""
    B, H, nx, nu = c.B, c.H, c.nx, c.nu
    Z, X0 = d["Z"], d["X0"]
    x, u = Z[:, :H * nx].reshape(B, H, nx), Z[:, H * nx:].reshape(B, H, nu)
    xp = np.concatenate([X0[:, None, :], x[:, :-1]], axis=1)
    vx, vu = d["v"][:, :H * nx].reshape(B, H, nx), d["v"][:, H * nx:].reshape(B, H, nu)
    vt = np.concatenate([np.concatenate([np.zeros((B, 1, nx)), vx[:, :-1]], axis=1), vu], axis=2).reshape(B * H, nx + nu)
    ex = None if d["extra"] is None else d["extra"].reshape(B * H, -1)
    phi, dphi, _ = orc.step_rows(net, c.kind, c.DT, xp.reshape(B * H, nx), u.reshape(B * H, nu), extra=ex)
    return float(np.sum(d["w"].reshape(B * H, nx) * phi) + np.sum(d["lam"].reshape(B * H, nx) * np.einsum("rij,rj->ri", dphi, vt)))


@pytest.mark.parametrize("name", ["a", "c"])
def test_gtheta_equals_a_central_difference_of_the_oracles_S(name):
    """step 1e-6, bound 1e-6 of max |gtheta| (truncation of order h^2, rounding of order eps / h in fp64)"""
    c = wref.CASES[name]
    d = c.inputs()
    g = wref.reference(name)["g2"]
    net = c.net()
    h, fd, at = 1e-6, np.zeros_like(g), 0
    for l in range(len(net.W)):
        for arr in (net.W[l], net.b[l]):
            flat = arr.reshape(-1)           # (a view: the oracle's MLP reads the perturbed value)
            for i in range(flat.size):
                keep = flat[i]
                flat[i] = keep + h
                sp = _oracle_S(c, net, d)
                flat[i] = keep - h
                sm = _oracle_S(c, net, d)
                flat[i] = keep
                fd[at] = (sp - sm) / (2.0 * h)
                at += 1
    assert at == g.size
    err = np.abs(fd - g).max() / np.abs(g).max()
    print(f"case {name}: |fd - gtheta| / max |gtheta| = {err:.2e}")
    assert err <= 1e-6


@pytest.mark.parametrize("name", sorted(wref.CASES))
def test_second_order_part_is_visible_and_fp32_floors_are_as_recorded(name):
    """the lam . T v term is at least 1 % of max |gtheta| on every case (a device result without it is off by that much, far
    outside the tolerance); the float32 floors are those written down above, within a factor 4"""
    r = wref.reference(name)
    part = np.abs(r["g2"] - r["g1"]).max() / np.abs(r["g2"]).max()
    print(f"case {name}: second-order part {part:.2e}, f32 floors {r['e2_f32']:.2e} {r['e1_f32']:.2e}")
    assert part >= 0.01
    for live, rec in zip((r["e2_f32"], r["e1_f32"]), F32_FLOOR[name]):
        assert rec / 4.0 <= live <= rec * 4.0


def test_skipped_problems_drop_out_of_the_reference():
    c = wref.CASES["a"]
    d = c.inputs()
    p = c.phi()
    keep = np.array([1, 0, 1, 1, 0])
    full = p.gtheta(d["Z"], d["X0"], d["w"], d["lam"], d["v"], keep=keep)
    sel = keep != 0
    sub = p.gtheta(d["Z"][sel], d["X0"][sel], d["w"][sel], d["lam"][sel], d["v"][sel])
    assert np.array_equal(full, sub)


def test_wgrad_plans_cover_every_row_and_k_element_once(tmp_path):
    """tests/wgrad_plan_check.cpp over csrc/wgrad_plan.h with -fsanitize=address,undefined: ragged rows, chunk sizes and
    compute-unit counts, widths 1 .. 1024"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "wgrad_plan_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "pyneuralempc_amd", "csrc"), "-o", exe,
           os.path.join(REPO, "tests", "wgrad_plan_check.cpp")]
    subprocess.run(cmd, check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) plans checked, 0 failures", r.stdout)
    assert m and int(m.group(1)) > 10_000, r.stdout


def test_new_symbols_are_declared_exported_and_the_abi_is_still_8():
    from pyneuralempc_amd import _lib
    text = open(os.path.join(REPO, "include", "nempc.h")).read()
    assert re.search(r"#define NEMPC_ABI_VERSION 8\b", text) and _lib.ABI_VERSION == 8
    lib = _lib.load()
    for s in ("nempc_n_params", "nempc_weight_grad"):
        assert s in _lib.EXPORTS and re.search(r"\bint " + s + r"\(", text) and hasattr(lib, s)
    assert lib.nempc_abi_version() == 8
    # argument checks that need no device
    import ctypes
    assert lib.nempc_n_params(None, None) == _lib.EINVAL
    assert lib.nempc_weight_grad(None, 1, None, None, None, None, None, None, None, None) == _lib.EINVAL
    assert b"nempc_weight_grad" in lib.nempc_last_error()
