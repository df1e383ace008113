"""CPU: the float64 reference of KKT solves with caller-supplied right-hand sides (tests/kkt_solve_reference.py) checks itself
against the dense solve, the shipped sensitivity reference and central differences of re-solved solutions; the library
exports nempc_kkt_solve; the device kernel's recursion (csrc/kernels_kktsolve_impl.h) passes a sanitized stand-alone host
program."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO
import kkt_solve_reference as kref
import sensitivity_reference as sref
import solver_step_cases as sc


def _rhs(case, k, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(k, case.n)), rng.normal(size=(k, case.H * case.nx))


@pytest.mark.parametrize("name", ["2x1_h20", "6x3_rk4"])
def test_affine_recursion_equals_the_dense_solve_at_converged_points(name):
    """At points converged by full Newton steps (two problems per shape), four random right-hand sides with and without
    rg: affine_riccati == dense_solve to 1e-11 (1 + |v|inf) (w: (1 + |w|inf)); with rz = e_i, rg = 0 the pull-back gx0 is row i
    of sensitivity_reference.dense at the same scale.  Observed: v 4e-15 .. 2e-14, gx0 against dz/dx0 <= 2e-14."""
    case = sc.nl_case(name)
    H, nx, nu, n = case.H, case.nx, case.nu, case.n
    for b in (0, 5):
        prob, x0 = case.problem(b), case.X0[b]
        z, lam = sref.converge(prob, x0, case.start(b))
        stage = sref.stage_data(prob, z, x0, lam)
        rz, rg = _rhs(case, 4, b)
        for g in (None, rg):
            d, r = kref.dense_solve(stage, H, nx, nu, None, rz, g), kref.affine_riccati(stage, H, nx, nu, None, rz, g)
            assert r["pd"]
            ev, ew, eg = (np.abs(r[k] - d[k]).max() for k in ("v", "w", "gx0"))
            print(f"[kkt_solve reference {name}] b={b} rg={'given' if g is not None else 'null'}: |v|inf {np.abs(d['v']).max():.3g}, "
                  f"affine-dense v {ev:.1e}, w {ew:.1e}, gx0 {eg:.1e}")
            assert ev <= 1e-11 * (1.0 + np.abs(d["v"]).max())
            assert ew <= 1e-11 * (1.0 + np.abs(d["w"]).max())
            assert eg <= 1e-11 * (1.0 + np.abs(d["v"]).max() + np.abs(d["w"]).max())
        S, _ = sref.dense(prob, z, x0, lam)
        r = kref.affine_riccati(stage, H, nx, nu, None, np.eye(n))
        e = np.abs(r["gx0"] - S).max()
        print(f"[kkt_solve reference {name}] b={b}: gx0(e_i) against dz/dx0 {e:.1e}")
        assert e <= 1e-11 * (1.0 + np.abs(S).max())


@pytest.mark.parametrize("name", list(sc.BOUNDED_SMALL))      # (why not the wide rows: solver_step_cases.BOUNDED_SMALL)
def test_affine_recursion_holds_on_the_central_path_of_the_bounded_qps(name):
    """Synthetic central-path points (mu = 2.5e-9) next to the exact solutions of the bounded QPs, three random right-hand
    sides with rg: affine_riccati == dense_solve within 1e-5 absolutely (the bar of the sensitivity reference's own test: a
    capped state puts Sigma = 1.8e11 inside P where it cancels in double).  Observed: printed."""
    case, lbe, ube, _ = sc.bounded_case(name)
    H, nx, nu = case.H, case.nx, case.nu
    for b, ref in enumerate(sc.bounded_reference(name)):
        prob, x0 = case.problem(b), case.X0[b]
        z, lam, zl, zu = sref.central_path_point(ref, lbe, ube, 2.5e-9)
        sig = sref.sigma_of(z, zl, zu, lbe, ube)
        stage = sref.stage_data(prob, z, x0, lam)
        rz, rg = _rhs(case, 3, b)
        d, r = kref.dense_solve(stage, H, nx, nu, sig, rz, rg), kref.affine_riccati(stage, H, nx, nu, sig, rz, rg)
        assert r["pd"]
        ev, ew, eg = (np.abs(r[k] - d[k]).max() for k in ("v", "w", "gx0"))
        print(f"[kkt_solve reference {name}] b={b}: max Sigma {sig.max():.2e}, affine-dense v {ev:.1e}, w {ew:.1e}, gx0 {eg:.1e} "
              f"(|v|inf {np.abs(d['v']).max():.3g}, |w|inf {np.abs(d['w']).max():.3g})")
        assert ev <= 1e-5
        assert eg <= 1e-5


@pytest.mark.parametrize("name", ["2x1_h20", "6x3_rk4"])
def test_vjp_equals_central_differences_of_resolved_solutions(name):
    """c' z*(theta) by central differences (h = 1e-5) of re-solved solutions (sref.converge) over every entry of x0, one xref
    row and one cu entry, against `vjp` with the cotangent c: 1e-7, the bar of the sensitivity reference's own test."""
    import copy
    case = sc.nl_case(name)
    H, nx, nu, n, h = case.H, case.nx, case.nu, case.n, 1e-5
    b = 0
    prob, x0 = case.problem(b), case.X0[b]
    z, lam = sref.converge(prob, x0, case.start(b))
    c = np.random.default_rng(3).normal(size=n)
    g = kref.vjp(prob, z, x0, lam, None, c)

    def resolved(p, x):
        zz, _ = sref.converge(p, x, z, 4)
        return float(c @ zz)

    def moved(attr, idx, d):
        p = copy.copy(prob)
        a = np.array(getattr(prob, attr), dtype=np.float64)
        a[idx] += d
        setattr(p, attr, a)
        return p

    errs = {}
    fd = np.array([(resolved(prob, x0 + h * e) - resolved(prob, x0 - h * e)) / (2 * h) for e in np.eye(nx)])
    errs["X0"] = np.abs(fd - g["X0"]).max()
    t = H // 2
    fd = np.array([(resolved(moved("xref", (t, i), h), x0) - resolved(moved("xref", (t, i), -h), x0)) / (2 * h) for i in range(nx)])
    errs["xref"] = np.abs(fd - g["xref"][t]).max()
    fd = (resolved(moved("xref", (H - 1, 0), h), x0) - resolved(moved("xref", (H - 1, 0), -h), x0)) / (2 * h)
    errs["xref terminal"] = abs(fd - g["xref"][H - 1, 0])
    fd = (resolved(moved("cu", (1 % H, nu - 1), h), x0) - resolved(moved("cu", (1 % H, nu - 1), -h), x0)) / (2 * h)
    errs["cu"] = abs(fd - g["cu"][1 % H, nu - 1])
    fd = (resolved(moved("uref", (0, 0), h), x0) - resolved(moved("uref", (0, 0), -h), x0)) / (2 * h)
    errs["uref"] = abs(fd - g["uref"][0, 0])
    fd = (resolved(moved("cx", (t, 0), h), x0) - resolved(moved("cx", (t, 0), -h), x0)) / (2 * h)
    errs["cx"] = abs(fd - g["cx"][t, 0])
    print(f"[kkt_solve reference {name}] vjp against central differences: " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert all(v <= 1e-7 for v in errs.values()), errs


def test_library_exports_the_kkt_solve_entry_point_and_checks_null_handles():
    from pyneuralempc_amd import _lib
    lib = _lib.load()
    assert lib.nempc_abi_version() == 8 == _lib.ABI_VERSION
    assert hasattr(lib, "nempc_kkt_solve") and "nempc_kkt_solve" in _lib.EXPORTS
    assert lib.nempc_kkt_solve(None, 1, None, None, None, None, None, None, None, 1, None, None, None, None, None, None, None) == -1
    assert b"nempc_kkt_solve: null handle" in lib.nempc_last_error()
    assert ctypes.sizeof(_lib.NempcConfig) == 192
    text = open(os.path.join(REPO, "include", "nempc.h")).read()
    assert re.search(r"#define NEMPC_ABI_VERSION 8\b", text)
    assert re.search(r"int nempc_kkt_solve\(nempc_handle h, int32_t B,", text)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = sorted(l.split()[-1] for l in out.splitlines() if l.split()[-1].startswith("nempc_"))
    assert syms == sorted(_lib.EXPORTS)


def test_affine_sweep_arithmetic_passes_the_sanitized_host_program(tmp_path):
    """tests/kkt_solve_check.cpp: the __host__ __device__ recursion of csrc/kernels_kktsolve_impl.h with one lane, compiled for
    the host with AddressSanitizer and UndefinedBehaviorSanitizer and run on its own, against Gaussian elimination on the
    dense KKT system: H in {1,2,3,5} x nx, nu in {1,2,3} x nrhs in {1,3} x {no Sigma, Sigma on controls, Sigma = 1e8 on a
    state, indefinite Quu}, every array at its exact size.  1e-10 relative, except the state-Sigma cases (bound and reason in
    the program's header, those of sensitivity_check.cpp; observed 1.6e-15 and 1.7e-8)."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "kkt_solve_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(REPO, "pyneuralempc_amd", "csrc"), "-o", exe, os.path.join(REPO, "tests", "kkt_solve_check.cpp")]
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-400:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    m = re.search(r"(\d+) cases, (\d+) entries checked, 0 failures", r.stdout)
    assert m and int(m.group(1)) == 288 and int(m.group(2)) > 7000, r.stdout
