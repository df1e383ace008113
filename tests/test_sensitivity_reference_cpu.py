"""CPU: the float64 sensitivity reference (tests/sensitivity_reference.py) checks itself three independent ways, the library
exports nempc_sensitivity, and the device kernel's recursion (csrc/kernels_sens_impl.h) passes a sanitized stand-alone host
program."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO
import sensitivity_reference as sref
import solver_step_cases as sc


@pytest.mark.parametrize("name", ["2x1_h20", "6x3_rk4"])
def test_reference_is_self_consistent_at_converged_points(name):
    """At points converged by full Newton steps (two problems per shape): the Riccati recursion equals the dense solve to
    1e-11 (1 + |S|inf), the analytic stage-0 right-hand side equals its central-difference form to 1e-8, and the dense
    sensitivities equal central differences (h = 1e-5) of re-solved solutions to 1e-7.  Observed: 1.2e-14, 7.9e-11, 4.9e-10."""
    case = sc.nl_case(name)
    for b in (0, 5):
        prob, x0 = case.problem(b), case.X0[b]
        z, lam = sref.converge(prob, x0, case.start(b))
        stat = np.abs(prob.gradient(z) + prob.jacobian(z, x0)[:case.H * case.nx].T @ lam).max()
        assert stat < 1e-10, stat
        S, dl = sref.dense(prob, z, x0, lam)
        ric = sref.riccati_at(prob, z, x0, lam)
        assert ric["pd"]
        scale = 1.0 + np.abs(S).max()
        e_ric, e_lam = np.abs(ric["S"] - S).max(), np.abs(ric["dlam"] - dl).max()
        Sf, _ = sref.dense_fd_rhs(prob, z, x0, lam)
        e_rhs = np.abs(Sf - S).max()
        h, Sd = 1e-5, np.zeros_like(S)
        for j in range(case.nx):
            e = np.zeros(case.nx)
            e[j] = h
            zp, _ = sref.converge(prob, x0 + e, z, 4)
            zm, _ = sref.converge(prob, x0 - e, z, 4)
            Sd[:, j] = (zp - zm) / (2 * h)
        e_fd = np.abs(Sd - S).max()
        print(f"[sensitivity reference {name}] b={b}: |S|inf = {scale - 1:.3g}, riccati-dense {e_ric:.1e}, fd rhs {e_rhs:.1e}, "
              f"fd of solutions {e_fd:.1e}")
        assert e_ric <= 1e-11 * scale
        assert e_lam <= 1e-11 * (1.0 + np.abs(dl).max())
        assert e_rhs <= 1e-8
        assert e_fd <= 1e-7
        # the gains reproduce the control rows from the state rows, and K_0 is du_0/dx0
        nx, nu, H = case.nx, case.nu, case.H
        np.testing.assert_array_equal(ric["gains"][0], ric["S"][H * nx:H * nx + nu])
        for t in range(1, H):
            np.testing.assert_allclose(ric["gains"][t] @ S[(t - 1) * nx:t * nx], S[H * nx + t * nu:H * nx + (t + 1) * nu],
                                       rtol=0, atol=1e-11 * scale)


@pytest.mark.parametrize("name", list(sc.BOUNDED_SMALL))      # (why not the wide rows: solver_step_cases.BOUNDED_SMALL)
def test_reference_recursion_holds_on_the_central_path_of_the_bounded_qps(name):
    """Synthetic central-path points (mu = 2.5e-9) next to the exact solutions of the bounded QPs: riccati == dense within
    1e-5 absolutely (observed 8.4e-8 on 2x1_h12 problem 0, whose capped state puts Sigma = 1.8e11 inside P where it cancels in
    double; <= 1.1e-12 on the seven problems with bounds active on controls only), the same recursion in float32 is useless
    on that problem (error 18), and the dense result is within 1e-4 of the active-set limit (observed 2.7e-7 .. 1.6e-5)."""
    case, lbe, ube, _ = sc.bounded_case(name)
    worst32 = 0.0
    for b, ref in enumerate(sc.bounded_reference(name)):
        prob, x0 = case.problem(b), case.X0[b]
        z, lam, zl, zu = sref.central_path_point(ref, lbe, ube, 2.5e-9)
        sig = sref.sigma_of(z, zl, zu, lbe, ube)
        S, _ = sref.dense(prob, z, x0, lam, sig)
        ric = sref.riccati_at(prob, z, x0, lam, sig)
        assert ric["pd"]
        e = np.abs(ric["S"] - S).max()
        r32 = sref.riccati_at(prob, z, x0, lam, sig, np.float32)
        e32 = np.abs(r32["S"] - S).max() if r32["pd"] else np.inf
        worst32 = max(worst32, e32)
        Sa, _ = sref.active_set(prob, ref[0], x0, ref[1], (ref[2] > 0) | (ref[3] > 0))
        gap = np.abs(S - Sa).max()
        print(f"[sensitivity reference {name}] b={b}: max Sigma {sig.max():.2e}, riccati-dense {e:.1e} (float32 {e32:.1e}), "
              f"dense - active set {gap:.1e}")
        assert e <= 1e-5
        assert gap <= 1e-4
    if name == "2x1_h12":
        assert worst32 > 1e-2, worst32        # (the state-capped problem: single precision loses every digit)


def test_sigma_and_the_verdict_of_the_reference():
    z, lb, ub = np.array([0.25, 0.75, 0.0]), np.array([-0.75, -0.75, -np.inf]), np.array([0.75, 0.75, np.inf])
    s = sref.sigma_of(z, np.array([2.0, 0.0, 1.0]), np.array([3.0, 0.0, 1.0]), lb, ub)
    np.testing.assert_allclose(s, [2.0 / 1.0 + 3.0 / 0.5, 0.0, 0.0], rtol=0, atol=1e-15)
    # an indefinite Quu: verdict and NaN, nothing raised
    case = sc.nl_case("2x1_h20")
    prob, x0 = case.problem(3), case.X0[3]
    lam = 300.0 * np.random.default_rng(7).normal(size=case.H * case.nx)
    r = sref.riccati_at(prob, case.Zrand[3], x0, lam)
    assert not r["pd"] and np.isnan(r["S"]).all() and r["margin"] > 0.0


def test_library_exports_the_sensitivity_entry_point_and_checks_null_handles():
    from pyneuralempc_amd import _lib
    lib = _lib.load()
    assert lib.nempc_abi_version() == 8 == _lib.ABI_VERSION
    assert hasattr(lib, "nempc_sensitivity") and "nempc_sensitivity" in _lib.EXPORTS
    assert lib.nempc_sensitivity(None, 1, None, None, None, None, None, None, None, None, None, None, None, None, None) == -1
    assert b"nempc_sensitivity: null handle" in lib.nempc_last_error()
    assert ctypes.sizeof(_lib.NempcConfig) == 192
    text = open(os.path.join(REPO, "include", "nempc.h")).read()
    assert re.search(r"#define NEMPC_ABI_VERSION 8\b", text)
    assert re.search(r"int nempc_sensitivity\(nempc_handle h, int32_t B,", text)
    # every export is a symbol of the library and the other way round
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    syms = sorted(l.split()[-1] for l in out.splitlines() if l.split()[-1].startswith("nempc_"))
    assert syms == sorted(_lib.EXPORTS)


def test_sweep_arithmetic_passes_the_sanitized_host_program(tmp_path):
    """tests/sensitivity_check.cpp: the __host__ __device__ recursion of csrc/kernels_sens_impl.h with one lane, compiled for
    the host with AddressSanitizer and UndefinedBehaviorSanitizer and run on its own, against Gaussian elimination on the
    dense KKT system: H in {1,2,3,5} x nx, nu in {1,2,3} x {no Sigma, Sigma on controls, Sigma = 1e8 on a state, indefinite
    Quu}, every array at its exact size.  1e-10 relative, except the state-Sigma cases (bound and reason in the program's
    header: a double recursion loses 2^-53 Sigma there; observed 3e-9)."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "sensitivity_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(REPO, "pyneuralempc_amd", "csrc"), "-o", exe, os.path.join(REPO, "tests", "sensitivity_check.cpp")]
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-400:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    m = re.search(r"(\d+) cases, (\d+) entries checked, 0 failures", r.stdout)
    assert m and int(m.group(1)) == 148 and int(m.group(2)) > 5000, r.stdout
