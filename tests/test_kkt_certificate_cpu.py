"""CPU: the NumPy KKT certificate (tests/kkt_certificate.py) checks itself, the library exports the two multiplier entry
points, and the device kernel's per-variable arithmetic passes a sanitized stand-alone host program."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO
import kkt_certificate as cert
import solver_step_cases as sc


@pytest.mark.parametrize("name", list(sc.BOUNDED_ROWS))
def test_reference_solutions_of_the_bounded_qp_are_kkt_points(name):
    """The exact active-set solutions of the bounded QPs (sc.bounded_reference) under the certificate: all four residuals
    <= 1e-12.  Measured: stationarity <= 1e-14, defects <= 2e-14, 3 to 10 active bounds per problem (4 to 17 on the wide rows)."""
    case, lbe, ube, _ = sc.bounded_case(name)
    for b, (z, lam, nlo, nhi) in enumerate(sc.bounded_reference(name)):
        r, s = cert.residuals(case.problem(b), z, case.X0[b], lam, nlo, nhi, lbe, ube)      # (no box rows here: m = H nx)
        nact = int((nlo > 0).sum() + (nhi > 0).sum())
        print(f"[certificate {name}] b={b}: r = {r.tolist()}, {nact} active bounds")
        assert (r <= 1e-12).all(), (b, r)
        lo, hi = (4, 17) if name in ("20x4_h6", "40x10_h3") else (3, 10)       # (the wide rows: 4 to 17)
        assert lo <= nact <= hi
        assert s.shape == (case.n,)


def test_a_perturbed_multiplier_shows_in_the_residual_it_belongs_to():
    """delta on one defect multiplier moves the stationarity vector by exactly delta times that row of the Jacobian (so
    r[0] rises to |delta| times the row's largest entry from a stationary point), delta on a bound multiplier by delta on
    its variable; a negative zl entry shows in r[3]; a multiplier on an infinite bound is ignored everywhere."""
    name = "2x1_h12"
    case, lbe, ube, _ = sc.bounded_case(name)
    z, lam, nlo, nhi = sc.bounded_reference(name)[0]
    prob, x0 = case.problem(0), case.X0[0]
    r0, s0 = cert.residuals(prob, z, x0, lam, nlo, nhi, lbe, ube)
    J = prob.jacobian(z, x0)
    for row, delta in ((0, 0.25), (7, -0.5), (prob.m - 1, 1e-3)):
        lp = lam.copy()
        lp[row] += delta
        r, s = cert.residuals(prob, z, x0, lp, nlo, nhi, lbe, ube)
        np.testing.assert_allclose(s - s0, delta * J[row], rtol=0, atol=1e-15)
        assert abs(r[0] - abs(delta) * np.abs(J[row]).max()) <= 1e-13
        assert r[1] == r0[1] and r[2] == r0[2] and r[3] == r0[3]
    i = int(np.argmax(nlo > 0)) if (nlo > 0).any() else int(np.argmax(nhi > 0))
    zl = nlo.copy()
    zl[i] += 0.125
    r, s = cert.residuals(prob, z, x0, lam, zl, nhi, lbe, ube)
    assert abs((s - s0)[i] + 0.125) <= 1e-15 and np.abs(np.delete(s - s0, i)).max() == 0.0
    free = int(np.argmax((nlo == 0) & (nhi == 0)))
    zl = nlo.copy()
    zl[free] = -0.375
    r, _ = cert.residuals(prob, z, x0, lam, zl, nhi, lbe, ube)
    assert r[3] == 0.375 and r[0] >= 0.375 - 1e-13
    assert r[2] == pytest.approx(0.375 * (z[free] - lbe[free]), abs=1e-15)
    lb_inf = lbe.copy()
    lb_inf[free] = -np.inf
    r, s = cert.residuals(prob, z, x0, lam, zl, nhi, lb_inf, ube)
    assert r[3] == 0.0 and np.abs(s - s0).max() == 0.0 and r[2] <= 1e-12
    # box rows of a Problem: the limits are intersected with lb / ub, and a box-row multiplier enters s on its state
    from oracle import nempc_oracle as orc
    pb = orc.Problem(case.net, case.H, case.nx, case.nu, sc.KINDS[case.integ], case.DT, box=(-0.2, 0.3), **case.obj)
    lamb = np.concatenate([lam, np.zeros(case.H * case.nx)])
    lamb[case.H * case.nx + 3] = 0.5
    rb, sb = cert.residuals(pb, z, x0, lamb, None, None, None, None)
    ru, su = cert.residuals(prob, z, x0, lam, None, None, None, None)
    d = sb - su
    assert d[3] == 0.5 and np.abs(np.delete(d, 3)).max() == 0.0
    xs = z[:case.H * case.nx]
    assert rb[1] == pytest.approx(max(ru[1], (xs - 0.3).max(), (-0.2 - xs).max()), abs=0)


def test_the_multiplier_sweep_error_is_at_the_floor_in_double():
    """cert.lam_sweep_error in float64 on the 2x1_h20 replay: the Python sweep loses less than 1e-12 on multipliers of
    order 10 (so the 1e-12 (1 + |lam|) floor governs the fp64 tolerance), and is cumulative."""
    case = sc.nl_case("2x1_h20")
    prob, x0 = case.problem(0), case.X0[0]
    e = cert.lam_sweep_error(prob, x0, case.start(0), 3, sc.REG, np.float64)
    assert len(e) == 3 and e[0] <= e[1] <= e[2] and e[2] < 1e-11, e
    e32 = cert.lam_sweep_error(prob, x0, case.start(0), 2, sc.REG, np.float32)
    assert e32[1] > 1e-8, e32
    assert cert.lam_tolerance(0.0, np.array([19.0])) == pytest.approx(2e-11)
    assert cert.lam_tolerance(1e-9, np.array([19.0])) == pytest.approx(1e-8)


def test_library_exports_the_multiplier_entry_points_and_checks_null_handles():
    from pyneuralempc_amd import _lib
    lib = _lib.load()
    assert lib.nempc_abi_version() == 8 == _lib.ABI_VERSION
    for sym in ("nempc_solve_duals", "nempc_kkt_residual"):
        assert hasattr(lib, sym) and sym in _lib.EXPORTS
    assert lib.nempc_solve_duals(None, 1, None, None, None, None, None, None, None, None, None, None, None) == -1
    assert b"null handle" in lib.nempc_last_error()
    assert lib.nempc_kkt_residual(None, 1, None, None, None, None, None, None, None, None, None, None) == -1
    assert b"nempc_kkt_residual" in lib.nempc_last_error()
    # the structs did not move: the two calls are additive
    assert ctypes.sizeof(_lib.NempcConfig) == 192
    text = open(os.path.join(REPO, "include", "nempc.h")).read()
    assert re.search(r"#define NEMPC_ABI_VERSION 8\b", text)


def test_kkt_kernel_arithmetic_passes_the_sanitized_host_program(tmp_path):
    """tests/kkt_residual_check.cpp: the __host__ __device__ function of csrc/kernels_kkt_impl.h, compiled for the host with
    AddressSanitizer and UndefinedBehaviorSanitizer and run on its own, against a dense triple loop -- every variable of
    (nx, nu, H) in {(2,1,1), (2,1,2), (2,1,3), (3,2,7), (6,3,8), (2,1,63)}, with and without box rows, null and non-null
    bound multipliers, no / finite / mixed infinite bounds, both element types, every array at its exact size."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "kkt_residual_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(REPO, "pyneuralempc_amd", "csrc"), "-o", exe, os.path.join(REPO, "tests", "kkt_residual_check.cpp")]
    # the sanitizer runtimes linked into the program itself where the compiler takes the option (GCC): it then runs the same
    # whatever else the environment loads into a process
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    m = re.search(r"(\d+) cases, (\d+) entries checked, 0 failures", r.stdout)
    assert m and int(m.group(1)) == 144 and int(m.group(2)) > 7000, r.stdout
