"""CPU: the input-rate binding (nempc_bind_rate) without a device -- the index header under sanitizers, the C ABI (one new
export, version still 8, the refusals documented), the Python argument checks, and the references of tests/rate_reference.py /
tests/rate_cases.py checking themselves."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import REPO

import kkt_reference as kkt
import rate_cases as rc
import rate_reference as rr
import solver_step_cases as sc


def _header():
    return open(os.path.join(REPO, "include", "nempc.h")).read()


# ---------------------------------------------------------------- index header
def test_the_index_header_passes_the_sanitized_host_program(tmp_path):
    """tests/rate_index_check.cpp: csrc/rate_index.h compiled for the host with AddressSanitizer and
    UndefinedBehaviorSanitizer and run on its own, every function against a brute-force restatement by labels, for (nx, nu, H)
    in {(2,1,1), (2,1,6), (6,3,4), (1,4,3), (70,3,2)}, with the stage dimensions handed to the LQ plan."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "rate_index_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(REPO, "pyneuralempc_amd", "csrc"), "-o", exe, os.path.join(REPO, "tests", "rate_index_check.cpp")]
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-400:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    m = re.search(r"(\d+) cases, (\d+) entries checked, 0 failures", r.stdout)
    assert m and int(m.group(1)) == 5 and int(m.group(2)) > 2000, r.stdout


def test_the_index_header_includes_nothing_of_hip():
    text = open(os.path.join(REPO, "pyneuralempc_amd", "csrc", "rate_index.h")).read()
    assert "#include" not in text


# ---------------------------------------------------------------- ABI
def test_bind_rate_is_declared_listed_and_exported():
    from pyneuralempc_amd import _lib
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"\bint nempc_bind_rate\(nempc_handle h, const double\* S, const double\* dlo, const double\* dhi, "
                     r"int32_t per_stage,\s*const void\* u_prev, int32_t B\);", code)
    lib = _lib.load()
    assert "nempc_bind_rate" in _lib.EXPORTS
    assert hasattr(lib, "nempc_bind_rate"), "libnempc.so does not export nempc_bind_rate"
    assert len(lib.nempc_bind_rate.argtypes) == 7


def test_bind_rate_with_a_null_handle_is_a_code_not_a_fault():
    from pyneuralempc_amd import _lib
    lib = _lib.load()
    assert lib.nempc_bind_rate(None, None, None, None, 0, None, 1) == -1
    assert b"nempc_bind_rate" in lib.nempc_last_error()


def test_the_abi_version_is_still_8():
    from pyneuralempc_amd import _lib
    m = re.search(r"#define NEMPC_ABI_VERSION (\d+)", _header())
    assert m and int(m.group(1)) == 8
    assert _lib.ABI_VERSION == 8 and _lib.load().nempc_abi_version() == 8


def test_the_header_documents_the_refusals_and_the_calls_that_ignore_the_binding():
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int nempc_bind_rate\(", _header(), flags=re.S)
    assert m
    doc = " ".join(m.group(1).replace("*", " ").split())
    for word in ("nempc_solve_duals", "nempc_kkt_residual", "nempc_sensitivity", "nempc_kkt_solve", "NEMPC_EUNSUPPORTED",
                 "nempc_bind_tracking", "nempc_bind_bounds", "rolling_window", "later change", "NEMPC_EINVAL", "stored not copied",
                 "stream order", "removes the binding"):
        assert word in doc, word
    assert re.search(r"nempc_eval, nempc_hess / nempc_hess_gn and nempc_rollout do not read the binding", doc)


# ---------------------------------------------------------------- Python argument validation (no device)
H, NU = 4, 2
_ARGS = dict(H=H, nu=NU, dtype=torch.float64, device="cpu")


def _check(**kw):
    from pyneuralempc_amd.engine import check_rate_args
    a = dict(u_prev=torch.zeros(3, NU, dtype=torch.float64), S=None, du_lb=None, du_ub=None)
    a.update(kw)
    return check_rate_args(**_ARGS, **a)


@pytest.mark.parametrize("kw,match", [
    (dict(u_prev=None, S=np.eye(NU)), "u_prev is required"),
    (dict(u_prev=np.zeros((3, NU))), "u_prev must be a torch.float64 tensor"),
    (dict(u_prev=torch.zeros(3, NU, dtype=torch.float32)), "u_prev must be a torch.float64 tensor"),
    (dict(u_prev=torch.zeros(3, NU + 1, dtype=torch.float64)), r"\(B,2\)"),
    (dict(u_prev=torch.zeros(NU, dtype=torch.float64)), r"\(B,2\)"),
    (dict(u_prev=torch.zeros(0, NU, dtype=torch.float64)), r"\(B,2\)"),
    (dict(u_prev=torch.zeros(3, NU, dtype=torch.float64, device="meta")), "on cpu"),
    (dict(S=np.eye(NU + 1)), r"S must be a finite \(2, 2\) matrix"),
    (dict(S=np.full((NU, NU), np.nan)), "S must be a finite"),
    (dict(du_lb=np.zeros(NU + 1)), r"du_lb must have shape \(2,\) \(every step\) or \(4, 2\)"),
    (dict(du_ub=np.zeros((H + 1, NU))), "du_ub must have shape"),
    (dict(du_lb=np.array([np.nan, 0.0])), "du_lb has a NaN"),
    (dict(du_lb=np.array([-1.0, 0.5]), du_ub=np.array([1.0, 0.5])), "du_lb >= du_ub"),
    (dict(du_lb=np.full((H, NU), -1.0), du_ub=np.array([1.0, -2.0])), "du_lb >= du_ub"),
    (dict(du_lb=np.array([np.inf, 0.0])), "du_lb >= du_ub"),
])
def test_bind_rate_arguments_are_checked_before_the_c_call(kw, match):
    with pytest.raises(ValueError, match=match):
        _check(**kw)


def test_bind_rate_arguments_that_pass_come_back_in_the_c_form():
    S, lo, hi, per = _check(S=[[1.0, 0.2], [0.0, 1.0]], du_lb=[-1.0, -np.inf], du_ub=np.full((H, NU), 2.0))
    assert per == 1 and lo.shape == hi.shape == (H, NU) and S.shape == (NU, NU) and lo.flags.c_contiguous
    assert _check(du_ub=[1.0, 2.0])[1:] == (None, pytest.approx(np.array([1.0, 2.0])), 0)
    assert _check() == (None, None, None, 0)


def _host_mpc(H):
    import pyneuralempc_amd as nEMPC
    model = nEMPC.model.TorchModel(lambda x, u, p=None, tvp=None: x + 0.1 * u.sum(-1, keepdim=True), 2, 1, device="cpu")
    integ = nEMPC.integrator.DiscretIntegrator(model, H)
    obj = nEMPC.objective.QuadraticObjective(Q=np.eye(2), R=0.1 * np.eye(1))
    dom = nEMPC.constraints.DomainConstraint(states_constraint=[[-5.0, 5.0]] * 2, control_constraint=[[-1.0, 1.0]])
    return nEMPC.controller.NMPC(integ, obj, [dom], H, 1.0, optimizer=nEMPC.optimizer.Slsqp())


@pytest.mark.parametrize("who", ["next_batch", "closed_loop_batch"])
@pytest.mark.parametrize("kw,match", [
    (dict(du_weight=np.eye(1)), "u_prev .* is required"),
    (dict(u_prev=np.zeros((2, 1)), du_weight=np.eye(1)), r"u_prev must have shape \(3, 1\)"),
    (dict(u_prev=np.zeros((3, 1)), du_weight=np.eye(2)), r"du_weight must have shape \(1, 1\)"),
    (dict(u_prev=np.zeros(1), du_lb=np.zeros(2)), r"du_lb must have shape \(1,\) \(every step\) or \(4, 1\)"),
    (dict(u_prev=np.zeros(1), du_lb=[0.1], du_ub=[0.1]), "du_lb >= du_ub"),
])
def test_the_controller_names_the_expected_shape_before_touching_a_device(who, kw, match):
    """B = 3, H = 4, nx = 2, nu = 1: a wrong rate argument is a ValueError raised before the device-path check that this
    host-integrator controller would fail (NotImplementedError), so no device is involved."""
    mpc = _host_mpc(4)
    args = (np.zeros((3, 2)),) + ((2,) if who == "closed_loop_batch" else ())
    with pytest.raises(ValueError, match=match):
        getattr(mpc, who)(*args, **kw)


def test_device_sqp_refuses_rate_terms_with_a_certificate_and_u_prev_without_rate_terms():
    from pyneuralempc_amd.optimizer.device import DeviceSqp
    with pytest.raises(ValueError, match="cannot be combined"):
        DeviceSqp(du_weight=np.eye(1), certificate=True)
    with pytest.raises(ValueError, match="needs rate terms"):
        DeviceSqp().set_u_prev([0.0])
    opt = DeviceSqp(du_lb=[-0.1], du_ub=[0.1])
    with pytest.raises(ValueError, match=r"u_prev must have shape \(1,\)"):
        opt.set_u_prev([0.0, 1.0], 1)
    with pytest.raises(ValueError, match="u_prev is for an optimizer with rate terms"):
        _host_mpc(4).next(np.zeros(2), u_prev=[0.0])


# ---------------------------------------------------------------- the references check themselves
def test_the_rate_gradient_and_hessian_match_finite_differences_of_the_value():
    case = rc.qp_case("6x3_rk4", 4)
    prob, up = case.problem(0), case.u_prev[0]
    rng = np.random.default_rng(5)
    z = rng.normal(size=prob.n)
    g = rr.rate_gradient(prob, z, case.S, up)
    Hr = rr.rate_hessian(prob, case.S)
    for _ in range(5):
        d = rng.normal(size=prob.n)
        fd = (rr.rate_value(prob, z + 1e-6 * d, case.S, up) - rr.rate_value(prob, z - 1e-6 * d, case.S, up)) / 2e-6
        assert abs(fd - g @ d) <= 1e-8 * (1.0 + abs(fd))
        gd = (rr.rate_gradient(prob, z + d, case.S, up) - g)             # (quadratic: exact)
        assert np.abs(gd - Hr @ d).max() <= 1e-12 * (1.0 + np.abs(gd).max())
    assert np.abs(Hr[:case.H * case.nx]).max() == 0.0


@pytest.mark.parametrize("name,H", rc.QP_CASES)
def test_the_dense_rate_qp_solution_satisfies_its_own_kkt_conditions(name, H):
    """Linear networks: one dense Newton step (reg = 0) from the cold start is the solution of the rate QP -- stationarity of
    f + rate + lam.g and the defects, from the oracle's own callbacks, to 1e-10; and the sweep over the augmented stages in
    float64 gives the same step (to 1e-10), so the tolerance recipe of the GPU test measures rounding, not a modelling gap."""
    case = rc.qp_case(name, H)
    for b in range(case.B):
        prob, x0, up = case.problem(b), case.X0[b], case.u_prev[b]
        z0 = case.start(b)
        dz, lam = rr.newton_step(prob, z0, x0, np.zeros(H * case.nx), 0.0, case.S, up)
        z = z0 + dz
        r = prob.gradient(z) + rr.rate_gradient(prob, z, case.S, up) + kkt._jac(prob, z, x0).T @ lam
        assert np.abs(r).max() <= 1e-10 and np.abs(kkt._defects(prob, z, x0)).max() <= 1e-10
        dzr = rr.riccati_step(prob, z0, x0, np.zeros(H * case.nx), sc.REG, case.S, up, np.float64)
        dz9, _ = rr.newton_step(prob, z0, x0, np.zeros(H * case.nx), sc.REG, case.S, up)
        assert np.abs(dzr - dz9).max() <= 1e-10


def test_the_levenberg_term_of_the_reference_sits_on_the_moves():
    """reg D'D, not reg I: with a large reg the two differ visibly, and the augmented sweep agrees with the former."""
    case = rc.qp_case("2x1_discret", 6)
    prob, x0, up = case.problem(0), case.X0[0], case.u_prev[0]
    z0, lam0 = case.start(0), np.zeros(6 * case.nx)
    dz, _ = rr.newton_step(prob, z0, x0, lam0, 0.5, case.S, up)
    assert np.abs(rr.riccati_step(prob, z0, x0, lam0, 0.5, case.S, up) - dz).max() <= 1e-10
    Hm = prob.lagrangian_hessian(z0, x0, lam0, 1.0) + rr.rate_hessian(prob, case.S)
    Hm[12:, 12:] += 0.5 * np.eye(6)
    J = kkt._jac(prob, z0, x0)
    K = np.block([[Hm, J.T], [J, np.zeros((12, 12))]])
    other = np.linalg.solve(K, -np.concatenate([prob.gradient(z0) + rr.rate_gradient(prob, z0, case.S, up), kkt._defects(prob, z0, x0)]))[:18]
    assert np.abs(other - dz).max() > 1e-3


@pytest.mark.parametrize("name", list(rc.LIMIT_ROWS))
def test_the_limit_cases_have_active_limits_and_bounds_in_every_problem(name):
    """What the GPU test of the limits stands on, from the reference alone: in every problem the limit on du_0 (against
    u_prev) is active, at least one control sits on a bound, no active multiplier is under NU_MIN, and the point satisfies the
    KKT conditions of the inequality-constrained QP to 1e-10 (stationarity with all four multiplier sets, complementarity by
    construction, feasibility)."""
    case, lb, ub, dlo, dhi = rc.limit_case(name)
    Hh, nx, nu = case.H, case.nx, case.nu
    G = np.zeros((Hh * nu, case.n))
    G[:, Hh * nx:] = rr.diff_operator(Hh, nu)
    for b, (z, lam, nlo, nhi, rlo, rhi) in enumerate(rc.limit_reference(name)):
        prob, x0, up = case.problem(b), case.X0[b], case.u_prev[b]
        assert (rlo + rhi)[:nu].max() > 0 and ((nlo + nhi)[Hh * nx:] > 0).sum() >= 1
        act = np.concatenate([v[v > 0] for v in (nlo, nhi, rlo, rhi)])
        assert act.min() >= rc.NU_MIN
        r = prob.gradient(z) + rr.rate_gradient(prob, z, case.S, up) + kkt._jac(prob, z, x0).T @ lam - nlo + nhi + G.T @ (rhi - rlo)
        assert np.abs(r).max() <= 1e-10 and np.abs(kkt._defects(prob, z, x0)).max() <= 1e-10
        dv = rr.moves(prob, z, up)
        assert (dv >= dlo - 1e-12).all() and (dv <= dhi + 1e-12).all() and (z >= lb - 1e-12).all() and (z <= ub + 1e-12).all()
        assert (np.abs(up) < ub[-1]).all()
