"""CPU: the linear stage rows (nempc_bind_stage_rows) without a device -- the index header and the AUG_ROWS branches of
stage_aug.h under sanitizers, the C ABI (one new export, version still 8, the refusals documented), LinearStageConstraint, the
Python argument checks, and the references of tests/rows_reference.py / tests/rows_cases.py checking themselves."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

import kkt_reference as kkt
import rows_cases as wc
import rows_reference as wr
import solver_step_cases as sc


def _header():
    return open(os.path.join(REPO, "include", "nempc.h")).read()


# ---------------------------------------------------------------- index header
def test_the_index_header_passes_the_sanitized_host_program(tmp_path):
    """tests/rows_index_check.cpp: csrc/rows_index.h and the AUG_ROWS branches of csrc/stage_aug.h compiled for the host with
    AddressSanitizer and UndefinedBehaviorSanitizer and run on their own, every function against a brute-force restatement by
    labels, for (nx, nu, nc, H) in {(2,1,1,1), (2,1,1,6), (6,3,2,4), (1,4,3,3), (70,3,5,2)}, both per_stage values."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "rows_index_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-I", os.path.join(REPO, "pyneuralempc_amd", "csrc"), "-o", exe, os.path.join(REPO, "tests", "rows_index_check.cpp")]
    if subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-400:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
    m = re.search(r"(\d+) cases, (\d+) entries checked, 0 failures", r.stdout)
    assert m and int(m.group(1)) == 5 and int(m.group(2)) > 2000, r.stdout


def test_the_index_header_includes_nothing():
    text = open(os.path.join(REPO, "pyneuralempc_amd", "csrc", "rows_index.h")).read()
    assert "#include" not in text


# ---------------------------------------------------------------- ABI
def test_bind_stage_rows_is_declared_listed_and_exported():
    from pyneuralempc_amd import _lib
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"\bint nempc_bind_stage_rows\(nempc_handle h, int32_t nc, const double\* C, const double\* rlo, "
                     r"const double\* rhi,\s*int32_t per_stage\);", code)
    lib = _lib.load()
    assert "nempc_bind_stage_rows" in _lib.EXPORTS
    assert hasattr(lib, "nempc_bind_stage_rows"), "libnempc.so does not export nempc_bind_stage_rows"
    assert len(lib.nempc_bind_stage_rows.argtypes) == 6


def test_bind_stage_rows_with_a_null_handle_is_a_code_not_a_fault():
    from pyneuralempc_amd import _lib
    lib = _lib.load()
    assert lib.nempc_bind_stage_rows(None, 1, None, None, None, 0) == -1
    assert b"nempc_bind_stage_rows" in lib.nempc_last_error()


def test_the_abi_version_is_still_8():
    from pyneuralempc_amd import _lib
    m = re.search(r"#define NEMPC_ABI_VERSION (\d+)", _header())
    assert m and int(m.group(1)) == 8
    assert _lib.ABI_VERSION == 8 and _lib.load().nempc_abi_version() == 8


def test_the_header_documents_the_refusals_the_pairing_and_the_calls_that_ignore_the_binding():
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int nempc_bind_stage_rows\(", _header(), flags=re.S)
    assert m
    doc = " ".join(m.group(1).replace("*", " ").split())
    for word in ("nempc_solve_duals", "nempc_kkt_residual", "nempc_sensitivity", "nempc_kkt_solve", "NEMPC_EUNSUPPORTED",
                 "nempc_bind_rate", "nempc_bind_tracking", "nempc_bind_bounds", "rolling_window", "later change", "NEMPC_EINVAL",
                 "copied", "removes the binding", "rlo >= rhi", "nc < 0", "NaN", "Pairing", "Constraint.forward(x, u)",
                 "the state the t-th step arrives at", "tol_constraint (1 + |Cx row|_1)", "bitwise reproducible"):
        assert word in doc, word
    assert re.search(r"nempc_eval, nempc_hess / nempc_hess_gn and nempc_rollout do not read the binding", doc)


# ---------------------------------------------------------------- LinearStageConstraint
H, NX, NU = 4, 2, 2


def _lsc(*a, **kw):
    from pyneuralempc_amd.constraints import LinearStageConstraint
    return LinearStageConstraint(*a, **kw)


def test_linear_stage_constraint_shapes_jacobian_and_type():
    from pyneuralempc_amd.constraints import Constraint
    rng = np.random.default_rng(3)
    C = rng.normal(size=(3, NX + NU))
    c = _lsc(C, [-1.0, -np.inf, 0.0], [1.0, 2.0, np.inf])
    x, u = rng.normal(size=(H, NX)), rng.normal(size=(H, NU))
    g = c.forward(x, u)
    assert g.shape == (H * 3,) and c.get_dim(H) == H * 3
    for t in range(H):      # row block t pairs state row t with control row t
        assert np.allclose(g[t * 3:(t + 1) * 3], C[:, :NX] @ x[t] + C[:, NX:] @ u[t], rtol=0, atol=1e-14)
    J = c.jacobian(x, u)
    assert J.shape == (H * 3, H * (NX + NU))
    z = np.concatenate([x.ravel(), u.ravel()])
    split = lambda v: (v[:H * NX].reshape(H, NX), v[H * NX:].reshape(H, NU))
    for k in range(z.size):
        e = np.zeros(z.size)
        e[k] = 1e-6
        fd = (c.forward(*split(z + e)) - c.forward(*split(z - e))) / 2e-6
        assert np.abs(fd - J[:, k]).max() <= 1e-9
    assert np.abs(c.hessian(x, u)).max() == 0.0 and c.hessian(x, u).shape == (H * 3, z.size, z.size)
    lo, hi = c.get_lower_bounds(H), c.get_upper_bounds(H)
    assert lo.shape == hi.shape == (H * 3,) and np.array_equal(lo[:3], [-1.0, -np.inf, 0.0]) and np.array_equal(hi[3:6], [1.0, 2.0, np.inf])
    assert c.get_type(H) == Constraint.INTER_TYPE
    assert _lsc(C, 0.0, None).get_type(H) == Constraint.INEQ_TYPE           # g >= 0
    assert _lsc(C, None, 1.0).get_type(H) == Constraint.INTER_TYPE


def test_linear_stage_constraint_takes_per_step_limits_and_stacks():
    from pyneuralempc_amd.constraints import LinearStageConstraint
    rng = np.random.default_rng(4)
    C1, C2 = rng.normal(size=(1, NX + NU)), rng.normal(size=(2, NX + NU))
    hi1 = np.arange(1.0, H + 1.0)[:, None]                  # (H,1)
    a, b = _lsc(C1, None, hi1), _lsc(C2, [-1.0, -2.0], [1.0, 2.0])
    assert np.array_equal(a.get_upper_bounds(H), hi1.ravel()) and np.isneginf(a.get_lower_bounds(H)).all()
    with pytest.raises(ValueError, match="per step for H = 4"):
        a.get_upper_bounds(H + 1)
    C, lo, hi = LinearStageConstraint.stack([a, b], H, NX + NU)
    assert C.shape == (3, NX + NU) and lo.shape == hi.shape == (H, 3)
    assert np.array_equal(C, np.concatenate([C1, C2])) and np.array_equal(hi[:, 0], hi1[:, 0]) and np.array_equal(lo[2], [-np.inf, -1.0, -2.0])
    x, u = rng.normal(size=(H, NX)), rng.normal(size=(H, NU))
    both = _lsc(C, lo, hi)
    assert np.array_equal(both.forward(x, u).reshape(H, 3)[:, 1:], b.forward(x, u).reshape(H, 2))
    with pytest.raises(ValueError, match="columns"):
        LinearStageConstraint.stack([a], H, NX + NU + 1)


@pytest.mark.parametrize("args,match", [
    ((np.zeros(4),), "C must be a finite"),
    ((np.full((1, 4), np.nan),), "C must be a finite"),
    ((np.ones((2, 4)), [0.0, 0.0, 0.0]), "lo must have shape"),
    ((np.ones((2, 4)), None, [np.nan, 1.0]), "hi has a NaN"),
    ((np.ones((2, 4)), [0.0, 1.0], [1.0, 1.0]), "lo >= hi"),
    ((np.ones((1, 4)), np.inf, None), "lo >= hi"),
])
def test_linear_stage_constraint_checks_its_arguments(args, match):
    with pytest.raises(ValueError, match=match):
        _lsc(*args)


@pytest.mark.parametrize("kw,match", [
    (dict(C=np.ones((1, 5))), r"C must be a finite \(nc, 4\) matrix"),
    (dict(C=np.ones((2, 4)), lo=np.zeros(3)), r"lo must have shape \(2,\) \(every step\) or \(4, 2\)"),
    (dict(C=np.ones((2, 4)), hi=np.zeros((5, 2))), "hi must have shape"),
    (dict(C=np.ones((2, 4)), lo=[np.nan, 0.0]), "lo has a NaN"),
    (dict(C=np.ones((2, 4)), lo=[0.0, 1.0], hi=np.ones((4, 2))), "lo >= hi"),
    (dict(C=np.ones((2, 4)), hi=[-np.inf, 1.0]), "lo >= hi"),
])
def test_bind_rows_arguments_are_checked_before_the_c_call(kw, match):
    from pyneuralempc_amd.engine import check_rows_args
    a = dict(C=None, lo=None, hi=None)
    a.update(kw)
    with pytest.raises(ValueError, match=match):
        check_rows_args(H, NX, NU, **a)


def test_bind_rows_arguments_that_pass_come_back_in_the_c_form():
    from pyneuralempc_amd.engine import check_rows_args
    C, lo, hi, per = check_rows_args(H, NX, NU, [[1.0, 0.0, 0.0, 2.0]], [-1.0], np.full((H, 1), 2.0))
    assert per == 1 and lo.shape == hi.shape == (H, 1) and C.shape == (1, 4) and lo.flags.c_contiguous and C.dtype == np.float64
    C, lo, hi, per = check_rows_args(H, NX, NU, np.ones((2, 4)), None, [1.0, np.inf])
    assert per == 0 and lo is None and hi.shape == (2,)


def _host_mpc(constraints, **opt):
    import pyneuralempc_amd as nEMPC
    model = nEMPC.model.TorchModel(lambda x, u, p=None, tvp=None: x + 0.1 * u.sum(-1, keepdim=True), 2, 1, device="cpu")
    integ = nEMPC.integrator.DiscretIntegrator(model, 4)
    obj = nEMPC.objective.QuadraticObjective(Q=np.eye(2), R=0.1 * np.eye(1))
    dom = nEMPC.constraints.DomainConstraint(states_constraint=[[-5.0, 5.0]] * 2, control_constraint=[[-1.0, 1.0]])
    return nEMPC.controller.NMPC(integ, obj, [dom] + constraints, 4, 1.0, optimizer=nEMPC.optimizer.Slsqp())


_RATE = dict(u_prev=np.zeros(1), du_lb=[-0.1], du_ub=[0.1])


@pytest.mark.parametrize("who,steps,kw,match", [
    ("next_batch", None, _RATE, "rate arguments"),
    ("next_batch", None, dict(xref=np.zeros((3, 4, 2))), "per-problem references"),
    ("next_batch", None, dict(uub=np.zeros((3, 4, 1))), "per-problem bounds"),
    ("next_batch", None, dict(return_duals=True), "return_duals"),
    ("next_batch", None, dict(return_gain=True), "return_gain"),
    ("closed_loop_batch", 6, _RATE, "rate arguments"),
    ("closed_loop_batch", 6, dict(xref=np.zeros((3, 9, 2))), "per-problem references"),
    ("closed_loop_batch", 6, dict(uub=np.zeros((3, 9, 1))), "per-problem bounds"),
])
def test_the_controller_refuses_what_rows_do_not_combine_with_before_touching_a_device(who, steps, kw, match):
    """B = 3, H = 4, nx = 2, nu = 1 on a host-integrator controller: the combination is a ValueError raised before the
    device-path check that this controller would fail (NotImplementedError), so no device is involved."""
    mpc = _host_mpc([_lsc([[1.0, 0.0, 1.0]], None, 0.5)])
    args = (np.zeros((3, 2)),) + ((steps,) if steps else ())
    with pytest.raises(ValueError, match=match):
        getattr(mpc, who)(*args, **kw)


def test_the_controller_checks_the_rows_width_and_still_refuses_other_constraints():
    from pyneuralempc_amd.constraints import Constraint
    with pytest.raises(ValueError, match="columns"):
        _host_mpc([_lsc([[1.0, 0.0]], None, 0.5)]).next_batch(np.zeros((3, 2)))
    with pytest.raises(NotImplementedError, match="next_batch"):        # (rows alone pass the check; the host integrator does not)
        _host_mpc([_lsc([[1.0, 0.0, 1.0]], None, 0.5)]).next_batch(np.zeros((3, 2)))

    class Other(Constraint):
        def get_dim(self, H):
            return 0
    with pytest.raises(NotImplementedError, match="next_batch"):
        _host_mpc([Other()]).next_batch(np.zeros((3, 2)))


def test_the_host_glue_takes_the_constraint_as_any_row_constraint():
    """The SLSQP problem of a host-integrator controller (the unfused callbacks): the rows, their Jacobian and their bounds follow
    the integrator's defects in g, as for any row constraint."""
    import pyneuralempc_amd as nEMPC

    def _host_mpc(constraints):       # (an objective that lives on the host: QuadraticObjective evaluates on the device)
        model = nEMPC.model.TorchModel(lambda x, u, p=None, tvp=None: x + 0.1 * u.sum(-1, keepdim=True), 2, 1, device="cpu")
        integ = nEMPC.integrator.DiscretIntegrator(model, 4)
        obj = nEMPC.objective.TorchObjectifFunc(lambda x, u, p=None, tvp=None: (x * x).sum() + 0.1 * (u * u).sum(), device="cpu")
        dom = nEMPC.constraints.DomainConstraint(states_constraint=[[-5.0, 5.0]] * 2, control_constraint=[[-1.0, 1.0]])
        return nEMPC.controller.NMPC(integ, obj, [dom] + constraints, 4, 1.0, optimizer=nEMPC.optimizer.Slsqp())
    c = _lsc([[1.0, 0.0, 1.0], [0.0, 2.0, -1.0]], [-np.inf, -1.0], [0.5, 1.0])
    pb = _host_mpc([c]).get_pb(np.array([1.0, -0.5]))
    z = np.random.default_rng(6).normal(size=4 * 3)
    x, u = z[:8].reshape(4, 2), z[8:].reshape(4, 1)
    g, J = pb._all_constraints(z), pb._all_jacobian(z)
    assert g.shape == (8 + 8,) and J.shape == (16, 12)
    assert np.array_equal(g[8:], c.forward(x, u)) and np.array_equal(J[8:], c.jacobian(x, u))
    assert np.array_equal(pb.get_constraint_lower_bounds()[8:], np.tile([-np.inf, -1.0], 4))
    assert np.array_equal(pb.get_constraint_upper_bounds()[8:], np.tile([0.5, 1.0], 4))


def test_device_sqp_refuses_rows_with_rate_terms_or_a_certificate():
    from pyneuralempc_amd.optimizer.device import DeviceSqp

    class Integ:
        on_device, H = True, 4

    class Problem:
        _fused, integrator = None, Integ()
        constraints_list = [_lsc([[1.0, 0.0, 1.0]], None, 0.5)]
    for opt in (DeviceSqp(du_lb=[-0.1], du_ub=[0.1]), DeviceSqp(certificate=True), DeviceSqp(gain=True)):
        with pytest.raises(ValueError, match="LinearStageConstraint cannot be combined"):
            opt.solve(Problem(), None)


# ---------------------------------------------------------------- the references check themselves
def test_the_row_matrix_is_the_jacobian_of_the_constraint_class():
    case = wc.qp_case("6x3_rk4", 4)
    prob = case.problem(0)
    rng = np.random.default_rng(5)
    z = rng.normal(size=prob.n)
    x, u = z[:4 * 6].reshape(4, 6), z[4 * 6:].reshape(4, 3)
    c = _lsc(case.C)
    assert np.array_equal(wr.row_matrix(prob, case.C), c.jacobian(x, u))
    assert np.allclose(wr.row_values(prob, z, case.C).ravel(), c.forward(x, u), rtol=0, atol=1e-14)


@pytest.mark.parametrize("name,H", wc.QP_CASES)
def test_the_sweep_over_the_augmented_stages_gives_the_plain_newton_step(name, H):
    """Rows without limits change nothing: the Riccati sweep over s = [x ; y] in float64 equals the dense plain step (to 1e-10),
    so the tolerance recipe of the GPU test measures rounding, not a modelling gap."""
    case = wc.qp_case(name, H)
    for b in range(case.B):
        prob, x0 = case.problem(b), case.X0[b]
        z0 = case.start(b)
        dz = kkt.newton_step(prob, z0, x0, np.zeros(H * case.nx), sc.REG, diagnostics=False)[0]
        dzr = wr.riccati_step(prob, z0, x0, np.zeros(H * case.nx), sc.REG, case.C, np.float64)
        assert np.abs(dzr - dz).max() <= 1e-10


@pytest.mark.parametrize("name", list(wc.LIMIT_ROWS))
def test_the_limit_cases_have_active_rows_and_bounds_in_every_problem(name):
    """What the GPU test of the limits stands on, from the reference alone: the selection finds its 4 problems; in every one at
    least one row is active, at least one control sits on a bound, no active multiplier is under NU_MIN, and the point
    satisfies the KKT conditions of the inequality-constrained QP to 1e-10 (stationarity with all four multiplier sets,
    complementarity by construction, feasibility).  And no limit test can pass vacuously: the unconstrained solution (no
    bounds, no rows) of every kept problem reaches, on some row, at least twice that row's limit."""
    case, lb, ub, rlo, rhi = wc.limit_case(name)
    Hh, nx = case.H, case.nx
    assert case.B == wc.LIMIT_B and len(wc.limit_reference(name)) == wc.LIMIT_B
    G = wr.row_matrix(case.problem(0), case.C)
    lo, hi = (np.broadcast_to(v, (Hh, case.nc)).ravel() for v in (rlo, rhi))
    for b, (z, lam, nlo, nhi, qlo, qhi) in enumerate(wc.limit_reference(name)):
        prob, x0 = case.problem(b), case.X0[b]
        assert ((qlo + qhi) > 0).sum() >= 1 and ((nlo + nhi)[Hh * nx:] > 0).sum() >= 1
        act = np.concatenate([v[v > 0] for v in (nlo, nhi, qlo, qhi)])
        assert act.min() >= wc.NU_MIN
        r = prob.gradient(z) + kkt._jac(prob, z, x0).T @ lam - nlo + nhi + G.T @ (qhi - qlo)
        assert np.abs(r).max() <= 1e-10 and np.abs(kkt._defects(prob, z, x0)).max() <= 1e-10
        rv = G @ z
        assert (rv >= lo - 1e-12).all() and (rv <= hi + 1e-12).all() and (z >= lb - 1e-12).all() and (z <= ub + 1e-12).all()
        # complementarity: a positive multiplier sits on a limit that holds with equality
        assert np.abs((rv - lo)[qlo > 0]).max(initial=0.0) <= 1e-10 and np.abs((hi - rv)[qhi > 0]).max(initial=0.0) <= 1e-10
        free = G @ wc.unconstrained(prob, case.start(b), x0)
        ratio = float(np.max(np.maximum(free / hi, free / lo)))
        print(f"[rows limits {name}] b={b}: {int(((qlo + qhi) > 0).sum())} active rows, {int(((nlo + nhi) > 0).sum())} active bounds, "
              f"nu_min {act.min():.3e}, unconstrained row / limit {ratio:.2f}")
        assert ratio >= 2.0
