"""CPU: the C ABI of the per-problem bounds binding (one new export, version still 8), the controller's shape checks, and
the fixture of tests/bounds_cases.py checking itself; no compute calls on a device."""
import os
import re

import numpy as np
import pytest

from conftest import REPO

import bounds_cases as bc
import solver_step_cases as sc


def _header():
    return open(os.path.join(REPO, "include", "nempc.h")).read()


def test_bind_bounds_is_declared_listed_and_exported():
    from pyneuralempc_amd import _lib
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"\bint nempc_bind_bounds\(nempc_handle h, const void\* xlb, const void\* xub, const void\* ulb, "
                     r"const void\* uub,\s*int32_t B, int64_t ld_x, int64_t ld_u\);", code)
    lib = _lib.load()
    assert "nempc_bind_bounds" in _lib.EXPORTS
    assert hasattr(lib, "nempc_bind_bounds"), "libnempc.so does not export nempc_bind_bounds"
    assert len(lib.nempc_bind_bounds.argtypes) == 8


def test_bind_bounds_with_a_null_handle_is_a_code_not_a_fault():
    from pyneuralempc_amd import _lib
    lib = _lib.load()
    assert lib.nempc_bind_bounds(None, None, None, None, None, 1, 0, 0) == -1
    assert b"nempc_bind_bounds" in lib.nempc_last_error()


def test_the_abi_version_is_still_8():
    from pyneuralempc_amd import _lib
    m = re.search(r"#define NEMPC_ABI_VERSION (\d+)", _header())
    assert m and int(m.group(1)) == 8
    assert _lib.ABI_VERSION == 8 and _lib.load().nempc_abi_version() == 8


def _host_mpc(H):
    import pyneuralempc_amd as nEMPC
    model = nEMPC.model.TorchModel(lambda x, u, p=None, tvp=None: x + 0.1 * u.sum(-1, keepdim=True), 2, 1, device="cpu")
    integ = nEMPC.integrator.DiscretIntegrator(model, H)
    obj = nEMPC.objective.QuadraticObjective(Q=np.eye(2), R=0.1 * np.eye(1))
    dom = nEMPC.constraints.DomainConstraint(states_constraint=[[-5.0, 5.0]] * 2, control_constraint=[[-1.0, 1.0]])
    return nEMPC.controller.NMPC(integ, obj, [dom], H, 1.0, optimizer=nEMPC.optimizer.Slsqp())


@pytest.mark.parametrize("name,shape", [("xlb", (3, 5, 2)), ("xlb", (2, 4, 2)), ("xub", (3, 4, 1)), ("ulb", (3, 4, 2)),
                                        ("xub", (4,)), ("uub", (3, 4, 1, 1)), ("uub", (5, 1))])
def test_next_batch_names_the_expected_shape_before_touching_a_device(name, shape):
    """B = 3, H = 4, nx = 2, nu = 1: a wrong shape is a ValueError naming (B,H,d) -- raised before the device-path check that
    this host-integrator controller would fail (NotImplementedError), so no device is involved."""
    mpc = _host_mpc(4)
    d = 2 if name in ("xlb", "xub") else 1
    with pytest.raises(ValueError, match=re.escape(f"{name} must have shape {(3, 4, d)}")):
        mpc.next_batch(np.zeros((3, 2)), **{name: np.zeros(shape)})
    for ok in ((3, 4, d), (4, d)):
        with pytest.raises(NotImplementedError, match="next_batch"):
            mpc.next_batch(np.zeros((3, 2)), **{name: np.zeros(ok)})


def test_closed_loop_batch_wants_steps_plus_horizon_minus_one_rows():
    mpc = _host_mpc(4)
    with pytest.raises(ValueError, match=re.escape(f"xub must have shape {(3, 6, 2)}")):
        mpc.closed_loop_batch(np.zeros((3, 2)), 3, xub=np.zeros((3, 4, 2)))
    with pytest.raises(ValueError, match=re.escape(f"ulb must have shape {(3, 6, 1)}")):
        mpc.closed_loop_batch(np.zeros((3, 2)), 3, ulb=np.zeros((3, 7, 1)))
    with pytest.raises(NotImplementedError, match="closed_loop_batch"):
        mpc.closed_loop_batch(np.zeros((3, 2)), 3, xlb=np.zeros((3, 6, 2)), uub=np.zeros((6, 1)))


@pytest.mark.parametrize("name", list(bc.ROWS))
def test_the_schedules_are_what_the_module_says(name):
    case, s = bc.schedule(name)
    L = case.H + bc.EXTRA_ROWS
    assert s["xlb"].shape == s["xub"].shape == (case.B, L, case.nx) and s["ulb"].shape == s["uub"].shape == (case.B, L, case.nu)
    assert (s["xlb"] < s["xub"]).all() and (s["ulb"] < s["uub"]).all()
    # every problem and every row has control limits of its own
    flat = s["uub"][:, :, 0]
    assert len(np.unique(np.round(flat, 12))) == flat.size


@pytest.mark.parametrize("offset", bc.OFFSETS)
@pytest.mark.parametrize("name", list(bc.ROWS))
def test_the_references_solve_with_strict_complementarity_and_away_from_the_shared_solutions(name, offset):
    """Condition A: every reference solves (kkt.qp_solution raises otherwise) and its smallest active multiplier is >= NU_MIN.
    Condition B: each solution differs from the same problem's solution under bounded_case's shared bounds by more than 100
    times the end-point tolerance of the GPU test -- a solver that reads another problem's or another row's bounds, or the
    shared ones, cannot pass it.  On this fixture: multipliers 4.1e-3 .. 2.8e-1, distances 5.8e-2 .. 4.8e-1, tolerances
    1.3e-7 .. 4.5e-7, pull of the inactive bounds at most 0.18 of the tolerance (1.34 of it at mu_min = 1e-9, next test)."""
    case, _ = bc.schedule(name)
    ref, shared = bc.reference(name, offset), sc.bounded_reference(name)
    for b in range(case.B):
        zs = ref[b][0]
        lo, hi = bc.window(name, b, offset)
        assert (zs >= lo - 1e-12).all() and (zs <= hi + 1e-12).all()
        nu_min = bc.smallest_active_multiplier(ref[b])
        assert nu_min >= sc.NU_MIN, (b, nu_min)
        dist = float(np.abs(zs - shared[b][0]).max())
        tol = bc.end_point_tolerance(nu_min, zs)
        print(f"[bounds fixture {name} offset {offset}] b={b}: nu_min {nu_min:.3e}, distance to the shared-bounds solution "
              f"{dist:.3e}, tolerance {tol:.3e}")
        assert dist > 100.0 * tol, (b, dist, tol)
        # Condition C: at the tests' mu_min the inactive bounds pull the last sub-problem's minimiser by under a quarter of the
        # tolerance, which models active bounds and the stopping test only (bounds_cases.MU_MIN)
        pull = bc.inactive_pull(name, offset, b)
        assert pull <= 0.25 * tol, (b, pull, tol)


def test_a_decade_more_of_mu_min_would_put_a_central_path_point_outside_the_bound():
    """Why bounds_cases.MU_MIN is 1e-10: at 1e-9 the inactive bounds alone move 3x2_h7 / offset 3 / problem 2 by more than the
    end-point bound computed with that mu_min."""
    z = bc.reference("3x2_h7", 3)[2][0]
    nu_min = bc.smallest_active_multiplier(bc.reference("3x2_h7", 3)[2])
    tol9 = 10.0 * (1e-9 / nu_min + bc.TOL_STEP * (1.0 + float(np.abs(z).max())))
    assert bc.inactive_pull("3x2_h7", 3, 2, mu=1e-9) > tol9
