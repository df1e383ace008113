"""CPU: the C ABI of the per-problem tracking binding (one new export, version still 8) and the controller's shape checks;
no compute calls."""
import os
import re

import numpy as np
import pytest

from conftest import REPO


def _header():
    return open(os.path.join(REPO, "include", "nempc.h")).read()


def test_bind_tracking_is_declared_listed_and_exported():
    from pyneuralempc_amd import _lib
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"\bint nempc_bind_tracking\(nempc_handle h, const void\* xref, const void\* uref, const void\* cx, "
                     r"const void\* cu,\s*int32_t B, int64_t ld_x, int64_t ld_u\);", code)
    lib = _lib.load()
    assert "nempc_bind_tracking" in _lib.EXPORTS
    assert hasattr(lib, "nempc_bind_tracking"), "libnempc.so does not export nempc_bind_tracking"
    assert len(lib.nempc_bind_tracking.argtypes) == 8


def test_bind_tracking_with_a_null_handle_is_a_code_not_a_fault():
    from pyneuralempc_amd import _lib
    lib = _lib.load()
    assert lib.nempc_bind_tracking(None, None, None, None, None, 1, 0, 0) == -1
    assert b"nempc_bind_tracking" in lib.nempc_last_error()


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


@pytest.mark.parametrize("name,shape", [("xref", (3, 5, 2)), ("xref", (2, 4, 2)), ("xref", (3, 4, 1)), ("uref", (3, 4, 2)),
                                        ("cx", (4,)), ("cu", (3, 4, 1, 1)), ("cu", (5, 1))])
def test_next_batch_names_the_expected_shape_before_touching_a_device(name, shape):
    """B = 3, H = 4, nx = 2, nu = 1: a wrong shape is a ValueError naming (B,H,d) -- raised before the device-path check that
    this host-integrator controller would fail (NotImplementedError), so no device is involved."""
    mpc = _host_mpc(4)
    d = 2 if name in ("xref", "cx") else 1
    with pytest.raises(ValueError, match=re.escape(f"{name} must have shape {(3, 4, d)}")):
        mpc.next_batch(np.zeros((3, 2)), **{name: np.zeros(shape)})
    # a right shape, per problem or shared, passes the check and reaches the device-path refusal
    for ok in ((3, 4, d), (4, d)):
        with pytest.raises(NotImplementedError, match="next_batch"):
            mpc.next_batch(np.zeros((3, 2)), **{name: np.zeros(ok)})


def test_closed_loop_batch_wants_steps_plus_horizon_minus_one_rows():
    mpc = _host_mpc(4)
    with pytest.raises(ValueError, match=re.escape(f"xref must have shape {(3, 6, 2)}")):
        mpc.closed_loop_batch(np.zeros((3, 2)), 3, xref=np.zeros((3, 4, 2)))
    with pytest.raises(ValueError, match=re.escape(f"cu must have shape {(3, 6, 1)}")):
        mpc.closed_loop_batch(np.zeros((3, 2)), 3, cu=np.zeros((3, 7, 1)))
    with pytest.raises(NotImplementedError, match="closed_loop_batch"):
        mpc.closed_loop_batch(np.zeros((3, 2)), 3, xref=np.zeros((3, 6, 2)), uref=np.zeros((6, 1)))
