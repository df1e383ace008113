"""CPU: the roll-out's C ABI (version 8, two new exports) and the closed loop's precondition check; no compute calls."""
import os
import re

import numpy as np
import pytest

from conftest import REPO


def _header():
    return open(os.path.join(REPO, "include", "nempc.h")).read()


def test_abi_version_is_8_in_header_binding_and_library():
    from pyneuralempc_amd import _lib
    m = re.search(r"#define NEMPC_ABI_VERSION (\d+)", _header())
    assert m and int(m.group(1)) == 8
    assert _lib.ABI_VERSION == 8
    assert _lib.load().nempc_abi_version() == 8


def test_rollout_entry_points_are_declared_listed_and_exported():
    from pyneuralempc_amd import _lib
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"\bint nempc_rollout\(nempc_handle h, int32_t B, const void\* X0, void\* Z, void\* f, void\* stream\);", code)
    assert re.search(r"\bint nempc_last_rollout_kernel\(nempc_handle h\);", code)
    lib = _lib.load()
    for name in ("nempc_rollout", "nempc_last_rollout_kernel"):
        assert name in _lib.EXPORTS
        assert hasattr(lib, name), f"libnempc.so does not export {name}"
    # argument checks that need no device: a null handle is a code, not a fault
    assert lib.nempc_rollout(None, 1, None, None, None, None) == -1 and b"nempc_rollout" in lib.nempc_last_error()
    assert lib.nempc_last_rollout_kernel(None) == -1


def test_rollout_unit_is_built_through_the_isa_stage():
    from pyneuralempc_amd import _build
    assert "kernels_rollout.hip" in _build.SOURCES
    reports = {r["unit"]: r for r in _build.isa_reports()}
    assert "kernels_rollout.hip" in reports, "the build left no ISA report for the roll-out unit"
    assert reports["kernels_rollout.hip"]["left"] == [] and reports["kernels_rollout.hip"]["store_hazards"] == []


def test_closed_loop_batch_refuses_a_host_integrator_before_touching_a_device():
    import pyneuralempc_amd as nEMPC
    H = 4
    model = nEMPC.model.TorchModel(lambda x, u, p=None, tvp=None: x + 0.1 * u.sum(-1, keepdim=True), 2, 1, device="cpu")
    integ = nEMPC.integrator.DiscretIntegrator(model, H)
    obj = nEMPC.objective.QuadraticObjective(Q=np.eye(2), R=0.1 * np.eye(1))
    dom = nEMPC.constraints.DomainConstraint(states_constraint=[[-5.0, 5.0]] * 2, control_constraint=[[-1.0, 1.0]])
    mpc = nEMPC.controller.NMPC(integ, obj, [dom], H, 1.0, optimizer=nEMPC.optimizer.Slsqp())
    with pytest.raises(NotImplementedError, match="closed_loop_batch"):
        mpc.closed_loop_batch(np.zeros((3, 2)), 2)
    with pytest.raises(NotImplementedError, match="next_batch"):
        mpc.next_batch(np.zeros((3, 2)), init="rollout")
