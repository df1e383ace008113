"""GPU: every case of tests/mfma_plan_cases.py once.  The kernel codes after the call equal the record made before the
dispatch moved into csrc/mfma_plan.h (tests/golden/mfma_launches.json), and the outputs equal the CPU oracle to the
tolerances test_gpu_parity.py uses for the dtype (fp64: f, grad 1e-12 + 1e-12, g 1e-12 + 2e-12, Jacobians 1e-11 + 2e-12,
Hessians 1e-10 + 1e-11 as its seeded tests; fp32: 1e-4 of the largest reference magnitude).  The first and the last problem of a batch are
compared: a batch's rows are spread over the workgroups, so these are the first tile and the (ragged) last one."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
import mfma_plan_cases as mc

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "mfma_launches.json")) as _fh:
    RECORD = json.load(_fh)


def _close(case, name, got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if case["dtype"] == "f32":
        err = np.abs(got - ref).max() / max(1.0, np.abs(ref).max())
        assert err < 1e-4, f"{case['id']}/{name}: max rel err {err:.3e}"
    elif case["call"] == "eval":
        np.testing.assert_allclose(got, ref, rtol=1e-11 if name.startswith("jac") else 1e-12, atol=1e-12 if name in ("f", "grad") else 2e-12,
                                   err_msg=f"{case['id']}/{name}")
    else:
        np.testing.assert_allclose(got, ref, rtol=1e-10, atol=1e-11, err_msg=f"{case['id']}/{name}")


@pytest.mark.parametrize("case", mc.CASES, ids=[c["id"] for c in mc.CASES])
def test_recorded_case(case):
    codes, res, eng = mc.run(case)
    rec = RECORD[case["id"]]
    assert codes == {k: rec[k] for k in ("row", "hess", "dense_writer")}, (case["id"], codes, rec)
    _, prob, inp = mc.problem(case)
    rows, cols = eng.jac_structure()
    for b in sorted({0, case["B"] - 1}):
        ref = mc.expected(case, prob, inp, b)
        if "jac_sparse" in case["want"]:
            ref["jac_sparse"] = prob.jacobian(inp["Z"][b], inp["X0"][b])[rows, cols]
        assert set(ref) == set(case["want"])
        for k, v in ref.items():
            _close(case, k, res[k][b], v)
        if "jac_dense" in res and mc.NETS[case["net"]][3] is None:      # (tanh: no derivative is zero by value) structural zeros are exact zeros (a caller-owned matrix gets the full matrix)
            assert np.array_equal(res["jac_dense"][b] != 0, ref["jac_dense"] != 0)
