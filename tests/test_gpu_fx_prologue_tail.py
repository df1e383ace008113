"""The fused one-launch evaluation (rows_coopfx_kernel<..., FUSE>) at the smallest shapes at which its prologue and its
output stage can go wrong: the grid size arrives in the leading kernel arguments (the kernel pairs workgroup i with
i + ceil(grid / 2) for the objective), the dense-matrix pointer is fetched behind the prologue's loads, and every
(row, state) item of a pass has to be written by exactly one lane.

Every case runs the compiled 2/1, 2 x 64 fp64 tanh shape through CallbackEngine.bind and is compared two ways:
  (a) bit for bit with the separate-launch path of the same handle (row launch + the library's own assembly and objective
      launches: what test_gpu_fullsize.test_c2_fused_evaluation_full_size uses as its unfused side), and
  (b) with the CPU oracle to 1e-12 absolute, structural zeros of the dense Jacobian exactly zero;
then once more after a second bind to fresh output buffers pre-filled with NaN (an item that nothing writes would show).
The dense rows leave the fixed-shape kernel as 16-byte vectors, so at an odd n (H = 5, H = 1: n = 3 H) the dense request
is not served by it at all but by rows_coop_kernel's one-launch dense form.  That is another kernel family, which agrees
with the separate launches (the fixed-shape kernel's rows + assembly) to rounding only -- g and jac_dense differ by one
ulp, 2.2e-16 -- so comparison (a) has no bit-for-bit meaning there: those two cases assert the path taken, the oracle,
the structural zeros and the NaN re-bind, and the same shapes run the fixed-shape kernel bit for bit through the sparse
contract, which has no such limit."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import nempc_oracle as orc
from test_gpu_fullsize import ALL, DEFAULT, _engine, _slices

pytestmark = pytest.mark.gpu

ABS = dict(rtol=0.0, atol=1e-12)
NX, NU = 2, 1
SPARSE = ("f", "grad", "g", "jac_sparse")

_NET = orc.MLP.random(NX + NU, [64, 64], NX, seed=0)


def _objective(H):
    return dict(Q=np.array([[1.0, 0.2], [0.1, 0.7]]), R=np.array([[0.3]]), xref=np.linspace(-1, 1, H * NX).reshape(H, NX),
                uref=np.full((H, NU), 0.1), cx=np.full((H, NX), 0.05), cu=np.full((H, NU), -0.2),
                QT=np.array([[2.0, 0.0], [0.3, 1.5]]))


def _setup(B, H, integrator="discret", box=None):
    eng = _engine(_NET, H, NX, NU, B, integrator=integrator, box=box)
    ob = _objective(H)
    eng.set_objective(Q=ob["Q"], R=ob["R"], xref=ob["xref"], uref=0.1, cx=0.05, cu=-0.2, QT=ob["QT"])
    prob = orc.Problem(_NET, H, NX, NU, orc.UNITY if integrator == "unity" else orc.DISCRET, box=box, **ob)
    Zh, X0h = orc.synthetic_inputs(B, H, NX, NU, seed=4)
    return eng, prob, Zh, X0h


def _bound(eng, Z, X0, want, out=None):
    """One evaluation through a bound launcher; -> clones of its outputs."""
    launch, outs = eng.bind(Z, X0, want, out=out)
    if out is not None:
        for v in out.values():
            v.fill_(float("nan"))       # (bind itself evaluated once into them)
    launch()
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in outs.items()}


def _check(B, H, integrator="discret", box=None, want=DEFAULT):
    eng, prob, Zh, X0h = _setup(B, H, integrator, box)
    Z, X0 = eng.to_device(Zh), eng.to_device(X0h)
    fused = _bound(eng, Z, X0, want)
    other_family = "jac_dense" in want and eng.n % 2 == 1      # (module docstring)
    if other_family:
        assert eng.last_row_kernel == "rows_coop_kernel+dense"
    else:
        assert eng.last_row_kernel == ("rows_coopfx_kernel+sparse" if "jac_sparse" in want else "rows_coopfx_kernel")
    # (a) the separate launches of the same handle, bit for bit
    unf = {k: v.clone() for k, v in eng.eval(Z, X0, ALL).items()}
    for k in want:
        print(f"B={B} H={H} {k}: max |fused - separate launches| = {float((fused[k] - unf[k]).abs().max()):.3e}")
    if not other_family:
        for k in want:
            assert torch.equal(fused[k], unf[k]), k
    # (b) the oracle, and exact structural zeros
    rows, cols = eng.jac_structure()
    if "jac_dense" in want:
        mask = np.zeros((eng.m, eng.n), dtype=bool)
        mask[rows, cols] = True
        jac = fused["jac_dense"].cpu().numpy()
        assert np.all(jac[:, ~mask] == 0.0)
    for sl in _slices(B):
        f, grad, g, J = prob.eval_batch(Zh[sl], X0h[sl])
        ref = {"f": f, "grad": grad, "g": g, "jac_dense": J, "jac_sparse": J[:, rows, cols]}
        for k in want:
            np.testing.assert_allclose(fused[k][sl].cpu().numpy(), ref[k], err_msg=k, **ABS)
    # once more into fresh buffers full of NaN
    fresh = {k: torch.empty_like(v) for k, v in fused.items()}
    again = _bound(eng, Z, X0, want, out=fresh)
    for k in want:
        assert torch.equal(again[k], fused[k]), k
    return eng, Z, X0, fused


def test_odd_grid_unpaired_middle_workgroup():
    """B = 3, H = 16: 3 tiles on 3 workgroups -- workgroup 0 evaluates the objective of its own problems and of workgroup
    2's, workgroup 1 (the unpaired middle one) its own only; the pairing uses the grid size passed in the arguments."""
    _check(3, 16)


def test_single_workgroup_ragged_tile():
    """B = 1, H = 5: one tile of 5 rows (row masking; H < 16).  n = 15 is odd: rows_coop_kernel+dense serves the request
    (module docstring); the fixed-shape kernel at this shape: the next test."""
    _check(1, 5)


@pytest.mark.parametrize("H,want", [(5, SPARSE), (6, DEFAULT), (6, SPARSE)])
def test_single_workgroup_ragged_tile_fixed_shape_kernel(H, want):
    """The same in one launch: the band values at H = 5 (no 16-byte rows needed), both contracts at H = 6 (n even)."""
    _check(1, H, want=want)


def test_trajectory_of_one_step():
    """B = 5, H = 1: invH == 0 (row == problem), no state block at t >= 1, several problems in the one tile (n = 3 is odd:
    rows_coop_kernel+dense, module docstring)."""
    _check(5, 1)


def test_trajectory_of_one_step_fixed_shape_kernel():
    """B = 5, H = 1 through the sparse contract, one launch of the fixed-shape kernel at any n."""
    _check(5, 1, want=SPARSE)


def test_ragged_last_tile_single_tile_workgroups():
    """B = 7, H = 20: 140 rows = 8 full tiles and one of 12 rows, one tile per workgroup (the NT = 1 pass)."""
    _check(7, 20)


def test_more_tiles_than_workgroups_mixed_passes():
    """More tiles than the grid holds workgroups, unevenly: several passes per workgroup (3 tiles, then a shorter one, the
    next pass's inputs in flight meanwhile), some workgroups with one tile more than the others.  B = 2200 on 256 CUs
    (2750 tiles on 512 workgroups); on a device with another CU count the next B at which a workgroup has >= 5 tiles and
    the split leaves a remainder (two workgroups of this shape per CU)."""
    from pyneuralempc_amd import _lib
    lib = _lib.load()
    H = 20
    probe = _engine(_NET, H, NX, NU, 1)
    num_cus = lib.nempc_num_cus(probe._handle)
    del probe
    g, q, r = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    B = 2200
    while True:
        assert lib.nempc_plan_grid((B * H + 15) // 16, num_cus, 2, ctypes.byref(g), ctypes.byref(q), ctypes.byref(r)) == 0
        if q.value >= 5 and r.value != 0:
            break
        B += 37
    _check(B, H)


def test_box_rows():
    """B = 7, H = 20 with box rows: the +1 selectors and g's box half; the background zeros are cut at problem
    boundaries."""
    _check(7, 20, box=(-2.0, 2.0))


def test_sparse_contract_band_values():
    """B = 7, H = 20, band values instead of the dense matrix: bit for bit the dense result gathered through
    nempc_jac_structure."""
    eng, Z, X0, sp = _check(7, 20, want=SPARSE)
    dense = _bound(eng, Z, X0, DEFAULT)
    rows, cols = eng.jac_structure()
    assert torch.equal(sp["jac_sparse"], dense["jac_dense"][:, torch.as_tensor(rows.astype(np.int64), device=Z.device),
                                                            torch.as_tensor(cols.astype(np.int64), device=Z.device)])
    for k in ("f", "grad", "g"):
        assert torch.equal(sp[k], dense[k]), k


@pytest.mark.parametrize("want", [("g", "jac_dense"), ("f", "g")])
def test_output_subsets(want):
    """B = 7, H = 20: without the objective (its copies of Z are not fetched), and defects + objective only (no reverse
    sweep, no dense rows: the dense-matrix pointer the prologue fetches is null)."""
    _check(7, 20, want=want)


def test_unity_transcription():
    """B = 7, H = 20, Unity: no identity added to the state block (ident = 0)."""
    _check(7, 20, integrator="unity")
