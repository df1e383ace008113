"""Resident dense-Jacobian buffers (nempc_jac_dense_resident): the engine's own jac_dense is zero-filled once, when it is
created, and every evaluation into it writes the structural non-zeros only.

The reference side of every check is THE SAME HANDLE evaluated into a caller-supplied `out=` buffer pre-filled with NaN:
caller buffers are never registered, so that is the full-matrix path.  The comparison is bit for bit (torch.equal), the
structural zeros exactly 0.0, and both sides are also held against the CPU oracle at the 1e-12 absolute of
test_gpu_fx_prologue_tail (fp32: the 1e-4 of scale of test_gpu_parity._f32_close -- 1e-12 is below fp32's resolution).
The network is that module's 2/1, 2 x 64 tanh one.  That an evaluation really left the zeros alone is checked the only way
it shows: a NaN planted on a structural zero of the engine's buffer is still there afterwards (the engine is dropped
right after -- planting it breaks the read-only contract of engine-owned outputs on purpose).
The odd-n cases run rows_coop_kernel+dense, which agrees with the separate launches to rounding only (that module's
docstring); both sides here are that kernel, so they are compared bit for bit as well.  It still writes its background
zeros into a resident buffer (correct, only not faster), so the planted-NaN check is not made there."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from oracle import nempc_oracle as orc
from test_gpu_fullsize import ALL, DEFAULT
from test_gpu_fx_prologue_tail import NX, NU, _NET, _objective

pytestmark = pytest.mark.gpu

ABS = dict(rtol=0.0, atol=1e-12)


def _setup(B, H, integrator="discret", box=None, dtype=torch.float64, kernel="auto"):
    from pyneuralempc_amd import CallbackEngine
    eng = CallbackEngine(_NET.W, _NET.b, H, NX, NU, integrator=integrator, dtype=dtype, device="cuda:0", max_batch=B,
                         kernel=kernel)
    if box is not None:
        eng.set_box_rows(*box)
    ob = _objective(H)
    eng.set_objective(Q=ob["Q"], R=ob["R"], xref=ob["xref"], uref=0.1, cx=0.05, cu=-0.2, QT=ob["QT"])
    prob = orc.Problem(_NET, H, NX, NU, orc.UNITY if integrator == "unity" else orc.DISCRET, box=box, **ob)
    return eng, prob


def _iterate(B, H, k):
    return orc.synthetic_inputs(B, H, NX, NU, seed=4 + 7 * k)


def _shapes(eng, B):
    return {"f": (B,), "grad": (B, eng.n), "g": (B, eng.m), "jac_dense": (B, eng.m, eng.n),
            "jac_tiles": (B, eng.H, eng.nx, eng.nin), "jac_sparse": (B, eng.nnz_jac)}


def _full(eng, Z, X0, want):
    """The non-resident path: caller-supplied outputs full of NaN."""
    sh = _shapes(eng, Z.shape[0])
    out = {k: torch.full(sh[k], float("nan"), dtype=eng.dtype, device=Z.device) for k in want}
    res = eng.eval(Z, X0, want, out=out)
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in res.items()}


def _own(eng, Z, X0, want):
    """Into the engine's own (resident) buffers."""
    res = eng.eval(Z, X0, want)
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in res.items()}


def _mask(eng):
    rows, cols = eng.jac_structure()
    mask = np.zeros((eng.m, eng.n), dtype=bool)
    mask[rows, cols] = True
    return mask


def _compare(eng, prob, Zh, X0h, got, ref, want, what):
    for k in want:
        a, b = got[k], ref[k]
        print(f"{what} {k}: max |resident - full| = {float((a - b).abs().max()):.3e}, NaN: {int(torch.isnan(a).sum())}")
    for k in want:
        assert torch.equal(got[k], ref[k]), (what, k)
    if "jac_dense" in want:
        jac = got["jac_dense"].cpu().numpy()
        assert np.all(jac[:, ~_mask(eng)] == 0.0), what
    if prob is not None:
        f, grad, g, J = prob.eval_batch(Zh, X0h)
        orf = {"f": f, "grad": grad, "g": g, "jac_dense": J}
        for k in want:
            if k in orf:
                v = got[k].cpu().numpy().astype(np.float64)
                if eng.dtype == torch.float32:
                    scale = max(1.0, np.abs(orf[k]).max())
                    assert np.abs(v - orf[k]).max() / scale < 1e-4, (what, k)
                else:
                    np.testing.assert_allclose(v, orf[k], err_msg=f"{what} {k}", **ABS)


def _assert_zeros_left_alone(eng, Z, X0, want=DEFAULT):
    """A NaN on a structural zero of the engine's buffer survives an evaluation: the fast path is on.  Last use of eng."""
    buf = eng.eval(Z, X0, want)["jac_dense"]
    torch.cuda.synchronize()
    r, c = [int(v[0]) for v in np.nonzero(~_mask(eng))]
    buf[0, r, c] = float("nan")
    eng.eval(Z, X0, want)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[0, r, c])), "the evaluation rewrote a structural zero of a resident buffer"
    assert int(torch.isnan(buf).sum()) == 1


def _three_iterates(B, H, kernel_name, iterates=3, want=DEFAULT, zeros_left_alone=True, **kw):
    eng, prob = _setup(B, H, **kw)
    Zh, X0h = _iterate(B, H, 0)
    Z, X0 = eng.to_device(Zh), eng.to_device(X0h)
    for k in range(iterates):
        if k:
            Zh, X0h = _iterate(B, H, k)
            Z.copy_(eng.to_device(Zh)); X0.copy_(eng.to_device(X0h))      # the next iterate, in place
        got = _own(eng, Z, X0, want)
        assert eng.last_row_kernel == kernel_name
        ref = _full(eng, Z, X0, want)
        assert eng.last_row_kernel == kernel_name
        _compare(eng, prob, Zh, X0h, got, ref, want, f"B={B} H={H} iterate {k}")
    if zeros_left_alone:
        _assert_zeros_left_alone(eng, Z, X0, want)


@pytest.mark.parametrize("B,H", [(7, 20), (3, 16)])
def test_fused_kernel_three_iterates(B, H):
    """1. B = 7, H = 20 (ragged last tile, single-tile workgroups) and B = 3, H = 16: three evaluations into the engine's
    buffer with Z / X0 overwritten in place between them, each bit-equal to the non-resident evaluation of that iterate."""
    _three_iterates(B, H, "rows_coopfx_kernel")


def test_fused_kernel_box_rows():
    """2. B = 7, H = 20 with box rows (-2, 2): the +1 selectors, and the zero runs that are cut at problem boundaries."""
    _three_iterates(7, 20, "rows_coopfx_kernel", box=(-2.0, 2.0))


def test_fused_kernel_unity():
    """3. The same under Unity (no identity in the state block)."""
    _three_iterates(7, 20, "rows_coopfx_kernel", integrator="unity")


def test_fused_kernel_fp32():
    """4. fp32 with H = 4: n = 12, a multiple of the four floats of a 16-byte vector."""
    _three_iterates(7, 4, "rows_coopfx_kernel", dtype=torch.float32)


def test_mixed_writers_into_one_resident_buffer():
    """5. One resident buffer, four writers in turn, bit-equal after each: the fused launch, the row launch + assembly
    launch (ALL), the launch without the objective, the fused launch at a new iterate."""
    B, H = 7, 20
    eng, prob = _setup(B, H)
    Zh, X0h = _iterate(B, H, 0)
    Z, X0 = eng.to_device(Zh), eng.to_device(X0h)
    ptrs = set()
    for step, want in enumerate((DEFAULT, ALL, ("g", "jac_dense"), DEFAULT)):
        if step == 3:
            Zh, X0h = _iterate(B, H, 1)
            Z.copy_(eng.to_device(Zh)); X0.copy_(eng.to_device(X0h))
        res = eng.eval(Z, X0, want)
        torch.cuda.synchronize()
        ptrs.add(res["jac_dense"].data_ptr())
        got = {k: v.clone() for k, v in res.items()}
        ref = _full(eng, Z, X0, want)
        _compare(eng, prob, Zh, X0h, got, ref, want, f"writer {step} {want}")
    assert len(ptrs) == 1
    _assert_zeros_left_alone(eng, Z, X0, ALL)          # (the assembly launch leaves them alone as well)


@pytest.mark.parametrize("B,H", [(1, 5), (5, 1)])
def test_odd_n_cooperative_kernel(B, H):
    """6. Odd n (15 and 3): rows_coop_kernel's one-launch dense form into a resident buffer, two iterates."""
    _three_iterates(B, H, "rows_coop_kernel+dense", iterates=2, zeros_left_alone=False)


def test_valu_kernel_assembly_path():
    """7. kernel="valu", B = 3, H = 6: the row launch + assembly launch on a resident buffer, two iterates."""
    eng, prob = _setup(3, 6, kernel="valu")
    assert eng.kernel_variant == "valu"
    Zh, X0h = _iterate(3, 6, 0)
    Z, X0 = eng.to_device(Zh), eng.to_device(X0h)
    for k in range(2):
        if k:
            Zh, X0h = _iterate(3, 6, k)
            Z.copy_(eng.to_device(Zh)); X0.copy_(eng.to_device(X0h))
        _compare(eng, prob, Zh, X0h, _own(eng, Z, X0, DEFAULT), _full(eng, Z, X0, DEFAULT), DEFAULT, f"valu iterate {k}")
    _assert_zeros_left_alone(eng, Z, X0)


def _raw_eval(eng, B, Z, X0, jac):
    """nempc_eval with g and jac_dense only, straight through the C ABI, on the current stream."""
    g = torch.empty(B, eng.m, dtype=eng.dtype, device=Z.device)
    rc = eng.lib.nempc_eval(eng._handle, B, ctypes.c_void_p(Z.data_ptr()), ctypes.c_void_p(X0.data_ptr()), None, None,
                            ctypes.c_void_p(g.data_ptr()), ctypes.c_void_p(jac.data_ptr()), None, None, eng._stream())
    assert rc == 0, eng.lib.nempc_last_error()
    torch.cuda.synchronize()


def test_c_abi_smaller_batch_and_unregister():
    """8a/8b. A registration for B = 7 evaluated with B = 4 on the same pointer: the first four problems are correct, the
    rest untouched.  Unregistered and filled with NaN, the buffer gets the full matrix back."""
    from pyneuralempc_amd import _lib
    B, H = 7, 20
    eng, prob = _setup(B, H)
    Zh, X0h = _iterate(B, H, 0)
    Z, X0 = eng.to_device(Zh), eng.to_device(X0h)
    ref = _full(eng, Z, X0, ("g", "jac_dense"))["jac_dense"]
    reg = eng.lib.nempc_jac_dense_resident
    buf = torch.full((B, eng.m, eng.n), float("nan"), dtype=eng.dtype, device=Z.device)
    assert reg(eng._handle, ctypes.c_void_p(buf.data_ptr()), B) == 0
    assert int((buf != 0).sum()) == 0                  # the call returns after its zero fill
    assert reg(eng._handle, ctypes.c_void_p(buf.data_ptr()), B + 1) == _lib.EINVAL        # beyond max_batch
    buf[4:] = 7.0                                      # a mark the evaluation of four problems must not touch
    _raw_eval(eng, 4, Z[:4].contiguous(), X0[:4].contiguous(), buf)
    assert torch.equal(buf[:4], ref[:4])
    assert bool((buf[4:] == 7.0).all())
    assert eng.last_row_kernel == "rows_coopfx_kernel"
    # more problems than registered: the full path (the marks are overwritten, the zeros rewritten)
    assert reg(eng._handle, ctypes.c_void_p(buf.data_ptr()), 4) == 0
    buf[4:] = 7.0
    _raw_eval(eng, B, Z, X0, buf)
    assert torch.equal(buf, ref)
    # unregister (twice: the second time the pointer is unknown, which is not an error), NaN, evaluate
    assert reg(eng._handle, ctypes.c_void_p(buf.data_ptr()), 0) == 0
    assert reg(eng._handle, ctypes.c_void_p(buf.data_ptr()), 0) == 0
    buf.fill_(float("nan"))
    _raw_eval(eng, B, Z, X0, buf)
    assert torch.equal(buf, ref)


def test_c_abi_set_box_rows_drops_registrations():
    """8c. set_box_rows on, off, on across evaluations into ONE registered allocation: never a stale +1, never a NaN --
    every change of the rows drops the registration, so the next evaluation writes the full matrix of the new shape."""
    B, H = 7, 20
    eng, _ = _setup(B, H)
    Zh, X0h = _iterate(B, H, 0)
    Z, X0 = eng.to_device(Zh), eng.to_device(X0h)
    reg = eng.lib.nempc_jac_dense_resident
    raw = torch.empty(B * 2 * H * NX * eng.n, dtype=eng.dtype, device=Z.device)      # room for the shape with box rows
    for box in ((-2.0, 2.0), None, (-2.0, 2.0)):
        eng.set_box_rows(*(box if box else (None, None)))
        prob = orc.Problem(_NET, H, NX, NU, orc.DISCRET, box=box, **_objective(H))
        buf = raw[:B * eng.m * eng.n].view(B, eng.m, eng.n)
        raw.fill_(float("nan"))                        # (the registration of the previous shape must be gone by now)
        _raw_eval(eng, B, Z, X0, buf)
        ref = _full(eng, Z, X0, ("g", "jac_dense"))["jac_dense"]
        assert torch.equal(buf, ref), box
        np.testing.assert_allclose(buf.cpu().numpy(), prob.eval_batch(Zh, X0h)[3], **ABS)
        assert reg(eng._handle, ctypes.c_void_p(raw.data_ptr()), B) == 0
        _raw_eval(eng, B, Z, X0, buf)                  # ... and once on the fast path of this shape
        assert torch.equal(buf, ref), box
    # the engine's own buffers across the same changes
    for box in ((-2.0, 2.0), None, (-2.0, 2.0)):
        eng.set_box_rows(*(box if box else (None, None)))
        for _ in range(2):
            got = _own(eng, Z, X0, DEFAULT)
            _compare(eng, None, Zh, X0h, got, _full(eng, Z, X0, DEFAULT), DEFAULT, f"box {box}")


def test_c_abi_ninth_registration_is_refused_and_harmless():
    """8d. A table of eight: the ninth registration returns NEMPC_EFULL, and evaluations into that buffer are still
    correct (full matrix)."""
    from pyneuralempc_amd import _lib
    B, H = 3, 16
    eng, _ = _setup(B, H)
    Zh, X0h = _iterate(B, H, 0)
    Z, X0 = eng.to_device(Zh), eng.to_device(X0h)
    ref = _full(eng, Z, X0, ("g", "jac_dense"))["jac_dense"]
    reg = eng.lib.nempc_jac_dense_resident
    bufs = [torch.full((B, eng.m, eng.n), float("nan"), dtype=eng.dtype, device=Z.device) for _ in range(9)]
    for b in bufs[:8]:
        assert reg(eng._handle, ctypes.c_void_p(b.data_ptr()), B) == 0
    assert reg(eng._handle, ctypes.c_void_p(bufs[8].data_ptr()), B) == _lib.EFULL
    assert bool(torch.isnan(bufs[8]).all())            # refused: not even zero-filled
    for b in bufs:
        _raw_eval(eng, B, Z, X0, b)
        assert torch.equal(b, ref)
    # the engine's own buffer finds the table full: it silently stays on the full-matrix path
    _compare(eng, None, Zh, X0h, _own(eng, Z, X0, DEFAULT), _full(eng, Z, X0, DEFAULT), DEFAULT, "table full")
    # a slot freed is a slot usable
    assert reg(eng._handle, ctypes.c_void_p(bufs[0].data_ptr()), 0) == 0
    assert reg(eng._handle, ctypes.c_void_p(bufs[8].data_ptr()), B) == 0
    _raw_eval(eng, B, Z, X0, bufs[8])
    assert torch.equal(bufs[8], ref)
    for b in bufs:
        reg(eng._handle, ctypes.c_void_p(b.data_ptr()), 0)


_CHILD = r"""
import sys
import numpy as np, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_jac_resident as t
eng, _ = t._setup(7, 20)
Zh, X0h = t._iterate(7, 20, 0)
Z, X0 = eng.to_device(Zh), eng.to_device(X0h)
outs = []
for k in range(2):
    if k:
        Zh, X0h = t._iterate(7, 20, k)
        Z.copy_(eng.to_device(Zh)); X0.copy_(eng.to_device(X0h))
    r = t._own(eng, Z, X0, t.DEFAULT)
    outs += [r[n].cpu().numpy() for n in t.DEFAULT]
# the switch is off: a NaN planted on a structural zero is overwritten by the next evaluation
buf = eng.eval(Z, X0)["jac_dense"]
r_, c_ = [int(v[0]) for v in np.nonzero(~t._mask(eng))]
buf[0, r_, c_] = float("nan")
eng.eval(Z, X0); torch.cuda.synchronize()
assert float(buf[0, r_, c_]) == 0.0
np.savez(sys.argv[2], *outs)
"""


def test_knob_off_in_a_child_process(tmp_path):
    """9. NEMPC_JAC_RESIDENT=0 in a fresh child process: bit-equal outputs to the default of this process."""
    path = str(tmp_path / "off.npz")
    env = dict(os.environ, NEMPC_JAC_RESIDENT="0")
    r = subprocess.run([sys.executable, "-c", _CHILD, REPO, path], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    off = np.load(path)
    eng, _ = _setup(7, 20)
    Zh, X0h = _iterate(7, 20, 0)
    Z, X0 = eng.to_device(Zh), eng.to_device(X0h)
    i = 0
    for k in range(2):
        if k:
            Zh, X0h = _iterate(7, 20, k)
            Z.copy_(eng.to_device(Zh)); X0.copy_(eng.to_device(X0h))
        got = _own(eng, Z, X0, DEFAULT)
        for n in DEFAULT:
            assert np.array_equal(got[n].cpu().numpy(), off[f"arr_{i}"]), (k, n)
            i += 1
    _assert_zeros_left_alone(eng, Z, X0)
