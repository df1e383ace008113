"""Resident dense-Jacobian buffers, the constant entries: the -1 of every defect row and the +1 of every box row are written
once into a registered buffer, like its structural zeros, and the fused launch and post_scatter_kernel leave them alone.

The reference side of every check is THE SAME SEQUENCE OF CALLS in a child process started with NEMPC_JAC_RESIDENT=0 (the knob
is read once per process): one child for the whole module runs every sequence below and hands the arrays back in one file.
Every comparison is bit for bit (numpy.array_equal).  On top of that every engine-owned result is held against the structure
itself: -1 at (t nx + i, t nx + i), +1 at (H nx + t nx + i, t nx + i) with box rows, exactly 0.0 outside the pattern of
nempc_jac_structure.  The network is a 2/1, 2 x 64 tanh one in fp64 (the headline's compiled shape); H = 2 and H = 4 keep n even,
so the fused launch writes the matrix; B = 1, 15, 16, 17, 33 give B H rows in tiles of 16: a partial tile alone, single-tile
passes, and two- plus one-tile passes with a ragged last tile."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from oracle import nempc_oracle as orc

pytestmark = pytest.mark.gpu

DEFAULT = ("f", "grad", "g", "jac_dense")
NX, NU = 2, 1
_NET = orc.MLP.random(NX + NU, [64, 64], NX, seed=0)


def _setup(B, H, integrator="discret", box=None, kernel="auto"):
    """-> (engine, None): the 2/1, 2 x 64 tanh network in fp64 with a full quadratic + linear objective."""
    from pyneuralempc_amd import CallbackEngine
    eng = CallbackEngine(_NET.W, _NET.b, H, NX, NU, integrator=integrator, dtype=torch.float64, device="cuda:0", max_batch=B,
                         kernel=kernel)
    if box is not None:
        eng.set_box_rows(*box)
    eng.set_objective(Q=np.array([[1.0, 0.2], [0.1, 0.7]]), R=np.array([[0.3]]), xref=np.linspace(-1, 1, H * NX).reshape(H, NX),
                      uref=0.1, cx=0.05, cu=-0.2, QT=np.array([[2.0, 0.0], [0.3, 1.5]]))
    return eng, None


def _iterate(B, H, k):
    return orc.synthetic_inputs(B, H, NX, NU, seed=4 + 7 * k)


def _mask(eng):
    rows, cols = eng.jac_structure()
    mask = np.zeros((eng.m, eng.n), dtype=bool)
    mask[rows, cols] = True
    return mask


def _raw_eval(eng, B, Z, X0, jac):
    """nempc_eval with g and jac_dense only, straight through the C ABI, on the current stream."""
    g = torch.empty(B, eng.m, dtype=eng.dtype, device=Z.device)
    rc = eng.lib.nempc_eval(eng._handle, B, ctypes.c_void_p(Z.data_ptr()), ctypes.c_void_p(X0.data_ptr()), None, None,
                            ctypes.c_void_p(g.data_ptr()), ctypes.c_void_p(jac.data_ptr()), None, None, eng._stream())
    assert rc == 0, eng.lib.nempc_last_error()
    torch.cuda.synchronize()


BOX = (-2.0, 2.0)
HS, BS = (2, 4), (1, 15, 16, 17, 33)
OWNED = [(H, B, integ, box) for H, B, integ, box in itertools.product(HS, BS, ("discret", "unity"), (None, BOX))]
BOXCHANGE = [(2, 17), (4, 33), (4, 1)]
SMALLER = [(2, None), (4, BOX)]
CALLER = [(2, 17, None), (4, 33, BOX), (4, 15, None)]


def _name(kind, *args):
    return kind + ":" + ",".join("box" if a == BOX else str(a) for a in args)


def _dev(eng, B, H, k):
    Zh, X0h = _iterate(B, H, k)
    return eng.to_device(Zh), eng.to_device(X0h)


def _eval(eng, Z, X0, out=None):
    res = eng.eval(Z, X0, DEFAULT, out=out)
    torch.cuda.synchronize()
    return [res[k].cpu().numpy() for k in DEFAULT]


def _check_structure(eng, J, what):
    """J (B, m, n) of an engine-owned buffer: every constant present, every structural zero exactly 0.0."""
    hx = eng.H * NX
    k = np.arange(hx)
    assert np.all(J[:, k, k] == -1.0), what
    if eng.m == 2 * hx:
        assert np.all(J[:, hx + k, k] == 1.0), what
    assert np.all(J[:, ~_mask(eng)] == 0.0), what


def seq_owned(H, B, integ, box, kernel="auto", writer="row_launch", live=False):
    """Two evaluations with different Z into the engine's own (registered) buffer."""
    eng, _ = _setup(B, H, integrator=integ, box=box, kernel=kernel)
    outs = []
    for k in range(2):
        Z, X0 = _dev(eng, B, H, k)
        outs += _eval(eng, Z, X0)
        if live:
            assert eng.last_dense_writer == writer
            _check_structure(eng, outs[-1], (H, B, integ, box, k))
    if live:
        # the constants are left alone the only way it shows: a NaN planted on the -1 of row 0 survives an evaluation (last
        # use of eng -- planting it breaks the read-only contract of engine-owned outputs on purpose)
        buf = eng.eval(Z, X0, DEFAULT)["jac_dense"]
        torch.cuda.synchronize()
        buf[0, 0, 0] = float("nan")
        eng.eval(Z, X0, DEFAULT)
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[0, 0, 0])) and int(torch.isnan(buf).sum()) == 1, "a resident buffer's constant was rewritten"
    return outs


def seq_boxchange(H, B, live=False):
    """A registered evaluation, box rows on, box rows off again: two evaluations after each change (the first re-registers a
    fresh buffer of the new shape, the second finds it resident)."""
    eng, _ = _setup(B, H)
    outs = []
    k = 0
    for box in (None, BOX, None, BOX):
        if k:
            eng.set_box_rows(*(box if box else (None, None)))
        for _ in range(2):
            Z, X0 = _dev(eng, B, H, k)
            outs += _eval(eng, Z, X0)
            k += 1
            if live:
                assert eng.last_dense_writer == "row_launch"
                _check_structure(eng, outs[-1], (H, B, box, k))
    return outs


def seq_boxchange_one_allocation(H, B, live=False):
    """The same changes through the C ABI on ONE registered allocation: set_box_rows drops the registration (constants and
    zeros alike), the next evaluation writes the full matrix of the new shape over whatever the old one left behind."""
    eng, _ = _setup(B, H)
    reg = eng.lib.nempc_jac_dense_resident
    Z, X0 = _dev(eng, B, H, 0)
    raw = torch.empty(B * 2 * H * NX * eng.n, dtype=eng.dtype, device=Z.device)
    outs = []
    for box in (None, BOX, None):
        eng.set_box_rows(*(box if box else (None, None)))
        buf = raw[:B * eng.m * eng.n].view(B, eng.m, eng.n)
        for k in range(3):                               # unregistered (full matrix), then registered twice
            if k == 1:
                assert reg(eng._handle, ctypes.c_void_p(raw.data_ptr()), B) == 0
            Zk, X0k = _dev(eng, B, H, k)
            _raw_eval(eng, B, Zk, X0k, buf)
            outs.append(buf.cpu().numpy())
            if live:
                _check_structure(eng, outs[-1], (H, B, box, k))
    reg(eng._handle, ctypes.c_void_p(raw.data_ptr()), 0)
    return outs


def seq_smaller(H, box, live=False):
    """A registration for 33 problems evaluated with 17, then 33, then 15: the problems of each call are right, the rest keep
    what they held (zeros after the registration, the previous call's matrix later)."""
    Bmax = 33
    eng, _ = _setup(Bmax, H, box=box)
    reg = eng.lib.nempc_jac_dense_resident
    buf = torch.full((Bmax, eng.m, eng.n), float("nan"), dtype=eng.dtype, device="cuda:0")
    assert reg(eng._handle, ctypes.c_void_p(buf.data_ptr()), Bmax) == 0
    outs = []
    for k, B in enumerate((17, 33, 15)):
        Z, X0 = _dev(eng, Bmax, H, k)
        _raw_eval(eng, B, Z[:B].contiguous(), X0[:B].contiguous(), buf)
        outs.append(buf.cpu().numpy())
        if live:
            assert eng.last_dense_writer == "row_launch"
            _check_structure(eng, outs[-1][:17 if k == 0 else Bmax], (H, box, B))      # (every problem evaluated so far)
            if k == 0:
                assert np.all(outs[-1][17:] == 0.0)      # beyond the evaluated problems: still the registration's zeros
    reg(eng._handle, ctypes.c_void_p(buf.data_ptr()), 0)
    return outs


def seq_caller(H, B, box, live=False):
    """A caller-owned out= buffer full of NaN, after an evaluation into the engine's own buffer and again after it."""
    eng, _ = _setup(B, H, box=box)
    outs = []
    for k in range(2):
        Z, X0 = _dev(eng, B, H, k)
        outs += _eval(eng, Z, X0)
        mine = {"jac_dense": torch.full((B, eng.m, eng.n), float("nan"), dtype=eng.dtype, device=Z.device)}
        got = _eval(eng, Z, X0, out=mine)
        outs += got
        if live:
            assert not np.isnan(got[-1]).any()
            assert np.array_equal(got[-1], outs[-5]), "caller-owned and engine-owned matrices differ"
            _check_structure(eng, got[-1], (H, B, box, k))
    return outs


SEQS = {}
for c in OWNED:
    SEQS[_name("owned", *c)] = (seq_owned, c)
for c in BOXCHANGE:
    SEQS[_name("boxchange", *c)] = (seq_boxchange, c)
    SEQS[_name("boxchange1", *c)] = (seq_boxchange_one_allocation, c)
for c in SMALLER:
    SEQS[_name("smaller", *c)] = (seq_smaller, c)
for c in CALLER:
    SEQS[_name("caller", *c)] = (seq_caller, c)
SEQS["valu"] = (seq_owned, (2, 17, "discret", None, "valu"))
SEQS["valu:box"] = (seq_owned, (2, 17, "discret", BOX, "valu"))

_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_jac_resident_constants as t
arrays = {}
for name, (fn, args) in t.SEQS.items():
    for i, a in enumerate(fn(*args)):
        arrays[f"{name}#{i}"] = a
np.savez(sys.argv[2], **arrays)
"""


@pytest.fixture(scope="module")
def knob_off(tmp_path_factory):
    """Every sequence of this module under NEMPC_JAC_RESIDENT=0, computed once in one fresh child process."""
    path = str(tmp_path_factory.mktemp("jac_constants") / "off.npz")
    env = dict(os.environ, NEMPC_JAC_RESIDENT="0")
    r = subprocess.run([sys.executable, "-c", _CHILD, REPO, path], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return np.load(path)


def _against_knob_off(knob_off, name, **kw):
    fn, args = SEQS[name]
    got = fn(*args, live=True, **kw)
    for i, a in enumerate(got):
        ref = knob_off[f"{name}#{i}"]
        assert a.shape == ref.shape and np.array_equal(a, ref, equal_nan=True), (name, i)
    assert len([k for k in knob_off.files if k.startswith(name + "#")]) == len(got)


@pytest.mark.parametrize("case", OWNED, ids=lambda c: _name("owned", *c))
def test_engine_owned_buffer(knob_off, case):
    _against_knob_off(knob_off, _name("owned", *case))


@pytest.mark.parametrize("case", BOXCHANGE, ids=lambda c: _name("boxchange", *c))
def test_box_row_changes(knob_off, case):
    _against_knob_off(knob_off, _name("boxchange", *case))


@pytest.mark.parametrize("case", BOXCHANGE, ids=lambda c: _name("boxchange1", *c))
def test_box_row_changes_on_one_allocation(knob_off, case):
    _against_knob_off(knob_off, _name("boxchange1", *case))


@pytest.mark.parametrize("case", SMALLER, ids=lambda c: _name("smaller", *c))
def test_smaller_batch_than_registered(knob_off, case):
    _against_knob_off(knob_off, _name("smaller", *case))


@pytest.mark.parametrize("case", CALLER, ids=lambda c: _name("caller", *c))
def test_caller_owned_buffer_gets_every_entry(knob_off, case):
    _against_knob_off(knob_off, _name("caller", *case))


@pytest.mark.parametrize("name", ["valu", "valu:box"])
def test_post_scatter_kernel_path(knob_off, name):
    _against_knob_off(knob_off, name, writer="post_scatter_kernel")


def test_first_evaluation_captured_into_a_graph():
    """A registered buffer whose constants are still missing, first evaluated on a stream that is being captured: the fill
    would be recorded, not run, so that call takes the full-matrix path -- every replay writes the constants itself."""
    B, H = 17, 2
    eng, _ = _setup(B, H, box=BOX)
    Z, X0 = _dev(eng, B, H, 0)
    nan = torch.full((B, eng.m, eng.n), float("nan"), dtype=eng.dtype, device=Z.device)
    _raw_eval(eng, B, Z, X0, nan)                                # (full matrix; the same request, so nothing is set up later)
    ref = nan.cpu().numpy()
    assert not np.isnan(ref).any()
    buf, g = torch.full_like(nan, float("nan")), torch.empty(B, eng.m, dtype=eng.dtype, device=Z.device)
    reg = eng.lib.nempc_jac_dense_resident
    assert reg(eng._handle, ctypes.c_void_p(buf.data_ptr()), B) == 0
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=side):
        rc = eng.lib.nempc_eval(eng._handle, B, ctypes.c_void_p(Z.data_ptr()), ctypes.c_void_p(X0.data_ptr()), None, None,
                                ctypes.c_void_p(g.data_ptr()), ctypes.c_void_p(buf.data_ptr()), None, None,
                                ctypes.c_void_p(side.cuda_stream))
    assert rc == 0, eng.lib.nempc_last_error()
    torch.cuda.synchronize()
    assert int((buf != 0).sum()) == 0                            # recorded, not run
    for _ in range(2):
        buf[0, 0, 0] = float("nan")                              # on a -1: a replay that skipped the constants would leave it
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy(), ref)
    _raw_eval(eng, B, Z, X0, buf)                                # an ordinary call: fills the constants, then resident
    assert np.array_equal(buf.cpu().numpy(), ref)
    buf[0, 0, 1] = float("nan")                                  # a structural zero is left alone now
    _raw_eval(eng, B, Z, X0, buf)
    assert bool(torch.isnan(buf[0, 0, 1])) and int(torch.isnan(buf).sum()) == 1
    reg(eng._handle, ctypes.c_void_p(buf.data_ptr()), 0)
