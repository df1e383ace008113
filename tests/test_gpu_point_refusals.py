"""GPU: what the three post-solve point calls (nempc_kkt_residual, nempc_sensitivity, nempc_kkt_solve) refuse, through the raw
C ABI, and in which ORDER where two refusals apply at once.

The expected (return code, message fragment) pairs were recorded from the library as it stood before the three entry points
came to share one prologue (csrc/nempc_api.hip); they pin the texts and the order of the checks that prologue has to keep.
Smallest shape the calls accept: H = 2, nx = 2, nu = 1, one hidden layer of 8, DISCRET, fp64, B = 2.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import nempc_oracle as orc

pytestmark = pytest.mark.gpu

H, NX, NU, B = 2, 2, 1, 2
N, HX = H * (NX + NU), H * NX
EINVAL, EUNSUPPORTED = -1, -5
ENTRIES = ("nempc_kkt_residual", "nempc_sensitivity", "nempc_kkt_solve")
BUILT_FOR = {"nempc_kkt_residual": b"(the band product is built for the tiles of a plain model)",
             "nempc_sensitivity": b"(the sweep is built for the stages of a plain model)",
             "nempc_kkt_solve": b"(the sweep is built for the stages of a plain model)"}
REQUIRED = {"nempc_kkt_residual": b"null argument (Z, X0, lam and r are required)",
            "nempc_sensitivity": b"null argument (Z, X0, lam and status are required)",
            "nempc_kkt_solve": b"null argument (Z, X0, lam, rz and status are required)"}
# a batch beyond the tracking binding: nempc_kkt_residual has no check of its own, its evaluation refuses
TRACKING = {"nempc_kkt_residual": b"nempc_eval: B exceeds the batch the bound tracking data cover",
            "nempc_sensitivity": b"nempc_sensitivity: B exceeds the batch the bound tracking data cover",
            "nempc_kkt_solve": b"nempc_kkt_solve: B exceeds the batch the bound tracking data cover"}


def _engine(window):
    from pyneuralempc_amd import CallbackEngine
    net = orc.MLP.random(window * (NX + NU), [8], NX, seed=0)
    return CallbackEngine(net.W, net.b, H, NX, NU, integrator="discret", dtype=torch.float64, device="cuda:0", max_batch=B,
                          rolling_window=window)


def _caller(eng):
    """-> call(entry, B, Z=..., out=...): the entry point on valid device arrays of B + 1 problems, with `Z` (a required pointer)
    and the outputs replaceable; returns (return code, message)."""
    rng = np.random.default_rng(0)
    dev = lambda *shape: eng.to_device(rng.uniform(-0.5, 0.5, size=shape))
    # (lam = 0: the Hessian of the Lagrangian is the objective's, so every accepted call ends with status 0)
    t = {"Z": dev(B + 1, N), "X0": dev(B + 1, NX), "lam": 0.0 * dev(B + 1, HX), "rz": dev(B + 1, 1, N), "r": dev(B + 1, 4),
         "dU0": dev(B + 1, NU, NX), "v": dev(B + 1, 1, N), "status": torch.zeros(B + 1, dtype=torch.int32, device=eng.device)}
    p = {k: ctypes.c_void_p(v.data_ptr()) for k, v in t.items()}

    def call(entry, nb, Z=p["Z"], out=True, nrhs=1):
        head = (eng._handle, nb, Z, p["X0"], p["lam"], None, None, None, None)
        if entry == "nempc_kkt_residual":
            rc = eng.lib.nempc_kkt_residual(*head, p["r"], None, None)
        elif entry == "nempc_sensitivity":
            rc = eng.lib.nempc_sensitivity(*head, p["dU0"] if out else None, None, None, None, p["status"], None)
        else:
            rc = eng.lib.nempc_kkt_solve(*head, nrhs, p["rz"], None, p["v"] if out else None, None, None, p["status"], None)
        return rc, eng.lib.nempc_last_error()

    call.keep = t
    return call


def _refused(got, code, *fragments):
    rc, msg = got
    assert rc == code and all(f in msg for f in fragments), (rc, msg, code, fragments)


def test_point_calls_refuse_with_the_recorded_codes_and_messages_in_the_recorded_order():
    roll = _engine(2)
    call = _caller(roll)
    for e in ENTRIES:
        # a rolling-window handle, before anything else: the batch is outside max_batch and Z is null as well
        _refused(call(e, B), EUNSUPPORTED, e.encode() + b": rolling_window > 1 handles are not supported", BUILT_FOR[e])
        _refused(call(e, B + 1, Z=None), EUNSUPPORTED, e.encode() + b": rolling_window > 1 handles are not supported")
    eng = _engine(1)
    call = _caller(eng)
    one = lambda d: torch.zeros(1, H, d, dtype=torch.float64, device=eng.device)
    for e in ENTRIES:
        who = e.encode()
        assert call(e, B)[0] == 0
        # B > max_batch, before the null pointer
        _refused(call(e, B + 1), EINVAL, who + b": B outside [0, max_batch]")
        _refused(call(e, B + 1, Z=None), EINVAL, who + b": B outside [0, max_batch]")
        _refused(call(e, -1), EINVAL, who + b": B outside [0, max_batch]")
        # a null required pointer, before the coverage of the bindings
        _refused(call(e, B, Z=None), EINVAL, who + b": " + REQUIRED[e])
        eng.bind_bounds(ulb=one(NU) - 1.0)
        _refused(call(e, B, Z=None), EINVAL, who + b": " + REQUIRED[e])
        # B beyond the bounds binding
        _refused(call(e, B), EINVAL, who + b": B exceeds the batch the bound per-problem bounds cover")
        assert call(e, 1)[0] == 0
        # ... and beyond the tracking binding: where the entry point checks that itself, it does so first
        eng.bind_tracking(xref=one(NX))
        if e == "nempc_kkt_residual":
            _refused(call(e, B), EINVAL, who + b": B exceeds the batch the bound per-problem bounds cover")
        else:
            _refused(call(e, B), EINVAL, TRACKING[e])
        eng.bind_bounds()
        _refused(call(e, B), EINVAL, TRACKING[e])
        assert call(e, 1)[0] == 0
        eng.bind_tracking()
        assert call(e, B)[0] == 0
    # no output asked for: refused even for an empty batch, but after the batch range
    no_out = b"nempc_sensitivity: no output asked for (dU0, dZ, dlam, gains all null)"
    _refused(call("nempc_sensitivity", 0, out=False), EINVAL, no_out)
    _refused(call("nempc_sensitivity", B, out=False, Z=None), EINVAL, no_out)
    _refused(call("nempc_sensitivity", B + 1, out=False), EINVAL, b"nempc_sensitivity: B outside [0, max_batch]")
    assert call("nempc_sensitivity", 0)[0] == 0 and call("nempc_kkt_residual", 0, Z=None)[0] == 0
    # nempc_kkt_solve: the batch range, then nrhs, then the outputs, then the empty batch, then the pointers
    _refused(call("nempc_kkt_solve", B + 1, nrhs=0), EINVAL, b"nempc_kkt_solve: B outside [0, max_batch]")
    _refused(call("nempc_kkt_solve", 0, nrhs=65, out=False), EINVAL, b"nempc_kkt_solve: nrhs outside [1, 64]")
    _refused(call("nempc_kkt_solve", 0, out=False), EINVAL, b"nempc_kkt_solve: no output asked for (v, w, gx0 all null)")
    assert call("nempc_kkt_solve", 0, Z=None)[0] == 0
    torch.cuda.synchronize()
    assert call.keep["status"][:B].tolist() == [0, 0]
