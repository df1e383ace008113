"""GPU: nempc_weight_grad / CallbackEngine.weight_grad against tests/weight_grad_reference.py on the cases of its table, and
autograd.solve(..., weights=...) end to end.

Tolerance (normalised by max |gtheta|): 8 times the error of the reference formula evaluated on the CPU in the handle's
dtype against the float64 reference, with a floor of 64 eps of the dtype.  In float64 that evaluation IS the reference, so the
bound is the floor, 1.4e-14; in float32 the CPU errors are F32_FLOOR of tests/test_weight_grad_cpu.py (0.8e-7 .. 2.9e-7), eight
times that is 0.6e-6 .. 2.3e-6, and the floor of 64 eps = 7.6e-6 is what binds on every case.  A missing term or a wrong factor
row is an error of order 1 (the second-order part is 50 - 80 % of max |gtheta| on every case, asserted on the CPU).
Measured on the device (MI355X), error / max |gtheta|, (with lam and v, first order):
    fp64  a 2.7e-16 2.6e-16   b 2.6e-16 2.8e-16   c 1.2e-15 6.2e-16   d 7.1e-16 3.2e-16   e = a
    fp32  a 1.1e-07 1.2e-07   b 2.2e-07 1.1e-07   c 6.2e-07 3.1e-07   d 4.0e-07 1.8e-07   e = a
End to end (fp64): plumbing 4.1e-16; directional derivative -6.49300365 against the central difference -6.49300366; the batch
with a failed problem equals the batch without it to the bit."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

if __name__ == "__main__":          # the chunked child process: no conftest there
    _here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(_here), _here]

from oracle import nempc_oracle as orc
import weight_grad_reference as wref

pytestmark = pytest.mark.gpu

DTYPES = {"fp64": torch.float64, "fp32": torch.float32}
EPS = {"fp64": 2.0 ** -52, "fp32": 2.0 ** -23}
FLOOR_EPS = 64.0          # floor of the tolerance, in eps of the dtype
MARGIN = 8.0              # device error allowed, in units of the CPU evaluation's error in the same dtype
_ENG = {}


def tolerance(name, dt, first_order):
    r = wref.reference(name)
    floor = 0.0 if dt == "fp64" else (r["e1_f32"] if first_order else r["e2_f32"])
    return max(MARGIN * floor, FLOOR_EPS * EPS[dt])


def engine(name, dt):
    """one handle per (case, dtype), extras bound, shared by the tests of this module"""
    from pyneuralempc_amd import CallbackEngine
    if (name, dt) not in _ENG:
        c = wref.CASES[name]
        net = c.net()
        eng = CallbackEngine(net.W, net.b, c.H, c.nx, c.nu, integrator=c.integ, DT=c.DT, dtype=DTYPES[dt], device="cuda:0",
                             max_batch=c.B, kernel=c.kernel, n_extra=c.ne, activations=net.act)
        if c.ne:
            eng.bind_extra(eng.to_device(c.inputs()["extra"]))
        _ENG[(name, dt)] = eng
    return _ENG[(name, dt)]


def device_inputs(eng, c, sel=None):
    d = c.inputs()
    pick = (lambda a: a) if sel is None else (lambda a: a[sel])
    return {k: eng.to_device(pick(d[k])) for k in ("Z", "X0", "lam", "v", "w")}


def both(eng, t, skip=None):
    g2 = eng.weight_grad(t["Z"], t["X0"], t["w"], lam=t["lam"], v=t["v"], skip=skip, flat=True)
    g1 = eng.weight_grad(t["Z"], t["X0"], t["w"], skip=skip, flat=True)
    return g2, g1


CASE_DT = [(n, dt) for n in sorted(wref.CASES) for dt in DTYPES]


@pytest.mark.parametrize("name,dt", CASE_DT)
def test_matches_the_reference_and_is_reproducible(name, dt):
    c, eng, ref = wref.CASES[name], engine(name, dt), wref.reference(name)
    if name == "d":
        assert eng.kernel_variant == "layered"
    if name == "e":
        assert eng.kernel_variant.startswith("mfma")
    t = device_inputs(eng, c)
    g2, g1 = both(eng, t)
    assert g2.shape == (eng.n_params,) == ref["g2"].shape
    for g, key, first in ((g2, "g2", False), (g1, "g1", True)):
        err = np.abs(g.double().cpu().numpy() - ref[key]).max() / np.abs(ref[key]).max()
        print(f"[weight_grad] case {name} {dt} {key}: error / max |gtheta| = {err:.2e} (bound {tolerance(name, dt, first):.2e})")
        assert err <= tolerance(name, dt, first)
    h2, h1 = both(eng, t)
    assert torch.equal(g2.view(torch.uint8), h2.view(torch.uint8)) and torch.equal(g1.view(torch.uint8), h1.view(torch.uint8))
    # the per-layer views are the flat tensor's
    parts = eng.weight_grad(t["Z"], t["X0"], t["w"], lam=t["lam"], v=t["v"])
    flat = torch.cat([torch.cat([dW.reshape(-1), db]) for dW, db in parts])
    assert [tuple(dW.shape) for dW, _ in parts] == [w.shape for w in c.net().W] and torch.equal(flat, g2)


@pytest.mark.parametrize("name,dt", CASE_DT)
def test_skipped_problems_with_nan_data_equal_the_batch_without_them(name, dt):
    c, eng = wref.CASES[name], engine(name, dt)
    drop = [1, c.B - 2]
    t = device_inputs(eng, c)
    skip = torch.zeros(c.B, dtype=torch.int32, device="cuda:0")
    for b in drop:
        skip[b] = 1
        for k in ("lam", "v", "w"):
            t[k][b] = float("nan")
    g2, g1 = both(eng, t, skip)
    assert bool(torch.isfinite(g2).all()) and bool(torch.isfinite(g1).all())
    sel = np.array([b for b in range(c.B) if b not in drop])
    try:
        if c.ne:
            eng.bind_extra(eng.to_device(c.inputs()["extra"][sel]))
        s2, s1 = both(eng, device_inputs(eng, c, sel))
    finally:
        if c.ne:
            eng.bind_extra(eng.to_device(c.inputs()["extra"]))
    assert torch.equal(g2.view(torch.uint8), s2.view(torch.uint8)) and torch.equal(g1.view(torch.uint8), s1.view(torch.uint8))
    # ... and differs from the full batch (the dropped problems matter)
    f2, _ = both(eng, device_inputs(eng, c))
    assert not torch.equal(f2, g2)


@pytest.mark.parametrize("name,dt", CASE_DT)
def test_refusals_leave_the_device_usable(name, dt):
    from pyneuralempc_amd import _lib
    c, eng = wref.CASES[name], engine(name, dt)
    t = device_inputs(eng, c)
    before, _ = both(eng, t)
    g = torch.empty(eng.n_params, dtype=DTYPES[dt], device="cuda:0")
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())

    def call(B, lam, v, w, h=None):
        return eng.lib.nempc_weight_grad(h or eng._handle, B, p(t["Z"]), p(t["X0"]), p(lam), p(v), p(w), None, p(g), None)

    def refused(rc, code, word):
        msg = eng.lib.nempc_last_error().decode()
        assert rc == code and "nempc_weight_grad" in msg and word in msg, (rc, msg)

    refused(call(c.B, None, t["v"], t["w"]), _lib.EINVAL, "both or neither")
    refused(call(c.B, t["lam"], None, t["w"]), _lib.EINVAL, "both or neither")
    refused(call(c.B + 1, t["lam"], t["v"], t["w"]), _lib.EINVAL, "max_batch")
    refused(call(c.B, t["lam"], t["v"], None), _lib.EINVAL, "null")
    if c.ne:
        try:
            eng.bind_extra(eng.to_device(c.inputs()["extra"][:c.B - 1]))
            refused(call(c.B, t["lam"], t["v"], t["w"]), _lib.EINVAL, "extras")
        finally:
            eng.bind_extra(eng.to_device(c.inputs()["extra"]))
    with pytest.raises(ValueError):
        eng.weight_grad(t["Z"], t["X0"], t["w"], lam=t["lam"])
    after, _ = both(eng, t)
    assert torch.equal(before, after)


def test_rolling_window_handles_are_refused():
    import solver_step_cases as sc
    from pyneuralempc_amd import _lib
    case = sc.qp_case("roll3_fwd", 10)
    eng = case.engine()
    X0 = case.bind(eng, 2)
    Z = eng.to_device(case.Zrand[:2])
    w = torch.zeros(2, case.H * case.nx, dtype=torch.float64, device="cuda:0")
    with pytest.raises(_lib.NempcError) as e:
        eng.weight_grad(Z, X0, w)
    assert e.value.code == -5 and "nempc_weight_grad" in str(e.value) and "rolling_window" in str(e.value)
    assert eng.n_params == sum((w.shape[0] + 1) * w.shape[1] for w in case.net.W)
    eng.eval(Z, X0, want=("g",))           # the handle still evaluates
    torch.cuda.synchronize()


def _child(out):
    res = {}
    for dt in DTYPES:
        eng = engine("c", dt)
        g2, g1 = both(eng, device_inputs(eng, wref.CASES["c"]))
        res[dt + "_g2"], res[dt + "_g1"] = g2.cpu().numpy(), g1.cpu().numpy()
    np.savez(out, **res)


def test_chunked_accumulation_equals_the_single_chunk_bit_for_bit(tmp_path):
    """case c with NEMPC_WGRAD_CHUNK_ROWS=96 in a fresh child process: 350 rows in chunks of 96, 96, 96 and 62 (the ragged
    last one), three K slices per chunk against eleven in one: the same slices added in the same order"""
    out = str(tmp_path / "chunked.npz")
    env = dict(os.environ, NEMPC_WGRAD_CHUNK_ROWS="96")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = np.load(out)
    for dt in DTYPES:
        eng = engine("c", dt)
        g2, g1 = both(eng, device_inputs(eng, wref.CASES["c"]))
        assert np.array_equal(got[dt + "_g2"].view(np.uint8), g2.cpu().numpy().view(np.uint8))
        assert np.array_equal(got[dt + "_g1"].view(np.uint8), g1.cpu().numpy().view(np.uint8))


# ---- end to end: autograd.solve(..., weights=...) on the device, fp64 ------------------------------------------------------
E2E_H, E2E_B = 6, 8
E2E_KW = dict(tol_constraint=1e-10, tol_step=1e-10, max_iter=200)


def _e2e():
    from pyneuralempc_amd import CallbackEngine
    c = wref.CASES["a"]
    net = c.net()
    eng = CallbackEngine(net.W, net.b, E2E_H, c.nx, c.nu, integrator=c.integ, dtype=torch.float64, device="cuda:0", max_batch=E2E_B)
    rng = np.random.default_rng(7)
    X0 = eng.to_device(rng.uniform(-0.5, 0.5, size=(E2E_B, c.nx)))
    C = eng.to_device(rng.normal(size=(E2E_B, E2E_H * (c.nx + c.nu))))
    D = [rng.normal(size=a.shape) for pair in zip(net.W, net.b) for a in pair]
    nrm = np.sqrt(sum(float((a * a).sum()) for a in D))
    return c, net, eng, X0, C, [a / nrm for a in D]


def _theta(net, eng, shift=None):
    flat = [a for pair in zip(net.W, net.b) for a in pair]
    if shift is not None:
        flat = [a + s for a, s in zip(flat, shift)]
    return [eng.to_device(a).requires_grad_(True) for a in flat]


def test_autograd_weight_gradients_end_to_end():
    """case a's network, unbounded, H = 6, B = 8, solver tolerances 1e-10, loss = (C * Z).sum().  (1) the weight gradients
    equal -reference at the returned Z, lam and kkt_solve's v, w (the plumbing), at the module's fp64 tolerance; (2) the
    directional derivative along a seeded unit direction equals the central difference of the loss over two more solves at
    theta +- 1e-5 D to a relative 1e-3 (h^2 truncation plus solver tolerance / h = 1e-5; a wrong sign or a missing term is off
    by order 1)."""
    from pyneuralempc_amd import autograd as nag
    c, net, eng, X0, C, D = _e2e()
    theta = _theta(net, eng)
    Z, st = nag.solve(eng, X0, weights=theta, **E2E_KW)
    assert (st == 0).all()
    (C * Z).sum().backward()
    got = np.concatenate([t.grad.cpu().numpy().ravel() for t in theta])
    Z2, _, _, duals = eng.solve(X0, return_duals=True, **E2E_KW)
    assert torch.equal(Z2, Z.detach())
    out = eng.kkt_solve(Z2, X0, duals["lam"], duals["zl"], duals["zu"], rz=C, want=("v", "w"))
    assert (out["status"] == 0).all()
    p = wref.TorchPhi(net, E2E_H, c.nx, c.nu, c.kind, c.DT)
    ref = -p.gtheta(Z2.cpu().numpy(), X0.cpu().numpy(), out["w"].cpu().numpy(), duals["lam"].cpu().numpy(), out["v"].cpu().numpy())
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"[weight_grad e2e] plumbing: error / max |gtheta| = {err:.2e}")
    assert err <= FLOOR_EPS * EPS["fp64"]
    # directional derivative
    h = 1e-5
    loss = []
    for sgn in (1.0, -1.0):
        with torch.no_grad():
            Zs, ss = nag.solve(eng, X0, weights=_theta(net, eng, [sgn * h * d for d in D]), **E2E_KW)
        assert (ss == 0).all()
        loss.append(float((C * Zs).sum()))
    fd = (loss[0] - loss[1]) / (2.0 * h)
    dd = float(sum((t.grad.cpu().numpy() * d).sum() for t, d in zip(theta, D)))
    print(f"[weight_grad e2e] directional derivative {dd:.8e}, central difference {fd:.8e}")
    assert abs(dd - fd) <= 1e-3 * abs(fd)


def test_autograd_skips_a_failed_problem_in_the_weight_gradient():
    """one problem forced to fail by a bind_bounds row with lo >= hi: finite weight gradients, equal to those of the batch
    without it (the module's fp64 tolerance)"""
    from pyneuralempc_amd import autograd as nag
    c, net, eng, X0, C, _ = _e2e()
    bad = 3
    xlb = torch.full((E2E_B, E2E_H, c.nx), -float("inf"), dtype=torch.float64, device="cuda:0")
    xub = torch.full((E2E_B, E2E_H, c.nx), float("inf"), dtype=torch.float64, device="cuda:0")
    xlb[bad, 2, 0], xub[bad, 2, 0] = 1.0, 0.5
    eng.bind_bounds(xlb=xlb, xub=xub)
    theta = _theta(net, eng)
    Z, st = nag.solve(eng, X0, weights=theta, **E2E_KW)
    assert st.tolist() == [1 if b == bad else 0 for b in range(E2E_B)]
    (C * Z).sum().backward()
    got = np.concatenate([t.grad.cpu().numpy().ravel() for t in theta])
    assert np.isfinite(got).all() and np.abs(got).max() > 0.0
    eng.bind_bounds()
    sel = [b for b in range(E2E_B) if b != bad]
    theta2 = _theta(net, eng)
    Z2, st2 = nag.solve(eng, X0[sel].contiguous(), weights=theta2, **E2E_KW)
    assert (st2 == 0).all()
    (C[sel] * Z2).sum().backward()
    ref = np.concatenate([t.grad.cpu().numpy().ravel() for t in theta2])
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"[weight_grad e2e] failed problem skipped: difference / max |gtheta| = {err:.2e}")
    assert err <= FLOOR_EPS * EPS["fp64"]


if __name__ == "__main__":
    _child(sys.argv[1])
