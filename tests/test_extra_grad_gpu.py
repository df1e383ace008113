"""GPU: nempc_extra_grad / CallbackEngine.extra_grad against tests/extra_grad_reference.py on the cases of its table, against
the library's own Jacobian, and autograd.solve(..., extra=, Q=, R=) end to end.

Tolerance (normalised by max |gE|): the rule of tests/test_weight_grad_gpu.py -- 8 times the error of the reference formula
evaluated on the CPU in the handle's dtype against the float64 reference, with a floor of 64 eps of the dtype.  In float64 that
evaluation IS the reference, so the bound is the floor, 1.4e-14; in float32 the CPU errors are F32_FLOOR of
tests/test_extra_grad_cpu.py (0.4e-7 .. 2.7e-7), eight times that is at most 2.2e-6, and the floor of 64 eps = 7.6e-6 is what
binds on every case.  A missing second-order term is an error of 0.28 .. 0.72 of max |gE| (asserted on the CPU).
Measured on the device (MI355X), error / max |gE|, (with lam and v, first order):
    fp64  a 1.9e-16 1.9e-16   b 2.6e-16 4.4e-16   c 2.1e-16 2.6e-16   d 3.2e-16 5.5e-16
          e 3.4e-16 1.7e-16   f 3.3e-16 4.7e-16   g 6.2e-16 7.0e-16      (e, f, g: WS_CASES, the workspace forms)
    fp32  a 0.8e-07 2.1e-07   b 2.1e-07 0.8e-07   c 1.8e-07 1.8e-07   d 2.3e-07 2.8e-07
          e 1.2e-07 1.0e-07   f 2.8e-07 2.7e-07   g 5.3e-07 4.8e-07
Against w' J of the twin engine (fp64, first order): a 4.8e-16 (bound 1.3e-11), c 3.9e-16 (bound 4.9e-10).
End to end (fp64): plumbing 3.8e-16; directional derivative against the central difference: extra 2.12143040e-01 /
2.12143040e-01, Q -1.58254116e-01 / -1.58254111e-01, R -7.09104002e+00 / -7.09104008e+00; with a failed problem Qbar and the
other problems' extrabar have the bits of the batch without it."""
import ctypes

import numpy as np
import pytest
import torch

import extra_grad_reference as eref
from test_weight_grad_gpu import DTYPES, EPS, FLOOR_EPS, MARGIN

pytestmark = pytest.mark.gpu

_ENG = {}


def tolerance(name, dt, first_order):
    """tests/test_weight_grad_gpu.py::tolerance with this module's reference"""
    r = eref.reference(name)
    floor = 0.0 if dt == "fp64" else (r["e1_f32"] if first_order else r["e2_f32"])
    return max(MARGIN * floor, FLOOR_EPS * EPS[dt])


def engine(name, dt):
    """one handle per (case, dtype), extras bound, shared by the tests of this module"""
    from pyneuralempc_amd import CallbackEngine
    if (name, dt) not in _ENG:
        c = eref.ALL_CASES[name]
        net = c.net()
        eng = CallbackEngine(net.W, net.b, c.H, c.nx, c.nu, integrator=c.integ, DT=c.DT, dtype=DTYPES[dt], device="cuda:0",
                             max_batch=c.B, kernel=c.kernel, n_extra=c.ne, activations=net.act)
        eng.bind_extra(eng.to_device(c.inputs()["extra"]))
        _ENG[(name, dt)] = eng
    return _ENG[(name, dt)]


def device_inputs(eng, c, sel=None):
    d = c.inputs()
    pick = (lambda a: a) if sel is None else (lambda a: a[sel])
    return {k: eng.to_device(pick(d[k])) for k in ("Z", "X0", "lam", "v", "w")}


def both(eng, t):
    return eng.extra_grad(t["Z"], t["X0"], t["w"], lam=t["lam"], v=t["v"]), eng.extra_grad(t["Z"], t["X0"], t["w"])


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


CASE_DT = [(n, dt) for n in sorted(eref.CASES) for dt in DTYPES]
ALL_CASE_DT = [(n, dt) for n in sorted(eref.ALL_CASES) for dt in DTYPES]
LANES = {"a": "1 lane", "b": "16 lanes", "c": "16 lanes", "d": "64 lanes", "e": "1 lane", "f": "16 lanes", "g": "64 lanes"}


def form(name, dt):
    """the launch form csrc/egrad_plan.h picks: lanes from the widest layer; the workspace for the WS_CASES in float64"""
    return f"egrad_rows_kernel<{LANES[name]}, {'workspace' if name in eref.WS_CASES and dt == 'fp64' else 'lds'}>"


@pytest.mark.parametrize("name,dt", ALL_CASE_DT)
def test_matches_the_reference_and_is_reproducible(name, dt):
    c, eng, ref = eref.ALL_CASES[name], engine(name, dt), eref.reference(name)
    if name == "d":
        assert eng.kernel_variant == "layered"
    t = device_inputs(eng, c)
    g2, g1 = both(eng, t)
    assert eng.last_extra_grad_kernel == form(name, dt)
    assert tuple(g2.shape) == (c.B, c.H, c.ne) == ref["g2"].shape and g2.dtype == DTYPES[dt]
    for g, key, first in ((g2, "g2", False), (g1, "g1", True)):
        err = np.abs(g.double().cpu().numpy() - ref[key]).max() / np.abs(ref[key]).max()
        print(f"[extra_grad] case {name} {dt} {key}: error / max |gE| = {err:.2e} (bound {tolerance(name, dt, first):.2e})")
        assert err <= tolerance(name, dt, first)
    h2, h1 = both(eng, t)
    assert same_bits(g2, h2) and same_bits(g1, h1)


@pytest.mark.parametrize("name,dt", CASE_DT)
def test_problems_are_independent_to_the_bit(name, dt):
    c, eng = eref.CASES[name], engine(name, dt)
    t = device_inputs(eng, c)
    g2, g1 = both(eng, t)
    # the first three problems alone (the binding's first rows are theirs)
    s2, s1 = both(eng, device_inputs(eng, c, slice(0, 3)))
    assert same_bits(s2, g2[:3]) and same_bits(s1, g1[:3])
    # one problem full of NaN: its rows are NaN, every other row keeps its bits
    bad = c.B - 2
    for k in ("Z", "lam", "v", "w"):
        t[k][bad] = float("nan")
    n2, n1 = both(eng, t)
    keep = [b for b in range(c.B) if b != bad]
    assert same_bits(n2[keep], g2[keep]) and same_bits(n1[keep], g1[keep])
    assert bool(torch.isnan(n2[bad]).all()) and bool(torch.isnan(n1[bad]).all())


@pytest.mark.parametrize("name", ["a", "c"])
def test_first_order_call_equals_the_jacobian_of_a_twin_engine_contracted_with_w(name):
    """a second handle with the SAME weights, nu' = nu + ne and no extras reads the same network input [x | u, e]; the columns
    of its dense Jacobian at the e slots of u'_t = [u_t ; e_t], contracted with w on the host in float64, are gE of the
    first-order call.  Bound: this module's tolerance plus the project's fp64 Jacobian parity bound (1e-12, the golden tests)
    carried through the contraction, nx * 1e-12 * max |w| * max |J| / max |gE|.  No torch restatement takes part."""
    from pyneuralempc_amd import CallbackEngine
    c, eng = eref.CASES[name], engine(name, "fp64")
    d, net = c.inputs(), c.net()
    nu2 = c.nu + c.ne
    twin = CallbackEngine(net.W, net.b, c.H, c.nx, nu2, integrator=c.integ, DT=c.DT, dtype=torch.float64, device="cuda:0",
                          max_batch=c.B, activations=net.act)
    U = np.concatenate([d["Z"][:, c.H * c.nx:].reshape(c.B, c.H, c.nu), d["extra"]], axis=2)
    Z2 = np.concatenate([d["Z"][:, :c.H * c.nx], U.reshape(c.B, -1)], axis=1)
    J = twin.eval(twin.to_device(Z2), twin.to_device(d["X0"]), want=("jac_dense",))["jac_dense"].cpu().numpy()
    J = J[:, :c.H * c.nx].reshape(c.B, c.H, c.nx, -1)
    w = d["w"].reshape(c.B, c.H, c.nx)
    want = np.zeros((c.B, c.H, c.ne))
    for t in range(c.H):
        cols = c.H * c.nx + t * nu2 + c.nu + np.arange(c.ne)
        want[:, t] = np.einsum("bi,bij->bj", w[:, t], J[:, t][:, :, cols])
    dev = device_inputs(eng, c)
    got = eng.extra_grad(dev["Z"], dev["X0"], dev["w"]).cpu().numpy()
    scale = np.abs(want).max()
    bound = tolerance(name, "fp64", True) + c.nx * 1e-12 * np.abs(w).max() * np.abs(J).max() / scale
    err = np.abs(got - want).max() / scale
    print(f"[extra_grad] case {name} fp64 against w' J of the twin engine: {err:.2e} (bound {bound:.2e})")
    assert err <= bound


@pytest.mark.parametrize("name,dt", [("b", "fp64"), ("c", "fp32")])
def test_refusals_leave_the_device_usable(name, dt):
    from pyneuralempc_amd import CallbackEngine, _lib
    import solver_step_cases as sc
    c, eng = eref.CASES[name], engine(name, dt)
    t = device_inputs(eng, c)
    before2, before1 = both(eng, t)
    g = torch.empty((c.B, c.H, c.ne), dtype=DTYPES[dt], device="cuda:0")
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())

    def call(B, lam, v, w, out, h=None):
        return eng.lib.nempc_extra_grad(h or eng._handle, B, p(t["Z"]), p(t["X0"]), p(lam), p(v), p(w), p(out), None)

    def refused(rc, code, word):
        msg = eng.lib.nempc_last_error().decode()
        assert rc == code and "nempc_extra_grad" in msg and word in msg, (rc, msg)
        a2, a1 = both(eng, t)               # ... and a valid call gives the bits it gave before
        assert same_bits(a2, before2) and same_bits(a1, before1)

    net = c.net()
    plain = CallbackEngine([w[:c.nx + c.nu] for w in net.W[:1]] + net.W[1:], net.b, c.H, c.nx, c.nu, integrator=c.integ, DT=c.DT,
                           dtype=DTYPES[dt], device="cuda:0", max_batch=c.B, activations=net.act)
    refused(call(c.B, t["lam"], t["v"], t["w"], g, plain._handle), _lib.EINVAL, "n_extra = 0")
    with pytest.raises(_lib.NempcError):
        plain.extra_grad(t["Z"], t["X0"], t["w"])
    roll = sc.qp_case("roll3_fwd", 10)
    reng = roll.engine()
    rX0 = roll.bind(reng, 2)
    rZ = reng.to_device(roll.Zrand[:2])
    rw = torch.zeros(2, roll.H * roll.nx, dtype=torch.float64, device="cuda:0")
    rg = torch.empty(2, roll.H, 1, dtype=torch.float64, device="cuda:0")
    refused(eng.lib.nempc_extra_grad(reng._handle, 2, p(rZ), p(rX0), None, None, p(rw), p(rg), None), -5, "rolling_window")
    try:
        eng.bind_extra(eng.to_device(c.inputs()["extra"][:c.B - 1]))
        rc = call(c.B, t["lam"], t["v"], t["w"], g)
        msg = eng.lib.nempc_last_error().decode()
        assert rc == _lib.EINVAL and "nempc_extra_grad" in msg and "extras" in msg
        with pytest.raises(ValueError):
            eng.extra_grad(t["Z"], t["X0"], t["w"])
    finally:
        eng.bind_extra(eng.to_device(c.inputs()["extra"]))
    a2, a1 = both(eng, t)                  # (the binding is back: the call is valid again)
    assert same_bits(a2, before2) and same_bits(a1, before1)
    refused(call(c.B, t["lam"], None, t["w"], g), _lib.EINVAL, "both or neither")
    refused(call(c.B, None, t["v"], t["w"], g), _lib.EINVAL, "both or neither")
    refused(call(c.B, t["lam"], t["v"], None, g), _lib.EINVAL, "null")
    refused(call(c.B, t["lam"], t["v"], t["w"], None), _lib.EINVAL, "gE is null")
    refused(call(c.B + 1, t["lam"], t["v"], t["w"], g), _lib.EINVAL, "max_batch")
    with pytest.raises(ValueError):
        eng.extra_grad(t["Z"], t["X0"], t["w"], lam=t["lam"])
    reng.eval(rZ, rX0, want=("g",))           # the refused handles still evaluate
    torch.cuda.synchronize()


# ---- end to end: autograd.solve(..., extra=, Q=, R=) on the device, fp64 -------------------------------------------------------
E2E_H, E2E_B = 6, 8
E2E_KW = dict(tol_constraint=1e-10, tol_step=1e-10, max_iter=200)     # (as _e2e() of tests/test_weight_grad_gpu.py)


def _e2e():
    from pyneuralempc_amd import CallbackEngine
    c = eref.CASES["a"]
    net = c.net()
    eng = CallbackEngine(net.W, net.b, E2E_H, c.nx, c.nu, integrator=c.integ, dtype=torch.float64, device="cuda:0", max_batch=E2E_B,
                         n_extra=c.ne, activations=net.act)
    rng = np.random.default_rng(7)
    X0 = eng.to_device(rng.uniform(-0.5, 0.5, size=(E2E_B, c.nx)))
    C = eng.to_device(rng.normal(size=(E2E_B, E2E_H * (c.nx + c.nu))))
    extra = eng.to_device(0.5 * rng.normal(size=(E2E_B, E2E_H, c.ne)))
    Q = eng.to_device(np.eye(c.nx) + 0.1 * rng.normal(size=(c.nx, c.nx)))
    R = eng.to_device(0.3 * np.eye(c.nu) + 0.03 * rng.normal(size=(c.nu, c.nu)))
    xref = eng.to_device(0.1 * rng.normal(size=(E2E_B, E2E_H, c.nx)))
    return c, net, eng, X0, C, extra, Q, R, xref, rng


def test_autograd_extras_and_cost_weights_end_to_end():
    """case a's network with one extra, unbounded, H = 6, B = 8, solver tolerances 1e-10, per-problem xref, loss = (C * Z).sum().
    (1) extrabar equals -reference at the returned Z, lam and kkt_solve's v, w (the plumbing) at the module's fp64 tolerance;
    (2) for extra, then Q, then R: the directional derivative along a seeded unit direction equals the central difference of
    the loss over two more solves at +- 1e-5 to a relative 1e-3 -- the first-order bar of
    test_autograd_weight_gradients_end_to_end (h^2 truncation plus solver tolerance / h; a wrong sign or a missing term is off
    by order 1)."""
    from pyneuralempc_amd import autograd as nag
    c, net, eng, X0, C, extra, Q, R, xref, rng = _e2e()
    leaf = dict(extra=extra.clone().requires_grad_(True), Q=Q.clone().requires_grad_(True), R=R.clone().requires_grad_(True))
    Z, st = nag.solve(eng, X0, xref=xref, **leaf, **E2E_KW)
    assert (st == 0).all()
    (C * Z).sum().backward()
    Z2, _, _, duals = eng.solve(X0, return_duals=True, **E2E_KW)
    assert torch.equal(Z2, Z.detach())
    out = eng.kkt_solve(Z2, X0, duals["lam"], duals["zl"], duals["zu"], rz=C, want=("v", "w"))
    assert (out["status"] == 0).all()
    p = eref.TorchPhi(net, E2E_H, c.nx, c.nu, c.kind, c.DT)
    d = {k: a.cpu().numpy() for k, a in (("Z", Z2), ("X0", X0), ("w", out["w"]), ("lam", duals["lam"]), ("v", out["v"]), ("extra", extra))}
    ref = -eref.gE(p, d)
    err = np.abs(leaf["extra"].grad.cpu().numpy() - ref).max() / np.abs(ref).max()
    print(f"[extra_grad e2e] plumbing: error / max |gE| = {err:.2e}")
    assert err <= FLOOR_EPS * EPS["fp64"]
    h = 1e-5
    for key in ("extra", "Q", "R"):
        D = rng.normal(size=tuple(leaf[key].shape))
        D = eng.to_device(D / np.sqrt((D * D).sum()))
        loss = []
        for sgn in (1.0, -1.0):
            kw = {k: v.detach() for k, v in leaf.items()}
            kw[key] = kw[key] + sgn * h * D
            with torch.no_grad():
                Zs, ss = nag.solve(eng, X0, xref=xref, **kw, **E2E_KW)
            assert (ss == 0).all()
            loss.append(float((C * Zs).sum()))
        fd = (loss[0] - loss[1]) / (2.0 * h)
        dd = float((leaf[key].grad * D).sum())
        print(f"[extra_grad e2e] {key}: directional derivative {dd:.8e}, central difference {fd:.8e}")
        assert abs(dd - fd) <= 1e-3 * abs(fd)


def test_autograd_shared_p_receives_the_sum_over_problems_and_steps():
    from pyneuralempc_amd import autograd as nag
    c, net, eng, X0, C, extra, Q, R, xref, _ = _e2e()
    pvec = torch.tensor([0.3], dtype=torch.float64, device="cuda:0", requires_grad=True)
    full = pvec.detach()[None, None, :].expand(E2E_B, E2E_H, -1).contiguous().requires_grad_(True)
    Z, st = nag.solve(eng, X0, extra=pvec[None, None, :].expand(E2E_B, E2E_H, -1), **E2E_KW)
    (C * Z).sum().backward()
    Zf, _ = nag.solve(eng, X0, extra=full, **E2E_KW)
    (C * Zf).sum().backward()
    assert (st == 0).all() and torch.equal(Z.detach(), Zf.detach())
    want = full.grad.sum((0, 1))
    assert float((pvec.grad - want).abs().max()) <= FLOOR_EPS * EPS["fp64"] * float(full.grad.abs().sum())
    assert float(pvec.grad.abs().max()) > 0.0


@pytest.mark.parametrize("on_fail", ["nan", "zero"])
def test_autograd_skips_a_failed_problem_in_Qbar_and_fills_its_extrabar(on_fail):
    """one problem forced to fail by a bind_bounds row with lo >= hi: Qbar has the bits of the batch without it, that problem's
    extrabar is the fill and every other problem's extrabar keeps its bits"""
    from pyneuralempc_amd import autograd as nag
    c, net, eng, X0, C, extra, Q, R, xref, _ = _e2e()
    bad = 3
    xlb = torch.full((E2E_B, E2E_H, c.nx), -float("inf"), dtype=torch.float64, device="cuda:0")
    xub = torch.full((E2E_B, E2E_H, c.nx), float("inf"), dtype=torch.float64, device="cuda:0")
    xlb[bad, 2, 0], xub[bad, 2, 0] = 1.0, 0.5
    eng.bind_bounds(xlb=xlb, xub=xub)
    e1, Q1 = extra.clone().requires_grad_(True), Q.clone().requires_grad_(True)
    Z, st = nag.solve(eng, X0, xref=xref, extra=e1, Q=Q1, on_fail=on_fail, **E2E_KW)
    assert st.tolist() == [1 if b == bad else 0 for b in range(E2E_B)]
    (C * Z).sum().backward()
    eng.bind_bounds()
    sel = [b for b in range(E2E_B) if b != bad]
    e2, Q2 = extra[sel].clone().requires_grad_(True), Q.clone().requires_grad_(True)
    Z2, st2 = nag.solve(eng, X0[sel].contiguous(), xref=xref[sel].contiguous(), extra=e2, Q=Q2, **E2E_KW)
    assert (st2 == 0).all()
    (C[sel] * Z2).sum().backward()
    assert bool(torch.isfinite(Q1.grad).all()) and float(Q1.grad.abs().max()) > 0.0
    assert same_bits(Q1.grad, Q2.grad)
    assert bool(torch.isnan(e1.grad[bad]).all()) if on_fail == "nan" else bool((e1.grad[bad] == 0).all())
    assert same_bits(e1.grad[sel], e2.grad)
