"""GPU: per-problem tracking references and linear costs (nempc_bind_tracking) in nempc_eval, nempc_rollout, nempc_solve
and the controller's batched calls.

References throughout: one oracle.nempc_oracle.Problem per problem, built with that problem's xref / uref / cx / cu.
Tolerances of f and grad: test_gpu_parity's (fp64 1e-12 abs + 1e-12 rel; fp32 1e-4 of max(1, |ref|inf)).
"""
import functools

import numpy as np
import pytest
import torch

from oracle import nempc_oracle as orc
import kkt_reference as kkt
import solver_step_cases as sc

pytestmark = pytest.mark.gpu

F64 = dict(rtol=1e-12, atol=1e-12)
NAMES = ("xref", "uref", "cx", "cu")
BATCHES = (1, 17, 37)        # ragged 16-row tiles
BMAX = 37
WANTS = (("f", "grad", "g", "jac_dense"), ("f", "grad", "g", "jac_sparse"), ("f",), ("grad",), ("f", "grad", "g", "jac_tiles"))

# name: (nx, nu, hidden, integrator, DT, H, kernel, window, row kernel of the dense contract)
SHAPES = {
    "2x1_fused":   (2, 1, [64, 64], "discret", 1.0, 20, "auto", 1),        # the compiled-shape fused launch
    "6x3_coop":    (6, 3, [32, 32], "rk4", 0.1, 5, "auto", 1),             # rows_coop_kernel
    "6x3_tile":    (6, 3, [32, 32], "rk4", 0.1, 5, "mfma_tile", 1),
    "6x3_layered": (6, 3, [32, 32], "rk4", 0.1, 5, "layered", 1),
    "3x2_valu":    (3, 2, [8], "unity", 1.0, 70, "valu", 1),               # more steps than lanes: the t += 64 trip
    "roll2":       (2, 1, [16], "discret", 1.0, 6, "auto", 2),             # rolling window: eval and rollout only
}
DTYPES = {"float64": torch.float64, "float32": torch.float32}
CASES = [(s, d) for s in SHAPES for d in DTYPES]


def _close(dtype, got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if dtype == "float64":
        np.testing.assert_allclose(got, ref, err_msg=what, **F64)
    else:
        err = np.abs(got - ref).max() / max(1.0, np.abs(ref).max())
        assert err < 1e-4, f"{what}: max rel err {err:.3e}"


class Setup:
    """One shape: network, shared objective (non-symmetric Q, R and a QT, non-zero xref / uref / cx / cu), BMAX inputs and
    per-problem tracking data drawn around nothing in particular (they differ between problems at REF_SCALE)."""

    def __init__(self, shape):
        nx, nu, hidden, integ, DT, H, kernel, w = SHAPES[shape]
        self.nx, self.nu, self.H, self.integ, self.DT, self.kernel, self.w = nx, nu, H, integ, DT, kernel, w
        self.net = orc.MLP.random(w * (nx + nu), hidden, nx, seed=11)
        self.net.W[-1] *= 0.3
        self.obj = sc.objective(nx, nu, H, 12)
        rng = np.random.default_rng(13)
        self.Z, self.X0 = orc.synthetic_inputs(BMAX, H, nx, nu, seed=14)
        self.hist_x = rng.uniform(-0.5, 0.5, size=(BMAX, w - 1, nx)) if w > 1 else None
        self.hist_u = rng.uniform(-0.5, 0.5, size=(BMAX, w - 1, nu)) if w > 1 else None
        dims = dict(xref=nx, uref=nu, cx=nx, cu=nu)
        self.per = {k: sc.REF_SCALE * rng.normal(size=(BMAX, H, dims[k])) for k in NAMES}

    def problem(self, b, bound):
        """Oracle problem of problem b: the arrays named in `bound` are its own, the others the shared table's."""
        ob = dict(self.obj)
        for k in bound:
            ob[k] = self.per[k][b]
        roll = {} if self.w == 1 else dict(window=self.w, forward_rolling=True, hist_x=self.hist_x[b], hist_u=self.hist_u[b])
        return orc.Problem(self.net, self.H, self.nx, self.nu, sc.KINDS[self.integ], self.DT, **ob, **roll)

    @functools.lru_cache(maxsize=None)
    def reference(self, bound):
        """(f (BMAX,), grad (BMAX, n)) of the oracle with the arrays in `bound` per problem: computed once per shape."""
        ps = [self.problem(b, bound) for b in range(BMAX)]
        return (np.array([p.objective(self.Z[b]) for b, p in enumerate(ps)]),
                np.stack([p.gradient(self.Z[b]) for b, p in enumerate(ps)]))


@functools.lru_cache(maxsize=None)
def _setup(shape):
    return Setup(shape)


@functools.lru_cache(maxsize=None)
def _engine(shape, dtype):
    from pyneuralempc_amd import CallbackEngine
    s = _setup(shape)
    eng = CallbackEngine(s.net.W, s.net.b, s.H, s.nx, s.nu, integrator=s.integ, DT=s.DT, dtype=DTYPES[dtype], device="cuda:0",
                         max_batch=BMAX, kernel=s.kernel, rolling_window=s.w, activations=s.net.act)
    eng.set_objective(**s.obj)
    if s.w > 1:
        eng.bind_history(eng.to_device(s.hist_x), eng.to_device(s.hist_u))
    return eng


def _inputs(eng, s, B):
    return eng.to_device(s.Z[:B]), eng.to_device(s.X0[:B])


def _eval(eng, Z, X0, want):
    return {k: v.clone() for k, v in eng.eval(Z, X0, want=want).items()}


def _shared_copies(eng, s, B):
    """B copies of the handle's own xref / uref / cx / cu, in the handle's dtype"""
    return {k: eng.to_device(np.broadcast_to(s.obj[k][None], (B,) + s.obj[k].shape)) for k in NAMES}


@pytest.mark.parametrize("shape,dtype", CASES)
def test_evaluation_against_one_oracle_problem_per_problem(shape, dtype):
    """Item 1.  All four arrays bound: f and grad of every `want` against the per-problem oracle; g and every Jacobian output
    equal the unbound call's bit for bit (the rows still come from the fused launches).  Then each array bound alone, the
    other three left to the (non-zero) shared table."""
    s, eng = _setup(shape), _engine(shape, dtype)
    try:
        for B in BATCHES:
            Z, X0 = _inputs(eng, s, B)
            eng.bind_tracking()
            plain = {w: _eval(eng, Z, X0, w) for w in WANTS}
            eng.bind_tracking(**{k: eng.to_device(s.per[k][:B]) for k in NAMES})
            f_ref, g_ref = s.reference(NAMES)
            for w in WANTS:
                res = _eval(eng, Z, X0, w)
                if "f" in w:
                    _close(dtype, res["f"].cpu(), f_ref[:B], f"{shape} B={B} {w} f")
                if "grad" in w:
                    _close(dtype, res["grad"].cpu(), g_ref[:B], f"{shape} B={B} {w} grad")
                for k in w:
                    if k not in ("f", "grad"):
                        assert torch.equal(res[k], plain[w][k]), f"{shape} B={B} {w}: {k} differs from the unbound call's"
            for name in NAMES:
                eng.bind_tracking(**{name: eng.to_device(s.per[name][:B])})
                f_ref1, g_ref1 = s.reference((name,))
                res = _eval(eng, Z, X0, WANTS[0])
                _close(dtype, res["f"].cpu(), f_ref1[:B], f"{shape} B={B} {name} alone: f")
                _close(dtype, res["grad"].cpu(), g_ref1[:B], f"{shape} B={B} {name} alone: grad")
                # ... and it is not the shared result: the binding was read
                assert not torch.equal(res["f"], plain[WANTS[0]]["f"])
    finally:
        eng.bind_tracking()


@pytest.mark.parametrize("shape,dtype", CASES)
def test_uniform_binding_equals_the_shared_objective_bit_for_bit(shape, dtype):
    """Item 2.  B copies of the handle's own data bound: f and grad of every `want`, and the f of rollout, carry the bits of
    the unbound call (same lane-to-step mapping, operation order and reduction tree)."""
    s, eng = _setup(shape), _engine(shape, dtype)
    try:
        for B in BATCHES:
            Z, X0 = _inputs(eng, s, B)
            eng.bind_tracking()
            plain = {w: _eval(eng, Z, X0, w) for w in WANTS}
            Zr, fr = eng.rollout(X0, U=Z[:, s.H * s.nx:].clone(), want_f=True)
            eng.bind_tracking(**_shared_copies(eng, s, B))
            for w in WANTS:
                res = _eval(eng, Z, X0, w)
                for k in w:
                    assert torch.equal(res[k], plain[w][k]), f"{shape} {dtype} B={B} {w}: {k}"
            Zr2, fr2 = eng.rollout(X0, U=Z[:, s.H * s.nx:].clone(), want_f=True)
            assert torch.equal(Zr, Zr2) and torch.equal(fr, fr2)
    finally:
        eng.bind_tracking()


@pytest.mark.parametrize("shape,dtype", CASES)
def test_leading_dimension_and_offset(shape, dtype):
    """Item 3.  A (B, H+3, d) tensor bound at offset 2 against the contiguous copy of its rows 2 .. H+1, bit for bit; and a
    (B, H, d) view whose problems lie H+3 rows apart."""
    s, eng = _setup(shape), _engine(shape, dtype)
    rng = np.random.default_rng(15)
    B, H = 17, s.H
    Z, X0 = _inputs(eng, s, B)
    long = {k: eng.to_device(sc.REF_SCALE * rng.normal(size=(B, H + 3, s.per[k].shape[2]))) for k in NAMES}
    try:
        eng.bind_tracking(**{k: v[:, 2:H + 2].contiguous() for k, v in long.items()})
        ref = _eval(eng, Z, X0, WANTS[0])
        eng.bind_tracking(**long, offset=2)
        got = _eval(eng, Z, X0, WANTS[0])
        assert torch.equal(got["f"], ref["f"]) and torch.equal(got["grad"], ref["grad"])
        eng.bind_tracking(**{k: v[:, :H].contiguous() for k, v in long.items()})
        ref0 = _eval(eng, Z, X0, WANTS[0])
        views = {k: v[:, :H] for k, v in long.items()}
        assert not views["xref"].is_contiguous() or B == 1
        eng.bind_tracking(**views)
        got0 = _eval(eng, Z, X0, WANTS[0])
        assert torch.equal(got0["f"], ref0["f"]) and torch.equal(got0["grad"], ref0["grad"])
        assert not torch.equal(ref0["f"], ref["f"])
        with pytest.raises(ValueError):
            eng.bind_tracking(**long, offset=4)          # rows 4 .. H+3 reach past the tensor
    finally:
        eng.bind_tracking()


def test_coverage_check_and_unbinding():
    """Item 4.  A binding that covers 8 problems refuses an evaluation (and a roll-out with f, and a solve) of 9 with
    NEMPC_EINVAL; unbinding restores the shared result bit for bit."""
    from pyneuralempc_amd._lib import NempcError
    s, eng = _setup("2x1_fused"), _engine("2x1_fused", "float64")
    Z, X0 = _inputs(eng, s, 9)
    eng.bind_tracking()
    plain = _eval(eng, Z, X0, WANTS[0])
    try:
        eng.bind_tracking(xref=eng.to_device(s.per["xref"][:8]))
        for call in (lambda: eng.eval(Z, X0), lambda: eng.eval(Z, X0, want=("f",)), lambda: eng.rollout(X0, want_f=True),
                     lambda: eng.solve(X0, max_iter=1)):
            with pytest.raises(NempcError) as ei:
                call()
            assert ei.value.code == -1 and "tracking" in str(ei.value)
        eng.eval(Z, X0, want=("g", "jac_dense"))           # nothing that reads the binding: no refusal
        eng.rollout(X0)
        got8 = _eval(eng, Z[:8].contiguous(), X0[:8].contiguous(), WANTS[0])
        assert not torch.equal(got8["f"], plain["f"][:8])
    finally:
        eng.bind_tracking()
    again = _eval(eng, Z, X0, WANTS[0])
    for k in WANTS[0]:
        assert torch.equal(again[k], plain[k])


def test_reserve_and_a_rebuilt_handle_keep_the_binding():
    """The binding survives a grown workspace (nempc_reserve) and a handle built anew (_create), like the other bindings."""
    from pyneuralempc_amd import CallbackEngine
    s = _setup("2x1_fused")
    eng = CallbackEngine(s.net.W, s.net.b, s.H, s.nx, s.nu, integrator=s.integ, DT=s.DT, dtype=torch.float64, device="cuda:0",
                         max_batch=4, activations=s.net.act)
    eng.set_objective(**s.obj)
    B = 9
    Z, X0 = _inputs(eng, s, B)
    eng.bind_tracking(**{k: eng.to_device(s.per[k][:B]) for k in NAMES})
    f_ref, g_ref = s.reference(NAMES)
    res = _eval(eng, Z, X0, WANTS[0])               # (B > max_batch: reserve)
    assert eng.max_batch == B
    _close("float64", res["f"].cpu(), f_ref[:B], "after reserve: f")
    _close("float64", res["grad"].cpu(), g_ref[:B], "after reserve: grad")
    eng._create(16)
    again = _eval(eng, Z, X0, WANTS[0])
    for k in WANTS[0]:
        assert torch.equal(again[k], res[k]), k


# ---- solver

QP_CASES = [(n, H) for n, H in sc.QP_CASES if sc.QP_ROWS[n][8] == 1]       # (rolling-window solves take no binding)


def _qp_refs(case, B):
    """Per-problem references and linear costs of a QP case, REF_SCALE-sized, rounded to the handle's precision."""
    rng = np.random.default_rng(21)
    dims = dict(xref=case.nx, uref=case.nu, cx=case.nx, cu=case.nu)
    return {k: sc._round(sc.REF_SCALE * rng.normal(size=(B, case.H, dims[k])), case.dtype) for k in NAMES}


@pytest.mark.parametrize("name,H", QP_CASES)
def test_one_newton_step_per_problem_references(name, H):
    """Item 5.  Linear networks, no bounds, max_iter = 1: Z[b] against kkt_reference.newton_step of problem b's own oracle
    Problem within solver_step_cases.step_tolerance (ten times what a Riccati sweep in the handle's precision loses on
    that system).  Every lq_kernel the row names; batches of 1, 3 and 16 (3 at H = 355, whose dense reference is the
    slow part).  The references differ between problems at REF_SCALE = 0.1: reading problem 0's for everybody misses the
    tolerance by orders of magnitude (asserted on the reference side: problem 1's step under problem 0's data is more than a
    hundred tolerances from its own)."""
    case = sc.qp_case(name, H)
    Bmax = 3 if H == sc.H_GLOBAL else case.B
    per = _qp_refs(case, Bmax)
    ref = []
    for b in range(Bmax):
        prob = orc.Problem(case.net, H, case.nx, case.nu, sc.KINDS[case.integ], case.DT,
                           extra=None if case.extra is None else case.extra[b], Q=case.obj["Q"], R=case.obj["R"],
                           QT=case.obj["QT"], **{k: per[k][b] for k in NAMES})
        z0, x0 = case.start(b), case.X0[b]
        dz, _, _, _ = kkt.newton_step(prob, z0, x0, np.zeros(H * case.nx), sc.REG, diagnostics=False)
        dzr, _ = kkt.riccati_step(prob, z0, x0, np.zeros(H * case.nx), sc.REG, sc.np_dtype(case))
        ref.append((z0 + dz, sc.step_tolerance(float(np.abs(dzr - dz).max()), z0 + dz)))
    eng = case.engine()
    bad, worst = [], 0.0
    try:
        for B in [b for b in (1, 3, 16) if b <= Bmax]:
            X0 = case.bind(eng, B)
            eng.bind_tracking(**{k: eng.to_device(per[k][:B]) for k in NAMES})
            for k in case.kernels:
                Z = eng.solve(X0, None, reg=sc.REG, max_iter=1, lq_kernel=k)[0].cpu().double().numpy()
                for b in range(B):
                    z1, tol = ref[b]
                    e = float(np.abs(Z[b] - z1).max())
                    worst = max(worst, e / tol)
                    if not e <= tol:
                        bad.append(f"{k} B={B} b={b}: |Z - (z0 + dz)| = {e:.3e} > {tol:.3e}")
        # the check is sharp: problem 1's step under problem 0's data is not within the tolerance of its own
        wrong = orc.Problem(case.net, H, case.nx, case.nu, sc.KINDS[case.integ], case.DT,
                            extra=None if case.extra is None else case.extra[1], Q=case.obj["Q"], R=case.obj["R"],
                            QT=case.obj["QT"], **{k: per[k][0] for k in NAMES})
        dzw, _, _, _ = kkt.newton_step(wrong, case.start(1), case.X0[1], np.zeros(H * case.nx), sc.REG, diagnostics=False)
        assert np.abs(case.start(1) + dzw - ref[1][0]).max() > 100.0 * ref[1][1]
    finally:
        eng.bind_tracking()
    print(f"[tracking qp {name} H={H}] variant {eng.kernel_variant}, rows {eng.last_row_kernel}; error / tolerance {worst:.3f}")
    assert not bad, "\n".join(bad)


@functools.lru_cache(maxsize=None)
def _nl_solver(B):
    """2/1 2 x 64 tanh Discret, H = 20, bounds on u (the setting of test_gpu_solver's compaction test), per-problem data."""
    from pyneuralempc_amd import CallbackEngine
    nx, nu, H = 2, 1, 20
    net = orc.MLP.random(nx + nu, [64, 64], nx, seed=3)
    net.W[-1] *= 0.2
    net.b[-1] *= 0.2
    eng = CallbackEngine(net.W, net.b, H, nx, nu, integrator="discret", dtype=torch.float64, device="cuda:0", max_batch=B)
    obj = dict(Q=np.eye(nx), R=0.1 * np.eye(nu), xref=np.zeros((H, nx)), uref=np.zeros((H, nu)), cx=np.zeros((H, nx)),
               cu=np.zeros((H, nu)))
    eng.set_objective(**obj)
    rng = np.random.default_rng(4)
    X0 = rng.uniform(-0.8, 0.8, size=(B, nx))
    lb = np.concatenate([np.full(H * nx, -3.0), np.full(H * nu, -0.5)])
    # a set-point per problem, held over the horizon, plus stage-wise noise; control reference and prices per problem
    per = dict(xref=rng.uniform(-0.4, 0.4, size=(B, 1, nx)) + 0.02 * rng.normal(size=(B, H, nx)),
               uref=0.05 * rng.normal(size=(B, H, nu)), cx=0.02 * rng.normal(size=(B, H, nx)), cu=0.05 * rng.normal(size=(B, H, nu)))
    return eng, obj, X0, lb, per


@pytest.mark.parametrize("linesearch", ["loop", "deferred"])
@pytest.mark.parametrize("B", [48, 160])
def test_solver_indexes_the_binding_by_the_callers_problem(B, linesearch):
    """Item 6.  compact=0 and compact=1 give identical status, per-problem iterations and Z; permuting the batch (X0, start
    and the bound tensors together) permutes the results -- all bit for bit.  B = 48 is the issue's size; run() compacts
    only above 64 active problems, so B = 160 is added: there the problems do change slots."""
    eng, _, X0h, lb, per = _nl_solver(B)
    X0 = eng.to_device(X0h)
    Zi = eng.rollout(X0)
    kw = dict(lb=lb, ub=-lb, max_iter=40, linesearch=linesearch, return_iterations=True)
    try:
        eng.bind_tracking(**{k: eng.to_device(v) for k, v in per.items()})
        Za, sa, ia, pa = eng.solve(X0, Zi, compact=False, **kw)
        Zb, sb, ib, pb = eng.solve(X0, Zi, compact=True, **kw)
        assert torch.equal(sa, sb) and torch.equal(pa, pb) and ia == ib and torch.equal(Za, Zb)
        ok = sa == 0
        print(f"[tracking solve B={B} {linesearch}] converged {int(ok.sum())}/{B}, convergence iterations "
              f"{int(pa[ok].min())}..{int(pa[ok].max())}, budget {ia}")
        # most, not all, converge early: compaction has something to do and some problems ride to the end of the budget
        assert int(ok.sum()) >= B // 2 and int(pa[ok].max()) > int(pa[ok].min())
        perm = torch.as_tensor(np.random.default_rng(5).permutation(B), device=X0.device)
        eng.bind_tracking(**{k: eng.to_device(v)[perm].contiguous() for k, v in per.items()})
        for compact in (False, True):
            Zp, sp, ip, pp = eng.solve(X0[perm].contiguous(), Zi[perm].contiguous(), compact=compact, **kw)
            assert torch.equal(sp, sa[perm]) and torch.equal(pp, pa[perm]) and torch.equal(Zp, Za[perm]), compact
    finally:
        eng.bind_tracking()


def test_solver_uniform_binding_against_the_shared_objective():
    """Item 7.  Bound copies of the shared data against the unbound solve: same status; on the problems converged in both,
    Z within 10 tol_step (1 + max|Z|) -- each run's last step is below tol_step (1 + max|z|), and the factor 10 is the margin
    for the two runs going through different launch forms (shared: objective fused into the row launch; bound: the
    binding's kernel).  On an MI355X the two runs turn out bit-identical (45 of 48 converged in both, max |Z - Z'| = 0: the
    binding's kernel returns the fused objective's bits, and the rows do not depend on the launch form), so that is what is
    asserted, for every problem, converged or not; the bound is kept as the weaker statement."""
    B, tol_step = 48, 1e-8
    eng, obj, X0h, lb, _ = _nl_solver(B)
    X0 = eng.to_device(X0h)
    kw = dict(lb=lb, ub=-lb, max_iter=60, tol_step=tol_step)
    eng.bind_tracking()
    Za, sa, _ = eng.solve(X0, **kw)
    try:
        eng.bind_tracking(**{k: eng.to_device(np.broadcast_to(obj[k][None], (B,) + obj[k].shape)) for k in NAMES})
        Zb, sb, _ = eng.solve(X0, **kw)
    finally:
        eng.bind_tracking()
    assert torch.equal(sa, sb)
    both = (sa == 0) & (sb == 0)
    assert int(both.sum()) >= B // 2
    za, zb = Za[both].cpu().numpy(), Zb[both].cpu().numpy()
    bound = 10.0 * tol_step * (1.0 + np.abs(za).max(axis=1))
    err = np.abs(za - zb).max(axis=1)
    print(f"[tracking solve, uniform binding] converged in both {int(both.sum())}/{B}, max |Z - Z'| = {err.max():.3e} "
          f"(bound {bound.min():.3e}), bit-identical: {bool(torch.equal(Za, Zb))}")
    assert (err <= bound).all()
    assert torch.equal(Za, Zb)


def test_solver_refuses_a_binding_on_a_rolling_window_model():
    """Item 8."""
    from pyneuralempc_amd._lib import NempcError
    s, eng = _setup("roll2"), _engine("roll2", "float64")
    X0 = eng.to_device(s.X0[:4])
    try:
        eng.bind_tracking(xref=eng.to_device(s.per["xref"][:4]))
        with pytest.raises(NempcError) as ei:
            eng.solve(X0, max_iter=2)
        assert ei.value.code == -5 and "rolling" in str(ei.value)
    finally:
        eng.bind_tracking()
    eng.solve(X0, max_iter=2)         # unbound, the rolling solve runs


# ---- controller

def _mpc(net, H, nx, nu, **obj_kw):
    import pyneuralempc_amd as nEMPC
    model = nEMPC.model.MLPModel(net.W, net.b, nx, nu, device="cuda:0")
    integ = nEMPC.integrator.DiscretIntegrator(model, H)
    obj = nEMPC.objective.QuadraticObjective(device="cuda:0", Q=np.eye(nx), R=0.05 * np.eye(nu), **obj_kw)
    dom = nEMPC.constraints.DomainConstraint(states_constraint=[[-5.0, 5.0]] * nx, control_constraint=[[-0.3, 0.3]] * nu)
    return nEMPC.controller.NMPC(integ, obj, [dom], H, 1.0, optimizer=nEMPC.optimizer.DeviceSqp()), integ, obj, dom


def _small_net():
    nx, nu, H = 2, 1, 12
    net = orc.MLP.random(nx + nu, [32, 32], nx, seed=2)
    net.W[-1] *= 0.2
    net.b[-1] *= 0.2
    return net, nx, nu, H


def test_next_batch_with_one_reference_per_problem():
    """Item 9.  next_batch(X0, xref=Xref) with 6 distinct references against, per problem, next_batch of that one problem on
    an NMPC whose QuadraticObjective holds its reference: equal status, Z within item 7's bound.  Afterwards mpc.next gives
    what it gave before the call (the binding is gone from the shared engine)."""
    net, nx, nu, H = _small_net()
    B, tol_step = 6, 1e-8
    rng = np.random.default_rng(6)
    X0 = rng.uniform(-0.6, 0.6, size=(B, nx))
    Xref = rng.uniform(-0.3, 0.3, size=(B, 1, nx)) + 0.02 * rng.normal(size=(B, H, nx))
    mpc, _, _, _ = _mpc(net, H, nx, nu)
    before = mpc.next(X0[0])
    assert before[0] is not None
    xs, us, st = mpc.next_batch(X0, xref=Xref, max_iter=80, tol_step=tol_step)
    after = mpc.next(X0[0])
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert int((st == 0).sum()) >= B - 1
    for b in range(B):
        one, _, _, _ = _mpc(net, H, nx, nu, xref=Xref[b])
        x1, u1, s1 = one.next_batch(X0[b:b + 1], max_iter=80, tol_step=tol_step)
        assert s1[0] == st[b]
        if st[b] == 0:
            z, z1 = np.concatenate([xs[b].ravel(), us[b].ravel()]), np.concatenate([x1[0].ravel(), u1[0].ravel()])
            assert np.abs(z - z1).max() <= 10.0 * tol_step * (1.0 + np.abs(z1).max()), b
    # an (H, d) value means "shared", through the binding: the objective's own reference gives the unbound result's status
    xs2, us2, st2 = mpc.next_batch(X0, xref=np.zeros((H, nx)), max_iter=80, tol_step=tol_step)
    xs3, us3, st3 = mpc.next_batch(X0, max_iter=80, tol_step=tol_step)
    assert np.array_equal(st2, st3)
    assert np.abs(xs2 - xs3).max() <= 10.0 * tol_step * (1.0 + np.abs(xs3).max())


def test_closed_loop_batch_follows_a_moving_reference_per_problem():
    """Item 9, closed loop: closed_loop_batch(X0, steps=3, xref=(B, 3+H-1, nx)) equals, bit for bit, the loop written out
    here from eng.solve, eng.rollout and eng.bind_tracking with contiguous per-step copies of the window."""
    from pyneuralempc_amd.optimizer.base import fused_evaluator
    net, nx, nu, H = _small_net()
    B, steps = 5, 3
    rng = np.random.default_rng(7)
    X0 = rng.uniform(-0.6, 0.6, size=(B, nx))
    L = steps + H - 1
    Xref = rng.uniform(-0.3, 0.3, size=(B, 1, nx)) + 0.05 * np.sin(0.4 * np.arange(L))[None, :, None] * rng.normal(size=(B, 1, nx))
    Cu = 0.02 * rng.normal(size=(B, L, nu))
    mpc, integ, obj, dom = _mpc(net, H, nx, nu)
    X, U, status = mpc.closed_loop_batch(X0, steps, xref=Xref, cu=Cu, max_iter=80)
    assert X.shape == (B, steps + 1, nx) and U.shape == (B, steps, nu) and status.shape == (steps, B)
    eng = fused_evaluator(integ, obj, None).engine
    lb, ub = np.asarray(dom.get_lower_bounds(H), dtype=np.float64), np.asarray(dom.get_upper_bounds(H), dtype=np.float64)
    xr, cu = eng.to_device(Xref), eng.to_device(Cu)
    Xk, Zi = eng.to_device(X0), None
    Xs, Us, Ss = [Xk], [], []
    try:
        for k in range(steps):
            eng.bind_tracking(xref=xr[:, k:k + H].contiguous(), cu=cu[:, k:k + H].contiguous())
            Z, s_k, _ = eng.solve(Xk, Zi, lb, ub, **(dict(max_iter=80) if k == 0 else dict(max_iter=80, mu_init=1e-4)))
            Uk = Z[:, H * nx:].reshape(B, H, nu).clone()
            Xk = eng.rollout(Xk, U=Uk)[:, :nx].clone().contiguous()
            Zi = eng.rollout(Xk, U=torch.cat([Uk[:, 1:], Uk[:, -1:]], dim=1))
            Xs.append(Xk), Us.append(Uk[:, 0]), Ss.append(s_k)
    finally:
        eng.bind_tracking()
    assert np.array_equal(X, torch.stack(Xs, dim=1).cpu().numpy())
    assert np.array_equal(U, torch.stack(Us, dim=1).cpu().numpy())
    assert np.array_equal(status, torch.stack(Ss, dim=0).cpu().numpy())
    # the reference moved the loops apart: not the shared objective's trajectories
    X_shared, _, _ = mpc.closed_loop_batch(X0, steps, max_iter=80)
    assert not np.array_equal(X, X_shared)
