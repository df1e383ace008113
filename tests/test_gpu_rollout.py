"""GPU: the on-device roll-out (nempc_rollout, csrc/kernels_rollout.hip) -- both kernels, every integrator, extras, rolling
windows, every activation family -- against the CPU oracle one step at a time and over the whole trajectory, its contract,
and the two places it is wired into: the solver's feasible start and the batched closed loop.

Inputs: weights, dims, integrator, extras from the committed goldens; X0, U (and the histories of the rolling cases, a
different one per problem) seeded uniform in +-0.5.  fp64 bound rtol = atol = 1e-12 (the project's, test_gpu_parity.F64),
fp32 rtol = atol = 3e-4 (test_gpu_parity's layered test), both per STEP: the oracle's Phi at the device's own x_{t-1}.
"""
import numpy as np
import pytest
import torch

from oracle import nempc_oracle as orc
from helpers import case_activations, case_extra, load_case, oracle_problem

pytestmark = pytest.mark.gpu

F64 = dict(rtol=1e-12, atol=1e-12)
F32 = dict(rtol=3e-4, atol=3e-4)
KIND_NAME = {0: "discret", 1: "unity", 2: "rk4"}
CASES = ["c1_discret", "c2_unity", "c2_rk4", "c3_rk4", "odd_dims", "h1", "tvp_p_discret", "tvp_p_rk4",
         "act_mixed_box", "act_linear_hidden", "act_selu_rk4", "act_mix3_c2", "deep4_mixed_c2",
         "act_swish_gelu_box", "act_zout_rk4",
         "wide256_c2", "deep5_mixed_rk4",
         "roll2_discret", "roll3_unity_rev", "roll3_discret_rev", "roll4_wide", "roll2_tvp_p", "roll4_short"]
# cases a kernel="mfma" handle takes (one activation or an output-based mix under a linear output layer, <= 3 hidden layers of
# width <= 128, 4 up to 64)
MFMA_HANDLE_CASES = {"c1_discret", "c2_unity", "c2_rk4", "c3_rk4", "odd_dims", "h1", "tvp_p_discret", "tvp_p_rk4",
                     "act_linear_hidden", "act_selu_rk4", "act_mix3_c2", "deep4_mixed_c2", "roll2_discret", "roll3_unity_rev",
                     "roll3_discret_rev", "roll4_wide", "roll2_tvp_p", "roll4_short"}
BMAX = 40
BATCHES = (1, 17, 40)          # one partial tile, two tiles with a partial one, three tiles with a partial one


def _mfma_fits(d, W):
    """the matrix-core roll-out's shape bounds (include/nempc.h)"""
    hidden = [w.shape[1] for w in W[:-1]]
    return int(d["nx"]) <= 16 and W[0].shape[0] <= 32 and len(hidden) <= 4 and all(h <= 128 for h in hidden)


_inputs = {}


def _case(name):
    """golden case + the seeded inputs of its BMAX problems (made once, shared, never changed)"""
    if name not in _inputs:
        d, W, b = load_case(name)
        H, nx, nu, w = int(d["H"]), int(d["nx"]), int(d["nu"]), int(d.get("window", 1))
        rng = np.random.default_rng(2024)
        X0 = rng.uniform(-0.5, 0.5, size=(BMAX, nx))
        U = rng.uniform(-0.5, 0.5, size=(BMAX, H, nu))
        if w > 1:
            d["hist_x"] = rng.uniform(-0.5, 0.5, size=(BMAX, w - 1, nx))
            d["hist_u"] = rng.uniform(-0.5, 0.5, size=(BMAX, w - 1, nu))
        for a in (X0, U):
            a.setflags(write=False)
        _inputs[name] = (d, W, b, X0, U)
    return _inputs[name]


def _engine(name, dtype, kernel="auto", B=BMAX):
    from pyneuralempc_amd import CallbackEngine
    d, W, b, _, _ = _case(name)
    ex = case_extra(d)
    w = int(d.get("window", 1))
    eng = CallbackEngine(W, b, int(d["H"]), int(d["nx"]), int(d["nu"]), integrator=KIND_NAME[int(d["kind"])],
                         DT=float(d["DT"]), dtype=dtype, device="cuda:0", max_batch=B, kernel=kernel,
                         n_extra=0 if ex is None else ex.shape[1], rolling_window=w,
                         forward_rolling=bool(int(d.get("forward_rolling", 1))), activations=case_activations(d))
    if ex is not None:
        eng.bind_extra(eng.to_device(np.broadcast_to(ex[None], (B,) + ex.shape).copy()))
    if w > 1:
        eng.bind_history(eng.to_device(d["hist_x"][:B]), eng.to_device(d["hist_u"][:B]))
    eng.set_objective(Q=d["Q"], R=d["R"], xref=d["xref"], uref=d["uref"], cu=d["cu"])
    return eng


def _per_step_check(name, Z, X0, tol, what):
    """|Phi_oracle(x_{t-1}^dev, u_t) - x_t^dev| within tol for every problem: the device's Z handed to Problem.tiles"""
    d, W, b, _, _ = _case(name)
    worst = 0.0
    for i in range(Z.shape[0]):
        x, phi, _, _ = oracle_problem(d, W, b, i).tiles(Z[i], X0[i])
        assert np.isfinite(x).all(), f"{what}: problem {i} not finite"
        worst = max(worst, float(np.abs(x - phi).max()))
        np.testing.assert_allclose(x, phi, err_msg=f"{what}: problem {i}", **tol)
    return worst


def _oracle_rollout(prob, x0, u):
    """NumPy roll-out through the oracle: row t of Problem.tiles depends on the states < t only, so H passes fill them in.
    -> states (H,nx), tiles dPhi (H,nx,tw) at the rolled-out point."""
    H, nx = prob.H, prob.nx
    z = np.concatenate([np.zeros(H * nx), np.asarray(u).ravel()])
    dphi = None
    for t in range(H):
        _, phi, dphi, _ = prob.tiles(z, x0)
        z[t * nx:(t + 1) * nx] = phi[t]
    _, phi, dphi, _ = prob.tiles(z, x0)
    assert np.array_equal(phi.ravel(), z[:H * nx])
    return z[:H * nx].reshape(H, nx), dphi


def _growth(prob, dphi):
    """G: the largest 2-norm of a product A_t ... A_{s+1} of consecutive state-transition blocks (first-order propagation of
    an error made at step s into step t).  Rolling windows: A_t is the transition of the window state [y_{t-w+1} .. y_t]
    (y = [x0 ; states]): the shift, and dPhi_t's state columns in the last block row; columns of history entries (data,
    never perturbed) stay zero."""
    H, nx, w = prob.H, prob.nx, prob.window
    back = w - 1
    A = []
    for t in range(H):
        M = np.zeros((w * nx, w * nx))
        M[:back * nx, nx:] = np.eye(back * nx)
        for j in range(w):                      # block j of the window state = y_{t-back+j}
            if t - back + j < 0:
                continue
            slot = j if prob.forward_rolling else back - j
            M[back * nx:, j * nx:(j + 1) * nx] = dphi[t][:, slot * nx:(slot + 1) * nx]
        A.append(M)
    G = 0.0
    for s in range(H):
        P = np.eye(w * nx)
        for t in range(s + 1, H):
            P = A[t] @ P
            G = max(G, float(np.linalg.norm(P, 2)))
    return G


@pytest.mark.parametrize("name", CASES)
def test_every_step_matches_the_oracle_at_the_device_states(name, monkeypatch):
    """Item 1: per-step parity, non-compounding, both forced kernels where the shape allows, B = 1 / 17 / 40, both dtypes;
    the two kernels agree with each other within the same bound; nempc_last_rollout_kernel reports what was forced."""
    from pyneuralempc_amd._lib import NempcError
    d, W, b, X0h, Uh = _case(name)
    H, nx = int(d["H"]), int(d["nx"])
    for dtype, tol in ((torch.float64, F64), (torch.float32, F32)):
        eng = _engine(name, dtype)
        X0, U = eng.to_device(X0h), eng.to_device(Uh)
        got = {}
        for which in (1, 2):
            monkeypatch.setenv("NEMPC_ROLLOUT_KERNEL", str(which))
            if which == 2 and not _mfma_fits(d, W):
                with pytest.raises(NempcError) as e:
                    eng.rollout(X0[:1].contiguous(), U[:1].contiguous())
                assert e.value.code == -5
                continue
            for B in BATCHES:
                Z = eng.rollout(X0[:B].contiguous(), U[:B].contiguous())
                assert eng.last_rollout_kernel == {1: "rollout_wave_kernel", 2: "rollout_mfma_kernel"}[which]
                Zh = Z.to("cpu", torch.float64).numpy()
                assert np.array_equal(Zh[:, H * nx:], U[:B].reshape(B, -1).to("cpu", torch.float64).numpy())
                worst = _per_step_check(name, Zh, X0[:B].to("cpu", torch.float64).numpy(), tol, f"{name} kernel {which} B={B} {dtype}")
                print(f"{name} {dtype} kernel {which} B={B}: max per-step |Phi_oracle - x| = {worst:.3e}, max|x| = {np.abs(Zh[:, :H * nx]).max():.3g}")
                if B == BMAX:
                    got[which] = Zh
                else:       # a problem's trajectory does not depend on the batch it sits in
                    assert which not in got or np.array_equal(Zh, got[which][:B])
        monkeypatch.delenv("NEMPC_ROLLOUT_KERNEL")
        if len(got) == 2:
            np.testing.assert_allclose(got[1][:, :H * nx], got[2][:, :H * nx], **tol)
        Z = eng.rollout(X0, U)              # by shape: whichever the library picks, it is one of the two above
        picked = {"rollout_wave_kernel": 1, "rollout_mfma_kernel": 2}[eng.last_rollout_kernel]
        assert picked in got and np.array_equal(Z.to("cpu", torch.float64).numpy(), got[picked])


@pytest.mark.parametrize("name", CASES)
def test_rolled_out_point_has_no_defect_under_the_row_kernels(name):
    """Item 2: the defects the existing row kernels see at the rolled-out point vanish within the per-step bound -- on handles
    of every kernel family that takes the network (the roll-out runs on each of them, too)."""
    from pyneuralempc_amd._lib import NempcError
    d, W, b, X0h, Uh = _case(name)
    H, nx, B = int(d["H"]), int(d["nx"]), 17
    ran = []
    for dtype, tol in ((torch.float64, F64), (torch.float32, F32)):
        for kernel in ("valu", "mfma", "layered"):
            try:
                eng = _engine(name, dtype, kernel, B)
            except NempcError as e:
                assert e.code == -5, e
                continue
            X0, U = eng.to_device(X0h[:B]), eng.to_device(Uh[:B])
            Z = eng.rollout(X0, U)
            g = eng.eval(Z, X0, want=("g",))["g"][:, :H * nx].to("cpu", torch.float64).numpy()
            x = Z[:, :H * nx].to("cpu", torch.float64).numpy()
            print(f"{name} {dtype} {kernel}: max |defect| = {np.abs(g).max():.3e}")
            np.testing.assert_allclose(x + g, x, err_msg=f"{name} {kernel} {dtype}", **tol)
            ran.append(kernel)
    # every case runs on a generic and a layered handle, these also on the register-resident matrix-core kernels
    assert ran.count("valu") == 2 and ran.count("layered") == 2, ran
    assert ran.count("mfma") == (2 if name in MFMA_HANDLE_CASES else 0), ran


@pytest.mark.parametrize("name", CASES)
def test_whole_trajectory_against_the_oracle_rollout(name):
    """Item 3 (fp64): the whole trajectory against a NumPy roll-out through the oracle, within
        1e-12 (1 + max|x|) (1 + H G),
    G the largest 2-norm of a product of consecutive state-transition blocks at the oracle's trajectory (window-augmented for
    the rolling cases): an error of 1e-12 (1 + |x|) made at one step reaches a later step multiplied by at most G to first
    order, and H steps make one each.  Measured on the 17 seeded problems (oracle only):

    case                     H           G      max|x|
    c1_discret              10       68.88       10.51
    c2_unity                20      0.8109      0.7377
    c2_rk4                  20        1.47        1.19
    c3_rk4                  30       11.06       2.897
    odd_dims                 7       1.216       0.534
    h1                       1           0       1.065
    tvp_p_discret            6        3.26       3.737
    tvp_p_rk4                6       1.388       1.094
    act_mixed_box            9       1.684       6.528
    act_linear_hidden        5      0.6073      0.5761
    act_selu_rk4             7       1.425        1.08
    act_mix3_c2              6        1.71       1.486
    deep4_mixed_c2           6       1.186       1.075
    act_swish_gelu_box       9       18.59       4.473
    act_zout_rk4             6        1.39       0.593
    wide256_c2               6       3.694       2.971
    deep5_mixed_rk4          5       1.128       1.191
    roll2_discret            8       20.18       7.524
    roll3_unity_rev          7         1.3       1.059
    roll3_discret_rev        6       12.28       4.371
    roll4_wide               6        6.61         2.9
    roll2_tvp_p              6       4.618       4.231
    roll4_short              2       1.774       1.654
    """
    d, W, b, X0h, Uh = _case(name)
    H, nx, B = int(d["H"]), int(d["nx"]), 17
    eng = _engine(name, torch.float64, B=B)
    Z = eng.rollout(eng.to_device(X0h[:B]), eng.to_device(Uh[:B])).cpu().numpy()
    Gmax = xmax = errmax = 0.0
    for i in range(B):
        prob = oracle_problem(d, W, b, i)
        xs, dphi = _oracle_rollout(prob, X0h[i], Uh[i])
        G = _growth(prob, dphi)
        tol = 1e-12 * (1.0 + np.abs(xs).max()) * (1.0 + H * G)
        err = float(np.abs(Z[i, :H * nx].reshape(H, nx) - xs).max())
        Gmax, xmax, errmax = max(Gmax, G), max(xmax, float(np.abs(xs).max())), max(errmax, err)
        assert err <= tol, f"{name} problem {i}: |x_dev - x_oracle| = {err:.3e} > {tol:.3e} (G = {G:.3g})"
    print(f"{name}: G = {Gmax:.4g}, max|x| = {xmax:.4g}, max trajectory error = {errmax:.3e}")


@pytest.mark.parametrize("name", ["c2_rk4", "tvp_p_discret", "roll3_unity_rev", "act_zout_rk4"])
def test_contract_states_never_read_controls_never_written(name, monkeypatch):
    """Item 4: controls bit-identical after the call; a NaN state part gives the finite result of the zero-filled call;
    two calls agree bit for bit; want_f is eval's f at the returned point exactly -- on either kernel."""
    d, W, b, X0h, Uh = _case(name)
    H, nx, nu, B = int(d["H"]), int(d["nx"]), int(d["nu"]), 17
    eng = _engine(name, torch.float64, B=B)
    X0, U = eng.to_device(X0h[:B]), eng.to_device(Uh[:B])
    for which in (1, 2):
        monkeypatch.setenv("NEMPC_ROLLOUT_KERNEL", str(which))
        Zz = torch.cat([torch.zeros(B, H * nx, dtype=torch.float64, device="cuda:0"), U.reshape(B, -1)], dim=1).contiguous()
        Zn = Zz.clone()
        Zn[:, :H * nx] = float("nan")
        out = eng.rollout(X0, Z=Zz)
        assert out is Zz                                                    # updated in place
        eng.rollout(X0, Z=Zn)
        assert torch.isfinite(Zn).all() and torch.equal(Zn, Zz)
        assert torch.equal(Zz[:, H * nx:], U.reshape(B, -1))
        Z2, f = eng.rollout(X0, U=U.reshape(B, H * nu), want_f=True)         # the flat form of U; a second call
        assert torch.equal(Z2, Zz)
        assert torch.equal(f, eng.eval(Z2, X0, want=("f",))["f"])
        Z0 = eng.rollout(X0)                                                # no U, no Z: zero controls
        assert torch.equal(Z0, eng.rollout(X0, U=torch.zeros_like(U)))
    with pytest.raises(ValueError):
        eng.rollout(X0, U=U, Z=Zz)


@pytest.mark.parametrize("name", ["c2_rk4", "roll3_discret_rev"])
def test_several_tiles_per_workgroup_give_the_same_trajectories(name, monkeypatch):
    """More tiles than compute units: up to four waves share a workgroup's staged weights.  On a handle told the device has ONE
    compute unit (NEMPC_NUM_CUS) B = 17 / 40 / 100 run 2 / 3 / 4 waves per workgroup (the last with a second, partly filled
    workgroup): bit for bit the trajectories of the one-tile-per-workgroup launch."""
    d, W, b, X0h, Uh = _case(name)
    reps = -(-100 // BMAX)
    X0h, Uh = np.tile(X0h, (reps, 1))[:100], np.tile(Uh, (reps, 1, 1))[:100]
    if int(d.get("window", 1)) > 1:
        d = dict(d, hist_x=np.tile(d["hist_x"], (reps, 1, 1))[:100], hist_u=np.tile(d["hist_u"], (reps, 1, 1))[:100])
    monkeypatch.setenv("NEMPC_ROLLOUT_KERNEL", "2")
    outs = []
    for cus in (None, "1"):
        if cus:
            monkeypatch.setenv("NEMPC_NUM_CUS", cus)
        eng = _engine(name, torch.float64, B=100)
        if int(d.get("window", 1)) > 1:
            eng.bind_history(eng.to_device(d["hist_x"]), eng.to_device(d["hist_u"]))
        X0, U = eng.to_device(X0h), eng.to_device(Uh)
        outs.append([eng.rollout(X0[:B].contiguous(), U[:B].contiguous()) for B in (17, 40, 100)])
        assert eng.last_rollout_kernel == "rollout_mfma_kernel"
    for a, c in zip(*outs):
        assert torch.isfinite(a).all() and torch.equal(a, c)
    # by shape (that last handle: one compute unit): the matrix-core kernel from 2.5 tiles per compute unit on for hidden
    # widths <= 64, the generic kernel below that
    monkeypatch.delenv("NEMPC_ROLLOUT_KERNEL")
    narrow = all(w.shape[1] <= 64 for w in W[:-1])
    eng.rollout(X0[:40].contiguous(), U[:40].contiguous())
    assert eng.last_rollout_kernel == ("rollout_mfma_kernel" if narrow else "rollout_wave_kernel")
    eng.rollout(X0[:17].contiguous(), U[:17].contiguous())
    assert eng.last_rollout_kernel == "rollout_wave_kernel"


def test_error_paths_return_codes():
    """Item 4: B beyond the bound history / extras, a rolling model without history, and the matrix-core kernel forced on a
    256-wide network are codes (exceptions on the Python side), not faults."""
    import ctypes
    import os
    from pyneuralempc_amd import CallbackEngine
    from pyneuralempc_amd._lib import NempcError
    d, W, b, X0h, Uh = _case("roll2_tvp_p")
    H, nx, nu, w = int(d["H"]), int(d["nx"]), int(d["nu"]), int(d["window"])
    ex = case_extra(d)
    eng = CallbackEngine(W, b, H, nx, nu, integrator="discret", dtype=torch.float64, device="cuda:0", max_batch=8,
                         n_extra=ex.shape[1], rolling_window=w, forward_rolling=True)
    X0 = eng.to_device(X0h[:8])
    Z = torch.zeros(8, eng.n, dtype=torch.float64, device="cuda:0")

    def call(B):
        return eng.lib.nempc_rollout(eng._handle, B, ctypes.c_void_p(X0.data_ptr()), ctypes.c_void_p(Z.data_ptr()), None, None)
    assert call(4) == -4 and b"nempc_bind_extra" in eng.lib.nempc_last_error()          # NEMPC_ESTATE
    eng.bind_extra(eng.to_device(np.broadcast_to(ex[None], (8,) + ex.shape).copy()))
    assert call(4) == -4 and b"nempc_bind_history" in eng.lib.nempc_last_error()
    eng.bind_history(eng.to_device(d["hist_x"][:6]), eng.to_device(d["hist_u"][:6]))
    assert call(6) == 0
    # f on a handle whose objective was never set: nempc_create gives every handle the default objective (Q = I, R = 0.1 I),
    # so there is no handle without one through the C ABI and NEMPC_ESTATE cannot be provoked; the call succeeds and f is
    # that default objective at the rolled-out point
    f = torch.full((8,), float("nan"), dtype=torch.float64, device="cuda:0")
    assert eng.lib.nempc_rollout(eng._handle, 6, ctypes.c_void_p(X0.data_ptr()), ctypes.c_void_p(Z.data_ptr()),
                                 ctypes.c_void_p(f.data_ptr()), None) == 0
    torch.cuda.synchronize()
    zh = Z[:6].cpu().numpy()
    np.testing.assert_allclose(f[:6].cpu().numpy(), (zh[:, :H * nx] ** 2).sum(axis=1) + 0.1 * (zh[:, H * nx:] ** 2).sum(axis=1), **F64)
    assert torch.isnan(f[6:]).all()
    assert call(7) == -1 and b"history" in eng.lib.nempc_last_error()                    # beyond the bound history
    assert call(9) == -1                                                                 # beyond max_batch
    assert call(0) == 0
    with pytest.raises(ValueError):
        eng.rollout(X0)                                                                  # the Python check, same condition
    eng.bind_extra(eng.to_device(np.broadcast_to(ex[None], (4,) + ex.shape).copy()))
    assert call(4) == 0 and call(5) == -1                                                # beyond the bound extras
    torch.cuda.synchronize()
    wide = _engine("wide256_c2", torch.float64, B=4)
    Xw = wide.to_device(_case("wide256_c2")[3][:4])
    os.environ["NEMPC_ROLLOUT_KERNEL"] = "2"
    try:
        with pytest.raises(NempcError) as e:
            wide.rollout(Xw)
        assert e.value.code == -5
    finally:
        del os.environ["NEMPC_ROLLOUT_KERNEL"]
    wide.rollout(Xw)
    assert wide.last_rollout_kernel == "rollout_wave_kernel"


def _solver_problem(H=12, B=16):
    from pyneuralempc_amd import CallbackEngine
    nx, nu = 2, 1
    net = orc.MLP.random(nx + nu, [32, 32], nx, seed=2)
    net.W[-1] *= 0.2
    net.b[-1] *= 0.2
    eng = CallbackEngine(net.W, net.b, H, nx, nu, dtype=torch.float64, device="cuda:0", max_batch=B)
    eng.set_objective(Q=np.eye(nx), R=0.05 * np.eye(nu), xref=np.full((H, nx), 1.0))
    X0 = eng.to_device(np.random.default_rng(3).uniform(-0.6, 0.6, size=(B, nx)))
    lb = np.concatenate([np.full(H * nx, -5.0), np.full(H * nu, -1.0)])
    return net, eng, X0, lb


def test_solver_starts_from_the_rollout():
    """Item 5: init="rollout" is solve from Z_init = rollout(X0), bit for bit; what it reports converged is feasible under
    the oracle and inside the bounds; the default is init="tile".  Iteration counts of both starts are printed, not asserted."""
    nx, nu, H, B = 2, 1, 12, 16
    net, eng, X0, lb = _solver_problem(H, B)
    prob = orc.Problem(net, H, nx, nu, orc.DISCRET, Q=np.eye(nx), R=0.05 * np.eye(nu), xref=np.full((H, nx), 1.0))
    Za, sa, ita = eng.solve(X0, lb=lb, ub=-lb, max_iter=80, init="rollout")
    Zb, sb, itb = eng.solve(X0, Z_init=eng.rollout(X0), lb=lb, ub=-lb, max_iter=80)
    assert torch.equal(Za, Zb) and torch.equal(sa, sb) and ita == itb
    za, x0 = Za.cpu().numpy(), X0.cpu().numpy()
    assert int((sa == 0).sum()) > 0
    for i in np.nonzero(sa.cpu().numpy() == 0)[0]:
        assert np.abs(prob.constraints(za[i], x0[i])).max() <= 1e-8            # tol_constraint's fp64 default
        assert (za[i] >= lb - 1e-12).all() and (za[i] <= -lb + 1e-12).all()
    Zt, st, itt = eng.solve(X0, lb=lb, ub=-lb, max_iter=80)
    Zu, su, itu = eng.solve(X0, lb=lb, ub=-lb, max_iter=80, init="tile")
    assert torch.equal(Zt, Zu) and torch.equal(st, su) and itt == itu
    # a given start keeps its controls: its states are replaced by their roll-out
    Zi = Zt.clone()
    Zi[:, :H * nx] = float("nan")
    Zc, sc, _ = eng.solve(X0, Z_init=Zi, lb=lb, ub=-lb, max_iter=80, init="rollout")
    Zd, sd, _ = eng.solve(X0, Z_init=eng.rollout(X0, U=Zt[:, H * nx:]), lb=lb, ub=-lb, max_iter=80)
    assert torch.equal(Zc, Zd) and torch.equal(sc, sd) and torch.isnan(Zi[:, :H * nx]).all()
    with pytest.raises(ValueError):
        eng.solve(X0, lb=lb, ub=-lb, init="zeros")
    print(f"iterations: init='tile' {itt} ({int((st == 0).sum())}/{B} converged), init='rollout' {ita} ({int((sa == 0).sum())}/{B} converged)")


def _closed_loop_by_hand(eng, X, lb, ub, steps, D, hist=None, **opts):
    """the loop closed_loop_batch documents, written out with eng.solve / eng.rollout / torch slicing"""
    B, H, nx, nu = X.shape[0], eng.H, eng.nx, eng.nu
    Xs, Us, Ss, Zi = [X], [], [], None
    for k in range(steps):
        Z, status, _ = eng.solve(X, Zi, lb, ub, **(opts if k == 0 else dict(opts, mu_init=1e-4)))
        U = Z[:, H * nx:].reshape(B, H, nu).clone()
        Xn = eng.rollout(X, U=U)[:, :nx].clone()
        if D is not None:
            Xn = Xn + D[:, k]
        if hist is not None:
            hist = (torch.cat([hist[0][:, 1:], X[:, None, :]], dim=1).contiguous(),
                    torch.cat([hist[1][:, 1:], U[:, :1]], dim=1).contiguous())
            eng.bind_history(*hist)
        X = Xn.contiguous()
        Zi = eng.rollout(X, U=torch.cat([U[:, 1:], U[:, -1:]], dim=1))
        Xs.append(X), Us.append(U[:, 0]), Ss.append(status)
    return torch.stack(Xs, dim=1).cpu().numpy(), torch.stack(Us, dim=1).cpu().numpy(), torch.stack(Ss, dim=0).cpu().numpy()


@pytest.mark.parametrize("rolling", [False, True])
def test_closed_loop_batch(rolling):
    """Item 6: NMPC.closed_loop_batch against the same loop written out here (bit for bit), its plant steps against the
    oracle's Phi within the per-step bound, its controls within their bounds -- on the 2 x 32 network of the solver tests
    (H = 12) and on a rolling-window model (roll2_discret's network, H = 8); 4 steps, disturbance +-0.02 on steps 1 and 2."""
    import pyneuralempc_amd as nEMPC
    B, steps = 16, 4
    rng = np.random.default_rng(5)
    if rolling:
        d, W, b = load_case("roll2_discret")
        nx, nu, w, H = int(d["nx"]), int(d["nu"]), int(d["window"]), 8
        net = orc.MLP(W, b, case_activations(d))
        model = nEMPC.model.MLPModelRollingInput(W, b, nx, nu, rolling_window=w, device="cuda:0")
        px, pu = rng.uniform(-0.5, 0.5, size=(B, w - 1, nx)), rng.uniform(-0.2, 0.2, size=(B, w - 1, nu))
        obj_kw = dict(Q=np.eye(nx), R=0.1 * np.eye(nu))
    else:
        nx, nu, w, H = 2, 1, 1, 12
        net = orc.MLP.random(nx + nu, [32, 32], nx, seed=2)
        net.W[-1] *= 0.2
        net.b[-1] *= 0.2
        model = nEMPC.model.MLPModel(net.W, net.b, nx, nu, device="cuda:0")
        px = pu = None
        obj_kw = dict(Q=np.eye(nx), R=0.05 * np.eye(nu))
    integ = nEMPC.integrator.DiscretIntegrator(model, H)
    obj = nEMPC.objective.QuadraticObjective(device="cuda:0", **obj_kw)
    dom = nEMPC.constraints.DomainConstraint(states_constraint=[[-5.0, 5.0]] * nx, control_constraint=[[-0.3, 0.3]] * nu)
    mpc = nEMPC.controller.NMPC(integ, obj, [dom], H, 1.0, optimizer=nEMPC.optimizer.DeviceSqp())
    X0 = rng.uniform(-0.6, 0.6, size=(B, nx))
    D = np.zeros((B, steps, nx))
    D[:, 1:3] = rng.uniform(-0.02, 0.02, size=(B, 2, nx))
    kw = {} if not rolling else dict(prev_x=px, prev_u=pu)
    X, U, status = mpc.closed_loop_batch(X0, steps, disturbance=D, max_iter=80, **kw)
    assert X.shape == (B, steps + 1, nx) and U.shape == (B, steps, nu) and status.shape == (steps, B)
    assert np.array_equal(X[:, 0], X0)
    # the same loop by hand on the controller's own engine
    from pyneuralempc_amd.optimizer.base import fused_evaluator
    eng = fused_evaluator(integ, obj, None).engine
    lb, ub = np.asarray(dom.get_lower_bounds(H), dtype=np.float64), np.asarray(dom.get_upper_bounds(H), dtype=np.float64)
    hist = None
    if rolling:
        hist = (eng.to_device(px), eng.to_device(pu))
        eng.bind_history(*hist)
    X2, U2, S2 = _closed_loop_by_hand(eng, eng.to_device(X0), lb, ub, steps, eng.to_device(D), hist, max_iter=80)
    assert np.array_equal(X, X2) and np.array_equal(U, U2) and np.array_equal(status, S2)
    assert (np.abs(U) <= 0.3 + 1e-12).all()
    print(f"closed loop ({'rolling' if rolling else 'plain'}): converged per step {(status == 0).sum(axis=1).tolist()} of {B}")
    # the plant steps against the oracle: x_{k+1} - disturbance_k = Phi(x_k, u_k), histories moving with the loop
    hx = None if not rolling else px.copy()
    hu = None if not rolling else pu.copy()
    for k in range(steps):
        for i in range(B):
            if rolling:
                phi, _, _ = orc.step_rows_rolling(net, orc.DISCRET, X[i, k][None], U[i, k][None], hx[i], hu[i], w, True)
            else:
                phi, _, _ = orc.step_rows(net, orc.DISCRET, 1.0, X[i, k][None], U[i, k][None])
            np.testing.assert_allclose(X[i, k + 1] - D[i, k], phi[0], **F64)
        if rolling:
            hx = np.concatenate([hx[:, 1:], X[:, k][:, None]], axis=1)
            hu = np.concatenate([hu[:, 1:], U[:, k][:, None]], axis=1)


def test_closed_loop_batch_refuses_time_varying_parameters():
    import pyneuralempc_amd as nEMPC
    net = orc.MLP.random(2 + 1 + 1, [16], 2, seed=1)
    model = nEMPC.model.MLPModel(net.W, net.b, 2, 1, tvp_dim=1, device="cuda:0")
    integ = nEMPC.integrator.DiscretIntegrator(model, 4)
    obj = nEMPC.objective.QuadraticObjective(Q=np.eye(2), R=0.1 * np.eye(1), device="cuda:0")
    dom = nEMPC.constraints.DomainConstraint(states_constraint=[[-5.0, 5.0]] * 2, control_constraint=[[-1.0, 1.0]])
    mpc = nEMPC.controller.NMPC(integ, obj, [dom], 4, 1.0, optimizer=nEMPC.optimizer.DeviceSqp())
    with pytest.raises(NotImplementedError, match="tvp"):
        mpc.closed_loop_batch(np.zeros((2, 2)), 2)
