#!/usr/bin/env python3
"""What the solution sensitivities (CallbackEngine.sensitivity, nempc_sensitivity) cost, and how well they predict.
    python tools/sensitivity_bench.py [--reps 100] [--rounds 5] [--batch 1024] > profiles/sensitivity.txt
Two shapes: the headline (B = 1024, H = 20, 2/1 network 2 x 64 tanh, Discret, fp64: bench.py c2) and configs[2] dims
(6/3 network 3 x 128 tanh, H = 30, RK4, fp32: bench.py c3).  Per shape the bounded problems are solved first and the calls
are timed at the solution with its multipliers.  Arms, alternated `rounds` times in one process, device events around
`reps` back-to-back calls after a warm-up, median round with the spread:
  sensitivity(want = du0)          evaluation + Lagrangian blocks + sweep, the gain K0 only
  sensitivity(want = all four)     ... with dz, dlam and the time-varying gains written as well
  eval(grad, g, jac_tiles)         one evaluation
  hess(hblocks)                    the Lagrangian blocks (sensitivity - eval - hess: the sweep kernel with its launch)
  kkt_residual                     one evaluation + the residual kernel
  sensitivity(want = dz)           the call kkt_solve is measured against: the same evaluation, block launch and backward sweep
  kkt_solve(nrhs = 1 | 16)         adjoint solve (CallbackEngine.kkt_solve, nempc_kkt_solve), random right-hand sides, v and gx0
and the solve's wall time per iteration (a solve ends in a stream synchronisation).  Then the first-order predictor:
|Z(x0 + d) - Z(x0) - S d|inf over the problems whose two solves converged and whose sensitivity status is 0, d random with
|d|inf = 1e-2 and 1e-3 (the error should fall a hundredfold: it is second order).  Records, not gates."""
import argparse, os, sys, time
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pyneuralempc_amd import CallbackEngine

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=100)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--batch", type=int, default=1024)
args = ap.parse_args()
B = args.batch


def mlp(dims, seed, out_scale):
    rng = np.random.default_rng(seed)
    W = [rng.normal(size=(a, b)) * np.sqrt(2.0 / (a + b)) for a, b in zip(dims[:-1], dims[1:])]
    b = [0.1 * rng.normal(size=d) for d in dims[1:]]
    W[-1] *= out_scale
    b[-1] *= out_scale
    return W, b


def timed(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps          # us per call


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


SHAPES = [
    ("c2  2/1 2x64 H=20 discret f64", dict(nx=2, nu=1, hidden=[64, 64], H=20, integrator="discret", DT=1.0, dtype=torch.float64)),
    ("c3  6/3 3x128 H=30 rk4 f32", dict(nx=6, nu=3, hidden=[128, 128, 128], H=30, integrator="rk4", DT=0.1, dtype=torch.float32)),
]
for title, c in SHAPES:
    nx, nu, H = c["nx"], c["nu"], c["H"]
    n, hx = H * (nx + nu), H * nx
    W, b = mlp([nx + nu] + c["hidden"] + [nx], 3, 0.2)
    eng = CallbackEngine(W, b, H, nx, nu, integrator=c["integrator"], DT=c["DT"], dtype=c["dtype"], device="cuda:0", max_batch=B)
    eng.set_objective(Q=np.eye(nx), R=0.1 * np.eye(nu))
    rng = np.random.default_rng(4)
    x0 = rng.uniform(-0.8, 0.8, size=(B, nx))
    X0 = eng.to_device(x0)
    lb = np.concatenate([np.full(hx, -3.0), np.full(H * nu, -0.5)])
    kw = dict(lb=lb, ub=-lb, max_iter=60, return_duals=True)
    Z, st, it, d = eng.solve(X0, **kw)
    ok = (st == 0).cpu().numpy()
    ts = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.solve(X0, **kw)
        ts.append((time.perf_counter() - t0) * 1e6)
    ones = torch.ones(B, dtype=c["dtype"], device="cuda:0")
    launch_eval, _ = eng.bind(Z, X0, want=("grad", "g", "jac_tiles"))
    arms = [("sensitivity(want = du0)", lambda: eng.sensitivity(Z, X0, d["lam"], d["zl"], d["zu"], lb, -lb, want=("du0",))),
            ("sensitivity(want = du0, dz, dlam, gains)",
             lambda: eng.sensitivity(Z, X0, d["lam"], d["zl"], d["zu"], lb, -lb, want=("du0", "dz", "dlam", "gains"))),
            ("eval(grad, g, jac_tiles)", launch_eval),
            ("hess(hblocks)", lambda: eng.hess(Z, X0, d["lam"], ones, want=("hblocks",))),
            ("kkt_residual", lambda: eng.kkt_residual(Z, X0, d["lam"], d["zl"], d["zu"], lb, -lb)),
            ("sensitivity(want = dz)", lambda: eng.sensitivity(Z, X0, d["lam"], d["zl"], d["zu"], lb, -lb, want=("dz",)))]
    for k in (1, 16):
        rz = eng.to_device(np.random.default_rng(6).normal(size=(B, k, n)))
        arms.append((f"kkt_solve(nrhs = {k}, want = v, gx0)",
                     lambda rz=rz: eng.kkt_solve(Z, X0, d["lam"], d["zl"], d["zu"], lb, -lb, rz=rz, want=("v", "gx0"))))
    res = {k: [] for k, _ in arms}
    for _ in range(args.rounds):
        for k, fn in arms:
            res[k].append(timed(fn, args.reps))
    print(f"{title}, B = {B} ({eng.kernel_variant} handle; us per call, median of {args.rounds} rounds of {args.reps} calls [min .. max])")
    for k, _ in arms:
        v = sorted(res[k])
        print(f"    {k:52s} {med(v):9.2f}   [{v[0]:.2f} .. {v[-1]:.2f}]")
    print(f"    solve to convergence ({it} iterations, {int(ok.sum())}/{B} converged): {med(ts):.1f} us of wall time, "
          f"{med(ts) / max(it, 1):.1f} us per iteration; sensitivity(du0) = {med(res[arms[0][0]]) / (med(ts) / max(it, 1)):.2f} iterations")
    s = eng.sensitivity(Z, X0, d["lam"], d["zl"], d["zu"], lb, -lb, want=("dz",))
    S, sst = s["dz"].double().cpu().numpy(), s["status"].cpu().numpy()
    z = Z.double().cpu().numpy()
    print(f"    sensitivity status: {int((sst == 0).sum())} ok, {int((sst == 1).sum())} not positive definite, {int((sst == 2).sum())} undefined Sigma")
    for size in (1e-2, 1e-3):
        dx = size * np.random.default_rng(5).uniform(-1.0, 1.0, size=(B, nx))
        Zp, stp, _, _ = eng.solve(eng.to_device(x0 + dx), **kw)
        use = ok & (stp == 0).cpu().numpy() & (sst == 0)
        err = np.abs(Zp.double().cpu().numpy() - z - np.einsum("bij,bj->bi", S, dx))[use]
        move = np.abs(Zp.double().cpu().numpy() - z)[use]
        print(f"    predictor, |d|inf = {size:g}: |Z(x0 + d) - Z(x0) - S d|inf median {np.median(err.max(axis=1)):.3e}, max {err.max():.3e} "
              f"over {int(use.sum())} problems (|Z(x0 + d) - Z(x0)|inf median {np.median(move.max(axis=1)):.3e})")
    print()
