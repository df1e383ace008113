#!/usr/bin/env python3
"""Roll-out time (both kernels) beside one evaluation of the same handle, and the solver's two cold starts.
    python tools/rollout_bench.py [--reps 200] [--rounds 3]
Shapes: B = 1024 and 16384, H = 20, 2/1 network 2 x 64, Discret, fp64 (bench.py c2) and the c3 shape (6/3, 3 x 128, H = 30,
RK4, fp32).  Times are device events around `reps` back-to-back calls after a warm-up, the arms alternated `rounds` times
in one process; the median round is reported with the spread.  Then init="tile" against init="rollout" on the problem of
tests/test_gpu_solver.py::test_warm_started_closed_loop_converges_in_fewer_iterations (cold start only).
Prints to stdout; profiles/r08_rollout.txt is this output, then that of `closed_loop_bench.py --device-loop` and of
`closed_loop_warm_starts.py`, redirected into one file."""
import argparse, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import nempc_oracle as orc
from pyneuralempc_amd import CallbackEngine

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--batches", default="1024,16384", help="1024: the bench shapes' batch; 16384: four 16-problem tiles per compute unit")
args = ap.parse_args()


def timed(fn, reps):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps          # us per call


SHAPES = [("c2  2/1 2x64 H=20 discret f64", 2, 1, [64, 64], 20, "discret", 1.0, torch.float64),
          ("c3  6/3 3x128 H=30 rk4 f32", 6, 3, [128, 128, 128], 30, "rk4", 0.1, torch.float32)]
for B, (name, nx, nu, hidden, H, integ, DT, dtype) in [(int(v), sh) for sh in SHAPES for v in args.batches.split(",")]:
    net = orc.MLP.random(nx + nu, hidden, nx, seed=0)
    eng = CallbackEngine(net.W, net.b, H, nx, nu, integrator=integ, DT=DT, dtype=dtype, device="cuda:0", max_batch=B)
    rng = np.random.default_rng(1)
    X0 = eng.to_device(rng.uniform(-0.5, 0.5, size=(B, nx)))
    Z = eng.rollout(X0, U=eng.to_device(rng.uniform(-0.5, 0.5, size=(B, H, nu))))

    def roll(which):
        def fn():
            os.environ["NEMPC_ROLLOUT_KERNEL"] = which
            eng.rollout(X0, Z=Z)
        return fn
    launch_all, _ = eng.bind(Z, X0)
    launch_g, _ = eng.bind(Z, X0, want=("g",))
    arms = [("rollout generic (1)", roll("1")), ("rollout matrix-core (2)", roll("2")),
            ("eval f, grad, g, jac_dense", launch_all), ("eval g only", launch_g)]
    res = {k: [] for k, _ in arms}
    reps = max(20, args.reps * 1024 // B)
    for _ in range(args.rounds):
        for k, fn in arms:
            res[k].append(timed(fn, reps))
    os.environ.pop("NEMPC_ROLLOUT_KERNEL", None)
    print(f"{name}, B = {B} ({eng.kernel_variant} handle; us per call, median of {args.rounds} rounds of {reps} calls [min .. max])")
    for k, _ in arms:
        v = sorted(res[k])
        print(f"    {k:30s} {v[len(v) // 2]:9.1f}   [{v[0]:.1f} .. {v[-1]:.1f}]")

# the two cold starts of the solver
nx, nu, H, Bs = 2, 1, 20, 64
net = orc.MLP.random(nx + nu, [64, 64], nx, seed=0)
eng = CallbackEngine(net.W, net.b, H, nx, nu, dtype=torch.float64, device="cuda:0", max_batch=Bs)
X = eng.to_device(np.random.default_rng(100).uniform(-0.5, 0.5, size=(Bs, nx)))
lb = np.concatenate([np.full(H * nx, -3.0), np.full(H * nu, -0.5)])
print(f"solver cold start, 2/1 2x64 H=20, B = {Bs}, max_iter = 80 (the closed-loop test's problem):")
for init in ("tile", "rollout"):
    Zs, st, it, per = eng.solve(X, lb=lb, ub=-lb, max_iter=80, init=init, return_iterations=True)
    ok = st == 0
    p = per[ok].float()
    print(f"    init={init:8s} {it:3d} iterations, {int(ok.sum())}/{Bs} converged, per-problem iterations to converge: median "
          f"{p.median().item() if len(p) else 0:.0f} max {p.max().item() if len(p) else 0:.0f}")
