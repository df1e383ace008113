#!/usr/bin/env python3
"""What a per-problem tracking binding (nempc_bind_tracking) costs at the headline shape.
    python tools/tracking_bench.py [--reps 200] [--rounds 3] [--batch 1024] > profiles/tracking_objective.txt
Shape: B = 1024, H = 20, 2/1 network 2 x 64 tanh, Discret, fp64 (bench.py c2).  Arms, alternated `rounds` times in one
process, device events around `reps` back-to-back calls after a warm-up, median round with the spread:
  eval(f, grad, g, jac_dense)  shared objective: ONE launch (rows_coopfx_kernel with the objective and the dense rows)
                               with a binding: that launch with f = grad = NULL, then objective_tracking_kernel
  eval(f, grad)                shared: objective_kernel alone; with a binding: objective_tracking_kernel alone
Then a 40-iteration solve at the same dims (bounds on u, the setting of tests/test_gpu_solver.py's compaction test) with the
shared objective, with B copies of it bound (the same problems: the iterates are bit-identical, the difference is the
launch forms) and with a set-point per problem: wall time per iteration and converged share.  Records, not gates: they
decide whether fusing the per-problem objective into the row launches is worth a follow-up (DESIGN "Per-problem tracking
data")."""
import argparse, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import nempc_oracle as orc
from pyneuralempc_amd import CallbackEngine

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--solves", type=int, default=5, help="timed solves per arm and round")
args = ap.parse_args()
B, H, nx, nu = args.batch, 20, 2, 1
NAMES = ("xref", "uref", "cx", "cu")


def timed(arm, reps):
    setup, fn = arm
    setup()                 # (the binding is set once per timed window: the window holds the evaluation calls alone)
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


def report(title, arms, res):
    print(title)
    for k, _ in arms:
        v = sorted(res[k])
        print(f"    {k:44s} {v[len(v) // 2]:9.1f}   [{v[0]:.1f} .. {v[-1]:.1f}]")


net = orc.MLP.random(nx + nu, [64, 64], nx, seed=0)
eng = CallbackEngine(net.W, net.b, H, nx, nu, integrator="discret", dtype=torch.float64, device="cuda:0", max_batch=B)
rng = np.random.default_rng(1)
shared = dict(xref=0.1 * rng.normal(size=(H, nx)), uref=0.1 * rng.normal(size=(H, nu)), cx=0.1 * rng.normal(size=(H, nx)),
              cu=0.1 * rng.normal(size=(H, nu)))
eng.set_objective(Q=np.eye(nx), R=0.1 * np.eye(nu), **shared)
Zh, X0h = orc.synthetic_inputs(B, H, nx, nu, seed=1)
Z, X0 = eng.to_device(Zh), eng.to_device(X0h)
per = {k: eng.to_device(v[None] + 0.1 * rng.normal(size=(B,) + v.shape)) for k, v in shared.items()}
launch_all, out_all = eng.bind(Z, X0)
launch_obj, out_obj = eng.bind(Z, X0, want=("f", "grad"))


def arm(launch, bound):
    return (lambda: eng.bind_tracking(**per)) if bound else (lambda: eng.bind_tracking()), launch


arms = [("eval f, grad, g, jac_dense   shared", arm(launch_all, False)), ("eval f, grad, g, jac_dense   bound", arm(launch_all, True)),
        ("eval f, grad (objective_kernel)   shared", arm(launch_obj, False)),
        ("eval f, grad (objective_tracking_kernel)   bound", arm(launch_obj, True))]
res = {k: [] for k, _ in arms}
for _ in range(args.rounds):
    for k, fn in arms:
        res[k].append(timed(fn, args.reps))
eng.bind_tracking()
report(f"c2  2/1 2x64 H=20 discret f64, B = {B} ({eng.kernel_variant} handle, rows {eng.last_row_kernel}; us per call, "
       f"median of {args.rounds} rounds of {args.reps} calls [min .. max])", arms, res)

# ---- the solver, both ways
net = orc.MLP.random(nx + nu, [64, 64], nx, seed=3)
net.W[-1] *= 0.2
net.b[-1] *= 0.2
eng = CallbackEngine(net.W, net.b, H, nx, nu, integrator="discret", dtype=torch.float64, device="cuda:0", max_batch=B)
zero = dict(xref=np.zeros((H, nx)), uref=np.zeros((H, nu)), cx=np.zeros((H, nx)), cu=np.zeros((H, nu)))
eng.set_objective(Q=np.eye(nx), R=0.1 * np.eye(nu), **zero)
rng = np.random.default_rng(4)
X0 = eng.to_device(rng.uniform(-0.8, 0.8, size=(B, nx)))
lb = np.concatenate([np.full(H * nx, -3.0), np.full(H * nu, -0.5)])
uniform = {k: eng.to_device(np.broadcast_to(v[None], (B,) + v.shape)) for k, v in zero.items()}
setpts = dict(uniform, xref=eng.to_device(np.broadcast_to(rng.uniform(-0.4, 0.4, size=(B, 1, nx)), (B, H, nx))))
ITERS = 40


def solve_arm(binding):
    def fn():
        if binding is None:
            eng.bind_tracking()
        else:
            eng.bind_tracking(**binding)
        t0 = time.perf_counter()
        out = eng.solve(X0, lb=lb, ub=-lb, max_iter=ITERS)        # (synchronises: the host clock brackets finished work)
        return time.perf_counter() - t0, out
    return fn


sarms = [("solve, shared objective", solve_arm(None)), ("solve, B copies of it bound", solve_arm(uniform)),
         ("solve, one set-point per problem bound", solve_arm(setpts))]
sres, info = {k: [] for k, _ in sarms}, {}
for k, fn in sarms:
    fn()                    # warm-up: workspaces, code objects
for _ in range(args.rounds):
    for k, fn in sarms:
        ts = []
        for _ in range(args.solves):
            dt, (Zs, st, it) = fn()
            ts.append(dt * 1e6 / max(it, 1))
        sres[k].append(sorted(ts)[len(ts) // 2])
        info[k] = (it, int((st == 0).sum()), Zs.clone())
eng.bind_tracking()
report(f"solve, same dims, B = {B}, max_iter = {ITERS}, bounds on u (us of wall time per iteration, median of {args.rounds} rounds of "
       f"{args.solves} solves [min .. max])", sarms, sres)
for k, _ in sarms:
    it, ok, _ = info[k]
    print(f"    {k:44s} {it:3d} iterations run, {ok}/{B} converged ({100.0 * ok / B:.1f} %)")
print(f"    shared and uniform-bound iterates bit-identical: {bool(torch.equal(info[sarms[0][0]][2], info[sarms[1][0]][2]))}")
