#!/usr/bin/env python3
"""What an input-rate binding (nempc_bind_rate) costs at the headline shape.
    python tools/rate_bench.py [--solves 8] [--batch 1024] >> profiles/rate_penalty.txt
Shape: B = 1024, H = 20, 2/1 network 2 x 64 tanh, Discret, fp64, bounds on u, a 40-iteration budget (the solver setting of
tools/tracking_bench.py).  One solve, three ways, alternated in one process after a warm-up solve each (two handles of the
same network: the solver's workspace is sized for the stage it runs on, and a handle that alternates between the plain and
the augmented stage would rebuild it inside every timed solve):
  plain      no binding: the compiled 2/1 schedule (LQ scan, two launches per iteration)
  penalty    S = 0.2 I, no limits: the augmented 3/1 stage -- run-time-dimension LQ kernel, gather / rows / blocks / spread /
             acceptance launches of their own
  limits     the same penalty and |du| <= 0.1
Per leg: mean of `solves` single-solve wall timings with their range (the host clock brackets a synchronising call),
iterations run, time per iteration, converged share.  A record, not a gate."""
import argparse, os, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import nempc_oracle as orc
from pyneuralempc_amd import CallbackEngine

ap = argparse.ArgumentParser()
ap.add_argument("--solves", type=int, default=8, help="timed solves per leg (at least six)")
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--iters", type=int, default=40)
args = ap.parse_args()
B, H, nx, nu = args.batch, 20, 2, 1
if args.solves < 6:
    sys.exit("--solves must be at least 6")

net = orc.MLP.random(nx + nu, [64, 64], nx, seed=3)
net.W[-1] *= 0.2
net.b[-1] *= 0.2
engines = []
for _ in range(2):
    e = CallbackEngine(net.W, net.b, H, nx, nu, integrator="discret", dtype=torch.float64, device="cuda:0", max_batch=B)
    e.set_objective(Q=np.eye(nx), R=0.1 * np.eye(nu))
    engines.append(e)
eng, eng_rate = engines
rng = np.random.default_rng(4)
X0 = eng.to_device(rng.uniform(-0.8, 0.8, size=(B, nx)))
u_prev = eng.to_device(rng.uniform(-0.2, 0.2, size=(B, nu)))
lb = np.concatenate([np.full(H * nx, -3.0), np.full(H * nu, -0.5)])
S = 0.2 * np.eye(nu)
legs = [("plain (no binding)", None), ("penalty S = 0.2 I", dict(u_prev=u_prev, S=S)),
        ("penalty and limits |du| <= 0.1", dict(u_prev=u_prev, S=S, du_lb=[-0.1] * nu, du_ub=[0.1] * nu))]


def solve(binding):
    e = eng if binding is None else eng_rate
    if binding is not None:
        e.bind_rate(**binding)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = e.solve(X0, lb=lb, ub=-lb, max_iter=args.iters)        # (synchronises)
    return time.perf_counter() - t0, out, e.last_lq_kernel


res, info = {k: [] for k, _ in legs}, {}
for k, bnd in legs:
    info[k] = [solve(bnd)[2]]              # warm-up: workspaces, code objects
for _ in range(args.solves):
    for k, bnd in legs:
        dt, (Z, st, it), _ = solve(bnd)
        res[k].append(dt * 1e3)
        info[k][1:] = [it, int((st == 0).sum())]
eng_rate.bind_rate()
print(f"rate_bench: 2/1 2x64 tanh H={H} discret f64, B = {B}, max_iter = {args.iters}, bounds on u ({eng.kernel_variant} handle); "
      f"ms per solve, mean of {args.solves} single solves [min .. max]")
base = float(np.mean(res[legs[0][0]]))
for k, _ in legs:
    v = res[k]
    lq, it, ok = info[k]
    print(f"    {k:34s} {np.mean(v):8.3f}   [{min(v):.3f} .. {max(v):.3f}]   x{np.mean(v) / base:5.2f}   {it:3d} iterations, "
          f"{1e3 * np.mean(v) / max(it, 1):7.1f} us / iteration, LQ plan {lq}, {ok}/{B} converged")
