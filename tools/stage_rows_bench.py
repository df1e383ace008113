#!/usr/bin/env python3
"""What a stage-rows binding (nempc_bind_stage_rows) costs at the headline solver shape, and that the plain solve costs what it
did before the binding existed.
    python tools/stage_rows_bench.py [--solves 8] [--batch 1024] [--parent-lib PATH/libnempc.so] >> profiles/stage_rows.txt
Shape: B = 1024, H = 20, 2/1 network 2 x 64 tanh, Discret, fp64, bounds on u, a 40-iteration budget (the solver setting of
tools/rate_bench.py).  One solve, four ways, alternated in one process after three warm-up solves each (which also prime the
clocks; one handle per leg, all of the same network: the solver's workspace is sized for the stage it runs on, and a handle that
alternates between stages would rebuild it inside every timed solve):
  plain        no binding: the compiled 2/1 schedule (LQ scan, two launches per iteration)
  row, no limit  one mixed row with infinite limits: the augmented 3/1 stage -- run-time-dimension LQ kernel, gather / rows /
               blocks / spread / acceptance launches of their own --, no barrier term from the row
  row, active  the same row with an upper limit that is active in most problems
  rate S = 0   a rate binding with S = 0 and no limits: the existing augmented path at the same stage size (3/1)
Per leg: mean of `solves` single-solve wall timings with their range (the host clock brackets a synchronising call),
iterations run, time per iteration, converged share.
--parent-lib: the plain leg alone, in child processes that load either this tree's library or the given build of the parent
commit (NEMPC_LIB), alternated `--rounds` times; per library the mean over the rounds of the per-process means, and the spread
of those means, which is the run-to-run spread the difference is held against.  A record, not a gate."""
import argparse, json, os, subprocess, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import nempc_oracle as orc
from pyneuralempc_amd import CallbackEngine, _lib

ap = argparse.ArgumentParser()
ap.add_argument("--solves", type=int, default=8, help="timed solves per leg (at least five)")
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--iters", type=int, default=40)
ap.add_argument("--parent-lib", default=None, help="libnempc.so built from the parent commit")
ap.add_argument("--rounds", type=int, default=5, help="alternations of the two libraries (at least five)")
ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
args = ap.parse_args()
B, H, nx, nu = args.batch, 20, 2, 1
if args.solves < 5 or args.rounds < 5:
    sys.exit("--solves and --rounds must be at least 5")
WARM = 3

net = orc.MLP.random(nx + nu, [64, 64], nx, seed=3)
net.W[-1] *= 0.2
net.b[-1] *= 0.2


def engine():
    e = CallbackEngine(net.W, net.b, H, nx, nu, integrator="discret", dtype=torch.float64, device="cuda:0", max_batch=B)
    e.set_objective(Q=np.eye(nx), R=0.1 * np.eye(nu))
    return e


rng = np.random.default_rng(4)
X0h = rng.uniform(-0.8, 0.8, size=(B, nx))
lb = np.concatenate([np.full(H * nx, -3.0), np.full(H * nu, -0.5)])


def timed(e, X0):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = e.solve(X0, lb=lb, ub=-lb, max_iter=args.iters)        # (synchronises)
    return (time.perf_counter() - t0) * 1e3, out


if args.child:      # the plain leg alone, on whatever library NEMPC_LIB names
    e = engine()
    X0 = e.to_device(X0h)
    for _ in range(WARM):
        timed(e, X0)
    v = [timed(e, X0) for _ in range(args.solves)]
    Z, st, it = v[-1][1]
    print(json.dumps(dict(ms=[t for t, _ in v], iters=it, converged=int((st == 0).sum()), lq=e.last_lq_kernel,
                          zsum=float(Z.double().abs().sum().item()))))
    sys.exit(0)

eng, eng_rows, eng_act, eng_rate = engine(), engine(), engine(), engine()
X0 = eng.to_device(X0h)
ROW = np.array([[1.0, -0.5, 2.0]])
# the active limit: 40 % of the largest value the row reaches in the plain solution
Zp = eng.solve(X0, lb=lb, ub=-lb, max_iter=args.iters)[0].cpu().numpy()
rv = Zp[:, :H * nx].reshape(B, H, nx) @ ROW[0, :nx] + Zp[:, H * nx:].reshape(B, H, nu) @ ROW[0, nx:]
LIMIT = round(0.4 * float(rv.max()), 3)
u_prev = eng.to_device(np.zeros((B, nu)))
legs = [("plain (no binding)", eng, lambda: None),
        ("one row, infinite limits", eng_rows, lambda: eng_rows.bind_rows(ROW)),
        (f"one row <= {LIMIT} (active)", eng_act, lambda: eng_act.bind_rows(ROW, None, [LIMIT])),
        ("rate binding, S = 0, no limits", eng_rate, lambda: eng_rate.bind_rate(u_prev=u_prev, S=np.zeros((nu, nu))))]
res, info = {k: [] for k, _, _ in legs}, {}
for k, e, bind in legs:
    bind()
    for _ in range(WARM):
        timed(e, X0)
    info[k] = [e.last_lq_kernel]
for _ in range(args.solves):
    for k, e, bind in legs:
        bind()
        dt, (Z, st, it) = timed(e, X0)
        res[k].append(dt)
        info[k][1:] = [it, int((st == 0).sum())]
        if "active" in k:
            zr = Z.cpu().numpy()
            info[k].append(int((((zr[:, :H * nx].reshape(B, H, nx) @ ROW[0, :nx] + zr[:, H * nx:].reshape(B, H, nu) @ ROW[0, nx:])
                                 >= LIMIT - 1e-6).any(axis=1)).sum()))
eng_rows.bind_rows()
eng_act.bind_rows()
eng_rate.bind_rate()
print(f"stage_rows_bench: 2/1 2x64 tanh H={H} discret f64, B = {B}, max_iter = {args.iters}, bounds on u ({eng.kernel_variant} handle); "
      f"ms per solve, mean of {args.solves} single solves [min .. max] after {WARM} warm-up solves per leg")
base = float(np.mean(res[legs[0][0]]))
for k, _, _ in legs:
    v = res[k]
    lq, it, ok = info[k][:3]
    extra = f", row active in {info[k][-1]}/{B} problems" if "active" in k else ""
    print(f"    {k:34s} {np.mean(v):8.3f}   [{min(v):.3f} .. {max(v):.3f}]   x{np.mean(v) / base:5.2f}   {it:3d} iterations, "
          f"{1e3 * np.mean(v) / max(it, 1):7.1f} us / iteration, LQ plan {lq}, {ok}/{B} converged{extra}")

if args.parent_lib:
    libs = [("this tree", _lib.LIB_PATH), ("parent commit", os.path.abspath(args.parent_lib))]
    means = {k: [] for k, _ in libs}
    last = {}
    for _ in range(args.rounds):
        for k, path in libs:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--solves", str(args.solves), "--batch", str(B),
                                "--iters", str(args.iters)], env=dict(os.environ, NEMPC_LIB=path), capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                sys.exit(f"child process on {k} failed ({r.returncode}): {r.stderr[-800:]}")
            last[k] = json.loads(r.stdout.strip().splitlines()[-1])
            means[k].append(float(np.mean(last[k]["ms"])))
    print(f"  plain solve, this tree against a build of the parent commit: {args.rounds} alternated processes each, {args.solves} timed solves "
          f"per process after {WARM} warm-up solves; ms per solve, mean of the per-process means [min .. max of them]")
    for k, _ in libs:
        v = means[k]
        print(f"    {k:16s} {np.mean(v):8.3f}   [{min(v):.3f} .. {max(v):.3f}]   {last[k]['iters']} iterations, LQ plan {last[k]['lq']}, "
              f"{last[k]['converged']}/{B} converged, sum |Z| = {last[k]['zsum']:.12e}")
    a, b = means["this tree"], means["parent commit"]
    spread = max(max(a) - min(a), max(b) - min(b))
    diff = float(np.mean(a) - np.mean(b))
    print(f"    difference of the means {diff:+.3f} ms; run-to-run spread of the per-process means {spread:.3f} ms: "
          + ("within the spread" if diff <= spread else "SLOWER than the parent by more than the spread"))
