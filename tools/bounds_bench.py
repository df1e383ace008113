#!/usr/bin/env python3
"""What per-problem bounds (nempc_bind_bounds) cost, and that solves without a binding do not pay for them.
    python tools/bounds_bench.py [--rounds 4] [--parent-tree DIR] > profiles/per_problem_bounds.txt
Two shapes, B = 1024: the headline 2/1 (2 x 64 tanh, Discret, H = 20, fp64, tools/solver_bench.py's problem, 40 iterations) and
configs[2] dims (6/3, 3 x 128 tanh, RK4, H = 30, fp32, bench.py's solver_c3 problem, 40 iterations).  One RUN is a fresh process
that times ONE solve per arm (the second of two, wall clock around a call that ends in a stream synchronisation):
    bounded      |x| <= 3, |u| <= 0.5 as the host lb / ub of the call
    unbounded    no bounds
    uniform      the same limits bound per problem (B copies), no host vector   [only a library that has nempc_bind_bounds]
--parent-tree: a checkout of the parent commit with its library built; its runs import the package from there (--pkg-root).
Every round is then three runs in this order: parent, parent again, branch
(the method of profiles/solver_split_ab.txt): the parent's own runs give the A/A range the branch's mean is held against.
A record; the verdict line says whether each branch mean lies inside the parent's range."""
import argparse, os, subprocess, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--parent-tree", default=None)
ap.add_argument("--pkg-root", default=REPO, help="checkout the package is imported from")
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--iters", type=int, default=40)
ap.add_argument("--one-run", action="store_true", help="(internal) time the arms once with the package of --pkg-root")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.pkg_root))

SHAPES = {"c2": dict(nx=2, nu=1, hidden=[64, 64], H=20, integ="discret", DT=1.0, f64=True, seed=0, scale=0.2, x0_seed=11, x0=1.0),
          "c3": dict(nx=6, nu=3, hidden=[128, 128, 128], H=30, integ="rk4", DT=0.1, f64=False, seed=0, scale=1.0, x0_seed=100, x0=0.5)}


def one_run():
    import numpy as np, torch
    from oracle import nempc_oracle as orc
    from pyneuralempc_amd import CallbackEngine
    B, mi = args.batch, args.iters
    for name, c in SHAPES.items():
        nx, nu, H = c["nx"], c["nu"], c["H"]
        net = orc.MLP.random(nx + nu, c["hidden"], nx, seed=c["seed"])
        net.W[-1] *= c["scale"]
        net.b[-1] *= c["scale"]
        eng = CallbackEngine(net.W, net.b, H, nx, nu, integrator=c["integ"], DT=c["DT"], dtype=torch.float64 if c["f64"] else torch.float32,
                             device="cuda:0", max_batch=B)
        X0 = eng.to_device(np.random.default_rng(c["x0_seed"]).uniform(-c["x0"], c["x0"], size=(B, nx)))
        lb = np.concatenate([np.full(H * nx, -3.0), np.full(H * nu, -0.5)])
        arms = ["bounded", "unbounded"] + (["uniform"] if hasattr(eng, "bind_bounds") and hasattr(eng.lib, "nempc_bind_bounds") else [])
        for arm in arms:
            if arm == "uniform":
                xs, us = torch.full((B, H, nx), 3.0, dtype=eng.dtype, device=eng.device), torch.full((B, H, nu), 0.5, dtype=eng.dtype, device=eng.device)
                eng.bind_bounds(xlb=-xs, xub=xs, ulb=-us, uub=us)
            kw = dict(lb=lb, ub=-lb) if arm == "bounded" else {}
            for rep in range(2):
                torch.cuda.synchronize()
                t = time.perf_counter()
                Z, st, it = eng.solve(X0, max_iter=mi, **kw)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t
            if arm == "uniform":
                eng.bind_bounds()
            print(f"#run {name} {arm} {dt * 1e3:.4f} {it} {int((st == 0).sum())}")


if args.one_run:
    one_run()
    sys.exit(0)


def run(tree):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one-run", "--pkg-root", os.path.abspath(tree or REPO),
                        "--batch", str(args.batch), "--iters", str(args.iters)], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        print(r.stdout[-2000:] + r.stderr[-2000:])
        sys.exit(1)
    out = {}
    for ln in r.stdout.splitlines():
        if ln.startswith("#run "):
            _, shape, arm, ms, it, ok = ln.split()
            out[(shape, arm)] = (float(ms), int(it), int(ok))
    return out


sides = ([("parent", args.parent_tree), ("parent_again", args.parent_tree)] if args.parent_tree else []) + [("branch", None)]
res, raw = {}, []
for rnd in range(args.rounds):
    for side, tree in sides:
        out = run(tree)
        raw.append(f"== round {rnd} {side}")
        for (shape, arm), (ms, it, ok) in out.items():
            raw.append(f"{shape} {arm} B={args.batch} max_iter={args.iters}: {ms:.3f} ms, {it} iterations, {ok}/{args.batch} converged")
            res.setdefault((shape, arm, "parent" if side.startswith("parent") else "branch"), []).append(ms)
mean = lambda v: sum(v) / len(v)
print(f"Per-problem bounds: single-solve timings, B = {args.batch}, {args.iters} iterations, one process per run, {args.rounds} rounds of "
      f"{' / '.join(s for s, _ in sides)} (ms per solve)")
for shape in SHAPES:
    for arm in ("bounded", "unbounded", "uniform"):
        br = res.get((shape, arm, "branch"))
        if not br:
            continue
        pa = res.get((shape, arm, "parent"))
        line = f"{shape} {arm:10s} branch {' '.join(f'{v:.3f}' for v in br)} (mean {mean(br):.3f})"
        if pa:
            inside = min(pa) <= mean(br) <= max(pa)
            line += (f"   parent {' '.join(f'{v:.3f}' for v in pa)} (range {min(pa):.3f} .. {max(pa):.3f}, mean {mean(pa):.3f})   "
                     f"branch mean {'inside' if inside else 'OUTSIDE'} the parent's range")
        elif arm == "uniform":
            sh = res[(shape, "bounded", "branch")]
            line += f"   against the shared vector's {mean(sh):.3f}: {100.0 * (mean(br) - mean(sh)) / mean(sh):+.1f} %"
        print(line)
print("\nRaw output:")
print("\n".join(raw))
