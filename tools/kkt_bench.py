#!/usr/bin/env python3
"""What the KKT residual evaluator and the returned multipliers cost at the headline shape.
    python tools/kkt_bench.py [--reps 200] [--rounds 5] [--batch 1024] [--parent-tree DIR] > profiles/kkt_residual.txt
Shape: B = 1024, H = 20, 2/1 network 2 x 64 tanh, Discret, fp64 (bench.py c2).  Arms, alternated `rounds` times in one
process, device events around `reps` back-to-back calls after a warm-up, median round with the spread:
  eng.kkt_residual(Z, X0, lam, zl, zu, lb, ub)     one evaluation (grad, g, jac_tiles into the handle's buffers) + kkt_residual_kernel
  eng.eval(want=("grad", "g", "jac_tiles"))        that evaluation alone, into the caller's tensors
Their difference is the new kernel's cost (launch included); next to it the bytes the kernel moves -- tiles, gradient,
defects, Z, three multiplier arrays, two bound vectors in, r out -- over that time as a share of the 6.3 TB/s an MI355X
streams from HBM (8 TB/s on paper).  Then a 2-iteration solve at the same dims with bounds on u, with and without the
multipliers handed back (host clock around the call: a solve ends in a stream synchronisation).

--parent-tree: a checkout of the parent commit with its library built.  The tool then starts itself once more in a fresh
process that imports the package from there (--pkg-root DIR --arms parent: eval and the plain solve only, that library has
neither new entry point) and prints both tables and the comparison: kkt_residual here against eval there, and the plain solve here against the plain solve
there within the spread of the rounds.  Records, not gates."""
import argparse, os, subprocess, sys, time
import numpy as np, torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--batch", type=int, default=1024)
ap.add_argument("--solves", type=int, default=20, help="timed solves per arm and round")
ap.add_argument("--arms", choices=("all", "parent"), default="all")
ap.add_argument("--parent-tree", default=None)
ap.add_argument("--pkg-root", default=REPO, help="checkout the package is imported from")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.pkg_root))
from pyneuralempc_amd import CallbackEngine
B, H, nx, nu = args.batch, 20, 2, 1
n, hx = H * (nx + nu), H * nx
HBM_TBS = 6.3
new_arms = args.arms == "all"


def mlp(seed, out_scale):
    """2 x 64 tanh network, seeded (Glorot-scaled normal weights, small biases; output layer scaled by out_scale)."""
    rng = np.random.default_rng(seed)
    dims = [nx + nu, 64, 64, nx]
    W = [rng.normal(size=(a, b)) * np.sqrt(2.0 / (a + b)) for a, b in zip(dims[:-1], dims[1:])]
    b = [0.1 * rng.normal(size=d) for d in dims[1:]]
    W[-1] *= out_scale
    b[-1] *= out_scale
    return W, b


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


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def report(title, arms, res, out):
    out.append(title)
    for k, _ in arms:
        v = sorted(res[k])
        out.append(f"    {k:52s} {med(v):9.2f}   [{v[0]:.2f} .. {v[-1]:.2f}]")


lines = []
W, b = mlp(0, 1.0)
eng = CallbackEngine(W, b, H, nx, nu, integrator="discret", dtype=torch.float64, device="cuda:0", max_batch=B)
eng.set_objective(Q=np.eye(nx), R=0.1 * np.eye(nu))
rng = np.random.default_rng(1)
Z, X0 = eng.to_device(rng.uniform(-0.5, 0.5, size=(B, n))), eng.to_device(rng.uniform(-0.5, 0.5, size=(B, nx)))
lam, zl, zu = eng.to_device(rng.normal(size=(B, hx))), eng.to_device(rng.uniform(size=(B, n))), eng.to_device(rng.uniform(size=(B, n)))
lb = np.concatenate([np.full(hx, -np.inf), np.full(H * nu, -0.5)])
launch_eval, _ = eng.bind(Z, X0, want=("grad", "g", "jac_tiles"))
arms = [("eval(grad, g, jac_tiles)", launch_eval)]
if new_arms:
    arms.insert(0, ("kkt_residual", lambda: eng.kkt_residual(Z, X0, lam, zl, zu, lb, -lb)))
res = {k: [] for k, _ in arms}
for _ in range(args.rounds):
    for k, fn in arms:
        res[k].append(timed(fn, args.reps))
report(f"c2  2/1 2x64 H=20 discret f64, B = {B} ({eng.kernel_variant} handle, rows {eng.last_row_kernel}; us per call, median of "
       f"{args.rounds} rounds of {args.reps} calls [min .. max])", arms, res, lines)
if new_arms:
    diffs = sorted(a - c for a, c in zip(res["kkt_residual"], res["eval(grad, g, jac_tiles)"]))
    esz = 8
    moved = B * (hx * (nx + nu) + n + hx + n + hx + 2 * n + 4) * esz + 2 * n * 8     # tiles, grad, g, Z, lam, zl, zu, r; lb, ub
    d = med(diffs)
    lines.append(f"    kkt_residual - eval, round by round: median {d:.2f} us [{diffs[0]:.2f} .. {diffs[-1]:.2f}]: kkt_residual_kernel with "
                 f"its launch; it moves {moved / 1e6:.2f} MB -> {moved / max(d, 1e-9) / 1e6:.3f} TB/s, "
                 f"{100.0 * moved / max(d, 1e-9) / 1e6 / HBM_TBS:.1f} % of {HBM_TBS} TB/s "
                 f"({100.0 * d / med(res['eval(grad, g, jac_tiles)']):.1f} % of the evaluation it follows)")

# ---- a 2-iteration solve, with and without the multipliers
W, b = mlp(3, 0.2)
eng = CallbackEngine(W, b, H, nx, nu, integrator="discret", dtype=torch.float64, device="cuda:0", max_batch=B)
eng.set_objective(Q=np.eye(nx), R=0.1 * np.eye(nu))
X0 = eng.to_device(np.random.default_rng(4).uniform(-0.8, 0.8, size=(B, nx)))
lbs = np.concatenate([np.full(hx, -3.0), np.full(H * nu, -0.5)])


def solve_arm(duals):
    def fn():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = eng.solve(X0, lb=lbs, ub=-lbs, max_iter=2, **({"return_duals": True} if duals else {}))
        return (time.perf_counter() - t0) * 1e6, out
    return fn


sarms = [("solve, max_iter = 2", solve_arm(False))] + ([("solve, max_iter = 2, return_duals", solve_arm(True))] if new_arms else [])
sres, outs = {k: [] for k, _ in sarms}, {}
for k, fn in sarms:
    for _ in range(5):
        fn()
for _ in range(args.rounds):
    for k, fn in sarms:
        ts = []
        for _ in range(args.solves):
            dt, outs[k] = fn()
            ts.append(dt)
        sres[k].append(med(ts))
report(f"solve, same dims, B = {B}, bounds on u (us of wall time per solve, median of {args.rounds} rounds of the median of "
       f"{args.solves} solves [min .. max])", sarms, sres, lines)
if new_arms:
    lines.append(f"    Z identical with and without the multipliers: {bool(torch.equal(outs[sarms[0][0]][0], outs[sarms[1][0]][0]))}")

if args.arms == "parent":
    print("\n".join(lines))
    print(f"#medians eval {med(res['eval(grad, g, jac_tiles)']):.4f} {min(res['eval(grad, g, jac_tiles)']):.4f} {max(res['eval(grad, g, jac_tiles)']):.4f} "
          f"solve {med(sres[sarms[0][0]]):.4f} {min(sres[sarms[0][0]]):.4f} {max(sres[sarms[0][0]]):.4f}")
    sys.exit(0)

print("\n".join(lines))
if args.parent_tree:
    # the parent commit's package and library in a fresh process of its own (this one is idle meanwhile)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--arms", "parent", "--pkg-root", os.path.abspath(args.parent_tree),
                        "--reps", str(args.reps), "--rounds", str(args.rounds), "--batch", str(B), "--solves", str(args.solves)],
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        print(r.stdout[-3000:] + r.stderr[-3000:])
        sys.exit(1)
    body = [ln for ln in r.stdout.splitlines() if not ln.startswith("#medians")]
    tail = [ln for ln in r.stdout.splitlines() if ln.startswith("#medians")][0].split()
    pe, pe_lo, pe_hi, ps, ps_lo, ps_hi = (float(tail[i]) for i in (2, 3, 4, 6, 7, 8))
    print("\nparent commit (its package, its library), same tool, same machine, right after:")
    print("\n".join(body))
    k = med(res["kkt_residual"])
    s = sres[sarms[0][0]]
    print(f"\nkkt_residual here {k:.2f} us against eval of the parent {pe:.2f} us [{pe_lo:.2f} .. {pe_hi:.2f}]: + {k - pe:.2f} us "
          f"({100.0 * (k - pe) / pe:.1f} %)")
    print(f"plain solve here {med(s):.1f} us [{min(s):.1f} .. {max(s):.1f}] against the parent's {ps:.1f} us [{ps_lo:.1f} .. {ps_hi:.1f}]: "
          f"{'inside' if min(s) <= ps_hi and ps_lo <= max(s) else 'OUTSIDE'} each other's spread")
