#!/usr/bin/env python3
"""The layered path beyond 16 states / 32 decision inputs against the generic thread-per-row kernel, on one build: the whole
evaluation (f, grad, g, sparse Jacobian) and the exact-Hessian callback at B = 1024, H = 20.  HIP events after 40 ms of priming
launches, best of three (as tools/layered_ab.py); one process per (shape, kernel) so that no handle's workspace is in another's way.
   python tools/layered_wide_bench.py [OUT.txt]          LIMITS=1: also 64/64 (128 inputs, both limits) at B = 64"""
import os, subprocess, sys, json, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
#         name                 nx nu  window  hidden        integrator  dtype
CASES = {"rk4_24_6_3x256_f32": (24, 6, 1, [256] * 3, "rk4", "float32"),
         "roll4_6_3_2x128_f64": (6, 3, 4, [128] * 2, "discret", "float64"),
         "40_8_2x256_f64": (40, 8, 1, [256] * 2, "discret", "float64")}
BATCH = {}
if os.environ.get("LIMITS"):
    CASES["64_64_2x256_f64_B64"] = (64, 64, 1, [256] * 2, "discret", "float64")
    BATCH["64_64_2x256_f64_B64"] = 64
if len(sys.argv) < 2 or sys.argv[1] != "--one":
    lines = [f"{'shape':22s} {'callback':5s} {'layered us':>11s} {'generic us':>11s} {'ratio':>6s}   kernels (layered | generic)"]
    for name in CASES:
        got = {}
        for kern in ("layered", "valu"):
            r = subprocess.run([sys.executable, __file__, "--one", name, kern], capture_output=True, text=True, timeout=400)
            if r.returncode != 0 or not r.stdout.strip():
                sys.exit(f"{name}/{kern} failed ({r.returncode}): {r.stderr[-800:]}")
            got[kern] = json.loads(r.stdout.strip().splitlines()[-1])
        for cb, kk in (("eval", "row_kernel"), ("hess", "hess_kernel")):
            lay, gen = got["layered"], got["valu"]
            lines.append(f"{name:22s} {cb:5s} {lay[cb]:11.1f} {gen[cb]:11.1f} {gen[cb] / lay[cb]:6.1f}   {lay[kk]} | {gen[kk]}")
        print("\n".join(lines[-2:]), flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write("\n".join(lines) + "\n")
    sys.exit(0)
sys.path.insert(0, REPO)
import numpy as np, torch
from oracle import nempc_oracle as orc
from pyneuralempc_amd import CallbackEngine
nx, nu, window, hidden, integ, dt = CASES[sys.argv[2]]
kern = sys.argv[3]
B, H = BATCH.get(sys.argv[2], 1024), 20
def timed(fn, reps):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < 0.04:
        fn()
        torch.cuda.synchronize()
    best = 1e9
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps): fn()
        e1.record(); torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / reps)
    return round(best, 1)
net = orc.MLP.random(window * (nx + nu), hidden, nx, seed=0)
eng = CallbackEngine(net.W, net.b, H, nx, nu, integrator=integ, DT=0.1 if integ == "rk4" else 1.0, dtype=getattr(torch, dt),
                     device="cuda:0", max_batch=B, kernel=kern, rolling_window=window)
assert eng.kernel_variant == kern
eng.set_objective(Q=np.eye(nx), R=0.1 * np.eye(nu))
rng = np.random.default_rng(7)
if window > 1:
    eng.bind_history(eng.to_device(rng.normal(size=(B, window - 1, nx))), eng.to_device(rng.uniform(-1, 1, size=(B, window - 1, nu))))
Zh, X0h = orc.synthetic_inputs(B, H, nx, nu, seed=1)
Z, X0 = eng.to_device(Zh), eng.to_device(X0h)
lam, sig = eng.to_device(rng.normal(size=(B, eng.m))), eng.to_device(rng.uniform(0.5, 1.5, size=B))
step, _ = eng.bind(Z, X0, ("f", "grad", "g", "jac_sparse"))
ch, _ = eng.bind_hess(Z, X0, lam, sig)
reps = 10 if kern == "layered" else 1
res = {"eval": timed(step, reps), "row_kernel": eng.last_row_kernel, "hess": timed(ch, reps), "hess_kernel": eng.last_hess_kernel}
print(json.dumps(res))
