#!/usr/bin/env python3
"""The dense contract through the row launch + assembly launch (launch_post) under several builds of the library,
interleaved rounds in one process per build: HIP-event time of an evaluation (f, grad, g, jac_dense) into the engine's own
buffers at configs[1] dims (2/1, H = 20, fp64, B = 1024) for the layered path (2 x 256 tanh) and for kernel="valu"
(2 x 64 tanh), output hashes.   python tools/jac_resident_post_ab.py <libA.so> <libB.so>[@NAME=VALUE] ...   (ROUNDS=3)"""
import os, subprocess, sys, json
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if len(sys.argv) > 1 and sys.argv[1] != "--one":
    for rnd in range(int(os.environ.get("ROUNDS", 3))):
        for lib in sys.argv[1:]:
            path, _, kv = lib.partition("@")
            env = dict(os.environ, **dict([kv.split("=", 1)])) if kv else None
            r = subprocess.run([sys.executable, __file__, "--one", path], capture_output=True, text=True, env=env)
            print(rnd, os.path.basename(lib), r.stdout.strip().splitlines()[-1] if r.stdout.strip() else r.stderr[-600:], flush=True)
    sys.exit(0)
sys.path.insert(0, REPO)
import numpy as np, torch, hashlib
from pyneuralempc_amd import _lib
_lib.LIB_PATH = sys.argv[2]; _lib._lib = None
from oracle import nempc_oracle as orc
from pyneuralempc_amd import CallbackEngine
H, nx, nu, B = 20, 2, 1, 1024
want = ("f", "grad", "g", "jac_dense")
res = {}
for name, hidden, kernel in (("layered_2x256", [256, 256], "auto"), ("valu_2x64", [64, 64], "valu")):
    net = orc.MLP.random(nx + nu, hidden, nx, seed=0)
    eng = CallbackEngine(net.W, net.b, H, nx, nu, dtype=torch.float64, device="cuda:0", max_batch=B, kernel=kernel)
    Z, X0 = orc.synthetic_inputs(B, H, nx, nu, seed=1)
    Z, X0 = eng.to_device(Z), eng.to_device(X0)
    step, outs = eng.bind(Z, X0, want)
    reps = 300
    for _ in range(50): step()
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps): step()
        e1.record(); torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / reps)
    h = hashlib.sha1(b"".join(outs[k].cpu().numpy().tobytes() for k in want)).hexdigest()[:8]
    res[f"{name}:{eng.kernel_variant}"] = (round(best, 3), h)
    del eng
print(json.dumps(res))
