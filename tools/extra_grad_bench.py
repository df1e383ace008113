#!/usr/bin/env python3
"""nempc_extra_grad beside nempc_weight_grad's first-order call, one nempc_hess call and the same gradient taken by torch
autograd on the device (TorchPhi.S of tests/weight_grad_reference.py differentiated with respect to the extras), all on the
same handle in one session, at the headline shape (2/1, MLP 2 x 64, H = 20, Discret, fp64, B = 1024) and at configs[2] dims
(6/3, MLP 3 x 128, H = 30, RK4, fp32, B = 1024), each with n_extra = 2.

    python tools/extra_grad_bench.py [--reps N] [--rounds 5] [--out profiles/extra_grad.txt]

Per call: HIP-event time over `reps` back-to-back calls after a warm-up, the median of `rounds` such rounds (min and max beside
it).  The one condition: at both shapes nempc_extra_grad takes no longer than nempc_weight_grad's first-order call -- it does a
strict subset of that call's work.  Exit status 1 when it does not hold."""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

NE = 2
SHAPES = {
    "headline": dict(nx=2, nu=1, hidden=[64, 64], H=20, integ="discret", DT=1.0, dt="f64", B=1024),
    "configs2": dict(nx=6, nu=3, hidden=[128, 128, 128], H=30, integ="rk4", DT=0.1, dt="f32", B=1024),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=0, help="calls per round (default: 200 at the headline shape, 20 at configs[2])")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the report to this file")
    args = ap.parse_args()
    import numpy as np
    import torch
    from oracle import nempc_oracle as orc
    from pyneuralempc_amd import CallbackEngine
    import weight_grad_reference as wref
    if not torch.cuda.is_available():
        sys.exit("extra_grad_bench.py measures on the device; there is none")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn, reps):
        """median, min, max over the rounds of the time per call, seconds"""
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e-3 / reps)
        return statistics.median(ts), min(ts), max(ts)

    ok = True
    for name, s in SHAPES.items():
        dt = torch.float64 if s["dt"] == "f64" else torch.float32
        net = orc.MLP.random(s["nx"] + s["nu"] + NE, s["hidden"], s["nx"], seed=0)
        net.W[-1] *= 0.1
        B, H, nx, nu = s["B"], s["H"], s["nx"], s["nu"]
        eng = CallbackEngine(net.W, net.b, H, nx, nu, integrator=s["integ"], DT=s["DT"], dtype=dt, device="cuda:0", max_batch=B,
                             n_extra=NE)
        rng = np.random.default_rng(3)
        Zh, X0h = orc.synthetic_inputs(B, H, nx, nu, seed=1)
        Z, X0 = eng.to_device(Zh), eng.to_device(X0h)
        E = eng.to_device(0.5 * rng.normal(size=(B, H, NE)))
        eng.bind_extra(E)
        lam, v, w = (eng.to_device(rng.normal(size=sh)) for sh in ((B, eng.m), (B, eng.n), (B, H * nx)))
        sig = eng.to_device(np.ones(B))
        e1 = lambda: eng.extra_grad(Z, X0, w)
        e2 = lambda: eng.extra_grad(Z, X0, w, lam=lam, v=v)
        w1 = lambda: eng.weight_grad(Z, X0, w, flat=True)
        hess, _ = eng.bind_hess(Z, X0, lam, sig)
        kind = {"discret": orc.DISCRET, "unity": orc.UNITY, "rk4": orc.RK4}[s["integ"]]
        p = wref.TorchPhi(net, H, nx, nu, kind, s["DT"], dt, device="cuda:0")
        Eg = E.clone().requires_grad_(True)
        ta1 = lambda: torch.autograd.grad(p.S(p.theta0, Z, X0, w, extra=Eg), Eg)
        ta2 = lambda: torch.autograd.grad(p.S(p.theta0, Z, X0, w, lam, v, extra=Eg), Eg)
        g_lib, g_ta = e2(), ta2()[0]
        err = float((g_lib - g_ta).abs().max() / g_ta.abs().max())
        reps = args.reps or (200 if name == "headline" else 20)
        fmt = lambda t: f"{t[0] * 1e6:10.1f} us per call   (min {t[1] * 1e6:.1f}, max {t[2] * 1e6:.1f})"
        te1, te2, tw1, th = timed(e1, reps), timed(e2, reps), timed(w1, reps), timed(hess, reps)
        ta = timed(ta1, max(3, reps // 10)), timed(ta2, max(3, reps // 10))
        say(f"{name} ({nx}/{nu} + {NE} extras, MLP {s['hidden']}, H = {H}, {s['integ']}, {s['dt']}, B = {B}; variant "
            f"{eng.kernel_variant}; {eng.last_extra_grad_kernel}; median of {args.rounds} rounds of {reps} calls)")
        say(f"  nempc_extra_grad, first order (v = lam = NULL)    {fmt(te1)}")
        say(f"  nempc_extra_grad, with lam and v                  {fmt(te2)}")
        say(f"  nempc_weight_grad, first order, same handle       {fmt(tw1)}")
        say(f"  nempc_hess (hvals), same handle                   {fmt(th)}   [{eng.last_hess_kernel}]")
        say(f"  torch autograd on the device, first order         {fmt(ta[0])}   ({ta[0][0] / te1[0]:.1f} x the library)")
        say(f"  torch autograd on the device, with lam and v      {fmt(ta[1])}   ({ta[1][0] / te2[0]:.1f} x the library)")
        say(f"  library against torch: |difference| / max |gE| = {err:.2e}")
        holds = te1[0] <= tw1[0]
        ok = ok and holds
        say(f"  condition (extra_grad first order <= weight_grad first order): {'holds' if holds else 'DOES NOT HOLD'} "
            f"({te1[0] / tw1[0]:.3f} of it)")
        del eng
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
