#!/usr/bin/env python3
"""nempc_weight_grad beside one nempc_hess call on the same handle, and beside the same gradient taken by torch autograd on
the device from a batched torch restatement of Phi (tests/weight_grad_reference.py), at the headline shape (2/1, MLP 2 x 64,
H = 20, Discret, fp64, B = 1024) and at configs[2] dims (6/3, MLP 3 x 128, H = 30, RK4, fp32, B = 1024).

    python tools/weight_grad_bench.py                      HIP-event times per call (warm, many repetitions), results compared
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/weight_grad_bench.py --profile
                                                           a run of its own: the library's calls only, for the kernel times
    python tools/weight_grad_bench.py --stats DIR/.../*_kernel_stats.csv
                                                           the accumulation GEMM's achieved share of the matrix peak and of HBM
                                                           bandwidth from those kernel times and the shapes (no device needed)

Work of the accumulation per layer: 2 * pairs * factor_rows * (in + 1) * out flop and pairs * factor_rows * (in + 1 + out)
elements read (pairs = 2 with lam / v, else 1; factor rows = B * H * stages), plus the slabs written and read back once."""
import argparse
import csv
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]

PEAK_TF = {"f64": 78.6, "f32": 157.3}       # v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32 at 2.4 GHz x 1024 SIMDs
HBM_TBS = 8.0                               # spec; about 6.3 achievable
PROFILE_CALLS = 10                          # calls of each kind per shape in the --profile leg
SHAPES = {
    "headline": dict(nx=2, nu=1, hidden=[64, 64], H=20, integ="discret", DT=1.0, dt="f64", B=1024),
    "configs2": dict(nx=6, nu=3, hidden=[128, 128, 128], H=30, integ="rk4", DT=0.1, dt="f32", B=1024),
}


def gemm_work(s, pairs):
    dims = [s["nx"] + s["nu"]] + s["hidden"] + [s["nx"]]
    frows = s["B"] * s["H"] * (4 if s["integ"] == "rk4" else 1)
    esz = 8 if s["dt"] == "f64" else 4
    flop = sum(2.0 * pairs * frows * (i + 1) * o for i, o in zip(dims[:-1], dims[1:]))
    byts = sum(pairs * frows * (i + 1 + o) * esz for i, o in zip(dims[:-1], dims[1:]))
    return flop, byts


def from_stats(path):
    rows = list(csv.DictReader(open(path)))
    for r in rows:
        name = r.get("Name") or r.get("KernelName") or ""
        if "wgrad_" in name or "rowhess" in name or "layered" in name:
            print(f"{name[:90]:90s} calls {r.get('Calls')} avg {float(r.get('AverageNs', 0)) / 1e3:9.1f} us")
    for r in rows:
        name = r.get("Name") or r.get("KernelName") or ""
        if "wgrad_gemm_kernel" not in name:
            continue
        dt = "f64" if "<double>" in name or "IdE" in name else "f32"
        s = next(v for v in SHAPES.values() if v["dt"] == dt)
        # the profile leg makes PROFILE_CALLS first-order and as many second-order calls per shape; a call launches the kernel
        # once per chunk of rows, so the time per call is the total over the calls, and the work is the mean of the two kinds
        t = float(r["TotalDurationNs"]) * 1e-9 / (2 * PROFILE_CALLS)
        flop = 0.5 * (gemm_work(s, 1)[0] + gemm_work(s, 2)[0])
        byts = 0.5 * (gemm_work(s, 1)[1] + gemm_work(s, 2)[1])
        print(f"wgrad_gemm_kernel {dt}: {int(r['Calls']) / (2 * PROFILE_CALLS):.0f} launch(es) and {t * 1e6:.1f} us per call (mean of first order and "
              f"with v), {flop / t / 1e12:.2f} TFLOP/s = {flop / t / 1e12 / PEAK_TF[dt]:.3f} of the {dt} matrix peak, "
              f"{byts / t / 1e12:.2f} TB/s = {byts / t / 1e12 / HBM_TBS:.3f} of HBM spec")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--profile", action="store_true", help="library calls only, few repetitions (run under rocprofv3)")
    ap.add_argument("--stats", help="kernel_stats.csv of such a run: shares of peak of the accumulation GEMM")
    args = ap.parse_args()
    if args.stats:
        return from_stats(args.stats)
    import numpy as np
    import torch
    from oracle import nempc_oracle as orc
    from pyneuralempc_amd import CallbackEngine
    import weight_grad_reference as wref
    if not torch.cuda.is_available():
        sys.exit("weight_grad_bench.py measures on the device; there is none")

    def timed(fn, reps):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / reps

    for name, s in SHAPES.items():
        dt = torch.float64 if s["dt"] == "f64" else torch.float32
        net = orc.MLP.random(s["nx"] + s["nu"], s["hidden"], s["nx"], seed=0)
        net.W[-1] *= 0.1
        B, H, nx, nu = s["B"], s["H"], s["nx"], s["nu"]
        eng = CallbackEngine(net.W, net.b, H, nx, nu, integrator=s["integ"], DT=s["DT"], dtype=dt, device="cuda:0", max_batch=B)
        rng = np.random.default_rng(3)
        Zh, X0h = orc.synthetic_inputs(B, H, nx, nu, seed=1)
        Z, X0 = eng.to_device(Zh), eng.to_device(X0h)
        lam, v, w = (eng.to_device(rng.normal(size=sh)) for sh in ((B, eng.m), (B, eng.n), (B, H * nx)))
        sig = eng.to_device(np.ones(B))
        first = lambda: eng.weight_grad(Z, X0, w, flat=True)
        second = lambda: eng.weight_grad(Z, X0, w, lam=lam, v=v, flat=True)
        hess, _ = eng.bind_hess(Z, X0, lam, sig)
        if args.profile:
            for _ in range(PROFILE_CALLS):
                first(); second(); hess()
            torch.cuda.synchronize()
            continue
        kind = {"discret": orc.DISCRET, "unity": orc.UNITY, "rk4": orc.RK4}[s["integ"]]
        p = wref.TorchPhi(net, H, nx, nu, kind, s["DT"], dt, device="cuda:0")
        theta = [t.clone().requires_grad_(True) for t in p.theta0]
        ta1 = lambda: torch.autograd.grad(p.S(theta, Z, X0, w), theta)
        ta2 = lambda: torch.autograd.grad(p.S(theta, Z, X0, w, lam, v), theta)
        g_lib, g_ta = second(), torch.cat([x.reshape(-1) for x in ta2()])
        err = float((g_lib - g_ta).abs().max() / g_ta.abs().max())
        reps = 200 if name == "headline" else 20
        t1, t2, th = timed(first, reps), timed(second, reps), timed(hess, reps)
        a1, a2 = timed(ta1, max(3, reps // 10)), timed(ta2, max(3, reps // 10))
        f1, b1 = gemm_work(s, 1)
        f2, b2 = gemm_work(s, 2)
        print(f"{name} ({nx}/{nu}, MLP {s['hidden']}, H = {H}, {s['integ']}, {s['dt']}, B = {B}; {eng.n_params} parameters; "
              f"variant {eng.kernel_variant})")
        print(f"  nempc_weight_grad, first order (v = lam = NULL)   {t1 * 1e6:10.1f} us per call")
        print(f"  nempc_weight_grad, with lam and v                 {t2 * 1e6:10.1f} us per call")
        print(f"  nempc_hess (hvals), same handle                   {th * 1e6:10.1f} us per call   [{eng.last_hess_kernel}]")
        print(f"  torch autograd on the device, first order         {a1 * 1e6:10.1f} us per call   ({a1 / t1:.1f} x the library)")
        print(f"  torch autograd on the device, with lam and v      {a2 * 1e6:10.1f} us per call   ({a2 / t2:.1f} x the library)")
        print(f"  library against torch: |difference| / max |gtheta| = {err:.2e}")
        print(f"  accumulation work: first order {f1 / 1e9:.2f} GFLOP / {b1 / 1e6:.1f} MB, with v {f2 / 1e9:.2f} GFLOP / {b2 / 1e6:.1f} MB "
              f"(least time at peak: {max(f2 / PEAK_TF[s['dt']] / 1e12, b2 / HBM_TBS / 1e12) * 1e6:.1f} us; kernel times: --profile run)",
              flush=True)
        del eng


if __name__ == "__main__":
    main()
