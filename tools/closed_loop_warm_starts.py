#!/usr/bin/env python3
"""Closed loop at C2 dims with the MODEL as the plant (x+ = first state of the roll-out of the solved controls), B = 1024,
10 steps, 40 iterations per solve, under three warm starts: the solver's states shifted and clamped into the bounds; the
roll-out of the shifted controls (what NMPC.closed_loop_batch does); the same with the controls clamped.  Prints
(iterations, problems solved) per MPC step to stdout (third part of profiles/r08_rollout.txt)."""
import os, sys, numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import nempc_oracle as orc
from pyneuralempc_amd import CallbackEngine
B, steps, mi, nx, nu, H = 1024, 10, 40, 2, 1, 20
net = orc.MLP.random(nx + nu, [64, 64], nx, seed=0)
eng = CallbackEngine(net.W, net.b, H, nx, nu, dtype=torch.float64, device="cuda:0", max_batch=B)
lb = np.concatenate([np.full(H * nx, -3.0), np.full(H * nu, -0.5)])
X0 = eng.to_device(np.random.default_rng(100).uniform(-0.5, 0.5, size=(B, nx)))
for arm in ("shift+clamp solver states", "rollout warm start", "rollout warm start, controls clamped"):
    X, Zi = X0.clone(), None
    out = []
    for k in range(steps):
        Z, st, it = eng.solve(X, Zi, lb=lb, ub=-lb, max_iter=mi, **({} if Zi is None else {"mu_init": 1e-4}))
        xs, us = Z[:, :H * nx].reshape(B, H, nx).clone(), Z[:, H * nx:].reshape(B, H, nu).clone()
        X = eng.rollout(X, U=us)[:, :nx].clone()            # the true plant
        us2 = torch.cat([us[:, 1:], us[:, -1:]], dim=1)
        if arm.startswith("shift"):
            xs2 = torch.cat([xs[:, 1:], xs[:, -1:]], dim=1).clamp(-2.999, 2.999)
            Zi = torch.cat([xs2.reshape(B, -1), us2.clamp(-0.499, 0.499).reshape(B, -1)], dim=1).contiguous()
        else:
            if arm.endswith("clamped"):
                us2 = us2.clamp(-0.499, 0.499)
            Zi = eng.rollout(X, U=us2.contiguous())
        out.append((it, int((st == 0).sum())))
    print(f"{arm:40s} (iterations, solved of {B}) per step: {out}")
