"""Reference of nempc_extra_grad: S of include/nempc.h from the torch restatement of tests/weight_grad_reference.py (its
`TorchPhi.S` takes the extras), differentiated with respect to the extras by torch.autograd.grad.  S is a sum over rows and row
(b,t) of the extras enters row (b,t) of S only, so the gradient of the sum IS the per-row gradient gE[b,t,:].  float64 is the
reference; the same code in float32 gives the rounding floor the fp32 device tolerance is measured from.  Also the cases of
the device tests."""
import numpy as np
import torch

from weight_grad_reference import Case, TorchPhi  # noqa: F401  (TorchPhi: re-exported for the tests and the bench)

# the smallest shapes that reach each way the kernel can go wrong (the issue's table)
CASES = {
    "a": Case("a", 2, 1, (8, 8), ("tanh", "tanh", "linear"), "discret", 3, 5, ne=1),
    "b": Case("b", 3, 2, (20, 12), ("tanh", "swish", "softplus"), "unity", 4, 9, ne=2),
    "c": Case("c", 3, 2, (16, 16), ("elu", "sigmoid", "linear"), "rk4", 5, 70, DT=0.1, ne=3),
    "d": Case("d", 2, 1, (144,), ("gelu", "linear"), "discret", 2, 33, ne=5, kernel="layered"),
}

# beyond the table: shapes whose saved activation derivatives leave LDS in float64 (csrc/egrad_plan.h: more than 64 KiB per
# workgroup) and stay in it in float32, one per lane-group size; g has more rows than the capped grid has groups (the
# workgroups walk the rows with a grid stride)
WS_CASES = {
    "e": Case("e", 2, 1, (8, 8), ("tanh", "tanh", "linear"), "rk4", 3, 70, DT=0.1, ne=1),
    "f": Case("f", 3, 2, (64, 64, 64, 64), ("tanh", "sigmoid", "tanh", "softplus", "linear"), "rk4", 2, 9, DT=0.1, ne=2),
    "g": Case("g", 2, 1, (256, 256, 256, 256), ("tanh", "tanh", "tanh", "tanh", "linear"), "rk4", 2, 1100, DT=0.1, ne=2),
}
ALL_CASES = {**CASES, **WS_CASES}

_REF = {}


def S_of_extra(p, d, second=True):
    """-> (callable extra -> S, the extras as a tensor of p's dtype)"""
    Z, X0, w, lam, v = (p.t(d[k]) for k in ("Z", "X0", "w", "lam", "v"))
    if not second:
        lam = v = None
    return (lambda e: p.S(p.theta0, Z, X0, w, lam, v, e)), p.t(d["extra"])


def gE(p, d, second=True):
    """(B,H,ne) numpy float64: dS / d extra with p's dtype"""
    fn, e = S_of_extra(p, d, second)
    e = e.clone().requires_grad_(True)
    with torch.enable_grad():
        (g,) = torch.autograd.grad(fn(e), e)
    return g.detach().to(torch.float64).numpy()


def reference(name):
    """-> dict: g2 (with lam, v), g1 (first order), f32 floors e2_f32 / e1_f32 (the float32 evaluation's error against float64,
    normalised by max |gE|).  Computed once, shared, never modified."""
    if name not in _REF:
        c = ALL_CASES[name]
        d = c.inputs()
        p64, p32 = c.phi(torch.float64), c.phi(torch.float32)
        g2, g1 = gE(p64, d, True), gE(p64, d, False)
        h2, h1 = gE(p32, d, True), gE(p32, d, False)
        for a in (g1, g2):
            a.setflags(write=False)
        _REF[name] = dict(g2=g2, g1=g1, e2_f32=float(np.abs(h2 - g2).max() / np.abs(g2).max()),
                          e1_f32=float(np.abs(h1 - g1).max() / np.abs(g1).max()))
    return _REF[name]
