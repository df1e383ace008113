"""Reference of nempc_weight_grad: a torch restatement of the integrator map Phi, built from the oracle's MLP (weights and
activation names), all three integrators, extras.  S(theta) is formed literally as include/nempc.h writes it,

    S = sum_b keep_b sum_t ( w_{b,t} . Phi_t(xi_{b,t}; theta) + lam_{b,t} . ( T_t(xi_{b,t}; theta) v_{b,[t]} ) ),

with T v from torch.func.jvp, and differentiated with torch.autograd.grad.  float64 is the reference; the same code in
float32 gives the rounding floor the fp32 device tolerance is measured from.  Also the cases of the device tests."""
import math
from dataclasses import dataclass, field

import numpy as np
import torch

from oracle import nempc_oracle as orc


def torch_act(spec, z):
    name, par = orc.act_split(spec)
    if name == "linear":
        return z
    if name == "tanh":
        return torch.tanh(z)
    if name == "relu":
        return torch.relu(z)
    if name == "sigmoid":
        return torch.sigmoid(z)
    if name == "softplus":
        return torch.nn.functional.softplus(z)
    if name == "elu":
        return torch.where(z > 0, z, par * torch.expm1(torch.clamp(z, max=0.0)))
    if name == "leaky_relu":
        return torch.where(z > 0, z, par * z)
    if name == "selu":
        return orc.SELU_LAMBDA * torch.where(z > 0, z, orc.SELU_ALPHA * torch.expm1(torch.clamp(z, max=0.0)))
    if name == "swish":
        return z * torch.sigmoid(z)
    if name == "gelu":
        return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))
    if name == "softsign":
        return z / (1.0 + torch.abs(z))
    if name == "mish":
        return z * torch.tanh(torch.nn.functional.softplus(z))
    if name == "exponential":
        return torch.exp(z)
    if name == "relu6":
        return torch.clamp(z, 0.0, 6.0)
    raise ValueError(name)


class TorchPhi:
    """Phi of an orc.Problem-like shape in torch.  theta: flat list [W_0, b_0, W_1, b_1, ...]."""

    def __init__(self, net, H, nx, nu, kind, DT=1.0, dtype=torch.float64, device="cpu"):
        self.act, self.H, self.nx, self.nu, self.kind, self.DT, self.dtype = list(net.act), H, nx, nu, kind, float(DT), dtype
        self.device = torch.device(device)     # (tools/weight_grad_bench.py times the same formula on the device)
        self.theta0 = []
        for W, b in zip(net.W, net.b):
            self.theta0 += [torch.tensor(W, dtype=dtype, device=self.device), torch.tensor(b, dtype=dtype, device=self.device)]

    def t(self, a):
        return None if a is None else torch.as_tensor(np.asarray(a), dtype=self.dtype, device=self.device)

    def net(self, theta, xi):
        a = xi
        for l, name in enumerate(self.act):
            a = torch_act(name, a @ theta[2 * l] + theta[2 * l + 1])
        return a

    def phi(self, theta, xp, u, extra=None):
        """rows (..., nx), (..., nu) [, (..., ne)] -> Phi (..., nx); u and the extras held over the RK4 stages"""
        def f(x):
            return self.net(theta, torch.cat([x, u] + ([extra] if extra is not None else []), dim=-1))
        if self.kind == orc.UNITY:
            return f(xp)
        if self.kind == orc.DISCRET:
            return xp + f(xp)
        DT = self.DT
        k1 = f(xp)
        k2 = f(xp + 0.5 * DT * k1)
        k3 = f(xp + 0.5 * DT * k2)
        k4 = f(xp + DT * k3)
        return xp + (DT / 6.0) * (k1 + 2.0 * k2 + 2.0 * k3 + k4)

    def rows(self, Z, X0):
        B, H, nx, nu = Z.shape[0], self.H, self.nx, self.nu
        x, u = Z[:, :H * nx].reshape(B, H, nx), Z[:, H * nx:].reshape(B, H, nu)
        return torch.cat([X0[:, None, :], x[:, :-1]], dim=1), u

    def phi_and_tiles(self, theta, Z, X0, extra=None):
        """Phi (B,H,nx) and the tiles (B,H,nx,nx+nu) by autograd (for the check against the oracle)"""
        xp, u = self.rows(Z, X0)
        xu = torch.cat([xp, u], dim=-1).reshape(-1, self.nx + self.nu)
        ex = None if extra is None else extra.reshape(xu.shape[0], -1)

        def one(r, e):
            return self.phi(theta, r[:self.nx], r[self.nx:], e)
        if ex is None:
            T = torch.func.vmap(torch.func.jacfwd(lambda r: one(r, None)))(xu)
        else:
            T = torch.func.vmap(torch.func.jacfwd(one, argnums=0))(xu, ex)
        return self.phi(theta, xp, u, extra), T.reshape(Z.shape[0], self.H, self.nx, self.nx + self.nu)

    def S(self, theta, Z, X0, w, lam=None, v=None, extra=None, keep=None):
        B, H, nx, nu = Z.shape[0], self.H, self.nx, self.nu
        xp, u = self.rows(Z, X0)
        wr = w.reshape(B, H, nx)
        km = torch.ones(B, dtype=self.dtype, device=self.device) if keep is None else torch.as_tensor(keep, dtype=self.dtype, device=self.device)
        if v is None:
            return (km[:, None, None] * wr * self.phi(theta, xp, u, extra)).sum()
        vx, vu = v[:, :H * nx].reshape(B, H, nx), v[:, H * nx:].reshape(B, H, nu)
        vxp = torch.cat([torch.zeros(B, 1, nx, dtype=self.dtype, device=self.device), vx[:, :-1]], dim=1)       # v_x[-1] = 0
        Phi, Tv = torch.func.jvp(lambda a, b: self.phi(theta, a, b, extra), (xp, u), (vxp, vu))
        lr = lam[:, :H * nx].reshape(B, H, nx)                                               # (box-row entries are not read)
        return (km[:, None, None] * (wr * Phi + lr * Tv)).sum()

    def gtheta(self, Z, X0, w, lam=None, v=None, extra=None, keep=None, theta=None):
        """flat gtheta (P,) as numpy float64, layout [W_0 | b_0 | W_1 | b_1 | ...]; NaN rows of a dropped problem are cut out"""
        theta = [t.clone().requires_grad_(True) for t in (self.theta0 if theta is None else theta)]
        args = [self.t(a) for a in (Z, X0, w, lam, v, extra)]
        if keep is not None:
            sel = torch.as_tensor(np.asarray(keep) != 0)
            args = [None if a is None else a[sel] for a in args]
        Zt, X0t, wt, lt, vt, et = args
        with torch.enable_grad():            # (callers may sit inside an autograd Function's backward)
            g = torch.autograd.grad(self.S(theta, Zt, X0t, wt, lt, vt, et), theta)
        return np.concatenate([x.detach().to(torch.float64).numpy().ravel() for x in g])


@dataclass
class Case:
    name: str
    nx: int
    nu: int
    hidden: tuple
    acts: tuple            # per layer, the output layer included
    integ: str
    H: int
    B: int
    DT: float = 1.0
    ne: int = 0
    kernel: str = "auto"
    seed: int = 0
    data: dict = field(default_factory=dict)

    @property
    def kind(self):
        return {"discret": orc.DISCRET, "unity": orc.UNITY, "rk4": orc.RK4}[self.integ]

    @property
    def n(self):
        return self.H * (self.nx + self.nu)

    def net(self):
        return orc.MLP.random(self.nx + self.nu + self.ne, list(self.hidden), self.nx, seed=self.seed, activations=list(self.acts))

    def inputs(self):
        """seeded normal Z, X0, lam, v, w (and extras) of unit scale, float64 numpy"""
        if not self.data:
            rng = np.random.default_rng(100 + self.seed)
            d = dict(Z=rng.normal(size=(self.B, self.n)), X0=rng.normal(size=(self.B, self.nx)),
                     lam=rng.normal(size=(self.B, self.H * self.nx)), v=rng.normal(size=(self.B, self.n)),
                     w=rng.normal(size=(self.B, self.H * self.nx)))
            d["extra"] = rng.normal(size=(self.B, self.H, self.ne)) if self.ne else None
            self.data = d
        return self.data

    def phi(self, dtype=torch.float64):
        return TorchPhi(self.net(), self.H, self.nx, self.nu, self.kind, self.DT, dtype)

    def problem(self, b):
        ex = self.inputs()["extra"]
        return orc.Problem(self.net(), self.H, self.nx, self.nu, self.kind, self.DT, extra=None if ex is None else ex[b])


# the smallest shapes that reach each way the kernels can go wrong (the issue's table)
CASES = {
    "a": Case("a", 2, 1, (8, 8), ("tanh", "tanh", "linear"), "discret", 3, 5),
    "b": Case("b", 3, 2, (20, 12), ("tanh", "swish", "softplus"), "unity", 4, 9, ne=2),
    "c": Case("c", 3, 2, (16, 16), ("elu", "sigmoid", "linear"), "rk4", 5, 70, DT=0.1),
    "d": Case("d", 2, 1, (144,), ("gelu", "linear"), "discret", 2, 33, kernel="layered"),
    "e": Case("e", 2, 1, (8, 8), ("tanh", "tanh", "linear"), "discret", 3, 5, kernel="mfma"),
}

_REF = {}


def reference(name):
    """-> dict: g2 (with lam, v), g1 (first order), f32 floors e2_f32 / e1_f32 (the float32 evaluation's error against float64,
    normalised by max |gtheta|).  Computed once, shared, never modified."""
    if name not in _REF:
        c = CASES[name]
        d = c.inputs()
        p64, p32 = c.phi(torch.float64), c.phi(torch.float32)
        g2 = p64.gtheta(d["Z"], d["X0"], d["w"], d["lam"], d["v"], d["extra"])
        g1 = p64.gtheta(d["Z"], d["X0"], d["w"], None, None, d["extra"])
        h2 = p32.gtheta(d["Z"], d["X0"], d["w"], d["lam"], d["v"], d["extra"])
        h1 = p32.gtheta(d["Z"], d["X0"], d["w"], None, None, d["extra"])
        for a in (g1, g2):
            a.setflags(write=False)
        _REF[name] = dict(g2=g2, g1=g1, e2_f32=float(np.abs(h2 - g2).max() / np.abs(g2).max()),
                          e1_f32=float(np.abs(h1 - g1).max() / np.abs(g1).max()))
    return _REF[name]
