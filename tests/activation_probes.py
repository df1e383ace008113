"""Activation edge probes (helper, no tests): one pre-activation per stage set to an exact double at which the device's
activation code can go wrong -- the kinks, the switches of its range reductions, its clamps, the overflow / underflow of
the hardware exp2 -- and a network that carries that value unchanged into ONE hidden unit and its derivatives unchanged out
of it.

The probe network (Discret, DT = 1, nx = 2, nu = 1): the probe unit `p` of the first hidden layer reads only u, with weight
exactly 1 and bias 0, so its pre-activation at stage (b, t) IS the decision variable u_t; every other unit reads only the
two states.  Deeper variants hand the probe on through a unit-`p`-to-unit-`p` weight of 1 that nothing else touches.  Row
`p` of the output layer is gain * [1, -0.5].  Hence, with one non-linear layer s on the way,
    d g[stage t rows] / d u_t        = gain * [1, -0.5] * s'(z*)                       (the "isolating column")
    d2 L / d u_t d u_t                = sigma * 2 R + gain * (lam_t . [1, -0.5]) * s''(z*)
and nothing else contributes to either: every other term is a product with an exact zero weight.  All weights are multiples
of 2^-10 in about +-1 (exact in fp32), the multipliers multiples of 2^-6, R = 0.25, sigma a multiple of 1/2.

s, s', s'' of the 13 non-linear activations are written out in mpmath at 50 digits (symbolic derivatives; TensorFlow's
conventions at the kinks, as the oracle documents them)."""
import functools

import numpy as np

from oracle import nempc_oracle as orc

NX, NU, B, H, WIDTH = 2, 1, 7, 7, 24          # 49 stages: three 16-row tiles and one ragged row
# -2^32 ln 2 to the nearest integer: the 1.5 * 2^52 shift of the lean exp reduction hands n over as the LOW DWORD of the
# shifted value, so without the clamp at +-1024 n = -2^32 arrives as 0 there and e^z comes out as 0.83 instead of 0 (on this
# side of it, up to |z| = 1100, the hardware ldexp saturates by itself and the clamp changes nothing)
N_WRAP = -2977044472.0
OUT_ROW = np.array([1.0, -0.5])
R_WEIGHT = 0.25

# the probe table.  Why each group is there:
_PROBE_GROUPS = (
    (0.0, -0.0, 2.0 ** -60, -2.0 ** -60, 1e-300, -1e-300),         # the kinks: `a > 0` branches, sign(z), expm1 at n == 0
    (0.17, -0.17, 0.1733, -0.1733, 0.3465, -0.3465, -0.3466),      # n = 0 / +-1 of the exp reduction, ln2 / 4 of the polynomial
    (1.0, -1.0),
    (5.999999, 6.0, 6.000001),                                     # relu6's upper kink
    (9.999, -9.999, 10.001, -10.001),                              # fp32 tanh clamp
    (19.999, -19.999, 20.0, -20.0, 20.001, -20.001),               # fp64 tanh clamp
    (36.7, -36.7, 40.0, -40.0, 88.8, -88.8, 103.0, -103.0),        # e^-z below one ulp of 1; fp32 exp2 overflow / underflow
    (700.0, -700.0, 709.7, -709.7, 745.0, -745.0, 800.0, -800.0, 1024.0, -1024.0, 1100.0, -1100.0),   # fp64 overflow / underflow, the +-1024 clamp
    (N_WRAP,),                                                     # what that clamp is for
)
PROBES = np.array([v for grp in _PROBE_GROUPS for v in grp])
PROBES.setflags(write=False)
SPARE = 0.5                                    # the stages the table does not fill (none at B = H = 7: 49 probes)
EXP_CAP = 40.0                                 # e^800 is infinite: the function's own range (test_oracle makes the same cut)

ACTS = ("tanh", "relu", "sigmoid", "softplus", "elu:0.5", "leaky_relu:0.1", "selu", "swish", "gelu", "softsign", "mish",
        "exponential", "relu6")                # the 13 non-linear activations, the parameterised ones away from their defaults
OUTPUT_BASED = ACTS[:7]
COMPILED = ("tanh", "relu", "sigmoid", "softplus", "elu")      # Act<T, ACT> instantiations of the matrix-core kernels
RUNTIME = ("elu:0.5", "leaky_relu:0.1", "selu")                # run-time codes only


def probes(spec, dtype=np.float64):
    """The probe table of an activation (exponential: capped at +40), rounded to `dtype` and returned as float64"""
    z = PROBES.copy()
    if orc.act_split(spec)[0] == "exponential":
        z = np.minimum(z, EXP_CAP)
    return z.astype(dtype).astype(np.float64)


def _grid(rng, shape):
    return rng.integers(-1024, 1025, size=shape) / 1024.0


def probe_net(acts, p, widths=(WIDTH,), gain=1.0, seed=7):
    """acts: one name per layer, the output layer included.  Unit `p` of every hidden layer is the probe unit."""
    rng = np.random.default_rng(seed)
    dims = [NX + NU] + list(widths) + [NX]
    W = [_grid(rng, (i, o)) for i, o in zip(dims[:-1], dims[1:])]
    b = [_grid(rng, (o,)) for o in dims[1:]]
    W[0][NX:, :] = 0.0                         # nobody but the probe unit reads u ...
    W[0][:, p] = 0.0
    W[0][NX, p] = 1.0                          # ... and it reads nothing else
    b[0][p] = 0.0
    for l in range(1, len(widths)):
        W[l][p, :] = 0.0
        W[l][:, p] = 0.0
        W[l][p, p] = 1.0
        b[l][p] = 0.0
    W[-1][p, :] = gain * OUT_ROW
    return orc.MLP(W, b, list(acts))


@functools.lru_cache(maxsize=None)
def probe_inputs(spec, single=False, nb=B, nh=H):
    """Z, X0, lam, w, sigma of the probe problem (read-only; `single`: rounded to float32 first, so that 1e-300 is 0 and
    19.999 the float it becomes on the device)."""
    dt = np.float32 if single else np.float64
    Z, X0 = orc.synthetic_inputs(nb, nh, NX, NU, seed=11)
    u = np.full(nb * nh, SPARE)
    z = probes(spec, dt)
    assert z.size <= u.size
    u[:z.size] = z
    Z[:, nh * NX:] = u.reshape(nb, nh * NU)
    rng = np.random.default_rng(12)
    lam = rng.integers(-128, 129, size=(nb, nh * NX)) / 64.0
    w = rng.integers(8, 25, size=(nb, nh * NX)) / 16.0           # [0.5, 1.5]
    sigma = rng.integers(1, 4, size=nb) / 2.0
    out = tuple(a.astype(dt).astype(np.float64) for a in (Z, X0, lam, w, sigma))
    for a in out:
        a.setflags(write=False)
    return out


def probe_problem(net, nh=H):
    return orc.Problem(net, nh, NX, NU, orc.DISCRET, 1.0, Q=np.eye(NX), R=np.array([[R_WEIGHT]]))


def stage_of_probe(i, nh=H):
    """(problem, step) of probe i"""
    return divmod(i, nh)


def isolating_column(jac, nh=H):
    """(B, m, n) dense Jacobians -> (B * H, nx): d g[stage rows] / d u_t of every stage"""
    nb = jac.shape[0]
    out = np.empty((nb, nh, NX))
    for t in range(nh):
        out[:, t] = jac[:, t * NX:(t + 1) * NX, nh * NX + t]
    return out.reshape(nb * nh, NX)


def uu_entry(hdense, nh=H):
    """(B, n, n) dense Hessians -> (B * H,): the (u_t, u_t) entry of every stage"""
    nb = hdense.shape[0]
    i = nh * NX + np.arange(nh)
    return hdense[:, i, i].reshape(nb * nh)


def stage_blocks(prob):
    """Per stage t: the variables its Hessian block couples (x_{t-1}, u_t)"""
    out = []
    for t in range(prob.H):
        c = prob.tile_columns(t)
        out.append(c[c >= 0])
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# Closed forms, mpmath at 50 digits
# ---------------------------------------------------------------------------------------------------------------------------
def closed_form(spec, z):
    """(s, s', s'') of activation `spec` at the double z, as mpmath numbers"""
    import mpmath as mp
    mp.mp.dps = 50
    name, par = orc.act_split(spec)
    z = mp.mpf(float(z))
    one, zero = mp.mpf(1), mp.mpf(0)
    g = one / (one + mp.exp(-z))                       # sigmoid
    gg = one / ((one + mp.exp(-z)) * (one + mp.exp(z)))  # g (1 - g) without the cancellation
    if name == "tanh":
        t, c = mp.tanh(z), mp.sech(z) ** 2
        return t, c, -2 * t * c
    if name == "relu":                                 # TensorFlow: gradient 0 at 0
        return (z, one, zero) if z > 0 else (zero, zero, zero)
    if name == "sigmoid":
        return g, gg, -gg * mp.tanh(z / 2)             # 1 - 2 g = -tanh(z / 2)
    if name == "softplus":
        return (z + mp.log1p(mp.exp(-z)) if z > 0 else mp.log1p(mp.exp(z))), g, gg
    if name in ("elu", "selu"):                        # the derivative at 0 is the left one: alpha (la al for selu)
        if name == "elu":
            la, al = one, mp.mpf(par)
        else:                                          # Keras' constants to their full printed length
            la, al = mp.mpf("1.0507009873554804934193349852946"), mp.mpf("1.6732632423543772848170429916717")
        if z > 0:
            return la * z, la, zero
        return la * al * mp.expm1(z), la * al * mp.exp(z), la * al * mp.exp(z)
    if name == "leaky_relu":                           # tf.nn.leaky_relu: alpha at 0
        return (z, one, zero) if z > 0 else (mp.mpf(par) * z, mp.mpf(par), zero)
    if name == "swish":
        return z * g, g + z * gg, gg * (2 - z * mp.tanh(z / 2))
    if name == "gelu":
        Phi = mp.erfc(-z / mp.sqrt(2)) / 2
        phi = mp.exp(-z * z / 2) / mp.sqrt(2 * mp.pi)
        return z * Phi, Phi + z * phi, phi * (2 - z * z)
    if name == "softsign":                             # s''(0) = 0
        r = one / (one + abs(z))
        return z * r, r * r, -2 * mp.sign(z) * r ** 3
    if name == "mish":
        sp = z + mp.log1p(mp.exp(-z)) if z > 0 else mp.log1p(mp.exp(z))
        t = mp.tanh(sp)
        u = mp.sech(sp) ** 2 * g                       # dt / dz
        return z * t, t + z * u, 2 * u + z * u * ((one - g) - 2 * t * g)
    if name == "exponential":
        return mp.exp(z), mp.exp(z), mp.exp(z)
    if name == "relu6":                                # TensorFlow: gradient 0 at 0 and at 6
        if z <= 0:
            return zero, zero, zero
        return (mp.mpf(6), zero, zero) if z >= 6 else (z, one, zero)
    raise ValueError(spec)


def kink_or_saturated(spec, z, tanh_clamp):
    """The probes at which s' is one of the activation's constants by a BRANCH (or, for tanh, by its clamp): +-0, relu6's 6,
    tanh beyond `tanh_clamp`, relu / relu6 at negative z, relu6 above 6."""
    name = orc.act_split(spec)[0]
    m = z == 0.0
    if name == "tanh":
        m = m | (np.abs(z) > tanh_clamp)
    if name in ("relu", "relu6"):
        m = m | (z < 0.0)
    if name == "relu6":
        m = m | (z >= 6.0)
    return m
