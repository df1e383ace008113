"""GPU: every place the device evaluates an activation, at the edge probes of tests/activation_probes.py -- saturation
(|z| up to 1100; exponential up to 40), the kinks (+-0, relu6's 6), the switches of the lean exp / tanh reductions and the
clamps of the fp64 and fp32 forms -- in float64 and float32, against the float64 oracle (itself held to 1e-14 of 50-digit
closed forms at the same probes by tests/test_activation_probes_cpu.py).

The probe network isolates one hidden unit: the Jacobian column of u_t in the rows of stage t is [1, -0.5] s'(z*), the
(u_t, u_t) entry of the Lagrangian Hessian is sigma 2 R + (lam_t . [1, -0.5]) s''(z*), g carries s(z*).

Bounds (the project's own, applied so that a large entry cannot hide a small one):
  fp64  elementwise rtol = atol = 1e-12 for g and the Jacobian; rtol 1e-10 / atol 1e-11 for the Lagrangian Hessian;
        rtol 1e-11 / atol 1e-12 for the Gauss-Newton Hessian.
  fp32  reference: the oracle in float64 at the float32-rounded inputs.  Rows 1e-4, Lagrangian Hessian 2e-3, both of
        max(1, |ref|_inf) PER STAGE (a stage: its nx rows of g, its Jacobian rows, its Hessian block) -- one elu probe at 800
        must not loosen the stage next to it.  Gauss-Newton Hessian: 2e-3 per stage as well, which follows from the rows
        bound: a block is sum_k w_k T_k^T T_k over nx = 2 rows with w in [0.5, 1.5], so tile entries within 1e-4 max(1, |T|)
        move it by at most 2 nx w_max 1e-4 |T|^2 = 6e-4 |T|^2, and its own largest entry is at least w_min |T|^2 = |T|^2 / 2.
  exact where the oracle's s' (s'') is exactly 0, 1 or alpha by a branch or by tanh's clamp, the isolating column and the
        (u_t, u_t) entry equal the oracle's as values (one product summed with exact zeros; alpha = 0.5 and [1, -0.5] are
        exact).  A branch taken the wrong way at a == 0 shows here and nowhere else.
No output may hold a NaN or an infinity at any probe.  Every case asserts the kernels it ran on."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import activation_probes as ap
from oracle import nempc_oracle as orc

pytestmark = pytest.mark.gpu

F64 = {"g": dict(rtol=1e-12, atol=1e-12), "jac": dict(rtol=1e-12, atol=1e-12), "hess": dict(rtol=1e-10, atol=1e-11),
       "gn": dict(rtol=1e-11, atol=1e-12)}
F32 = {"g": 1e-4, "jac": 1e-4, "hess": 2e-3, "gn": 2e-3}
DTYPES = [torch.float64, torch.float32]
POSITIONS = [0, ap.WIDTH - 1]              # the first unit, and the last real one next to the padded lanes
TANH_CLAMP = {torch.float64: 20.0, torch.float32: 10.0}


def _ro(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _net(acts, p, widths=(ap.WIDTH,), gain=1.0):
    return ap.probe_net(acts, p, widths, gain)


@functools.lru_cache(maxsize=None)
def _reference(acts, p, spec, single, widths=(ap.WIDTH,), gain=1.0, nb=ap.B, nh=ap.H):
    """The oracle on the probe problem, made once per case and shared read-only"""
    prob = ap.probe_problem(_net(acts, p, widths, gain), nh)
    Z, X0, lam, w, sig = ap.probe_inputs(spec, single, nb, nh)
    with np.errstate(over="ignore"):
        ref = {"g": np.stack([prob.constraints(Z[i], X0[i]) for i in range(nb)]),
               "jac": np.stack([prob.jacobian(Z[i], X0[i]) for i in range(nb)]),
               "hess": np.stack([prob.lagrangian_hessian(Z[i], X0[i], lam[i], sig[i]) for i in range(nb)]),
               "gn": np.stack([prob.gauss_newton_hessian(Z[i], X0[i], w[i], sig[i]) for i in range(nb)])}
    for k, v in ref.items():
        assert np.isfinite(v).all(), (acts, k)       # (the exponential cap guarantees it)
    ref["prob"] = prob
    return _ro(ref)


def _dense(eng, hv):
    rows, cols = eng.hess_structure()
    hd = np.zeros((hv.shape[0], eng.n, eng.n))
    hd[:, rows, cols] = hv
    hd[:, cols, rows] = hv
    return hd


def _device(kernel, acts, p, spec, dtype, widths=(ap.WIDTH,), gain=1.0, nb=ap.B, nh=ap.H, hess=True, sparse=False):
    """One handle on the probe problem: g, dense Jacobian, defect-only g, Lagrangian and Gauss-Newton Hessian values (as
    dense matrices), and the kernels that produced them."""
    from pyneuralempc_amd import CallbackEngine
    net = _net(acts, p, widths, gain)
    eng = CallbackEngine(net.W, net.b, nh, ap.NX, ap.NU, integrator="discret", DT=1.0, dtype=dtype, device="cuda:0", max_batch=nb,
                         kernel=kernel, activations=net.act)
    eng.set_objective(Q=np.eye(ap.NX), R=np.array([[ap.R_WEIGHT]]))
    Z, X0, lam, w, sig = (eng.to_device(a) for a in ap.probe_inputs(spec, dtype == torch.float32, nb, nh))
    f64 = lambda t: t.to("cpu", torch.float64).numpy().copy()
    out = {"variant": eng.kernel_variant}
    res = eng.eval(Z, X0, ("g", "jac_dense"))
    out["g"], out["jac"], out["rows_kernel"] = f64(res["g"]), f64(res["jac_dense"]), eng.last_row_kernel
    out["g_only"], out["g_only_kernel"] = f64(eng.eval(Z, X0, ("g",))["g"]), eng.last_row_kernel
    if sparse:
        out["jac_sparse"], out["sparse_kernel"] = f64(eng.eval(Z, X0, ("g", "jac_sparse"))["jac_sparse"]), eng.last_row_kernel
        out["jac_structure"] = eng.jac_structure()
    if hess:
        out["hess"], out["hess_kernel"] = _dense(eng, f64(eng.hess(Z, X0, lam, sig)["hvals"])), eng.last_hess_kernel
        out["gn"], out["gn_kernel"] = _dense(eng, f64(eng.hess_gn(Z, X0, w, sig)["hvals"])), eng.last_row_kernel
    return out


def _per_stage(a, what, prob):
    """(B, H): the largest |entry| of every stage's part of an output"""
    a = np.abs(a)
    nb, nh = a.shape[0], prob.H
    if what in ("g", "jac"):
        return a.reshape(nb, nh, -1).max(axis=2)
    return np.stack([a[:, c][:, :, c].reshape(nb, -1).max(axis=1) for c in ap.stage_blocks(prob)], axis=1)


def _compare(out, ref, dtype, tag, keys=("g", "jac", "hess", "gn")):
    """The bounds of the module docstring; prints the largest error of each output as a fraction of its bound."""
    prob = ref["prob"]
    keys = [k for k in keys if k in out]
    for k in keys + (["g_only"] if "g_only" in out else []):
        assert np.isfinite(out[k]).all(), f"{tag}: {k} holds a NaN or an infinity"
    report, fails = [], []
    for k in keys:
        for name in ([k, "g_only"] if k == "g" and "g_only" in out else [k]):
            got, want = out[name], ref[k]
            if dtype == torch.float64:
                frac = np.abs(got - want) / (F64[k]["atol"] + F64[k]["rtol"] * np.abs(want))
                report.append(f"{name} {np.abs(got - want).max():.2e} ({frac.max():.2g} of the bound)")
                if frac.max() > 1.0:
                    i = np.unravel_index(np.argmax(frac), frac.shape)
                    fails.append(f"{name}{list(map(int, i))}: {got[i]!r} against {want[i]!r} (rtol {F64[k]['rtol']:.0e}, atol {F64[k]['atol']:.0e})")
            else:
                rel = _per_stage(got - want, k, prob) / np.maximum(1.0, _per_stage(want, k, prob))
                report.append(f"{name} {rel.max():.2e} of max(1, |ref|) per stage (bound {F32[k]:.0e})")
                if rel.max() > F32[k]:
                    b, t = map(int, np.unravel_index(np.argmax(rel), rel.shape))
                    fails.append(f"{name} stage ({b}, {t}): error {rel.max():.3e} of max(1, |ref|_inf) > {F32[k]:.0e}")
    print(f"ACTEDGE {tag}: " + "; ".join(report))
    assert not fails, f"{tag}: " + "; ".join(fails)


def _exact(out, ref, spec, dtype, tag, clamp=None):
    """Kinks and saturation: where the oracle's s' / s'' is exactly 0, 1 or alpha there, so is the device's"""
    single = dtype == torch.float32
    z = ap.probes(spec, np.float32 if single else np.float64)
    with np.errstate(over="ignore"):
        a = orc.act_f(spec, z)
        s1, s2 = orc.act_s1(spec, z, a), orc.act_s2(spec, z, a)
    consts = [0.0, 1.0, orc.act_split(spec)[1]]
    at = ap.kink_or_saturated(spec, z, TANH_CLAMP[dtype] if clamp is None else clamp)
    n = z.size
    m1, m2 = at & np.isin(s1, consts), at & np.isin(s2, consts)
    if orc.act_split(spec)[0] in ("tanh", "relu", "elu", "leaky_relu", "softsign", "exponential", "relu6"):
        assert m1[:2].all() and m2[:2].all(), spec       # (+-0 is such a probe for these)
    # the device holds alpha in its own type: 0.5 is exact, leaky_relu's 0.1 is float32(0.1) there
    c1, c2 = (s1.astype(np.float32).astype(np.float64), s2.astype(np.float32).astype(np.float64)) if single else (s1, s2)
    lam, sig = ap.probe_inputs(spec, single)[2::2]
    lrow = (lam.reshape(-1, ap.NX) @ ap.OUT_ROW)[:n]
    want_col, want_uu = np.outer(c1, ap.OUT_ROW), np.repeat(sig, ap.H)[:n] * 2 * ap.R_WEIGHT + lrow * c2      # (exact products)
    if not single:
        assert np.array_equal(ap.isolating_column(ref["jac"])[:n][m1], want_col[m1])
        assert np.array_equal(ap.uu_entry(ref["hess"])[:n][m2], want_uu[m2])
    col = ap.isolating_column(out["jac"])[:n]
    bad = m1 & (col != want_col).any(axis=1)
    assert not bad.any(), f"{tag}: isolating column at probes {z[bad]}: {col[bad].tolist()} != {want_col[bad].tolist()}"
    if "hess" in out:
        huu = ap.uu_entry(out["hess"])[:n]
        bad = m2 & (huu != want_uu)
        assert not bad.any(), f"{tag}: (u, u) Lagrangian entry at probes {z[bad]}: {huu[bad].tolist()} != {want_uu[bad].tolist()}"
    return int(m1.sum()), int(m2.sum())


def _acts_of(spec, two_layer=False):
    return ("linear", spec, "linear") if two_layer else (spec, "linear")


def _widths_of(two_layer):
    return (ap.WIDTH, ap.WIDTH) if two_layer else (ap.WIDTH,)


# ---------------------------------------------------------------------------------------------------------------------------
# register-resident matrix-core kernels
# ---------------------------------------------------------------------------------------------------------------------------
def _mfma_kernels(kernel, dtype):
    """(rows, defect-only, Lagrangian Hessian) kernels of a one- or two-hidden-layer width-24 network.  n = 21 is not a
    multiple of 4: in fp32 the cooperative kernel has no one-launch dense form there (rows + the assembly launch)."""
    if kernel == "mfma_tile":
        return "rows_mfma_kernel", "rows_mfma_kernel", "rowhess_mfma_kernel"
    return ("rows_coop_kernel+dense" if dtype == torch.float64 else "rows_coop_kernel"), "rows_mfma_kernel", "rowhess_coop_kernel"


def _mfma_case(kernel, spec, two_layer, p, dtype):
    acts, widths = _acts_of(spec, two_layer), _widths_of(two_layer)
    tag = f"{kernel} {'/'.join(acts)} p={p} {str(dtype)[6:]}"
    out = _device(kernel, acts, p, spec, dtype, widths)
    rows_k, g_k, hess_k = _mfma_kernels(kernel, dtype)
    assert out["variant"] == kernel, tag
    assert (out["rows_kernel"], out["g_only_kernel"], out["hess_kernel"]) == (rows_k, g_k, hess_k), (tag, out["rows_kernel"],
                                                                                                   out["g_only_kernel"], out["hess_kernel"])
    assert out["gn_kernel"] in (rows_k, "rows_coop_kernel", "rows_mfma_kernel"), (tag, out["gn_kernel"])
    ref = _reference(acts, p, spec, dtype == torch.float32, widths)
    _compare(out, ref, dtype, tag)
    _exact(out, ref, spec, dtype, tag)
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", POSITIONS)
@pytest.mark.parametrize("act", ap.COMPILED)
def test_matrix_core_kernels_compiled_in_activations(act, p, dtype):
    """Act<T, ACT>: the wave-per-tile family and the cooperative family, which share these formulas by construction and
    therefore also agree with each other to the project's 1e-12 (fp64)."""
    outs = {k: _mfma_case(k, act, False, p, dtype) for k in ("mfma_tile", "mfma")}
    if dtype == torch.float64:
        for k in ("g", "jac", "hess", "gn"):
            np.testing.assert_allclose(outs["mfma"][k], outs["mfma_tile"][k], rtol=1e-12, atol=1e-12, err_msg=f"{act} {k}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", POSITIONS)
@pytest.mark.parametrize("kernel", ["mfma_tile", "mfma"])
@pytest.mark.parametrize("act", ap.RUNTIME)
def test_matrix_core_kernels_run_time_codes(act, kernel, p, dtype):
    """ActL<.., NEMPC_ACT_RUNTIME>: the activations that exist as run-time codes only, with alpha away from 1"""
    _mfma_case(kernel, act, False, p, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kernel", ["mfma_tile", "mfma"])
@pytest.mark.parametrize("act", ap.OUTPUT_BASED)
def test_matrix_core_kernels_run_time_codes_second_layer(act, kernel, dtype):
    """["linear", act, "linear"]: the activation under test at layer index 1 of ActSpec / act_param, the probe handed on
    through a linear first layer; probe unit 23."""
    _mfma_case(kernel, act, True, ap.WIDTH - 1, dtype)


# ---------------------------------------------------------------------------------------------------------------------------
# headline fixed-shape launch: 2/1, 2 x 64 tanh, H = 6
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_headline_fixed_shape_launch(dtype):
    """rows_coopfx_kernel on its compiled shape, the probe in unit 63 of the first tanh layer and handed on to unit 63 of the
    second: g, the dense Jacobian and the band values.  fp32 at n = 18 (not a multiple of 4) gets its dense rows from the
    cooperative kernel's one-launch form; the band values come from the fixed-shape kernel in both types."""
    nb, nh, p, widths, acts = 9, 6, 63, (64, 64), ("tanh", "tanh", "linear")       # 54 stages: three tiles and a ragged one
    tag = f"headline {str(dtype)[6:]}"
    out = _device("mfma", acts, p, "tanh", dtype, widths, nb=nb, nh=nh, hess=False, sparse=True)
    assert out["rows_kernel"] == ("rows_coopfx_kernel" if dtype == torch.float64 else "rows_coop_kernel+dense"), (tag, out["rows_kernel"])
    assert out["sparse_kernel"] == "rows_coopfx_kernel+sparse", (tag, out["sparse_kernel"])
    ref = _reference(acts, p, "tanh", dtype == torch.float32, widths, 1.0, nb, nh)
    _compare(out, ref, dtype, tag)
    rows, cols = out["jac_structure"]
    band, rband = out["jac_sparse"], ref["jac"][:, rows, cols]
    assert np.isfinite(band).all()
    if dtype == torch.float64:
        np.testing.assert_allclose(band, rband, err_msg=f"{tag}: jac_sparse", **F64["jac"])
    else:       # a band value against the largest entry of its own row's stage
        scale = np.maximum(1.0, _per_stage(ref["jac"], "jac", ref["prob"]))[:, rows // ap.NX]
        assert (np.abs(band - rband) / scale).max() <= F32["jac"], tag


# ---------------------------------------------------------------------------------------------------------------------------
# generic kernel
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", ap.ACTS)
def test_generic_kernel(act, dtype):
    """kernel="valu": the library tanh, act_f / act_d1 / act_r2 and act_from_z, all 13 activations"""
    tag = f"valu {act} {str(dtype)[6:]}"
    out = _device("valu", (act, "linear"), ap.WIDTH - 1, act, dtype)
    assert (out["variant"], out["rows_kernel"], out["g_only_kernel"], out["hess_kernel"], out["gn_kernel"]) == \
        ("valu", "rows_valu_kernel", "rows_valu_kernel", "rowhess_valu_kernel", "rows_valu_kernel"), tag
    ref = _reference((act, "linear"), ap.WIDTH - 1, act, dtype == torch.float32)
    _compare(out, ref, dtype, tag)
    _exact(out, ref, act, dtype, tag)


# ---------------------------------------------------------------------------------------------------------------------------
# layered path
# ---------------------------------------------------------------------------------------------------------------------------
# ["tanh", act]: the output layer's pre-activations are G [1, -0.5] tanh(u) + order one.  The defect's derivative with
# respect to the tanh unit's output is G s_out'(z): the oracle's own 1 - a^2 carries an absolute error of 2.2e-16 (one
# rounding of tanh), which that factor multiplies.  G = 16 keeps it at 4e-15 for every activation with |s'| <= 1.05;
# exponential's s' = e^z gets G = 2 (z within about +-6: 2 e^6 2.2e-16 = 2e-13), far below the 1e-12 bar either way.
OUT_GAIN = {"exponential": 2.0}
OUT_GAIN_DEFAULT = 16.0


def _layered_case(acts, p, spec, dtype, gain=1.0, exact=True, hess_kernel="layered_gemm_kernel"):
    tag = f"layered {'/'.join(acts)} p={p} {str(dtype)[6:]}"
    out = _device("layered", acts, p, spec, dtype, gain=gain)
    assert (out["variant"], out["rows_kernel"], out["g_only_kernel"], out["hess_kernel"], out["gn_kernel"]) == \
        ("layered", "layered_gemm_kernel", "layered_gemm_kernel", hess_kernel, "layered_gemm_kernel"), (tag, out["hess_kernel"])
    ref = _reference(acts, p, spec, dtype == torch.float32, (ap.WIDTH,), gain)
    _compare(out, ref, dtype, tag)
    if exact:
        _exact(out, ref, spec, dtype, tag)
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", POSITIONS)
@pytest.mark.parametrize("act", ap.ACTS)
def test_layered_path(act, p, dtype):
    """lg_act_all / lg_act_all_n (and, by default, lg_dval in the Hessian sweeps and the first-layer kernel), all 13"""
    _layered_case((act, "linear"), p, act, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", ap.ACTS)
def test_layered_path_activation_on_the_output_layer(act, dtype):
    """["tanh", act]: the output layer's own epilogue (layered_outfinish_kernel).  The probe saturates the tanh unit, whose
    output row is 16 [1, -0.5]: the output layer sees |z| up to about 16 (exponential: 2 [1, -0.5], see OUT_GAIN).  The
    rows are the layered path's; the Lagrangian blocks of a non-linear output layer behind a single hidden layer are the one
    shape its sweeps do not take (kernels_layered.hip, layered_hess_usable): the handle hands them to the generic kernel."""
    _layered_case(("tanh", act), ap.WIDTH - 1, "tanh", dtype, gain=OUT_GAIN.get(act, OUT_GAIN_DEFAULT), exact=False,
                  hess_kernel="rowhess_valu_kernel")


_DFA_WORKER = r"""
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import numpy as np, torch
import activation_probes as ap
import test_gpu_activation_edges as t
res = {}
for act in ap.OUTPUT_BASED:
    for p in t.POSITIONS:
        for dtype in t.DTYPES:
            out = t._device("layered", (act, "linear"), p, act, dtype)
            for k, v in out.items():
                res[f"{act}|{p}|{str(dtype)[6:]}|{k}"] = np.asarray(v)
np.savez(sys.argv[2], **res)
"""


@pytest.fixture(scope="module")
def dfa_runs(tmp_path_factory):
    """NEMPC_LAYERED_DFA is read once per process: one child process per setting runs every (activation, position, dtype)"""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tmp = tmp_path_factory.mktemp("dfa")
    script = tmp / "worker.py"
    script.write_text(_DFA_WORKER)
    runs = {}
    for dfa in ("0", "2"):
        out = tmp / f"dfa{dfa}.npz"
        r = subprocess.run([sys.executable, str(script), repo, str(out)], env=dict(os.environ, NEMPC_LAYERED_DFA=dfa),
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (dfa, r.stderr[-1500:])
        runs[dfa] = dict(np.load(out))
    return runs


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("p", POSITIONS)
@pytest.mark.parametrize("act", ap.OUTPUT_BASED)
def test_layered_path_derivatives_from_the_stored_activation(dfa_runs, act, p, dtype):
    """NEMPC_LAYERED_DFA = 0 (every layer stores s' and s'': act_d1 / act_r2) and = 2 (none that can form them from its
    activation does, in the rows path too: lg_dval / lg_dval_n, the second copy of the formulas).  Each against the oracle;
    the two share their formulas by construction and agree to the project's 1e-12 in fp64."""
    outs = {}
    for dfa in ("0", "2"):
        pre = f"{act}|{p}|{str(dtype)[6:]}|"
        out = {k[len(pre):]: (v if v.ndim else str(v)) for k, v in dfa_runs[dfa].items() if k.startswith(pre)}
        tag = f"layered DFA={dfa} {act} p={p} {str(dtype)[6:]}"
        assert (out["variant"], out["rows_kernel"], out["hess_kernel"]) == ("layered", "layered_gemm_kernel", "layered_gemm_kernel"), tag
        ref = _reference((act, "linear"), p, act, dtype == torch.float32)
        _compare(out, ref, dtype, tag)
        _exact(out, ref, act, dtype, tag)
        outs[dfa] = out
    if dtype == torch.float64:
        for k in ("g", "jac", "hess", "gn"):
            np.testing.assert_allclose(outs["2"][k], outs["0"][k], rtol=1e-12, atol=1e-12, err_msg=f"{act} {k}: DFA 2 against 0")


# ---------------------------------------------------------------------------------------------------------------------------
# roll-out
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", [1, 2])
@pytest.mark.parametrize("act", ["tanh", "elu:0.5", "swish", "relu6"])
def test_rollout_kernels(which, act, dtype, monkeypatch):
    """nempc_rollout through the probes, one step at a time as test_gpu_rollout does: the oracle's Phi at the device's own
    x_{t-1} (fp64 rtol = atol = 1e-12, fp32 3e-4, that file's bounds).  Both kernels take both activation groups (roll_act):
    two output-based and two z-based activations each."""
    from pyneuralempc_amd import CallbackEngine
    net = _net((act, "linear"), ap.WIDTH - 1)
    prob = ap.probe_problem(net)
    Zh, X0h = ap.probe_inputs(act, dtype == torch.float32)[:2]
    eng = CallbackEngine(net.W, net.b, ap.H, ap.NX, ap.NU, integrator="discret", DT=1.0, dtype=dtype, device="cuda:0", max_batch=ap.B,
                         activations=net.act)
    X0 = eng.to_device(X0h)
    U = eng.to_device(Zh[:, ap.H * ap.NX:].copy())
    monkeypatch.setenv("NEMPC_ROLLOUT_KERNEL", str(which))
    Z = eng.rollout(X0, U).to("cpu", torch.float64).numpy()
    monkeypatch.delenv("NEMPC_ROLLOUT_KERNEL")
    assert eng.last_rollout_kernel == {1: "rollout_wave_kernel", 2: "rollout_mfma_kernel"}[which]
    assert np.array_equal(Z[:, ap.H * ap.NX:], Zh[:, ap.H * ap.NX:])
    tol = dict(rtol=1e-12, atol=1e-12) if dtype == torch.float64 else dict(rtol=3e-4, atol=3e-4)
    worst = 0.0
    for i in range(ap.B):
        with np.errstate(over="ignore"):
            x, phi, _, _ = prob.tiles(Z[i], X0h[i])
        assert np.isfinite(x).all(), (act, which, i)
        worst = max(worst, float((np.abs(x - phi) / (tol["atol"] + tol["rtol"] * np.abs(phi))).max()))
        np.testing.assert_allclose(x, phi, err_msg=f"rollout kernel {which} {act} problem {i}", **tol)
    print(f"ACTEDGE rollout kernel {which} {act} {str(dtype)[6:]}: per-step error {worst:.2g} of the bound, max|x| = {np.abs(Z).max():.3g}")
