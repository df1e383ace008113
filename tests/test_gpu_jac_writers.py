"""Every writer of the dense Jacobian, into buffers the CALLER owns.

The engine's own jac_dense is a resident buffer: evaluations into it run the writers that store the structural non-zeros only
(post_scatter_kernel, the null-background form of the fused launch).  A C ABI caller, an `out=` user and the configs[4] ring
of bench.py get the full-matrix writers instead -- post_flat_kernel, post_kernel, assemble_dense_kernel, the background-zero
form of the fused launch, rows_coop_kernel+dense.  This module holds those against the references, case by case.

Every dense output that is not the engine's own is a view into a larger 1-D tensor, [lead guard | B*m*n body | tail guard]:
the guards (>= 64 elements each) hold a finite sentinel and are compared bit for bit afterwards, the body starts as NaN.
`lead` a multiple of 16 bytes keeps the matrix 16-byte aligned; one element more (fp32: one, two, three) gives an
element-aligned pointer that no 16-byte vector store may be aimed at.  Wherever a dense matrix is written:
  (i)   no NaN is left and the guards are intact;
  (ii)  it equals the reference at the project's bars (fp64 rtol = atol = 1e-12, fp32 test_gpu_parity._f32_close);
  (iii) jac != 0 has the reference's pattern: structural zeros are exact;
  (iv)  it is bit-equal to the same handle's evaluation into its own resident buffer at the same iterate and `want`, and
        last_row_kernel is the same on both sides (the resident flag must not change the row kernel);
  (v)   last_dense_writer is the expected one.  For the assembly launches the expectation comes from tests/post_plan_rule.py,
        a Python restatement of csrc/post_plan.h that test_post_plan_cpu.py checks against the header's stand-alone program.

(a) the goldens of test_gpu_parity (its fp64 and fp32 lists, imported) plus the same names under kernel="auto", and the
    rolling-window goldens; DEFAULT, ("g", "jac_dense") and ALL.
(b) seeded shapes of the fixed-shape launch the goldens do not hold: 3 -> 30 -> 30 -> 2 in both precisions, 2 x 64 in fp32 at
    n = 60, B = 7 and 33.
(c) the assembly arms on kernel="valu" with a 1 x 8 tanh network: flat stream, per-problem grid through a misaligned lead,
    scatter -- all bit-equal to each other; m*n = 6 at B = 700, 294, the odd 735, 2400 (plain, box rows, tracking bound),
    65 280 (refused by the reciprocal's error bound in both precisions) and 64 000 (10/6 at H = 20: the largest m*n of any
    nx, nu <= 16, H <= 64, with or without box rows, that is a multiple of 4 and below the first refusal, 64 060).
B*m*n >= 2^32 needs tens of GB of output: that limit stays with the CPU check (tests/post_plan_check.cpp).

Wall time on an MI355X: 10.7 s for the 365 cases of this module run alone (the slowest, a c1 golden on the generic kernel,
0.7 s); the whole GPU suite with it 218 s for 1702 tests, so about 208 s for the 1337 tests it had before."""
import functools

import numpy as np
import pytest
import torch

from oracle import nempc_oracle as orc
from helpers import ROLLING_NAMES, load_case
import post_plan_rule as rule
import test_gpu_parity as par
import test_gpu_rolling as rol
from test_gpu_fx_prologue_tail import _NET as NET_2X64

pytestmark = pytest.mark.gpu

DEFAULT = ("f", "grad", "g", "jac_dense")
GJ = ("g", "jac_dense")
ALL = par.ALL
GUARD = 64                     # elements of each guard (the aligned lead: 512 bytes in fp64, 256 in fp32)
SENTINEL = -12345.6875         # finite, exact in fp32
DTYPES = {"fp64": torch.float64, "fp32": torch.float32}
# the fp32 list of test_gpu_parity: the cases its test_golden_fp32 is parametrised over
_FP32_CASES = list(next(m for m in par.test_golden_fp32.pytestmark if m.name == "parametrize").args[1])


@pytest.fixture(scope="module", autouse=True)
def _drop_handles_afterwards():
    yield
    for cached in (_golden_engine, _rolling_engine, _seeded_engine, _arm):
        cached.cache_clear()


# ------------------------------------------------------------------ the guarded buffer and the five properties
class Guarded:
    """[lead guard | B*m*n body | tail guard] in one 1-D tensor; .view is the contiguous (B, m, n) body."""

    def __init__(self, eng, B, extra_lead):
        self.lead, self.count = GUARD + extra_lead, B * eng.m * eng.n
        self.raw = torch.full((self.lead + self.count + GUARD,), SENTINEL, dtype=eng.dtype, device=eng.device)
        assert self.raw.data_ptr() % 16 == 0
        body = self.raw[self.lead:self.lead + self.count]
        body.fill_(float("nan"))
        self.view = body.view(B, eng.m, eng.n)
        assert self.view.is_contiguous() and self.view.data_ptr() == self.raw.data_ptr() + self.lead * self.raw.element_size()

    def guards_intact(self):
        lead, tail = self.raw[:self.lead], self.raw[self.lead + self.count:]
        return bool(torch.equal(lead, torch.full_like(lead, SENTINEL)) and torch.equal(tail, torch.full_like(tail, SENTINEL)))


def _shapes(eng, B):
    return {"f": (B,), "grad": (B, eng.n), "g": (B, eng.m), "jac_dense": (B, eng.m, eng.n),
            "jac_tiles": (B, eng.H, eng.nx, eng.nin), "jac_sparse": (B, eng.nnz_jac)}


def _own(eng, Z, X0, want):
    """Into the engine's own (resident) buffers.  -> clones, row kernel, dense writer"""
    res = eng.eval(Z, X0, want)
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in res.items()}, eng.last_row_kernel, eng.last_dense_writer


def _guarded(eng, Z, X0, want, extra_lead):
    """Into caller-owned outputs full of NaN, the dense matrix behind `GUARD + extra_lead` elements of guard."""
    B = Z.shape[0]
    sh = _shapes(eng, B)
    gb = Guarded(eng, B, extra_lead)
    out = {k: torch.full(sh[k], float("nan"), dtype=eng.dtype, device=Z.device) for k in want if k != "jac_dense"}
    out["jac_dense"] = gb.view
    res = eng.eval(Z, X0, want, out=out)
    torch.cuda.synchronize()
    assert res["jac_dense"].data_ptr() == gb.view.data_ptr()
    return res, gb, eng.last_row_kernel, eng.last_dense_writer


def _expected_writer(eng, want, row_kernel, B, ptr, objective):
    """The dense writer of an evaluation into a caller-owned matrix at `ptr` whose row kernel was `row_kernel`."""
    esz = 8 if eng.dtype == torch.float64 else 4
    if eng.kernel_variant == "mfma" and "jac_sparse" not in want:
        if row_kernel == "rows_coop_kernel+dense":
            return "row_launch"
        # the fused fixed-shape launch writes whole 16-byte vectors of a row: it declines other n and other pointers, and
        # the same kernel then runs as the plain row launch in front of an assembly launch
        if row_kernel == "rows_coopfx_kernel" and eng.n % (16 // esz) == 0 and ptr % 16 == 0:
            return "row_launch"
    return rule.assembly_writer(eng.m * eng.n, B, esz, ptr, False, objective)


def _hold(got, ref, dtype, what):
    got = got.cpu().numpy().astype(np.float64)
    if dtype == torch.float64:
        np.testing.assert_allclose(got, ref, err_msg=what, **par.F64)
    else:
        par._f32_close(got, ref, what)


def _check(eng, Zh, X0h, want, refs, what, leads=(0,), tracking=False, resident_side=True, seen=None):
    """Properties (i) to (v) of one handle at one iterate for every lead in `leads` (extra elements on top of the aligned
    guard), all the dense matrices bit-equal to each other.  refs: {"f", "grad", "g", "jac_dense"} -> float64 arrays.
    -> {lead: writer name}, "own" for the engine's buffer"""
    Z, X0 = eng.to_device(Zh), eng.to_device(X0h)
    B = Z.shape[0]
    objective = ("f" in want or "grad" in want) and not tracking
    writers = {}
    own = None
    if resident_side:
        own, k_own, w_own = _own(eng, Z, X0, want)
        writers["own"] = w_own
    for lead in leads:
        res, gb, k_out, w_out = _guarded(eng, Z, X0, want, lead)
        tag = f"{what} want={'+'.join(want)} lead={lead}"
        print(f"{tag}: row kernel {k_out}, dense writer {w_out}" + (f" (own buffer: {w_own})" if own is not None else ""))
        # (i)
        for k in want:
            assert int(torch.isnan(res[k]).sum()) == 0, (tag, k)
        assert gb.guards_intact(), tag
        # (ii)
        for k in want:
            if k in refs:
                _hold(res[k], refs[k], eng.dtype, f"{tag} {k}")
        # (iii)
        jac = res["jac_dense"].cpu().numpy()
        assert np.array_equal(jac != 0, refs["jac_dense"] != 0), tag
        if "jac_sparse" in want:
            rows, cols = eng.jac_structure()
            assert np.array_equal(res["jac_sparse"].cpu().numpy(), jac[:, rows, cols]), tag
        # (v)
        expect = _expected_writer(eng, want, k_out, B, gb.view.data_ptr(), objective)
        assert w_out == expect, (tag, w_out, expect)
        writers[lead] = w_out
        # (iv)
        if own is not None:
            assert k_own == k_out, (tag, k_own, k_out)
            assert w_own == ("row_launch" if expect == "row_launch" else "post_scatter_kernel"), (tag, w_own)
            for k in want:
                assert torch.equal(res[k], own[k]), (tag, k)
        # every pair of writers on this handle and iterate: the same bits
        if lead != leads[0]:
            assert torch.equal(res["jac_dense"], first), (tag, "differs from lead", leads[0])
        else:
            first = res["jac_dense"].clone()
    if seen is not None:
        seen.update((str(eng.dtype), w) for w in writers.values())
    return writers


# ------------------------------------------------------------------ (a) the golden matrix
@functools.lru_cache(maxsize=None)
def _golden_engine(name, kernel, dtype):
    d, W, b = load_case(name)
    return par._engine(d, W, b, DTYPES[dtype], kernel), d


@functools.lru_cache(maxsize=None)
def _rolling_engine(name, kernel, dtype):
    d, W, b = load_case(name)
    return rol._engine(d, W, b, DTYPES[dtype], kernel), d


def _with_auto(cases):
    return list(cases) + [(n, "auto") for n in dict.fromkeys(n for n, _ in cases)]


def _golden(eng, d, what):
    refs = {"f": d["f"], "grad": d["grad"], "g": d["g"], "jac_dense": d["jac"]}
    for want in (DEFAULT, GJ, ALL):
        _check(eng, d["Z"], d["X0"], want, refs, what)


@pytest.mark.parametrize("name,kernel", _with_auto(par._FP64_CASES))
def test_golden_fp64_into_a_caller_owned_buffer(name, kernel):
    eng, d = _golden_engine(name, kernel, "fp64")
    assert kernel == "auto" or eng.kernel_variant == kernel
    _golden(eng, d, f"{name}/{kernel}/fp64")


@pytest.mark.parametrize("name,kernel", _with_auto(_FP32_CASES))
def test_golden_fp32_into_a_caller_owned_buffer(name, kernel):
    eng, d = _golden_engine(name, kernel, "fp32")
    _golden(eng, d, f"{name}/{kernel}/fp32")


def _rolling_cases(names):
    return [(n, k) for n in names for k in rol._kernels(load_case(n)[0]) + ["auto"]]


@pytest.mark.parametrize("name,kernel", _rolling_cases(ROLLING_NAMES))
def test_rolling_golden_fp64_into_a_caller_owned_buffer(name, kernel):
    eng, d = _rolling_engine(name, kernel, "fp64")
    _golden(eng, d, f"{name}/{kernel}/fp64")


@pytest.mark.parametrize("name,kernel", _rolling_cases(["roll2_discret", "roll3_unity_rev", "roll4_wide"]))
def test_rolling_golden_fp32_into_a_caller_owned_buffer(name, kernel):
    eng, d = _rolling_engine(name, kernel, "fp32")
    _golden(eng, d, f"{name}/{kernel}/fp32")


# ------------------------------------------------------------------ (b) compiled shapes the goldens do not hold
_NET_2X30 = orc.MLP.random(3, [30, 30], 2, seed=21)          # the reference's example network shape: padded width 32
_SEEDED_NETS = {"2x30": _NET_2X30, "2x64": NET_2X64}


def _objective(H, nx, nu, seed=5):
    rng = np.random.default_rng(seed)
    return dict(Q=np.eye(nx) + 0.1 * rng.normal(size=(nx, nx)), R=0.3 * np.eye(nu) + 0.05 * rng.normal(size=(nu, nu)),
                xref=0.5 * rng.normal(size=(H, nx)), uref=0.2 * rng.normal(size=(H, nu)), cx=0.1 * rng.normal(size=(H, nx)),
                cu=0.1 * rng.normal(size=(H, nu)))


@functools.lru_cache(maxsize=None)
def _seeded_engine(net, dtype, H, B, kernel="auto"):
    from pyneuralempc_amd import CallbackEngine
    n = _SEEDED_NETS[net]
    eng = CallbackEngine(n.W, n.b, H, 2, 1, dtype=DTYPES[dtype], device="cuda:0", max_batch=B, kernel=kernel)
    ob = _objective(H, 2, 1)
    eng.set_objective(**ob)
    Zh, X0h = orc.synthetic_inputs(B, H, 2, 1, seed=31 + B)
    f, grad, g, J = orc.Problem(n, H, 2, 1, orc.DISCRET, **ob).eval_batch(Zh, X0h)
    return eng, Zh, X0h, {"f": f, "grad": grad, "g": g, "jac_dense": J}


@pytest.mark.parametrize("B", [7, 33])
@pytest.mark.parametrize("net,dtype", [("2x30", "fp64"), ("2x30", "fp32"), ("2x64", "fp32")])
def test_fixed_shape_launch_on_shapes_the_goldens_do_not_hold(net, dtype, B):
    """H = 20 (n = 60: whole vectors in both precisions), B*H = 140 and 660 rows: the fused launch with its background zeros
    (caller's buffer) and without (the engine's), bit-equal."""
    eng, Zh, X0h, refs = _seeded_engine(net, dtype, 20, B)
    for want in (DEFAULT, GJ):
        w = _check(eng, Zh, X0h, want, refs, f"{net}/{dtype}/B={B}")
        assert eng.last_row_kernel == "rows_coopfx_kernel"
        assert w == {"own": "row_launch", 0: "row_launch"}


# ------------------------------------------------------------------ (c) the assembly arms
# name -> (nx, nu, H, B, box, tracking); m*n in the comment
_ARMS = {
    "h1_b700": (2, 1, 1, 700, None, False),           # 6: fp64 flat, 341 problems per block, ragged last block; fp32 6 % 4 != 0
    "h7": (2, 1, 7, 5, None, False),                  # 294: fp64 flat, fp32 per-problem
    "odd_735": (3, 2, 7, 3, None, False),             # 21 x 35 = 735: per-problem in both, odd problems start off a 16-byte boundary
    "h20": (2, 1, 20, 5, None, False),                # 40 x 60 = 2400: 1.17 blocks in fp64
    "h20_box": (2, 1, 20, 5, (-2.0, 2.0), False),     # 80 x 60
    "h20_tracking": (2, 1, 20, 5, None, True),        # f / grad from objective_tracking_kernel: the writers get no objective
    "refused_65280": (15, 2, 16, 2, None, False),     # 240 x 272 = 65 280: past the error bound in both precisions
    "admitted_64000": (10, 6, 20, 2, None, False),    # 200 x 320 = 64 000: the last reachable multiple of 4 before it
}
ADMITTED_MN, REFUSED_MN = 64000, 65280


def _arm_net(nx, nu):
    net = orc.MLP.random(nx + nu, [8], nx, seed=17)
    return net


@functools.lru_cache(maxsize=None)
def _arm(name, dtype, kernel="valu"):
    """Engine, iterate and float64 references of one row of _ARMS: computed once."""
    from pyneuralempc_amd import CallbackEngine
    nx, nu, H, B, box, tracking = _ARMS[name]
    net = _arm_net(nx, nu)
    eng = CallbackEngine(net.W, net.b, H, nx, nu, dtype=DTYPES[dtype], device="cuda:0", max_batch=B, kernel=kernel)
    if box is not None:
        eng.set_box_rows(*box)
    ob = _objective(H, nx, nu)
    eng.set_objective(**ob)
    Zh, X0h = orc.synthetic_inputs(B, H, nx, nu, seed=41)
    f, grad, g, J = orc.Problem(net, H, nx, nu, orc.DISCRET, box=box, **ob).eval_batch(Zh, X0h)
    if tracking:          # every problem against its own references and linear costs
        rng = np.random.default_rng(43)
        per = {k: 0.4 * rng.normal(size=(B, H, dim)) for k, dim in (("xref", nx), ("uref", nu), ("cx", nx), ("cu", nu))}
        eng.bind_tracking(**{k: eng.to_device(v) for k, v in per.items()})
        probs = [orc.Problem(net, H, nx, nu, orc.DISCRET, **dict(ob, **{k: v[b] for k, v in per.items()})) for b in range(B)]
        f = np.array([p.objective(Zh[b]) for b, p in enumerate(probs)])
        grad = np.stack([p.gradient(Zh[b]) for b, p in enumerate(probs)])
    return eng, Zh, X0h, {"f": f, "grad": grad, "g": g, "jac_dense": J}


def _arm_expectation(name, dtype, want):
    """{lead: writer} by the restated rule alone (torch allocations and the aligned guard keep lead 0 on 16 bytes)."""
    nx, nu, H, B, box, tracking = _ARMS[name]
    mn = (2 if box else 1) * H * nx * H * (nx + nu)
    esz = 8 if dtype == "fp64" else 4
    objective = ("f" in want or "grad" in want) and not tracking
    leads = (0, 1) if dtype == "fp64" else (0, 1, 2, 3)
    exp = {lead: rule.assembly_writer(mn, B, esz, lead * esz, False, objective) for lead in leads}
    exp["own"] = "post_scatter_kernel"
    return exp


@pytest.mark.parametrize("want", [DEFAULT, GJ], ids=["default", "g+jac"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("name", list(_ARMS))
def test_assembly_arms(name, dtype, want):
    """kernel="valu": every dense matrix comes from the row launch + an assembly launch.  Aligned lead, misaligned leads and the
    engine's own buffer on one handle and iterate: the writers the rule names, (i) to (v) each, the same bits from all."""
    eng, Zh, X0h, refs = _arm(name, dtype)
    assert eng.kernel_variant == "valu" and eng.m * eng.n == (2 if _ARMS[name][4] else 1) * eng.H * eng.nx * eng.n
    exp = _arm_expectation(name, dtype, want)
    got = _check(eng, Zh, X0h, want, refs, f"{name}/{dtype}", leads=tuple(k for k in exp if k != "own"), tracking=_ARMS[name][5])
    assert eng.last_row_kernel == "rows_valu_kernel"
    assert got == exp, (got, exp)


def test_the_named_shapes_sit_on_both_sides_of_the_boundary():
    """65 280 is refused by the error bound and 64 000 admitted, in both precisions and for the B of the test; 64 000 is the
    largest m*n = [2] H^2 nx (nx + nu) over nx, nu <= 16, H <= 64 that is a multiple of 4 and below the first refusal."""
    first = min(rule.first_inexact(esz, 1 << 17) for esz in (8, 4))
    assert first == 64060
    reach = {box * H * nx * H * (nx + nu) for nx in range(1, 17) for nu in range(1, 17) for H in range(1, 65) for box in (1, 2)}
    assert max(v for v in reach if v % 4 == 0 and v < first) == ADMITTED_MN
    for esz in (8, 4):
        assert rule.flat_refusal(REFUSED_MN, 2, esz, 0) == rule.INEXACT and rule.flat_refusal(ADMITTED_MN, 2, esz, 0) is None
    for name, mn in (("refused_65280", REFUSED_MN), ("admitted_64000", ADMITTED_MN)):
        nx, nu, H, _, _, _ = _ARMS[name]
        assert H * nx * H * (nx + nu) == mn
    for dtype in ("fp64", "fp32"):
        assert _arm_expectation("refused_65280", dtype, DEFAULT)[0] == "post_kernel"
        assert _arm_expectation("refused_65280", dtype, GJ)[0] == "assemble_dense_kernel"
        assert _arm_expectation("admitted_64000", dtype, DEFAULT)[0] == "post_flat_kernel"


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("net", ["1x8", "2x64"])
def test_fused_launches_decline_a_misaligned_buffer(net, dtype):
    """kernel="auto", 2/1 at H = 20, the matrix one element off a 16-byte boundary: the fused fixed-shape launch (2 x 64) and
    rows_coop_kernel+dense (1 x 8) both decline, the rows come from the plain row launch and the per-problem grid stores
    element by element -- (i) to (iii) against the oracle, the expected writer, the guards."""
    if net == "2x64":
        eng, Zh, X0h, refs = _seeded_engine("2x64", dtype, 20, 5)
    else:
        eng, Zh, X0h, refs = _arm("h20", dtype, "auto")
    assert eng.kernel_variant == "mfma"
    for want, writer in ((DEFAULT, "post_kernel"), (GJ, "assemble_dense_kernel")):
        got = _check(eng, Zh, X0h, want, refs, f"auto/{net}/{dtype}", leads=(1,), resident_side=False)
        assert got == {1: writer}
        assert eng.last_row_kernel in ("rows_coopfx_kernel", "rows_coop_kernel", "rows_mfma_kernel")
        assert eng.last_row_kernel == ("rows_coopfx_kernel" if net == "2x64" else eng.last_row_kernel)
        # ... and the aligned buffer next to it is the row launch's again
        assert _check(eng, Zh, X0h, want, refs, f"auto/{net}/{dtype}", leads=(0,))[0] == "row_launch"


def test_every_writer_code_is_asserted_in_both_dtypes():
    """The five codes of nempc_last_dense_writer, each met and asserted by _check in fp64 and in fp32 (printed)."""
    seen = set()
    for dtype in ("fp64", "fp32"):
        eng, Zh, X0h, refs = _arm("h20", dtype)
        for want in (DEFAULT, GJ):
            _check(eng, Zh, X0h, want, refs, f"h20/{dtype}", leads=(0, 1), seen=seen)
        eng, Zh, X0h, refs = _seeded_engine("2x64", dtype, 20, 5)
        _check(eng, Zh, X0h, DEFAULT, refs, f"2x64/{dtype}", seen=seen)
        assert eng.eval(eng.to_device(Zh), eng.to_device(X0h), ("f", "g")) and eng.last_dense_writer is None      # code 0
    from pyneuralempc_amd import CallbackEngine
    names = {v: k for k, v in CallbackEngine.DENSE_WRITERS.items()}
    for dt, w in sorted(seen, key=lambda p: (p[0], names[p[1]])):
        print(f"asserted: {dt} code {names[w]} {w}")
    assert seen == {(str(dt), w) for dt in DTYPES.values() for w in names if w is not None}
