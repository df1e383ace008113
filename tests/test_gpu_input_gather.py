"""GPU parity of the register-resident matrix-core kernels on extra network inputs and rolling windows: every case of
tests/input_gather_cases.py against the oracle -- defects, dense Jacobian, tiles, band values, the defect-only call,
Lagrangian Hessian values and, where the case asks, the Gauss-Newton values -- with extras that differ for every problem
and every stage and a history per problem, so that a kernel reading the wrong row's extras or history misses the oracle
(tests/test_input_gather_cases_cpu.py shows each case would see it).  The kernel names are asserted against the case
module's restatement of the plan: nothing passes by falling back to another kernel.  The bound extras are then overwritten
IN PLACE and everything is compared again: the binding holds a pointer, not a copy.

Bars (input_gather_cases.BAR), relative to max(1, |ref|inf), those of the plain-input sweeps of test_gpu_parity.py:
fp64 1e-10 first order, 1e-9 Hessian and Gauss-Newton values; fp32 2e-4 and 2e-3.

Whether the register-staged ("early") path of rows_coop_kernel ran is inferred from the restated launcher predicate
(input_gather_cases.early): the library reports the kernel, not the staging path.

On an MI355X (256 compute units) all 88 cases pass, 7.7 s for the module, the slowest case 0.7 s (the first: it loads the
library), and the sweep found no kernel defect.  Per class: the kernels that ran (last_row_kernel after the tile / dense
call, last_hess_kernel; the defect-only call ran rows_mfma_kernel everywhere) and the largest error as a fraction of its
bar, first order / Hessian values / Gauss-Newton values:

  class  cases  kernels                                                              fp64                   fp32
  a      10     rows_coop_kernel[+dense] early, rowhess_coop_kernel; 6/3 3 x 128     4.2e-6 3.8e-7 1.6e-7   1.2e-3 5.7e-5 6.6e-5
                fp64: rows_mfma_kernel streamed, rowhess_mfma_kernel
  b       4     rows_coop_kernel[+dense] early, 3 - 5 passes a workgroup (width 64)  3.2e-6 2.7e-7 -        8.0e-4 4.9e-5 -
                and 18 (width 128), rowhess_coop_kernel
  c       6     rows_coop_kernel[+dense] direct (1/2 2 x 64 ne = 8 in fp64: early),  3.3e-6 2.1e-7 3.8e-7   5.1e-4 3.8e-5 5.7e-5
                rowhess_coop_kernel
  d      16     rows_coop_kernel direct, rowhess_coop_kernel (2/1 1 x 96 w = 4 in    4.0e-6 3.9e-7 1.9e-7   8.7e-4 6.8e-5 4.7e-5
                fp64: rowhess_mfma_kernel, by the other's LDS)
  e      24     rows_mfma_kernel resident and streamed, rowhess_mfma_kernel          5.7e-6 5.8e-7 4.0e-7   1.5e-3 7.7e-5 7.1e-5
  f      12     rows_coop_kernel[+dense] early / rows_mfma_kernel resident and       2.2e-6 2.0e-7 -        3.2e-4 2.6e-5 -
                streamed, rk4:rowhess_coop_kernel / rk4:rowhess_mfma_kernel
  i      16     all of the above                                                     4.3e-6 3.0e-7 3.3e-7   1.2e-3 4.7e-5 7.4e-5

(classes g and h are the Hessian and Gauss-Newton columns of the others.)  The absolute errors are a few units in the last
place: 5.7e-16 at most in fp64, 2.9e-7 in fp32 -- no fp32 case came near its bar, so none needed a float32 CPU evaluation
of its own.  A wrong row's extras or history would have moved the defects by at least 64 bars (fp32) / 1.3e8 bars (fp64).
"""
import functools

import numpy as np
import pytest
import torch

import input_gather_cases as ig

pytestmark = pytest.mark.gpu

NOT_OURS = ("rows_valu_kernel", "rowhess_valu_kernel", "layered_gemm_kernel")


def _err(got, ref):
    return float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max()))


def _host(t):
    return t.to("cpu", torch.float64).numpy().copy()


@functools.lru_cache(maxsize=None)
def _num_cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _reference(c, net, d, extras, keep):
    """The oracle's outputs of the compared problems, stacked in the order of `keep`."""
    out = dict(g=[], jac=[], tiles=[], hvals=[], gn=[])
    for b in keep:
        prob = ig.problem(c, net, d, b, extras=extras)
        z, x0 = d["Z"][b], d["X0"][b]
        out["g"].append(prob.constraints(z, x0))
        out["jac"].append(prob.jacobian(z, x0))
        if c["window"] == 1:
            _, A, Bt = prob.tiles_AB(z, x0)
            out["tiles"].append(np.concatenate([A, Bt], axis=2))
        else:
            out["tiles"].append(prob.tiles(z, x0)[2])
        out["hvals"].append(prob.hessian_values(z, x0, d["lam"][b], d["sigma"][b]))
        if c["gn"]:
            out["gn"].append(prob.gauss_newton_values(z, x0, d["w"][b], d["sigma"][b]))
    return {k: np.stack(v) for k, v in out.items() if v}


@pytest.mark.parametrize("case_id", [c["id"] for c in ig.CASES])
def test_input_gather_against_the_oracle(case_id):
    c = ig.BY_ID[case_id]
    net, d = ig.data(case_id)
    cus = c["cus"] or _num_cus()
    expect, bar = ig.expected_kernels(c, cus), ig.BAR[c["dtype"]]
    keep = ig.compared_problems(c, cus)
    eng = ig.engine(c, net)
    assert eng.kernel_variant == c["kernel"]
    E = None
    if c["ne"]:
        E = eng.to_device(d["E"])
        eng.bind_extra(E)
        assert eng._extra.data_ptr() == E.data_ptr()
    if c["window"] > 1:
        eng.bind_history(eng.to_device(d["hx"]), eng.to_device(d["hu"]))
    Z, X0, lam, sigma, w = (eng.to_device(d[k]) for k in ("Z", "X0", "lam", "sigma", "w"))
    rows, cols = eng.jac_structure()
    structural = np.zeros((eng.m, eng.n), dtype=bool)
    structural[rows, cols] = True
    orows, ocols = ig.problem(c, net, d, 0).hessian_structure()
    hrows, hcols = eng.hess_structure()
    assert np.array_equal(hrows, orows) and np.array_equal(hcols, ocols)
    worst = dict(first=0.0, hess=0.0, gn=0.0)

    def check(kind, what, got, ref):
        e = _err(got, ref)
        worst[kind] = max(worst[kind], e / bar[kind])
        print(f"{case_id} {what}: {e:.2e} = {e / bar[kind]:.3f} of the bar")
        assert e < bar[kind], (case_id, what, e, bar[kind])

    for nth, extras in enumerate(("E", "E2") if c["ne"] else ("E",)):
        tag = f"[{extras}]"
        if nth:
            E.copy_(eng.to_device(d["E2"]))          # in place: the handle keeps reading the tensor it was given
        ref = _reference(c, net, d, extras, keep)
        # ---- tiles, dense matrix and band values from one launch's tiles
        res = {k: _host(v) for k, v in eng.eval(Z, X0, want=("g", "jac_dense", "jac_tiles", "jac_sparse")).items()}
        assert eng.last_row_kernel == expect["tiles"], (case_id, eng.last_row_kernel)
        check("first", "g" + tag, res["g"][keep], ref["g"])
        check("first", "jac_dense" + tag, res["jac_dense"][keep], ref["jac"])
        check("first", "jac_tiles" + tag, res["jac_tiles"][keep], ref["tiles"])
        assert np.array_equal(res["jac_sparse"], res["jac_dense"][:, rows, cols]), case_id
        nz = res["jac_dense"] != 0
        assert not nz[:, ~structural].any(), case_id
        relu = "relu" in (c["act"] if isinstance(c["act"], list) else [c["act"]])
        if not relu:                                 # (a dead relu unit is an exact 0 inside the pattern)
            assert np.array_equal(nz[keep], ref["jac"] != 0), case_id
        # ---- the dense matrix alone: plain models get it from the cooperative launch itself
        res = {k: _host(v) for k, v in eng.eval(Z, X0, want=("g", "jac_dense")).items()}
        assert eng.last_row_kernel == expect["dense"], (case_id, eng.last_row_kernel)
        check("first", "g, dense call" + tag, res["g"][keep], ref["g"])
        check("first", "jac_dense, dense call" + tag, res["jac_dense"][keep], ref["jac"])
        assert not (res["jac_dense"] != 0)[:, ~structural].any(), case_id
        # ---- defects alone
        g = _host(eng.eval(Z, X0, want=("g",))["g"])
        assert eng.last_row_kernel == expect["defect"], (case_id, eng.last_row_kernel)
        check("first", "g, defect-only call" + tag, g[keep], ref["g"])
        # ---- Lagrangian Hessian values
        hv = _host(eng.hess(Z, X0, lam, sigma)["hvals"])
        assert eng.last_hess_kernel == expect["hess"], (case_id, eng.last_hess_kernel)
        check("hess", "hvals" + tag, hv[keep], ref["hvals"])
        if c["gn"]:
            gv = _host(eng.hess_gn(Z, X0, w, sigma)["hvals"])
            assert eng.last_row_kernel == expect["tiles"], (case_id, eng.last_row_kernel)
            check("gn", "gn hvals" + tag, gv[keep], ref["gn"])
        assert eng.last_row_kernel not in NOT_OURS and eng.last_hess_kernel not in NOT_OURS
    print(f"SUMMARY {case_id} class {ig.class_of(c)} rows {expect['tiles']} / {expect['dense']} hess {expect['hess']} "
          f"early {ig.early(c, cus)} worst first {worst['first']:.3f} hess {worst['hess']:.3f} gn {worst['gn']:.3f}")
