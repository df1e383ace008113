"""The cases that pin which register-resident kernel serves a request (csrc/mfma_plan.h): one list, used by the recorder
(tools/record_mfma_launches.py -> tests/golden/mfma_launches.json), by the stand-alone plan check (test_mfma_plan_cpu.py) and
by the device test (test_gpu_mfma_plan.py).  Small on purpose: B <= 64, H <= 20.

A case names a network, a dtype, the call and what it asks for; `cus` overrides the device's compute-unit count
(NEMPC_NUM_CUS, read when the handle is created) so that the tile-count rule can be crossed on any device."""
import os

import numpy as np

# name -> (nx, nu, hidden widths, hidden activations (None = tanh), extra network inputs)
NETS = {
    "c2": (2, 1, [64, 64], None, 0),                      # compiled shape, every activation in fp64
    "c2relu": (2, 1, [64, 64], "relu", 0),               # compiled in fp64 only
    "c2rt": (2, 1, [64, 64], ["relu", "tanh"], 0),       # per-layer codes at run time: no compiled shape
    "lv": (2, 1, [30, 30], None, 0),                      # the 3 -> 30 -> 30 -> 2 example network (padded width 32)
    "s64": (3, 2, [48, 32], None, 0),                     # padded width 64, not a compiled shape
    "w32": (4, 2, [32], None, 0),                         # one hidden layer
    "c3": (6, 3, [128, 128, 128], None, 0),               # 6/3 3 x 128: compiled dimensions in fp32, streamed weights in fp64
    "in17": (16, 1, [64], None, 0),                       # nin = 17: two 16-row input blocks
    "ks5": (12, 4, [32, 32], None, 2),                    # nin + ne = 18: five k-steps
}

EVAL_ALL = ("f", "grad", "g", "jac_dense")


def _c(id, net, dtype, call, want, B=8, H=4, kind="discret", kernel="mfma", cus=0, misalign=False):
    return dict(id=id, net=net, dtype=dtype, call=call, want=tuple(want), B=B, H=H, kind=kind, kernel=kernel, cus=cus,
                misalign=misalign, window=1)


def _both(id, net, call, want, **kw):
    return [_c(f"{id}-{dt}", net, dt, call, want, **kw) for dt in ("f64", "f32")]


CASES = (
    # ---- row codes 2 - 7
    _both("tiles-coop", "s64", "eval", ("g", "jac_tiles")) +                                  # 2
    _both("defect-only", "s64", "eval", ("g",)) +                                             # 3 (a defect-only call)
    _both("fused-dense", "c2", "eval", EVAL_ALL, B=9, H=20) +                                 # 4
    _both("coop-dense", "s64", "eval", EVAL_ALL) +                                            # 5
    _both("fused-sparse", "c2", "eval", ("f", "grad", "g", "jac_sparse"), B=9, H=20) +        # 6
    _both("coop-sparse", "s64", "eval", ("f", "grad", "g", "jac_sparse")) +                   # 7
    _both("fused-forward-only", "c2", "eval", ("f", "g"), B=9, H=20) +
    _both("tiles-compiled", "c2", "eval", ("g", "jac_tiles"), B=9, H=20) +
    _both("lv-dense", "lv", "eval", EVAL_ALL, B=5, H=7) +
    _both("relu-dense", "c2relu", "eval", EVAL_ALL, B=5, H=6) +
    _both("rt-dense", "c2rt", "eval", EVAL_ALL, B=5, H=6) +
    _both("w32-dense-sparse", "w32", "eval", ("g", "jac_dense", "jac_sparse"), B=3, H=3, kind="unity") +
    _both("ragged-dense", "s64", "eval", EVAL_ALL, B=3, H=3) +                                # row blocks no whole 16-byte vectors in fp32
    _both("rk4-dense", "s64", "eval", EVAL_ALL, B=5, H=4, kind="rk4") +
    # ---- both sides of the tile-count rule (one compute unit: 32 tiles)
    _both("cus1-under", "s64", "eval", ("g", "jac_tiles"), B=16, H=20, cus=1) +
    _both("cus1-over", "s64", "eval", ("g", "jac_tiles"), B=32, H=20, cus=1) +
    _both("cus1-over-dense", "s64", "eval", EVAL_ALL, B=32, H=20, cus=1) +
    _both("cus1-compiled", "c2", "eval", EVAL_ALL, B=32, H=20, cus=1) +
    # ---- shapes
    _both("two-block-input", "in17", "eval", EVAL_ALL, B=3, H=2) +
    _both("five-k-steps", "ks5", "eval", EVAL_ALL, B=3, H=4) +
    _both("tile-variant", "c2", "eval", EVAL_ALL, B=9, H=20, kernel="mfma_tile") +
    _both("c3-dense", "c3", "eval", EVAL_ALL, B=5, H=6) +                                      # fp32: compiled dimensions; fp64: streamed
    _both("c3-tiles", "c3", "eval", ("g", "jac_tiles"), B=5, H=6) +
    _both("misaligned-dense", "c2", "eval", EVAL_ALL, B=9, H=20, misalign=True) +
    _both("misaligned-coop-dense", "s64", "eval", EVAL_ALL, misalign=True) +
    # ---- Hessian codes 2, 3, 4 and their forms inside the RK4 pipeline
    _both("hess-coop", "s64", "hess", ("hvals", "hdense")) +                                   # 2
    _both("hess-coop-hvals", "s64", "hess", ("hvals",)) +                                      # 2, tril values from the kernel
    _both("hess-tile", "s64", "hess", ("hvals", "hdense"), kernel="mfma_tile") +               # 3
    _both("hess-tile-hvals", "s64", "hess", ("hvals",), kernel="mfma_tile") +
    _both("hess-two-block", "in17", "hess", ("hvals",), B=3, H=2) +                            # 3
    _both("hess-compiled", "c2", "hess", ("hvals", "hdense"), B=9, H=20) +                     # 4
    _both("hess-compiled-hvals", "c2", "hess", ("hvals",), B=9, H=20) +
    _both("hess-c3", "c3", "hess", ("hvals",), B=3, H=5) +                                     # fp32: 4; fp64: 3, streamed
    _both("hess-rk4-coop", "s64", "hess", ("hvals", "hdense"), kind="rk4") +                   # 12
    _both("hess-rk4-tile", "s64", "hess", ("hvals", "hdense"), kind="rk4", kernel="mfma_tile") +   # 13
    _both("hess-rk4-c3", "c3", "hess", ("hvals",), B=3, H=5, kind="rk4") +                     # fp32: 14; fp64: 13
    _both("hess-rk4-c2", "c2", "hess", ("hvals",), B=5, H=6, kind="rk4") +
    _both("hess-cus1-over", "s64", "hess", ("hvals",), B=32, H=20, cus=1) +
    # ---- Gauss-Newton callback
    _both("gn-compiled", "c2", "hess_gn", ("hvals",), B=9, H=20) +                             # fp64: one launch
    _both("gn-compiled-dense", "c2", "hess_gn", ("hvals", "hdense"), B=9, H=20) +
    _both("gn-coop", "s64", "hess_gn", ("hvals",)) +
    _both("gn-lv", "lv", "hess_gn", ("hvals",), B=5, H=7)
)
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES) and all(c["B"] <= 64 and c["H"] <= 20 for c in CASES)

TORCH_DTYPE = {"f64": "float64", "f32": "float32"}


def problem(case):
    """-> (oracle network, oracle problem, host inputs dict): seeded, the same for the recorder and the tests."""
    from oracle import nempc_oracle as orc
    nx, nu, hidden, acts, ne = NETS[case["net"]]
    net = orc.MLP.random(nx + nu + ne, hidden, nx, seed=3, activations=None if acts is None else
                         (acts if isinstance(acts, str) else list(acts) + ["linear"]))
    B, H = case["B"], case["H"]
    rng = np.random.default_rng(11)
    extra = rng.normal(size=(H, ne)) if ne else None
    kind = {"discret": orc.DISCRET, "unity": orc.UNITY, "rk4": orc.RK4}[case["kind"]]
    Q = np.eye(nx) + 0.1 * np.arange(nx * nx).reshape(nx, nx)
    prob = orc.Problem(net, H, nx, nu, kind, 0.1 if case["kind"] == "rk4" else 1.0, Q=Q, R=0.2 * np.eye(nu), extra=extra)
    Z, X0 = orc.synthetic_inputs(B, H, nx, nu, seed=5)
    inp = dict(Z=Z, X0=X0, lam=rng.normal(size=(B, prob.m)), sigma=rng.uniform(0.5, 1.5, size=B),
               w=rng.uniform(0.1, 2.0, size=(B, H * nx)), extra=extra, Q=Q, R=0.2 * np.eye(nu))
    return net, prob, inp


def run(case):
    """The case's call on the device.  -> (codes dict, outputs as host float64 arrays).  NEMPC_NUM_CUS is set around the
    handle's creation only."""
    import torch
    from pyneuralempc_amd import CallbackEngine
    net, prob, inp = problem(case)
    nx, nu, _, _, ne = NETS[case["net"]]
    dtype = getattr(torch, TORCH_DTYPE[case["dtype"]])
    B, H = case["B"], case["H"]
    old = os.environ.pop("NEMPC_NUM_CUS", None)
    if case["cus"]:
        os.environ["NEMPC_NUM_CUS"] = str(case["cus"])
    try:
        eng = CallbackEngine(net.W, net.b, H, nx, nu, integrator=case["kind"], DT=prob.DT, dtype=dtype, device="cuda:0",
                             max_batch=B, kernel=case["kernel"], n_extra=ne, activations=net.act)
    finally:
        os.environ.pop("NEMPC_NUM_CUS", None)
        if old is not None:
            os.environ["NEMPC_NUM_CUS"] = old
    if ne:
        eng.bind_extra(eng.to_device(np.broadcast_to(inp["extra"][None], (B, H, ne)).copy()))
    eng.set_objective(Q=inp["Q"], R=inp["R"])
    Z, X0 = eng.to_device(inp["Z"]), eng.to_device(inp["X0"])
    torch.cuda.synchronize()
    if case["call"] == "eval":
        out = None
        if "jac_dense" in case["want"]:
            # a caller-owned matrix (the full matrix every call); misalign: one element past a 16-byte boundary
            flat = torch.full((B * eng.m * eng.n + 4,), float("nan"), dtype=dtype, device="cuda:0")
            off = 1 if case["misalign"] else 0
            out = {"jac_dense": flat[off:off + B * eng.m * eng.n].view(B, eng.m, eng.n)}
            assert out["jac_dense"].data_ptr() % 16 == (flat.element_size() if case["misalign"] else 0)
        res = eng.eval(Z, X0, want=case["want"], out=out)
    elif case["call"] == "hess":
        res = eng.hess(Z, X0, eng.to_device(inp["lam"]), eng.to_device(inp["sigma"]), want=case["want"])
    else:
        res = eng.hess_gn(Z, X0, eng.to_device(inp["w"]), eng.to_device(inp["sigma"]), want=case["want"])
    torch.cuda.synchronize()
    lib, hd = eng.lib, eng._handle
    codes = dict(row=lib.nempc_last_row_kernel(hd), hess=lib.nempc_last_hess_kernel(hd),
                 dense_writer=lib.nempc_last_dense_writer(hd))
    return codes, {k: v.to("cpu", torch.float64).numpy() for k, v in res.items()}, eng


def expected(case, prob, inp, b):
    """The CPU oracle's outputs of problem b, for the names the case asks for."""
    Z, X0 = inp["Z"][b], inp["X0"][b]
    out = {}
    if case["call"] == "eval":
        jac = prob.jacobian(Z, X0) if any(k.startswith("jac") for k in case["want"]) else None
        for k in case["want"]:
            if k == "f": out[k] = prob.objective(Z)
            elif k == "grad": out[k] = prob.gradient(Z)
            elif k == "g": out[k] = prob.constraints(Z, X0)
            elif k == "jac_dense": out[k] = jac
            elif k == "jac_tiles":
                _, A, Bt = prob.tiles_AB(Z, X0)
                out[k] = np.concatenate([A, Bt], axis=2)
    else:
        Hm = (prob.lagrangian_hessian(Z, X0, inp["lam"][b], inp["sigma"][b]) if case["call"] == "hess" else
              prob.gauss_newton_hessian(Z, X0, inp["w"][b], inp["sigma"][b]))
        r, c = prob.hessian_structure()
        for k in case["want"]:
            out[k] = Hm if k == "hdense" else Hm[r, c]
    return out
