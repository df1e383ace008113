"""GPU: a handle gives its device memory back, and nempc_reserve leaves it computing what a fresh handle computes.

One cycle creates a handle on every path that owns workspaces of its own -- the generic kernels, the register-resident
matrix-core kernels, the layered pipeline, the RK4 Hessian pipeline, extra network inputs, and the 64/32 linear shape whose
nempc_kkt_solve working sets live outside LDS --, runs every call that allocates or grows one (eval, hess, solve, kkt_solve,
weight_grad, extra_grad), replaces the weights, reserves 4 x the batch, evaluates at the larger batch and destroys the handle.
"""
import functools
import gc

import numpy as np
import pytest
import torch

import solver_step_cases as sc

pytestmark = pytest.mark.gpu

GROW = 4
# The slack: the largest drift of the free figure with the library of the commit before DevBuf -- five processes, one warm-up
# and four measured cycles each, every later cycle against the first measured one -- was 0 bytes, at max_batch 1024 as at
# 8 and 512 (profiles/handle_ownership.txt, section 2).
SLACK_BYTES = 0
# The batch: 0 is below any buffer, but the figure moves in steps of 2 MiB (small allocations share chunks of that size: same
# section), so a buffer counts as covered when the copies that three cycles would leak take more than a chunk.  Per kind of
# handle, as held at destruction, after the reserve to GROW * MAX_BATCH = 4096 problems (H = 4, n = 12, m = 8, nin = 3):
#   the five 2/1 handles, 15 copies: d_g_ws 4096 * m * 8 = 256 KiB each, 3.75 MiB -- the smallest max_batch-sized workspace;
#     d_kkt_grad 384 KiB, d_tiles_ws 768 KiB, d_hess_ws 1152 KiB each;
#   the RK4 handle alone, 3 copies: d_rk4_nu 16384 rows * 4 * nx * 8 = 1 MiB each, 3 MiB (d_rk4_ht 4.5 MiB, d_rk4_stage 7.5 MiB).
# (At 512 d_g_ws came to 1.9 MiB and d_rk4_nu to 1.5 MiB: under a step.)  Not covered, whatever the batch within a few
# seconds: the copies nempc_reserve replaces, sized for MAX_BATCH itself (d_g_ws 64 KiB x 15, d_kkt_grad 96 KiB x 15,
# d_rk4_nu 256 KiB x 3), and what max_batch does not size (weights, maps, the objective table, the pair table).  For those
# DevBuf::alloc's own reset and tests/dev_buf_check.cpp stand.  At max_batch 8 the figure does not see a whole kept handle.
MAX_BATCH = 1024

#        name: (nx, nu, hidden, integrator, DT, H, n_extra, activation, handle keywords, calls)
EVERY = ("eval", "hess", "solve", "kkt_solve", "weight_grad")
SHAPES = {
    "generic": (2, 1, [16], "discret", 1.0, 4, 0, "tanh", {"kernel": "valu"}, EVERY),
    "matrix_core": (2, 1, [16, 16], "discret", 1.0, 4, 0, "tanh", {"kernel": "mfma"}, EVERY),
    "layered": (2, 1, [16, 16], "discret", 1.0, 4, 0, "tanh", {"kernel": "layered"}, EVERY),
    "rk4": (2, 1, [16, 16], "rk4", 0.1, 4, 0, "tanh", {"kernel": "mfma"}, EVERY),
    "extras": (2, 1, [16], "discret", 1.0, 4, 2, "tanh", {}, EVERY + ("extra_grad",)),
    # tests/test_gpu_sensitivity.py's 64x32_global_scratch row: 172 KB a problem, nempc_kkt_solve's region in global memory
    "global_scratch": (64, 32, [8], "discret", 1.0, 2, 0, "linear", {}, ("eval", "hess", "kkt_solve")),
}


@functools.lru_cache(maxsize=None)
def _case(name, max_batch):
    nx, nu, hidden, integ, DT, H, ne, act, _, _ = SHAPES[name]
    return sc.Case(name, nx, nu, hidden, integ, DT, H, ("auto",), "float64", n_extra=ne, act=act, B=GROW * max_batch,
                   seed=sc.QP_SEED if act == "linear" else 1, scale_b=True)


def _second_weights(case):
    return [0.9 * w for w in case.net.W], [b + 0.01 for b in case.net.b]


def _engine(name, max_batch, batch, second=False):
    from pyneuralempc_amd import CallbackEngine
    case = _case(name, max_batch)
    W, b = _second_weights(case) if second else (case.net.W, case.net.b)
    eng = CallbackEngine(W, b, case.H, case.nx, case.nu, integrator=case.integ, DT=case.DT, dtype=torch.float64, device="cuda:0",
                         max_batch=batch, n_extra=case.n_extra, activations=case.net.act, **SHAPES[name][8])
    eng.set_objective(**case.obj)
    return eng


def _np(t):
    return t.detach().cpu().numpy().copy()


def _evaluate(eng, case, B):
    """eval and hess of the first B problems at the case's random points, as host arrays"""
    case.bind(eng, B)
    Z, X0 = eng.to_device(case.Zrand[:B]), eng.to_device(case.X0[:B])
    lam = eng.to_device(np.random.default_rng(5).normal(size=(B, eng.m)))
    out = {k: _np(v) for k, v in eng.eval(Z, X0).items()}
    out["hvals"] = _np(eng.hess(Z, X0, lam, torch.ones(B, dtype=eng.dtype, device=eng.device))["hvals"])
    return out


def _calls(eng, case, B, calls):
    """every call of `calls` once at batch B: the ones that allocate or grow a workspace of the handle do so here"""
    X0 = case.bind(eng, B)
    n, hx, nu = eng.n, case.H * case.nx, case.nu
    rng = np.random.default_rng(7)
    lb = np.concatenate([np.full(hx, -np.inf), np.full(case.H * nu, -0.6)])
    Z, lam = eng.to_device(case.Zrand[:B]), eng.to_device(rng.normal(size=(B, eng.m)))
    zl = zu = None
    if "eval" in calls:
        eng.eval(Z, X0)
    if "hess" in calls:
        eng.hess(Z, X0, lam, torch.ones(B, dtype=eng.dtype, device=eng.device))
    if "solve" in calls:
        Z, _, _, duals = eng.solve(X0, lb=lb, ub=-lb, max_iter=10, return_duals=True)
        lam, zl, zu = duals["lam"], duals["zl"], duals["zu"]
    v = w = None
    if "kkt_solve" in calls:
        res = eng.kkt_solve(Z, X0, lam, zl, zu, lb, -lb, rz=eng.to_device(rng.normal(size=(B, 2, n))), want=("v", "w", "gx0"))
        v, w = res["v"][:, 0].contiguous(), res["w"][:, 0].contiguous()
    if "weight_grad" in calls:
        eng.weight_grad(Z, X0, w, lam=lam, v=v, flat=True)
    if "extra_grad" in calls:
        eng.extra_grad(Z, X0, w, lam=lam, v=v)


def cycle(max_batch=MAX_BATCH):
    """Steps 1 to 5 of the module docstring for every shape.  -> {name: the evaluation at the larger batch}"""
    out = {}
    for name in SHAPES:
        case = _case(name, max_batch)
        eng = _engine(name, max_batch, max_batch)
        _calls(eng, case, max_batch, SHAPES[name][9])
        eng.set_weights(*_second_weights(case))
        eng.reserve(GROW * max_batch)
        out[name] = _evaluate(eng, case, GROW * max_batch)
        eng._destroy()          # (not left to Python's collector)
    return out


def free_bytes():
    """the device's free figure with nothing of this process' tensors cached"""
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return torch.cuda.mem_get_info()[0]


def measured_cycles(max_batch=MAX_BATCH, cycles=4):
    """free bytes after each of `cycles` cycles (a warm-up cycle first is the caller's)"""
    free = []
    for _ in range(cycles):
        cycle(max_batch)
        free.append(free_bytes())
    return free


@pytest.fixture(scope="module")
def warm():
    """The warm-up cycle (code objects and the runtime's own pools are taken on first use): its results serve (a)."""
    return cycle()


def test_a_reserved_handle_computes_what_a_fresh_one_does(warm):
    """(a) f, grad, g, the dense Jacobian and the Hessian values at 4 x the batch -- after every call, a second
    set_weights and the reserve -- are the bits of a fresh handle created at that size with those weights."""
    for name in SHAPES:
        case = _case(name, MAX_BATCH)
        eng = _engine(name, MAX_BATCH, GROW * MAX_BATCH, second=True)
        fresh = _evaluate(eng, case, GROW * MAX_BATCH)
        eng._destroy()
        assert set(fresh) == set(warm[name]) == {"f", "grad", "g", "jac_dense", "hvals"}
        for key, ref in fresh.items():
            assert np.isfinite(ref).all() and np.array_equal(warm[name][key], ref), (name, key)


def test_destroyed_handles_give_their_device_memory_back(warm):
    """(b) the device's free figure after each of three further cycles is no lower than after the first measured one by more
    than SLACK_BYTES."""
    free = measured_cycles()
    print(f"[handle lifecycle] free bytes after each measured cycle: {free}; drift {[free[0] - f for f in free[1:]]}")
    for f in free[1:]:
        assert free[0] - f <= SLACK_BYTES, free
