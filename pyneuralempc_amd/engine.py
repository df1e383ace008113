"""Batched callback engine: the thin host wrapper over the C ABI.

One ``CallbackEngine`` = one ``nempc_handle``: a fixed problem family (dims, integrator, network,
objective, optional box rows) evaluated for a batch of B independent problems per call on one
MI355X.  torch is used for device memory and streams only; every number is produced by the HIP
kernels in csrc/.
"""
import ctypes

import numpy as np
import torch

from . import _lib

_TORCH_DTYPES = {torch.float64: _lib.F64, torch.float32: _lib.F32}


def resolve_activations(activations, n_layers):
    """Per-layer activation names of an n_layers-deep dense stack.  None: tanh hidden layers and a linear output layer
    (the reference's nn_model.h5); one name: that activation on every hidden layer, linear output; a sequence: one name
    per layer, the output layer included.  Names as Keras spells them (_lib.ACTIVATION_IDS); "elu:0.5" / "leaky_relu:0.1"
    carry their alpha (_lib.split_activation)."""
    if activations is None:
        names = ["tanh"] * (n_layers - 1) + ["linear"]
    elif isinstance(activations, str):
        names = [activations] * (n_layers - 1) + ["linear"]
    else:
        names = [str(a) for a in activations]
        if len(names) != n_layers:
            raise ValueError(f"activations: expected one name per dense layer ({n_layers}), got {len(names)}")
    for a in names:
        _lib.split_activation(a)
    return names


def _as_c_double(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def check_rate_args(H, nu, dtype, device, u_prev, S, du_lb, du_ub):
    """Arguments of CallbackEngine.bind_rate, checked before the C call (no device is touched): u_prev a `dtype` tensor
    (B,nu) on `device`, B >= 1, required; S (nu,nu) finite; du_lb / du_ub (nu,) or (H,nu) -- both the same form when both
    are given --, no NaN, du_lb < du_ub on every entry.  -> (S, du_lb, du_ub as float64 arrays or None, per_stage 0 | 1)."""
    H, nu = int(H), int(nu)
    if u_prev is None:
        raise ValueError("bind_rate: u_prev is required whenever S, du_lb or du_ub is given")
    if (not isinstance(u_prev, torch.Tensor) or u_prev.dtype != dtype or u_prev.device != torch.device(device) or u_prev.dim() != 2
            or u_prev.shape[1] != nu or u_prev.shape[0] < 1):
        got = (tuple(u_prev.shape), u_prev.dtype, str(u_prev.device)) if isinstance(u_prev, torch.Tensor) else type(u_prev).__name__
        raise ValueError(f"bind_rate: u_prev must be a {dtype} tensor (B,{nu}) on {device}, got {got}")
    Sa = None
    if S is not None:
        Sa = np.asarray(S, dtype=np.float64)
        if Sa.shape != (nu, nu) or not np.isfinite(Sa).all():
            raise ValueError(f"bind_rate: S must be a finite {(nu, nu)} matrix, got shape {Sa.shape}")
    lims, forms = {}, set()
    for name, v in (("du_lb", du_lb), ("du_ub", du_ub)):
        if v is None:
            continue
        a = np.asarray(v, dtype=np.float64)
        if a.shape not in ((nu,), (H, nu)):
            raise ValueError(f"bind_rate: {name} must have shape {(nu,)} (every step) or {(H, nu)} (per step), got {a.shape}")
        if np.isnan(a).any():
            raise ValueError(f"bind_rate: {name} has a NaN")
        lims[name] = a
        forms.add(a.ndim)
    if len(forms) > 1:        # one form in the C interface
        lims = {k: np.broadcast_to(a, (H, nu)) for k, a in lims.items()}
    if len(lims) == 2 and (lims["du_lb"] >= lims["du_ub"]).any():
        raise ValueError("bind_rate: du_lb >= du_ub on some entry (the barrier needs an interior)")
    if "du_lb" in lims and np.isposinf(lims["du_lb"]).any() or "du_ub" in lims and np.isneginf(lims["du_ub"]).any():
        raise ValueError("bind_rate: du_lb >= du_ub on some entry (the barrier needs an interior)")
    per_stage = 1 if any(a.ndim == 2 for a in lims.values()) else 0
    cont = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    return cont(Sa), cont(lims.get("du_lb")), cont(lims.get("du_ub")), per_stage


def check_rows_args(H, nx, nu, C, lo, hi):
    """Arguments of CallbackEngine.bind_rows, checked before the C call (no device is touched): C (nc, nx+nu) finite, nc >= 1;
    lo / hi (nc,) or (H,nc) -- both the same form when both are given --, no NaN, lo < hi on every entry.
    -> (C, lo, hi as float64 arrays or None, per_stage 0 | 1)."""
    H, nio = int(H), int(nx) + int(nu)
    Ca = np.asarray(C, dtype=np.float64)
    if Ca.ndim != 2 or Ca.shape[0] < 1 or Ca.shape[1] != nio or not np.isfinite(Ca).all():
        raise ValueError(f"bind_rows: C must be a finite (nc, {nio}) matrix with nc >= 1, got shape {Ca.shape}")
    nc = Ca.shape[0]
    lims, forms = {}, set()
    for name, v in (("lo", lo), ("hi", hi)):
        if v is None:
            continue
        a = np.asarray(v, dtype=np.float64)
        if a.shape not in ((nc,), (H, nc)):
            raise ValueError(f"bind_rows: {name} must have shape {(nc,)} (every step) or {(H, nc)} (per step), got {a.shape}")
        if np.isnan(a).any():
            raise ValueError(f"bind_rows: {name} has a NaN")
        lims[name] = a
        forms.add(a.ndim)
    if len(forms) > 1:        # one form in the C interface
        lims = {k: np.broadcast_to(a, (H, nc)) for k, a in lims.items()}
    if len(lims) == 2 and (lims["lo"] >= lims["hi"]).any() or \
            "lo" in lims and np.isposinf(lims["lo"]).any() or "hi" in lims and np.isneginf(lims["hi"]).any():
        raise ValueError("bind_rows: lo >= hi on some entry (the barrier needs an interior)")
    per_stage = 1 if any(a.ndim == 2 for a in lims.values()) else 0
    cont = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)
    return cont(Ca), cont(lims.get("lo")), cont(lims.get("hi")), per_stage


def _ptr(t):
    """device pointer of a tensor for the C ABI; None stays None (an optional argument)"""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class CallbackEngine:
    def __init__(self, weights, biases, H, nx, nu, integrator="discret", DT=1.0, dtype=torch.float64,
                 device="cuda", max_batch=1, kernel="auto", n_extra=0, rolling_window=1, forward_rolling=True,
                 activations=None):
        if not torch.cuda.is_available():
            raise RuntimeError("pyneuralempc_amd needs a HIP device (torch.cuda.is_available() is False); "
                               "there is no CPU fallback")
        self.lib = _lib.load()
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("CallbackEngine runs on a HIP device only")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if dtype not in _TORCH_DTYPES:
            raise ValueError("dtype must be torch.float64 or torch.float32")
        self.dtype = dtype
        # rolling-window models (model/tensorflow.py:132, model/jax.py:93): the network of step t reads the last
        # `rolling_window` states and controls; nin is the tile width = number of decision inputs one step reads
        self.rolling_window = int(rolling_window)
        if self.rolling_window < 1:
            raise ValueError("Your rolling windows need to be an integer gretter than 1.")
        self.forward_rolling = bool(forward_rolling)
        self._history = None
        self.H, self.nx, self.nu = int(H), int(nx), int(nu)
        self.nin = self.rolling_window * (self.nx + self.nu)
        self.n_extra = int(n_extra)   # tvp_dim + p_dim of the reference's Model: network inputs that are not variables
        self._extra = None
        self._tracking = None
        self._bounds = None
        self._rate = None
        self._rows = None
        self.integrator = integrator if isinstance(integrator, int) else _lib.INTEGRATOR_IDS[integrator]
        self.DT = float(DT)
        self.kernel = kernel
        self._weights = [np.ascontiguousarray(w, dtype=np.float64) for w in weights]
        self._biases = [np.ascontiguousarray(b, dtype=np.float64).reshape(-1) for b in biases]
        if len(self._weights) != len(self._biases) or not self._weights:
            raise ValueError("weights and biases must be non-empty lists of equal length")
        if len(self._weights) > _lib.MAX_LAYERS:
            raise ValueError(f"at most {_lib.MAX_LAYERS} dense layers are supported")
        prev = self.nin + self.n_extra
        for w, b in zip(self._weights, self._biases):
            if w.ndim != 2 or w.shape[0] != prev or b.shape != (w.shape[1],):
                raise ValueError("layer shapes do not chain: expected kernel (in,out) and bias (out,)")
            prev = w.shape[1]
        if prev != self.nx:
            raise ValueError("Your model do not provide a suitable output dim ! It must get the same dim as the "
                             "state dim.")
        self.activations = resolve_activations(activations, len(self._weights))
        self._objective = None
        self._box = None
        self._handle = None
        self.max_batch = 0
        self._buffers = {}
        self._create(int(max_batch))

    # ------------------------------------------------------------------ handle management
    def _create(self, max_batch):
        self._destroy()
        self._buffers = {}          # (their registrations went with the handle)
        cfg = _lib.NempcConfig()
        cfg.abi_version = _lib.ABI_VERSION
        cfg.device = self.device.index
        cfg.dtype = _TORCH_DTYPES[self.dtype]
        cfg.integrator = self.integrator
        cfg.H, cfg.nx, cfg.nu = self.H, self.nx, self.nu
        cfg.n_layers = len(self._weights)
        for i, w in enumerate(self._weights):
            cfg.widths[i] = w.shape[1]
            name, par = _lib.split_activation(self.activations[i])
            cfg.activations[i], cfg.act_param[i] = _lib.ACTIVATION_IDS[name], par
        cfg.max_batch = max_batch
        cfg.kernel = _lib.KERNEL_NAMES[self.kernel] if isinstance(self.kernel, str) else int(self.kernel)
        cfg.n_extra = self.n_extra
        cfg.rolling_window = self.rolling_window
        cfg.rolling_reverse = 0 if self.forward_rolling else 1
        cfg.DT = self.DT
        h = ctypes.c_void_p()
        _lib.check(self.lib.nempc_create(ctypes.byref(cfg), ctypes.byref(h)))
        self._handle = h
        self.max_batch = max_batch
        nl = len(self._weights)
        dp = ctypes.POINTER(ctypes.c_double)
        Wp = (dp * nl)(*[w.ctypes.data_as(dp) for w in self._weights])
        bp = (dp * nl)(*[b.ctypes.data_as(dp) for b in self._biases])
        _lib.check(self.lib.nempc_set_weights(self._handle, Wp, bp))
        if self._objective is not None:
            self.set_objective(**self._objective)
        if self._box is not None:
            self.set_box_rows(*self._box)
        if self._extra is not None:
            _lib.check(self.lib.nempc_bind_extra(self._handle, ctypes.c_void_p(self._extra.data_ptr()),
                                                 int(self._extra.shape[0])))
        if self._history is not None:
            self.bind_history(*self._history)
        if self._tracking is not None:
            self.bind_tracking(**self._tracking[0], offset=self._tracking[1])
        if self._bounds is not None:
            self.bind_bounds(**self._bounds[0], offset=self._bounds[1])
        if self._rate is not None:
            self.bind_rate(**self._rate)
        if self._rows is not None:
            self.bind_rows(**self._rows)
        self._refresh_dims()
        self._buffers = {}

    def _destroy(self):
        if getattr(self, "_handle", None):
            self.lib.nempc_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self._destroy()
        except Exception:
            pass

    def __getstate__(self):
        raise TypeError("CallbackEngine holds device handles and is not picklable; pickle the plugin objects")

    def _refresh_dims(self):
        n, m, nj, nh = (ctypes.c_int32() for _ in range(4))
        _lib.check(self.lib.nempc_dims(self._handle, ctypes.byref(n), ctypes.byref(m), ctypes.byref(nj),
                                       ctypes.byref(nh)))
        self.n, self.m, self.nnz_jac, self.nnz_hess = n.value, m.value, nj.value, nh.value

    def reserve(self, B):
        """Grow the handle's workspaces to hold B problems (nempc_reserve: the handle, its bindings and its
        communicator are kept)."""
        if B > self.max_batch:
            _lib.check(self.lib.nempc_reserve(self._handle, int(B)))
            self.max_batch = int(B)
            self._drop_buffers()

    @property
    def kernel_variant(self):
        v = self.lib.nempc_kernel_variant(self._handle)
        return {_lib.KERNEL_VALU: "valu", _lib.KERNEL_MFMA: "mfma", _lib.KERNEL_MFMA_TILE: "mfma_tile",
                _lib.KERNEL_LAYERED: "layered"}[v]

    @property
    def last_row_kernel(self):
        """Name of the row kernel the most recent evaluation launched."""
        return self.ROW_KERNELS[self.lib.nempc_last_row_kernel(self._handle)]

    # what the nempc_last_* codes name (the enums of csrc/mfma_plan.h and DenseWriter of csrc/post_plan.h)
    ROW_KERNELS = {0: None, 1: "rows_valu_kernel", 2: "rows_coop_kernel", 3: "rows_mfma_kernel", 4: "rows_coopfx_kernel",
                   5: "rows_coop_kernel+dense", 6: "rows_coopfx_kernel+sparse", 7: "rows_coop_kernel+sparse", 8: "layered_gemm_kernel"}
    HESS_KERNELS = {0: None, 1: "rowhess_valu_kernel", 2: "rowhess_coop_kernel", 3: "rowhess_mfma_kernel", 4: "rowhess_coopfx_kernel",
                    5: "layered_gemm_kernel"}
    HESS_IN_RK4 = 10          # added to a HESS_KERNELS code: the kernel ran inside the RK4 pipeline
    LQ_KERNELS = {0: None, 1: "thread_global", 2: "thread_lds", 3: "wave_lds", 4: "scan"}
    ROLLOUT_KERNELS = {0: None, 1: "rollout_wave_kernel", 2: "rollout_mfma_kernel"}
    DENSE_WRITERS = {0: None, 1: "row_launch", 2: "assemble_dense_kernel", 3: "post_kernel", 4: "post_flat_kernel",
                     5: "post_scatter_kernel"}

    @property
    def last_dense_writer(self):
        """Name of the kernel that wrote jac_dense in the most recent evaluation: "row_launch" (the fused fixed-shape launch
        or rows_coop_kernel+dense), "assemble_dense_kernel", "post_kernel", "post_flat_kernel", "post_scatter_kernel" (the
        engine's own resident buffer); None when no dense matrix was asked for."""
        fn = getattr(self.lib, "nempc_last_dense_writer", None)
        if fn is None:
            raise RuntimeError("this libnempc.so has no nempc_last_dense_writer")
        return self.DENSE_WRITERS[fn(self._handle)]

    @property
    def last_hess_kernel(self):
        """Name of the network kernel the most recent Lagrangian-Hessian evaluation launched ("rk4:" prefix: inside the RK4
        pipeline)."""
        v = self.lib.nempc_last_hess_kernel(self._handle)
        name = self.HESS_KERNELS[v % self.HESS_IN_RK4]
        return ("rk4:" + name) if v >= self.HESS_IN_RK4 and name else name

    @property
    def last_lq_kernel(self):
        """LQ plan of the most recent solve: "thread_global" (thread per problem, working set in global memory),
        "thread_lds", "wave_lds", "scan"; None before the first solve."""
        return self.LQ_KERNELS[self.lib.nempc_last_lq_kernel(self._handle)]

    # ------------------------------------------------------------------ parameters
    def set_objective(self, Q=None, R=None, xref=None, uref=None, cx=None, cu=None, QT=None):
        """Quadratic + linear stage cost; QT (nx,nx) is the state weight of the last step (terminal cost), None = Q."""
        H, nx, nu = self.H, self.nx, self.nu
        keep, ptrs = [], []
        for v, shape in ((Q, (nx, nx)), (R, (nu, nu)), (xref, (H, nx)), (uref, (H, nu)), (cx, (H, nx)),
                         (cu, (H, nu))):
            if v is None:
                ptrs.append(None)
            else:
                a, p = _as_c_double(np.broadcast_to(np.asarray(v, dtype=np.float64), shape))
                keep.append(a)
                ptrs.append(p)
        _lib.check(self.lib.nempc_set_objective(self._handle, *ptrs))
        if QT is None:
            _lib.check(self.lib.nempc_set_terminal_weight(self._handle, None))
        else:
            a, pt = _as_c_double(np.asarray(QT, dtype=np.float64).reshape(nx, nx))
            _lib.check(self.lib.nempc_set_terminal_weight(self._handle, pt))
        self._objective = dict(Q=Q, R=R, xref=xref, uref=uref, cx=cx, cu=cu, QT=QT)
        self._refresh_dims()

    def set_objective_weights(self, Q=None, R=None, QT=None):
        """Re-upload the objective with the given weights replaced: xref / uref / cx / cu and the weights not given stay as
        last set (`set_objective`'s arguments, or the library's defaults where it was given nothing)."""
        ob = dict(self._objective or {})
        for key, val in (("Q", Q), ("R", R), ("QT", QT)):
            if val is not None:
                ob[key] = val
        self.set_objective(**ob)

    def objective_weights(self):
        """(Q (nx,nx), R (nu,nu), QT (nx,nx)) of the handle's objective as float64 arrays: what set_objective was given,
        the library's defaults (I, 0.1 I) where it was given nothing, QT = Q without a terminal weight."""
        ob = self._objective or {}
        Q = np.eye(self.nx) if ob.get("Q") is None else np.array(np.broadcast_to(np.asarray(ob["Q"], dtype=np.float64), (self.nx, self.nx)))
        R = 0.1 * np.eye(self.nu) if ob.get("R") is None else np.array(np.broadcast_to(np.asarray(ob["R"], dtype=np.float64), (self.nu, self.nu)))
        QT = Q.copy() if ob.get("QT") is None else np.asarray(ob["QT"], dtype=np.float64).reshape(self.nx, self.nx).copy()
        return Q, R, QT

    def objective_refs(self):
        """(xref (H,nx), uref (H,nu)) of the handle's shared objective as float64 arrays (zeros where set_objective was given
        nothing): what a problem tracks where no per-problem row is bound."""
        ob = self._objective or {}
        return tuple(np.zeros(shape) if ob.get(k) is None else np.array(np.broadcast_to(np.asarray(ob[k], dtype=np.float64), shape))
                     for k, shape in (("xref", (self.H, self.nx)), ("uref", (self.H, self.nu))))

    @property
    def has_terminal_weight(self):
        """True when the last step is weighed by a QT of its own (set_objective's QT), False when Q weighs every step."""
        return (self._objective or {}).get("QT") is not None

    def tracking_refs(self):
        """{name: (B,H,d) view} of the tensors bound with bind_tracking, the horizon's rows; {} without a binding."""
        if getattr(self, "_tracking", None) is None:
            return {}
        given, offset = self._tracking
        return {k: t[:, offset:offset + self.H] for k, t in given.items()}

    def bind_extra(self, E):
        """Bind the extra network inputs (B,H,n_extra) = [tvp_t ; p] per step for the following evaluations
        (reference: KerasTFModel._gather_input, model/tensorflow.py:39-47).  The tensor is kept alive here."""
        if self.n_extra == 0:
            raise ValueError("this engine was created with n_extra = 0")
        if E.device != self.device or E.dtype != self.dtype or E.dim() != 3 or tuple(E.shape[1:]) != (self.H, self.n_extra):
            raise ValueError(f"extra inputs must be a {self.dtype} tensor (B,{self.H},{self.n_extra}) on {self.device}")
        self._extra = E.contiguous()
        _lib.check(self.lib.nempc_bind_extra(self._handle, ctypes.c_void_p(self._extra.data_ptr()),
                                             int(self._extra.shape[0])))

    def bind_history(self, hist_x, hist_u):
        """Bind the history of a rolling-window model: hist_x (B, w-1, nx) states before x0 (oldest first), hist_u
        (B, w-1, nu) controls before u_0 -- the batched form of set_prev_data (model/tensorflow.py:178-189)."""
        back = self.rolling_window - 1
        if back == 0:
            raise ValueError("this engine was created with rolling_window = 1")
        for t, d, name in ((hist_x, self.nx, "hist_x"), (hist_u, self.nu, "hist_u")):
            if (not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype != self.dtype or t.dim() != 3
                    or tuple(t.shape[1:]) != (back, d)):
                raise ValueError(f"{name} must be a {self.dtype} tensor (B,{back},{d}) on {self.device}")
        if hist_x.shape[0] != hist_u.shape[0]:
            raise ValueError("hist_x and hist_u must cover the same batch")
        self._history = (hist_x.contiguous(), hist_u.contiguous())
        _lib.check(self.lib.nempc_bind_history(self._handle, ctypes.c_void_p(self._history[0].data_ptr()),
                                               ctypes.c_void_p(self._history[1].data_ptr()),
                                               int(self._history[0].shape[0])))

    def bind_tracking(self, xref=None, uref=None, cx=None, cu=None, offset=0):
        """Bind per-problem tracking references / linear costs for the following eval / rollout / solve calls
        (nempc_bind_tracking): problem b is scored against xref[b], uref[b], cx[b], cu[b]; an array left None keeps the
        shared values of set_objective, and the weights Q, R, QT stay shared.  xref, cx: device tensors (B,L,nx); uref, cu:
        (B,L,nu); L >= offset + H, and rows offset .. offset+H-1 of every problem are the horizon's (a window sliding over a
        longer reference needs no copy: bind the same tensors at the next offset).  The tensors are kept alive here, not
        copied.  bind_tracking() with nothing removes the binding."""
        self._tracking = self._bind_rows(self.lib.nempc_bind_tracking, "tracking", ("xref", "uref", "cx", "cu"), (("xref", xref), ("cx", cx)),
                                         (("uref", uref), ("cu", cu)), offset)

    def bind_bounds(self, xlb=None, xub=None, ulb=None, uub=None, offset=0):
        """Bind per-problem, per-stage lower / upper bounds on states and controls for the following solve / kkt_residual /
        sensitivity calls (nempc_bind_bounds): problem b is solved inside the intersection of the call's shared lb / ub, the box
        rows and its own rows xlb[b], xub[b] (on x_1 .. x_H), ulb[b], uub[b] (on u_0 .. u_{H-1}); an array left None adds
        nothing, +-inf means no bound there.  xlb, xub: device tensors (B,L,nx); ulb, uub: (B,L,nu); L >= offset + H, and rows
        offset .. offset+H-1 of every problem are the horizon's (a window sliding over a longer schedule needs no copy: bind
        the same tensors at the next offset).  The tensors are kept alive here, not copied.  bind_bounds() with nothing
        removes the binding.  eval / hess / rollout do not read it."""
        self._bounds = self._bind_rows(self.lib.nempc_bind_bounds, "bounds", ("xlb", "xub", "ulb", "uub"), (("xlb", xlb), ("xub", xub)),
                                       (("ulb", ulb), ("uub", uub)), offset)

    def bind_rate(self, u_prev=None, S=None, du_lb=None, du_ub=None):
        """Bind an input-rate penalty and rate limits for the following solve calls (nempc_bind_rate): with
        du_t = u_t - u_{t-1} and u_{-1} = u_prev[b], problem b minimises f(z) + sum_t du_t' S du_t inside du_lb <= du_t <= du_ub
        (and the bounds of the call as before).  u_prev: device tensor (B,nu) of the engine's dtype, kept alive here, not copied
        (write into it between solves to move on); S (nu,nu), used as given like R, None = no penalty; du_lb / du_ub (nu,) for
        every step or (H,nu) per step, None or +-inf = no limit, du_lb < du_ub on every entry.  bind_rate() with nothing
        removes the binding.  eval / hess / rollout do not read it; kkt_residual, sensitivity, kkt_solve and
        solve(return_duals=True) refuse while it is on, and so does a solve with bind_tracking / bind_bounds rows."""
        fn = getattr(self.lib, "nempc_bind_rate", None)
        if fn is None:
            raise RuntimeError("this libnempc.so has no nempc_bind_rate")
        if u_prev is None and S is None and du_lb is None and du_ub is None:
            _lib.check(fn(self._handle, None, None, None, 0, None, 0))
            self._rate = None
            return
        if self.rolling_window > 1:
            raise ValueError("bind_rate: rolling-window models are not supported")
        Sa, lo, hi, per_stage = check_rate_args(self.H, self.nu, self.dtype, self.device, u_prev, S, du_lb, du_ub)
        u_prev = u_prev if u_prev.is_contiguous() else u_prev.contiguous()
        ptr = lambda a: None if a is None else _as_c_double(a)[1]
        _lib.check(fn(self._handle, ptr(Sa), ptr(lo), ptr(hi), per_stage, ctypes.c_void_p(u_prev.data_ptr()),
                      int(u_prev.shape[0])))
        self._rate = dict(u_prev=u_prev, S=Sa, du_lb=lo, du_ub=hi)

    def bind_rows(self, C=None, lo=None, hi=None):
        """Bind linear stage inequality rows for the following solve calls (nempc_bind_stage_rows): every problem is solved
        inside lo_t <= Cx x_t + Cu u_t <= hi_t for t = 0 .. H-1, C = [Cx | Cu] (nc, nx+nu), x_t / u_t row t of the state / control
        block of z (x_t: the state the t-th step arrives at).  lo / hi (nc,) for every step or (H,nc) per step, None or -+inf =
        no limit on that side, lo < hi on every entry.  Host arrays, copied.  bind_rows() with nothing removes the binding.
        eval / hess / rollout do not read it; kkt_residual, sensitivity, kkt_solve and solve(return_duals=True) refuse while it
        is on, and so does a solve with bind_rate, bind_tracking or bind_bounds.  At convergence every row holds to
        tol_constraint * (1 + |Cx row|_1)."""
        fn = getattr(self.lib, "nempc_bind_stage_rows", None)
        if fn is None:
            raise RuntimeError("this libnempc.so has no nempc_bind_stage_rows")
        if C is None:
            if lo is not None or hi is not None:
                raise ValueError("bind_rows: lo / hi need C")
            _lib.check(fn(self._handle, 0, None, None, None, 0))
            self._rows = None
            return
        if self.rolling_window > 1:
            raise ValueError("bind_rows: rolling-window models are not supported")
        Ca, lo, hi, per_stage = check_rows_args(self.H, self.nx, self.nu, C, lo, hi)
        ptr = lambda a: None if a is None else _as_c_double(a)[1]
        _lib.check(fn(self._handle, int(Ca.shape[0]), ptr(Ca), ptr(lo), ptr(hi), per_stage))
        self._rows = dict(C=Ca, lo=lo, hi=hi)

    def _bind_rows(self, bind, what, order, xpair, upair, offset):
        """bind_tracking / bind_bounds: check the (B,L,d) device tensors (xpair: the two of width nx, upair: of width nu),
        settle one leading dimension per pair and hand the row-`offset` pointers to the C function `bind` in its argument
        `order`.  -> what to keep alive and rebind with, or None when nothing was given."""
        H, given = self.H, {}
        offset = int(offset)
        dims = {k: self.nx for k, _ in xpair}
        dims.update({k: self.nu for k, _ in upair})
        for name, t in xpair + upair:
            d = dims[name]
            if t is None:
                continue
            if (not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype != self.dtype or t.dim() != 3
                    or t.shape[2] != d or offset < 0 or t.shape[1] < offset + H or t.shape[0] < 1):
                raise ValueError(f"{name} must be a {self.dtype} tensor (B,L,{d}) on {self.device} with L >= offset + H = "
                                 f"{offset + H}, got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
            if t.stride(2) != 1 or t.stride(1) != d or (t.shape[0] > 1 and t.stride(0) < t.shape[1] * d):
                t = t.contiguous()
            given[name] = t
        if not given:
            _lib.check(bind(self._handle, None, None, None, None, 0, 0, 0))
            return None
        if len({int(t.shape[0]) for t in given.values()}) != 1:
            raise ValueError(f"the bound {what} tensors must cover the same batch")
        ld = {}
        for key, pair, d in (("x", xpair, self.nx), ("u", upair, self.nu)):
            names = tuple(k for k, _ in pair)
            ts = [given[k] for k in names if k in given]
            lds = {int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1]) * d for t in ts}
            if len(lds) > 1:     # one leading dimension per pair in the C interface
                for k in names:
                    if k in given:
                        given[k] = given[k].contiguous()
                lds = {int(given[k].shape[1]) * d for k in names if k in given}
                if len(lds) > 1:
                    raise ValueError(f"{names[0]} and {names[1]} must have the same length L")
            ld[key] = lds.pop() if lds else 0
        esz = 8 if self.dtype == torch.float64 else 4
        ptr = lambda k: (ctypes.c_void_p(given[k].data_ptr() + offset * dims[k] * esz) if k in given else None)
        B = int(next(iter(given.values())).shape[0])
        _lib.check(bind(self._handle, *[ptr(k) for k in order], B, ld["x"], ld["u"]))
        return (given, offset)

    def _check_extra(self, B):
        if self.n_extra and (self._extra is None or self._extra.shape[0] < B):
            raise ValueError("n_extra > 0: call bind_extra with a (B,H,n_extra) tensor covering the batch first")
        if self.rolling_window > 1 and (self._history is None or self._history[0].shape[0] < B):
            raise ValueError("You must give history window with set_prev_data before calling any inferance function.")

    def set_box_rows(self, lo, hi):
        self._drop_buffers()        # m changes: the next evaluation allocates (and registers) afresh
        if lo is None:
            _lib.check(self.lib.nempc_set_box_rows(self._handle, 0, None, None))
            self._box = None
        else:
            a, pa = _as_c_double(np.broadcast_to(np.asarray(lo, dtype=np.float64), (self.nx,)))
            b, pb = _as_c_double(np.broadcast_to(np.asarray(hi, dtype=np.float64), (self.nx,)))
            _lib.check(self.lib.nempc_set_box_rows(self._handle, 1, pa, pb))
            self._box = (lo, hi)
        self._refresh_dims()

    # ------------------------------------------------------------------ structure / bounds (host)
    def constraint_bounds(self):
        cl, cu = np.empty(self.m), np.empty(self.m)
        dp = ctypes.POINTER(ctypes.c_double)
        _lib.check(self.lib.nempc_constraint_bounds(self._handle, cl.ctypes.data_as(dp), cu.ctypes.data_as(dp)))
        return cl, cu

    def jac_structure(self):
        r, c = np.empty(self.nnz_jac, dtype=np.int32), np.empty(self.nnz_jac, dtype=np.int32)
        ip = ctypes.POINTER(ctypes.c_int32)
        _lib.check(self.lib.nempc_jac_structure(self._handle, r.ctypes.data_as(ip), c.ctypes.data_as(ip)))
        return r, c

    def hess_structure(self):
        r, c = np.empty(self.nnz_hess, dtype=np.int32), np.empty(self.nnz_hess, dtype=np.int32)
        ip = ctypes.POINTER(ctypes.c_int32)
        _lib.check(self.lib.nempc_hess_structure(self._handle, r.ctypes.data_as(ip), c.ctypes.data_as(ip)))
        return r, c

    # ------------------------------------------------------------------ evaluation
    def _check_in(self, t, shape, name):
        if not isinstance(t, torch.Tensor) or t.device != self.device or t.dtype != self.dtype:
            raise ValueError(f"{name} must be a {self.dtype} tensor on {self.device}")
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")

    def _out(self, name, shape):
        key = (name, tuple(shape))
        buf = self._buffers.get(key)
        if buf is None:
            buf = torch.empty(shape, dtype=self.dtype, device=self.device)
            self._buffers[key] = buf
            if name == "jac_dense":
                # the engine's own dense Jacobian is written by nempc_eval of this handle and by nobody else: a resident
                # buffer (nempc_jac_dense_resident zero-fills it now; the first evaluation adds the constant -1 / +1 entries,
                # and every evaluation writes the computed non-zeros only).
                # A full table or a failed registration leaves it on the full-matrix path, which is correct as well.
                fn = getattr(self.lib, "nempc_jac_dense_resident", None)
                if fn is not None:
                    with torch.cuda.device(self.device):
                        fn(self._handle, ctypes.c_void_p(buf.data_ptr()), int(shape[0]))
        return buf

    def _drop_buffers(self):
        """Forget the reusable output tensors.  A registered dense Jacobian is unregistered first: once the tensor is gone
        the allocator may hand its address to somebody else, and a registration left behind would let an evaluation
        into that address skip the zeros."""
        fn = getattr(self.lib, "nempc_jac_dense_resident", None)
        if fn is not None and self._handle:
            for (name, _), buf in self._buffers.items():
                if name == "jac_dense":
                    fn(self._handle, ctypes.c_void_p(buf.data_ptr()), 0)
        self._buffers = {}

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def eval(self, Z, X0, want=("f", "grad", "g", "jac_dense"), out=None):
        """One batched callback evaluation.  Z (B,n), X0 (B,nx) device tensors.  Returns a dict with
        the requested outputs (device tensors, reused between calls unless `out` supplies them):
        f (B,), grad (B,n), g (B,m), jac_dense (B,m,n), jac_tiles (B,H,nx,w*(nx+nu)), jac_sparse (B,nnz_jac).
        Asynchronous on the current torch stream.
        The engine's own output tensors are READ-ONLY for the caller: its jac_dense is a resident buffer whose structural
        zeros and constant -1 / +1 entries are written once, and every evaluation writes the computed non-zeros only --
        whatever a caller writes into it stays there.  Tensors passed through `out` are the caller's: they get the full matrix every call."""
        B = int(Z.shape[0])
        self._check_in(Z, (B, self.n), "Z")
        self._check_in(X0, (B, self.nx), "X0")
        self._check_extra(B)
        self.reserve(B)
        shapes = {"f": (B,), "grad": (B, self.n), "g": (B, self.m), "jac_dense": (B, self.m, self.n),
                  "jac_tiles": (B, self.H, self.nx, self.nin), "jac_sparse": (B, self.nnz_jac)}
        res, ptr = {}, {}
        for k in shapes:
            if k in want:
                t = out[k] if (out is not None and k in out) else self._out(k, shapes[k])
                self._check_in(t, shapes[k], k)
                res[k] = t
                ptr[k] = ctypes.c_void_p(t.data_ptr())
            else:
                ptr[k] = None
        unknown = set(want) - set(shapes)
        if unknown:
            raise ValueError(f"unknown outputs requested: {sorted(unknown)}")
        with torch.cuda.device(self.device):
            _lib.check(self.lib.nempc_eval(self._handle, B, ctypes.c_void_p(Z.data_ptr()),
                                           ctypes.c_void_p(X0.data_ptr()), ptr["f"], ptr["grad"], ptr["g"],
                                           ptr["jac_dense"], ptr["jac_tiles"], ptr["jac_sparse"], self._stream()))
        return res

    def bind(self, Z, X0, want=("f", "grad", "g", "jac_dense"), out=None):
        """Pre-validated evaluation for hot loops: returns (launch, outputs) where launch() re-evaluates the
        callbacks at the CURRENT contents of Z / X0 into the fixed `outputs` tensors (caller-supplied through `out`,
        else the engine's reusable buffers) with one ctypes call (no per-call allocation or checking).  Valid while
        Z, X0 and the outputs stay alive and the workspaces are not re-sized (reserve / set_box_rows).
        As with eval, outputs the engine owns are read-only for the caller; outputs passed through `out` may be
        overwritten between launches (each launch rewrites them in full)."""
        B = int(Z.shape[0])
        res = self.eval(Z, X0, want, out=out)             # validates, allocates outputs, warms the kernels
        ptr = {k: (ctypes.c_void_p(res[k].data_ptr()) if k in res else None)
               for k in ("f", "grad", "g", "jac_dense", "jac_tiles", "jac_sparse")}
        handle, fn = self._handle, self.lib.nempc_eval
        zp, xp = ctypes.c_void_p(Z.data_ptr()), ctypes.c_void_p(X0.data_ptr())
        stream = self._stream()
        args = (handle, B, zp, xp, ptr["f"], ptr["grad"], ptr["g"], ptr["jac_dense"], ptr["jac_tiles"],
                ptr["jac_sparse"], stream)

        def launch():
            rc = fn(*args)
            if rc:
                _lib.check(rc)
        return launch, res

    def hess(self, Z, X0, lam, sigma, want=("hvals",)):
        """Lagrangian Hessian: hvals (B,nnz_hess) in hess_structure() order, optional hdense (B,n,n)
        and hblocks (B,H,w*(nx+nu),w*(nx+nu))."""
        B = int(Z.shape[0])
        self._check_in(Z, (B, self.n), "Z")
        self._check_in(X0, (B, self.nx), "X0")
        self._check_in(lam, (B, self.m), "lam")
        self._check_in(sigma, (B,), "sigma")
        self._check_extra(B)
        self.reserve(B)
        shapes = {"hvals": (B, self.nnz_hess), "hdense": (B, self.n, self.n),
                  "hblocks": (B, self.H, self.nin, self.nin)}
        res, ptr = {}, {}
        for k in shapes:
            if k in want:
                res[k] = self._out(k, shapes[k])
                ptr[k] = ctypes.c_void_p(res[k].data_ptr())
            else:
                ptr[k] = None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.nempc_hess(self._handle, B, ctypes.c_void_p(Z.data_ptr()),
                                           ctypes.c_void_p(X0.data_ptr()), ctypes.c_void_p(lam.data_ptr()),
                                           ctypes.c_void_p(sigma.data_ptr()), ptr["hvals"], ptr["hdense"],
                                           ptr["hblocks"], self._stream()))
        return res

    def hess_gn(self, Z, X0, w=None, sigma=None, want=("hvals",)):
        """Gauss-Newton Hessian (nempc_hess_gn): sigma * d2f + sum_t T_t^T diag(w_t) T_t in hess_structure() order, from
        the first-order tiles only.  w (B, H*nx) weights per defect row (None = ones), sigma (B,) (None = ones)."""
        B = int(Z.shape[0])
        self._check_in(Z, (B, self.n), "Z")
        self._check_in(X0, (B, self.nx), "X0")
        if w is not None:
            self._check_in(w, (B, self.H * self.nx), "w")
        if sigma is None:
            sigma = torch.ones(B, dtype=self.dtype, device=self.device)
        self._check_in(sigma, (B,), "sigma")
        self._check_extra(B)
        self.reserve(B)
        shapes = {"hvals": (B, self.nnz_hess), "hdense": (B, self.n, self.n),
                  "hblocks": (B, self.H, self.nin, self.nin)}
        res, ptr = {}, {}
        for k in shapes:
            if k in want:
                res[k] = self._out("gn_" + k, shapes[k])
                ptr[k] = ctypes.c_void_p(res[k].data_ptr())
            else:
                ptr[k] = None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.nempc_hess_gn(self._handle, B, ctypes.c_void_p(Z.data_ptr()),
                                              ctypes.c_void_p(X0.data_ptr()),
                                              None if w is None else ctypes.c_void_p(w.data_ptr()),
                                              ctypes.c_void_p(sigma.data_ptr()), ptr["hvals"], ptr["hdense"],
                                              ptr["hblocks"], self._stream()))
        return res

    def bind_hess(self, Z, X0, lam, sigma, want=("hvals",), gauss_newton=False):
        """Pre-validated Hessian callback for hot loops (the counterpart of bind): returns (launch, outputs); launch()
        re-evaluates the callback at the CURRENT contents of Z / X0 / lam / sigma into the fixed outputs with one ctypes
        call.  gauss_newton=True binds nempc_hess_gn, `lam` then being the (B, H*nx) row weights or None."""
        B = int(Z.shape[0])
        res = self.hess_gn(Z, X0, lam, sigma, want) if gauss_newton else self.hess(Z, X0, lam, sigma, want)
        if gauss_newton and sigma is None:
            raise ValueError("bind_hess: pass sigma explicitly (the bound call reads the tensor every time)")
        ptr = {k: (ctypes.c_void_p(res[k].data_ptr()) if k in res else None) for k in ("hvals", "hdense", "hblocks")}
        fn = self.lib.nempc_hess_gn if gauss_newton else self.lib.nempc_hess
        args = (self._handle, B, ctypes.c_void_p(Z.data_ptr()), ctypes.c_void_p(X0.data_ptr()),
                None if lam is None else ctypes.c_void_p(lam.data_ptr()), ctypes.c_void_p(sigma.data_ptr()),
                ptr["hvals"], ptr["hdense"], ptr["hblocks"], self._stream())

        def launch():
            rc = fn(*args)
            if rc:
                _lib.check(rc)
        return launch, res

    @property
    def last_rollout_kernel(self):
        """Name of the kernel the most recent roll-out launched."""
        return self.ROLLOUT_KERNELS[self.lib.nempc_last_rollout_kernel(self._handle)]

    def rollout(self, X0, U=None, Z=None, want_f=False):
        """Forward simulation of the model on the device (nempc_rollout): x_t = Phi(x_{t-1}, u_t), x_{-1} = X0, one launch
        for the whole horizon.  X0 (B,nx); the controls come from U (B,H,nu) or (B,H*nu), or from the control part of Z (B,n),
        which is then updated IN PLACE (its states are overwritten and never read); neither = zero controls.  Returns
        Z (B,n) = [rolled-out states | controls], or (Z, f (B,)) with the objective at that point when want_f.
        Asynchronous on the current torch stream."""
        B = int(X0.shape[0])
        self._check_in(X0, (B, self.nx), "X0")
        if U is not None and Z is not None:
            raise ValueError("rollout: pass U or Z, not both")
        if Z is not None:
            self._check_in(Z, (B, self.n), "Z")
        else:
            Z = torch.zeros(B, self.n, dtype=self.dtype, device=self.device)
            if U is not None:
                if not isinstance(U, torch.Tensor) or U.device != self.device or U.dtype != self.dtype:
                    raise ValueError(f"U must be a {self.dtype} tensor on {self.device}")
                if tuple(U.shape) not in ((B, self.H, self.nu), (B, self.H * self.nu)):
                    raise ValueError(f"U must have shape {(B, self.H, self.nu)} or {(B, self.H * self.nu)}, got {tuple(U.shape)}")
                Z[:, self.H * self.nx:] = U.reshape(B, self.H * self.nu)
        self._check_extra(B)
        self.reserve(B)
        f = torch.empty(B, dtype=self.dtype, device=self.device) if want_f else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.nempc_rollout(self._handle, B, ctypes.c_void_p(X0.data_ptr()), ctypes.c_void_p(Z.data_ptr()),
                                              None if f is None else ctypes.c_void_p(f.data_ptr()), self._stream()))
        return (Z, f) if want_f else Z

    def solve(self, X0, Z_init=None, lb=None, ub=None, max_iter=200, max_linesearch=6, check_every=4,
              tol_constraint=None, tol_step=None, mu_init=1e-1, mu_min=None, mu_factor=0.2, reg=None, lq_kernel="auto",
              compact=True, return_iterations=False, barrier="primal-dual", linesearch="auto", lq_attempts=0, init="tile",
              return_duals=False):
        """Batched on-device solve (Gauss-Newton SQP, see csrc/solver.hip).  X0 (B,nx) device tensor; Z_init (B,n)
        or None for the reference's cold start [x0 tiled H ; zeros] (optimizer/ipopt.py:149); init="rollout" makes the start
        dynamically feasible instead: the states of the start (Z_init's, or of zero controls) are replaced by the roll-out of
        its controls (`rollout`; the solver moves a start outside the bounds into their interior itself); lb/ub (n) host
        vectors as DomainConstraint produces them; tolerances default by dtype (fp64 1e-8, fp32 1e-4); lq_kernel picks the LQ solve ("auto" | "thread" per problem | "wave"
        per problem | "scan": parallel in time, 2/1 stages in fp64); compact=True gathers the unconverged problems to the front as the batch converges (same results,
        shorter launches); linesearch "loop" backtracks inside an iteration (every problem waits for the slowest search),
        "deferred" tries one step length per iteration and lets a rejected problem retry at half the length in the next one
        (about half the time per iteration at the 2/1 shape, more iterations for hard problems), "auto" defers for small
        stages and loops for matrix-core-bound ones; lq_attempts bounds the Riccati sweeps a problem may try per iteration
        (0: the library's default of 3).  Returns (Z (B,n), status (B,) int32 [0 ok / 1 fail], iters) [+ per-problem convergence
        iteration (B,) int32 with return_iterations=True] [+ with return_duals=True, last, the multipliers the returned
        iterates carry (nempc_solve_duals): {"lam": (B,m), "zl": (B,n), "zu": (B,n)} device tensors in the convention
        grad f + J' lam - zl + zu = 0, zl, zu >= 0; lam goes straight into `hess` and `kkt_residual`]."""
        B = int(X0.shape[0])
        self._check_in(X0, (B, self.nx), "X0")
        self._check_extra(B)
        self.reserve(B)
        # tolerances an iterate of the handle's precision can reach (fp32 stalls near 1e-5 relative)
        f64 = self.dtype == torch.float64
        tol_constraint = (1e-8 if f64 else 1e-4) if tol_constraint is None else tol_constraint
        tol_step = (1e-8 if f64 else 1e-4) if tol_step is None else tol_step
        mu_min = (1e-9 if f64 else 1e-5) if mu_min is None else mu_min
        reg = (1e-9 if f64 else 1e-6) if reg is None else reg
        if init not in ("tile", "rollout"):
            raise ValueError("init must be 'tile' or 'rollout'")
        if Z_init is None and init == "rollout":
            Z = self.rollout(X0)
        elif Z_init is None:
            Z = torch.cat([X0.repeat(1, self.H), torch.zeros(B, self.H * self.nu, dtype=self.dtype, device=self.device)],
                          dim=1).contiguous()
        else:
            self._check_in(Z_init, (B, self.n), "Z_init")
            Z = Z_init.clone()
            if init == "rollout":
                self.rollout(X0, Z=Z)
        keep = []
        ptrs = [self._host_vector(v, keep) for v in (lb, ub)]
        its_dev = torch.zeros(B, dtype=torch.int32, device=self.device) if return_iterations else None
        opts = _lib.NempcSolverOpts(max_iter=max_iter, max_linesearch=max_linesearch, check_every=check_every,
                                    lq_kernel={"auto": 0, "thread": 1, "wave": 2, "scan": 3}[lq_kernel],
                                    tol_constraint=tol_constraint, tol_step=tol_step, mu_init=mu_init, mu_min=mu_min,
                                    mu_factor=mu_factor, reg=reg, compact=1 if compact else 0,
                                    barrier={"primal-dual": 0, "primal": 1}[barrier],
                                    iters_out=None if its_dev is None else its_dev.data_ptr(),
                                    linesearch={"auto": 0, "loop": 1, "deferred": 2}[linesearch], lq_attempts=int(lq_attempts))
        status = torch.empty(B, dtype=torch.int32, device=self.device)
        iters = ctypes.c_int32(0)
        duals = None
        if return_duals:
            duals = {"lam": torch.empty(B, self.m, dtype=self.dtype, device=self.device),
                     "zl": torch.empty(B, self.n, dtype=self.dtype, device=self.device),
                     "zu": torch.empty(B, self.n, dtype=self.dtype, device=self.device)}
        with torch.cuda.device(self.device):
            if duals is None:
                _lib.check(self.lib.nempc_solve(self._handle, B, ctypes.c_void_p(X0.data_ptr()), ctypes.c_void_p(Z.data_ptr()),
                                                ptrs[0], ptrs[1], ctypes.byref(opts), ctypes.c_void_p(status.data_ptr()),
                                                ctypes.byref(iters), self._stream()))
            else:
                _lib.check(self.lib.nempc_solve_duals(self._handle, B, ctypes.c_void_p(X0.data_ptr()),
                                                      ctypes.c_void_p(Z.data_ptr()), ptrs[0], ptrs[1], ctypes.byref(opts),
                                                      ctypes.c_void_p(status.data_ptr()), ctypes.byref(iters),
                                                      ctypes.c_void_p(duals["lam"].data_ptr()),
                                                      ctypes.c_void_p(duals["zl"].data_ptr()),
                                                      ctypes.c_void_p(duals["zu"].data_ptr()), self._stream()))
        res = (Z, status, iters.value) + ((its_dev,) if return_iterations else ()) + ((duals,) if return_duals else ())
        return res

    def _host_vector(self, v, keep):
        """lb / ub: (n) host vector (or what broadcasts to one) -> pointer to doubles for the C ABI, None stays None; the
        array the pointer names goes into `keep`"""
        if v is None:
            return None
        a, p = _as_c_double(np.broadcast_to(np.asarray(v, dtype=np.float64), (self.n,)))
        keep.append(a)
        return p

    def _check_point(self, B, Z, X0, lam, zl, zu):
        self._check_in(Z, (B, self.n), "Z")
        self._check_in(X0, (B, self.nx), "X0")
        self._check_in(lam, (B, self.m), "lam")
        for name, t in (("zl", zl), ("zu", zu)):
            if t is not None:
                self._check_in(t, (B, self.n), name)

    def _point(self, Z, X0, lam, zl, zu, lb, ub, checked=False):
        """A primal-dual point for nempc_kkt_residual / nempc_sensitivity / nempc_kkt_solve: shape checks (unless the caller
        made them, with checks of its own behind them), bound extras, workspaces for the batch.  -> (B, the seven C
        arguments after B, the host arrays to keep alive over the call)."""
        B = int(Z.shape[0])
        if not checked:
            self._check_point(B, Z, X0, lam, zl, zu)
        if self.rolling_window == 1:      # (a rolling-window handle is refused by the library, history bound or not)
            self._check_extra(B)
        self.reserve(B)
        keep = []
        bounds = [self._host_vector(v, keep) for v in (lb, ub)]
        return B, (_ptr(Z), _ptr(X0), _ptr(lam), _ptr(zl), _ptr(zu), *bounds), keep

    def kkt_residual(self, Z, X0, lam, zl=None, zu=None, lb=None, ub=None, want_stat=False):
        """KKT residuals of B primal-dual points (nempc_kkt_residual; any points, a solver's or not).  Z (B,n), X0 (B,nx),
        lam (B,m) device tensors; zl, zu (B,n) multipliers of z >= lb, z <= ub or None (zeros); lb / ub (n) host vectors as in
        `solve` (None = unbounded; box rows are intersected).  Returns r (B,4) = [stationarity |grad f + J' lam - zl + zu|_inf,
        primal feasibility, complementarity, dual feasibility] per problem, or (r, stat (B,n)) with the stationarity vector
        when want_stat (the engine's own output tensors, reused between calls like `eval`'s).  One callback evaluation and
        one reduction kernel; asynchronous on the current torch stream."""
        B, point, keep = self._point(Z, X0, lam, zl, zu, lb, ub)
        r = self._out("kkt_r", (B, 4))
        stat = self._out("kkt_stat", (B, self.n)) if want_stat else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.nempc_kkt_residual(self._handle, B, *point, _ptr(r), _ptr(stat), self._stream()))
        return (r, stat) if want_stat else r

    def sensitivity(self, Z, X0, lam, zl=None, zu=None, lb=None, ub=None, want=("du0",)):
        """Solution sensitivities with respect to the initial state at B primal-dual points (nempc_sensitivity; any points,
        a solver's or not).  Inputs as `kkt_residual`.  want: any of "du0" (B,nu,nx) du_0*/dx0 = K_0 -- the feedback gain of
        u = u0* + K0 (x_measured - x0) --, "dz" (B,n,nx) rows dz_i/dx0 in z order, "dlam" (B,H*nx,nx), "gains" (B,H,nu,nx)
        the time-varying K_t with du_t = K_t dx_{t-1}.  Returns a dict of new device tensors with those keys plus "status" (B,)
        int32: 0 ok; 1 some Quu_t is not positive definite (not a strict local minimiser; nothing is regularised); 2 a
        non-zero bound multiplier on a gap <= 0.  Outputs of a problem with status != 0 are NaN.  The sweep runs in double
        whatever the engine's dtype.  One evaluation, one Hessian-block launch and one sweep kernel; asynchronous on the
        current torch stream."""
        names = ("du0", "dz", "dlam", "gains")
        want = tuple(want)
        if not want or any(k not in names for k in want):
            raise ValueError(f"want must name at least one of {names}")
        B, point, keep = self._point(Z, X0, lam, zl, zu, lb, ub)
        shapes = {"du0": (B, self.nu, self.nx), "dz": (B, self.n, self.nx), "dlam": (B, self.H * self.nx, self.nx),
                  "gains": (B, self.H, self.nu, self.nx)}
        res = {k: torch.empty(shapes[k], dtype=self.dtype, device=self.device) for k in want}
        res["status"] = torch.empty(B, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self.lib.nempc_sensitivity(self._handle, B, *point, _ptr(res.get("du0")), _ptr(res.get("dz")),
                                                  _ptr(res.get("dlam")), _ptr(res.get("gains")), _ptr(res["status"]),
                                                  self._stream()))
        return res

    def kkt_solve(self, Z, X0, lam, zl=None, zu=None, lb=None, ub=None, rz=None, rg=None, want=("v",)):
        """Solves K [v ; w] = [rz ; rg] with the symmetric KKT matrix K = [[W + Sigma, J'], [J, 0]] of B primal-dual points
        (nempc_kkt_solve; any points, a solver's or not).  Inputs as `sensitivity`.  rz (B,n) -- one right-hand side per
        problem, the outputs then lose that axis -- or (B,k,n) with any k (the library takes 64 per call; larger sets go in
        chunks), in z order; rg (B,H*nx) / (B,k,H*nx) in defect order or None (zeros).  want: any of "v" (B,k,n), "w"
        (B,k,H*nx), "gx0" (B,k,nx) = -[v ; w]' d/dx0 [grad L ; g].  With rz the cotangent of z* (rg None), gx0 is the cotangent
        of x0 and v carries those of the tracking data (pyneuralempc_amd.autograd); with the right-hand side
        -d/dtheta [grad L ; g], v and w are dz*/dtheta and dlam/dtheta.  Returns a dict of new device tensors with those keys
        plus "status" (B,) int32 as `sensitivity`'s; outputs of a problem with status != 0 are NaN.  Asynchronous on the
        current torch stream, except that a call whose working sets do not fit on chip allocates (and synchronises the
        device) when k or the batch grow."""
        names = ("v", "w", "gx0")
        want = tuple(want)
        if not want or any(k not in names for k in want):
            raise ValueError(f"want must name at least one of {names}")
        if rz is None:
            raise ValueError("rz is required")
        B, hx = int(Z.shape[0]), self.H * self.nx
        self._check_point(B, Z, X0, lam, zl, zu)
        single = rz.dim() == 2
        if single:
            rz = rz.unsqueeze(1)
            rg = None if rg is None else rg.unsqueeze(1)
        if rz.dim() != 3 or rz.shape[1] < 1:
            raise ValueError(f"rz must be (B,{self.n}) or (B,k,{self.n}) with k >= 1")
        k = int(rz.shape[1])
        self._check_in(rz, (B, k, self.n), "rz")
        if rg is not None:
            self._check_in(rg, (B, k, hx), "rg")
        B, point, keep = self._point(Z, X0, lam, zl, zu, lb, ub, checked=True)
        shapes = {"v": (B, k, self.n), "w": (B, k, hx), "gx0": (B, k, self.nx)}
        res = {key: torch.empty(shapes[key], dtype=self.dtype, device=self.device) for key in want}
        res["status"] = torch.empty(B, dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            for c0 in range(0, k, 64):
                c1 = min(k, c0 + 64)
                whole = c0 == 0 and c1 == k
                rzc = rz.contiguous() if whole else rz[:, c0:c1].contiguous()
                rgc = None if rg is None else (rg.contiguous() if whole else rg[:, c0:c1].contiguous())
                outs = {key: (res[key] if whole else torch.empty((B, c1 - c0) + shapes[key][2:], dtype=self.dtype, device=self.device))
                        for key in want}
                _lib.check(self.lib.nempc_kkt_solve(self._handle, B, *point, c1 - c0, _ptr(rzc), _ptr(rgc), _ptr(outs.get("v")),
                                                    _ptr(outs.get("w")), _ptr(outs.get("gx0")), _ptr(res["status"]), self._stream()))
                if not whole:
                    for key in want:
                        res[key][:, c0:c1] = outs[key]
        if single:
            for key in want:
                res[key] = res[key][:, 0]
        return res

    # ------------------------------------------------------------------ the network's weights as parameters
    @property
    def n_params(self):
        """P = sum_l (in_l + 1) * out_l (nempc_n_params): the length of `weight_grad`'s flat result"""
        P = ctypes.c_int64()
        _lib.check(self._wgrad_fn("nempc_n_params")(self._handle, ctypes.byref(P)))
        return int(P.value)

    def _wgrad_fn(self, name):
        fn = getattr(self.lib, name, None)
        if fn is None:
            raise RuntimeError(f"the loaded libnempc.so has no {name}; rebuild it")
        return fn

    def set_weights(self, weights, biases):
        """Replace the network's weights and biases (nempc_set_weights on the live handle: objective, bindings, workspaces
        stay).  Shapes must be those the engine was built with.  Synchronises the device first: the library frees and
        re-allocates its weight buffers, and queued work may still read them."""
        ws = [np.ascontiguousarray(w, dtype=np.float64) for w in weights]
        bs = [np.ascontiguousarray(b, dtype=np.float64).reshape(-1) for b in biases]
        if len(ws) != len(self._weights) or len(bs) != len(self._biases):
            raise ValueError(f"expected {len(self._weights)} weight matrices and as many biases")
        for l, (w, b) in enumerate(zip(ws, bs)):
            if w.shape != self._weights[l].shape or b.shape != self._biases[l].shape:
                raise ValueError(f"layer {l}: expected kernel {self._weights[l].shape} and bias {self._biases[l].shape}, "
                                 f"got {w.shape} and {b.shape}")
        nl = len(ws)
        dp = ctypes.POINTER(ctypes.c_double)
        Wp = (dp * nl)(*[w.ctypes.data_as(dp) for w in ws])
        bp = (dp * nl)(*[b.ctypes.data_as(dp) for b in bs])
        torch.cuda.synchronize(self.device)
        _lib.check(self.lib.nempc_set_weights(self._handle, Wp, bp))
        self._weights, self._biases = ws, bs

    def weight_grad(self, Z, X0, w, lam=None, v=None, skip=None, flat=False):
        """gtheta = d/dtheta sum_b sum_t ( w_{b,t} . Phi_t + lam_{b,t} . (T_t v_{b,[t]}) ), theta = the network's weights and
        biases (nempc_weight_grad; Z, X0, lam, v, w held fixed).  Z (B,n), X0 (B,nx), w (B,H*nx) in defect order; lam (B,m)
        and v (B,n) both or neither -- without them the second term drops and the result is the gradient of a defect-weighted
        loss; with `kkt_solve`'s (v, w) the cotangent of theta behind the solution is -gtheta.  skip (B,) int32 or bool, or
        None: problems with a non-zero entry contribute exact zeros, whatever (NaN included) their lam / v / w hold.  Returns
        [(dW_0, db_0), (dW_1, db_1), ...] as views of one new flat device tensor in the layout of the weights, or that tensor
        (n_params,) with flat=True.  Bitwise reproducible from call to call.  Asynchronous on the current torch stream, except
        a call that has to allocate or grow the handle's workspace for it (the first one)."""
        fn = self._wgrad_fn("nempc_weight_grad")
        B = int(Z.shape[0])
        self._check_in(Z, (B, self.n), "Z")
        self._check_in(X0, (B, self.nx), "X0")
        self._check_in(w, (B, self.H * self.nx), "w")
        if (lam is None) != (v is None):
            raise ValueError("lam and v are given both or neither")
        if lam is not None:
            self._check_in(lam, (B, self.m), "lam")
            self._check_in(v, (B, self.n), "v")
        if skip is not None:
            if not isinstance(skip, torch.Tensor) or skip.device != self.device or tuple(skip.shape) != (B,):
                raise ValueError(f"skip must be a ({B},) tensor on {self.device}")
            skip = skip.to(torch.int32).contiguous()
        if self.rolling_window == 1:      # (a rolling-window handle is refused by the library, history bound or not)
            self._check_extra(B)
        self.reserve(B)
        g = torch.empty(self.n_params, dtype=self.dtype, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(fn(self._handle, B, _ptr(Z), _ptr(X0), _ptr(lam), _ptr(v), _ptr(w), _ptr(skip), _ptr(g), self._stream()))
        if flat:
            return g
        out, at = [], 0
        for wl in self._weights:
            i, o = wl.shape
            out.append((g[at:at + i * o].view(i, o), g[at + i * o:at + (i + 1) * o]))
            at += (i + 1) * o
        return out

    # ------------------------------------------------------------------ the extra inputs p / tvp as parameters
    EXTRA_GRAD_KERNELS = {0: None, 1: "egrad_rows_kernel<1 lane, lds>", 2: "egrad_rows_kernel<16 lanes, lds>",
                          3: "egrad_rows_kernel<64 lanes, lds>", 5: "egrad_rows_kernel<1 lane, workspace>",
                          6: "egrad_rows_kernel<16 lanes, workspace>", 7: "egrad_rows_kernel<64 lanes, workspace>"}

    def extra_grad(self, Z, X0, w, lam=None, v=None):
        """gE[b,t,:] = d/d e_{b,t} ( w_{b,t} . Phi_t + lam_{b,t} . (T_t v_{b,[t]}) ), e_{b,t} row (b,t) of the tensor bound with
        `bind_extra` (nempc_extra_grad; Z, X0, lam, v, w and the weights held fixed) -- per row, no sum over t or b: the
        gradient of a constant parameter p is the caller's sum over t of its slots.  Z (B,n), X0 (B,nx), w (B,H*nx) in defect
        order; lam (B,m) and v (B,n) both or neither -- without them the result is w' dPhi/de, the gradient of a
        defect-weighted loss; with `kkt_solve`'s (v, w) the cotangent of the extras behind the solution is -gE.  Returns a new
        (B,H,n_extra) device tensor.  Problems are independent and the call is bitwise reproducible.  Asynchronous on the
        current torch stream, except a first call that has to allocate the handle's workspace for it."""
        fn = self._wgrad_fn("nempc_extra_grad")
        B = int(Z.shape[0])
        self._check_in(Z, (B, self.n), "Z")
        self._check_in(X0, (B, self.nx), "X0")
        self._check_in(w, (B, self.H * self.nx), "w")
        if (lam is None) != (v is None):
            raise ValueError("lam and v are given both or neither")
        if lam is not None:
            self._check_in(lam, (B, self.m), "lam")
            self._check_in(v, (B, self.n), "v")
        if self.rolling_window == 1 and self.n_extra:      # (a rolling-window or n_extra = 0 handle is refused by the library)
            self._check_extra(B)
        self.reserve(B)
        g = torch.empty((B, self.H, self.n_extra), dtype=self.dtype, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(fn(self._handle, B, _ptr(Z), _ptr(X0), _ptr(lam), _ptr(v), _ptr(w), _ptr(g), self._stream()))
        return g

    @property
    def last_extra_grad_kernel(self):
        """Launch form of the most recent `extra_grad` (nempc_last_extra_grad_kernel): lanes per row, and where the saved
        activation derivatives lived; None before the first call."""
        return self.EXTRA_GRAD_KERNELS[self._wgrad_fn("nempc_last_extra_grad_kernel")(self._handle)]

    def sync(self):
        _lib.check(self.lib.nempc_sync(self._handle, self._stream()))

    # ------------------------------------------------------------------ multi-GPU: the u0 all-gather on RCCL
    def comm_init(self, nranks, rank, unique_id):
        """Collective over the ranks: build this handle's RCCL communicator from the 128-byte id rank 0 obtained
        with `CallbackEngine.comm_unique_id()` (parallel.init_u0_comm moves it over torch.distributed)."""
        if len(unique_id) != _lib.COMM_ID_BYTES:
            raise ValueError(f"unique_id must be {_lib.COMM_ID_BYTES} bytes")
        buf = (ctypes.c_char * _lib.COMM_ID_BYTES).from_buffer_copy(bytes(unique_id))
        with torch.cuda.device(self.device):
            _lib.check(self.lib.nempc_comm_init(self._handle, int(nranks), int(rank), ctypes.cast(buf, ctypes.c_void_p)))
        self._comm = (int(nranks), int(rank))

    @staticmethod
    def comm_unique_id():
        buf = (ctypes.c_char * _lib.COMM_ID_BYTES)()
        _lib.check(_lib.load().nempc_comm_unique_id(ctypes.cast(buf, ctypes.c_void_p)))
        return bytes(buf)

    @property
    def comm(self):
        """(nranks, rank) of the handle's communicator, or None."""
        return getattr(self, "_comm", None)

    def allgather_u0(self, Z=None, u0=None, rows_per_rank=None, out=None):
        """nempc_allgather_u0: first controls of this rank's B problems -- read from Z (B,n) or given as u0 (B,nu) --
        gathered over the communicator into (nranks*rows_per_rank, nu), rank-major; asynchronous on the current
        stream.  rows_per_rank defaults to B (equal shards); ragged shards pass the largest shard size."""
        if self.comm is None:
            raise RuntimeError("allgather_u0: call comm_init first")
        if (Z is None) == (u0 is None):
            raise ValueError("pass exactly one of Z and u0")
        src = Z if Z is not None else u0
        B = int(src.shape[0])
        self._check_in(src, (B, self.n if Z is not None else self.nu), "Z" if Z is not None else "u0")
        rows = B if rows_per_rank is None else int(rows_per_rank)
        shape = (self.comm[0] * rows, self.nu)
        if out is None:
            out = self._out("u0_gathered", shape)
        self._check_in(out, shape, "out")
        zp = ctypes.c_void_p(Z.data_ptr()) if Z is not None else None
        up = ctypes.c_void_p(u0.data_ptr()) if u0 is not None else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.nempc_allgather_u0(self._handle, B, rows, zp, up, ctypes.c_void_p(out.data_ptr()),
                                                   self._stream()))
        return out

    def bind_allgather_u0(self, Z, stream=None, rows_per_rank=None):
        """Pre-validated all-gather for hot loops (the counterpart of `bind`): returns (launch, gathered) where launch()
        re-issues nempc_allgather_u0 on `stream` (a torch.cuda.Stream; default: the current one) at the CURRENT contents
        of Z with one ctypes call."""
        out = self.allgather_u0(Z=Z, rows_per_rank=rows_per_rank)          # validates, allocates, warms
        B = int(Z.shape[0])
        rows = B if rows_per_rank is None else int(rows_per_rank)
        st = ctypes.c_void_p((stream or torch.cuda.current_stream(self.device)).cuda_stream)
        args = (self._handle, B, rows, ctypes.c_void_p(Z.data_ptr()), None, ctypes.c_void_p(out.data_ptr()), st)
        fn = self.lib.nempc_allgather_u0

        def launch():
            rc = fn(*args)
            if rc:
                _lib.check(rc)
        return launch, out

    # ------------------------------------------------------------------ host convenience (B=1 drop-in path)
    def to_device(self, a):
        # (a read-only view -- np.broadcast_to -- is copied: torch refuses to alias memory it may not write)
        return torch.as_tensor(np.require(a, dtype=np.float64, requirements=["C", "W"])).to(self.device, self.dtype)

    def eval_numpy(self, Z, X0, want=("f", "grad", "g", "jac_dense")):
        Z = np.atleast_2d(np.asarray(Z, dtype=np.float64))
        X0 = np.atleast_2d(np.asarray(X0, dtype=np.float64))
        res = self.eval(self.to_device(Z), self.to_device(X0), want)
        return {k: v.to("cpu", torch.float64).numpy() for k, v in res.items()}
