"""Thin tensor-level wrappers over the C ABI.  PyTorch is used for device memory,
the current HIP stream and (elsewhere) torch.distributed -- nothing else.

Every function takes/returns torch tensors that live on the GPU; nothing here
synchronises with the host.
"""
import ctypes

import torch

from . import _lib
from ._lib import (SMOOTH_FIRST_ORDER, SMOOTH_ZERO_ORDER_AB, SMOOTH_ZERO_ORDER_B,
                   check, dbl_array)

F64 = torch.float64
F32 = torch.float32


def require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError("irs_mpc_amd needs an AMD GPU (no CPU fallback exists).")
    return torch.device("cuda", torch.cuda.current_device())


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t, dtype):
    if t is None:
        return None
    assert t.is_cuda and t.dtype == dtype and t.is_contiguous(), (t.device, t.dtype, t.is_contiguous())
    return t.data_ptr()


def _ws_args(ws):
    """The (pointer, bytes) pair of an optional workspace tensor."""
    return (ws.data_ptr(), ws.numel()) if ws is not None else (None, 0)


def _check_shapes(named):
    """Every (name, tensor, shape) of `named` names a tensor of that shape."""
    for name, t, shape in named:
        assert tuple(t.shape) == shape, (name, tuple(t.shape), shape)


def _outputs(out, shapes, device):
    """`out`, or freshly allocated tensors (name -> shape; `info` int32, the rest f64): checked to have those shapes."""
    o = out if out is not None else DeviceModel._tv_alloc(shapes, device)
    for name, shape in shapes.items():         # (in place: through _check_shapes this costs a microsecond per call)
        assert tuple(o[name].shape) == shape, (name, tuple(o[name].shape), shape)
    return o


def _descent_outputs(dm, T, lead, device, out=None, **given):
    """The outputs K, k, x_new, u_new, cost, info of a Riccati descent over T steps, of one problem (lead = ()) or of B
    (lead = (B,)): `out`, or fresh tensors with the `given` ones (x_new=, u_new=; None = fresh) in their places."""
    n, m = dm.n, dm.m
    shapes = dict(K=lead + (T, m, n), k=lead + (T, m), x_new=lead + (T + 1, n), u_new=lead + (T, m), cost=lead or (1,),
                  info=lead or (1,))
    given = {name: t for name, t in given.items() if t is not None}
    if out is None and given:
        out = DeviceModel._tv_alloc({name: shape for name, shape in shapes.items() if name not in given}, device)
        out.update(given)
    return _outputs(out, shapes, device)


def to_dev(a, dtype=F64):
    """numpy / tensor -> contiguous device tensor of `dtype`."""
    dev = require_gpu()
    if isinstance(a, torch.Tensor):
        return a.to(device=dev, dtype=dtype).contiguous()
    return torch.as_tensor(a).to(device=dev, dtype=dtype).contiguous()


def smooth_geometry(model_id, mode, T, N, rng=False):
    """The launch geometry of the sample pass for (model, mode, T, N) (irs_smooth_geometry): no launch, no device.
    dict(family, block, nblk, chunk0, chunk, wg0_rr, branch), family / branch by name (_lib.SMOOTH_FAMILIES / _PLANS)."""
    out = (ctypes.c_int * 8)()
    check(_lib.load().irs_smooth_geometry(int(model_id), int(mode), int(T), int(N), int(bool(rng)), out),
          "irs_smooth_geometry")
    return dict(family=_lib.SMOOTH_FAMILIES[out[0]], block=out[1], nblk=out[2], chunk0=out[3], chunk=out[4],
                wg0_rr=out[5], branch=_lib.SMOOTH_PLANS[out[6]])


class CemSource:
    """Where the B candidate sequences of a CEM operation come from (csrc/cem.hpp): `supplied` as a tensor, or `drawn`
    inside the kernels, never stored.  Knows B, T, m and the device; `args` is the run of C arguments that stands for
    the source in an entry -- every irs_cem_* entry comes as `name` taking the tensor and `name`_drawn taking the
    stream in the same place (`suffix` tells which) -- built once; the source keeps its tensors alive."""
    __slots__ = ("suffix", "B", "T", "m", "args", "tensors", "device")

    def __init__(self, suffix, B, T, m, args, tensors):
        self.suffix, self.B, self.T, self.m, self.args, self.tensors = suffix, B, T, m, args, tensors
        self.device = tensors[0].device

    @classmethod
    def supplied(cls, u_cand):
        """The candidates u_cand (B,T,m)."""
        B, T, m = u_cand.shape
        return cls("", B, T, m, (_ptr(u_cand, F64),), (u_cand,))

    @classmethod
    def drawn(cls, u_mean, std, B, seed, it, sample_offset=0):
        """Candidates sample_offset .. sample_offset + B of the stream of (seed, it), scaled by std (T,m) around
        u_mean (T,m) (include/irs_hip.h: irs_cem_candidates writes them out)."""
        T, m = u_mean.shape
        return cls("_drawn", int(B), T, m, (_ptr(u_mean, F64), _ptr(std, F64), int(seed), int(it), int(sample_offset)),
                   (u_mean, std))


def _quasistatic_weight(Qd):
    if Qd is None:
        raise ValueError("the quasistatic CEM cost needs Qd")
    return Qd


class CemModelFree:
    """The CEM surface of every class with a `lib` -- DeviceModel and torch_system.TorchDeviceModel -- over two
    primitives on a CemSource: cem_refit_from (selection + refit, which never see the plant) and the subclass's
    cem_costs(src, x0, Q, R, xd_trj, Qd=None) -> costs (B) of the candidates of `src`, rollout + evaluate_cost each
    or, with Qd, the quasistatic eval_cost (du input cost, terminal Qd)."""

    def cem_refit_from(self, src, costs, n_elite):
        """Elite selection + mean/std refit (a drawn source: the elites regenerated from their indices): returns
        elite_idx (n_elite), u_new (T,m), std_new (T,m), fresh tensors."""
        idx = torch.empty((n_elite,), dtype=torch.int32, device=src.device)
        u_new = torch.empty((src.T, src.m), dtype=F64, device=src.device)
        std_new = torch.empty((src.T, src.m), dtype=F64, device=src.device)
        name = "irs_cem_refit" + src.suffix
        check(getattr(self.lib, name)(src.T, src.m, src.B, int(n_elite), *src.args, _ptr(costs, F64), idx.data_ptr(),
                                      _ptr(u_new, F64), _ptr(std_new, F64), _stream()), name)
        return idx, u_new, std_new

    def cem_rollout_costs(self, u_cand, x0, Q, R, xd_trj):
        """costs (B) of the B candidate sequences u_cand (B,T,m): rollout + evaluate_cost each."""
        return self.cem_costs(CemSource.supplied(u_cand), x0, Q, R, xd_trj)

    def cem_rollout_costs_quasistatic(self, u_cand, x0, Q, Qd, R, xd_trj):
        """costs (B) with the quasistatic eval_cost (du input cost, terminal Qd)."""
        return self.cem_costs(CemSource.supplied(u_cand), x0, Q, R, xd_trj, Qd=_quasistatic_weight(Qd))

    # device-resident form: the candidates are drawn inside the kernels (include/irs_hip.h), never stored
    def cem_rollout_costs_drawn(self, u_mean, std, B, seed, it, x0, Q, R, xd_trj, sample_offset=0):
        """cem_rollout_costs of B candidates drawn around u_mean (T,m) with std (T,m): no (B,T,m) tensor."""
        return self.cem_costs(CemSource.drawn(u_mean, std, B, seed, it, sample_offset), x0, Q, R, xd_trj)

    def cem_rollout_costs_quasistatic_drawn(self, u_mean, std, B, seed, it, x0, Q, Qd, R, xd_trj, sample_offset=0):
        """cem_rollout_costs_quasistatic of B drawn candidates."""
        return self.cem_costs(CemSource.drawn(u_mean, std, B, seed, it, sample_offset), x0, Q, R, xd_trj,
                              Qd=_quasistatic_weight(Qd))

    def cem_refit(self, u_cand, costs, n_elite):
        """cem_refit_from on the candidates u_cand (B,T,m)."""
        return self.cem_refit_from(CemSource.supplied(u_cand), costs, n_elite)

    def cem_refit_drawn(self, u_mean, std, seed, it, costs, n_elite, sample_offset=0):
        """cem_refit_from on the costs.shape[0] candidates drawn around u_mean with std."""
        return self.cem_refit_from(CemSource.drawn(u_mean, std, costs.shape[0], seed, it, sample_offset), costs, n_elite)

    def cem_candidates(self, u_mean, std, B, seed, it, sample_offset=0):
        """The (B,T,m) candidates the drawn kernels see (verification only)."""
        src = CemSource.drawn(u_mean, std, B, seed, it, sample_offset)
        u_cand = torch.empty((src.B, src.T, src.m), dtype=F64, device=src.device)
        check(self.lib.irs_cem_candidates(src.T, src.m, src.B, *src.args, _ptr(u_cand, F64), _stream()),
              "irs_cem_candidates")
        return u_cand

    def _cem_histories(self, u_trj0, n_descents):
        """What cem_iterate returns: u_hist, std_hist (n_descents,T,m), x_hist (n_descents,T+1,n), cost_hist
        (n_descents), on the device of u_trj0 (T,m)."""
        k, (T, m) = int(n_descents), u_trj0.shape
        return {key: torch.empty(shape, dtype=F64, device=u_trj0.device)
                for key, shape in (("u_hist", (k, T, m)), ("std_hist", (k, T, m)), ("x_hist", (k, T + 1, self.n)),
                                   ("cost_hist", (k,)))}


class DeviceModel(CemModelFree):
    """A registered device functor (irs_model_id) with its constants bound."""

    def __init__(self, model_id, params):
        self.lib = _lib.load()
        self.model_id = int(model_id)
        self.params = [float(p) for p in params]
        n, m, npar = (_lib.c_int(), _lib.c_int(), _lib.c_int())
        check(self.lib.irs_model_info(self.model_id, n, m, npar), "irs_model_info")
        self.n, self.m = n.value, m.value
        if npar.value != len(self.params):
            raise ValueError("model %d expects %d params, got %d" % (model_id, npar.value, len(self.params)))
        self._p = dbl_array(self.params)
        self._np = len(self.params)
        self._ws = {}

    def fill_call(self, c):
        """The model head every call struct of the C ABI starts with: id, parameter count, parameters."""
        c.model, c.n_params = self.model_id, self._np
        for i, v in enumerate(self.params):
            c.params[i] = v

    # ---- DynamicalSystem plugin surface -----------------------------------
    def dynamics_batch(self, X, U):
        B = X.shape[0]
        Xn = torch.empty((B, self.n), dtype=F64, device=X.device)
        check(self.lib.irs_dynamics_batch(self.model_id, self._p, self._np, _ptr(X, F64), _ptr(U, F64),
                                          B, _ptr(Xn, F64), _stream()), "irs_dynamics_batch")
        return Xn

    def jacobian_xu_batch(self, X, U):
        B = X.shape[0]
        J = torch.empty((B, self.n, self.n + self.m), dtype=F64, device=X.device)
        check(self.lib.irs_jacobian_xu_batch(self.model_id, self._p, self._np, _ptr(X, F64), _ptr(U, F64),
                                             B, _ptr(J, F64), _stream()), "irs_jacobian_xu_batch")
        return J

    def contact_samples_f32(self, x, u, du):
        """Per-sample f32 lanes of the FIRST_ORDER sample pass of a contact model (irs_contact_samples_f32):
        x (n), u (m) f64, du (B,m) f32 -> Xn (B,n) f32, Bs (B,n,m) f32, active_mask (B) i32."""
        B = du.shape[0]
        Xn = torch.empty((B, self.n), dtype=F32, device=du.device)
        Bs = torch.empty((B, self.n, self.m), dtype=F32, device=du.device)
        mask = torch.empty((B,), dtype=torch.int32, device=du.device)
        check(self.lib.irs_contact_samples_f32(self.model_id, self._p, self._np, _ptr(x, F64), _ptr(u, F64),
                                               _ptr(du, F32), B, _ptr(Xn, F32), _ptr(Bs, F32), mask.data_ptr(),
                                               _stream()), "irs_contact_samples_f32")
        return Xn, Bs, mask

    def rollout_cost(self, x0, u_trj, Q, R, xd_trj):
        T = u_trj.shape[0]
        x_trj = torch.empty((T + 1, self.n), dtype=F64, device=u_trj.device)
        cost = torch.empty((1,), dtype=F64, device=u_trj.device)
        check(self.lib.irs_rollout_cost(self.model_id, self._p, self._np, T, _ptr(x0, F64), _ptr(u_trj, F64),
                                        _ptr(Q, F64), _ptr(R, F64), _ptr(xd_trj, F64), _ptr(x_trj, F64),
                                        _ptr(cost, F64), _stream()), "irs_rollout_cost")
        return x_trj, cost

    # ---- smoothing --------------------------------------------------------
    def sums_len(self, mode):
        return self.lib.irs_sums_len(self.model_id, mode)

    def smooth_geometry(self, mode, T, N, rng=False):
        return smooth_geometry(self.model_id, mode, T, N, rng)

    def _workspace(self, mode, T, N, device):
        need = self.lib.irs_smooth_workspace_bytes(self.model_id, mode, T, N)
        key = (mode, device)
        ws = self._ws.get(key)
        if ws is None or ws.numel() < need:
            ws = torch.empty((max(need, 8192),), dtype=torch.uint8, device=device)
            check(self.lib.irs_workspace_init(ws.data_ptr(), ws.numel(), _stream()), "irs_workspace_init")
            self._ws[key] = ws
        return ws

    def _tv_shapes(self, lead, mode=None):
        """The shapes of At, Bt, ct, info -- and of sums, given the mode -- behind the leading dimensions `lead`."""
        shapes = dict(At=lead + (self.n, self.n), Bt=lead + (self.n, self.m), ct=lead + (self.n,), info=lead)
        return shapes if mode is None else dict(sums=lead + (self.sums_len(mode),), **shapes)

    @staticmethod
    def _tv_alloc(shapes, device):
        return {k: torch.empty(shape, dtype=torch.int32 if k == "info" else F64, device=device)
                for k, shape in shapes.items()}

    def _tv_outputs(self, T, device, out):
        if out is not None:
            return out
        return dict(self._tv_alloc(self._tv_shapes((T,)), device), sums=None)

    def smooth_call(self, mode, T, N, x_trj, u_trj, o, ws, dx=None, du=None, rng=None, n_total=None, sample_offset=0):
        """The irs_smooth_call of one sample pass, for irs_smooth_run.  Samples supplied (dx, du) or, with
        rng = (std_x, std_u, seed, iter), drawn on the device; o = dict(sums, At, Bt, ct, info) asks for the fused
        solve, dict(sums) for the sums alone; ws = the workspace tensor; n_total (default N) = the samples per
        timestep over all devices."""
        c = _lib.SmoothCall()
        self.fill_call(c)
        c.mode, c.T, c.N = int(mode), int(T), int(N)
        c.x_trj, c.u_trj = _ptr(x_trj, F64), _ptr(u_trj, F64)
        if rng is not None:
            std_x, std_u, seed, it = rng
            c.use_rng, c.seed, c.sample_offset = 1, int(seed), int(sample_offset)
            set_call_iter(c, it, std_x, std_u)
        else:
            c.dx, c.du = _ptr(dx, F32), _ptr(du, F32)
        c.sums = _ptr(o["sums"], F64)
        if "At" in o:
            c.At, c.Bt, c.ct = (_ptr(o[k], F64) for k in ("At", "Bt", "ct"))
            c.info = o["info"].data_ptr()
        c.n_total = int(N if n_total is None else n_total)
        c.workspace, c.workspace_bytes = ws.data_ptr(), ws.numel()
        return c

    def _smooth_run(self, mode, T, N, x_trj, u_trj, o, **samples):
        """One irs_smooth_run into `o` (see smooth_call); a `sums` that is None is allocated."""
        device = u_trj.device
        if o["sums"] is None:
            o["sums"] = torch.empty((T, self.sums_len(mode)), dtype=F64, device=device)
        c = self.smooth_call(mode, T, N, x_trj, u_trj, o, self._workspace(mode, T, N, device), **samples)
        check(self.lib.irs_smooth_run(ctypes.byref(c), _stream()), "irs_smooth_run")
        return o

    def smooth(self, mode, x_trj, u_trj, dx, du, out=None):
        """Whole get_TV_matrices in one launch (single GPU), samples supplied.
        Returns dict(sums, At, Bt, ct, info); pass `out` (a previous result) to reuse buffers."""
        T, N = du.shape[0], du.shape[1]
        return self._smooth_run(mode, T, N, x_trj, u_trj, self._tv_outputs(T, du.device, out), dx=dx, du=du)

    def smooth_rng(self, mode, x_trj, u_trj, N, std_x, std_u, seed, it, out=None):
        T = u_trj.shape[0]
        return self._smooth_run(mode, T, N, x_trj, u_trj, self._tv_outputs(T, u_trj.device, out),
                                rng=(std_x, std_u, seed, it))

    # ---- B sample passes per launch ------------------------------------------
    # the two kinds, by their workspace cache key: the method, its entries of the C ABI, and whether it takes std_x_dev
    _SMOOTH_BATCH = {
        "smooth_batch": ("smooth_rng_batch", "irs_smooth_batch_workspace_bytes", "irs_smooth_batch_workspace_init",
                         "irs_smooth_rng_batch", False),
        "smooth_general_batch": ("smooth_rng_general_batch", "irs_smooth_general_batch_workspace_bytes",
                                 "irs_smooth_general_batch_workspace_init", "irs_smooth_rng_general_batch", True)}

    def _smooth_batch_served(self, kind, mode):
        return getattr(self.lib, self._SMOOTH_BATCH[kind][1])(self.model_id, int(mode), 1, 1, 1) > 0

    def _smooth_rng_batch(self, kind, mode, X, U, N, std_x_dev, std_u_dev, seed_dev, it, out):
        """smooth_rng_batch / smooth_rng_general_batch (`kind`: a key of _SMOOTH_BATCH)."""
        method, ws_bytes, ws_init, launch, takes_std_x = self._SMOOTH_BATCH[kind]
        mode, N = int(mode), int(N)
        B = U.shape[0]
        T = out["info"].shape[1] if out is not None else U.shape[1]
        dev = U.device
        for name, t, cols in (("X", X, self.n), ("U", U, self.m)):
            assert t.is_cuda and t.dtype == F64 and t.dim() == 3 and t.shape[0] == B and t.shape[1] >= T, name
            assert t.shape[2] == cols and t.stride(2) == 1 and t.stride(1) == cols, (name, t.shape, t.stride())
            assert B == 1 or t.stride(0) >= T * cols, (name, t.stride())
        assert not takes_std_x or tuple(std_x_dev.shape) == (B, self.n)
        assert tuple(std_u_dev.shape) == (B, self.m) and tuple(seed_dev.shape) == (B,) and seed_dev.dtype == torch.int64
        assert seed_dev.is_cuda and seed_dev.is_contiguous()
        o = _outputs(out, self._tv_shapes((B, T), mode), dev)
        assert o["info"].dtype == torch.int32 and o["info"].is_contiguous()
        need = getattr(self.lib, ws_bytes)(self.model_id, mode, T, N, B)
        if need == 0:
            raise NotImplementedError("%s: model %d, mode %d is not served" % (method, self.model_id, mode))
        key = (kind, mode, T, N)                             # one slice layout per buffer: the counters stay put
        before = self._ws.get((key, dev))
        ws = self._cached_workspace(key, need, dev)
        if ws is not before:                                 # a fresh allocation: its counters are zeroed once
            check(getattr(self.lib, ws_init)(ws.data_ptr(), ws.numel(), _stream()), ws_init)
        xs = X.stride(0) if B > 1 else X.shape[1] * self.n
        us = U.stride(0) if B > 1 else U.shape[1] * self.m
        stds = (_ptr(std_x_dev, F64), _ptr(std_u_dev, F64)) if takes_std_x else (_ptr(std_u_dev, F64),)
        check(getattr(self.lib, launch)(self.model_id, self._p, self._np, mode, T, N, B, X.data_ptr(), xs,
                                        U.data_ptr(), us, *stds, seed_dev.data_ptr(), int(it), _ptr(o["sums"], F64),
                                        _ptr(o["At"], F64), _ptr(o["Bt"], F64), _ptr(o["ct"], F64),
                                        o["info"].data_ptr(), ws.data_ptr(), ws.numel(), _stream()), launch)
        return o

    def smooth_batch_supported(self, mode):
        """Whether smooth_rng_batch serves this model in `mode`: what the uniform-geometry kernel serves (the exact
        planar hand's u-only modes; IRS_UG is read per call)."""
        return self._smooth_batch_served("smooth_batch", mode)

    def smooth_rng_batch(self, mode, X, U, N, std_u_dev, seed_dev, it, out=None):
        """The sample passes of B problems in one launch (irs_smooth_rng_batch): problem b's outputs are, bit for bit,
        those of smooth_rng(mode, X[b], U[b], N, None, std_u[b], seed[b], it).  X (B,T+1,n) or (B,T,n) -- T rows of
        each problem are read -- and U (B,>=T,m) f64, contiguous in their last two dimensions (the problem stride is
        taken from the tensor); T = the rows of `out`, else of U.  std_u_dev (B,m) f64, seed_dev (B) int64 holding the
        uint64 bits, both on the device.  Returns dict(sums (B,T,P), At (B,T,n,n), Bt (B,T,n,m), ct (B,T,n), info
        (B,T)); pass `out` to write into tensors of those shapes."""
        return self._smooth_rng_batch("smooth_batch", mode, X, U, N, None, std_u_dev, seed_dev, it, out)

    def tvlqr_descent(self, At, Bt, ct, Q, Qd, R, xd_trj, x0, alpha_R=0.5, out=None):
        """Riccati backward pass + closed-loop rollout + cost in one launch."""
        T = At.shape[0]
        o = _descent_outputs(self, T, (), At.device, out)
        check(self.lib.irs_tvlqr_descent(self.model_id, self._p, self._np, T, _ptr(At, F64), _ptr(Bt, F64),
                                         _ptr(ct, F64), _ptr(Q, F64), _ptr(Qd, F64), _ptr(R, F64),
                                         float(alpha_R), _ptr(xd_trj, F64), _ptr(x0, F64), _ptr(o["K"], F64),
                                         _ptr(o["k"], F64), _ptr(o["x_new"], F64), _ptr(o["u_new"], F64),
                                         _ptr(o["cost"], F64), o["info"].data_ptr(), _stream()),
              "irs_tvlqr_descent")
        return o

    # ---- B problems of an analytic model per launch ---------------------------------
    def tvlqr_descent_batch(self, At, Bt, ct, Q, Qd, R, xd_trj, x0, alpha_R=0.5, out=None):
        """B descents in one launch (irs_tvlqr_descent_batch): problem b's outputs are, bit for bit, those of
        tvlqr_descent on At[b], Bt[b], ct[b], xd_trj[b], x0[b] with the shared Q, Qd, R.  At (B,T,n,n), Bt (B,T,n,m),
        ct (B,T,n), xd_trj (B,T+1,n), x0 (B,n).  Returns dict(K (B,T,m,n), k (B,T,m), x_new (B,T+1,n), u_new (B,T,m),
        cost (B), info (B)); pass `out` to write into tensors of those shapes."""
        B, T = At.shape[0], At.shape[1]
        n, m = self.n, self.m
        _check_shapes((("At", At, (B, T, n, n)), ("Bt", Bt, (B, T, n, m)), ("ct", ct, (B, T, n)),
                       ("xd_trj", xd_trj, (B, T + 1, n)), ("x0", x0, (B, n))))
        o = _descent_outputs(self, T, (B,), At.device, out)
        check(self.lib.irs_tvlqr_descent_batch(self.model_id, self._p, self._np, T, B, _ptr(At, F64), _ptr(Bt, F64),
                                               _ptr(ct, F64), _ptr(Q, F64), _ptr(Qd, F64), _ptr(R, F64),
                                               float(alpha_R), _ptr(xd_trj, F64), _ptr(x0, F64), _ptr(o["K"], F64),
                                               _ptr(o["k"], F64), _ptr(o["x_new"], F64), _ptr(o["u_new"], F64),
                                               _ptr(o["cost"], F64), _ptr(o["info"], torch.int32), _stream()),
              "irs_tvlqr_descent_batch")
        return o

    def plan_within_bounds_batch(self, At, Bt, ct, K, k, x_new, xlo, xhi, ulo, uhi, flag=None):
        """flag (B) int32: 1 where some tail plan of problem b leaves ITS box xlo, xhi (B,n), ulo, uhi (B,m) -- one
        launch (irs_tvlqr_plan_within_bounds_batch), the single entry's decision per problem."""
        B, T = At.shape[0], At.shape[1]
        _check_shapes((("xlo", xlo, (B, self.n)), ("xhi", xhi, (B, self.n)), ("ulo", ulo, (B, self.m)),
                       ("uhi", uhi, (B, self.m)), ("x_new", x_new, (B, T + 1, self.n)),
                       ("K", K, (B, T, self.m, self.n)), ("k", k, (B, T, self.m))))
        if flag is None:
            flag = torch.empty((B,), dtype=torch.int32, device=At.device)
        check(self.lib.irs_tvlqr_plan_within_bounds_batch(self.n, self.m, T, B, _ptr(At, F64), _ptr(Bt, F64),
                                                          _ptr(ct, F64), _ptr(K, F64), _ptr(k, F64), _ptr(x_new, F64),
                                                          _ptr(xlo, F64), _ptr(xhi, F64), _ptr(ulo, F64), _ptr(uhi, F64),
                                                          _ptr(flag, torch.int32), _stream()),
              "irs_tvlqr_plan_within_bounds_batch")
        return flag

    def tvlqr_box_descent_batch(self, At, Bt, ct, Q, Qd, R, xd_trj, x0, xlo, xhi, ulo, uhi, alpha_R=0.5, rho=10.0,
                                relax=1.6, max_iter=5000, eps=1e-8, run_flag=None, records_in_hbm=False, out=None):
        """B bounded descents in one launch (irs_tvlqr_box_descent_batch): problem b's outputs are, bit for bit, those
        of irs_tvlqr_box_descent_if on problem b's blocks and ITS box xlo, xhi (B,n), ulo, uhi (B,m), with the shared
        Q, Qd, R and ADMM settings.  run_flag (B) int32 or None: problem b is neither read nor written where
        run_flag[b] == 0.  Beyond the LDS horizon the factor records go to a cached workspace, one slice per problem;
        records_in_hbm=True puts them there at any horizon (same bits).  Returns dict(x_new (B,T+1,n), u_new (B,T,m),
        cost (B), info (B,3)); pass `out` to write into tensors of those shapes."""
        B, T = At.shape[0], At.shape[1]
        dev = At.device
        n, m = self.n, self.m
        _check_shapes((("At", At, (B, T, n, n)), ("Bt", Bt, (B, T, n, m)), ("ct", ct, (B, T, n)),
                       ("xd_trj", xd_trj, (B, T + 1, n)), ("x0", x0, (B, n)), ("xlo", xlo, (B, n)), ("xhi", xhi, (B, n)),
                       ("ulo", ulo, (B, m)), ("uhi", uhi, (B, m))))
        assert run_flag is None or tuple(run_flag.shape) == (B,), tuple(run_flag.shape)
        o = _outputs(out, dict(x_new=(B, T + 1, n), u_new=(B, T, m), cost=(B,), info=(B, 3)), dev)
        ws = None
        if records_in_hbm or self.lib.irs_tvlqr_box_workspace_bytes(self.model_id, T, 0) > 0:
            need = self.lib.irs_tvlqr_box_descent_batch_workspace_bytes(self.model_id, T, B)
            ws = self._cached_workspace("box_batch", need, dev)
        check(self.lib.irs_tvlqr_box_descent_batch(self.model_id, self._p, self._np, T, B, _ptr(At, F64), _ptr(Bt, F64),
                                                   _ptr(ct, F64), _ptr(Q, F64), _ptr(Qd, F64), _ptr(R, F64),
                                                   float(alpha_R), _ptr(xd_trj, F64), _ptr(x0, F64), _ptr(xlo, F64),
                                                   _ptr(xhi, F64), _ptr(ulo, F64), _ptr(uhi, F64), float(rho),
                                                   float(relax), int(max_iter), float(eps), _ptr(o["x_new"], F64),
                                                   _ptr(o["u_new"], F64), _ptr(o["cost"], F64),
                                                   _ptr(o["info"], torch.int32), _ptr(run_flag, torch.int32),
                                                   *_ws_args(ws), _stream()),
              "irs_tvlqr_box_descent_batch")
        return o

    def smooth_general_batch_supported(self, mode):
        """Whether smooth_rng_general_batch serves this model in `mode`: the analytic models in the modes that perturb
        x and u (zero-order AB, first order)."""
        return self._smooth_batch_served("smooth_general_batch", mode)

    def smooth_rng_general_batch(self, mode, X, U, N, std_x_dev, std_u_dev, seed_dev, it, out=None):
        """The sample passes of B problems of an analytic model in one launch (irs_smooth_rng_general_batch): problem b
        sees the draws of smooth_rng(mode, X[b], U[b], N, std_x[b], std_u[b], seed[b], it) and its results agree with
        that call's up to f32 rounding (not bit for bit).  Arguments and result as smooth_rng_batch, plus std_x_dev
        (B,n) f64 on the device."""
        return self._smooth_rng_batch("smooth_general_batch", mode, X, U, N, std_x_dev, std_u_dev, seed_dev, it, out)

    # ---- box-constrained descent ----------------------------------------------
    # the dynamic-LDS budget of the bounded-descent kernels (IRS_LDS_BUDGET in csrc/irs_common.hpp), for callers that
    # compare the size queries with it; every placement decision reads irs_box_horizon_limit instead
    BOX_LDS_LIMIT = 160 * 1024 - 512

    def box_descent_supported(self, T, du=False):
        """Whether the bounded TV-LQR kernel runs horizon T: with its factor records on chip, or in a workspace in
        HBM.  du: the position-controlled form (quasistatic solver 1)."""
        return 0 < int(T) <= self.box_horizon_limit(du)

    def box_horizon_limit(self, du=False):
        """The longest horizon the bounded TV-LQR kernel runs (records in HBM; 0: the model has no such form)."""
        return self.lib.irs_box_horizon_limit(self.model_id, _lib.BOX_ADMM_DU if du else _lib.BOX_ADMM)

    def _cached_workspace(self, key, need, device):
        """A byte buffer of at least `need` bytes, cached under (key, device), grown on demand; None for need == 0."""
        if need == 0:
            return None
        ws = self._ws.get((key, device))
        if ws is None or ws.numel() < need:
            ws = self._ws[(key, device)] = torch.empty((need,), dtype=torch.uint8, device=device)
        return ws

    def _box_workspace(self, T, du, device, force=False):
        """The bounded TV-LQR kernel's factor records, when they do not fit LDS (or `force`: at any horizon)."""
        if force:
            need = self.lib.irs_box_records_bytes(self.model_id, int(T), _lib.BOX_ADMM_DU if du else _lib.BOX_ADMM)
        else:
            need = self.lib.irs_tvlqr_box_workspace_bytes(self.model_id, int(T), 1 if du else 0)
        return self._cached_workspace("box", need, device)

    @staticmethod
    def _lazy_outputs(o, enforced, count, device):
        """The two outputs of a lazy launch in `o`: enforced (count,) int32, in/out -- a copy of `enforced` (None: all
        zero, the set starts empty) -- and lazy (3,) f64."""
        if enforced is None:
            o["enforced"] = torch.zeros((count,), dtype=torch.int32, device=device)
        else:
            o["enforced"] = torch.as_tensor(enforced).to(device=device, dtype=torch.int32, copy=True).contiguous()
            if tuple(o["enforced"].shape) != (count,):
                raise ValueError("enforced must have %d entries, not %s" % (count, tuple(o["enforced"].shape)))
        o["lazy"] = torch.empty((3,), dtype=F64, device=device)

    def _box_admm_call(self, family, prefix, outs, ws, o, rho, relax, max_iter, eps, adaptive_rho, lazy_bounds, enforced,
                       components, wsx_extra=()):
        """One bounded-ADMM launch of `family` (a C entry's name without its suffix).  prefix: the entry's arguments
        from T to its bounds (and solver); outs: its output pointers.  Picks the entry -- _wsx for the fixed penalty,
        _set for adaptive_rho, _lazy for lazy_bounds (`components` entries in its set) -- appends that entry's tail,
        and adds to `o` what the entry writes besides `outs`."""
        dev = o["info"].device
        if lazy_bounds or adaptive_rho:
            if "adapt" not in o:
                o["adapt"] = torch.empty((3,), dtype=F64, device=dev)
            if lazy_bounds:
                self._lazy_outputs(o, enforced, components, dev)
            st = _lib.admm_settings(rho, relax, max_iter, eps, adaptive=bool(adaptive_rho))
            name, tail = family + "_set", [ctypes.byref(st), *outs, _ptr(o["adapt"], F64), *_ws_args(ws)]
            if lazy_bounds:
                name, tail = family + "_lazy", tail + [o["enforced"].data_ptr(), _ptr(o["lazy"], F64)]
        else:
            name = family + "_wsx"
            tail = [float(rho), float(relax), int(max_iter), float(eps), *outs, *wsx_extra, *_ws_args(ws)]
        check(getattr(self.lib, name)(self.model_id, self._p, self._np, *prefix, *tail, _stream()), name)
        return o

    def tvlqr_box_descent(self, At, Bt, ct, Q, Qd, R, xd_trj, x0, xlo, xhi, ulo, uhi, alpha_R=0.5,
                          rho=10.0, relax=1.6, max_iter=5000, eps=1e-8, records_in_hbm=False, adaptive_rho=False,
                          lazy_bounds=False, enforced=None):
        """local_descent with active abs bounds (T warm-started tail QPs by ADMM around one
        Riccati factorisation).  Beyond the LDS horizon the factor records go to a cached workspace in HBM;
        records_in_hbm=True puts them there at any horizon (same result, bit for bit).  Returns
        dict(x_new, u_new, info[3]).  adaptive_rho: the penalty follows the residuals from `rho` on, the kernel
        refactorising as it moves (irs_admm_settings); the result then also holds adapt[3] = (factorisations of the
        launch, final rho, ADMM iterations of all tails).  lazy_bounds: the bounds are enforced lazily
        (irs_tvlqr_box_descent_lazy) -- only components whose bound a converged tail plan would break carry the
        penalty term, so "no bound" written as a large finite number costs nothing; `enforced` (n + m, nonzero = in
        the set from the start, e.g. the previous descent's result) seeds the set.  The result then also holds
        enforced[n + m] (int32: the final set), lazy[3] = (activations, last tail that activated, ADMM iterations)
        and adapt[3]."""
        T = At.shape[0]
        dev = At.device
        o = dict(x_new=torch.empty((T + 1, self.n), dtype=F64, device=dev),
                 u_new=torch.empty((T, self.m), dtype=F64, device=dev),
                 info=torch.empty((3,), dtype=torch.int32, device=dev))
        ws = self._box_workspace(T, False, dev, force=records_in_hbm)
        prefix = [T, *(_ptr(a, F64) for a in (At, Bt, ct, Q, Qd, R)), float(alpha_R),
                  *(_ptr(a, F64) for a in (xd_trj, x0, xlo, xhi, ulo, uhi))]
        outs = [_ptr(o["x_new"], F64), _ptr(o["u_new"], F64), o["info"].data_ptr()]
        return self._box_admm_call("irs_tvlqr_box_descent", prefix, outs, ws, o, rho, relax, max_iter, eps,
                                   adaptive_rho, lazy_bounds, enforced, self.n + self.m)

    def tvlqr_box_solve(self, At, Bt, ct, Q, Qd, R, xd_trj, x0, x_lo=None, x_hi=None, u_lo=None, u_hi=None,
                        du_lo=None, du_hi=None, position_controlled=False, alpha_R=0.5, rho=10.0, relax=1.6,
                        max_iter=5000, eps=1e-8, adaptive_rho=False, records_in_hbm=False, lazy_bounds=False,
                        enforced=None):
        """solve_tvlqr stand-alone: ONE bounded QP by ADMM, its plan returned.  Bounds are per-time rows or None;
        du bounds need the position-controlled form.  Beyond the LDS horizon the factor records go to a cached
        workspace in HBM (records_in_hbm=True: at any horizon).  Returns dict(x_star, u_star, info[3]); adaptive_rho
        as in tvlqr_box_descent (adds adapt[3]); lazy_bounds / enforced likewise (adds enforced, lazy and adapt; the
        components are [x | u], position controlled [x | u abs | du])."""
        T = At.shape[0]
        dev = At.device
        o = dict(x_star=torch.zeros((T + 1, At.shape[1]), dtype=F64, device=dev),
                 u_star=torch.zeros((T, Bt.shape[2]), dtype=F64, device=dev),
                 info=torch.full((3,), -1, dtype=torch.int32, device=dev))
        ws = self._box_workspace(T, position_controlled, dev, force=records_in_hbm)   # None while they fit on chip
        prefix = [T, *(_ptr(a, F64) for a in (At, Bt, ct, Q, Qd, R)), float(alpha_R), _ptr(xd_trj, F64), _ptr(x0, F64),
                  1 if position_controlled else 0, *(_ptr(a, F64) for a in (x_lo, x_hi, u_lo, u_hi, du_lo, du_hi))]
        outs = [_ptr(o["x_star"], F64), _ptr(o["u_star"], F64), o["info"].data_ptr()]
        return self._box_admm_call("irs_tvlqr_box_solve", prefix, outs, ws, o, rho, relax, max_iter, eps, adaptive_rho,
                                   lazy_bounds, enforced, At.shape[1] + (2 if position_controlled else 1) * Bt.shape[2])

    SOLVER_AUTO, SOLVER_ADMM, SOLVER_ACTIVE_SET, SOLVER_ACTIVE_SET_MFMA = 0, 1, 2, 3

    def quasistatic_descent_supported(self, T, solver=1):
        """Whether `solver` can run horizon T (3: always, for models that fit the matrix-core tile -- beyond
        the LDS-resident size its records go to a workspace in HBM; 1: likewise, up to box_horizon_limit(du=True);
        2: while its data fit LDS)."""
        kind = {2: _lib.BOX_ACTIVE_SET, 3: _lib.BOX_ACTIVE_SET_MFMA}.get(int(solver), _lib.BOX_ADMM_DU)
        return 0 < int(T) <= self.lib.irs_box_horizon_limit(self.model_id, kind)

    def _descent_workspace(self, T, solver, device):
        need = self.lib.irs_quasistatic_descent_workspace_bytes(self.model_id, int(T), int(solver))
        return self._cached_workspace("descent", need, device)

    def quasistatic_box_descent(self, At, Bt, ct, Q, Qd, R, xd_trj, x0, x_lo=None, x_hi=None, u_lo=None,
                                u_hi=None, du_lo=None, du_hi=None, solver=0, rho=10.0, relax=1.6,
                                max_iter=5000, eps=1e-8, out=None, act=None, adaptive_rho=False, lazy_bounds=False,
                                enforced=None):
        """IrsLqrQuasistatic.local_descent after get_TV_matrices (irs_lqr_quasistatic.py:286-345) +
        eval_cost.  Bounds are absolute per-time rows ((T+1,n) / (T,m)) or None.  solver: 0 auto,
        1 ADMM (beyond the LDS horizon with its records in HBM), 2 active set (one control box, no x bounds; lanes,
        LDS-resident), 3 the same on matrix-core tiles (any horizon).  `act` (T,m) f64 in {-1,0,+1}, in/out: the active set the first tail starts
        from / converged to (hand it from one iteration's descent to the next; zeros = cold start).
        Returns dict(x_new, u_new, cost, info[3]).  adaptive_rho (solver 1 only) as in tvlqr_box_descent (adds
        adapt[3]); lazy_bounds / enforced (solver 1 only) likewise, the components [x (n) | u abs (m) | du (m)]."""
        T = At.shape[0]
        dev = At.device
        o = out
        if o is None:
            o = dict(x_new=torch.empty((T + 1, self.n), dtype=F64, device=dev),
                     u_new=torch.empty((T, self.m), dtype=F64, device=dev),
                     cost=torch.empty((1,), dtype=F64, device=dev),
                     info=torch.empty((3,), dtype=torch.int32, device=dev))
        for b, shape in ((x_lo, (T + 1, self.n)), (x_hi, (T + 1, self.n)), (u_lo, (T, self.m)),
                         (u_hi, (T, self.m)), (du_lo, (T, self.m)), (du_hi, (T, self.m))):
            assert b is None or tuple(b.shape) == shape, (tuple(b.shape), shape)
        assert act is None or tuple(act.shape) == (T, self.m)
        ws = self._descent_workspace(T, solver, dev) if int(solver) in (0, 1, 3) else None
        for flag, on in (("lazy_bounds", lazy_bounds), ("adaptive_rho", adaptive_rho)):
            if on and int(solver) != 1:
                raise ValueError("%s belongs to the ADMM kernel: solver must be 1, not %d" % (flag, int(solver)))
        prefix = [T, *(_ptr(a, F64) for a in (At, Bt, ct, Q, Qd, R, xd_trj, x0, x_lo, x_hi, u_lo, u_hi, du_lo, du_hi)),
                  int(solver)]
        outs = [_ptr(o["x_new"], F64), _ptr(o["u_new"], F64), _ptr(o["cost"], F64), o["info"].data_ptr()]
        return self._box_admm_call("irs_quasistatic_box_descent", prefix, outs, ws, o, rho, relax, max_iter, eps,
                                   adaptive_rho, lazy_bounds, enforced, self.n + 2 * self.m,
                                   wsx_extra=[_ptr(act, F64)])

    # ---- B quasistatic descents per launch ------------------------------------
    def _descent_batch_workspace(self, T, B, device, force=False):
        """Cached per (T, B): the records of B problems, where they do not fit LDS (or `force`); else None."""
        if force:
            one = self.lib.irs_box_records_bytes(self.model_id, int(T), _lib.BOX_ACTIVE_SET_MFMA)
            need = int(B) * ((one + 255) // 256 * 256)
        else:
            need = self.lib.irs_quasistatic_descent_batch_workspace_bytes(self.model_id, int(T), int(B))
        return self._cached_workspace(("descent_batch", int(T), int(B)), need, device)

    def quasistatic_box_descent_batch(self, At, Bt, ct, Q, Qd, R, xd_trj, x0, u_lo=None, u_hi=None, du_lo=None,
                                      du_hi=None, max_iter=5000, eps=1e-8, out=None, act=None, records_in_hbm=False):
        """B quasistatic descents in one launch (solver 3's method; one workgroup per problem): At (B,T,n,n), Bt
        (B,T,n,m), ct (B,T,n), xd_trj (B,T+1,n), x0 (B,n), exactly one pair of bound rows (B,T,m); Q, Qd, R shared.
        `act` (B,T,m) in/out as in quasistatic_box_descent.  records_in_hbm=True puts the per-step records in a
        workspace at any horizon (same result, bit for bit).  Returns dict(x_new (B,T+1,n), u_new (B,T,m), cost (B),
        info (B,3)); pass `out` to write into tensors of those shapes (e.g. a slot of a history)."""
        B, T = At.shape[0], At.shape[1]
        dev = At.device
        n, m = self.n, self.m
        _check_shapes((("At", At, (B, T, n, n)), ("Bt", Bt, (B, T, n, m)), ("ct", ct, (B, T, n)),
                       ("xd_trj", xd_trj, (B, T + 1, n)), ("x0", x0, (B, n))))
        o = _outputs(out, dict(x_new=(B, T + 1, n), u_new=(B, T, m), cost=(B,), info=(B, 3)), dev)
        for b in (u_lo, u_hi, du_lo, du_hi, act):
            assert b is None or tuple(b.shape) == (B, T, self.m), (tuple(b.shape), (B, T, self.m))
        assert o["info"].dtype == torch.int32 and o["info"].is_contiguous()
        ws = self._descent_batch_workspace(T, B, dev, force=records_in_hbm)
        check(self.lib.irs_quasistatic_box_descent_batch(
            self.model_id, self._p, self._np, T, B, _ptr(At, F64), _ptr(Bt, F64), _ptr(ct, F64), _ptr(Q, F64),
            _ptr(Qd, F64), _ptr(R, F64), _ptr(xd_trj, F64), _ptr(x0, F64), _ptr(u_lo, F64), _ptr(u_hi, F64),
            _ptr(du_lo, F64), _ptr(du_hi, F64), int(max_iter), float(eps), _ptr(o["x_new"], F64), _ptr(o["u_new"], F64),
            _ptr(o["cost"], F64), o["info"].data_ptr(), _ptr(act, F64), *_ws_args(ws), _stream()),
            "irs_quasistatic_box_descent_batch")
        return o

    def quasistatic_bound_rows_batch(self, x_trj, idx, offsets, rel=False, out=None):
        """Trust-region rows of B problems in one launch: x_trj (B,T+1,n), idx (m) int32 = indices_u_into_x, offsets
        (B,2,m) or (B,2,T,m) -> lo, hi (B,T,m): x_trj[b,t,idx[j]] + offset, or (rel) the offset alone."""
        B, T = x_trj.shape[0], x_trj.shape[1] - 1
        assert tuple(offsets.shape) in ((B, 2, self.m), (B, 2, T, self.m)), tuple(offsets.shape)
        assert idx.dtype == torch.int32 and idx.is_cuda and idx.is_contiguous() and idx.numel() == self.m
        lo, hi = out if out is not None else (torch.empty((B, T, self.m), dtype=F64, device=x_trj.device),
                                              torch.empty((B, T, self.m), dtype=F64, device=x_trj.device))
        check(self.lib.irs_quasistatic_bound_rows_batch(self.n, self.m, T, B, _ptr(x_trj, F64), idx.data_ptr(),
                                                        _ptr(offsets, F64), int(offsets.dim() == 4), int(bool(rel)),
                                                        _ptr(lo, F64), _ptr(hi, F64), _stream()),
              "irs_quasistatic_bound_rows_batch")
        return lo, hi

    # ---- CEM baseline (the public names: CemModelFree) ------------------------
    def cem_costs(self, src, x0, Q, R, xd_trj, Qd=None):
        """CemModelFree.cem_costs in one launch; the entry is picked by (quasistatic, drawn)."""
        costs = torch.empty((src.B,), dtype=F64, device=src.device)
        name = ("irs_cem_rollout_costs" if Qd is None else "irs_cem_rollout_costs_quasistatic") + src.suffix
        weights = (_ptr(Q, F64), _ptr(R, F64)) if Qd is None else (_ptr(Q, F64), _ptr(Qd, F64), _ptr(R, F64))
        check(getattr(self.lib, name)(self.model_id, self._p, self._np, src.T, src.B, *src.args, _ptr(x0, F64), *weights,
                                      _ptr(xd_trj, F64), _ptr(costs, F64), _stream()), name)
        return costs
    def cem_iterate(self, u_trj0, std0, x0, Q, Qd, R, xd_trj, B, n_elite, n_descents, seed, iter0=1,
                    quasistatic=False):
        """n_descents CEM descents in ONE library call (irs_cem_iterate), nothing read back: a dict of the device
        histories u_hist, std_hist (n_descents,T,m), x_hist (n_descents,T+1,n), cost_hist (n_descents)."""
        T, m = u_trj0.shape
        o = self._cem_histories(u_trj0, n_descents)
        need = self.lib.irs_cem_iterate_scratch_bytes(T, m, int(B), int(n_elite))
        scratch = torch.empty((max(need, 8),), dtype=torch.uint8, device=u_trj0.device)
        c = _lib.CemIterateCall()
        self.fill_call(c)
        c.T, c.B, c.n_elite, c.n_descents, c.quasistatic = T, int(B), int(n_elite), int(n_descents), int(bool(quasistatic))
        c.seed, c.iter0 = int(seed), int(iter0)
        c.Q, c.Qd, c.R, c.xd_trj, c.x0 = (_ptr(a, F64) for a in (Q, Qd, R, xd_trj, x0))
        c.u_trj0, c.std0 = _ptr(u_trj0, F64), _ptr(std0, F64)
        c.u_hist, c.std_hist, c.x_hist, c.cost_hist = (_ptr(o[key], F64) for key in ("u_hist", "std_hist", "x_hist",
                                                                                      "cost_hist"))
        c.scratch, c.scratch_bytes = scratch.data_ptr(), scratch.numel()
        check(self.lib.irs_cem_iterate(ctypes.byref(c), _stream()), "irs_cem_iterate")
        return o

    def smooth_accumulate(self, mode, x_trj, u_trj, dx, du, sums=None):
        """Sample pass on supplied samples: dx (T,N,n) f32 (None for ZERO_ORDER_B), du (T,N,m) f32."""
        T, N = du.shape[0], du.shape[1]
        return self._smooth_run(mode, T, N, x_trj, u_trj, dict(sums=sums), dx=dx, du=du)["sums"]

    def smooth_accumulate_rng(self, mode, x_trj, u_trj, N, std_x, std_u, seed, it, sample_offset=0, sums=None):
        T = u_trj.shape[0]
        return self._smooth_run(mode, T, N, x_trj, u_trj, dict(sums=sums), rng=(std_x, std_u, seed, it),
                                sample_offset=sample_offset)["sums"]

    def rng_samples(self, T, N, std_x, std_u, seed, it, sample_offset=0):
        dev = require_gpu()
        dx = torch.empty((T, N, self.n), dtype=F32, device=dev)
        du = torch.empty((T, N, self.m), dtype=F32, device=dev)
        check(self.lib.irs_rng_samples(self.n, self.m, T, N, dbl_array(std_x), dbl_array(std_u), int(seed),
                                       int(it), int(sample_offset), _ptr(dx, F32), _ptr(du, F32), _stream()),
              "irs_rng_samples")
        return dx, du

    def smooth_finalize(self, mode, N_total, x_trj, u_trj, sums, out=None, workspace=None):
        """Solve step on (all-reduced) sums -> (At, Bt, ct, info); `out` = a previous result to reuse;
        `workspace` = the workspace tensor of the accumulate call that produced this rank's sums
        (contact models: its f64 nominal steps are reused)."""
        T = u_trj.shape[0]
        dev = u_trj.device
        if out is not None:
            At, Bt, ct, info = out
        else:
            At = torch.empty((T, self.n, self.n), dtype=F64, device=dev)
            Bt = torch.empty((T, self.n, self.m), dtype=F64, device=dev)
            ct = torch.empty((T, self.n), dtype=F64, device=dev)
            info = torch.empty((T,), dtype=torch.int32, device=dev)
        check(self.lib.irs_smooth_finalize_ws(self.model_id, self._p, self._np, mode, T, int(N_total),
                                              _ptr(x_trj, F64), _ptr(u_trj, F64), _ptr(sums, F64), _ptr(At, F64),
                                              _ptr(Bt, F64), _ptr(ct, F64), info.data_ptr(), *_ws_args(workspace),
                                              _stream()), "irs_smooth_finalize_ws")
        return At, Bt, ct, info

    def exact_linearize(self, x_trj, u_trj):
        T = u_trj.shape[0]
        dev = u_trj.device
        At = torch.empty((T, self.n, self.n), dtype=F64, device=dev)
        Bt = torch.empty((T, self.n, self.m), dtype=F64, device=dev)
        ct = torch.empty((T, self.n), dtype=F64, device=dev)
        check(self.lib.irs_exact_linearize(self.model_id, self._p, self._np, T, _ptr(x_trj, F64),
                                           _ptr(u_trj, F64), _ptr(At, F64), _ptr(Bt, F64), _ptr(ct, F64),
                                           _stream()), "irs_exact_linearize")
        return At, Bt, ct

    def closed_loop_rollout(self, K, k, x0, Q, R, xd_trj):
        T = K.shape[0]
        dev = K.device
        x_new = torch.empty((T + 1, self.n), dtype=F64, device=dev)
        u_new = torch.empty((T, self.m), dtype=F64, device=dev)
        cost = torch.empty((1,), dtype=F64, device=dev)
        check(self.lib.irs_closed_loop_rollout(self.model_id, self._p, self._np, T, _ptr(K, F64), _ptr(k, F64),
                                               _ptr(x0, F64), _ptr(Q, F64), _ptr(R, F64), _ptr(xd_trj, F64),
                                               _ptr(x_new, F64), _ptr(u_new, F64), _ptr(cost, F64), _stream()),
              "irs_closed_loop_rollout")
        return x_new, u_new, cost


def set_call_iter(c, it, std_x, std_u):
    """The iteration number and the standard deviations of an irs_smooth_call that draws on the device (std_x None:
    left as it is -- zero in a fresh call, which is what the u-only modes read)."""
    c.iter = int(it)
    if std_x is not None:
        for i, v in enumerate(std_x):
            c.std_x[i] = float(v)
    for i, v in enumerate(std_u):
        c.std_u[i] = float(v)


class SmoothPlan:
    """A pre-marshalled get_TV_matrices call (irs_smooth_call): `run()` is ONE FFI call
    that enqueues ONE kernel (fused path) and touches no Python-side allocation.

    Samples are either supplied (`dx`, `du` device f32 tensors) or drawn on the device
    (`rng=dict(N=..., std_x=..., std_u=..., seed=..., iter=...)`).  With `fuse=False`
    only `sums` is produced (multi-GPU path: all-reduce it, then `dm.smooth_finalize`)."""

    def __init__(self, dm, mode, x_trj, u_trj, dx=None, du=None, rng=None, fuse=True, n_total=None,
                 sample_offset=0):
        self.dm, self.mode = dm, mode
        T = u_trj.shape[0]
        device = u_trj.device
        self.N = N = int(rng["N"]) if rng is not None else du.shape[1]
        self.sums = torch.empty((T, dm.sums_len(mode)), dtype=F64, device=device)
        self.out = dict(dm._tv_outputs(T, device, None), sums=self.sums) if fuse else None
        self.ws = dm._workspace(mode, T, N, device)
        drawn = None if rng is None else (rng.get("std_x"), rng["std_u"], rng["seed"], rng.get("iter", 1))
        self.call = dm.smooth_call(mode, T, N, x_trj, u_trj, self.out or dict(sums=self.sums), self.ws, dx=dx, du=du,
                                   rng=drawn, n_total=n_total, sample_offset=sample_offset)
        self._keep = (dx, du)
        self._xu = (x_trj, u_trj)
        self._fn = dm.lib.irs_smooth_run
        self._ref = ctypes.byref(self.call)

    def set_trajectory(self, x_trj, u_trj):
        self._xu = (x_trj, u_trj)
        self.call.x_trj, self.call.u_trj = _ptr(x_trj, F64), _ptr(u_trj, F64)

    def set_samples(self, dx, du):
        self._keep = (dx, du)
        self.call.dx, self.call.du = _ptr(dx, F32), _ptr(du, F32)

    def set_iter(self, it, std_x, std_u):
        set_call_iter(self.call, it, std_x, std_u)

    def run(self, stream=None):
        rc = self._fn(self._ref, _stream() if stream is None else stream)
        if rc != 0:
            check(rc, "irs_smooth_run")
        return self.out if self.out is not None else self.sums


class DescentPlan:
    """A pre-marshalled irs_descent_call: Riccati + closed-loop rollout + cost, one launch."""

    def __init__(self, dm, At, Bt, ct, Q, Qd, R, xd_trj, x0, alpha_R=0.5, x_new=None, u_new=None):
        T = At.shape[0]
        self.out = _descent_outputs(dm, T, (), At.device, x_new=x_new, u_new=u_new)
        c = _lib.DescentCall()
        dm.fill_call(c)
        c.T, c.alpha_R = T, float(alpha_R)
        self._keep = (At, Bt, ct, Q, Qd, R, xd_trj, x0)
        c.At, c.Bt, c.ct = _ptr(At, F64), _ptr(Bt, F64), _ptr(ct, F64)
        c.Q, c.Qd, c.R = _ptr(Q, F64), _ptr(Qd, F64), _ptr(R, F64)
        c.xd_trj, c.x0 = _ptr(xd_trj, F64), _ptr(x0, F64)
        for name in ("K", "k", "x_new", "u_new", "cost"):
            setattr(c, name, self.out[name].data_ptr())
        c.info = self.out["info"].data_ptr()
        self.call = c
        self._fn = dm.lib.irs_descent_run
        self._ref = ctypes.byref(c)

    def run(self, stream=None):
        rc = self._fn(self._ref, _stream() if stream is None else stream)
        if rc != 0:
            check(rc, "irs_descent_run")
        return self.out


def evaluate_cost(x_trj, u_trj, Q, R, xd_trj):
    lib = _lib.load()
    T, n, m = u_trj.shape[0], x_trj.shape[1], u_trj.shape[1]
    cost = torch.empty((1,), dtype=F64, device=x_trj.device)
    check(lib.irs_evaluate_cost(n, m, T, _ptr(x_trj, F64), _ptr(u_trj, F64), _ptr(Q, F64), _ptr(R, F64),
                                _ptr(xd_trj, F64), _ptr(cost, F64), _stream()), "irs_evaluate_cost")
    return cost


def tvlqr_riccati(At, Bt, ct, Q, Qd, R, xd_trj, alpha_R=0.5):
    """Backward pass; returns K (T,m,n), k (T,m), info (1) device tensors."""
    lib = _lib.load()
    T, n, m = At.shape[0], At.shape[1], Bt.shape[2]
    dev = At.device
    K = torch.empty((T, m, n), dtype=F64, device=dev)
    k = torch.empty((T, m), dtype=F64, device=dev)
    info = torch.empty((1,), dtype=torch.int32, device=dev)
    check(lib.irs_tvlqr_riccati(n, m, T, _ptr(At, F64), _ptr(Bt, F64), _ptr(ct, F64), _ptr(Q, F64),
                                _ptr(Qd, F64), _ptr(R, F64), float(alpha_R), _ptr(xd_trj, F64), _ptr(K, F64),
                                _ptr(k, F64), info.data_ptr(), _stream()), "irs_tvlqr_riccati")
    return K, k, info


def tvlqr_linear_rollout(At, Bt, ct, K, k, x0):
    lib = _lib.load()
    T, n, m = At.shape[0], At.shape[1], Bt.shape[2]
    dev = At.device
    xs = torch.empty((T + 1, n), dtype=F64, device=dev)
    us = torch.empty((T, m), dtype=F64, device=dev)
    check(lib.irs_tvlqr_linear_rollout(n, m, T, _ptr(At, F64), _ptr(Bt, F64), _ptr(ct, F64), _ptr(K, F64),
                                       _ptr(k, F64), _ptr(x0, F64), _ptr(xs, F64), _ptr(us, F64), _stream()),
          "irs_tvlqr_linear_rollout")
    return xs, us


# ---- the values pass: the zero-order sample pass on function values the caller evaluated (csrc/smooth_values.hip) ----
def values_sums_len(n, m):
    return _lib.load().irs_values_sums_len(int(n), int(m))


def smooth_values_geometry(T, N):
    """The launch geometry of the values pass for (T, N) (irs_smooth_values_geometry): no launch, no device.
    dict(block, nblk, chunk, flush_trips)."""
    out = (ctypes.c_longlong * 4)()
    check(_lib.load().irs_smooth_values_geometry(int(T), int(N), out), "irs_smooth_values_geometry")
    return dict(block=out[0], nblk=out[1], chunk=out[2], flush_trips=out[3])


_values_ws = {}


def _values_workspace(n, m, T, N, device):
    """The cached scratch of the values pass for (`device`, the current stream), grown on demand (uninitialised: the
    pass zeroes nothing).  One per stream: a workspace takes one call in flight at a time, and calls on one stream run
    in order.  (An outgrown buffer goes back to torch's caching allocator, which orders its reuse behind the work
    queued on the stream it was allocated on: this one.)"""
    need = _lib.load().irs_smooth_values_workspace_bytes(n, m, T, N)
    key = (device, _stream())
    ws = _values_ws.get(key)
    if ws is None or ws.numel() < need:
        ws = _values_ws[key] = torch.empty((max(need, 256),), dtype=torch.uint8, device=device)
    return ws


def _values_shapes(dx, du, fz, f0):
    T, N, n = dx.shape
    m = du.shape[2]
    assert tuple(du.shape) == (T, N, m) and tuple(fz.shape) == (T, N, n) and tuple(f0.shape) == (T, n), \
        (tuple(dx.shape), tuple(du.shape), tuple(fz.shape), tuple(f0.shape))
    return T, N, n, m


def smooth_values_accumulate(dx, du, fz, f0, sums=None, workspace=None):
    """Statistics of the values pass: dx (T,N,n), du (T,N,m), fz (T,N,n), f0 (T,n) f32 -> sums (T,P) f64."""
    T, N, n, m = _values_shapes(dx, du, fz, f0)
    if sums is None:
        sums = torch.empty((T, values_sums_len(n, m)), dtype=F64, device=dx.device)
    ws = workspace if workspace is not None else _values_workspace(n, m, T, N, dx.device)
    check(_lib.load().irs_smooth_values_accumulate(n, m, T, N, _ptr(dx, F32), _ptr(du, F32), _ptr(fz, F32), _ptr(f0, F32),
                                                   _ptr(sums, F64), ws.data_ptr(), ws.numel(), _stream()),
          "irs_smooth_values_accumulate")
    return sums


def _values_outputs(T, n, m, device):
    return dict(sums=None,
                At=torch.empty((T, n, n), dtype=F64, device=device),
                Bt=torch.empty((T, n, m), dtype=F64, device=device),
                ct=torch.empty((T, n), dtype=F64, device=device),
                info=torch.empty((T,), dtype=torch.int32, device=device))


def smooth_values_finalize(N_total, x_trj, u_trj, fnom, sums, m=None, out=None):
    """Solve from (all-reduced) sums of the values pass -> (At, Bt, ct, info); fnom (T,n) f64 = f(x_t, u_t)."""
    T, n = fnom.shape
    m = u_trj.shape[1] if m is None else m
    o = out if out is not None else _values_outputs(T, n, m, fnom.device)
    check(_lib.load().irs_smooth_values_finalize(n, m, T, int(N_total), _ptr(x_trj, F64), _ptr(u_trj, F64),
                                                 _ptr(fnom, F64), _ptr(sums, F64), _ptr(o["At"], F64), _ptr(o["Bt"], F64),
                                                 _ptr(o["ct"], F64), o["info"].data_ptr(), _stream()),
          "irs_smooth_values_finalize")
    return o["At"], o["Bt"], o["ct"], o["info"]


def smooth_values(x_trj, u_trj, dx, du, fz, f0, fnom, out=None, workspace=None):
    """The values pass and its solve behind one call -> dict(sums, At, Bt, ct, info); `out` = a previous result."""
    T, N, n, m = _values_shapes(dx, du, fz, f0)
    o = out if out is not None else _values_outputs(T, n, m, dx.device)
    if o["sums"] is None:
        o["sums"] = torch.empty((T, values_sums_len(n, m)), dtype=F64, device=dx.device)
    ws = workspace if workspace is not None else _values_workspace(n, m, T, N, dx.device)
    check(_lib.load().irs_smooth_values(n, m, T, N, _ptr(x_trj, F64), _ptr(u_trj, F64), _ptr(dx, F32), _ptr(du, F32),
                                        _ptr(fz, F32), _ptr(f0, F32), _ptr(fnom, F64), _ptr(o["sums"], F64),
                                        _ptr(o["At"], F64), _ptr(o["Bt"], F64), _ptr(o["ct"], F64), o["info"].data_ptr(),
                                        ws.data_ptr(), ws.numel(), _stream()), "irs_smooth_values")
    return o


# ---- bounded TV-LQR of any size, resumable from tail to tail (csrc/boxqp_values.hip) ----
def box_values_horizon_limit(n, m):
    """The longest horizon the any-size bounded kernel serves at (n, m) (irs_box_values_horizon_limit); 0 for sizes
    out of range.  No launch, no device."""
    return _lib.load().irs_box_values_horizon_limit(int(n), int(m))


_box_values_ws = {}


def _box_values_workspace(n, m, T, device):
    """The cached workspace of the any-size bounded kernel for (`device`, the current stream), grown on demand.  It
    holds one descent's state from `begin` to its last `tail`; one per stream, like the values pass's scratch."""
    need = _lib.load().irs_box_values_workspace_bytes(n, m, T)
    key = (device, _stream())
    ws = _box_values_ws.get(key)
    if ws is None or ws.numel() < need:
        ws = _box_values_ws[key] = torch.empty((max(need, 256),), dtype=torch.uint8, device=device)
    return ws


def _bound_rows(b, width):
    """(tensor, rows) of a bound given as (width,) or (rows, width); (None, 1) for None."""
    if b is None:
        return None, 1
    assert b.shape[-1] == width and b.dim() in (1, 2), tuple(b.shape)
    return b, (1 if b.dim() == 1 else b.shape[0])


def box_values_handle(At, Bt, ct, Q, Qd, R, xd_trj, x_lo=None, x_hi=None, u_lo=None, u_hi=None, alpha_R=0.5, rho=10.0,
                      relax=1.6, workspace=None, info=None):
    """The description of one bounded descent (irs_box_values_call) without a launch: what box_values_begin starts and
    box_values_tail resumes.  Bounds: (n,) / (m,) for every step, or (T+1, n) / (T, m) rows; None = absent.  Keeps the
    tensors it points at alive.  workspace: a uint8 tensor (default: the cached one of this device and stream)."""
    T, n, m = At.shape[0], At.shape[1], Bt.shape[2]
    device = At.device
    ws = workspace if workspace is not None else _box_values_workspace(n, m, T, device)
    if info is None:
        info = torch.zeros((3,), dtype=torch.int32, device=device)
    (x_lo, rx0), (x_hi, rx1) = _bound_rows(x_lo, n), _bound_rows(x_hi, n)
    (u_lo, ru0), (u_hi, ru1) = _bound_rows(u_lo, m), _bound_rows(u_hi, m)
    if (x_lo is not None and x_hi is not None and rx0 != rx1) or (u_lo is not None and u_hi is not None and ru0 != ru1):
        raise ValueError("the two sides of a bound need the same number of rows")
    c = _lib.BoxValuesCall(n=n, m=m, T=T, At=_ptr(At, F64), Bt=_ptr(Bt, F64), ct=_ptr(ct, F64), Q=_ptr(Q, F64),
                           Qd=_ptr(Qd, F64), R=_ptr(R, F64), alpha_R=float(alpha_R), xd_trj=_ptr(xd_trj, F64),
                           x_lo=_ptr(x_lo, F64), x_hi=_ptr(x_hi, F64), x_rows=rx0 if x_lo is not None else rx1,
                           u_lo=_ptr(u_lo, F64), u_hi=_ptr(u_hi, F64), u_rows=ru0 if u_lo is not None else ru1,
                           rho=float(rho), relax=float(relax), workspace=ws.data_ptr(), workspace_bytes=ws.numel(),
                           info=info.data_ptr())
    return dict(call=c, n=n, m=m, T=T, info=info, workspace=ws, device=device,
                keep=(At, Bt, ct, Q, Qd, R, xd_trj, x_lo, x_hi, u_lo, u_hi))


def box_values_begin(At, Bt, ct, Q, Qd, R, xd_trj, x_lo=None, x_hi=None, u_lo=None, u_hi=None, alpha_R=0.5, rho=10.0,
                     relax=1.6, workspace=None, info=None):
    """Start a bounded descent: one launch factorises the whole horizon into the workspace (irs_box_values_begin).
    Returns the handle box_values_tail takes; handle["info"] (3,) int32 is the descent's info."""
    h = box_values_handle(At, Bt, ct, Q, Qd, R, xd_trj, x_lo, x_hi, u_lo, u_hi, alpha_R, rho, relax, workspace, info)
    check(_lib.load().irs_box_values_begin(ctypes.byref(h["call"]), _stream()), "irs_box_values_begin")
    return h


def box_values_tail(h, t, x_t, max_iter=5000, eps=1e-8, u_t=None, x_plan=None, u_plan=None):
    """Solve the tail QP t..T of a begun descent from the state x_t (n) -- one launch, warm started from the previous
    tail (irs_box_values_tail).  Returns u_t (m): the tail's first control, clipped; x_plan (T+1-t, n) / u_plan
    (T-t, m), where given, receive the tail's plan."""
    if u_t is None:
        u_t = torch.empty((h["m"],), dtype=F64, device=h["device"])
    check(_lib.load().irs_box_values_tail(ctypes.byref(h["call"]), int(t), _ptr(x_t, F64), int(max_iter), float(eps),
                                          _ptr(u_t, F64), _ptr(x_plan, F64), _ptr(u_plan, F64), _stream()),
          "irs_box_values_tail")
    return u_t


def box_values_solve(At, Bt, ct, Q, Qd, R, xd_trj, x0, x_lo=None, x_hi=None, u_lo=None, u_hi=None, alpha_R=0.5, rho=10.0,
                     relax=1.6, max_iter=5000, eps=1e-8, workspace=None):
    """solve_tvlqr stand-alone at any size: begin, tail 0, its plan.  Returns dict(x_star, u_star, info[3])."""
    h = box_values_begin(At, Bt, ct, Q, Qd, R, xd_trj, x_lo, x_hi, u_lo, u_hi, alpha_R, rho, relax, workspace)
    T, n, m = h["T"], h["n"], h["m"]
    x_star = torch.zeros((T + 1, n), dtype=F64, device=h["device"])
    u_star = torch.zeros((T, m), dtype=F64, device=h["device"])
    box_values_tail(h, 0, x0, max_iter, eps, x_plan=x_star, u_plan=u_star)
    return dict(x_star=x_star, u_star=u_star, info=h["info"])


# ---- model-free CEM rollout (csrc/cem.hip, cem_values_stage_kernel): the caller steps the plant between the stages ----
def cem_values_stage(t, x, src, Q, R, xd_trj, u_t, costs):
    """Stage t of the B candidate rollouts of `src` -- a CemSource, or the supplied candidates u_cand (B,T,m)
    themselves (irs_cem_values_stage[_drawn]): x (B,n) are the states at step t; costs (B) gets this stage's cost terms
    (written at t = 0, added after), u_t (B,m) the controls of step t (None at t = T).  One launch."""
    if not isinstance(src, CemSource):
        src = CemSource.supplied(src)
    name = "irs_cem_values_stage" + src.suffix
    check(getattr(_lib.load(), name)(x.shape[1], src.m, src.T, src.B, int(t), _ptr(x, F64), *src.args, _ptr(Q, F64),
                                     _ptr(R, F64), _ptr(xd_trj, F64), _ptr(u_t, F64), _ptr(costs, F64), _stream()), name)


def cem_values_stage_drawn(t, x, u_mean, std, seed, it, sample_offset, Q, R, xd_trj, u_t, costs):
    """cem_values_stage with the controls drawn around u_mean (T,m) with std (T,m) -- the stream of cem_candidates --
    for the B = x.shape[0] candidates sample_offset .. sample_offset + B."""
    cem_values_stage(t, x, CemSource.drawn(u_mean, std, x.shape[0], seed, it, sample_offset), Q, R, xd_trj, u_t, costs)
