"""Bring-your-own dynamics: a system defined by a torch callable instead of a device functor.

    class CartPole(TorchDynamicalSystem):
        def __init__(self, h):
            super().__init__()
            self.h, self.dim_x, self.dim_u = h, 4, 1

        def dynamics_batch_torch(self, x, u):      # (B,n), (B,m) GPU tensors -> (B,n)
            ...

    IrsLqrZeroOrder(CartPole(0.02), params, GaussianSmoothing(...)).iterate(10)

`dynamics_batch_torch` is all a subclass has to write.  It is called
  * in float32 with B = T (N + 1) rows by the zero-order sample pass: the N perturbed points of every timestep and
    the nominal point, in ONE call, so that dF = f(x + dx, u + du) - f(x, u) is a difference of values from the same
    code in the same precision;
  * in float64 with one row per step by rollouts (T calls per rollout, on the current stream, no host read between
    them), and with T rows for the nominal steps c_t is measured from.
`jacobian_xu_batch_torch(x, u) -> (B, n, n+m)` is optional; without it the Jacobians come from
torch.func.vmap(torch.func.jacrev(.)) of `dynamics_batch_torch` in float64, which needs a callable that torch.func can
transform (no in-place writes into its inputs, no data-dependent Python branches).

What runs where: the callable evaluates the model; the per-timestep statistics Z'Z and Z'dF of all T timesteps and
their least-squares solves are the values pass (csrc/smooth_values.hip, device.smooth_values); the Riccati pass, the
cost and the plan test are the model-free kernels every compiled system uses; the first-order mode is the float64 mean
of the sampled Jacobians in torch.

Bounds: a box bound that binds takes the stepped bounded descent when IrsLqrParameters.qp_model_free is set
(TorchDeviceModel.tvlqr_box_descent: one factorisation, then per t one tail-QP launch of csrc/boxqp_values.hip and one
float64 step of the callable, all on the current stream with nothing read on the host); without the flag it raises
NotImplementedError, as a compiled model is then needed.

CrossEntropyMethod: the B candidate rollouts are T + 1 stage launches of csrc/cem.hip (cem_values_stage_kernel: the
candidate's control of step t out, its cost terms in) with one float64 call of the callable on (B,n), (B,m) between
two of them; selection and refit are the model-free kernels of the compiled systems.  With CemParameters.device_seed
the candidates are drawn inside the stages, no (B,T,m) tensor exists, and `iterate` enqueues every descent before it
reads anything back (TorchDeviceModel.cem_iterate).

Limits: dim_x <= 32, dim_u <= 16; samples are evaluated in float32; a rollout is T torch steps; the bounded descent
has the fixed penalty only (qp_adaptive_rho and qp_lazy_bounds are compiled-only) and a horizon limit
(box_horizon_limit); no fused `irs_iterate` loop; the candidate rollouts of a CEM descent are T + 1 stage launches and
T calls of the callable where a compiled system's are one launch.  The quasistatic classes (CrossEntropyMethodQuasistatic among them) and the
position-controlled form of `solve_tvlqr` stay compiled-models-only.
"""
import numpy as np
import torch

from . import _lib
from . import device as dev
from ._lib import SMOOTH_FIRST_ORDER, SMOOTH_ZERO_ORDER_AB, check, dbl_array
from .dynamical_system import DynamicalSystem

MAX_DIM_X, MAX_DIM_U = 32, 16       # the generic Riccati kernel's and the values pass's limits

class TorchDynamicalSystem(DynamicalSystem):
    """A DynamicalSystem whose dynamics are a torch callable; see the module docstring."""

    def dynamics_batch_torch(self, x, u):
        raise NotImplementedError("This class is virtual.")

    def dm(self):
        if getattr(self, "_dm", None) is None:
            self._dm = TorchDeviceModel(self)
        return self._dm

    # ---- the reference's four virtuals (NumPy float64 in and out), served from the torch callable ----
    def dynamics(self, x, u):
        return self.dynamics_batch(np.asarray(x, float)[None, :], np.asarray(u, float)[None, :])[0]

    def dynamics_batch(self, x, u):
        return self.dm().dynamics_batch(dev.to_dev(x), dev.to_dev(u)).cpu().numpy()

    def jacobian_xu(self, x, u):
        return self.jacobian_xu_batch(np.asarray(x, float)[None, :], np.asarray(u, float)[None, :])[0]

    def jacobian_xu_batch(self, x, u):
        return self.dm().jacobian_xu_batch(dev.to_dev(x), dev.to_dev(u)).cpu().numpy()


class TorchDeviceModel(dev.CemModelFree):
    """What `IrsLqr` and `CrossEntropyMethod` call on `system.dm()`, for a TorchDynamicalSystem: the method names,
    signatures and result keys of device.DeviceModel."""

    compiled = False            # no device functor: no fused loop; bounded descents are stepped (tvlqr_box_descent)
    model_id = None

    def __init__(self, system):
        self.system = system
        self.n, self.m = int(system.dim_x), int(system.dim_u)
        if not (1 <= self.n <= MAX_DIM_X and 1 <= self.m <= MAX_DIM_U):
            raise ValueError("TorchDynamicalSystem needs 1 <= dim_x <= %d and 1 <= dim_u <= %d, got (%d, %d)"
                             % (MAX_DIM_X, MAX_DIM_U, self.n, self.m))
        self.lib = _lib.load()

    # ---- the callable ---------------------------------------------------------------------------------------
    def _f(self, X, U):
        with torch.no_grad():
            Y = self.system.dynamics_batch_torch(X, U)
        if not (isinstance(Y, torch.Tensor) and tuple(Y.shape) == (X.shape[0], self.n) and Y.dtype == X.dtype
                and Y.device == X.device):
            raise TypeError("dynamics_batch_torch must return a (%d, %d) %s tensor on %s, got %s"
                            % (X.shape[0], self.n, X.dtype, X.device,
                               (tuple(Y.shape), Y.dtype, Y.device) if isinstance(Y, torch.Tensor) else type(Y)))
        return Y.contiguous()

    def dynamics_batch(self, X, U):
        return self._f(X, U)

    def jacobian_xu_batch(self, X, U):
        user = getattr(self.system, "jacobian_xu_batch_torch", None)
        if user is not None:
            with torch.no_grad():
                J = user(X, U)
        else:
            def one(x, u):
                return self.system.dynamics_batch_torch(x[None, :], u[None, :])[0]
            Jx, Ju = torch.func.vmap(torch.func.jacrev(one, argnums=(0, 1)))(X, U)
            J = torch.cat([Jx, Ju], dim=2)
        if tuple(J.shape) != (X.shape[0], self.n, self.n + self.m) or J.dtype != X.dtype:
            raise TypeError("the Jacobian must be a (%d, %d, %d) %s tensor, got %s %s"
                            % (X.shape[0], self.n, self.n + self.m, X.dtype, tuple(J.shape), J.dtype))
        return J.detach().contiguous()

    def _step(self, x, u):
        return self._f(x[None, :], u[None, :])[0]

    def rollout_cost(self, x0, u_trj, Q, R, xd_trj):
        T = u_trj.shape[0]
        xs = [x0]
        for t in range(T):
            xs.append(self._step(xs[-1], u_trj[t]))
        x_trj = torch.stack(xs)
        return x_trj, dev.evaluate_cost(x_trj, u_trj, Q, R, xd_trj)

    # ---- smoothing ------------------------------------------------------------------------------------------
    def sums_len(self, mode):
        if mode == SMOOTH_ZERO_ORDER_AB:
            return dev.values_sums_len(self.n, self.m)
        if mode == SMOOTH_FIRST_ORDER:
            return self.n * (self.n + self.m)
        raise NotImplementedError("smoothing mode %d needs a compiled (contact) model" % mode)

    def smooth_geometry(self, mode, T, N, rng=False):
        return dev.smooth_values_geometry(T, N)

    def _values(self, x_trj, u_trj, dx, du):
        """The float32 evaluation of the zero-order pass: every sample and, behind them in the same call, the nominal
        points.  Returns fz (T,N,n), f0 (T,n): two views of the callable's one result."""
        T, N = du.shape[0], du.shape[1]
        x32, u32 = x_trj[:T].to(dev.F32), u_trj[:T].to(dev.F32)
        X = torch.cat([(x32[:, None, :] + dx).reshape(T * N, self.n), x32])
        U = torch.cat([(u32[:, None, :] + du).reshape(T * N, self.m), u32])
        Y = self._f(X, U)
        return Y[:T * N].view(T, N, self.n), Y[T * N:]

    def _fnom(self, x_trj, u_trj):
        T = u_trj.shape[0]
        return self._f(x_trj[:T].contiguous(), u_trj)

    def _jacobian_sums(self, x_trj, u_trj, dx, du):
        """FIRST_ORDER statistics: the float64 sum over the samples of the Jacobians [A | B], (T, n (n+m))."""
        T, N = du.shape[0], du.shape[1]
        X = (x_trj[:T, None, :] + dx.to(dev.F64)).reshape(T * N, self.n)
        U = (u_trj[:T, None, :] + du.to(dev.F64)).reshape(T * N, self.m)
        J = self.jacobian_xu_batch(X, U)
        return J.view(T, N, self.n * (self.n + self.m)).sum(dim=1)

    def _from_jacobian_sums(self, N_total, x_trj, u_trj, sums):
        T, n = u_trj.shape[0], self.n
        AB = (sums / float(N_total)).view(T, n, n + self.m)
        At, Bt = AB[:, :, :n].contiguous(), AB[:, :, n:].contiguous()
        ct = self._fnom(x_trj, u_trj) - torch.einsum("tij,tj->ti", At, x_trj[:T]) - torch.einsum("tij,tj->ti", Bt, u_trj)
        return At, Bt, ct, torch.zeros((T,), dtype=torch.int32, device=u_trj.device)

    def smooth(self, mode, x_trj, u_trj, dx, du, out=None):
        """get_TV_matrices on supplied samples dx (T,N,n), du (T,N,m) f32 -> dict(sums, At, Bt, ct, info)."""
        if mode == SMOOTH_ZERO_ORDER_AB:
            fz, f0 = self._values(x_trj, u_trj, dx, du)
            return dev.smooth_values(x_trj, u_trj, dx, du, fz, f0, self._fnom(x_trj, u_trj), out=out)
        sums = self.smooth_accumulate(mode, x_trj, u_trj, dx, du)
        At, Bt, ct, info = self._from_jacobian_sums(du.shape[1], x_trj, u_trj, sums)
        return dict(sums=sums, At=At, Bt=Bt, ct=ct, info=info)

    def rng_samples(self, T, N, std_x, std_u, seed, it, sample_offset=0):
        """The Philox draws of the compiled models' sample pass, as tensors: through irs_rng_samples, and where that
        entry has no instantiation for (n, m) (IRS_ERR_UNSUPPORTED, decided before any launch) through its any-size
        twin irs_values_rng_samples, which writes the same stream."""
        device = dev.require_gpu()
        dx = torch.empty((T, N, self.n), dtype=dev.F32, device=device)
        du = torch.empty((T, N, self.m), dtype=dev.F32, device=device)
        args = (self.n, self.m, T, N, dbl_array(std_x), dbl_array(std_u), int(seed), int(it), int(sample_offset),
                dx.data_ptr(), du.data_ptr(), dev._stream())
        rc = self.lib.irs_rng_samples(*args)
        if rc == _lib.IRS_ERR_UNSUPPORTED:
            check(self.lib.irs_values_rng_samples(*args), "irs_values_rng_samples")
        else:
            check(rc, "irs_rng_samples")
        return dx, du

    def smooth_rng(self, mode, x_trj, u_trj, N, std_x, std_u, seed, it, out=None):
        dx, du = self.rng_samples(u_trj.shape[0], N, std_x, std_u, seed, it)
        return self.smooth(mode, x_trj, u_trj, dx, du, out=out)

    def smooth_accumulate(self, mode, x_trj, u_trj, dx, du, sums=None):
        if mode == SMOOTH_ZERO_ORDER_AB:
            fz, f0 = self._values(x_trj, u_trj, dx, du)
            return dev.smooth_values_accumulate(dx, du, fz, f0, sums=sums)
        if mode != SMOOTH_FIRST_ORDER:
            raise NotImplementedError("smoothing mode %d needs a compiled (contact) model" % mode)
        s = self._jacobian_sums(x_trj, u_trj, dx, du)
        if sums is not None:
            sums.copy_(s)
            return sums
        return s

    def smooth_accumulate_rng(self, mode, x_trj, u_trj, N, std_x, std_u, seed, it, sample_offset=0, sums=None):
        dx, du = self.rng_samples(u_trj.shape[0], N, std_x, std_u, seed, it, sample_offset)
        return self.smooth_accumulate(mode, x_trj, u_trj, dx, du, sums=sums)

    def smooth_finalize(self, mode, N_total, x_trj, u_trj, sums, out=None, workspace=None):
        if mode == SMOOTH_ZERO_ORDER_AB:
            o = None
            if out is not None:
                o = dict(zip(("At", "Bt", "ct", "info"), out))
            return dev.smooth_values_finalize(N_total, x_trj, u_trj, self._fnom(x_trj, u_trj), sums, m=self.m, out=o)
        return self._from_jacobian_sums(N_total, x_trj, u_trj, sums)

    def exact_linearize(self, x_trj, u_trj):
        T, n = u_trj.shape[0], self.n
        J = self.jacobian_xu_batch(x_trj[:T].contiguous(), u_trj)
        return self._from_jacobian_sums(1, x_trj, u_trj, J.reshape(T, n * (n + self.m)))[:3]

    # ---- descent --------------------------------------------------------------------------------------------
    def closed_loop_rollout(self, K, k, x0, Q, R, xd_trj):
        """u_t = K_t x_t + k_t, x_{t+1} = f(x_t, u_t): T float64 torch steps, nothing read on the host."""
        xs, us = [x0], []
        for t in range(K.shape[0]):
            us.append(K[t] @ xs[-1] + k[t])
            xs.append(self._step(xs[-1], us[-1]))
        x_new, u_new = torch.stack(xs), torch.stack(us)
        return x_new, u_new, dev.evaluate_cost(x_new, u_new, Q, R, xd_trj)

    def tvlqr_descent(self, At, Bt, ct, Q, Qd, R, xd_trj, x0, alpha_R=0.5, out=None):
        """Riccati backward pass (irs_tvlqr_riccati), the closed-loop rollout through the callable, the cost."""
        K, k, info = dev.tvlqr_riccati(At, Bt, ct, Q, Qd, R, xd_trj, alpha_R=alpha_R)
        x_new, u_new, cost = self.closed_loop_rollout(K, k, x0, Q, R, xd_trj)
        return dict(K=K, k=k, x_new=x_new, u_new=u_new, cost=cost, info=info)

    def box_descent_supported(self, T, du=False):
        """Whether the stepped bounded descent runs horizon T (the plain form only: du has no any-size kernel)."""
        return 0 < int(T) <= self.box_horizon_limit(du)

    def box_horizon_limit(self, du=False):
        """The longest horizon of the any-size bounded kernel at this (n, m) (irs_box_values_horizon_limit)."""
        return 0 if du else dev.box_values_horizon_limit(self.n, self.m)

    def tvlqr_box_descent(self, At, Bt, ct, Q, Qd, R, xd_trj, x0, xlo, xhi, ulo, uhi, alpha_R=0.5,
                          rho=10.0, relax=1.6, max_iter=5000, eps=1e-8, records_in_hbm=False, adaptive_rho=False,
                          lazy_bounds=False, enforced=None):
        """local_descent with active abs bounds, the signature and result keys of DeviceModel.tvlqr_box_descent:
        one factorisation (irs_box_values_begin), then for every t one warm-started tail QP (irs_box_values_tail)
        and one float64 step of the callable from the realised state -- 1 + T launches and T torch steps on the
        current stream, nothing read on the host.  The factor records are always in HBM.  Returns
        dict(x_new, u_new, info[3])."""
        if adaptive_rho or lazy_bounds:
            raise NotImplementedError("the stepped bounded descent of a TorchDynamicalSystem has the fixed penalty only: "
                                      "%s needs a compiled device model" % ("qp_adaptive_rho" if adaptive_rho
                                                                            else "qp_lazy_bounds"))
        T = At.shape[0]
        x_new = torch.empty((T + 1, self.n), dtype=dev.F64, device=At.device)
        u_new = torch.empty((T, self.m), dtype=dev.F64, device=At.device)
        h = dev.box_values_begin(At, Bt, ct, Q, Qd, R, xd_trj, xlo, xhi, ulo, uhi, alpha_R=alpha_R, rho=rho, relax=relax)
        x_new[0] = x0
        for t in range(T):
            dev.box_values_tail(h, t, x_new[t], max_iter, eps, u_t=u_new[t])
            x_new[t + 1] = self._step(x_new[t], u_new[t])
        return dict(x_new=x_new, u_new=u_new, info=h["info"])

    # ---- CEM baseline: DeviceModel's surface (the public names, selection and refit: dev.CemModelFree) -------------
    _NO_QUASISTATIC_CEM = ("the quasistatic CEM cost needs a compiled position-controlled model; a "
                           "TorchDynamicalSystem runs CrossEntropyMethod only")

    def _cem_rollout(self, src, x0, Q, R, xd_trj):
        """The time loop of the B rollouts of `src`: dev.cem_values_stage for t = 0..T with one float64 call of the
        callable between two stages -- T + 1 launches and T torch steps on the current stream, nothing read on the
        host."""
        x = x0.expand(src.B, self.n).contiguous()
        u_t = torch.empty((src.B, self.m), dtype=dev.F64, device=x0.device)
        costs = torch.empty((src.B,), dtype=dev.F64, device=x0.device)
        for t in range(src.T):
            dev.cem_values_stage(t, x, src, Q, R, xd_trj, u_t, costs)
            x = self._f(x, u_t)
        dev.cem_values_stage(src.T, x, src, Q, R, xd_trj, None, costs)
        return costs

    def cem_costs(self, src, x0, Q, R, xd_trj, Qd=None):
        if Qd is not None:
            raise NotImplementedError(self._NO_QUASISTATIC_CEM)
        return self._cem_rollout(src, x0, Q, R, xd_trj)

    def cem_iterate(self, u_trj0, std0, x0, Q, Qd, R, xd_trj, B, n_elite, n_descents, seed, iter0=1,
                    quasistatic=False):
        """n_descents CEM descents enqueued back to back, nothing read back: the dict of device histories
        DeviceModel.cem_iterate returns -- u_hist, std_hist (n_descents,T,m), x_hist (n_descents,T+1,n), cost_hist
        (n_descents).  Descent i draws around descent i - 1's refit with generator iteration iter0 + i, as
        irs_cem_iterate does; here the loop is the host's and only enqueues."""
        if quasistatic:
            raise NotImplementedError(self._NO_QUASISTATIC_CEM)
        o = self._cem_histories(u_trj0, n_descents)
        mean, std = u_trj0, std0
        for i in range(int(n_descents)):
            src = dev.CemSource.drawn(mean, std, B, seed, int(iter0) + i)
            _, mean, std = self.cem_refit_from(src, self.cem_costs(src, x0, Q, R, xd_trj), n_elite)
            x_new, cost = self.rollout_cost(x0, mean, Q, R, xd_trj)        # the mean's rollout (cem.py:182)
            for key, v in (("u_hist", mean), ("std_hist", std), ("x_hist", x_new)):
                o[key][i].copy_(v)
            o["cost_hist"][i:i + 1].copy_(cost.reshape(1))
        return o
