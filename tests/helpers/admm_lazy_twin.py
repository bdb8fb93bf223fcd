"""NumPy twin of the bounded TV-LQR kernel's lazily enforced bounds (box_descent_kernel<.., LAZY = true>,
irs_mpc_amd/csrc/boxqp.hip), built from the oracle's tvlqr_box_factor / tvlqr_box_solve alone: one ADMM iteration is one
call of tvlqr_box_solve with max_iter = 1, and a component whose bound is not enforced is handed to the oracle with the
bounds -inf / +inf on every row, so the arithmetic of the factorisation and of an iteration is the oracle's own.

The rule (constraint generation).  Components: [x (n) | u (m)].  Only the components of the set S carry a rho term and
are projected; S starts from `enforced` (entries of components without a finite bound are ignored) and only grows.

    when a tail converges (max(rp, rho rd) < eps over the components of S; with S empty, after one iteration):
        V = the components outside S with a finite bound whose plan entry leaves its bounds on a row of the tail,
            z < lo or z > hi with no tolerance (x rows t > t0, u rows t >= t0)
        if V is empty: the tail is done -- its plan is feasible for the full box and optimal for a relaxation of the
            full QP, hence the full QP's solution to the ADMM's tolerance
        else: S <- S + V;  on the tail's rows of the components of V:  w <- clip(z, lo, hi),  y <- 0;
            the Riccati factor is rebuilt with the new masks; the same tail goes on, its iteration count running on
            against max_iter (one event: (t0, V))
    a tail that ends at max_iter is not checked.

S persists across the warm-started tails of a descent.  The adaptive penalty (tests/helpers/admm_adaptive_twin.py: the
same rule, its maxima over the components of S) may run on top.
"""
import numpy as np

from oracle import irs_oracle as orc
from tests.helpers.admm_adaptive_twin import CHECK_EVERY, MAX_REFACTOR, RATIO_CLIP, TRIGGER


class LazyBoxAdmm:
    """The factor, the enforced set, the current rho and the counters of one launch (a descent or a single solve)."""

    def __init__(self, At, Bt, ct, Q, Qd, R, xlo, xhi, ulo, uhi, rho, alpha_R=0.5, enforced=None, adaptive=False,
                 check_every=CHECK_EVERY, trigger=TRIGGER, max_refactor=MAX_REFACTOR):
        T, n, m = At.shape[0], Q.shape[0], R.shape[0]
        self.mats = (At, Bt, ct, Q, Qd, R)
        self.T, self.n, self.m = T, n, m
        # the full box, one row per time step (row t of x bounds x_t, of u bounds u_t)
        self.xlo, self.xhi = np.array(orc._rows(xlo, T + 1, n)), np.array(orc._rows(xhi, T + 1, n))
        self.ulo, self.uhi = np.array(orc._rows(ulo, T, m)), np.array(orc._rows(uhi, T, m))
        finite = np.concatenate([(np.isfinite(self.xlo) | np.isfinite(self.xhi)).any(axis=0),
                                 (np.isfinite(self.ulo) | np.isfinite(self.uhi)).any(axis=0)])
        start = np.zeros(n + m, bool) if enforced is None else np.asarray(enforced).astype(bool)
        assert start.shape == (n + m,)
        self.finite, self.set = finite, finite & start
        self.alpha_R, self.rho = alpha_R, float(rho)
        self.adaptive, self.check_every, self.trigger, self.max_refactor = adaptive, check_every, trigger, max_refactor
        self.factorisations, self.events, self.iterations = 0, [], 0
        self._factor()

    def _box(self):
        """The box the oracle sees: the full one on the components of the set, +-inf elsewhere."""
        sx, su = self.set[:self.n], self.set[self.n:]
        return (np.where(sx, self.xlo, -np.inf), np.where(sx, self.xhi, np.inf),
                np.where(su, self.ulo, -np.inf), np.where(su, self.uhi, np.inf))

    def _factor(self):
        self.box = self._box()
        self.F = orc.tvlqr_box_factor(*self.mats, *self.box, self.rho, alpha_R=self.alpha_R)
        self.factorisations += 1

    def _violated(self, zx, zu, t0):
        """The dropped components whose plan entry leaves its bounds on a row of the tail."""
        out_x = ((zx[t0 + 1:] < self.xlo[t0 + 1:]) | (zx[t0 + 1:] > self.xhi[t0 + 1:])).any(axis=0)
        out_u = ((zu[t0:] < self.ulo[t0:]) | (zu[t0:] > self.uhi[t0:])).any(axis=0)
        return np.concatenate([out_x, out_u]) & self.finite & ~self.set

    def solve(self, xd, x_start, t0, state=None, max_iter=5000, eps=1e-8, relax=1.0):
        """One tail problem.  Returns zx, zu, state, iterations, converged."""
        At, Bt, ct, Q, Qd, R = self.mats
        T, n, m = self.T, self.n, self.m
        if state is None:
            state = (np.zeros((T + 1, n)), np.zeros((T + 1, n)), np.zeros((T, m)), np.zeros((T, m)))
        it, conv, refactors = 0, False, 0
        zx = zu = None
        while it < max_iter and not conv:
            it += 1
            mx, mu = self.F["mx"], self.F["mu"]
            wx_prev, wu_prev = state[0][t0 + 1:].copy(), state[2][t0:].copy()
            zx, zu, state, _ = orc.tvlqr_box_solve(self.F, At, Bt, ct, Q, Qd, xd, x_start, t0, *self.box, state, 1, eps,
                                                   relax)
            wx, yx, wu, yu = state
            rp = max(np.abs(mx * (zx[t0 + 1:] - wx[t0 + 1:])).max(), np.abs(mu * (zu[t0:] - wu[t0:])).max())
            rdw = max(np.abs(mx * (wx[t0 + 1:] - wx_prev)).max(), np.abs(mu * (wu[t0:] - wu_prev)).max())
            conv = max(rp, self.rho * rdw) < eps
            if self.adaptive and not conv and it % self.check_every == 0 and refactors < self.max_refactor:
                pn = max(np.abs(mx * zx[t0 + 1:]).max(), np.abs(mx * wx[t0 + 1:]).max(),
                         np.abs(mu * zu[t0:]).max(), np.abs(mu * wu[t0:]).max())
                dn = self.rho * max(np.abs(mx * yx[t0 + 1:]).max(), np.abs(mu * yu[t0:]).max())
                rd = self.rho * rdw
                if rp > 0.0 and rd > 0.0 and pn > 0.0 and dn > 0.0:
                    ratio = min(max(np.sqrt((rp / pn) / (rd / dn)), RATIO_CLIP[0]), RATIO_CLIP[1])
                    if ratio > self.trigger or ratio * self.trigger < 1.0:
                        s = 1.0 / ratio
                        self.rho *= ratio
                        yx[t0 + 1:] *= s
                        yu[t0:] *= s
                        self._factor()
                        refactors += 1
            if conv:
                new = self._violated(zx, zu, t0)
                if new.any():
                    nx, nu = new[:n], new[n:]
                    wx[t0 + 1:, nx] = np.clip(zx[t0 + 1:, nx], self.xlo[t0 + 1:, nx], self.xhi[t0 + 1:, nx])
                    yx[t0 + 1:, nx] = 0.0
                    wu[t0:, nu] = np.clip(zu[t0:, nu], self.ulo[t0:, nu], self.uhi[t0:, nu])
                    yu[t0:, nu] = 0.0
                    self.set = self.set | new
                    self.events.append((t0, tuple(int(i) for i in np.flatnonzero(new))))
                    self._factor()
                    conv = False
        self.iterations += it
        return zx, zu, state, it, conv


def local_descent_box_lazy(system, At, Bt, ct, Q, Qd, R, x0, xd_trj, xlo, xhi, ulo, uhi, rho=10.0, max_iter=5000,
                           eps=1e-8, relax=1.0, enforced=None, adaptive=False, **rule):
    """oracle local_descent_box with lazily enforced bounds (and, adaptive, the adaptive penalty on top).  Returns x_new,
    u_new, iters (per tail), failed tails (list of t), events (list of (tail, components)), the final set ((n + m,)
    bool), the LazyBoxAdmm (final rho, factorisation count)."""
    T, n, m = At.shape[0], system.dim_x, system.dim_u
    adm = LazyBoxAdmm(At, Bt, ct, Q, Qd, R, xlo, xhi, ulo, uhi, rho, enforced=enforced, adaptive=adaptive, **rule)
    x_new, u_new = np.zeros((T + 1, n)), np.zeros((T, m))
    x_new[0] = x0
    state, iters, failed = None, [], []
    for t in range(T):
        zx, zu, state, it, conv = adm.solve(xd_trj, x_new[t], t, state, max_iter, eps, relax)
        iters.append(it)
        if not conv:
            failed.append(t)
        u_new[t] = np.clip(zu[t], adm.ulo[t], adm.uhi[t])          # the first control: clipped to ALL bounds
        x_new[t + 1] = system.dynamics(x_new[t], u_new[t])
    return x_new, u_new, iters, failed, list(adm.events), adm.set.copy(), adm
