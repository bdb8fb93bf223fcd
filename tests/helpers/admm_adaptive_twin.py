"""NumPy twin of the bounded TV-LQR kernel's adaptive ADMM penalty (box_descent_kernel<.., ADAPT = true>,
irs_mpc_amd/csrc/boxqp.hip), built from the oracle's tvlqr_box_factor / tvlqr_box_solve: one ADMM iteration is one
call of tvlqr_box_solve with max_iter = 1, so the arithmetic of an iteration is the oracle's own.

The rule (residual balancing, as OSQP adapts its rho), applied after every `check_every`-th iteration of a tail that
has not converged, at most `max_refactor` times per tail:

    rp = max |z - w|,  rd = rho max |w - w_prev|       the residuals the convergence test already forms
    pn = max(|z|, |w|),  dn = rho max |y|              their scales (y: the scaled duals, rho y the multipliers)
    ratio = sqrt((rp / pn) / (rd / dn)), clipped to [1e-2, 1e2]
    if ratio > trigger or ratio < 1 / trigger:
        rho <- rho ratio;  y <- y rho_old / rho_new (the multipliers stay);  the Riccati factor is rebuilt

all maxima over the bounded components of the tail (x_t, t > t0; u_t, t >= t0).  A check whose four quantities are
not all positive is skipped.  The new rho stays for the following warm-started tails of a descent.
"""
import numpy as np

from oracle import irs_oracle as orc

# the constants the product ships as defaults (irs_admm_settings: check_every, trigger, max_refactor)
CHECK_EVERY, TRIGGER, MAX_REFACTOR = 1000, 5.0, 4
RATIO_CLIP = (1e-2, 1e2)


class AdaptiveBoxAdmm:
    """The factor, the current rho and the counters of one launch (a descent or a single solve)."""

    def __init__(self, At, Bt, ct, Q, Qd, R, xlo, xhi, ulo, uhi, rho, alpha_R=0.5, check_every=CHECK_EVERY,
                 trigger=TRIGGER, max_refactor=MAX_REFACTOR, adaptive=True):
        self.prob = (At, Bt, ct, Q, Qd, R, xlo, xhi, ulo, uhi)
        self.alpha_R, self.rho = alpha_R, float(rho)
        self.check_every, self.trigger, self.max_refactor, self.adaptive = check_every, trigger, max_refactor, adaptive
        self.factorisations = 0
        self._factor()

    def _factor(self):
        self.F = orc.tvlqr_box_factor(*self.prob, self.rho, alpha_R=self.alpha_R)
        self.factorisations += 1

    def solve(self, xd, x_start, t0, state=None, max_iter=5000, eps=1e-8, relax=1.0):
        """One tail problem.  Returns zx, zu, state, iterations, converged."""
        At, Bt, ct, Q, Qd, R, xlo, xhi, ulo, uhi = self.prob
        T, n, m = At.shape[0], Q.shape[0], R.shape[0]
        if state is None:
            state = (np.zeros((T + 1, n)), np.zeros((T + 1, n)), np.zeros((T, m)), np.zeros((T, m)))
        mx, mu = self.F["mx"], self.F["mu"]
        it, conv, refactors = 0, False, 0
        zx = zu = None
        while it < max_iter and not conv:
            it += 1
            wx_prev, wu_prev = state[0][t0 + 1:].copy(), state[2][t0:].copy()
            zx, zu, state, _ = orc.tvlqr_box_solve(self.F, At, Bt, ct, Q, Qd, xd, x_start, t0, xlo, xhi, ulo, uhi,
                                                   state, 1, eps, relax)
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
                        s = 1.0 / ratio                       # rho_old / rho_new
                        self.rho *= ratio
                        yx[t0 + 1:] *= s
                        yu[t0:] *= s
                        self._factor()
                        refactors += 1
        return zx, zu, state, it, conv


def local_descent_box_adaptive(system, At, Bt, ct, Q, Qd, R, x0, xd_trj, xlo, xhi, ulo, uhi, rho=10.0, max_iter=5000,
                               eps=1e-8, relax=1.0, adaptive=True, **rule):
    """oracle local_descent_box with the adaptive rule.  Returns x_new, u_new, iters (per tail), failed tails (list of
    t), the AdaptiveBoxAdmm (final rho, factorisation count)."""
    T, n, m = At.shape[0], system.dim_x, system.dim_u
    adm = AdaptiveBoxAdmm(At, Bt, ct, Q, Qd, R, xlo, xhi, ulo, uhi, rho, adaptive=adaptive, **rule)
    x_new, u_new = np.zeros((T + 1, n)), np.zeros((T, m))
    x_new[0] = x0
    state, iters, failed = None, [], []
    ulo_t, uhi_t = orc._rows(ulo, T, m), orc._rows(uhi, T, m)
    for t in range(T):
        zx, zu, state, it, conv = adm.solve(xd_trj, x_new[t], t, state, max_iter, eps, relax)
        iters.append(it)
        if not conv:
            failed.append(t)
        u_new[t] = np.clip(zu[t], ulo_t[t], uhi_t[t])
        x_new[t + 1] = system.dynamics(x_new[t], u_new[t])
    return x_new, u_new, iters, failed, adm
