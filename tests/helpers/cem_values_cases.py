"""Inputs and NumPy statements for the model-free CEM rollout (csrc/cem.hip, cem_values_stage_kernel), shared by
tests/test_cem_values_gpu.py and the seed search that chose its inputs.

NumpyCartPole / NumpyPendulum restate examples/torch_systems.py operation for operation in float64: `dynamics(x, u)` is
what oracle.irs_oracle.rollout steps, `dynamics_batch` the same on rows (the seed search rolls 50 000 candidates out).
"""
import numpy as np

U = 2.0 ** -53          # unit roundoff of float64


class NumpyCartPole:
    """examples/torch_systems.py, TorchCartPole."""

    def __init__(self, h, m_cart=1.0, m_pole=0.1, length=0.5, gravity=9.81):
        self.h, self.dim_x, self.dim_u = h, 4, 1
        self.mc, self.mp, self.l, self.g = m_cart, m_pole, length, gravity

    def dynamics_batch(self, x, u):
        th, xd, thd, f = x[:, 1], x[:, 2], x[:, 3], u[:, 0]
        s, c = np.sin(th), np.cos(th)
        den = self.mc + self.mp * s * s
        xdd = (f + self.mp * s * (self.l * thd * thd + self.g * c)) / den
        thdd = (-f * c - self.mp * self.l * thd * thd * c * s - (self.mc + self.mp) * self.g * s) / (self.l * den)
        return x + self.h * np.stack([xd, thd, xdd, thdd], axis=1)

    def dynamics(self, x, u):
        return self.dynamics_batch(np.asarray(x, float)[None, :], np.asarray(u, float)[None, :])[0]


class NumpyPendulum:
    """examples/torch_systems.py, TorchPendulum."""

    def __init__(self, h):
        self.h, self.dim_x, self.dim_u = h, 2, 1

    def dynamics_batch(self, x, u):
        next_speed = x[:, 1] + self.h * (-np.sin(x[:, 0]) + u[:, 0])
        next_angle = x[:, 0] + self.h * next_speed
        return np.stack([next_angle, next_speed], axis=1)

    def dynamics(self, x, u):
        return self.dynamics_batch(np.asarray(x, float)[None, :], np.asarray(u, float)[None, :])[0]


def rollout_costs(system, x0, cand, Q, R, xd_trj):
    """costs (B) of the candidates cand (B,T,m): cem.py:163-168 on rows."""
    B, T = cand.shape[0], cand.shape[1]
    x = np.tile(np.asarray(x0, float), (B, 1))
    costs = np.zeros(B)
    for t in range(T + 1):
        e = x - xd_trj[t]
        costs += np.einsum("bi,ij,bj->b", e, Q, e)
        if t < T:
            costs += np.einsum("bi,ij,bj->b", cand[:, t], R, cand[:, t])
            x = system.dynamics_batch(x, cand[:, t])
    return costs


def threshold_gap(costs, n_elite):
    """The relative gap between the n_elite-th and the (n_elite + 1)-th smallest cost: what a rounding error has to
    exceed to change the elite set."""
    c = np.sort(np.asarray(costs, float))
    assert np.isfinite(c).all()
    return (c[n_elite] - c[n_elite - 1]) / abs(c[n_elite - 1])


# ---- the stage alone ------------------------------------------------------------------------------------------------
STAGE_SIZES = [(1, 1), (4, 1), (7, 3), (12, 4), (32, 16)]
STAGE_HORIZONS = [1, 12]
STAGE_BATCHES = [1, 63, 65, 1000]


def dense_weight(rng, k):
    """L L' + I: dense, not diagonal, positive definite."""
    L = rng.normal(size=(k, k))
    return L @ L.T + np.eye(k)


def stage_case(n, m, T, B, seed=0):
    """Random states for every stage 0..T (no dynamics: the stages are chained on arbitrary states), candidates, dense
    Q and R, a target trajectory."""
    rng = np.random.default_rng([seed, n, m, T, B])
    return dict(n=n, m=m, T=T, B=B, x=rng.normal(size=(T + 1, B, n)), u_cand=rng.normal(size=(B, T, m)),
                Q=dense_weight(rng, n), R=dense_weight(rng, m), xd=rng.normal(size=(T + 1, n)))


def stage_reference(c):
    """costs (B) = sum_t e' Q e + u' R u, the sum of the absolute values of the same products, and their number k:
    |got - want| <= 4 k u sum|terms| is the plain bound of a float64 summation of k products (each product of three
    factors carries two roundings, each of the fewer than k additions one, and e = x - xd is formed identically on both
    sides), with a factor 4 for the two roundings of a product and the freedom to contract."""
    T, n, m = c["T"], c["n"], c["m"]
    want, mag = np.zeros(c["B"]), np.zeros(c["B"])
    for t in range(T + 1):
        e = c["x"][t] - c["xd"][t]
        terms = e[:, :, None] * c["Q"][None] * e[:, None, :]
        want += terms.sum(axis=(1, 2))
        mag += np.abs(terms).sum(axis=(1, 2))
        if t < T:
            u = c["u_cand"][:, t]
            terms = u[:, :, None] * c["R"][None] * u[:, None, :]
            want += terms.sum(axis=(1, 2))
            mag += np.abs(terms).sum(axis=(1, 2))
    return want, mag, (T + 1) * n * n + T * m * m
