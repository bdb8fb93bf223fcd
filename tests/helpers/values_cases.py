"""Inputs and the f64 NumPy statement of the values pass (csrc/smooth_values.hip), shared by
tests/test_values_pass_cpu.py (which certifies the inputs) and tests/test_values_pass_gpu.py (which runs the kernel).

Inputs: Gaussian dx, du (unit std); fz = f0 + z W + 1e-3 noise with one fixed random linear map W per case, all rounded
to f32 -- so the design Z = [dx du] has cond(Z) of about 3 once N >= 4 d and the reference's own conditioning is harmless.

Statement: Z and dF = fz - f0 (the subtraction IN f32, as the kernel forms it) widened to f64, lstsq per timestep,
c_t = fnom_t - A_t x_t - B_t u_t.
"""
import numpy as np

# the sizes of the accuracy cases: a full tile (d = 16), d and n crossing a tile, the smallest, the largest
SIZES = [(2, 1), (5, 2), (12, 4), (13, 4), (17, 1), (32, 16)]
HORIZONS = [1, 3]


def sample_counts(n, m):
    """4d, 4d + 1; 255 / 256 / 257 (one workgroup, exactly one, two); 1000: four workgroups per timestep at T <= 3, the
    last one ragged (232 samples: three full waves and a 40-sample block).  N >= 4 d throughout."""
    d = n + m
    return sorted({4 * d, 4 * d + 1, 255, 256, 257, 1000})


def make_case(n, m, T, N, seed=0):
    rng = np.random.default_rng([seed, n, m, T, N])
    d = n + m
    dx = rng.normal(size=(T, N, n)).astype(np.float32)
    du = rng.normal(size=(T, N, m)).astype(np.float32)
    W = rng.normal(size=(d, n)) / np.sqrt(d)
    f0 = rng.normal(size=(T, n)).astype(np.float32)
    z = np.concatenate([dx, du], axis=2).astype(np.float64)
    fz = (f0[:, None, :].astype(np.float64) + z @ W + 1e-3 * rng.normal(size=(T, N, n))).astype(np.float32)
    return dict(n=n, m=m, T=T, N=N, dx=dx, du=du, fz=fz, f0=f0,
                x_trj=rng.normal(size=(T + 1, n)), u_trj=rng.normal(size=(T, m)), fnom=rng.normal(size=(T, n)))


def design(c):
    """Z (T,N,d) and dF (T,N,n) in f64; dF from the f32 subtraction."""
    Z = np.concatenate([c["dx"], c["du"]], axis=2).astype(np.float64)
    dF = (c["fz"] - c["f0"][:, None, :]).astype(np.float64)
    return Z, dF


def affine_from(AB, c):
    n = c["n"]
    At, Bt = AB[:, :, :n], AB[:, :, n:]
    ct = c["fnom"] - np.einsum("tij,tj->ti", At, c["x_trj"][:c["T"]]) - np.einsum("tij,tj->ti", Bt, c["u_trj"])
    return At, Bt, ct


def reference(c):
    """(At, Bt, ct) of the f64 statement: SVD lstsq per timestep."""
    Z, dF = design(c)
    AB = np.stack([np.linalg.lstsq(Z[t], dF[t], rcond=None)[0].T for t in range(c["T"])])
    return affine_from(AB, c)


def sums_reference(c):
    """sums (T,P) in f64 and, entry by entry, the sum of the absolute values of its terms (what a rounding bound scales
    with): upper Gram of z row-major, then z dF'."""
    Z, dF = design(c)
    d = c["n"] + c["m"]
    iu = np.triu_indices(d)
    G = np.einsum("tsi,tsj->tij", Z, Z)[:, iu[0], iu[1]]
    H = np.einsum("tsi,tsk->tik", Z, dF).reshape(c["T"], -1)
    Ga = np.einsum("tsi,tsj->tij", np.abs(Z), np.abs(Z))[:, iu[0], iu[1]]
    Ha = np.einsum("tsi,tsk->tik", np.abs(Z), np.abs(dF)).reshape(c["T"], -1)
    return np.concatenate([G, H], axis=1), np.concatenate([Ga, Ha], axis=1)


def f32_gram_f64_solve(c):
    """The kernel's arithmetic restated in NumPy: products and sums of the statistics in f32, the normal equations
    solved in f64."""
    Z, dF = design(c)
    Z32, dF32 = Z.astype(np.float32), dF.astype(np.float32)
    G = np.einsum("tsi,tsj->tij", Z32, Z32).astype(np.float64)
    H = np.einsum("tsi,tsk->tik", Z32, dF32).astype(np.float64)
    AB = np.stack([np.linalg.solve(G[t], H[t]).T for t in range(c["T"])])
    return affine_from(AB, c)
