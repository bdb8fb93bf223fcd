"""Host admission of the device building blocks against the extended-precision reference of
tests/helpers/functor_reference.py: irs_sincos (f32, f64), the Dual arithmetic, the four analytic model functors, the
quadrotor's hand-derived step_jac / expand_jac / expand_entry (csrc/dual.hpp, csrc/models.hpp are __host__ __device__)
and a numpy f32 emulation of the Philox + Box-Muller draw (csrc/philox.hpp).

tests/helpers/functor_probe.hip is compiled once with hipcc and run on the state tables; every output is held to the
bound eps K (|g| + sum |dg/dv| |v|) + (sincos term) of the helper -- K counted from the source, everything else from
mpmath.  The host build does not use the device objects' flags: this is the check that reference and bounds are sane
before tests/test_functors_gpu.py sends the same tables through the compiled library.

Largest error / bound per model and regime, host build (hipcc -O2), as test_model_functors_within_bounds prints them
(pytest -s).  Columns: step<float>, step<double>, Dual<float> Jacobian, Dual<double> Jacobian and, for the quadrotor,
step_jac<float> + expand_jac, step_jac<double> + expand_jac.  No regime needs more than the counted K.
    pendulum    theta_1e-2     0.126 0.086 0.198 0.135
    pendulum    theta_1e-1     0.091 0.069 0.198 0.125
    pendulum    theta_1e0      0.073 0.068 0.198 0.142
    pendulum    theta_1e1      0.047 0.063 0.198 0.130
    pendulum    theta_1e2      0.058 0.055 0.198 0.132
    pendulum    k_pi_2         0.071 0.067 0.198 0.166
    quadrotor   moderate       0.065 0.046 0.169 0.099 0.131 0.095
    quadrotor   pitch_0.3      0.058 0.033 0.091 0.080 0.103 0.060
    quadrotor   pitch_0.1      0.077 0.046 0.095 0.129 0.075 0.129
    quadrotor   pitch_1e-2     0.051 0.041 0.156 0.168 0.097 0.380
    quadrotor   roll_yaw_1e3   0.055 0.037 0.307 0.185 0.116 0.119
    quadrotor   rates_0_large  0.078 0.074 0.217 0.170 0.136 0.093
    quadrotor   zero_thrust    0.054 0.033 0.134 0.142 0.116 0.132
    bicycle     moderate       0.096 0.085 0.097 0.083
    bicycle     steer_0.1      0.073 0.069 0.086 0.063
    bicycle     steer_1e-2     0.082 0.079 0.072 0.059
    bicycle     speed_0_neg    0.110 0.070 0.081 0.092
    bicycle     heading_1e3    0.077 0.072 0.105 0.084
    three_cart  stuck_123      0.062 0.062 0.045 0.045
    three_cart  contact_12 / contact_23 / free    0 (every operation exact on the dyadic rows)
    three_cart  surface        0.030 0.045 0.045 0.045
irs_sincos: f32 at most 9.22e-8 absolute over 7484 points (bound 1.5e-7); f64 1.24 ulp over the sweep (bound 2) and
450.94 ulp of a result below 7e-13 at the f64 neighbours of k pi/2 (absolute error below 4e-28; bound 564 = 1.25 x).
The f32 emulation of the smoothing stream's draw: at most 0.68 of its tolerance at the committed extremes.
"""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from oracle import irs_oracle as orc
from tests.helpers import functor_reference as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
MODEL_NAMES = list(fr.MODELS)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """Runs the compiled probe: probe(kind, payload bytes) -> float64 array."""
    work = tmp_path_factory.mktemp("functor_probe")
    exe = str(work / "functor_probe")
    src = os.path.join(ROOT, "tests", "helpers", "functor_probe.hip")
    r = subprocess.run([HIPCC, "-O2", "-std=c++17", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "irs_mpc_amd", "csrc"),
                        "-o", exe, src], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(kind, payload):
        fin, fout = str(work / (kind + ".in")), str(work / (kind + ".out"))
        with open(fin, "wb") as f:
            f.write(payload)
        r = subprocess.run([exe, kind, fin, fout], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout, r.stderr)
        return np.fromfile(fout, np.float64)
    return run


def probe_model(probe, name, V):
    """dict of the probe's outputs for table rows V: each (k, ...)."""
    M = fr.MODELS[name]
    n, d = M["n"], M["n"] + M["m"]
    params = list(M["params"]) + [0.0] * (12 - len(M["params"]))
    payload = struct.pack("<i", V.shape[0]) + struct.pack("<12d", *params) + np.ascontiguousarray(V, np.float32).tobytes()
    fields = [("step32", n), ("step64", n), ("dual32_f", n), ("dual32_J", n * d), ("dual64_f", n), ("dual64_J", n * d)]
    if name == "quadrotor":
        fields += [("hand32_f", n), ("hand32_Jc", 33), ("hand32_J", n * d), ("hand32_Je", n * d), ("hand64_f", n),
                   ("hand64_J", n * d)]
    out = probe(name, payload).reshape(V.shape[0], sum(k for _, k in fields))
    res, at = {}, 0
    for key, k in fields:
        res[key] = out[:, at:at + k].reshape((V.shape[0], n, d) if k == n * d else (V.shape[0], k))
        at += k
    return res


_probed = {}


def probed(probe, name):
    """(regime tables, probe outputs, references) of a model, computed once."""
    if name not in _probed:
        T = fr.tables(name)
        n = fr.MODELS[name]["n"]
        _probed[name] = {tag: (V, probe_model(probe, name, V), fr.references(name, V[:, :n], V[:, n:])) for tag, V in T.items()}
    return _probed[name]


def ratio(refs, name, prec, what, got):
    err = np.stack([fr.error(r, g, what) for r, g in zip(refs, got)])
    bnd = np.stack([fr.bound(name, r, prec, what) for r in refs])
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bnd)
    return q


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("name", MODEL_NAMES)
def test_restatement_matches_the_f64_oracle(name):
    """At moderate states the mpmath restatement (run on floats, and in mpmath) equals the f64 oracle classes to 1e-13,
    step and Jacobian: neither is a copy of the other's arithmetic gone wrong unnoticed."""
    M = fr.MODELS[name]
    n = M["n"]
    so = getattr(orc, fr.SYSTEM_CLASSES[name][1])(M["params"][0])
    if name == "three_cart":
        so.d = M["params"][1]
    tag = {"pendulum": "theta_1e0", "quadrotor": "moderate", "bicycle": "moderate", "three_cart": "contact_12"}[name]
    V = fr.tables(name)[tag][:6].astype(np.float64)
    for row in V:
        x, u = row[:n], row[n:]
        ref = fr.reference(name, x, u)
        want_f, want_J = so.dynamics(x, u), so.jacobian_xu(x, u)
        scale_f, scale_J = 1.0 + np.abs(want_f), 1.0 + np.abs(want_J)
        assert (np.abs(fr.step_float(name, x, u) - want_f) <= 1e-13 * scale_f).all()
        assert (fr.error(ref, want_f, "f") <= 1e-13 * scale_f).all()
        # (the three-cart oracle differentiates by central differences of 1e-7: 1e-9)
        assert (fr.error(ref, want_J, "J") <= (1e-8 if name == "three_cart" else 1e-13) * scale_J).all()


@pytest.mark.parametrize("name", MODEL_NAMES)
def test_second_derivatives_skip_only_affine_inputs(name):
    """reference() forms second derivatives only in the inputs MODELS lists as `curved`; over ALL inputs the conditioning
    sums come out the same, i.e. the step is affine in the others."""
    n = fr.MODELS[name]["n"]
    V = next(iter(fr.tables(name).values()))[1].astype(np.float64)
    a, b = fr.reference(name, V[:n], V[n:]), fr.reference(name, V[:n], V[n:], all_inputs=True)
    np.testing.assert_allclose(a["cond_J"], b["cond_J"], rtol=1e-12, atol=1e-18)


def test_three_cart_surface_rows_sit_where_they_claim():
    """The surface table has gaps exactly d, one f32 step to either side of d, and d -+ 1/8 -- in exact arithmetic."""
    d = fr.MODELS["three_cart"]["params"][1]
    lo, hi = float(np.nextafter(np.float32(d), np.float32(0))), float(np.nextafter(np.float32(d), np.float32(1)))
    seen = set()
    for g12, g23 in fr.three_cart_gaps(fr.tables("three_cart")["surface"]):
        assert float(g12) in (lo, d, hi, d - 0.125, d + 0.125) and float(g23) in (lo, d, hi, d - 0.125, d + 0.125)
        seen.add((float(g12), float(g23)))
    assert len(seen) == 25


# --------------------------------------------------------------------------------------------------------- irs_sincos
def _sincos(probe):
    if "sincos" not in _probed:
        x32, x64, _ = fr.sincos_points()
        out = probe("sincos", struct.pack("<ii", x32.size, x64.size) + x32.tobytes() + x64.tobytes()).reshape(-1, 2)
        _probed["sincos"] = (x32, x64, out[:x32.size], out[x32.size:])
    return _probed["sincos"]


@needs_hipcc
def test_irs_sincos_f32_documented_bound(probe):
    """|error| <= 1.5e-7 absolute on |x| < 1e3 (csrc/dual.hpp): a sweep per decade from 1e-6, the f32 neighbours of
    k pi/2 and (k + 1/2) pi/2 up to the domain limit, +-0, denormals, the smallest normal."""
    x32, _, got, _ = _sincos(probe)
    hi, lo = fr.sincos_reference(x32)
    err = np.abs((got - hi) - lo)
    print("irs_sincos f32: %d points, max |error| %.3e at x = %r" % (x32.size, err.max(), x32[err.max(axis=1).argmax()]))
    assert np.isfinite(got).all()
    assert (err <= fr.SINCOS_ABS_F32).all()
    assert (got[x32 == 0] == [0.0, 1.0]).all()


@needs_hipcc
def test_irs_sincos_f64_documented_bound(probe):
    """|error| <= 2 ulp of the result on |x| < 1e6 over the sweep and the edge points.  At the f64 neighbours of k pi/2
    and (k + 1/2) pi/2 the smaller of the pair is held to 564 ulp of itself instead: measured 450.94 ulp (an absolute
    error of at most 3.9e-28 on a result below 7e-13), bound = 1.25 x measured; see functor_reference.py."""
    _, x64, _, got = _sincos(probe)
    near = fr.sincos_points()[2]
    hi, lo = fr.sincos_reference(x64)
    err = np.abs((got - hi) - lo)
    ulp = np.array([[np.spacing(abs(v)) for v in row] for row in hi])
    q = err / ulp
    i = q.max(axis=1).argmax()
    print("irs_sincos f64: %d points, max error %.3f ulp at x = %r" % (x64.size, q.max(), x64[i]))
    assert np.isfinite(got).all()
    print("    sweep and edges %.3f ulp, neighbours of k pi/4 %.3f ulp" % (q[~near].max(), q[near].max()))
    assert (q[~near] <= fr.SINCOS_ULP_F64).all()
    assert (q[near] <= fr.SINCOS_ULP_F64_NEIGHBOURS).all()
    assert (np.maximum(q[near, 0], q[near, 1])[np.abs(hi[near]).min(axis=1) > 1e-3] <= fr.SINCOS_ULP_F64).all()


# ------------------------------------------------------------------------------------------------- the model functors
@needs_hipcc
@pytest.mark.parametrize("name", MODEL_NAMES)
def test_model_functors_within_bounds(probe, name):
    """step<float>, step<double>, model_jacobian<., float> and <., double> (values and Jacobian) and, for the quadrotor,
    step_jac<float> / <double> expanded by expand_jac: every component within the bound, in every regime."""
    worst = {}
    for tag, (V, out, refs) in probed(probe, name).items():
        checks = [("step32", "f32", "f"), ("step64", "f64", "f"), ("dual32_f", "f32", "f"), ("dual64_f", "f64", "f"),
                  ("dual32_J", "f32", "J"), ("dual64_J", "f64", "J")]
        if name == "quadrotor":
            checks += [("hand32_J", "f32", "J"), ("hand64_J", "f64", "J"), ("hand64_f", "f64", "f")]
        row = {}
        for key, prec, what in checks:
            assert np.isfinite(out[key]).all(), (tag, key)
            row[key] = ratio(refs, name, prec, what, out[key])
        worst[tag] = {k: float(v.max()) for k, v in row.items()}
        print("%-10s %-14s " % (name, tag) + " ".join("%s %.3f" % (k, v) for k, v in worst[tag].items()))
    for tag, row in worst.items():
        for key, v in row.items():
            assert v <= 1.0, (name, tag, key, v)


@needs_hipcc
def test_step_jac_steps_equal_step_bit_for_bit(probe):
    """step_jac's step values == step's, f32 and f64, on every table row (the sample pass swaps one for the other)."""
    for tag, (V, out, _) in probed(probe, "quadrotor").items():
        np.testing.assert_array_equal(out["hand32_f"], out["step32"], err_msg=tag)
        np.testing.assert_array_equal(out["hand64_f"], out["step64"], err_msg=tag)
        np.testing.assert_array_equal(out["dual32_f"], out["step32"], err_msg=tag)


@needs_hipcc
def test_expand_entry_equals_expand_jac(probe):
    """expand_entry(q) == entry q of expand_jac for all 192 entries, on every table row (compared as values: -0 == 0)."""
    for tag, (V, out, _) in probed(probe, "quadrotor").items():
        np.testing.assert_array_equal(out["hand32_Je"], out["hand32_J"], err_msg=tag)


@needs_hipcc
def test_three_cart_takes_the_strict_branch_on_the_surfaces(probe):
    """On a switching surface and one f32 step to either side, f32 and f64 take the branch strict `<` gives: the
    Jacobian of the step is that of the reference's branch EXACTLY up to the rounding of 1/3 (the branches' Jacobians
    differ by at least 1/6 in some entry), and so are the velocities."""
    V, out, refs = probed(probe, "three_cart")["surface"]
    J = fr.stack(refs, "J_hi")
    branches = {tuple(np.round(j.ravel() * 6).astype(int)) for j in J}
    assert len(branches) == 4
    for key, tol in (("dual32_J", 2.0 ** -24), ("dual64_J", 2.0 ** -53)):
        assert (np.abs(out[key] - J) <= tol).all(), key


# ------------------------------------------------------------------------------------------------------------- RNG
def test_rng_extremes_file_is_what_the_scan_finds():
    """tests/golden/rng_extremes.json against a re-scan of the first 2^20 indices: the file lists exactly those of them
    that beat its own thresholds, and every listed index has the word it is listed for."""
    g = fr.rng_extremes()
    assert (g["seed"], g["it"], g["scanned"]) == (fr.RNG_SEED, fr.RNG_IT, fr.RNG_SCAN)
    part = 1 << 20
    w = fr.philox_words(np.arange(part, dtype=np.uint64))
    small, large = fr.philox_words(g["u1_smallest"])[:, 0], fr.philox_words(g["u1_largest"])[:, 0]
    assert len(set(g["u1_smallest"])) == 16 and len(set(g["u1_largest"])) == 16
    assert small.max() < 16 * 1024 and large.min() > 2 ** 32 - 16 * 1024      # ~16 of 2^24 draws below 2^8 k: plausible
    assert set(np.nonzero(w[:, 0] <= small.max())[0]) == {i for i in g["u1_smallest"] if i < part}
    assert set(np.nonzero(w[:, 0] >= large.min())[0]) == {i for i in g["u1_largest"] if i < part}
    u2 = (w[:, 1].astype(np.float64) + 0.5) / 4294967296.0
    for k, den in fr.RNG_U2_TARGETS:
        idx = g["u2_near_%d_%d" % (k, den)]
        dist = np.abs((fr.philox_words(idx)[:, 1].astype(np.float64) + 0.5) / 4294967296.0 - k / den)
        assert len(set(idx)) == 16 and dist.max() < 1e-5
        assert set(np.nonzero(np.abs(u2 - k / den) < dist.max())[0]) <= set(idx)


def test_f32_draw_stays_inside_the_documented_deviation():
    """A numpy f32 emulation of the smoothing stream's draw at every committed index: within rtol 2e-5 / atol 2e-6 plus
    the radius deviation min(rad, 2^-25 / rad (1 + 2^-20)) of the mpmath Box-Muller -- and NOT within the plain
    tolerance at the largest u1 words, which is the tail the deviation term is there for."""
    g = fr.rng_extremes()
    idx = fr.rng_extreme_indices(g)
    w = fr.philox_words(idx)
    z, rad = fr.box_muller(w)
    ze = fr.box_muller_f32(w).astype(np.float64)
    err = np.abs(ze - z)
    print("f32 emulation: max |err| / tol = %.3f" % (err / fr.rng_tolerance(z, rad, False)).max())
    assert (err <= fr.rng_tolerance(z, rad, False)).all()
    tail = [idx.index(i) for i in g["u1_largest"]]
    assert (err[tail] > fr.rng_tolerance(z[tail], rad[tail], True)).any()
    # the mpmath draw equals the f64 specification
    _, zo = orc.device_gaussian_samples(1, 1, 0, 4, np.zeros(0), np.ones(4), fr.RNG_SEED, fr.RNG_IT, sample_offset=idx[0])
    np.testing.assert_allclose(zo[0, 0], z[0], rtol=1e-12, atol=1e-15)
