// Uniform-geometry sample pass: the u-only smoothing modes of the exact 8-row contact models
//   irs_lqr/quasistatic_dynamics.py:242-266  calc_B_zero_order    (ZERO_ORDER_B)
//   irs_lqr/quasistatic_dynamics.py:193-208  calc_AB_first_order  (FIRST_ORDER, u-only noise)
// -- the metric's workload (planar_hand, gradient modes "zero_order_B" / "first_order").
//
// In these modes the STATE of a timestep is not perturbed, only the command.  The step QP of sample s,
//     min_dq 1/2 dq'D dq + b(u_s)'dq   s.t.  phi + J dq >= 0,
// then has the SAME geometry (D, J, phi) for every sample of the timestep; only the actuated entries of b move,
// linearly in du.  Its dual  min_{lam >= 0} 1/2 lam'W lam + r'lam  has ONE Hessian W = J D^-1 J' per timestep and
// r = r0 + C du.  The general kernel (smooth.hip) carries J, W and a masked LDL' of W_AA in the registers of every
// lane (388 registers: one wave per SIMD) and re-factorises per sample.  Here
//   * everything uniform lives in LDS (C, J D^-1, the table) or in ONE set of registers per lane (W, r0: 52);
//   * the workgroup tabulates, once, for ALL 2^8 candidate active sets A the map  r -> [lam_A ; slacks off A]
//     (G_A: rows of -W_AA^-1 on A -- row order, with the pivot rule of irs_contact_qp_dual_exact: a dependent row
//     drops out -- and of I + W M off A; built by principal pivot steps from the empty set, one rank-1 update of an
//     8 x 13 tableau per row of A, eight lanes per tableau: ug_build_table), not as G_A itself but as what
//     the sample loop applies it to: G_A r = h_A + H_A du in the QP's four parameters (h_A = G_A r0, H_A = G_A C':
//     8 + 32 floats) and, for the dual steps, U_A = G_A W (64 floats): 256 x 116 floats in LDS;
//   * a sample is solved by a few projected sweeps (a guess of A), then primal-dual active-set iterations that
//     cost ONE affine table row (12 reads, 40 FMA) each: A <- (A minus the ONE row with the most negative lam_i) +
//     every row with slack < 0 (ug_pdas: releasing all rows with lam_i <= 0 at once cycles on this W), until the KKT
//     conditions hold -- the exact optimum of the QP, certified per sample;
//   * samples that do not settle within the iteration cap (a tenth of the benchmark's) are parked in the wave's LDS ring
//     (as in smooth.hip) and finished 64 at a time: first more of the same iterations from the parked set, which
//     settle all but a few in 10^5, then, for what is left, the Goldfarb-Idnani dual active-set method (finite, no
//     cycling), whose step reads its direction as one column of U_A (first-order pass: one row of W and a product
//     with G_A);
//   * zero-order statistics: sum z z', sum z lam', sum z -- the primal step is a UNIFORM linear map of lam, so
//     it is applied once per workgroup to the sums (sum z df' = (sum z lam') (J D^-1) - ...), not per sample;
//   * first-order statistics: the derivative of the step through its active set depends on the active set
//     ALONE (geometry fixed), so the sample pass only counts active sets (integer LDS atomics: order-free,
//     deterministic) and B(I) is evaluated once per occupied set from the same table (whose X block is then G_A).
// Per-lane state: r, lam, a mask and the accumulators -- the kernel fits two (or more) waves per SIMD.
// The f64 nominal step f(x_t, u_t) is evaluated by the last wave of workgroup 0 of every timestep, cooperatively
// (lane c owns contact row c; an 8x8 masked LDL' spread over the 64 lanes), from the f32 pipeline's active set,
// re-checked against the KKT conditions in f64.
#include "smooth_common.hpp"
#include "ug_geometry.hpp"

namespace {

#ifndef IRS_UG_SWEEPS
#define IRS_UG_SWEEPS 6
#endif
#ifndef IRS_UG_FLIP_ALL
#define IRS_UG_FLIP_ALL 0
#endif
constexpr bool kUgFlipAll = IRS_UG_FLIP_ALL != 0;           // the iteration flips every non-optimal row at once (the rule the single release replaced, with its caps 4 / 0; same-day timing)
#ifndef IRS_UG_PDAS
#define IRS_UG_PDAS (IRS_UG_FLIP_ALL ? 4 : 3)
#endif
#ifndef IRS_UG_PDAS_FLUSH
#define IRS_UG_PDAS_FLUSH (IRS_UG_FLIP_ALL ? 0 : 8)
#endif
#ifndef IRS_UG_BLOCK
#define IRS_UG_BLOCK 512
#endif
constexpr int kUgBlock = IRS_UG_BLOCK;
constexpr int kUgSweeps = IRS_UG_SWEEPS;      // projected sweeps that guess the active set
constexpr int kUgPdas = IRS_UG_PDAS;          // primal-dual active-set iterations of the first attempt
constexpr int kUgPdasFlush = IRS_UG_PDAS_FLUSH;   // further iterations a parked sample gets in the flush, before the dual steps
#ifndef IRS_UG_STEP_COLUMNS
#define IRS_UG_STEP_COLUMNS 1
#endif
constexpr bool kUgStepColumns = IRS_UG_STEP_COLUMNS != 0;   // zero-order pass: dual steps read a column of G W (0: G and a product)
#ifndef IRS_UG_TABLE_LDL
#define IRS_UG_TABLE_LDL 0
#endif
constexpr bool kUgTableLdl = IRS_UG_TABLE_LDL != 0;         // the table by one masked LDL' per entry (the build the pivot steps replaced; reference and timing)
// One table entry, in floats (every piece 16-byte aligned, 464 B per entry):
//   [ h = G r0 (8) | H = G C' (4 columns of 8, one per command) | tau (8: 1 off the reduced set, 0 on it) |
//     the reduced set + pad (4) | X (8 x 8, column-major) ]
// X = G W for the zero-order pass (a dual step reads its direction u = G W[:,p] as column p), X = G for the first-order
// pass (its epilogue reads M on the set from it).
constexpr int kUgTabH = 8, kUgTabTau = 40, kUgTabSet = 48, kUgTabX = 52;
constexpr int kUgTabStride = 116;
#ifndef IRS_UG_NOM_ROUNDS
#define IRS_UG_NOM_ROUNDS 2
#endif
constexpr int kUgNomRounds = IRS_UG_NOM_ROUNDS;   // sample rounds the nominal wave sits out (its f64 step takes about that long)
constexpr int kUgRing = 128;                  // parked samples per wave: < 64 waiting + <= 64 new ones

template <class Model>
struct alignas(16) UgLds {
    static constexpr int NC = Model::NC, n = Model::NX, m = Model::NU;
    float tab[1 << NC][kUgTabStride];     // first: every ds_read_b128 of the sample loop is 16-byte aligned
    float W[NC][NC];          // dual Hessian J D^-1 J'
    float invw[NC];           // omega / W_ii
    float Wd[NC];             // W_ii
    float r0[NC];             // phi - J D^-1 b(u_t)
    float phi[NC];
    float C[m][NC];           // r = r0 + sum_j C[j][:] du_j
    float JD[n][NC];          // JD[k][c] = J[c][k] D^-1_k   (primal recovery: dq_k = sum_c JD[k][c] lam_c - Db_k)
    float Jc[NC][n];          // J
    float Dinv[n];
    float Db0[n];             // D^-1 b(u_t)
    float DK[m];              // D^-1_act(j) K_j  (= 1 up to rounding)
    float q[n];
};

__device__ __forceinline__ float ug_uniform(float v) {
    return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

// the uniform operands the sample loop keeps in registers
template <int NC>
struct UgUni {
    float W[NC * (NC + 1) / 2];
    float invw[NC];
    float r0[NC];
    __device__ __forceinline__ float w(int i, int j) const {
        return i <= j ? W[i * NC - i * (i - 1) / 2 + (j - i)] : W[j * NC - j * (j - 1) / 2 + (i - j)];
    }
};

// v = G_a r + tol tau_a for r = r0 + C du, read as h_a + H_a du (table entry a; tau_i = 1 for a row off the reduced
// set -- whose v_i is a slack, optimal when >= -tol -- and 0 on it -- v_i a multiplier, optimal when > 0: with the
// tolerance folded in, "row i is optimal" is v_i > 0 for both kinds).  The step QP has four parameters, so the row is
// 8 + 4 x 8 numbers, not 8 x 8.  All 12 reads are issued before the first use: a wave has one partner on its SIMD to
// hide the LDS latency behind.  Returns the reduced set.
template <class Model>
__device__ __forceinline__ unsigned ug_lookup_affine(const UgLds<Model>& S, unsigned a, const float* du, float tol,
                                                     float* v, float* tau) {
    constexpr int NC = Model::NC, m = Model::NU;
    static_assert(NC == 8 && m == 4, "table entries are 8 rows by 4 commands");
    const float4* e = reinterpret_cast<const float4*>(&S.tab[a][0]);
    float4 g4[kUgTabSet / 4];
#pragma unroll
    for (int c = 0; c < kUgTabSet / 4; ++c) g4[c] = e[c];
    const unsigned ap = __float_as_uint(S.tab[a][kUgTabSet]);
    tau[0] = g4[kUgTabTau / 4].x; tau[1] = g4[kUgTabTau / 4].y; tau[2] = g4[kUgTabTau / 4].z; tau[3] = g4[kUgTabTau / 4].w;
    tau[4] = g4[kUgTabTau / 4 + 1].x; tau[5] = g4[kUgTabTau / 4 + 1].y; tau[6] = g4[kUgTabTau / 4 + 1].z; tau[7] = g4[kUgTabTau / 4 + 1].w;
    v[0] = fmaf(tau[0], tol, g4[0].x); v[1] = fmaf(tau[1], tol, g4[0].y);
    v[2] = fmaf(tau[2], tol, g4[0].z); v[3] = fmaf(tau[3], tol, g4[0].w);
    v[4] = fmaf(tau[4], tol, g4[1].x); v[5] = fmaf(tau[5], tol, g4[1].y);
    v[6] = fmaf(tau[6], tol, g4[1].z); v[7] = fmaf(tau[7], tol, g4[1].w);
#pragma unroll
    for (int j = 0; j < m; ++j) {
        const float4 lo = g4[kUgTabH / 4 + 2 * j], hi = g4[kUgTabH / 4 + 2 * j + 1];
        v[0] = fmaf(lo.x, du[j], v[0]); v[1] = fmaf(lo.y, du[j], v[1]);
        v[2] = fmaf(lo.z, du[j], v[2]); v[3] = fmaf(lo.w, du[j], v[3]);
        v[4] = fmaf(hi.x, du[j], v[4]); v[5] = fmaf(hi.y, du[j], v[5]);
        v[6] = fmaf(hi.z, du[j], v[6]); v[7] = fmaf(hi.w, du[j], v[7]);
    }
    return ap;
}

// The direction of a dual step towards row p (off the set a): u = G_a W[:,p], with tau_a.  UCOL (the zero-order pass):
// column p of the entry's X = G_a W, 4 reads and no arithmetic; else (X = G_a): the row W[p][:] and the 8 x 8 product.
template <class Model, bool UCOL>
__device__ __forceinline__ void ug_step_direction(const UgLds<Model>& S, unsigned a, int p, float* u, float* tau) {
    constexpr int NC = Model::NC;
    const float* e = &S.tab[a][0];
    const float4 t0 = *reinterpret_cast<const float4*>(e + kUgTabTau), t1 = *reinterpret_cast<const float4*>(e + kUgTabTau + 4);
    if constexpr (UCOL) {
        const float4 lo = *reinterpret_cast<const float4*>(e + kUgTabX + NC * p);
        const float4 hi = *reinterpret_cast<const float4*>(e + kUgTabX + NC * p + 4);
        u[0] = lo.x; u[1] = lo.y; u[2] = lo.z; u[3] = lo.w;
        u[4] = hi.x; u[5] = hi.y; u[6] = hi.z; u[7] = hi.w;
    } else {
        const float4 wlo = *reinterpret_cast<const float4*>(&S.W[p][0]);
        const float4 whi = *reinterpret_cast<const float4*>(&S.W[p][4]);
        const float4* x4 = reinterpret_cast<const float4*>(e + kUgTabX);
        float4 g4[2 * NC];
#pragma unroll
        for (int c = 0; c < 2 * NC; ++c) g4[c] = x4[c];
        const float wp[NC] = {wlo.x, wlo.y, wlo.z, wlo.w, whi.x, whi.y, whi.z, whi.w};
#pragma unroll
        for (int i = 0; i < NC; ++i) u[i] = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const float4 lo = g4[2 * c], hi = g4[2 * c + 1];
            u[0] = fmaf(lo.x, wp[c], u[0]); u[1] = fmaf(lo.y, wp[c], u[1]);
            u[2] = fmaf(lo.z, wp[c], u[2]); u[3] = fmaf(lo.w, wp[c], u[3]);
            u[4] = fmaf(hi.x, wp[c], u[4]); u[5] = fmaf(hi.y, wp[c], u[5]);
            u[6] = fmaf(hi.z, wp[c], u[6]); u[7] = fmaf(hi.w, wp[c], u[7]);
        }
    }
    tau[0] = t0.x; tau[1] = t0.y; tau[2] = t0.z; tau[3] = t0.w;
    tau[4] = t1.x; tau[5] = t1.y; tau[6] = t1.z; tau[7] = t1.w;
}

// r = r0 + C du and the tolerance of the optimality tests (that of irs_contact_qp_dual_exact)
template <class Model>
__device__ __forceinline__ float ug_rhs(const UgUni<Model::NC>& U, const UgLds<Model>& S, const float* du, float* r) {
    constexpr int NC = Model::NC, m = Model::NU;
#pragma unroll
    for (int c = 0; c < NC; ++c) r[c] = U.r0[c];
#pragma unroll
    for (int j = 0; j < m; ++j) {
        const float4 lo = *reinterpret_cast<const float4*>(&S.C[j][0]);
        const float4 hi = *reinterpret_cast<const float4*>(&S.C[j][4]);
        r[0] = fmaf(lo.x, du[j], r[0]); r[1] = fmaf(lo.y, du[j], r[1]);
        r[2] = fmaf(lo.z, du[j], r[2]); r[3] = fmaf(lo.w, du[j], r[3]);
        r[4] = fmaf(hi.x, du[j], r[4]); r[5] = fmaf(hi.y, du[j], r[5]);
        r[6] = fmaf(hi.z, du[j], r[6]); r[7] = fmaf(hi.w, du[j], r[7]);
    }
    float scale = 1e-30f;
#pragma unroll
    for (int c = 0; c < NC; ++c) scale = fmaxf(scale, fabsf(r[c]));
    return 1e-6f * scale;
}

// Up to CAP primal-dual active-set iterations from the set `a`, one affine table row each.  With v the row at the
// reduced set ap and `bad` the rows that are not optimal (the sign bits of v):
//   every row off ap whose slack is below -tol joins (viol = bad & ~ap);
//   of the rows on ap whose multiplier is not positive (neg = bad & ap) exactly ONE leaves, the most negative one:
//       a <- (ap & ~worst) | viol.
// Flipping every bad row at once (-DIRS_UG_FLIP_ALL=1: a <- ap ^ bad, the rule this one replaced) cycles on this W,
// which is no M-matrix: 13 % of the benchmark's samples are unsettled after 4 iterations and still 6 % after 11;
// releasing one row at a time leaves 3 % after 4, 0.4 % after 6 and 0.03 % after 11.
// The worst row is the maximum of one unsigned key per row: the bit pattern of v_i (a row off ap pushed to +3e38, so
// its sign bit is clear) with the low three mantissa bits replaced by 7 - i.  Among keys with the sign bit set the
// largest is the most negative multiplier; multipliers that agree in all but those three bits tie, and the tie goes to
// the LOWEST row index (tests/helpers/ug_release_twin.py packs the same key).
// A lane that is `done` keeps lam and a.  A lane that settles takes lam = v on the set, 0 off it; else `a` is the set to
// try next (a warm start for more iterations or for ug_full).
template <class Model, int CAP>
__device__ __forceinline__ void ug_pdas(const UgLds<Model>& S, const float* du, float tolv, unsigned& a, float* lam, bool& done) {
    constexpr int NC = Model::NC;
    static_assert(NC == 8, "the release key packs a row index into three mantissa bits");
    for (int it = 0; it < CAP; ++it) {
        float v[NC], tau[NC];
        const unsigned ap = ug_lookup_affine<Model>(S, a, du, tolv, v, tau);
        // the sign bits, shifted in one v_alignbit each: row 0 ends in bit 0.  A multiplier of exactly +0 stays: it
        // satisfies the KKT conditions as it is
        unsigned bad = 0u;
#pragma unroll
        for (int i = NC - 1; i >= 0; --i) bad = __builtin_amdgcn_alignbit(bad, __float_as_uint(v[i]), 31);
        unsigned next;
        if constexpr (kUgFlipAll) {
            next = ap ^ bad;
        } else {
            unsigned key = 0u;
#pragma unroll
            for (int i = 0; i < NC; ++i)
                key = max(key, (__float_as_uint(fmaf(tau[i], 3.0e38f, v[i])) & ~7u) | (unsigned)(7 - i));
            const unsigned worst = (bad & ap) != 0u ? (0x80u >> (key & 7u)) : 0u;
            next = (ap & ~worst) | (bad & ~ap);
        }
        if (!done) {
            if (bad == 0u) {
#pragma unroll
                for (int i = 0; i < NC; ++i) lam[i] = fmaf(-tau[i], v[i], v[i]);      // v on the set, 0 off it
                done = true;
            }
            a = next;
        }
        if (__all(done)) break;
    }
}

// FIRST ATTEMPT: sweeps guess the active set, primal-dual active-set iterations settle it.  true: lam is the exact
// optimum (KKT certified); false: `a` is the set the iteration stopped on (a warm start for ug_full).
template <class Model>
__device__ __forceinline__ bool ug_try(const UgUni<Model::NC>& U, const UgLds<Model>& S, const float* r, const float* du,
                                       float tolv, float* lam, unsigned& a_out, int diag = 0) {
    constexpr int NC = Model::NC;
    float g[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) { lam[i] = 0.f; g[i] = r[i]; }
#pragma unroll 2
    for (int sw = 0; sw < ((diag & 64) ? 0 : kUgSweeps); ++sw) {
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            const float nw = fmaxf(fmaf(-g[i], U.invw[i], lam[i]), 0.f);
            const float dl = nw - lam[i];
            lam[i] = nw;
#pragma unroll
            for (int j = 0; j < NC; ++j) g[j] = fmaf(U.w(j, i), dl, g[j]);
        }
    }
    unsigned a = 0u;
#pragma unroll
    for (int i = 0; i < NC; ++i) a |= (lam[i] > 0.f) ? (1u << i) : 0u;
    bool done = (diag & 32) != 0;
    ug_pdas<Model, kUgPdas>(S, du, tolv, a, lam, done);
    a_out = a;
    return done;
}

// FULL METHOD from a warm set: the Goldfarb-Idnani dual active-set method in the dual variables, restated from
// irs_contact_qp_dual_exact (contact_models.hpp) with every factorisation replaced by a table row:
//   repair rounds: lam_A = -W_AA^-1 r_A; rows with lam_i <= 0 leave (<= 3 rounds; else start from lam = 0);
//   loop: p = most violated row off A; u = G_A W[:,p] (ug_step_direction) gives rho = -u on A and the slack rates
//   s = u off A; step to the first of { slack_p = 0 (p joins), some lam_i = 0 (i leaves) }.  Finite, no cycling.
// r (= r0 + C du) serves the cold start only; the repair rounds read the affine rows at du.
template <class Model, bool UCOL>
__device__ __forceinline__ void ug_full(const UgLds<Model>& S, const float* r, const float* du, float tolv, unsigned a,
                                        float* lam, int cap = 4 * Model::NC) {
    constexpr int NC = Model::NC;
    constexpr float kBig = 3.0e38f, piv_rel = 1e-5f;
    float g[NC];
    bool valid = false;
    for (int round = 0; round < 3; ++round) {
        if (__all(valid)) break;
        float v[NC], tau[NC];
        const unsigned ap = ug_lookup_affine<Model>(S, a, du, 0.f, v, tau);
        if (!valid) {
            unsigned negb = 0u;
#pragma unroll
            for (int i = 0; i < NC; ++i) {
                const bool in = tau[i] == 0.f;
                negb |= (in && !(v[i] > 0.f)) ? (1u << i) : 0u;
                lam[i] = in ? v[i] : 0.f;
                g[i] = in ? 0.f : v[i];
            }
            valid = negb == 0u;
            a = ap & ~negb;
        }
    }
    if (!valid) {
        a = 0u;
#pragma unroll
        for (int i = 0; i < NC; ++i) { lam[i] = 0.f; g[i] = r[i]; }
    }
    int p = -1;
    bool done = false;
    for (int it = 0; it < cap; ++it) {
        if (!done && p < 0) {
            float vmin = kBig;
            int c = 0;
#pragma unroll
            for (int i = 0; i < NC; ++i) {
                const float vv = ((a >> i) & 1u) ? kBig : g[i];
                if (vv < vmin) { vmin = vv; c = i; }
            }
            if (vmin >= -tolv) done = true;
            else p = c;
        }
        if (__all(done)) break;
        const int pp = (done || p < 0) ? 0 : p;
        float u[NC], tau[NC];
        ug_step_direction<Model, UCOL>(S, a, pp, u, tau);
        // in arithmetic rather than selects (tau_i = 1 off the reduced set, 0 on it): rho = -(1 - tau) u on the set,
        // the slack rates s = tau u off it -- a third of the instructions of the select form (400 -> ~270 per step)
        const float wpp = S.Wd[pp];
        float gp = 0.f, zp = 0.f;
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            const bool isp = i == pp;
            gp = isp ? g[i] : gp;
            zp = isp ? u[i] : zp;
        }
        const bool full_ok = zp > piv_rel * wpp;
        const float t2 = full_ok ? -gp * irs_rcp_fast(zp) : kBig;
        float rho[NC], qv[NC];
        float t1 = kBig;
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            rho[i] = fmaf(tau[i], u[i], -u[i]);
            qv[i] = rho[i] > 0.f ? lam[i] * irs_rcp_fast(rho[i]) : kBig;
            t1 = fminf(t1, qv[i]);
        }
        int kb = 0;                                        // the FIRST row that attains the minimum
#pragma unroll
        for (int i = NC - 1; i >= 0; --i) kb = (qv[i] == t1) ? i : kb;
        const float tmin = fminf(t1, t2);
        if (!done && !(tmin < kBig)) done = true;          // no step possible: infeasible primal, keep lam
        const float tt = done ? 0.f : tmin;
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            g[i] = fmaf(tt * tau[i], u[i], g[i]);
            lam[i] = fmaxf(fmaf(-tt, rho[i], lam[i]) + ((i == pp) ? tt : 0.f), 0.f);
        }
        if (!done) {
            const bool full = t2 <= t1;
            if (full) {
                a |= 1u << pp;
                p = -1;
            } else {
                a &= ~(1u << kb);
#pragma unroll
                for (int i = 0; i < NC; ++i) lam[i] = (i == kb) ? 0.f : lam[i];
            }
        }
    }
}

// -DIRS_UG_TABLE_LDL=1 (the build the pivot steps replaced; the reference of tests/test_smooth_ug_table_gpu.py and of
// same-day timings): one table entry for the candidate set `a`, by the masked LDL' in row order of irs_contact_qp_dual_exact_try (pivot
// rule included: a dependent row leaves the set).  G_a is never formed: it is APPLIED (a solve on the set with the
// right-hand side -x_A; x_i + sum_j W_ij y_j on the rows off it) to the 13 vectors the sample loop needs it on --
// r0 (h), the four C[j][:] (H) and the eight W[:,p] (X = G W; UCOL) or unit vectors (X = G).  `half` (0/1): this lane's
// share, 7 and 6 of them.
template <class Model, bool UCOL>
__device__ __forceinline__ void ug_build_entry(UgLds<Model>& S, unsigned a, int half) {
    constexpr int NC = Model::NC;
    constexpr float piv_rel = 1e-5f;
    float M_[NC][NC], inv[NC], W[NC][NC];
    bool act[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        act[i] = ((a >> i) & 1u) != 0u;
#pragma unroll
        for (int j = 0; j < NC; ++j) W[i][j] = S.W[i][j];
#pragma unroll
        for (int j = 0; j <= i; ++j) M_[i][j] = W[i][j];
    }
    unsigned ap = 0u;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const float dj = M_[j][j];
        const bool ok = act[j] && dj > piv_rel * W[j][j];
        act[j] = ok;
        ap |= ok ? (1u << j) : 0u;
        inv[j] = ok ? irs_rcp_fast(dj) : 0.f;
#pragma unroll
        for (int i = j + 1; i < NC; ++i) M_[j][i] = M_[i][j] * inv[j];
#pragma unroll
        for (int i = j + 1; i < NC; ++i)
#pragma unroll
            for (int k = j + 1; k <= i; ++k) M_[i][k] = M_[i][k] - M_[j][i] * M_[k][j];
    }
    float* e = &S.tab[a][0];
    constexpr int NAPP = 1 + Model::NU + NC, SHARE = (NAPP + 1) / 2;
    for (int qq = 0; qq < SHARE; ++qq) {
        const int q = half * SHARE + qq;
        if (q >= NAPP) break;
        const int c = q - (1 + Model::NU);                 // the column of X, if any
        float x[NC];
        if (UCOL || c < 0) {
            const float* src = q == 0 ? &S.r0[0] : (c < 0 ? &S.C[q - 1][0] : &S.W[c][0]);     // W is symmetric to the bit
            const float4 lo = *reinterpret_cast<const float4*>(src), hi = *reinterpret_cast<const float4*>(src + 4);
            x[0] = lo.x; x[1] = lo.y; x[2] = lo.z; x[3] = lo.w;
            x[4] = hi.x; x[5] = hi.y; x[6] = hi.z; x[7] = hi.w;
        } else {
#pragma unroll
            for (int i = 0; i < NC; ++i) x[i] = (i == c) ? 1.f : 0.f;
        }
        // y = -W_AA^-1 x_A on the set (zero off it)
        float y[NC];
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            float v = act[j] ? -x[j] : 0.f;
#pragma unroll
            for (int k = 0; k < j; ++k) v = v - M_[k][j] * y[k];
            y[j] = v;
        }
#pragma unroll
        for (int j = NC - 1; j >= 0; --j) {
            float v = y[j] * inv[j];
#pragma unroll
            for (int i = j + 1; i < NC; ++i) v = v - M_[j][i] * y[i];
            y[j] = v;
        }
        float col[NC];
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            float s = x[i];
#pragma unroll
            for (int j = 0; j < NC; ++j) s = fmaf(W[i][j], y[j], s);
            col[i] = act[i] ? y[i] : s;
        }
        float* dst = e + (c < 0 ? NC * q : kUgTabX + NC * c);
        *reinterpret_cast<float4*>(dst) = make_float4(col[0], col[1], col[2], col[3]);
        *reinterpret_cast<float4*>(dst + 4) = make_float4(col[4], col[5], col[6], col[7]);
    }
    if (half == 1) {
        *reinterpret_cast<float4*>(e + kUgTabTau) = make_float4(act[0] ? 0.f : 1.f, act[1] ? 0.f : 1.f, act[2] ? 0.f : 1.f, act[3] ? 0.f : 1.f);
        *reinterpret_cast<float4*>(e + kUgTabTau + 4) = make_float4(act[4] ? 0.f : 1.f, act[5] ? 0.f : 1.f, act[6] ? 0.f : 1.f, act[7] ? 0.f : 1.f);
        e[kUgTabSet] = __uint_as_float(ap);
    }
}

// ---- the table by pivot steps ---------------------------------------------------------------------------------
// Entry A is the tableau of the principal pivot transform of the dual on A: T_A = G_A [r0 | C' | W] (8 x 13), and
// T_0 = [r0 | C' | W] (G_0 = I).  Its last eight columns G_A W are the pivot columns: for a row p off A with
// d = (G_A W)[p][p] (the Schur complement of W_pp on A),
//     rho = -T[p,:] / d,   T[i,:] += (G_A W)[i][p] rho  (i != p),   T[p,:] = rho
// is T of A + {p}: one reciprocal and 8 x 13 FMAs instead of a factorisation and 13 applications.  Every set is reached
// from the empty one by pivoting its rows in increasing order -- the order of the masked LDL' above, whose pivot of row
// p IS d -- with that build's rule: a row with d <= 1e-5 W_pp is not pivoted (the entry is that of the set without it).
// The first-order pass stores G_A itself: eight more columns that start as the identity ride along.
//
// Eight lanes carry one tableau in registers, COLUMNS across the lanes (lane l: columns l, 8 + l [, 16 + l], eight
// rows each): a step needs the pivot column on every lane -- 8 broadcasts within the eight lanes, against 13 for the
// pivot row had the rows been dealt out -- and then only values of its own (rho_c = T[p][c] rinv; 7 FMAs; T[p][c] = rho_c
// with p a compile-time register index, no select by lane); and an entry is stored column by column, which is how it
// lies in LDS (two ds_write_b128 per column).
//   column:  0 h | 1..4 H | 5..12 G W | 13..15 unused | 16..23 G (first-order pass)
template <int NS>
struct UgTableau {
    float c[NS][8];    // this lane's columns 8 s + l
    unsigned set;      // the reduced set (the same on the eight lanes)
};

// lane P of every group of eight lanes (ds_swizzle, bit-mask mode: lane' = (lane & 0x18) | P within each 32)
template <int P>
__device__ __forceinline__ float ug_bcast8(float v) {
    return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x18 | (P << 5)));
}

// the pivot on row P where `want` (the same on the eight lanes of a tableau) and the pivot rule allow it
template <int P, int NS>
__device__ __forceinline__ void ug_pivot(UgTableau<NS>& R, bool want, float wpp) {
    constexpr float piv_rel = 1e-5f;
    constexpr int PS = (5 + P) >> 3, PL = (5 + P) & 7;     // where column P of G W lives
    float x[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = ug_bcast8<PL>(R.c[PS][i]);
    const float d = x[P];
    const bool ok = want && d > piv_rel * wpp;
    const float rinv = ok ? -irs_rcp_fast(d) : 0.f;        // not taken: rho = 0 and every row stays what it is
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const float rho = R.c[s][P] * rinv;
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (i != P) R.c[s][i] = fmaf(x[i], rho, R.c[s][i]);
        R.c[s][P] = ok ? rho : R.c[s][P];
    }
    R.set |= ok ? (1u << P) : 0u;
}

// lane l of the eight stores its columns of entry `a`.  Three of the eight have no second column (zero-order pass) or
// no h / H column (first-order pass): they store tau (lanes 5, 6) and the set with its pad (lane 7) in the same
// ds_write_b128 as the others' half columns, so an entry is four stores.  (Columns four apart share their banks, a
// 2-way conflict; letting some lanes store their upper half first removes most of it and was measured SLOWER, by 550
// ticks per workgroup: the selects cost more than the conflicts.)
template <class Model, bool UCOL, int NS>
__device__ __forceinline__ void ug_emit_entry(UgLds<Model>& S, unsigned a, const UgTableau<NS>& R, int l) {
    float* e = &S.tab[a][0];
    auto put = [&](int off, const float* v) {
        *reinterpret_cast<float4*>(e + off) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4*>(e + off + 4) = make_float4(v[4], v[5], v[6], v[7]);
    };
    // the full columns: h, H, G W columns 0..2 (zero-order pass) / G (first-order pass)
    if constexpr (UCOL) put(l < 5 ? 8 * l : kUgTabX + 8 * (l - 5), R.c[0]);
    else put(kUgTabX + 8 * l, R.c[2]);
    // lanes 0..4: G W columns 3..7 / h, H; lanes 5..7: tau and the set
    const float* v = UCOL ? R.c[1] : R.c[0];
    const int half = l == 6 ? 4 : 0;
    float4 q;
    q.x = l < 5 ? v[0] : (l == 7 ? __uint_as_float(R.set) : (((R.set >> (half + 0)) & 1u) ? 0.f : 1.f));
    q.y = l < 5 ? v[1] : (l == 7 ? 0.f : (((R.set >> (half + 1)) & 1u) ? 0.f : 1.f));
    q.z = l < 5 ? v[2] : (l == 7 ? 0.f : (((R.set >> (half + 2)) & 1u) ? 0.f : 1.f));
    q.w = l < 5 ? v[3] : (l == 7 ? 0.f : (((R.set >> (half + 3)) & 1u) ? 0.f : 1.f));
    const int off = l < 5 ? (UCOL ? kUgTabX + 8 * (l + 3) : 8 * l) : (l == 7 ? kUgTabSet : kUgTabTau + half);
    *reinterpret_cast<float4*>(e + off) = q;
    if (l < 5) *reinterpret_cast<float4*>(e + off + 4) = make_float4(v[4], v[5], v[6], v[7]);
}

// All 256 entries: 64 tableaux of eight lanes.  Tableau g (6 bits) pivots the rows 0..5 that g has, emits entry g, and
// reaches g|64, g|128 and g|192 by pivots on rows 6 and 7 (row 7 once on a copy of g's tableau, once after row 6).
// The eight tableaux of a wave differ in the bits 0..2 -- those steps run for everyone, `want` decides -- and share the
// bits 3..5, whose steps the wave skips when it does not have them; the two waves of a SIMD (w and w + 4) are given
// complementary shared bits, so every SIMD runs 15 steps.
template <class Model, bool UCOL>
__device__ __forceinline__ void ug_build_table(UgLds<Model>& S, int tid) {
    constexpr int NC = Model::NC, NS = UCOL ? 2 : 3, NW = kUgBlock / 64;
    static_assert(NC == 8 && Model::NU == 4, "an 8 x 13 tableau, eight lanes each");
    const int l = tid & 7;
    for (int w = __builtin_amdgcn_readfirstlane(tid >> 6); w < 8; w += NW) {
        const unsigned shared = (unsigned)(w ^ ((w & 4) ? 3 : 0));
        const unsigned g = ((unsigned)(tid >> 3) & 7u) | (shared << 3);
        UgTableau<NS> R;
        {
            // T_0: column 0 = r0, 1..4 = C[j][:], 5..12 = W[:,c] (W is symmetric to the bit) [, G_0 = I]
            const float* c0 = l == 0 ? &S.r0[0] : (l < 5 ? &S.C[l - 1][0] : &S.W[l - 5][0]);
            const float* c1 = &S.W[l < 5 ? l + 3 : 0][0];              // lanes 5..7: an unused column, kept finite
            const float4 a0 = *reinterpret_cast<const float4*>(c0), a1 = *reinterpret_cast<const float4*>(c0 + 4);
            const float4 b0 = *reinterpret_cast<const float4*>(c1), b1 = *reinterpret_cast<const float4*>(c1 + 4);
            R.c[0][0] = a0.x; R.c[0][1] = a0.y; R.c[0][2] = a0.z; R.c[0][3] = a0.w;
            R.c[0][4] = a1.x; R.c[0][5] = a1.y; R.c[0][6] = a1.z; R.c[0][7] = a1.w;
            R.c[1][0] = b0.x; R.c[1][1] = b0.y; R.c[1][2] = b0.z; R.c[1][3] = b0.w;
            R.c[1][4] = b1.x; R.c[1][5] = b1.y; R.c[1][6] = b1.z; R.c[1][7] = b1.w;
            if constexpr (!UCOL) {
#pragma unroll
                for (int i = 0; i < NC; ++i) R.c[2][i] = (l == i) ? 1.f : 0.f;
            }
        }
        R.set = 0u;
        ug_pivot<0>(R, (g & 1u) != 0u, S.Wd[0]);
        ug_pivot<1>(R, (g & 2u) != 0u, S.Wd[1]);
        ug_pivot<2>(R, (g & 4u) != 0u, S.Wd[2]);
        if (shared & 1u) ug_pivot<3>(R, true, S.Wd[3]);
        if (shared & 2u) ug_pivot<4>(R, true, S.Wd[4]);
        if (shared & 4u) ug_pivot<5>(R, true, S.Wd[5]);
        UgTableau<NS> R6 = R, R7 = R;
        ug_pivot<6>(R6, true, S.Wd[6]);
        ug_pivot<7>(R7, true, S.Wd[7]);
        UgTableau<NS> R67 = R6;
        ug_pivot<7>(R67, true, S.Wd[7]);
        // the stores last, back to back: a broadcast queued behind stores would wait for them
        ug_emit_entry<Model, UCOL>(S, g, R, l);
        ug_emit_entry<Model, UCOL>(S, g | 64u, R6, l);
        ug_emit_entry<Model, UCOL>(S, g | 128u, R7, l);
        ug_emit_entry<Model, UCOL>(S, g | 192u, R67, l);
    }
}

// ---- the f64 nominal step, one wave, cooperatively ------------------------------------------------------------
// lane c < NC owns contact row c of the f64 geometry; lane (i,k) = 8 i + k owns entry (i,k) of the dual Hessian and
// of its masked LDL' (row order, pivot rule of the f64 solver: 1e-7).  The active set comes from the f32 pipeline at
// du = 0 and is re-checked -- and, if need be, corrected by primal-dual steps -- against the KKT conditions in f64
// (tolerance 1e-10 of max |r|, as irs_contact_qp_dual_exact<double>).  The primal solution of the step QP is unique,
// so whatever route finds a KKT point finds f(x_t, u_t).  Not settled within 8 corrections (never observed): the f32
// solution stands (1e-6 accurate).
struct UgNomLds {
    double J[8][7];
    double q[7], Dinv[7], b[7];
};

// (a) the f64 geometry: independent of the f32 prologue and of the table, so the nominal wave runs it BEFORE the
// workgroup's first barrier, beside wave 0's f32 assembly.  Leaves J, q, D^-1, b in LDS and returns r_c on lane c.
// The assembly is spread over the lanes (ug_geometry.hpp): lane c holds row c of J and element c of q, D^-1, b.
template <class Model, class Args>
__device__ __forceinline__ double ug_nominal_geometry(const Args& a, UgNomLds& L, int t, int lane) {
    constexpr int NC = Model::NC, n = Model::NX, m = Model::NU;
    static_assert(std::is_base_of<PlanarHandModel, Model>::value && NC == 8, "ug_hand_geometry is the planar hand's assembly");
    double x64[n], u64[m];
#pragma unroll
    for (int i = 0; i < n; ++i) x64[i] = a.x_trj[(size_t)t * n + i];
#pragma unroll
    for (int j = 0; j < m; ++j) u64[j] = a.u_trj[(size_t)t * m + j];
    UgHandLane<double> g;
    ug_hand_geometry<double>(a.p, x64, u64, lane, g);
    if (lane < NC) {
#pragma unroll
        for (int k = 0; k < n; ++k) L.J[lane][k] = g.J[k];
    }
    if (lane < n) { L.q[lane] = g.q; L.Dinv[lane] = g.Dinv; L.b[lane] = g.b; }
    // r_c = phi_c - sum_k J[c][k] (b_k D^-1_k) on lane c, over the k whose b is not zero, in ascending order: the
    // object's weight (k = 1) and the two joints of the row's arm (a row of link 0 has a zero at the second)
    const double bD = g.b * g.Dinv;
    const double bD1 = __shfl(bD, 1, 64), bD3 = __shfl(bD, 3, 64), bD4 = __shfl(bD, 4, 64), bD5 = __shfl(bD, 5, 64),
                 bD6 = __shfl(bD, 6, 64);
    const bool arm1 = (lane & 4) != 0;
    double s = fma(-bD1, g.J[1], g.phi);
    s = fma(-(arm1 ? bD5 : bD3), arm1 ? g.J[5] : g.J[3], s);
    s = fma(-(arm1 ? bD6 : bD4), arm1 ? g.J[6] : g.J[4], s);
    wave_sync();
    return lane < NC ? s : 0.0;
}

// (b) after the table exists: the f32 pipeline's active set at du = 0, then the cooperative f64 solve and its check
template <class Model, bool UCOL, class Args>
__device__ __forceinline__ void ug_nominal(const Args& a, const UgUni<Model::NC>& U, const UgLds<Model>& S,
                                           UgNomLds& L, double rr, int t, int lane) {
    constexpr int NC = Model::NC, n = Model::NX, m = Model::NU;
    static_assert(NC == 8 && n <= 8, "lane (i,k) = 8 i + k owns entry (i,k) of the 8 x 8 dual Hessian");
    // (1) the f32 pipeline at du = 0: the active set (every lane computes the same)
    float du0[m], r32[NC], lam32[NC];
#pragma unroll
    for (int j = 0; j < m; ++j) du0[j] = 0.f;
    const float tolv = ug_rhs<Model>(U, S, du0, r32);
    unsigned am = 0u;
    if (!ug_try<Model>(U, S, r32, du0, tolv, lam32, am)) ug_full<Model, UCOL>(S, r32, du0, tolv, am, lam32);
    unsigned set = 0u;
#pragma unroll
    for (int i = 0; i < NC; ++i) set |= (lam32[i] > 0.f) ? (1u << i) : 0u;
    set = (unsigned)__builtin_amdgcn_readfirstlane((int)set);
    {
        // entry (i,k) of W on lane 8 i + k
        const int li = lane >> 3, lk = lane & 7;
        double w = 0.0;
#pragma unroll
        for (int kk = 0; kk < n; ++kk) w += L.J[li][kk] * L.Dinv[kk] * L.J[lk][kk];
        double scale = 1e-300;
#pragma unroll
        for (int c = 0; c < NC; ++c) scale = fmax(scale, fabs(__shfl(rr, c, 64)));
        const double tol64 = 1e-10 * scale;
        double lamd = 0.0;          // lane i < NC: lam_i
        bool settled = false;
        for (int corr = 0; corr < 8 && !settled; ++corr) {
            // masked LDL' of W on `set`, entry-parallel
            double M = w, Lf = 0.0;
            unsigned eff = 0u;
            double invd[NC];
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                const double dj = __shfl(M, 9 * j, 64), wjj = __shfl(w, 9 * j, 64);
                const bool ok = ((set >> j) & 1u) && dj > 1e-7 * wjj;
                eff |= ok ? (1u << j) : 0u;
                invd[j] = ok ? 1.0 / dj : 0.0;
                const double Mij = __shfl(M, 8 * li + j, 64), Mkj = __shfl(M, 8 * lk + j, 64);
                if (lk == j && li > j) Lf = Mij * invd[j];
                if (li > j && lk > j) M -= Mij * invd[j] * Mkj;
            }
            // forward / diagonal / backward substitution on lanes 0..7
            const bool mine = lane < NC && ((eff >> lane) & 1u);
            double y = mine ? -rr : 0.0;
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                const double yj = __shfl(y, j, 64);
                const double Lij = __shfl(Lf, 8 * (lane & 7) + j, 64);
                if (lane < NC && lane > j) y -= Lij * yj;
            }
            double invme = 0.0;
#pragma unroll
            for (int j = 0; j < NC; ++j) invme = (lane == j) ? invd[j] : invme;
            y *= invme;
#pragma unroll
            for (int j = NC - 1; j >= 0; --j) {
                const double yj = __shfl(y, j, 64);
                const double Lji = __shfl(Lf, 8 * j + (lane & 7), 64);
                if (lane < j) y -= Lji * yj;
            }
            lamd = mine ? y : 0.0;
            // slacks: s_i = r_i + sum_k W_ik lam_k, reduced over the 8 lanes of row i
            double pr = w * __shfl(lamd, lk, 64);
            pr += __shfl_xor(pr, 1, 64);
            pr += __shfl_xor(pr, 2, 64);
            pr += __shfl_xor(pr, 4, 64);
            const double sl = rr + __shfl(pr, 8 * (lane & 7), 64);       // lane i < NC
            const bool neg = lane < NC && mine && !(lamd > 0.0);
            const bool viol = lane < NC && !mine && sl < -tol64;
            const unsigned negb = (unsigned)(__ballot(neg) & 0xffull), violb = (unsigned)(__ballot(viol) & 0xffull);
            if ((negb | violb) == 0u) settled = true;
            else set = (eff & ~negb) | violb;
        }
        // f_k = q_k + D^-1_k (sum_c J[c][k] lam_c - b_k) on lane k < n
        double f = 0.0;
        if (settled) {
            double acc = 0.0;
#pragma unroll
            for (int c = 0; c < NC; ++c) acc += L.J[c][lane < n ? lane : 0] * __shfl(lamd, c, 64);
            if (lane < n) f = L.q[lane] + L.Dinv[lane] * (acc - L.b[lane]);
        } else if (lane < n) {
            float acc = -S.Db0[lane];
#pragma unroll
            for (int c = 0; c < NC; ++c) acc = fmaf(S.JD[lane][c], lam32[c], acc);
            f = (double)(S.q[lane] + acc);
        }
        if (lane < n)
            __hip_atomic_store(a.fnom + (size_t)t * n + Model::perm(lane), f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// -DIRS_UG_STAMPS (tuning builds only): s_memtime at the phase boundaries of every workgroup -> a device buffer that
// irs_debug_ug_stamps copies out (tests/tools/ug_stamps.py; tools/ug_prologue_stamps.py prints the prologue's slots:
// 6 = wave 0's first fresh trip done, 10 = the nominal wave's f64 geometry done)
#ifdef IRS_UG_STAMPS
constexpr int kUgStampSlots = 12, kUgStampWgs = 2048;
__device__ unsigned long long ug_stamps[kUgStampWgs * kUgStampSlots];
#define UG_STAMP(slot)                                                                          \
    do {                                                                                        \
        if ((threadIdx.x & 63) == 0) {                                                          \
            const int wg_ = blockIdx.y * gridDim.x + blockIdx.x;                                \
            if (wg_ < kUgStampWgs && ((slot) < 8 ? threadIdx.x == 0 : true))                    \
                ug_stamps[wg_ * kUgStampSlots + (slot)] = __builtin_amdgcn_s_memtime();         \
        }                                                                                       \
    } while (0)
// samples per launch that [0] park, [1] settle in the flush's iterations, [2] enter the dual steps (irs_debug_ug_counts,
// tests/tools/ug_counts.py):
// counted per wave in scalars and added once, after the last stamp -- atomics inside the stamped phases stretch the timeline
__device__ unsigned ug_counts[3];
#define UG_COUNT_DECL unsigned ug_cnt_[3] = {0u, 0u, 0u}
#define UG_COUNT(k, pred) ug_cnt_[k] += (unsigned)__popcll(__ballot(pred))
#define UG_COUNT_FLUSH                                                                          \
    do {                                                                                        \
        if ((threadIdx.x & 63) == 0)                                                            \
            for (int k_ = 0; k_ < 3; ++k_)                                                      \
                if (ug_cnt_[k_] != 0u) atomicAdd(&ug_counts[k_], ug_cnt_[k_]);                  \
    } while (0)
#else
#define UG_STAMP(slot) do {} while (0)
#define UG_COUNT_DECL do {} while (0)
#define UG_COUNT(k, pred) do {} while (0)
#define UG_COUNT_FLUSH do {} while (0)
#endif

// The workgroup's prologue: the f32 geometry of the step QP at (x, u) (wave 0), what follows from it (W, r0, J D^-1, C:
// one quantity per thread) and the table (everyone; `build` false skips it: timing experiments).  Ends on a barrier.
// `early` runs in every thread once wave 0 has issued its loads of x and u: the place for memory requests of the
// caller's that should be in flight during the prologue without standing in front of those loads.
template <class Model, bool UCOL, class Early>
__device__ __forceinline__ void ug_prologue(const ModelParams& p, const double* x, const double* u, bool build,
                                            UgLds<Model>& S, int tid, Early early) {
    constexpr int n = Model::NX, m = Model::NU, NC = Model::NC;
    static_assert(std::is_base_of<PlanarHandModel, Model>::value && NC == 8, "ug_hand_geometry is the planar hand's assembly");
    const int lane = tid & 63, wave = tid >> 6;
    if (wave == 0) {
        // the model's QP assembly (trigonometry, closest points), spread over the lanes (ug_geometry.hpp): lane c < NC
        // holds and stores row c of J and phi_c, lane k < n element k of q, D^-1, b
        double xd[n], ud[m];
#pragma unroll
        for (int i = 0; i < n; ++i) xd[i] = x[i];
#pragma unroll
        for (int j = 0; j < m; ++j) ud[j] = u[j];
        early();
        float xb[n], ub[m];
#pragma unroll
        for (int i = 0; i < n; ++i) xb[i] = (float)xd[i];
#pragma unroll
        for (int j = 0; j < m; ++j) ub[j] = (float)ud[j];
        UgHandLane<float> g;
        ug_hand_geometry<float>(p, xb, ub, lane, g);
        if (lane < NC) {
            S.phi[lane] = g.phi;
#pragma unroll
            for (int k = 0; k < n; ++k) S.Jc[lane][k] = g.J[k];
        }
        if (lane < n) { S.Db0[lane] = g.b * g.Dinv; S.q[lane] = g.q; S.Dinv[lane] = g.Dinv; }
        if (lane >= Model::act(0) && lane < Model::act(0) + m) S.DK[lane - Model::act(0)] = g.Dinv * g.kp;
    } else {
        early();
    }
    __syncthreads();
    // what follows from it, one quantity per thread (the expressions of irs_contact_qp_dual_exact_try):
    //   W = J D^-1 J' (entry (i,j) from the row pair (max, min): symmetric to the bit), r0 = phi - J D^-1 b,
    //   J D^-1, C = J D^-1[:, act] K
    if (tid < NC * NC) {
        const int i = tid / NC, j = tid % NC, hi = i > j ? i : j, lo = i > j ? j : i;
        float w = (S.Jc[hi][0] * S.Dinv[0]) * S.Jc[lo][0];
#pragma unroll
        for (int k = 1; k < n; ++k) w = w + (S.Jc[hi][k] * S.Dinv[k]) * S.Jc[lo][k];
        S.W[i][j] = w;
        if (i == j) {
            S.Wd[i] = w;
            S.invw[i] = (float)kContactPgsOmega * irs_rcp_fast(w);
        }
    } else if (tid < NC * NC + NC) {
        const int i = tid - NC * NC;
        float ri = S.phi[i];
#pragma unroll
        for (int k = 0; k < n; ++k) ri = ri - S.Jc[i][k] * S.Db0[k];
        S.r0[i] = ri;
    } else if (tid < 2 * NC * NC + NC) {
        const int e = tid - (NC * NC + NC), k = e / NC, c = e % NC;
        if (k < n) S.JD[k][c] = S.Jc[c][k] * S.Dinv[k];
    } else if (tid < 2 * NC * NC + NC + m * NC) {
        const int e = tid - (2 * NC * NC + NC), j = e / NC, c = e % NC;
        S.C[j][c] = (S.Jc[c][Model::act(j)] * S.Dinv[Model::act(j)]) * Model::template stiffness<float>(p, j);
    }
    __syncthreads();
    UG_STAMP(1);
    if (build) {
        if constexpr (kUgTableLdl) {
            for (int e = tid; e < 2 * (1 << NC); e += kUgBlock) ug_build_entry<Model, UCOL>(S, (unsigned)(e >> 1), e & 1);
        } else {
            ug_build_table<Model, UCOL>(S, tid);
        }
    }
    __syncthreads();
}

// One workgroup runs the prologue at one state and copies the table out (irs_debug_ug_table; the pad of an entry as 0).
template <class Model, bool UCOL>
__global__ __launch_bounds__(kUgBlock) void ug_table_kernel(ModelParams p, const double* x, const double* u, float* out) {
    __shared__ UgLds<Model> S;
    const int tid = threadIdx.x;
    ug_prologue<Model, UCOL>(p, x, u, true, S, tid, [] {});
    constexpr int NE = 1 << Model::NC;
    for (int q = tid; q < NE * kUgTabStride; q += kUgBlock) {
        const int c = q % kUgTabStride;
        out[q] = (c > kUgTabSet && c < kUgTabX) ? 0.f : S.tab[q / kUgTabStride][c];
    }
}

// BATCH (smooth_common.hpp, SmoothRow): grid (nblk, B T); `a` is then the view of the row's problem, set up at the entry
template <class Model, int MODE, bool RNG, bool FUSE, bool BATCH>
__global__ __launch_bounds__(kUgBlock) void smooth_ug_kernel(SmoothArgs args, std::conditional_t<BATCH, SmoothBatch, SmoothSolo> bat) {
    using TR = SmoothTraits<Model, MODE>;
    constexpr int n = TR::n, m = TR::m, P = TR::P, NC = Model::NC;
    constexpr int BLOCK = kUgBlock, NW = BLOCK / 64;
    static_assert(TR::Z0 == n && NC == 8 && m == 4, "u-only smoothing of an 8-row contact model with 4 commands");
    static_assert(P < kBlock, "the hand-off's group reduction");
    // internal statistics of the zero-order pass: [upper Gram of du (NG) | du lam' (m x NC) | sum du (m)]
    constexpr int NG = m * (m + 1) / 2;
    constexpr int PI = TR::FIRST_B ? 1 : NG + m * NC + m;
    constexpr int PPI = irs_reduce_pad(TR::FIRST_B ? n * m : PI);
    constexpr int QE = m + 1;
    constexpr bool UCOL = !TR::FIRST_B && kUgStepColumns;      // the table's X: G W (dual steps read a column) / G (the first-order epilogue reads M)
    __shared__ UgLds<Model> S;
    __shared__ UgNomLds nomL;
    __shared__ float ring_all[NW * kUgRing * QE];
    __shared__ float red[NW * (PPI > TR::PP ? PPI : TR::PP)];
    __shared__ float toti[PPI];
    __shared__ unsigned hist[TR::FIRST_B ? (1 << NC) : 1];
    __shared__ double red64[TR::NGRP * P];
    __shared__ double tot[P];
    __shared__ FinalizeLds<Model, MODE> fin;
    __shared__ int s_ticket;

    decltype(auto) a = smooth_row<Model, MODE>(args, bat, (int)blockIdx.y);
    const int t = smooth_row_t(a, (int)blockIdx.y), blk = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;

    UG_STAMP(0);
    // ---- prologue: the timestep's geometry (wave 0; the nominal wave its f64 twin), then the table (everyone) ------
    const bool nominal_wave = blk == 0 && wave == NW - 1;
    double nom_r = 0.0;
    if (nominal_wave && !(a.diag & 2)) nom_r = ug_nominal_geometry<Model>(a, nomL, t, lane);
    if (nominal_wave) UG_STAMP(10);
    if constexpr (TR::FIRST_B) {
        for (int q = tid; q < (1 << NC); q += BLOCK) hist[q] = 0u;
    }
    // 64-sample blocks are dealt round robin to the waves of the timestep: rounds 0 .. kUgNomRounds - 1 to all but
    // the nominal wave (which is busy with the f64 step for about that long), later rounds to all of them
    const int V = a.nblk * NW;
    const int me = nominal_wave ? V - 1 : (blk == 0 ? wave : blk * NW - 1 + wave);
    const int nblocks = (a.N + 63) / 64;
    const int round0 = nominal_wave ? kUgNomRounds : 0;
    auto block_of = [&](int k) { return k < kUgNomRounds ? k * (V - 1) + me : kUgNomRounds * (V - 1) + (k - kUgNomRounds) * V + me; };
    // the perturbations of the NEXT fresh trip are requested while this one computes: a trip is ~1.5 us of
    // arithmetic, an HBM round trip ~0.5-1 us, and a SIMD holds two waves -- nothing else would hide it.  (No
    // other vector-memory operation sits inside a trip, so the wait lands where the sample is consumed.)  Those of
    // the FIRST trip are requested from inside the prologue and are in flight during the geometry and the table build.
    float du_next[m];
#pragma unroll
    for (int j = 0; j < m; ++j) du_next[j] = 0.f;
    auto request = [&](int block) {
        if constexpr (!RNG) {
            if (block < nblocks) {
                const int sidx = block * 64 + lane;
                const size_t row = (size_t)t * a.N + (sidx < a.N ? sidx : a.N - 1);
                load_row<m>(a.du + row * m, du_next);
            }
        }
    };
    ug_prologue<Model, UCOL>(a.p, a.x_trj + (size_t)t * n, a.u_trj + (size_t)t * m, !(a.diag & 4), S, tid,
                             [&] { if (!(a.diag & 8)) request(block_of(round0)); });

    UG_STAMP(2);
    // the uniform operands of the sweeps, in VECTOR registers (one copy per lane).  Measured on gfx950
    // (tools/microbench/valu_issue.hip): a v_fmac_f32 with ONE scalar-register operand costs a SIMD 6.4 cycles at two
    // waves per SIMD (12.4 at one) against 2.9 with vector operands only -- scalar operands are read through a path
    // the four SIMDs of a CU share -- so keeping W in SGPRs would more than halve the rate of the sweeps.
    UgUni<NC> U;
    {
        int q = 0;
#pragma unroll
        for (int i = 0; i < NC; ++i)
#pragma unroll
            for (int j = i; j < NC; ++j) U.W[q++] = S.W[i][j];
#pragma unroll
        for (int i = 0; i < NC; ++i) { U.invw[i] = S.invw[i]; U.r0[i] = S.r0[i]; }
    }

    float acc[PPI];
#pragma unroll
    for (int i = 0; i < PPI; ++i) acc[i] = 0.f;

    if (nominal_wave && !(a.diag & 2)) ug_nominal<Model, UCOL>(a, U, S, nomL, nom_r, t, lane);
    if (nominal_wave) UG_STAMP(8);
    UG_COUNT_DECL;
    if (!(a.diag & 8)) {
        int round = round0;
        float* ring = ring_all + wave * (kUgRing * QE);
        int qhead = 0, qtail = 0;                           // wave-uniform
        int bk = block_of(round);                           // (its perturbations: requested in the prologue)
        while (true) {
            const bool fresh = bk < nblocks;
            const int pending = qtail - qhead;
            const bool flush = pending >= 64 || (!fresh && pending > 0);
            if (!fresh && !flush) break;
            float du[m], r[NC], lam[NC];
            bool on, fin_ = true;
            if (flush) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                const int take = min(64, pending);
                on = lane < take;
                const int slot = (qhead + (on ? lane : 0)) & (kUgRing - 1);
#pragma unroll
                for (int j = 0; j < m; ++j) du[j] = ring[slot * QE + j];
                unsigned wm = __float_as_uint(ring[slot * QE + m]);
                const float tolv = ug_rhs<Model>(U, S, du, r);
                // the iteration goes on from the parked set; what it still does not settle takes the dual steps
                // (a lane past `take` carries lane 0's sample and finishes with it)
                bool settled = false;
                if constexpr (kUgPdasFlush > 0) ug_pdas<Model, kUgPdasFlush>(S, du, tolv, wm, lam, settled);
                UG_COUNT(1, on && settled);
                UG_COUNT(2, on && !settled);
                if (!__all(settled)) {
                    float lf[NC];
                    ug_full<Model, UCOL>(S, r, du, tolv, wm, lf, (a.diag & 128) ? 8 : ((a.diag & 256) ? 12 : 4 * NC));
#pragma unroll
                    for (int i = 0; i < NC; ++i) lam[i] = settled ? lam[i] : lf[i];
                }
                qhead += take;
            } else {
                const int sidx = bk * 64 + lane;
                on = sidx < a.N;
                if constexpr (RNG) {
                    const unsigned long long gidx = a.sample_offset + (unsigned long long)sidx;
#pragma unroll
                    for (int j = n / 4; j < (n + m + 3) / 4; ++j) {
                        float g4[4];
                        philox_normal4(gidx, (unsigned)t, (unsigned)j, a.iter, a.seed, g4);
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            const int idx = 4 * j + c;
                            if (idx >= n && idx < n + m) du[idx - n] = __fmul_rn(g4[c], a.std[idx]);
                        }
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < m; ++j) du[j] = du_next[j];
                    request(block_of(round + 1));
                }
                const float tolv = ug_rhs<Model>(U, S, du, r);
                unsigned mask = 0u;
                fin_ = ug_try<Model>(U, S, r, du, tolv, lam, mask, a.diag);
                if (a.diag & 16) fin_ = true;
                const bool hard = on && !fin_;
                const unsigned long long bal = __ballot(hard);
                UG_COUNT(0, hard);
                if (hard) {
                    const int slot = (qtail + __popcll(bal & ((1ull << lane) - 1ull))) & (kUgRing - 1);
#pragma unroll
                    for (int j = 0; j < m; ++j) ring[slot * QE + j] = du[j];
                    ring[slot * QE + m] = __uint_as_float(mask);
                }
                qtail += __popcll(bal);
                bk = block_of(++round);
            }
            const bool use = on && fin_;
            // a non-finite perturbation must not vanish in a clamp: poison the statistics (tested on the bit pattern)
            bool nonfinite = false;
#pragma unroll
            for (int j = 0; j < m; ++j) nonfinite = nonfinite || irs_nonfinite_bits(du[j]);
            if constexpr (TR::FIRST_B) {
                unsigned I = 0u;
#pragma unroll
                for (int i = 0; i < NC; ++i) I |= (lam[i] * S.Wd[i] > (float)kContactActiveTol) ? (1u << i) : 0u;
                if (use) __hip_atomic_fetch_add(&hist[I], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                if (on && nonfinite) acc[0] = irs_poison();
            } else {
                float zz[m];
#pragma unroll
                for (int j = 0; j < m; ++j) zz[j] = use ? du[j] : 0.f;
                int q = 0;
#pragma unroll
                for (int i = 0; i < m; ++i)
#pragma unroll
                    for (int j = i; j < m; ++j) { acc[q] = fmaf(zz[i], zz[j], acc[q]); ++q; }
#pragma unroll
                for (int i = 0; i < m; ++i)
#pragma unroll
                    for (int c = 0; c < NC; ++c) { acc[q] = fmaf(zz[i], lam[c], acc[q]); ++q; }
#pragma unroll
                for (int i = 0; i < m; ++i) { acc[q] += zz[i]; ++q; }
                if (on && nonfinite) acc[0] = irs_poison();
            }
            if (!flush && round == round0 + 1) UG_STAMP(6);     // wave 0: its first fresh trip done
        }
    }

    UG_STAMP(3);
    if (blk == 0 && wave == 1) UG_STAMP(9);
    // ---- workgroup statistics in the layout of `sums` (include/irs_hip.h) --------------------------------------
    if constexpr (TR::FIRST_B) {
        // sum over the samples of B(I_s) = sum over the occupied active sets of count(I) B(I), with
        //   Y = W_II^+ J[:, act] = -M_I J[:, act],   B[k][c] = [k = act c] - D^-1_k sum_i J[i][k] Y[i][c]
        // (irs_contact_qp_grad, WITH_A = false; the table's pivot rule is the derivative's, 1e-5)
        __syncthreads();
        unsigned poison_bits = __float_as_uint(acc[0]);
        asm volatile("" : "+v"(poison_bits));
#pragma unroll
        for (int i = 0; i < PPI; ++i) acc[i] = 0.f;
        for (int I = tid; I < (1 << NC); I += BLOCK) {
            const unsigned cnt = hist[I];
            if (cnt == 0u) continue;
            const float* e = &S.tab[I][0];
            const unsigned ap = __float_as_uint(e[kUgTabSet]);
            float Y[NC][m];
#pragma unroll
            for (int i = 0; i < NC; ++i) {
                const bool in = ((ap >> i) & 1u) != 0u;
#pragma unroll
                for (int c = 0; c < m; ++c) {
                    float s = 0.f;
#pragma unroll
                    for (int j = 0; j < NC; ++j) s = fmaf(e[kUgTabX + 8 * j + i], S.Jc[j][Model::act(c)], s);    // G[i][j] = M[i][j] on the set
                    Y[i][c] = in ? -s : 0.f;
                }
            }
#pragma unroll
            for (int k = 0; k < n; ++k)
#pragma unroll
                for (int c = 0; c < m; ++c) {
                    float s = 0.f;
#pragma unroll
                    for (int i = 0; i < NC; ++i) s = fmaf(S.Jc[i][k], Y[i][c], s);
                    const float Bkc = (k == Model::act(c) ? 1.f : 0.f) - S.Dinv[k] * s;
                    acc[Model::perm(k) * m + c] += (float)cnt * Bkc;
                }
        }
        if ((poison_bits & 0x7f800000u) == 0x7f800000u) acc[0] = irs_poison();
        block_reduce_lds<P, NW>(acc, red);
    } else {
        block_reduce_lds<PI, NW>(acc, red);
        __syncthreads();
        for (int q = tid; q < PI; q += BLOCK) {
            float s = red[q];
#pragma unroll
            for (int w = 1; w < NW; ++w) s += red[w * PPI + q];
            toti[q] = s;
        }
        __syncthreads();
        // [Gram | du (f - xb)' | sum du]:  df_k = sum_c JD[k][c] lam_c - Db0_k + [k = act j] (D^-1 K)_j du_j
        float out = 0.f;
        if (tid < P) {
            if (tid < NG) out = toti[tid];
            else if (tid < NG + m * n) {
                const int i = (tid - NG) / n, kext = (tid - NG) % n;
                int k = 0, jact = -1;
#pragma unroll
                for (int kk = 0; kk < n; ++kk) k = (Model::perm(kk) == kext) ? kk : k;
#pragma unroll
                for (int j = 0; j < m; ++j) jact = (Model::act(j) == k) ? j : jact;
                float s = -S.Db0[k] * toti[NG + m * NC + i];
                for (int c = 0; c < NC; ++c) s = fmaf(S.JD[k][c], toti[NG + i * NC + c], s);
                if (jact >= 0) {
                    const int lo = i < jact ? i : jact, hi = i < jact ? jact : i;
                    s = fmaf(S.DK[jact], toti[lo * m - lo * (lo - 1) / 2 + (hi - lo)], s);
                }
                out = s;
            } else {
                out = toti[NG + m * NC + (tid - NG - m * n)];
            }
        }
        __syncthreads();
        for (int q = tid; q < NW * TR::PP; q += BLOCK) red[q] = 0.f;
        __syncthreads();
        if (tid < P) red[tid] = out;
    }
    UG_STAMP(4);
    smooth_finish<Model, MODE, FUSE, BLOCK, true, std::remove_cv_t<std::remove_reference_t<decltype(a)>>>(a, red, red64, tot, fin, s_ticket, t, blk, tid, a.fnom + (size_t)t * n);
    UG_STAMP(5);
    UG_COUNT_FLUSH;
}

template <class Model, int MODE>
void ug_launch_m(const SmoothArgs& a, bool rng, bool fuse, hipStream_t st) {
    dim3 grid(a.nblk, a.T), block(kUgBlock);
    if (rng) {
        if (fuse) hipLaunchKernelGGL((smooth_ug_kernel<Model, MODE, true, true, false>), grid, block, 0, st, a, SmoothSolo{});
        else hipLaunchKernelGGL((smooth_ug_kernel<Model, MODE, true, false, false>), grid, block, 0, st, a, SmoothSolo{});
    } else {
        if (fuse) hipLaunchKernelGGL((smooth_ug_kernel<Model, MODE, false, true, false>), grid, block, 0, st, a, SmoothSolo{});
        else hipLaunchKernelGGL((smooth_ug_kernel<Model, MODE, false, false, false>), grid, block, 0, st, a, SmoothSolo{});
    }
}

template <class Model, int MODE>
void ug_launch_batch_m(const SmoothArgs& a, const SmoothBatch& bat, int B, hipStream_t st) {
    dim3 grid(a.nblk, B * a.T), block(kUgBlock);
    hipLaunchKernelGGL((smooth_ug_kernel<Model, MODE, true, true, true>), grid, block, 0, st, a, bat);
}

}  // namespace

#ifdef IRS_UG_STAMPS
extern "C" int irs_debug_ug_stamps(unsigned long long* host_out, int n_wgs) {
    if (n_wgs > kUgStampWgs) n_wgs = kUgStampWgs;
    return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(ug_stamps), (size_t)n_wgs * kUgStampSlots * sizeof(unsigned long long));
}
// the three sample counts since the last reset (reset != 0: zero them after the copy)
extern "C" int irs_debug_ug_counts(unsigned* host_out3, int reset) {
    hipError_t e = hipMemcpyFromSymbol(host_out3, HIP_SYMBOL(ug_counts), 3 * sizeof(unsigned));
    const unsigned zero[3] = {0u, 0u, 0u};
    if (e == hipSuccess && reset) e = hipMemcpyToSymbol(HIP_SYMBOL(ug_counts), zero, sizeof(zero));
    return (int)e;
}
#endif

// The table of one state as the sample pass builds it (first_order: the first-order pass's, whose X block is G): 256
// entries of 116 floats in the layout above.  params, x (7), u (4) and out are HOST pointers.  A test hook, not part of
// include/irs_hip.h.
extern "C" int irs_debug_ug_table(int model, const double* params, const double* x, const double* u, int first_order,
                                  float* out_256x116) {
    using Model = PlanarHandExactModel;
    if (model != IRS_MODEL_PLANAR_HAND_EXACT) return IRS_ERR_UNSUPPORTED;
    IRS_CHECK_ARG(x && u && out_256x116, "null pointer");
    ModelParams p;
    int rc = irs_load_params(model, params, Model::NPARAMS, &p);
    if (rc != IRS_OK) return rc;
    constexpr size_t NOUT = (size_t)(1 << Model::NC) * kUgTabStride;
    double* dxu = nullptr;
    float* dout = nullptr;
    if (hipMalloc(&dxu, (Model::NX + Model::NU) * sizeof(double)) != hipSuccess) return IRS_ERR_HIP;
    if (hipMalloc(&dout, NOUT * sizeof(float)) != hipSuccess) { (void)hipFree(dxu); return IRS_ERR_HIP; }
    hipError_t e = hipMemcpy(dxu, x, Model::NX * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dxu + Model::NX, u, Model::NU * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        if (first_order) hipLaunchKernelGGL((ug_table_kernel<Model, false>), dim3(1), dim3(kUgBlock), 0, 0, p, dxu, dxu + Model::NX, dout);
        else hipLaunchKernelGGL((ug_table_kernel<Model, kUgStepColumns>), dim3(1), dim3(kUgBlock), 0, 0, p, dxu, dxu + Model::NX, dout);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out_256x116, dout, NOUT * sizeof(float), hipMemcpyDeviceToHost);
    (void)hipFree(dxu);
    (void)hipFree(dout);
    return e == hipSuccess ? IRS_OK : IRS_ERR_HIP;
}

bool irs_smooth_ug_supported(int model, int mode) {
    const char* e = getenv("IRS_UG");
    if (e != nullptr && atoi(e) == 0) return false;
    return model == IRS_MODEL_PLANAR_HAND_EXACT && (mode == IRS_SMOOTH_ZERO_ORDER_B || mode == IRS_SMOOTH_FIRST_ORDER);
}

// workgroups per timestep: one 512-thread workgroup per CU holds the 116 KB table, so the grid is about the CU count
// and every wave loops over its share of the 64-sample blocks; never more workgroups than blocks / 8
int irs_smooth_ug_nblk(int T, int N) {
    static int cus = 0;
    if (cus == 0) {
        hipDeviceProp_t prop;
        int dev = 0;
        cus = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
                  ? prop.multiProcessorCount : 256;
        if (cus < 1) cus = 256;
    }
    const int nblocks = (N + 63) / 64, NW = kUgBlock / 64;
    int nb = cus / (T < 1 ? 1 : T);
    if (nb < 1) nb = 1;
    const int by_work = (nblocks + 1 + NW - 1) / NW;     // + 1: the nominal wave
    if (nb > by_work) nb = by_work;
    return nb < 1 ? 1 : nb;
}

int irs_smooth_ug_launch(int model, int mode, const SmoothArgs& a, bool rng, bool fuse, hipStream_t st) {
    if (model != IRS_MODEL_PLANAR_HAND_EXACT) return IRS_ERR_UNSUPPORTED;
    if (mode == IRS_SMOOTH_ZERO_ORDER_B) ug_launch_m<PlanarHandExactModel, IRS_SMOOTH_ZERO_ORDER_B>(a, rng, fuse, st);
    else if (mode == IRS_SMOOTH_FIRST_ORDER) ug_launch_m<PlanarHandExactModel, IRS_SMOOTH_FIRST_ORDER>(a, rng, fuse, st);
    else return IRS_ERR_UNSUPPORTED;
    return IRS_OK;
}

int irs_smooth_ug_launch_batch(int model, int mode, const SmoothArgs& a, const SmoothBatch& bat, int B, hipStream_t st) {
    if (model != IRS_MODEL_PLANAR_HAND_EXACT) return IRS_ERR_UNSUPPORTED;
    if (mode == IRS_SMOOTH_ZERO_ORDER_B) ug_launch_batch_m<PlanarHandExactModel, IRS_SMOOTH_ZERO_ORDER_B>(a, bat, B, st);
    else if (mode == IRS_SMOOTH_FIRST_ORDER) ug_launch_batch_m<PlanarHandExactModel, IRS_SMOOTH_FIRST_ORDER>(a, bat, B, st);
    else return IRS_ERR_UNSUPPORTED;
    return IRS_OK;
}
