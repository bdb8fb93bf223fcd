// Box-constrained TV-LQR: solve_tvlqr with ACTIVE abs bounds (irs_lqr/tv_lqr.py:112-123)
// inside the MPC loop of IrsLqr.local_descent (irs_lqr/irs_lqr.py:169-184): for every t the
// tail QP over t..T is re-solved from the realised state and only its first control is
// applied to the TRUE dynamics.
//
// The reference hands each QP to OSQP.  Here: ADMM on the box, with the equality-
// constrained (LQR) sub-problem solved exactly by a Riccati sweep,
//     z <- argmin f(z) + rho/2 |z - w + y|^2 ,  w <- clip(a z + (1-a) w + y) ,  y <- y + ... - w,
// where only bounded components carry a rho term.  The Riccati matrices depend on
// (A,B,Q,R,rho) but not on the linear terms, so ONE backward factorisation (kept in LDS)
// serves every ADMM iteration of every one of the T tail re-solves; an ADMM iteration is
// then two vector sweeps over the horizon.  Successive re-solves are warm started.
// Restated in oracle/irs_oracle.py (tvlqr_box_factor / tvlqr_box_solve / local_descent_box),
// whose solutions are certified against the QP's KKT conditions.
//
//
// Position-controlled (quasistatic) variant, DU = true: IrsLqrQuasistatic.local_descent
// (irs_lqr/irs_lqr_quasistatic.py:286-345) calls solve_tvlqr with indices_u_into_x, whose cost is
// on du_t = u_t - u_{t-1} (du_0 = u_0 - x_0[idx], irs_lqr/tv_lqr.py:98-108, full R: alpha = 1) and
// whose bounds are per-time trust regions (x_bound_abs, u_bound_abs) and rate limits
// (u_bound_rel).  That QP is the SAME box-LQR in the augmented state z = [x; u_prev] with control
// v = du:  z+ = [[A,B],[0,I]] z + [B;I] v + [c;0],  cost (x-xd)'Q(x-xd) + v'Rv,  box on z
// (x bounds; u bounds = bounds on the u_prev block one step later) and on v.  The augmented
// matrices are never materialised: accessors below read (A,B,c) directly.
//
// One wave, f64: a latency-bound chain like the Riccati pass.  The ADMM vectors and the scratch live in
// (dynamic) LDS.  The T factor records live there too while they fit (HBM = false); beyond that -- or when the
// caller asks for it -- they live in a caller workspace in HBM (HBM = true, same source): the factorisation
// builds each record in an LDS slot and stores it once, and the sweeps, whose record addresses are known in
// advance, stage them back through a 3-slot LDS ring two steps ahead of use (global_load_dwordx4 into
// registers, ds_write_b128 one step before the record is needed).  The arithmetic and its order are the same
// on both paths: they give bit-identical results.
#include <climits>

#include "boxqp.hpp"
#include "boxqp_layout.hpp"
#include "wave.hpp"

namespace {

template <int N, int M>
struct BoxLayout {
    // per-timestep factor record: box_rec_layout (boxqp_layout.hpp) at compile time
    static constexpr BoxRec rec = box_rec_layout(N, M);
    static constexpr int oAcl = rec.oAcl, oK = rec.oK, oMinv = rec.oMinv, oHinv = rec.oHinv, oB = rec.oB, oC = rec.oC,
                         oD = rec.oD, oQx = rec.oQx, S = rec.S;
    static __host__ __device__ size_t doubles(int T) {
        // factor records + qx_T + wx,yx,zx (T+1,N) + wu,yu,zu,k (T,M) + scratch
        return (size_t)T * S + N + 3 * (size_t)(T + 1) * N + 4 * (size_t)T * M + 4 * N * N + 8 * N + 4 * M + 64;
    }
    // records in HBM: stride padded to 16 B; on chip only the 3-slot staging ring stays in place of the records
    static constexpr int SP = rec.SP, RING = kBoxRing;
    static __host__ __device__ size_t hbm_doubles(int T) { return doubles(T) - (size_t)T * S + (size_t)RING * SP; }
    static size_t record_bytes(int T) { return ((size_t)T * SP * sizeof(double) + 255) / 256 * 256; }
};

typedef double v2d __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) v2d gv2d;    // global: a generic pointer would make these flat accesses,
                                                        // which also count in lgkmcnt and would stall at every wave_sync

// ADAPT: the penalty rho follows the residuals (the rule: see the MPC loop below), and the factorisation runs again
// with each new rho.  ADAPT = false reads nothing of `ad` and is the fixed-rho kernel, instruction for instruction.
//
// LAZY (on top of ADAPT): the bounds are enforced lazily -- constraint generation.  Only the components of a set S
// carry a rho term and are projected: mxv / muv are then "finite bound AND in S" (what the factorisation, the sweeps,
// the projection, the residuals and the adaptive rule's norms read), and the "finite bound" masks move to fxv / fuv.
// When a tail has converged, every dropped component's plan entry is compared with its bounds; components that leave
// them join S (w = clip(z), y = 0 on the tail's rows), the factorisation runs again from the tail's first step, and
// the same tail goes on.  A converged plan that keeps every dropped bound is feasible for the full QP and optimal for
// a relaxation of it: it is the full QP's solution, to the ADMM's tolerance.  S only grows, and stays for the tails
// that follow.  LAZY = false reads nothing of ad.lazy (the parameter is then a plain BoxAdapt).
template <class Model, bool DU, bool HBM, bool ADAPT, bool LAZY = false>
__global__ __launch_bounds__(64) void box_descent_kernel(BoxArgs a, double* recs,
                                                         std::conditional_t<LAZY, BoxAdaptLazy, BoxAdapt> ad) {
    static_assert(ADAPT || !LAZY, "the lazy form is compiled on top of the adaptive one");
    if (a.run_flag != nullptr && *a.run_flag == 0) return;          // uniform
    constexpr int NR = Model::NX, M = Model::NU;      // real state / control sizes
    constexpr int N = NR + (DU ? M : 0);              // size of the QP's state (z = [x; u_prev] if DU)
    constexpr double INF = __builtin_huge_val();
    using L = BoxLayout<N, M>;
    // augmented problem data, read straight from the caller's (A, B, c, Q, Qd, xd)
    auto A_ = [&](int t, int i, int j) -> double {
        if (i < NR) return j < NR ? a.At[((size_t)t * NR + i) * NR + j] : a.Bt[((size_t)t * NR + i) * M + (j - NR)];
        return i == j ? 1.0 : 0.0;
    };
    auto B_ = [&](int t, int i, int j) -> double {
        if (i < NR) return a.Bt[((size_t)t * NR + i) * M + j];
        return (i - NR) == j ? 1.0 : 0.0;
    };
    auto c_ = [&](int t, int i) -> double { return i < NR ? a.ct[(size_t)t * NR + i] : 0.0; };
    auto xd_ = [&](int t, int i) -> double { return i < NR ? a.xd[(size_t)t * NR + i] : 0.0; };
    // bounds of the QP's state component i at time t, and of its control component j
    auto zlo_ = [&](int t, int i) -> double {
        if (i < NR) return a.xlo ? a.xlo[(size_t)t * a.sx + i] : -INF;
        return (a.ulo && t >= 1) ? a.ulo[(size_t)(t - 1) * a.su + (i - NR)] : -INF;
    };
    auto zhi_ = [&](int t, int i) -> double {
        if (i < NR) return a.xhi ? a.xhi[(size_t)t * a.sx + i] : INF;
        return (a.uhi && t >= 1) ? a.uhi[(size_t)(t - 1) * a.su + (i - NR)] : INF;
    };
    auto vlo_ = [&](int t, int j) -> double {
        if (DU) return a.dlo ? a.dlo[(size_t)t * a.sd + j] : -INF;
        return a.ulo ? a.ulo[(size_t)t * a.su + j] : -INF;
    };
    auto vhi_ = [&](int t, int j) -> double {
        if (DU) return a.dhi ? a.dhi[(size_t)t * a.sd + j] : INF;
        return a.uhi ? a.uhi[(size_t)t * a.su + j] : INF;
    };
    extern __shared__ double lds[];
    const int T = a.T, lane = threadIdx.x;
    double* F = lds;                                   // T records of L::S doubles, or (HBM) the ring: 3 x L::SP
    double* qxT = F + (HBM ? (size_t)L::RING * L::SP : (size_t)T * L::S);   // Qd xd_T
    double* wx = qxT + N;                              // (T+1, N)
    double* yx = wx + (size_t)(T + 1) * N;
    double* zx = yx + (size_t)(T + 1) * N;
    double* wu = zx + (size_t)(T + 1) * N;             // (T, M)
    double* yu = wu + (size_t)T * M;
    double* zu = yu + (size_t)T * M;
    double* kk = zu + (size_t)T * M;
    double* P = kk + (size_t)T * M;                    // scratch: P, A, W (N x N), vectors
    double* Am = P + N * N;
    double* Wm = Am + N * N;
    double* PB = Wm + N * N;                           // N x M  (fits in N*N)
    double* pv = PB + N * N;                           // p (N)
    double* gv = pv + N;                               // g (N)
    double* sv = gv + N;                               // s (M) .. padded to N
    double* mxv = sv + N;                              // bounded masks (any finite bound at any t)
    double* muv = mxv + N;                             // (M)
    double* Hs = muv + M;                              // M x M scratch (<= 16)
    double* fxv = Hs + M * M;                          // LAZY: the finite-bound masks (N), (M), in the layout's slack
    double* fuv = fxv + N;
    static_assert(!LAZY || (5 * N + 2 * M + M * M <= 8 * N + 4 * M + 64 && M <= N), "no room for the lazy masks");
    (void)fxv; (void)fuv;

    // ---- setup ------------------------------------------------------------------------
    if (lane < N) {
        bool any = false;
        for (int t = 1; t <= T; ++t) any = any || isfinite(zlo_(t, lane)) || isfinite(zhi_(t, lane));
        mxv[lane] = any ? 1.0 : 0.0;
    }
    if (lane < M) {
        bool any = false;
        for (int t = 0; t < T; ++t) any = any || isfinite(vlo_(t, lane)) || isfinite(vhi_(t, lane));
        muv[lane] = any ? 1.0 : 0.0;
    }
    if constexpr (LAZY) {                              // (each lane: the entry it has just written)
        const int* e = ad.lazy.enforced_io;
        if (lane < N) {
            fxv[lane] = mxv[lane];
            if (e == nullptr || e[lane] == 0) mxv[lane] = 0.0;
        }
        if (lane < M) {
            fuv[lane] = muv[lane];
            if (e == nullptr || e[N + lane] == 0) muv[lane] = 0.0;
        }
    }
    for (int q = lane; q < (T + 1) * N; q += 64) { wx[q] = 0.0; yx[q] = 0.0; zx[q] = 0.0; }
    for (int q = lane; q < T * M; q += 64) { wu[q] = 0.0; yu[q] = 0.0; zu[q] = 0.0; kk[q] = 0.0; }
    wave_sync();
    double rho = a.rho, hr = 0.5 * rho;              // (ADAPT = false: never written again)
    auto qs = [&](const double* Qm, int i, int j) -> double {
        return (i < NR && j < NR) ? 0.5 * (Qm[i * NR + j] + Qm[j * NR + i]) : 0.0;
    };
    // ---- factorisation (boxqp_factor.inc), the whole horizon ----------------------------
    int bad = 0;
#define BOX_FACTOR_FROM 0
#include "boxqp_factor.inc"
#undef BOX_FACTOR_FROM

    // ---- HBM records: staging through the LDS ring -------------------------------------------
    // record t = L::SP / 2 16-byte chunks; lane l moves chunks l, l + 64, ..  (global_load_dwordx4 into registers;
    // the compiler's vmcnt wait lands at the ds_write_b128 that puts them in the ring, one step after the load)
    constexpr int NC = L::SP / 2, RC = (NC + 63) / 64;
    struct Stage { v2d v[RC]; };
    auto fetch = [&](int t, Stage& st) {
        const gv2d* src = (const gv2d*)(recs + (size_t)t * L::SP);
#pragma unroll
        for (int r = 0; r < RC; ++r)
            if (r * 64 + lane < NC) st.v[r] = src[r * 64 + lane];
    };
    auto put = [&](int t, const Stage& st) {
        v2d* dst = reinterpret_cast<v2d*>(F + (size_t)(t % L::RING) * L::SP);
#pragma unroll
        for (int r = 0; r < RC; ++r)
            if (r * 64 + lane < NC) dst[r * 64 + lane] = st.v[r];
    };
    (void)fetch; (void)put;

    // ---- MPC loop: T tail re-solves, first control applied to the true dynamics ----------
    double xr[NR], ur[M], xn[NR], up[M];
#pragma unroll
    for (int i = 0; i < NR; ++i) xr[i] = a.x0[i];
#pragma unroll
    for (int j = 0; j < M; ++j) up[j] = 0.0;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NR; ++i) a.x_new[i] = xr[i];
    }
    double cost = 0.0;
    auto quad = [&](const double* Wm_, const double* e, int K) -> double {   // e' sym(W) e, K = NR or M
        double s = 0.0;
        for (int i = 0; i < K; ++i)
            for (int j = 0; j < K; ++j) s += e[i] * Wm_[i * K + j] * e[j];
        return s;
    };
    int it_max = 0, n_fail = 0;
    const double al = a.relax;
    int n_factor = 1;                                  // ADAPT: factorisations and ADMM iterations of the launch,
    long long n_iter = 0;                              // reported in ad.out
    int n_lazy = 0, last_lazy = -1;                    // LAZY: activation events, the last tail that had one
    for (int tau = 0; tau < T; ++tau) {
        // the tail problem starts from the realised state; for DU its u_prev block is the
        // realised actuated position x_tau[idx] (tv_lqr.py:99-100 at the tail's local t = 0)
        double ub[M];
#pragma unroll
        for (int j = 0; j < M; ++j) ub[j] = 0.0;
        if constexpr (DU) {
#pragma unroll
            for (int j = 0; j < M; ++j) {
                double v = xr[0];
#pragma unroll
                for (int i = 1; i < NR; ++i) v = (i == Model::u_into_x(j)) ? xr[i] : v;
                ub[j] = v;
            }
        }
        if (lane < N) {
            double v = xr[0];
#pragma unroll
            for (int i = 1; i < NR; ++i) v = (i == lane) ? xr[i] : v;
#pragma unroll
            for (int j = 0; j < M; ++j) v = (NR + j == lane) ? ub[j] : v;
            zx[(size_t)tau * N + lane] = v;
        }
        wave_sync();
        int it = 0;
        bool conv = false;
        int n_refactor = 0;                            // ADAPT: of this tail, at most ad.max_refactor
        while (it < a.max_iter && !conv) {
            ++it;
            // backward affine sweep: p_T = -(Qd xd_T + rho/2 mx (w - y)_T)
            if (lane < N) pv[lane] = -(qxT[lane] + hr * mxv[lane] * (wx[(size_t)T * N + lane] - yx[(size_t)T * N + lane]));
            wave_sync();
            // (HBM: `hook` stages the record two steps ahead into the ring just before the step's last wave_sync)
            auto bw_step = [&](int t, auto hook) {
                const double* rec = HBM ? F + (size_t)(t % L::RING) * L::SP : F + (size_t)t * L::S;
                if (lane < N) gv[lane] = rec[L::oD + lane] + pv[lane];
                else if (lane < N + M) {
                    int j = lane - N;
                    sv[j] = -hr * muv[j] * (wu[(size_t)t * M + j] - yu[(size_t)t * M + j]);
                }
                wave_sync();
                if (lane < N) {                      // p_t
                    double s = -(rec[L::oQx + lane] + hr * mxv[lane] * (wx[(size_t)t * N + lane] - yx[(size_t)t * N + lane]));
                    for (int l = 0; l < N; ++l) s += rec[L::oAcl + l * N + lane] * gv[l];
                    for (int j = 0; j < M; ++j) s += rec[L::oK + j * N + lane] * sv[j];
                    pv[lane] = s;
                } else if (lane < N + M) {           // k_t
                    int j = lane - N;
                    double s = 0.0;
                    for (int l = 0; l < N; ++l) s -= rec[L::oMinv + j * N + l] * gv[l];
                    for (int l = 0; l < M; ++l) s -= rec[L::oHinv + j * M + l] * sv[l];
                    kk[(size_t)t * M + j] = s;
                }
                hook();
                wave_sync();
            };
            // forward sweep on the linear model: u = K x + k, x+ = Acl x + B k + c
            auto fw_step = [&](int t, auto hook) {
                const double* rec = HBM ? F + (size_t)(t % L::RING) * L::SP : F + (size_t)t * L::S;
                const double* xt = zx + (size_t)t * N;
                if (lane < N) {
                    double s = rec[L::oC + lane];
                    for (int l = 0; l < N; ++l) s += rec[L::oAcl + lane * N + l] * xt[l];
                    for (int j = 0; j < M; ++j) s += rec[L::oB + lane * M + j] * kk[(size_t)t * M + j];
                    zx[(size_t)(t + 1) * N + lane] = s;
                } else if (lane < N + M) {
                    int j = lane - N;
                    double s = kk[(size_t)t * M + j];
                    for (int l = 0; l < N; ++l) s += rec[L::oK + j * N + l] * xt[l];
                    zu[(size_t)t * M + j] = s;
                }
                hook();
                wave_sync();
            };
            if constexpr (!HBM) {
                for (int t = T - 1; t >= tau; --t) bw_step(t, [] {});
                for (int t = tau; t < T; ++t) fw_step(t, [] {});
            } else {
                // Ring invariant: a step t of either sweep starts with records t and t -+ 1 (the next one) in their
                // slots t % 3 and (t -+ 1) % 3, and record t -+ 2 in flight into registers; it issues the loads of
                // t -+ 3 and writes t -+ 2 into the slot of t +- 1, which nothing reads any more.  The factorisation
                // leaves T-1 and T-2 in place; a backward sweep ends with tau and tau+1 in place, a forward sweep with
                // T-1 and T-2 -- each what the next sweep starts from.  Two register sets, alternate steps.
                Stage sa, sb;
                if (T - 3 >= tau) fetch(T - 3, sa);
                for (int t = T - 1; t >= tau; t -= 2) {
                    if (t - 3 >= tau) fetch(t - 3, sb);
                    bw_step(t, [&] { if (t - 2 >= tau) put(t - 2, sa); });
                    if (t - 1 < tau) break;
                    if (t - 4 >= tau) fetch(t - 4, sa);
                    bw_step(t - 1, [&] { if (t - 3 >= tau) put(t - 3, sb); });
                }
                if (tau + 2 < T) fetch(tau + 2, sa);
                for (int t = tau; t < T; t += 2) {
                    if (t + 3 < T) fetch(t + 3, sb);
                    fw_step(t, [&] { if (t + 2 < T) put(t + 2, sa); });
                    if (t + 1 >= T) break;
                    if (t + 4 < T) fetch(t + 4, sa);
                    fw_step(t + 1, [&] { if (t + 3 < T) put(t + 3, sb); });
                }
            }
            // projection + dual update (x_tau is fixed: only t > tau), residuals
            double rp = 0.0, rd = 0.0;
            for (int q = (tau + 1) * N + lane; q < (T + 1) * N; q += 64) {
                const int i = q % N, t = q / N;
                if (mxv[i] != 0.0) {
                    const double zr = al * zx[q] + (1.0 - al) * wx[q];
                    const double wn = fmin(fmax(zr + yx[q], zlo_(t, i)), zhi_(t, i));
                    rp = fmax(rp, fabs(zx[q] - wn));
                    rd = fmax(rd, fabs(wn - wx[q]));
                    yx[q] += zr - wn;
                    wx[q] = wn;
                }
            }
            for (int q = tau * M + lane; q < T * M; q += 64) {
                const int j = q % M, t = q / M;
                if (muv[j] != 0.0) {
                    const double zr = al * zu[q] + (1.0 - al) * wu[q];
                    const double wn = fmin(fmax(zr + yu[q], vlo_(t, j)), vhi_(t, j));
                    rp = fmax(rp, fabs(zu[q] - wn));
                    rd = fmax(rd, fabs(wn - wu[q]));
                    yu[q] += zr - wn;
                    wu[q] = wn;
                }
            }
            const double res = wave_max(fmax(rp, rho * rd));
            conv = res < a.eps;
            wave_sync();
            if constexpr (ADAPT) {
                // Residual balancing, every ad.check_every iterations of a tail that has not converged: with the
                // residuals relative to their scales -- zn = max(|z|, |w|), yn = rho max |y| (the multipliers), over
                // the tail's bounded components like rp and rd -- rho <- rho sqrt((rp / zn) / (rd / yn)) (the factor
                // clipped to [1e-2, 1e2]) when that factor leaves [1 / trigger, trigger].  The multipliers rho y
                // stay: y <- y rho_old / rho_new.  The new rho stays for the tails that follow.  All of it uniform.
                if (!conv && it % ad.check_every == 0 && n_refactor < ad.max_refactor) {
                    double zn = 0.0, yn = 0.0;          // (each lane reads back the entries it has just written)
                    for (int q = (tau + 1) * N + lane; q < (T + 1) * N; q += 64)
                        if (mxv[q % N] != 0.0) {
                            zn = fmax(zn, fmax(fabs(zx[q]), fabs(wx[q])));
                            yn = fmax(yn, fabs(yx[q]));
                        }
                    for (int q = tau * M + lane; q < T * M; q += 64)
                        if (muv[q % M] != 0.0) {
                            zn = fmax(zn, fmax(fabs(zu[q]), fabs(wu[q])));
                            yn = fmax(yn, fabs(yu[q]));
                        }
                    zn = wave_max(zn);
                    yn = rho * wave_max(yn);
                    const double rpa = wave_max(rp), rda = rho * wave_max(rd);
                    if (rpa > 0.0 && rda > 0.0 && zn > 0.0 && yn > 0.0) {
                        const double ratio = fmin(fmax(sqrt((rpa / zn) / (rda / yn)), 1e-2), 1e2);
                        if (ratio > ad.trigger || ratio * ad.trigger < 1.0) {
                            const double sc = 1.0 / ratio;
                            rho *= ratio;
                            hr = 0.5 * rho;
                            for (int q = (tau + 1) * N + lane; q < (T + 1) * N; q += 64) yx[q] *= sc;
                            for (int q = tau * M + lane; q < T * M; q += 64) yu[q] *= sc;
                            wave_sync();
                            // HBM: the ring holds records T-1 and T-2 of the old factor (where a forward sweep leaves
                            // them) and no load is in flight; the factorisation builds the new T-1 and T-2 in those
                            // same slots and uses the third, which the next sweep fills before it reads it
#define BOX_FACTOR_FROM tau
#include "boxqp_factor.inc"
#undef BOX_FACTOR_FROM
                            ++n_refactor;
                            ++n_factor;
                        }
                    }
                }
            }
            if constexpr (LAZY) {
                // A converged tail: the dropped components (finite bound, not enforced) against their bounds on the
                // tail's rows of the plan, no tolerance.  The flags go through gv / sv, idle between sweeps; every
                // lane reads the same flags back, so the decision is uniform.
                if (conv) {
                    if (lane < N) gv[lane] = 0.0;
                    else if (lane < N + M) sv[lane - N] = 0.0;
                    wave_sync();
                    for (int q = (tau + 1) * N + lane; q < (T + 1) * N; q += 64) {
                        const int i = q % N, t = q / N;
                        if (fxv[i] != 0.0 && mxv[i] == 0.0 && (zx[q] < zlo_(t, i) || zx[q] > zhi_(t, i))) gv[i] = 1.0;
                    }
                    for (int q = tau * M + lane; q < T * M; q += 64) {
                        const int j = q % M, t = q / M;
                        if (fuv[j] != 0.0 && muv[j] == 0.0 && (zu[q] < vlo_(t, j) || zu[q] > vhi_(t, j))) sv[j] = 1.0;
                    }
                    wave_sync();
                    bool grow = false;
                    for (int i = 0; i < N; ++i) grow = grow || gv[i] != 0.0;
                    for (int j = 0; j < M; ++j) grow = grow || sv[j] != 0.0;
                    if (grow) {
                        // they join the set: w = clip(z), y = 0 on the tail's rows, and a factor with their rho terms
                        for (int q = (tau + 1) * N + lane; q < (T + 1) * N; q += 64) {
                            const int i = q % N, t = q / N;
                            if (gv[i] != 0.0) {
                                wx[q] = fmin(fmax(zx[q], zlo_(t, i)), zhi_(t, i));
                                yx[q] = 0.0;
                            }
                        }
                        for (int q = tau * M + lane; q < T * M; q += 64) {
                            const int j = q % M, t = q / M;
                            if (sv[j] != 0.0) {
                                wu[q] = fmin(fmax(zu[q], vlo_(t, j)), vhi_(t, j));
                                yu[q] = 0.0;
                            }
                        }
                        if (lane < N) { if (gv[lane] != 0.0) mxv[lane] = 1.0; }
                        else if (lane < N + M) { if (sv[lane - N] != 0.0) muv[lane - N] = 1.0; }
                        wave_sync();
                        // HBM: the ring is where a forward sweep leaves it, as for a new rho above
#define BOX_FACTOR_FROM tau
#include "boxqp_factor.inc"
#undef BOX_FACTOR_FROM
                        ++n_factor;
                        ++n_lazy;
                        last_lazy = tau;
                        conv = false;
                    }
                }
            }
        }
        it_max = max(it_max, it);
        if constexpr (ADAPT) n_iter += it;
        n_fail += conv ? 0 : 1;
        if (a.single_tail) {
            // solve_tvlqr's return value: the plan of this one QP (xt_star (T+1,n), ut_star (T,m)) -- the
            // linear-model rollout of the converged iterate; for DU the controls are the u_prev blocks
            for (int q = lane; q < (T + 1) * NR; q += 64) a.x_new[q] = zx[(size_t)(q / NR) * N + q % NR];
            for (int q = lane; q < T * M; q += 64)
                a.u_new[q] = DU ? zx[(size_t)(q / M + 1) * N + NR + q % M] : zu[q];
            if (lane == 0) {
                a.info[0] = bad; a.info[1] = it_max; a.info[2] = n_fail;
            }
            if constexpr (ADAPT) {
                if (lane == 0 && ad.out != nullptr) { ad.out[0] = (double)n_factor; ad.out[1] = rho; ad.out[2] = (double)n_iter; }
            }
            if constexpr (LAZY) {
                int* e = ad.lazy.enforced_io;
                if (e != nullptr && lane < N) e[lane] = mxv[lane] != 0.0 ? 1 : 0;
                if (e != nullptr && lane < M) e[N + lane] = muv[lane] != 0.0 ? 1 : 0;
                if (lane == 0 && ad.lazy.out != nullptr) {
                    ad.lazy.out[0] = (double)n_lazy; ad.lazy.out[1] = (double)last_lazy; ad.lazy.out[2] = (double)n_iter;
                }
            }
            return;
        }
        // first control of the tail solution (clipped), true dynamics step
#pragma unroll
        for (int j = 0; j < M; ++j) {
            double v = fmin(fmax(zu[(size_t)tau * M + j], vlo_(tau, j)), vhi_(tau, j));
            if constexpr (DU) v = fmin(fmax(ub[j] + v, zlo_(tau + 1, NR + j)), zhi_(tau + 1, NR + j));
            ur[j] = v;
        }
        // running cost of the realised trajectory: IrsLqr.evaluate_cost (irs_lqr.py:121-137), or
        // for DU IrsLqrQuasistatic.eval_cost (irs_lqr_quasistatic.py:153-194: R on u_t - u_{t-1})
        {
            double e[NR], dv[M];
#pragma unroll
            for (int i = 0; i < NR; ++i) e[i] = xr[i] - a.xd[(size_t)tau * NR + i];
#pragma unroll
            for (int j = 0; j < M; ++j) dv[j] = DU ? ur[j] - (tau == 0 ? ub[j] : up[j]) : ur[j];
            cost += quad(a.Q, e, NR) + quad(a.R, dv, M);
        }
        Model::template step<double>(a.p, xr, ur, xn);
#pragma unroll
        for (int i = 0; i < NR; ++i) xr[i] = xn[i];
#pragma unroll
        for (int j = 0; j < M; ++j) up[j] = ur[j];
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < M; ++j) a.u_new[(size_t)tau * M + j] = ur[j];
#pragma unroll
            for (int i = 0; i < NR; ++i) a.x_new[(size_t)(tau + 1) * NR + i] = xr[i];
        }
        wave_sync();
    }
    {
        double e[NR];
#pragma unroll
        for (int i = 0; i < NR; ++i) e[i] = xr[i] - a.xd[(size_t)T * NR + i];
        cost += quad(DU ? a.Qd : a.Q, e, NR);       // terminal: Qd (quasistatic :160-168) vs Q (irs_lqr.py:135-136)
    }
    if (lane == 0) {
        a.info[0] = bad; a.info[1] = it_max; a.info[2] = n_fail;
        if (a.cost) a.cost[0] = cost;
    }
    if constexpr (ADAPT) {
        if (lane == 0 && ad.out != nullptr) { ad.out[0] = (double)n_factor; ad.out[1] = rho; ad.out[2] = (double)n_iter; }
    }
    if constexpr (LAZY) {
        int* e = ad.lazy.enforced_io;
        if (e != nullptr && lane < N) e[lane] = mxv[lane] != 0.0 ? 1 : 0;
        if (e != nullptr && lane < M) e[N + lane] = muv[lane] != 0.0 ? 1 : 0;
        if (lane == 0 && ad.lazy.out != nullptr) {
            ad.lazy.out[0] = (double)n_lazy; ad.lazy.out[1] = (double)last_lazy; ad.lazy.out[2] = (double)n_iter;
        }
    }
}

template <class Model, bool DU, bool HBM, bool ADAPT, bool LAZY = false>
int launch_box_kernel(const BoxArgs& a, double* recs, size_t bytes,
                      const std::conditional_t<LAZY, BoxAdaptLazy, BoxAdapt>& ad, hipStream_t st) {
    constexpr auto kern = box_descent_kernel<Model, DU, HBM, ADAPT, LAZY>;
    const int rc = irs_raise_lds_limit<kern>(bytes, "irs_tvlqr_box_descent");
    if (rc != IRS_OK) return rc;
    hipLaunchKernelGGL(kern, dim3(1), dim3(64), bytes, st, a, recs, ad);
    return IRS_OK;
}

// adapt: null = the fixed-rho kernel; lazy: null = every finite bound enforced, else the lazy form (with adapt)
template <class Model, bool DU>
int launch_box(const BoxArgs& a, const BoxPlan& p, double* ws, const BoxAdapt* adapt, const BoxLazy* lazy,
               hipStream_t st) {
    const bool hbm = p.place == BoxPlace::AdmmHbm;
    if (lazy != nullptr) {
        BoxAdaptLazy al;
        static_cast<BoxAdapt&>(al) = *adapt;
        al.lazy = *lazy;
        return hbm ? launch_box_kernel<Model, DU, true, true, true>(a, ws, p.lds, al, st)
                   : launch_box_kernel<Model, DU, false, true, true>(a, nullptr, p.lds, al, st);
    }
    if (adapt == nullptr)
        return hbm ? launch_box_kernel<Model, DU, true, false>(a, ws, p.lds, BoxAdapt{}, st)
                   : launch_box_kernel<Model, DU, false, false>(a, nullptr, p.lds, BoxAdapt{}, st);
    return hbm ? launch_box_kernel<Model, DU, true, true>(a, ws, p.lds, *adapt, st)
               : launch_box_kernel<Model, DU, false, true>(a, nullptr, p.lds, *adapt, st);
}

// Trust-region rows of B problems in one launch (IrsLqrQuasistatic._bounds_dev, irs_lqr_quasistatic.py:303-325): entry
// (b, t, j) of lo / hi (B,T,m) is x_trj[b, t, idx[j]] + offset -- or, rel, the offset alone (bounds on u_t - u_{t-1}) --
// with offsets (B,2,m), or (B,2,T,m) if per_time.  One f64 add per entry: the bits of the host expression.
__global__ __launch_bounds__(256) void bound_rows_batch_kernel(int n, int m, int T, long long total, const double* x_trj,
                                                               const int* idx, const double* off, bool per_time, bool rel,
                                                               double* lo, double* hi) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= total) return;
    const int j = (int)(q % m), t = (int)(q / m % T);
    const long long b = q / m / T;
    const long long side = per_time ? (long long)T * m : m, o = b * 2 * side + (per_time ? (long long)t * m : 0) + j;
    const double c = rel ? 0.0 : x_trj[(b * (T + 1) + t) * n + idx[j]];
    lo[q] = c + off[o];
    hi[q] = c + off[o + side];
}

// The ADMM kernel: its records on chip when they fit LDS and no workspace is forced on them; otherwise in HBM,
// where only the ADMM vectors stay in LDS (hbm_doubles grows by 3 N + 4 M per step: that caps the horizon).
template <int N, int M>
BoxPlan admm_plan(int T, BoxWs ws) {
    using L = BoxLayout<N, M>;
    const size_t lds = L::doubles(T) * sizeof(double), hbm = L::hbm_doubles(T) * sizeof(double);
    const int max_T = (int)((IRS_LDS_BUDGET / sizeof(double) - L::hbm_doubles(0)) / (3 * N + 4 * M));
    if (ws == BoxWs::Always || (ws == BoxWs::IfNeeded && lds > IRS_LDS_BUDGET))
        return {hbm <= IRS_LDS_BUDGET ? BoxPlace::AdmmHbm : BoxPlace::None, hbm, L::record_bytes(T), max_T};
    if (lds <= IRS_LDS_BUDGET) return {BoxPlace::AdmmLds, lds, 0, max_T};
    return {BoxPlace::None, lds, L::record_bytes(T), max_T};
}

}  // namespace

// the plain (du = false) or position-controlled ADMM form of `model`; *p is left alone when it has no such form
static int admm_plan_of(int model, int T, bool du, BoxWs ws, BoxPlan* p) {
    IRS_DISPATCH_MODEL(model, {
        if (!du) *p = admm_plan<Model::NX, Model::NU>(T, ws);
        else if constexpr (has_u_into_x<Model>::value) *p = admm_plan<Model::NX + Model::NU, Model::NU>(T, ws);
    });
    return IRS_OK;
}

BoxPlan irs_box_plan(int model, int T, int kind, BoxWs ws) {
    BoxPlan p{BoxPlace::None, 0, 0, 0};
    if (irs_model_info(model, nullptr, nullptr, nullptr) != IRS_OK) return p;
    if (kind == IRS_BOX_ADMM || kind == IRS_BOX_ADMM_DU) {
        admm_plan_of(model, T, kind == IRS_BOX_ADMM_DU, ws, &p);
    } else if (kind == IRS_BOX_ACTIVE_SET) {
        // everything in LDS; the layout grows by the same record every step
        const size_t lds = irs_ctrlbox_lds_bytes(model, T), base = irs_ctrlbox_lds_bytes(model, 0);
        if (lds > 0)
            p = {lds <= IRS_LDS_BUDGET ? BoxPlace::Lanes : BoxPlace::None, lds, 0,
                 (int)((IRS_LDS_BUDGET - base) / (irs_ctrlbox_lds_bytes(model, 1) - base))};
    } else if (kind == IRS_BOX_ACTIVE_SET_MFMA) {
        // the records on chip while they fit, else in the workspace: no horizon cap
        const size_t lds = irs_ctrlbox_mfma_lds_bytes(model, T), rec = irs_ctrlbox_mfma_record_bytes(model, T);
        if (lds > 0 && ws == BoxWs::Always) p = {BoxPlace::TilesHbm, lds - rec, rec, INT_MAX};
        else if (lds > 0 && lds <= IRS_LDS_BUDGET) p = {BoxPlace::TilesLds, lds, 0, INT_MAX};
        else if (lds > 0 && ws != BoxWs::None) p = {BoxPlace::TilesHbm, lds - rec, rec, INT_MAX};
        else if (lds > 0) p = {BoxPlace::None, lds, rec, INT_MAX};
    }
    return p;
}

// The ADMM kernel on a filled BoxArgs, where the plan puts it: records on chip, or in `ws` -- whenever one is given
// (policy Always), or only where they do not fit LDS (IfNeeded).  du: the position-controlled form.
int irs_box_admm_launch(const char* fn, int model, bool du, const BoxArgs& a, void* ws, size_t ws_bytes, BoxWs policy,
                        hipStream_t st, const BoxAdapt* adapt, const BoxLazy* lazy) {
    const BoxPlan p = irs_box_plan(model, a.T, du ? IRS_BOX_ADMM_DU : IRS_BOX_ADMM,
                                   ws == nullptr ? BoxWs::None : policy);
    if (p.max_T == 0) {
        irs_set_error("%s: model %d is not position controlled", fn, model);
        return IRS_ERR_UNSUPPORTED;
    }
    if (p.place == BoxPlace::None) {
        if (ws == nullptr)
            irs_set_error("irs_tvlqr_box_descent: horizon T=%d needs %zu bytes of LDS (max ~160 KB) with its records on "
                          "chip; give a workspace of %zu bytes (T <= %d)", a.T, p.lds, p.records, p.max_T);
        else
            irs_set_error("irs_tvlqr_box_descent: horizon T=%d is beyond the bounded TV-LQR kernel's limit T <= %d with "
                          "its records in HBM (its ADMM vectors need %zu bytes of LDS, max ~160 KB)", a.T, p.max_T, p.lds);
        return IRS_ERR_UNSUPPORTED;
    }
    if (p.place == BoxPlace::AdmmHbm) {
        const WsFit f = ws_fit(p, 1, ws, ws_bytes);
        if (f.small) {
            irs_set_error("irs_tvlqr_box_descent: workspace %zu < %zu bytes", ws_bytes, f.need);
            return IRS_ERR_WORKSPACE;
        }
        if (f.misaligned) {
            irs_set_error("irs_tvlqr_box_descent: the workspace must be 256-byte aligned");
            return IRS_ERR_INVALID_ARG;
        }
    }
    double* recs = static_cast<double*>(ws);
    int rc = IRS_ERR_UNSUPPORTED;
    if (!du) {
        IRS_DISPATCH_MODEL(model, { rc = launch_box<Model, false>(a, p, recs, adapt, lazy, st); });
    } else {
        IRS_DISPATCH_MODEL(model, {
            if constexpr (has_u_into_x<Model>::value) rc = launch_box<Model, true>(a, p, recs, adapt, lazy, st);
        });
    }
    if (rc != IRS_OK) return rc;
    IRS_CHECK_LAUNCH();
    return IRS_OK;
}

extern "C" {

int irs_quasistatic_bound_rows_batch(int n, int m, int T, int B, const double* x_trj, const int* indices_u_into_x,
                                     const double* offsets, int per_time, int rel, double* lo, double* hi,
                                     void* stream) {
    IRS_CHECK_ARG(n > 0 && m > 0 && T > 0 && B > 0, "n, m, T and B must be positive");
    IRS_CHECK_ARG(offsets && lo && hi && (rel || (x_trj && indices_u_into_x)), "bad argument");
    const long long total = (long long)B * T * m;
    IRS_CHECK_ARG(total <= 0x7fffffffLL * 256, "too many rows for one launch");
    hipLaunchKernelGGL(bound_rows_batch_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       static_cast<hipStream_t>(stream), n, m, T, total, x_trj, indices_u_into_x, offsets, per_time != 0,
                       rel != 0, lo, hi);
    IRS_CHECK_LAUNCH();
    return IRS_OK;
}

}  // extern "C"
