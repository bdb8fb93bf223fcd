// box_descent_kernel, the ADMM kernel of the bounded TV-LQR (the method: boxqp.hip's header), and its LDS layout:
// included by boxqp.hip (one problem, one workgroup) and, with IRS_BOX_KERNEL_BATCH defined, by boxqp_batch.hip (B
// problems, grid B).  Two translation units rather than a shared __device__ body under two __global__ wrappers: that
// form was tried first and moved the compiled code of 108 of boxqp.hip's 109 single-problem kernels; with the separate
// unit boxqp.hip preprocesses to the text it had, and its kernels stay the code they were (DESIGN.md 7.1).
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
//
// IRS_BOX_KERNEL_BATCH (boxqp_batch.hip): B problems of the plain fixed-penalty form, grid B, workgroup b on problem b.
// Every per-problem array of `a` is then B contiguous blocks -- At, Bt, ct, xd, x0, x_new, u_new, cost (B), info (B,3),
// the constant bound rows xlo, xhi (B,n), ulo, uhi (B,m), run_flag (B) -- and problem b's records are at
// recs + b * rec_stride doubles; Q, Qd, R, the model's constants and the scalars are shared.  The pointers move to
// problem b, and from there on the kernel is the single one: a workgroup whose run_flag[b] is 0 returns in the next
// statement, before anything of problem b is read or written.
template <class Model, bool DU, bool HBM, bool ADAPT, bool LAZY = false>
#ifdef IRS_BOX_KERNEL_BATCH
__global__ __launch_bounds__(64) void box_descent_kernel(BoxArgs a, double* recs,
                                                         std::conditional_t<LAZY, BoxAdaptLazy, BoxAdapt> ad,
                                                         size_t rec_stride) {
    static_assert(!DU && !ADAPT && !LAZY, "the batch runs the plain fixed-penalty form");
    {
        constexpr size_t n = Model::NX, m = Model::NU;
        const size_t b = blockIdx.x, T = (size_t)a.T;
        a.At += b * T * n * n; a.Bt += b * T * n * m; a.ct += b * T * n; a.xd += b * (T + 1) * n; a.x0 += b * n;
        a.xlo += b * n; a.xhi += b * n; a.ulo += b * m; a.uhi += b * m;
        a.x_new += b * (T + 1) * n; a.u_new += b * T * m; a.info += b * 3;
        if (a.cost != nullptr) a.cost += b;
        if (a.run_flag != nullptr) a.run_flag += b;
        if (HBM) recs += b * rec_stride;
    }
#else
__global__ __launch_bounds__(64) void box_descent_kernel(BoxArgs a, double* recs,
                                                         std::conditional_t<LAZY, BoxAdaptLazy, BoxAdapt> ad) {
#endif
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
        // A tail whose first control is not finite has not converged, whatever the residuals say: fmin / fmax drop a
        // NaN, so the projection of a poisoned plan lands on a bound and both residuals can read zero.  A NaN or Inf in
        // the data of steps >= tau reaches this control through the backward sweep.  (Bit test, wave.hpp; every lane
        // reads the same M values.)
        {
            unsigned nf = 0;
#pragma unroll
            for (int j = 0; j < M; ++j) nf = max(nf, expo_bits(zu[(size_t)tau * M + j]));
            if (nf == kExpoOnes) conv = false;
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
        // pivots fine but the realised cost not finite (it sums over every x_t, u_t and xd_t): T + 1, "no such step"
        a.info[0] = bad != 0 ? bad : (nonfinite_bits(cost) ? T + 1 : 0);
        a.info[1] = it_max; a.info[2] = n_fail;
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
