// Box-constrained TV-LQR for ANY size 1 <= n <= 32, 1 <= m <= 16, resumable from tail to tail: the method of boxqp.hip
// (ADMM on the box around one Riccati factorisation, w <- clip(a z + (1-a) w + y), only components with a finite bound
// at any time carry the rho term; oracle/irs_oracle.py: tvlqr_box_factor / tvlqr_box_solve / local_descent_box) for a
// system WITHOUT a device functor.  boxqp.hip is compiled per Model and keeps the plant step inside its launch; a
// torch callable cannot run there.  Here the MPC loop of IrsLqr.local_descent (irs_lqr/irs_lqr.py:169-184) is split at
// the plant: the state of the T tail re-solves lives in a workspace in HBM, and the caller's plant runs between
// launches on the same stream.  The launch boundary is the hand-off: nothing waits on the host or on another stream.
//
//   box_values_begin_kernel   one wave, once per descent: the backward factorisation of the whole horizon.  Writes to
//     the workspace one record per step (Acl, K, Minv, Hinv, B, c, d, qx: box_rec_layout of the runtime
//     (n, m), boxqp.hip's own record), the masks (over the rows 1..T of x and 0..T-1 of u), Qd xd_T, zeroed warm-start vectors, and -- last --
//     the header (begun mark, n, m, T, rho, relax).  info = [t+1 of a non-PD Hessian, 0, 0].
//   box_values_tail_kernel<RC>   one wave, once per tail t: the tail QP t..T from the realised state x_t, warm started
//     from the workspace.  Its ADMM vectors are in LDS while it runs; the records are staged from HBM through a 3-slot
//     LDS ring two steps ahead of use, as the HBM = true path of boxqp.hip does (RC: 16-byte chunks per lane of one
//     record, the width of the two register sets in flight -- the sizes themselves are runtime values and every
//     matrix-vector product a loop).  Writes the warm start back, the clipped first control, the tail's plan if asked,
//     info[1] = max, info[2] += "stopped at max_iter".  A workspace whose header does not match (n, m, T, begun) makes
//     it write info[0] = -1 and return: it never walks records it did not write.
//
// What the workspace keeps between tails is the warm start (w, y): z and k are recomputed from x_t by the first
// iteration of every tail, so they stay in LDS.  One block owns the workspace: plain stores, no atomics.
#include "boxqp_layout.hpp"
#include "irs_common.hpp"
#include "wave.hpp"

namespace {

constexpr int kMaxN = 32, kMaxM = 16;       // the limits of irs_tvlqr_riccati and the values pass
constexpr int kHdr = 8;                     // header doubles: begun, n, m, T, rho, relax, 0, 0
constexpr double kBegun = 4952534258564131.0;
constexpr double INF = __builtin_huge_val();

typedef double v2d __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) v2d gv2d;          // global, not flat: see boxqp.hip
typedef __attribute__((address_space(1))) double gdbl;

// the workspace, in doubles: header | mx (32) | mu (16) | Qd xd_T (32) | wx, yx (T+1,n), wu, yu (T,m) | T records
struct Ws {
    size_t oMx, oMu, oQxT, oWx, oYx, oWu, oYu, oRec, total;
};
__host__ __device__ inline Ws ws_layout(int n, int m, int T) {
    Ws w;
    w.oMx = kHdr; w.oMu = w.oMx + kMaxN; w.oQxT = w.oMu + kMaxM; w.oWx = w.oQxT + kMaxN;
    w.oYx = w.oWx + (size_t)(T + 1) * n; w.oWu = w.oYx + (size_t)(T + 1) * n; w.oYu = w.oWu + (size_t)T * m;
    w.oRec = (w.oYu + (size_t)T * m + 1) / 2 * 2;
    w.total = w.oRec + (size_t)T * box_rec_layout(n, m).SP;
    return w;
}

// LDS doubles of a tail launch: the ring | qxT, p, g, mx (n each) | s, mu (m each) | wx, yx, zx (T+1,n) | wu, yu, zu, k
__host__ __device__ inline size_t tail_lds_doubles(int n, int m, int T) {
    return (size_t)kBoxRing * box_rec_layout(n, m).SP + 4 * n + 2 * m + 3 * (size_t)(T + 1) * n + 4 * (size_t)T * m;
}

// The one planner: what the size queries answer and what the launch path reads.  No HIP calls.
struct ValuesBoxPlan {
    int rc;             // 16-byte chunks per lane of one record
    size_t lds;         // dynamic LDS bytes of a tail launch
    size_t ws;          // workspace bytes
    int max_T;          // the longest horizon whose ADMM vectors fit LDS beside the ring
};
ValuesBoxPlan values_box_plan(int n, int m, int T) {
    const BoxRec r = box_rec_layout(n, m);
    const size_t budget = IRS_LDS_BUDGET / sizeof(double), base = tail_lds_doubles(n, m, 0);
    ValuesBoxPlan p;
    p.rc = (r.SP / 2 + 63) / 64;
    p.lds = tail_lds_doubles(n, m, T) * sizeof(double);
    p.ws = (ws_layout(n, m, T).total * sizeof(double) + 255) / 256 * 256;
    p.max_T = (int)((budget - base) / (size_t)(3 * n + 4 * m));
    return p;
}

struct BeginArgs {
    const double *At, *Bt, *ct, *Q, *Qd, *R, *xd;
    const double *xlo, *xhi, *ulo, *uhi;    // null = none; row t at ptr + t * stride (stride 0 = one row)
    int sx, su;
    double alpha, rho, relax;
    double* ws;
    int* info;
    int n, m, T;
};

__global__ __launch_bounds__(64) void box_values_begin_kernel(BeginArgs a) {
    __shared__ __attribute__((aligned(16))) double rec[kMaxN * kMaxN + 3 * kMaxM * kMaxN + kMaxM * kMaxM + 3 * kMaxN];
    __shared__ double P[kMaxN * kMaxN], Am[kMaxN * kMaxN], Wm[kMaxN * kMaxN], PB[kMaxN * kMaxM];
    __shared__ double Hs[kMaxM * kMaxM], Lm[kMaxM * kMaxM], Yw[kMaxM * kMaxM], Dg[kMaxM], Di[kMaxM];
    __shared__ double mxv[kMaxN], muv[kMaxM];
    const int n = a.n, m = a.m, T = a.T, lane = threadIdx.x;
    const BoxRec L = box_rec_layout(n, m);
    const Ws W = ws_layout(n, m, T);
    gdbl* ws = (gdbl*)a.ws;
    if (lane == 0) ws[0] = 0.0;                       // not begun until the header is written, last
    // masks: a finite bound at any time (x: rows 1..T, x_0 is data)
    if (lane < n) {
        bool any = false;
        for (int t = 1; t <= T; ++t) {
            const double lo = a.xlo ? a.xlo[(size_t)t * a.sx + lane] : -INF, hi = a.xhi ? a.xhi[(size_t)t * a.sx + lane] : INF;
            any = any || isfinite(lo) || isfinite(hi);
        }
        mxv[lane] = any ? 1.0 : 0.0;
        ws[W.oMx + lane] = mxv[lane];
    }
    if (lane < m) {
        bool any = false;
        for (int t = 0; t < T; ++t) {
            const double lo = a.ulo ? a.ulo[(size_t)t * a.su + lane] : -INF, hi = a.uhi ? a.uhi[(size_t)t * a.su + lane] : INF;
            any = any || isfinite(lo) || isfinite(hi);
        }
        muv[lane] = any ? 1.0 : 0.0;
        ws[W.oMu + lane] = muv[lane];
    }
    for (size_t q = W.oWx + lane; q < W.oRec; q += 64) ws[q] = 0.0;          // wx, yx, wu, yu (and the pad)
    wave_sync();
    const double hr = 0.5 * a.rho;
    auto qs = [&](const double* Qm, int i, int j) -> double { return 0.5 * (Qm[i * n + j] + Qm[j * n + i]); };
    int bad = 0;
    unsigned nf = 0;                                  // exponent bits of what this lane stores for the tails (wave.hpp)
    // P_T = Qd + rho/2 Mx ; qx_T = Qd xd_T
    for (int q = lane; q < n * n; q += 64) {
        const int i = q / n, j = q % n;
        P[q] = qs(a.Qd, i, j) + (i == j ? hr * mxv[i] : 0.0);
    }
    if (lane < n) {
        double s = 0.0;
        for (int j = 0; j < n; ++j) s += qs(a.Qd, lane, j) * a.xd[(size_t)T * n + j];
        ws[W.oQxT + lane] = s;
        nf = max(nf, expo_bits(s));
    }
    wave_sync();
    // ---- backward Riccati with Q^ = Q + rho/2 Mx, R^ = alpha R + rho/2 Mu (boxqp_factor.inc, runtime sizes) ----
    for (int t = T - 1; t >= 0; --t) {
        for (int q = lane; q < n * n; q += 64) Am[q] = a.At[(size_t)t * n * n + q];
        for (int q = lane; q < n * m; q += 64) rec[L.oB + q] = a.Bt[(size_t)t * n * m + q];
        if (lane < n) {
            rec[L.oC + lane] = a.ct[(size_t)t * n + lane];
            double s = 0.0;
            for (int j = 0; j < n; ++j) s += qs(a.Q, lane, j) * a.xd[(size_t)t * n + j];
            rec[L.oQx + lane] = s;
        }
        if (lane == 0 && L.SP != L.S) rec[L.S] = 0.0;
        wave_sync();
        const double* B = rec + L.oB;
        // PB = P B ; d = P c
        for (int q = lane; q < n * m; q += 64) {
            const int i = q / m, j = q % m;
            double s = 0.0;
            for (int l = 0; l < n; ++l) s += P[i * n + l] * B[l * m + j];
            PB[q] = s;
        }
        if (lane < n) {
            double s = 0.0;
            for (int l = 0; l < n; ++l) s += P[lane * n + l] * rec[L.oC + l];
            rec[L.oD + lane] = s;
        }
        wave_sync();
        // H = R^ + B'PB
        for (int q = lane; q < m * m; q += 64) {
            const int i = q / m, j = q % m;
            double s = 0.5 * a.alpha * (a.R[i * m + j] + a.R[j * m + i]) + (i == j ? hr * muv[i] : 0.0);
            for (int l = 0; l < n; ++l) s += B[l * m + i] * PB[l * m + j];
            Hs[q] = s;
        }
        wave_sync();
        // H = L D L' in LDS, a column per step: every lane forms the pivot, lane i > j the entry (i, j)
        for (int j = 0; j < m; ++j) {
            double dj = Hs[j * m + j];
            for (int l = 0; l < j; ++l) dj -= Lm[j * m + l] * Lm[j * m + l] * Dg[l];
            if (!(dj > 0.0) && bad == 0) bad = t + 1;
            const double dinv = 1.0 / dj;
            wave_sync();                              // every lane holds the pivot before Dg[j] is written
            if (lane == 0) { Dg[j] = dj; Di[j] = dinv; }
            if (lane > j && lane < m) {
                double s = Hs[lane * m + j];
                for (int l = 0; l < j; ++l) s -= Lm[lane * m + l] * Lm[j * m + l] * Dg[l];
                Lm[lane * m + j] = s * dinv;
            }
            wave_sync();
        }
        // H^-1: lane j < m solves L D L' y = e_j in its own column of Yw
        if (lane < m) {
            for (int i = 0; i < m; ++i) {
                double s = (i == lane) ? 1.0 : 0.0;
                for (int l = 0; l < i; ++l) s -= Lm[i * m + l] * Yw[l * m + lane];
                Yw[i * m + lane] = s;
            }
            for (int i = m - 1; i >= 0; --i) {
                double s = Yw[i * m + lane] * Di[i];
                for (int l = i + 1; l < m; ++l) s -= Lm[l * m + i] * Yw[l * m + lane];
                Yw[i * m + lane] = s;
            }
            for (int i = 0; i < m; ++i) rec[L.oHinv + i * m + lane] = Yw[i * m + lane];
        }
        wave_sync();
        // Minv = H^-1 B' (m x n) ; W = P A
        for (int q = lane; q < m * n; q += 64) {
            const int i = q / n, j = q % n;
            double s = 0.0;
            for (int l = 0; l < m; ++l) s += rec[L.oHinv + i * m + l] * B[j * m + l];
            rec[L.oMinv + q] = s;
        }
        for (int q = lane; q < n * n; q += 64) {
            const int i = q / n, j = q % n;
            double s = 0.0;
            for (int l = 0; l < n; ++l) s += P[i * n + l] * Am[l * n + j];
            Wm[q] = s;
        }
        wave_sync();
        // K = -Minv W
        for (int q = lane; q < m * n; q += 64) {
            const int i = q / n, j = q % n;
            double s = 0.0;
            for (int l = 0; l < n; ++l) s -= rec[L.oMinv + i * n + l] * Wm[l * n + j];
            rec[L.oK + q] = s;
        }
        wave_sync();
        // Acl = A + B K
        for (int q = lane; q < n * n; q += 64) {
            const int i = q / n, j = q % n;
            double s = Am[q];
            for (int l = 0; l < m; ++l) s += B[i * m + l] * rec[L.oK + l * n + j];
            rec[L.oAcl + q] = s;
        }
        wave_sync();
        // P <- Q^ + sym(W' Acl)
        double pn[kMaxN * kMaxN / 64];
#pragma unroll
        for (int r = 0; r < kMaxN * kMaxN / 64; ++r) {
            const int q = lane + 64 * r;
            pn[r] = 0.0;
            if (q < n * n) {
                const int i = q / n, j = q % n;
                double s = 0.0, s2 = 0.0;
                for (int l = 0; l < n; ++l) {
                    s += Wm[l * n + i] * rec[L.oAcl + l * n + j];
                    s2 += Wm[l * n + j] * rec[L.oAcl + l * n + i];
                }
                pn[r] = qs(a.Q, i, j) + (i == j ? hr * mxv[i] : 0.0) + 0.5 * (s + s2);
            }
        }
        wave_sync();
#pragma unroll
        for (int r = 0; r < kMaxN * kMaxN / 64; ++r) {
            const int q = lane + 64 * r;
            if (q < n * n) P[q] = pn[r];
        }
        {                                             // the finished record, once, to the workspace
            const v2d* src = reinterpret_cast<const v2d*>(rec);
            gv2d* dst = (gv2d*)(a.ws + W.oRec + (size_t)t * L.SP);
            for (int c = lane; c < L.SP / 2; c += 64) {
                const v2d v = src[c];
                dst[c] = v;
                nf = max(nf, max(expo_bits(v[0]), expo_bits(v[1])));
            }
        }
        wave_sync();
    }
    // pivots fine but a record entry not finite (c_t and xd_t reach d_t and Q xd_t, never a pivot): T + 1
    const bool nfw = __any(nf == kExpoOnes);
    if (lane == 0) {
        ws[1] = (double)n; ws[2] = (double)m; ws[3] = (double)T; ws[4] = a.rho; ws[5] = a.relax; ws[6] = 0.0; ws[7] = 0.0;
        ws[0] = kBegun;
        a.info[0] = bad != 0 ? bad : (nfw ? T + 1 : 0); a.info[1] = 0; a.info[2] = 0;
    }
}

struct TailArgs {
    const double *xlo, *xhi, *ulo, *uhi;
    int sx, su;
    const double* x_t;
    double *u_t, *x_plan, *u_plan;          // the plans may be null
    double* ws;
    int* info;
    double eps;
    int n, m, T, t, max_iter;
};

template <int RC>
__global__ __launch_bounds__(64) void box_values_tail_kernel(TailArgs a) {
    const int n = a.n, m = a.m, T = a.T, tau = a.t, lane = threadIdx.x;
    const gdbl* hdr = (const gdbl*)a.ws;
    if (!(hdr[0] == kBegun && hdr[1] == (double)n && hdr[2] == (double)m && hdr[3] == (double)T)) {   // uniform
        if (lane == 0) a.info[0] = -1;
        return;
    }
    const double rho = hdr[4], al = hdr[5], hr = 0.5 * rho;
    const BoxRec L = box_rec_layout(n, m);
    const Ws W = ws_layout(n, m, T);
    gdbl* ws = (gdbl*)a.ws;
    auto zlo_ = [&](int t, int i) -> double { return a.xlo ? a.xlo[(size_t)t * a.sx + i] : -INF; };
    auto zhi_ = [&](int t, int i) -> double { return a.xhi ? a.xhi[(size_t)t * a.sx + i] : INF; };
    auto vlo_ = [&](int t, int j) -> double { return a.ulo ? a.ulo[(size_t)t * a.su + j] : -INF; };
    auto vhi_ = [&](int t, int j) -> double { return a.uhi ? a.uhi[(size_t)t * a.su + j] : INF; };
    extern __shared__ __attribute__((aligned(16))) double lds[];
    double* F = lds;                                   // the ring: 3 x L.SP
    double* qxT = F + (size_t)kBoxRing * L.SP;
    double* pv = qxT + n;
    double* gv = pv + n;
    double* mxv = gv + n;
    double* sv = mxv + n;
    double* muv = sv + m;
    double* wx = muv + m;                              // (T+1, n)
    double* yx = wx + (size_t)(T + 1) * n;
    double* zx = yx + (size_t)(T + 1) * n;
    double* wu = zx + (size_t)(T + 1) * n;             // (T, m)
    double* yu = wu + (size_t)T * m;
    double* zu = yu + (size_t)T * m;
    double* kk = zu + (size_t)T * m;

    // ---- the warm start and the constants of the descent, from the workspace ----
    if (lane < n) {
        qxT[lane] = ws[W.oQxT + lane];
        mxv[lane] = ws[W.oMx + lane];
        zx[(size_t)tau * n + lane] = a.x_t[lane];
    } else if (lane < n + m) {
        muv[lane - n] = ws[W.oMu + lane - n];
    }
    for (int q = tau * n + lane; q < (T + 1) * n; q += 64) { wx[q] = ws[W.oWx + q]; yx[q] = ws[W.oYx + q]; }
    for (int q = tau * m + lane; q < T * m; q += 64) { wu[q] = ws[W.oWu + q]; yu[q] = ws[W.oYu + q]; }

    // ---- records: staging through the LDS ring (boxqp.hip, HBM = true) ----
    const int NC = L.SP / 2;
    struct Stage { v2d v[RC]; };
    auto fetch = [&](int t, Stage& st) {
        const gv2d* src = (const gv2d*)(a.ws + W.oRec + (size_t)t * L.SP);
#pragma unroll
        for (int r = 0; r < RC; ++r)
            if (r * 64 + lane < NC) st.v[r] = src[r * 64 + lane];
    };
    auto put = [&](int t, const Stage& st) {
        v2d* dst = reinterpret_cast<v2d*>(F + (size_t)(t % kBoxRing) * L.SP);
#pragma unroll
        for (int r = 0; r < RC; ++r)
            if (r * 64 + lane < NC) dst[r * 64 + lane] = st.v[r];
    };
    Stage sa, sb;
    // what the factorisation leaves in place in boxqp.hip: records T-1 and T-2, where the first sweep reads them
    fetch(T - 1, sa);
    if (T - 2 >= tau) fetch(T - 2, sb);
    put(T - 1, sa);
    if (T - 2 >= tau) put(T - 2, sb);
    wave_sync();

    int it = 0;
    bool conv = false;
    while (it < a.max_iter && !conv) {
        ++it;
        // backward affine sweep: p_T = -(Qd xd_T + rho/2 mx (w - y)_T)
        if (lane < n) pv[lane] = -(qxT[lane] + hr * mxv[lane] * (wx[(size_t)T * n + lane] - yx[(size_t)T * n + lane]));
        wave_sync();
        auto bw_step = [&](int t, auto hook) {
            const double* rec = F + (size_t)(t % kBoxRing) * L.SP;
            if (lane < n) gv[lane] = rec[L.oD + lane] + pv[lane];
            else if (lane < n + m) {
                const int j = lane - n;
                sv[j] = -hr * muv[j] * (wu[(size_t)t * m + j] - yu[(size_t)t * m + j]);
            }
            wave_sync();
            if (lane < n) {                      // p_t
                double s = -(rec[L.oQx + lane] + hr * mxv[lane] * (wx[(size_t)t * n + lane] - yx[(size_t)t * n + lane]));
#pragma unroll 8
                for (int l = 0; l < n; ++l) s += rec[L.oAcl + l * n + lane] * gv[l];
#pragma unroll 8
                for (int j = 0; j < m; ++j) s += rec[L.oK + j * n + lane] * sv[j];
                pv[lane] = s;
            } else if (lane < n + m) {           // k_t
                const int j = lane - n;
                double s = 0.0;
#pragma unroll 8
                for (int l = 0; l < n; ++l) s -= rec[L.oMinv + j * n + l] * gv[l];
#pragma unroll 8
                for (int l = 0; l < m; ++l) s -= rec[L.oHinv + j * m + l] * sv[l];
                kk[(size_t)t * m + j] = s;
            }
            hook();
            wave_sync();
        };
        // forward sweep on the linear model: u = K x + k, x+ = Acl x + B k + c
        auto fw_step = [&](int t, auto hook) {
            const double* rec = F + (size_t)(t % kBoxRing) * L.SP;
            const double* xt = zx + (size_t)t * n;
            if (lane < n) {
                double s = rec[L.oC + lane];
#pragma unroll 8
                for (int l = 0; l < n; ++l) s += rec[L.oAcl + lane * n + l] * xt[l];
#pragma unroll 8
                for (int j = 0; j < m; ++j) s += rec[L.oB + lane * m + j] * kk[(size_t)t * m + j];
                zx[(size_t)(t + 1) * n + lane] = s;
            } else if (lane < n + m) {
                const int j = lane - n;
                double s = kk[(size_t)t * m + j];
#pragma unroll 8
                for (int l = 0; l < n; ++l) s += rec[L.oK + j * n + l] * xt[l];
                zu[(size_t)t * m + j] = s;
            }
            hook();
            wave_sync();
        };
        // Ring invariant (boxqp.hip): a step t of either sweep starts with records t and t -+ 1 in their slots and
        // t -+ 2 in flight into registers; it issues the loads of t -+ 3 and writes t -+ 2 into the slot of t +- 1.
        // A backward sweep ends with tau and tau+1 in place, a forward sweep with T-1 and T-2.
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
        // projection + dual update (x_tau is fixed: only t > tau), residuals
        double rp = 0.0, rd = 0.0;
        for (int q = (tau + 1) * n + lane; q < (T + 1) * n; q += 64) {
            const int i = q % n, t = q / n;
            if (mxv[i] != 0.0) {
                const double zr = al * zx[q] + (1.0 - al) * wx[q];
                const double wn = fmin(fmax(zr + yx[q], zlo_(t, i)), zhi_(t, i));
                rp = fmax(rp, fabs(zx[q] - wn));
                rd = fmax(rd, fabs(wn - wx[q]));
                yx[q] += zr - wn;
                wx[q] = wn;
            }
        }
        for (int q = tau * m + lane; q < T * m; q += 64) {
            const int j = q % m, t = q / m;
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
    }
    // ---- the warm start of the next tail, the first control (clipped), the plan ----
    for (int q = (tau + 1) * n + lane; q < (T + 1) * n; q += 64) { ws[W.oWx + q] = wx[q]; ws[W.oYx + q] = yx[q]; }
    for (int q = tau * m + lane; q < T * m; q += 64) { ws[W.oWu + q] = wu[q]; ws[W.oYu + q] = yu[q]; }
    if (lane < m) a.u_t[lane] = fmin(fmax(zu[(size_t)tau * m + lane], vlo_(tau, lane)), vhi_(tau, lane));
    if (a.x_plan != nullptr)
        for (int q = lane; q < (T + 1 - tau) * n; q += 64) a.x_plan[q] = zx[(size_t)tau * n + q];
    if (a.u_plan != nullptr)
        for (int q = lane; q < (T - tau) * m; q += 64) a.u_plan[q] = zu[(size_t)tau * m + q];
    // a first control that is not finite: the tail has not converged, whatever the residuals say (fmin / fmax drop a
    // NaN, so a poisoned plan projects onto a bound and both residuals can read zero); bit test, wave.hpp
    const bool nfw = __any(lane < m && nonfinite_bits(zu[(size_t)tau * m + (lane < m ? lane : 0)]));
    if (nfw) conv = false;
    if (lane == 0) {
        a.info[1] = max(a.info[1], it);
        a.info[2] += conv ? 0 : 1;
    }
}

template <int RC>
int launch_tail_rc(const TailArgs& a, size_t lds, hipStream_t st) {
    constexpr auto kern = box_values_tail_kernel<RC>;
    const int rc = irs_raise_lds_limit<kern>(lds, "irs_box_values_tail");
    if (rc != IRS_OK) return rc;
    hipLaunchKernelGGL(kern, dim3(1), dim3(64), lds, st, a);
    return IRS_OK;
}

// the staging width: the smallest compiled class that holds a record's chunks per lane (at most 23: (32, 16))
int launch_tail(const TailArgs& a, const ValuesBoxPlan& p, hipStream_t st) {
    if (p.rc <= 1) return launch_tail_rc<1>(a, p.lds, st);
    if (p.rc <= 2) return launch_tail_rc<2>(a, p.lds, st);
    if (p.rc <= 4) return launch_tail_rc<4>(a, p.lds, st);
    if (p.rc <= 8) return launch_tail_rc<8>(a, p.lds, st);
    if (p.rc <= 16) return launch_tail_rc<16>(a, p.lds, st);
    return launch_tail_rc<23>(a, p.lds, st);
}

bool sizes_ok(int n, int m) { return n >= 1 && n <= kMaxN && m >= 1 && m <= kMaxM; }

// The argument checks both entries share; nothing here calls HIP.
int check_call(const char* fn, const irs_box_values_call* c) {
    if (c == nullptr) { irs_set_error("%s: call must not be NULL", fn); return IRS_ERR_INVALID_ARG; }
    if (!sizes_ok(c->n, c->m) || c->T < 1) {
        irs_set_error("%s: need 1<=n<=32, 1<=m<=16, T>=1 (got n=%d, m=%d, T=%d)", fn, c->n, c->m, c->T);
        return IRS_ERR_INVALID_ARG;
    }
    const ValuesBoxPlan p = values_box_plan(c->n, c->m, c->T);
    if (c->T > p.max_T) {
        irs_set_error("%s: horizon T=%d is beyond the any-size bounded TV-LQR kernel's limit T <= %d at (n, m) = (%d, %d) "
                      "(its ADMM vectors need %zu bytes of LDS, max ~160 KB)", fn, c->T, p.max_T, c->n, c->m, p.lds);
        return IRS_ERR_UNSUPPORTED;
    }
    if (!(c->At && c->Bt && c->ct && c->Q && c->Qd && c->R && c->xd_trj && c->info)) {
        irs_set_error("%s: null pointer", fn);
        return IRS_ERR_INVALID_ARG;
    }
    if (((c->x_lo || c->x_hi) && c->x_rows != 1 && c->x_rows != c->T + 1) ||
        ((c->u_lo || c->u_hi) && c->u_rows != 1 && c->u_rows != c->T)) {
        irs_set_error("%s: bounds are one row or one per step (x_rows 1 or %d, u_rows 1 or %d; got %d, %d)", fn, c->T + 1,
                      c->T, c->x_rows, c->u_rows);
        return IRS_ERR_INVALID_ARG;
    }
    if (!(c->rho > 0.0)) { irs_set_error("%s: rho must be positive", fn); return IRS_ERR_INVALID_ARG; }
    if (!(c->relax > 0.0 && c->relax < 2.0)) { irs_set_error("%s: relax must lie in (0, 2)", fn); return IRS_ERR_INVALID_ARG; }
    if (c->workspace == nullptr || c->workspace_bytes < p.ws) {
        irs_set_error("%s: workspace %zu < %zu bytes", fn, c->workspace ? c->workspace_bytes : (size_t)0, p.ws);
        return IRS_ERR_WORKSPACE;
    }
    if ((reinterpret_cast<uintptr_t>(c->workspace) & 255) != 0) {
        irs_set_error("%s: the workspace must be 256-byte aligned", fn);
        return IRS_ERR_WORKSPACE;
    }
    return IRS_OK;
}

}  // namespace

extern "C" {

size_t irs_box_values_workspace_bytes(int n, int m, int T) {
    if (!sizes_ok(n, m) || T < 1) return 0;
    return values_box_plan(n, m, T).ws;
}

int irs_box_values_horizon_limit(int n, int m) {
    return sizes_ok(n, m) ? values_box_plan(n, m, 1).max_T : 0;
}

size_t irs_box_values_lds_bytes(int n, int m, int T) {
    if (!sizes_ok(n, m) || T < 1) return 0;
    return values_box_plan(n, m, T).lds;
}

int irs_box_values_begin(const irs_box_values_call* c, void* stream) {
    const int rc = check_call(__func__, c);
    if (rc != IRS_OK) return rc;
    BeginArgs a{c->At, c->Bt, c->ct, c->Q, c->Qd, c->R, c->xd_trj, c->x_lo, c->x_hi, c->u_lo, c->u_hi,
                c->x_rows == 1 ? 0 : c->n, c->u_rows == 1 ? 0 : c->m, c->alpha_R, c->rho, c->relax,
                static_cast<double*>(c->workspace), c->info, c->n, c->m, c->T};
    hipLaunchKernelGGL(box_values_begin_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), a);
    IRS_CHECK_LAUNCH();
    return IRS_OK;
}

int irs_box_values_tail(const irs_box_values_call* c, int t, const double* x_t, int max_iter, double eps, double* u_t,
                        double* x_plan, double* u_plan, void* stream) {
    int rc = check_call(__func__, c);
    if (rc != IRS_OK) return rc;
    if (t < 0 || t >= c->T) {
        irs_set_error("%s: need 0 <= t < T (got t=%d, T=%d)", __func__, t, c->T);
        return IRS_ERR_INVALID_ARG;
    }
    IRS_CHECK_ARG(x_t && u_t, "null pointer");
    IRS_CHECK_ARG(max_iter > 0 && eps > 0.0, "need max_iter > 0 and eps > 0");
    const ValuesBoxPlan p = values_box_plan(c->n, c->m, c->T);
    TailArgs a{c->x_lo, c->x_hi, c->u_lo, c->u_hi, c->x_rows == 1 ? 0 : c->n, c->u_rows == 1 ? 0 : c->m, x_t, u_t,
               x_plan, u_plan, static_cast<double*>(c->workspace), c->info, eps, c->n, c->m, c->T, t, max_iter};
    rc = launch_tail(a, p, static_cast<hipStream_t>(stream));
    if (rc != IRS_OK) return rc;
    IRS_CHECK_LAUNCH();
    return IRS_OK;
}

}  // extern "C"
