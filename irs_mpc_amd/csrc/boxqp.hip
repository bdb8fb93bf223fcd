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
//
// The kernel's text is boxqp_kernel.inc: this unit compiles it for one problem per launch, boxqp_batch.hip for B.
#include <climits>

#include "boxqp.hpp"
#include "boxqp_layout.hpp"
#include "wave.hpp"

namespace {

#include "boxqp_kernel.inc"

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
// batch_B > 0: that many problems, one workgroup each, on the same plan -- a problem's records are placed where the
// single call would place them, in slice b of the workspace (boxqp_batch.hip).
int irs_box_admm_launch(const char* fn, int model, bool du, const BoxArgs& a, void* ws, size_t ws_bytes, BoxWs policy,
                        hipStream_t st, const BoxAdapt* adapt, const BoxLazy* lazy, int batch_B) {
    const BoxPlan p = irs_box_plan(model, a.T, du ? IRS_BOX_ADMM_DU : IRS_BOX_ADMM,
                                   ws == nullptr ? BoxWs::None : policy);
    if (batch_B > 0 && (du || adapt != nullptr || lazy != nullptr || !irs_box_batch_model(model))) {
        irs_set_error("%s: model %d has no batched bounded descent (served: the plain fixed-penalty form of the "
                      "pendulum, the quadrotor, the bicycle and the three carts)", fn, model);
        return IRS_ERR_UNSUPPORTED;
    }
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
    const WsFit f = ws_fit(p, batch_B > 0 ? (size_t)batch_B : 1, ws, ws_bytes);
    if (p.place == BoxPlace::AdmmHbm && batch_B > 0) {
        // problem b's records at ws + b * f.stride: B slices, each 256-byte aligned
        if (f.small) {
            irs_set_error("%s: workspace %zu < %zu bytes (%d slices of %zu)", fn, ws_bytes, f.need, batch_B, f.stride);
            return IRS_ERR_WORKSPACE;
        }
        if (f.misaligned) {
            irs_set_error("%s: the workspace must be 256-byte aligned", fn);
            return IRS_ERR_WORKSPACE;
        }
    } else if (p.place == BoxPlace::AdmmHbm) {
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
    if (batch_B > 0) {
        rc = irs_box_admm_launch_batch(model, a, p, recs, batch_B, f.stride, st);
    } else if (!du) {
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
