// Shared between the two bounded TV-LQR kernels (boxqp.hip: ADMM; ctrlbox.hip: active set).
#pragma once
#include <type_traits>

#include "irs_common.hpp"

struct BoxArgs {
    ModelParams p;
    const double *At, *Bt, *ct, *Q, *Qd, *R, *xd, *x0;
    // bounds: row t at ptr + t * stride (stride 0 = one constant row); null = unbounded; +-inf ok
    const double *xlo, *xhi;                 // on x_t, t = 0..T   (row 0 unused: x_0 is fixed)
    const double *ulo, *uhi;                 // on u_t, t = 0..T-1
    const double *dlo, *dhi;                 // DU only: on u_t - u_{t-1}
    int sx, su, sd;
    double *x_new, *u_new, *cost;            // cost may be null
    int* info;                               // [0] Hessian not PD at t+1, [1] max ADMM iterations used,
                                             // [2] number of tail problems that hit max_iter
    double alpha, rho, relax, eps;
    int T, max_iter;
    // active-set solver only (may be null): (T,m) in {-1 at lo, 0 free, +1 at hi}.  In: the active set
    // the FIRST tail starts from (zeros = cold start); out: the set that tail converged to -- what the
    // next iLQR iteration's descent should start from
    double* act_io;
    // ADMM kernel only: 1 = solve the FIRST tail problem alone and return its plan (x*, u*) in x_new / u_new --
    // the stand-alone solve_tvlqr (irs_lqr/tv_lqr.py:30-145); no true-dynamics step is taken
    int single_tail;
    // ADMM kernel only (may be null): DEV int; the kernel returns at once, touching nothing, when *run_flag == 0 --
    // the fused iterate (iterate.hip) enqueues the bounded descent behind the test "does any tail's unconstrained plan
    // leave the box", without a host round trip
    const int* run_flag;
};

// position-controlled models expose indices_u_into_x (quasistatic_dynamics.py:57-65)
template <class M, class = void>
struct has_u_into_x : std::false_type {};
template <class M>
struct has_u_into_x<M, std::void_t<decltype(M::u_into_x(0))>> : std::true_type {};


// Where a bounded descent runs: the ADMM kernel with its factor records on chip or in a workspace in HBM, the
// active-set solver on lanes (always on chip), or on matrix-core tiles with its records on chip or in HBM.
enum class BoxPlace { None, AdmmLds, AdmmHbm, Lanes, TilesLds, TilesHbm };
// how the caller offers a workspace: none, for records that do not fit LDS, or for the records at any horizon
enum class BoxWs { None, IfNeeded, Always };
struct BoxPlan {
    BoxPlace place;     // None: the horizon does not run this way (max_T == 0: the model has no such form)
    size_t lds;         // dynamic LDS bytes of the launch (None: what the placement tried last would need)
    size_t records;     // bytes the workspace must hold: the records when they do not stay on chip, else 0
    int max_T;          // the longest horizon of the form, with a workspace where it takes one (INT_MAX: no cap)
};
// boxqp.hip: the one placement decision of every bounded descent and size query.  kind: IRS_BOX_*.  No HIP calls.
BoxPlan irs_box_plan(int model, int T, int kind, BoxWs ws);
inline size_t round256(size_t bytes) { return (bytes + 255) / 256 * 256; }
// Whether a workspace can hold what plan `p` puts there: `count` slices of round256(p.records) bytes (one per problem
// of the launch; stride, need: the bytes of one, of all), 256-byte aligned.  The entries word their own errors.
struct WsFit { size_t stride, need; bool small, misaligned; };
inline WsFit ws_fit(const BoxPlan& p, size_t count, const void* ws, size_t ws_bytes) {
    const size_t stride = round256(p.records);
    return {stride, count * stride, ws_bytes < count * stride, (reinterpret_cast<uintptr_t>(ws) & 255) != 0};
}
inline bool irs_admm_settings_ok(double rho, double relax, int max_iter, double eps) {
    return rho > 0.0 && relax > 0.0 && relax < 2.0 && max_iter > 0 && eps > 0.0;
}
// The adaptive penalty of the ADMM kernel (irs_admm_settings with adaptive != 0): every check_every iterations of a
// tail the residuals are balanced -- rho is rescaled when the factor leaves [1 / trigger, trigger], and the Riccati
// factor rebuilt, at most max_refactor times per tail.  out (DEV, 3, may be null): [0] factorisations of the launch,
// [1] the rho it ended with, [2] its ADMM iterations, all tails.  Travels beside BoxArgs, whose layout every bounded-descent kernel shares.
struct BoxAdapt {
    int check_every, max_refactor;
    double trigger;
    double* out;
};
inline bool irs_admm_adapt_ok(int check_every, double trigger, int max_refactor) {
    return check_every > 0 && trigger > 1.0 && max_refactor >= 0;
}
// Lazily enforced bounds (the LAZY form of the ADMM kernel, compiled on top of the adaptive one; a fixed penalty is
// max_refactor = 0).  Components: the QP's state, then its control -- [x (n) | u (m)], or position controlled
// [x (n) | u abs (m) | du (m)].  enforced_io (DEV, may be null): in, nonzero = enforced from the start (ignored where
// the component has no finite bound; null: none); out, 1 where enforced when the launch ends, else 0.  out (DEV, 3, may
// be null): [0] activation events (each one factorisation), [1] the last tail that activated something or -1, [2] the
// ADMM iterations of the launch.  The lazy kernel takes BoxAdaptLazy where the others take BoxAdapt.
struct BoxLazy {
    int* enforced_io;
    double* out;
};
struct BoxAdaptLazy : BoxAdapt {
    BoxLazy lazy;
};
// boxqp.hip: the ADMM kernel (du: its position-controlled form) on a filled BoxArgs, where the plan puts it.  ws may be
// null; `policy` says what a workspace that is given is for.  fn: the entry a "model has no such form" error names.
// The caller has checked the ADMM settings (irs_admm_settings_ok), as every entry does before anything else.
// adapt: null = fixed rho; else the adaptive form of the kernel (checked by the caller: irs_admm_adapt_ok).
// lazy: null = every finite bound enforced; else the lazy form (adapt must be given: max_refactor = 0 for a fixed rho).
// batch_B = 0: the single problem `a`, one workgroup.  batch_B >= 1: the batched kernel over that many problems, one
// workgroup each (the plain fixed-penalty form of an analytic model only: du false, adapt and lazy null) -- every
// per-problem array of `a` is B contiguous blocks, the bound rows (B,n) / (B,m) and run_flag (B) included; Q / Qd / R
// and the scalars are shared; records in HBM: problem b's at ws + b * round256(records).  Its workspace errors are
// worded with `fn` and are IRS_ERR_WORKSPACE.
int irs_box_admm_launch(const char* fn, int model, bool du, const BoxArgs& a, void* ws, size_t ws_bytes, BoxWs policy,
                        hipStream_t st, const BoxAdapt* adapt = nullptr, const BoxLazy* lazy = nullptr, int batch_B = 0);
// boxqp_batch.hip: the batched instantiations of the kernel (boxqp_kernel.inc with a problem index), launched as planned
// -- AdmmLds, or AdmmHbm with problem b's records at ws + b * ws_stride bytes.  Called by irs_box_admm_launch alone.
int irs_box_admm_launch_batch(int model, const BoxArgs& a, const BoxPlan& p, double* ws, int B, size_t ws_stride,
                              hipStream_t st);
// the models the batched ADMM kernel is instantiated for: the analytic ones (IrsLqrBatch's)
inline bool irs_box_batch_model(int model) {
    return model == IRS_MODEL_PENDULUM || model == IRS_MODEL_QUADROTOR || model == IRS_MODEL_BICYCLE ||
           model == IRS_MODEL_THREE_CART;
}

// ctrlbox.hip: active-set solver for the quasistatic descent with ONE control box.
// kind 0: bounds on u_t (a.ulo/a.uhi), kind 1: bounds on u_t - u_{t-1} (a.dlo/a.dhi); a bound pair
// may be null (unbounded).  Launches with the plan's LDS bytes (place Lanes).
int irs_ctrlbox_launch(int model, const BoxArgs& a, int kind, const BoxPlan& p, hipStream_t st);
size_t irs_ctrlbox_lds_bytes(int model, int T);

// ctrlbox_mfma.hip: the same active-set method with every step riding in one 16 x 16 matrix-core tile.
// record_bytes: size of the per-step records (0 = the model does not fit the tile); lds_bytes: LDS needed
// to keep them on chip.  Launches as planned: TilesLds, or TilesHbm with the records in `ws`.
size_t irs_ctrlbox_mfma_record_bytes(int model, int T);
size_t irs_ctrlbox_mfma_lds_bytes(int model, int T);
// batch_B = 0: the single problem `a`, one workgroup.  batch_B >= 1: the batched kernel over that many problems, one
// workgroup each (B = 1 too: the batched instantiation, not the single one) -- every per-problem array of `a` is B
// contiguous blocks (problem b's at b times the block's size), Q / Qd / R and the scalars are shared; TilesHbm: problem
// b's records at ws + b * ws_stride bytes.
int irs_ctrlbox_mfma_launch(int model, const BoxArgs& a, int kind, const BoxPlan& p, double* ws, hipStream_t st,
                            int batch_B = 0, size_t ws_stride = 0);
