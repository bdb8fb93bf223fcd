// The extern "C" entries of the bounded descents (include/irs_hip.h) -- host code only; boxqp.hpp is all it knows of the
// kernels.  Every entry that ends in the ADMM kernel (boxqp.hip) describes its call in one record, BoxCall, and goes
// through one path, box_call: the checks in one order, one BoxArgs fill, one launch.  What differs between entries --
// the name their errors carry, which bounds they insist on, what a workspace is for -- is data on the record.
#include "boxqp.hpp"

namespace {

enum class BoxForm { Descent, Solve, Quasistatic };    // MPC descent on u bounds; ONE tail QP; descent on [x; u_prev]
// the name the launch words its errors with (one per form, whatever entry was called)
const char* const kFormName[] = {"irs_tvlqr_box_descent", "irs_tvlqr_box_solve", "irs_quasistatic_box_descent"};

struct BoxCall {
    const char* fn;                  // the name the checks word their errors with
    BoxForm form;
    bool du;                         // the position-controlled kernel (Quasistatic: always; Solve: on request)
    int model;
    const double* params;
    int n_params, T;
    const double *At, *Bt, *ct, *Q, *Qd, *R, *xd, *x0;
    const double *xlo, *xhi, *ulo, *uhi, *dlo, *dhi;   // Descent: one constant row each; else per-time rows
    bool all_bounds;                 // xlo, xhi, ulo, uhi must all be given (else: null pairs = unbounded)
    double alpha;
    const irs_admm_settings* settings;   // the caller's, or the entry's own holding its four scalars (adaptive = 0)
    double *x, *u, *cost;
    int* info;
    double* adapt_out;
    void* ws;
    size_t ws_bytes;
    BoxWs policy;                    // Always: the records must go to a workspace that is given, so it is checked first
    const int* run_flag;
    double* act_io;
    const BoxLazy* lazy;             // null: every finite bound enforced
    int batch;                       // 0: one problem; B > 0: that many, every per-problem array B contiguous blocks
    const char* solver_error;        // non-null: the entry's solver argument is refused, in these words
    void* stream;
};

// What the positional entries have in common, in the order they take it; all else null / zero.
BoxCall box_problem(const char* fn, BoxForm form, bool du, int model, const double* params, int n_params, int T,
                    const double* At, const double* Bt, const double* ct, const double* Q, const double* Qd,
                    const double* R, double alpha, const double* xd, const double* x0, const double* xlo,
                    const double* xhi, const double* ulo, const double* uhi, const double* dlo, const double* dhi,
                    const irs_admm_settings* settings, double* x, double* u, double* cost, int* info, void* ws,
                    size_t ws_bytes, BoxWs policy, void* stream) {
    BoxCall c{};
    c.fn = fn; c.form = form; c.du = du; c.model = model; c.params = params; c.n_params = n_params; c.T = T;
    c.At = At; c.Bt = Bt; c.ct = ct; c.Q = Q; c.Qd = Qd; c.R = R; c.alpha = alpha; c.xd = xd; c.x0 = x0;
    c.xlo = xlo; c.xhi = xhi; c.ulo = ulo; c.uhi = uhi; c.dlo = dlo; c.dhi = dhi;
    c.all_bounds = form == BoxForm::Descent;
    c.settings = settings; c.x = x; c.u = u; c.cost = cost; c.info = info;
    c.ws = ws; c.ws_bytes = ws_bytes; c.policy = policy; c.stream = stream;
    return c;
}

// the four scalars of a positional entry as the settings of a fixed penalty
irs_admm_settings fixed_rho(double rho, double relax, int max_iter, double eps) {
    irs_admm_settings s{};
    s.rho = rho; s.relax = relax; s.max_iter = max_iter; s.eps = eps;
    return s;
}

// a workspace the records must go to (the _wsx entries of the ADMM kernel): 256-byte aligned, large enough
// batch > 0: one slice per problem, and both complaints are IRS_ERR_WORKSPACE
int check_box_workspace(const char* fn, int model, int T, int du, const void* ws, size_t ws_bytes, int batch) {
    if (ws == nullptr) return IRS_OK;
    const BoxPlan p = irs_box_plan(model, T, du ? IRS_BOX_ADMM_DU : IRS_BOX_ADMM, BoxWs::Always);
    const WsFit f = ws_fit(p, batch > 0 ? (size_t)batch : 1, ws, ws_bytes);
    if (f.misaligned) {
        irs_set_error("%s: the workspace must be 256-byte aligned", fn);
        return batch > 0 ? IRS_ERR_WORKSPACE : IRS_ERR_INVALID_ARG;
    }
    if (p.max_T == 0) {
        irs_set_error("%s: model %d has no %s form", fn, model, du ? "position-controlled" : "plain");
        return IRS_ERR_UNSUPPORTED;
    }
    if (f.small) {
        irs_set_error("%s: workspace %zu < %zu bytes", fn, ws_bytes, f.need);
        return IRS_ERR_WORKSPACE;
    }
    return IRS_OK;
}

// `model` has no active-set form on the tiles: it does not fit them, or it is not position controlled at all
int no_tile_form(const char* fn, int model, int T) {
    irs_set_error(irs_box_plan(model, T, IRS_BOX_ADMM_DU, BoxWs::None).max_T > 0
                      ? "%s: model %d does not fit the 16 x 16 tile"
                      : "%s: model %d is not position controlled", fn, model);
    return IRS_ERR_UNSUPPORTED;
}

// solver 0 of the quasistatic descent: the tiles where the model fits them and their records have a place, else the
// lanes where they fit LDS, else ADMM
int auto_solver(int model, int T, bool one_box, const void* ws, size_t ws_bytes) {
    if (!one_box) return 1;
    const BoxPlan tiles = irs_box_plan(model, T, IRS_BOX_ACTIVE_SET_MFMA, ws ? BoxWs::IfNeeded : BoxWs::None);
    if (tiles.place != BoxPlace::None && ws_bytes >= tiles.records) return 3;
    return irs_box_plan(model, T, IRS_BOX_ACTIVE_SET, BoxWs::None).place == BoxPlace::Lanes ? 2 : 1;
}

// The checks of an irs_admm_settings (fn: the entry, for the message) and what the launch takes from it: *adapt is
// left null for adaptive == 0 -- the fixed-rho kernel -- and else points at *ad, filled with the rule's constants.
int read_admm_settings(const char* fn, const irs_admm_settings* s, double* adapt_out, BoxAdapt* ad,
                       const BoxAdapt** adapt) {
    *adapt = nullptr;
    if (s == nullptr) {
        irs_set_error("%s: settings must not be NULL", fn);
        return IRS_ERR_INVALID_ARG;
    }
    if (!irs_admm_settings_ok(s->rho, s->relax, s->max_iter, s->eps)) {
        irs_set_error("%s: bad ADMM parameter", fn);
        return IRS_ERR_INVALID_ARG;
    }
    if (s->adaptive == 0) return IRS_OK;
    if (!irs_admm_adapt_ok(s->check_every, s->trigger, s->max_refactor)) {
        irs_set_error("%s: the adaptive penalty needs check_every > 0, trigger > 1 and max_refactor >= 0", fn);
        return IRS_ERR_INVALID_ARG;
    }
    *ad = BoxAdapt{s->check_every, s->max_refactor, s->trigger, adapt_out};
    *adapt = ad;
    return IRS_OK;
}

// The lazy entries: the kernel's lazy form is compiled on top of the adaptive one, so a fixed penalty (adaptive == 0:
// *adapt null after read_admm_settings) runs there with a rule that never fires -- max_refactor = 0.
void lazy_adapt(double* adapt_out, BoxAdapt* ad, const BoxAdapt** adapt) {
    if (*adapt != nullptr) return;
    *ad = BoxAdapt{1, 0, 2.0, adapt_out};
    *adapt = ad;
}

// The one BoxArgs fill: all else null / zero, the model's constants, the horizon, the strides of the bound rows --
// per-time rows (n / m), Descent one constant row (0) -- and every field the record names.  c.settings is not null.
int box_fill(const BoxCall& c, BoxArgs* a) {
    *a = BoxArgs{};
    const int rc = irs_load_params(c.model, c.params, c.n_params, &a->p);
    if (rc != IRS_OK) return rc;
    int n = 0, m = 0, np;
    if (c.form != BoxForm::Descent) irs_model_info(c.model, &n, &m, &np);
    a->sx = n; a->su = m; a->sd = m; a->T = c.T;
    a->At = c.At; a->Bt = c.Bt; a->ct = c.ct; a->Q = c.Q; a->Qd = c.Qd; a->R = c.R; a->xd = c.xd; a->x0 = c.x0;
    a->xlo = c.xlo; a->xhi = c.xhi; a->ulo = c.ulo; a->uhi = c.uhi; a->dlo = c.dlo; a->dhi = c.dhi;
    a->alpha = c.alpha; a->rho = c.settings->rho; a->relax = c.settings->relax; a->max_iter = c.settings->max_iter;
    a->eps = c.settings->eps;
    a->x_new = c.x; a->u_new = c.u; a->cost = c.cost; a->info = c.info;
    a->act_io = c.act_io; a->run_flag = c.run_flag; a->single_tail = c.form == BoxForm::Solve ? 1 : 0;
    return IRS_OK;
}

// The checks of a bounded-ADMM call, in their one order, then its BoxArgs and -- *adapt, pointing at *ad or null -- the
// penalty rule of its launch.
int box_call_args(const BoxCall& c, BoxArgs* a, BoxAdapt* ad, const BoxAdapt** adapt) {
    const auto refuse = [&c](const char* msg) {
        irs_set_error("%s: %s", c.fn, msg);
        return IRS_ERR_INVALID_ARG;
    };
    if (!(c.T > 0 && c.At && c.Bt && c.ct && c.Q && c.Qd && c.R && c.xd && c.x0 && c.x && c.u && c.info &&
          (!c.all_bounds || (c.xlo && c.xhi && c.ulo && c.uhi))))
        return refuse("bad argument");
    if (c.solver_error != nullptr) return refuse(c.solver_error);
    if (!((c.xlo == nullptr) == (c.xhi == nullptr) && (c.ulo == nullptr) == (c.uhi == nullptr) &&
          (c.dlo == nullptr) == (c.dhi == nullptr)))
        return refuse("give both sides of a bound or neither");
    if (!(c.du || c.dlo == nullptr)) return refuse("du bounds need the position-controlled form");
    int rc = read_admm_settings(c.fn, c.settings, c.adapt_out, ad, adapt);
    if (rc != IRS_OK) return rc;
    if (c.batch > 0 && !irs_box_batch_model(c.model)) {
        irs_set_error("%s: model %d has no batched bounded descent (served: the pendulum, the quadrotor, the bicycle and "
                      "the three carts; a contact model's is irs_quasistatic_box_descent_batch)", c.fn, c.model);
        return IRS_ERR_UNSUPPORTED;
    }
    int np = 0;
    if (c.batch > 0 && (irs_model_info(c.model, nullptr, nullptr, &np) != IRS_OK || c.params == nullptr || c.n_params != np)) {
        irs_set_error("%s: model %d expects %d params, got %d", c.fn, c.model, np, c.n_params);
        return IRS_ERR_INVALID_ARG;
    }
    if (c.policy == BoxWs::Always) {
        rc = check_box_workspace(c.fn, c.model, c.T, c.du ? 1 : 0, c.ws, c.ws_bytes, c.batch);
        if (rc != IRS_OK) return rc;
    }
    rc = box_fill(c, a);
    if (rc != IRS_OK) return rc;
    if (c.lazy != nullptr) lazy_adapt(c.adapt_out, ad, adapt);
    return IRS_OK;
}

int box_call_launch(const BoxCall& c, const BoxArgs& a, const BoxAdapt* adapt) {
    // (a batch words the launch's errors with its own name: its workspace is B slices)
    return irs_box_admm_launch(c.batch > 0 ? c.fn : kFormName[(int)c.form], c.model, c.du, a, c.ws, c.ws_bytes, c.policy,
                               static_cast<hipStream_t>(c.stream), adapt, c.lazy, c.batch);
}

int box_call(const BoxCall& c) {
    BoxArgs a;
    BoxAdapt ad;
    const BoxAdapt* adapt;
    const int rc = box_call_args(c, &a, &ad, &adapt);
    return rc != IRS_OK ? rc : box_call_launch(c, a, adapt);
}

}  // namespace

extern "C" {

size_t irs_tvlqr_box_lds_bytes(int model, int T) {
    return T > 0 ? irs_box_plan(model, T, IRS_BOX_ADMM, BoxWs::None).lds : 0;
}

size_t irs_quasistatic_box_lds_bytes(int model, int T, int solver) {
    const int kind = solver == 2 ? IRS_BOX_ACTIVE_SET : solver == 3 ? IRS_BOX_ACTIVE_SET_MFMA : IRS_BOX_ADMM_DU;
    return T > 0 ? irs_box_plan(model, T, kind, BoxWs::None).lds : 0;
}

size_t irs_tvlqr_box_workspace_bytes(int model, int T, int du) {
    return T > 0 ? irs_box_plan(model, T, du ? IRS_BOX_ADMM_DU : IRS_BOX_ADMM, BoxWs::IfNeeded).records : 0;
}

size_t irs_tvlqr_box_hbm_lds_bytes(int model, int T, int du) {
    return T > 0 ? irs_box_plan(model, T, du ? IRS_BOX_ADMM_DU : IRS_BOX_ADMM, BoxWs::Always).lds : 0;
}

size_t irs_box_records_bytes(int model, int T, int kind) {
    return T > 0 ? irs_box_plan(model, T, kind, BoxWs::Always).records : 0;
}

size_t irs_quasistatic_descent_workspace_bytes(int model, int T, int solver) {
    if (T <= 0 || solver < 0 || solver > 3 || solver == 2) return 0;
    const size_t tiles = solver != 1 ? irs_box_plan(model, T, IRS_BOX_ACTIVE_SET_MFMA, BoxWs::IfNeeded).records : 0;
    const size_t admm = solver != 3 ? irs_box_plan(model, T, IRS_BOX_ADMM_DU, BoxWs::IfNeeded).records : 0;
    return tiles > admm ? tiles : admm;
}

int irs_box_horizon_limit(int model, int kind) {
    return kind >= IRS_BOX_ADMM && kind <= IRS_BOX_ACTIVE_SET_MFMA ? irs_box_plan(model, 1, kind, BoxWs::IfNeeded).max_T
                                                                   : 0;
}

// ---- local_descent with constant u / x boxes: irs_tvlqr_box_descent* ---------------------------------------------------
int irs_tvlqr_box_descent(int model, const double* params, int n_params, int T, const double* At,
                          const double* Bt, const double* ct, const double* Q, const double* Qd,
                          const double* R, double alpha_R, const double* xd_trj, const double* x0,
                          const double* xlo, const double* xhi, const double* ulo, const double* uhi,
                          double rho, double relax, int max_iter, double eps, double* x_new,
                          double* u_new, int* info, void* stream) {
    return irs_tvlqr_box_descent_if(model, params, n_params, T, At, Bt, ct, Q, Qd, R, alpha_R, xd_trj, x0, xlo, xhi, ulo,
                                    uhi, rho, relax, max_iter, eps, x_new, u_new, nullptr, info, nullptr, stream);
}

int irs_tvlqr_box_descent_if(int model, const double* params, int n_params, int T, const double* At,
                             const double* Bt, const double* ct, const double* Q, const double* Qd,
                             const double* R, double alpha_R, const double* xd_trj, const double* x0,
                             const double* xlo, const double* xhi, const double* ulo, const double* uhi,
                             double rho, double relax, int max_iter, double eps, double* x_new,
                             double* u_new, double* cost, int* info, const int* run_flag, void* stream) {
    // (its messages keep the name of the internal function that used to make these checks: an entry's error text
    // does not change)
    const irs_admm_settings s = fixed_rho(rho, relax, max_iter, eps);
    BoxCall c = box_problem("irs_tvlqr_box_descent_ifw", BoxForm::Descent, false, model, params, n_params, T, At, Bt, ct,
                            Q, Qd, R, alpha_R, xd_trj, x0, xlo, xhi, ulo, uhi, nullptr, nullptr, &s, x_new, u_new, cost,
                            info, nullptr, 0, BoxWs::None, stream);
    c.run_flag = run_flag;
    return box_call(c);
}

int irs_tvlqr_box_descent_wsx(int model, const double* params, int n_params, int T, const double* At,
                              const double* Bt, const double* ct, const double* Q, const double* Qd,
                              const double* R, double alpha_R, const double* xd_trj, const double* x0,
                              const double* xlo, const double* xhi, const double* ulo, const double* uhi,
                              double rho, double relax, int max_iter, double eps, double* x_new,
                              double* u_new, int* info, void* workspace, size_t workspace_bytes, void* stream) {
    const irs_admm_settings s = fixed_rho(rho, relax, max_iter, eps);
    return box_call(box_problem(__func__, BoxForm::Descent, false, model, params, n_params, T, At, Bt, ct, Q, Qd, R,
                                alpha_R, xd_trj, x0, xlo, xhi, ulo, uhi, nullptr, nullptr, &s, x_new, u_new, nullptr,
                                info, workspace, workspace_bytes, BoxWs::Always, stream));
}

int irs_tvlqr_box_descent_set(int model, const double* params, int n_params, int T, const double* At,
                              const double* Bt, const double* ct, const double* Q, const double* Qd,
                              const double* R, double alpha_R, const double* xd_trj, const double* x0,
                              const double* xlo, const double* xhi, const double* ulo, const double* uhi,
                              const irs_admm_settings* settings, double* x_new, double* u_new, int* info,
                              double* adapt_out, void* workspace, size_t workspace_bytes, void* stream) {
    BoxCall c = box_problem(__func__, BoxForm::Descent, false, model, params, n_params, T, At, Bt, ct, Q, Qd, R, alpha_R,
                            xd_trj, x0, xlo, xhi, ulo, uhi, nullptr, nullptr, settings, x_new, u_new, nullptr, info,
                            workspace, workspace_bytes, BoxWs::Always, stream);
    c.adapt_out = adapt_out;
    return box_call(c);
}

// B descents of an analytic model in one launch: the call record of irs_tvlqr_box_descent_if / _wsx plus a batch count
size_t irs_tvlqr_box_descent_batch_workspace_bytes(int model, int T, int B) {
    if (T <= 0 || B <= 0 || !irs_box_batch_model(model)) return 0;
    const BoxPlan p = irs_box_plan(model, T, IRS_BOX_ADMM, BoxWs::Always);
    return p.place == BoxPlace::AdmmHbm ? (size_t)B * round256(p.records) : 0;      // (None: beyond the horizon limit)
}

int irs_tvlqr_box_descent_batch(int model, const double* params, int n_params, int T, int B, const double* At,
                                const double* Bt, const double* ct, const double* Q, const double* Qd, const double* R,
                                double alpha_R, const double* xd_trj, const double* x0, const double* xlo,
                                const double* xhi, const double* ulo, const double* uhi, double rho, double relax,
                                int max_iter, double eps, double* x_new, double* u_new, double* cost, int* info,
                                const int* run_flag, void* workspace, size_t workspace_bytes, void* stream) {
    IRS_CHECK_ARG(B > 0, "B must be positive");
    const irs_admm_settings s = fixed_rho(rho, relax, max_iter, eps);
    BoxCall c = box_problem(__func__, BoxForm::Descent, false, model, params, n_params, T, At, Bt, ct, Q, Qd, R, alpha_R,
                            xd_trj, x0, xlo, xhi, ulo, uhi, nullptr, nullptr, &s, x_new, u_new, cost, info, workspace,
                            workspace_bytes, BoxWs::Always, stream);
    c.run_flag = run_flag;
    c.batch = B;
    return box_call(c);
}

// ---- IrsLqrQuasistatic.local_descent: irs_quasistatic_box_descent* -----------------------------------------------------
int irs_quasistatic_box_descent(int model, const double* params, int n_params, int T, const double* At,
                                const double* Bt, const double* ct, const double* Q, const double* Qd,
                                const double* R, const double* xd_trj, const double* x0,
                                const double* x_lo, const double* x_hi, const double* u_lo,
                                const double* u_hi, const double* du_lo, const double* du_hi,
                                int solver, double rho, double relax, int max_iter, double eps,
                                double* x_new, double* u_new, double* cost, int* info, void* stream) {
    return irs_quasistatic_box_descent_ws(model, params, n_params, T, At, Bt, ct, Q, Qd, R, xd_trj, x0, x_lo, x_hi,
                                          u_lo, u_hi, du_lo, du_hi, solver, rho, relax, max_iter, eps, x_new,
                                          u_new, cost, info, nullptr, stream);
}

int irs_quasistatic_box_descent_ws(int model, const double* params, int n_params, int T, const double* At,
                                   const double* Bt, const double* ct, const double* Q, const double* Qd,
                                   const double* R, const double* xd_trj, const double* x0,
                                   const double* x_lo, const double* x_hi, const double* u_lo,
                                   const double* u_hi, const double* du_lo, const double* du_hi,
                                   int solver, double rho, double relax, int max_iter, double eps,
                                   double* x_new, double* u_new, double* cost, int* info, double* act_io,
                                   void* stream) {
    return irs_quasistatic_box_descent_wsx(model, params, n_params, T, At, Bt, ct, Q, Qd, R, xd_trj, x0, x_lo, x_hi,
                                           u_lo, u_hi, du_lo, du_hi, solver, rho, relax, max_iter, eps, x_new,
                                           u_new, cost, info, act_io, nullptr, 0, stream);
}

int irs_quasistatic_box_descent_wsx(int model, const double* params, int n_params, int T, const double* At,
                                    const double* Bt, const double* ct, const double* Q, const double* Qd,
                                    const double* R, const double* xd_trj, const double* x0,
                                    const double* x_lo, const double* x_hi, const double* u_lo,
                                    const double* u_hi, const double* du_lo, const double* du_hi,
                                    int solver, double rho, double relax, int max_iter, double eps,
                                    double* x_new, double* u_new, double* cost, int* info, double* act_io,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    const irs_admm_settings s = fixed_rho(rho, relax, max_iter, eps);
    // alpha = 1: tv_lqr.py:107 adds du'R du as an expression, the full quadratic.  Records in the workspace only when
    // they do not fit LDS
    BoxCall c = box_problem(__func__, BoxForm::Quasistatic, true, model, params, n_params, T, At, Bt, ct, Q, Qd, R, 1.0,
                            xd_trj, x0, x_lo, x_hi, u_lo, u_hi, du_lo, du_hi, &s, x_new, u_new, cost, info, workspace,
                            workspace_bytes, BoxWs::IfNeeded, stream);
    c.act_io = act_io;
    if (!(solver >= 0 && solver <= 3))
        c.solver_error = "solver must be 0 (auto), 1 (ADMM), 2 (active set, lanes) or 3 (active set, matrix-core tiles)";
    BoxArgs a;
    BoxAdapt ad;
    const BoxAdapt* adapt;
    int rc = box_call_args(c, &a, &ad, &adapt);
    if (rc != IRS_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // one control box (or none) and no state bounds: the exact active-set solvers apply
    const bool one_box = x_lo == nullptr && !(u_lo != nullptr && du_lo != nullptr);
    if ((solver == 2 || solver == 3) && !one_box) {
        irs_set_error("irs_quasistatic_box_descent: the active-set solvers handle ONE of u / du bounds and no x bounds");
        return IRS_ERR_UNSUPPORTED;
    }
    if (solver == 0) solver = auto_solver(model, T, one_box, workspace, workspace_bytes);
    if (solver == 1) return box_call_launch(c, a, adapt);
    const BoxPlan p = irs_box_plan(model, T, solver == 3 ? IRS_BOX_ACTIVE_SET_MFMA : IRS_BOX_ACTIVE_SET,
                                   workspace != nullptr ? BoxWs::IfNeeded : BoxWs::None);
    if (p.max_T == 0) return no_tile_form("irs_quasistatic_box_descent", model, T);
    if (p.place == BoxPlace::None || workspace_bytes < p.records) {
        if (solver == 3)
            irs_set_error("irs_quasistatic_box_descent: horizon T=%d needs a %zu-byte workspace for the matrix-core "
                          "active-set solver (records do not fit LDS)", T, p.records);
        else
            irs_set_error("irs_quasistatic_box_descent: horizon T=%d needs %zu bytes of LDS (max ~160 KB)", T, p.lds);
        return IRS_ERR_UNSUPPORTED;
    }
    const int kind = du_lo != nullptr ? 1 : 0;
    rc = solver == 3 ? irs_ctrlbox_mfma_launch(model, a, kind, p, static_cast<double*>(workspace), st)
                     : irs_ctrlbox_launch(model, a, kind, p, st);
    if (rc != IRS_OK) return rc;
    IRS_CHECK_LAUNCH();
    return IRS_OK;
}

// the ADMM form (solver 1) alone, with its settings in a struct: the adaptive penalty is the ADMM kernel's
int irs_quasistatic_box_descent_set(int model, const double* params, int n_params, int T, const double* At,
                                    const double* Bt, const double* ct, const double* Q, const double* Qd,
                                    const double* R, const double* xd_trj, const double* x0,
                                    const double* x_lo, const double* x_hi, const double* u_lo,
                                    const double* u_hi, const double* du_lo, const double* du_hi,
                                    int solver, const irs_admm_settings* settings, double* x_new, double* u_new,
                                    double* cost, int* info, double* adapt_out, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    BoxCall c = box_problem(__func__, BoxForm::Quasistatic, true, model, params, n_params, T, At, Bt, ct, Q, Qd, R, 1.0,
                            xd_trj, x0, x_lo, x_hi, u_lo, u_hi, du_lo, du_hi, settings, x_new, u_new, cost, info,
                            workspace, workspace_bytes, BoxWs::IfNeeded, stream);
    c.adapt_out = adapt_out;
    if (solver != 1) c.solver_error = "solver must be 1 (ADMM): the settings are the ADMM kernel's";
    return box_call(c);
}

// ---- B problems per launch (solver 3's method) ---------------------------------------------------------------------
size_t irs_quasistatic_descent_batch_workspace_bytes(int model, int T, int B) {
    if (T <= 0 || B <= 0) return 0;
    return (size_t)B * round256(irs_box_plan(model, T, IRS_BOX_ACTIVE_SET_MFMA, BoxWs::IfNeeded).records);
}

int irs_quasistatic_box_descent_batch(int model, const double* params, int n_params, int T, int B, const double* At,
                                      const double* Bt, const double* ct, const double* Q, const double* Qd,
                                      const double* R, const double* xd_trj, const double* x0, const double* u_lo,
                                      const double* u_hi, const double* du_lo, const double* du_hi, int max_iter,
                                      double eps, double* x_new, double* u_new, double* cost, int* info, double* act_io,
                                      void* workspace, size_t workspace_bytes, void* stream) {
    IRS_CHECK_ARG(T > 0 && B > 0, "T and B must be positive");
    IRS_CHECK_ARG(At && Bt && ct && Q && Qd && R && xd_trj && x0 && x_new && u_new && info, "bad argument");
    IRS_CHECK_ARG((u_lo == nullptr) == (u_hi == nullptr) && (du_lo == nullptr) == (du_hi == nullptr),
                  "give both sides of a bound or neither");
    IRS_CHECK_ARG((u_lo != nullptr) != (du_lo != nullptr), "give exactly one of the u / du bound pairs");
    IRS_CHECK_ARG(max_iter > 0 && eps > 0.0, "bad solver parameter");
    const irs_admm_settings s = fixed_rho(10.0, 1.6, max_iter, eps);      // (rho, relax: what BoxArgs has always held here)
    BoxCall c = box_problem(__func__, BoxForm::Quasistatic, true, model, params, n_params, T, At, Bt, ct, Q, Qd, R, 1.0,
                            xd_trj, x0, nullptr, nullptr, u_lo, u_hi, du_lo, du_hi, &s, x_new, u_new, cost, info,
                            workspace, workspace_bytes, BoxWs::Always, stream);
    c.act_io = act_io;
    BoxArgs a;
    int rc = box_fill(c, &a);
    if (rc != IRS_OK) return rc;
    // a workspace puts the records there at any horizon (as irs_tvlqr_box_descent_wsx does); without one they must
    // fit LDS
    const BoxPlan p = irs_box_plan(model, T, IRS_BOX_ACTIVE_SET_MFMA, workspace != nullptr ? BoxWs::Always : BoxWs::None);
    if (p.max_T == 0) return no_tile_form("irs_quasistatic_box_descent_batch", model, T);
    const WsFit f = ws_fit(p, (size_t)B, workspace, workspace_bytes);
    if (p.place == BoxPlace::None || f.small) {
        irs_set_error("irs_quasistatic_box_descent_batch: horizon T=%d, B=%d needs a workspace of %zu bytes (given: %zu)",
                      T, B, f.need, workspace_bytes);
        return IRS_ERR_WORKSPACE;
    }
    if (p.place == BoxPlace::TilesHbm && f.misaligned) {
        irs_set_error("irs_quasistatic_box_descent_batch: the workspace must be 256-byte aligned");
        return IRS_ERR_INVALID_ARG;
    }
    rc = irs_ctrlbox_mfma_launch(model, a, du_lo != nullptr ? 1 : 0, p, static_cast<double*>(workspace),
                                 static_cast<hipStream_t>(stream), B, f.stride);
    if (rc != IRS_OK) return rc;
    IRS_CHECK_LAUNCH();
    return IRS_OK;
}

// ---- solve_tvlqr (irs_lqr/tv_lqr.py:30-145) stand-alone: ONE bounded QP, its plan returned ---------------------------
int irs_tvlqr_box_solve(int model, const double* params, int n_params, int T, const double* At, const double* Bt,
                        const double* ct, const double* Q, const double* Qd, const double* R, double alpha_R,
                        const double* xd_trj, const double* x0, int position_controlled,
                        const double* x_lo, const double* x_hi, const double* u_lo, const double* u_hi,
                        const double* du_lo, const double* du_hi, double rho, double relax, int max_iter,
                        double eps, double* x_star, double* u_star, int* info, void* stream) {
    return irs_tvlqr_box_solve_wsx(model, params, n_params, T, At, Bt, ct, Q, Qd, R, alpha_R, xd_trj, x0,
                                   position_controlled, x_lo, x_hi, u_lo, u_hi, du_lo, du_hi, rho, relax, max_iter, eps,
                                   x_star, u_star, info, nullptr, 0, stream);
}

int irs_tvlqr_box_solve_wsx(int model, const double* params, int n_params, int T, const double* At, const double* Bt,
                            const double* ct, const double* Q, const double* Qd, const double* R, double alpha_R,
                            const double* xd_trj, const double* x0, int position_controlled,
                            const double* x_lo, const double* x_hi, const double* u_lo, const double* u_hi,
                            const double* du_lo, const double* du_hi, double rho, double relax, int max_iter,
                            double eps, double* x_star, double* u_star, int* info, void* workspace,
                            size_t workspace_bytes, void* stream) {
    const irs_admm_settings s = fixed_rho(rho, relax, max_iter, eps);
    return box_call(box_problem(__func__, BoxForm::Solve, position_controlled != 0, model, params, n_params, T, At, Bt,
                                ct, Q, Qd, R, alpha_R, xd_trj, x0, x_lo, x_hi, u_lo, u_hi, du_lo, du_hi, &s, x_star,
                                u_star, nullptr, info, workspace, workspace_bytes, BoxWs::Always, stream));
}

int irs_tvlqr_box_solve_set(int model, const double* params, int n_params, int T, const double* At, const double* Bt,
                            const double* ct, const double* Q, const double* Qd, const double* R, double alpha_R,
                            const double* xd_trj, const double* x0, int position_controlled,
                            const double* x_lo, const double* x_hi, const double* u_lo, const double* u_hi,
                            const double* du_lo, const double* du_hi, const irs_admm_settings* settings,
                            double* x_star, double* u_star, int* info, double* adapt_out, void* workspace,
                            size_t workspace_bytes, void* stream) {
    BoxCall c = box_problem(__func__, BoxForm::Solve, position_controlled != 0, model, params, n_params, T, At, Bt, ct, Q,
                            Qd, R, alpha_R, xd_trj, x0, x_lo, x_hi, u_lo, u_hi, du_lo, du_hi, settings, x_star, u_star,
                            nullptr, info, workspace, workspace_bytes, BoxWs::Always, stream);
    c.adapt_out = adapt_out;
    return box_call(c);
}

// ---- lazily enforced bounds: the _set entries plus the set and its counters ------------------------------------------
int irs_tvlqr_box_descent_lazy(int model, const double* params, int n_params, int T, const double* At,
                               const double* Bt, const double* ct, const double* Q, const double* Qd,
                               const double* R, double alpha_R, const double* xd_trj, const double* x0,
                               const double* xlo, const double* xhi, const double* ulo, const double* uhi,
                               const irs_admm_settings* settings, double* x_new, double* u_new, int* info,
                               double* adapt_out, void* workspace, size_t workspace_bytes, int* enforced_io,
                               double* lazy_out, void* stream) {
    const BoxLazy lazy{enforced_io, lazy_out};
    BoxCall c = box_problem(__func__, BoxForm::Descent, false, model, params, n_params, T, At, Bt, ct, Q, Qd, R, alpha_R,
                            xd_trj, x0, xlo, xhi, ulo, uhi, nullptr, nullptr, settings, x_new, u_new, nullptr, info,
                            workspace, workspace_bytes, BoxWs::Always, stream);
    c.adapt_out = adapt_out; c.lazy = &lazy;
    return box_call(c);
}

int irs_tvlqr_box_solve_lazy(int model, const double* params, int n_params, int T, const double* At, const double* Bt,
                             const double* ct, const double* Q, const double* Qd, const double* R, double alpha_R,
                             const double* xd_trj, const double* x0, int position_controlled,
                             const double* x_lo, const double* x_hi, const double* u_lo, const double* u_hi,
                             const double* du_lo, const double* du_hi, const irs_admm_settings* settings,
                             double* x_star, double* u_star, int* info, double* adapt_out, void* workspace,
                             size_t workspace_bytes, int* enforced_io, double* lazy_out, void* stream) {
    const BoxLazy lazy{enforced_io, lazy_out};
    BoxCall c = box_problem(__func__, BoxForm::Solve, position_controlled != 0, model, params, n_params, T, At, Bt, ct, Q,
                            Qd, R, alpha_R, xd_trj, x0, x_lo, x_hi, u_lo, u_hi, du_lo, du_hi, settings, x_star, u_star,
                            nullptr, info, workspace, workspace_bytes, BoxWs::Always, stream);
    c.adapt_out = adapt_out; c.lazy = &lazy;
    return box_call(c);
}

int irs_quasistatic_box_descent_lazy(int model, const double* params, int n_params, int T, const double* At,
                                     const double* Bt, const double* ct, const double* Q, const double* Qd,
                                     const double* R, const double* xd_trj, const double* x0,
                                     const double* x_lo, const double* x_hi, const double* u_lo,
                                     const double* u_hi, const double* du_lo, const double* du_hi,
                                     int solver, const irs_admm_settings* settings, double* x_new, double* u_new,
                                     double* cost, int* info, double* adapt_out, void* workspace,
                                     size_t workspace_bytes, int* enforced_io, double* lazy_out, void* stream) {
    const BoxLazy lazy{enforced_io, lazy_out};
    BoxCall c = box_problem(__func__, BoxForm::Quasistatic, true, model, params, n_params, T, At, Bt, ct, Q, Qd, R, 1.0,
                            xd_trj, x0, x_lo, x_hi, u_lo, u_hi, du_lo, du_hi, settings, x_new, u_new, cost, info,
                            workspace, workspace_bytes, BoxWs::IfNeeded, stream);
    c.adapt_out = adapt_out; c.lazy = &lazy;
    if (solver != 1) c.solver_error = "solver must be 1 (ADMM): the lazily enforced bounds are the ADMM kernel's";
    return box_call(c);
}

}  // extern "C"
