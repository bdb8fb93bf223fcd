// The host side of the cross-entropy-method baseline: every extern "C" entry of the family.  No kernel is compiled
// here: cem.hip holds them behind the launches of cem.hpp.
//
// A CEM descent prices B candidates, selects and refits, and rolls the mean out; the candidates are supplied or drawn
// (CemSource).  Each of the three operations on candidates has ONE checked path here -- cem_cost_call, cem_refit_call,
// cem_stage_call -- that takes the source and the name of the entry (the refusal texts open with it, as IRS_CHECK_ARG's
// do with __func__: tests/test_cem_entries_cpu.py pins them, call by call), and the entries are the fills of those
// paths.  irs_cem_iterate strings the same launches together.
#include "boxqp.hpp"      // has_u_into_x, round256
#include "cem.hpp"

namespace {

int refuse(const char* fn, const char* msg) {
    irs_set_error("%s: %s", fn, msg);
    return IRS_ERR_INVALID_ARG;
}

// what IRS_CHECK_LAUNCH answers under the entry's name
int launched(const char* fn) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return IRS_OK;
    irs_set_error("%s: HIP error %s", fn, hipGetErrorString(e));
    return IRS_ERR_HIP;
}

// IRS_OK for a position-controlled model, else IRS_ERR_UNSUPPORTED
int position_controlled(int model) {
    int rc = IRS_ERR_UNSUPPORTED;
    IRS_DISPATCH_MODEL(model, {
        if (has_u_into_x<Model>::value) rc = IRS_OK;
    });
    return rc;
}

// [a, a + len) and [b, b + len) share an element
bool overlap(const double* a, const double* b, size_t len) { return a < b + len && b < a + len; }

// costs (B) of the source's candidates.  The quasistatic cost also needs Qd and a position-controlled model.
int cem_cost_call(const char* fn, CemCost cost, int model, const double* params, int n_params, int T, int B,
                  const CemSource& src, const double* x0, const double* Q, const double* Qd, const double* R,
                  const double* xd_trj, double* costs, void* stream) {
    const bool quasistatic = cost == CemCost::Quasistatic;
    if (!(T > 0 && B > 0 && !src.has_null() && x0 && Q && (Qd || !quasistatic) && R && xd_trj && costs))
        return refuse(fn, "bad argument");
    ModelParams p;
    int rc = irs_load_params(model, params, n_params, &p);
    if (rc != IRS_OK) return rc;
    rc = irs_cem_launch_rollout(cost, model, p, T, B, src, x0, Q, Qd, R, xd_trj, costs, static_cast<hipStream_t>(stream));
    if (rc != IRS_OK) {      // a model that irs_load_params knows always has the plain rollout
        irs_set_error("%s: model %d is not position controlled", fn, model);
        return rc;
    }
    return launched(fn);
}

// Selection and refit.  Only the drawn refit reads what it must not overwrite: the supplied one has no alias check.
int cem_refit_call(const char* fn, int T, int m, int B, int n_elite, const CemSource& src, const double* costs,
                   int* elite_idx, double* u_new, double* std_new, void* stream) {
    if (!(T > 0 && m > 0 && B > 0 && n_elite > 0 && n_elite <= B)) return refuse(fn, "need 0 < n_elite <= B");
    if (src.has_null() || !costs || !elite_idx || !u_new || !std_new) return refuse(fn, "null pointer");
    const size_t len = (size_t)T * m;
    if (src.drawn && (overlap(u_new, src.mean, len) || overlap(u_new, src.std, len) || overlap(std_new, src.mean, len) ||
                      overlap(std_new, src.std, len) || overlap(u_new, std_new, len)))
        return refuse(fn, "u_new / std_new must not alias u_mean / std (the refit reads the old ones while it writes)");
    irs_cem_launch_refit(T, m, B, n_elite, src, costs, elite_idx, u_new, std_new, static_cast<hipStream_t>(stream));
    return launched(fn);
}

// One stage of the model-free rollout; every refusal comes before any HIP call.
int cem_stage_call(const char* fn, int n, int m, int T, int B, int t, const CemSource& src, const double* x,
                   const double* Q, const double* R, const double* xd_trj, double* u_t, double* costs, void* stream) {
    if (n < 1 || n > kCemStageMaxN) return refuse(fn, "n must be in 1..32");
    if (m < 1 || m > kCemStageMaxM) return refuse(fn, "m must be in 1..16");
    if (T <= 0 || B <= 0) return refuse(fn, "T and B must be positive");
    if (t < 0 || t > T) return refuse(fn, "t must be in 0..T");
    if (!x || !Q || !R || !xd_trj || !costs) return refuse(fn, "null pointer");
    if (t < T && !u_t) return refuse(fn, "u_t is null at a stage t < T");
    if (src.has_null()) return refuse(fn, "null pointer");
    irs_cem_launch_stage(n, m, T, B, t, src, x, Q, R, xd_trj, u_t, costs, static_cast<hipStream_t>(stream));
    return launched(fn);
}

}  // namespace

extern "C" {

int irs_cem_rollout_costs(int model, const double* params, int n_params, int T, int B,
                          const double* u_cand, const double* x0, const double* Q, const double* R,
                          const double* xd_trj, double* costs, void* stream) {
    return cem_cost_call(__func__, CemCost::Plain, model, params, n_params, T, B, CemSource::supplied(u_cand), x0, Q,
                         nullptr, R, xd_trj, costs, stream);
}

int irs_cem_rollout_costs_quasistatic(int model, const double* params, int n_params, int T, int B,
                                      const double* u_cand, const double* x0, const double* Q,
                                      const double* Qd, const double* R, const double* xd_trj, double* costs,
                                      void* stream) {
    return cem_cost_call(__func__, CemCost::Quasistatic, model, params, n_params, T, B, CemSource::supplied(u_cand), x0,
                         Q, Qd, R, xd_trj, costs, stream);
}

int irs_cem_refit(int T, int m, int B, int n_elite, const double* u_cand, const double* costs,
                  int* elite_idx, double* u_new, double* std_new, void* stream) {
    return cem_refit_call(__func__, T, m, B, n_elite, CemSource::supplied(u_cand), costs, elite_idx, u_new, std_new,
                          stream);
}

// ---- device-resident form: candidates drawn in the kernels ---------------------------------------------------

int irs_cem_candidates(int T, int m, int B, const double* u_mean, const double* std, uint64_t seed, uint32_t iter,
                       uint64_t sample_offset, double* u_cand, void* stream) {
    IRS_CHECK_ARG(T > 0 && m > 0 && B > 0, "sizes must be positive");
    IRS_CHECK_ARG(u_mean && std && u_cand, "null pointer");
    const size_t total = (size_t)B * T * m;
    IRS_CHECK_ARG((total + 255) / 256 <= 0x7fffffffull, "B T m too large for one launch");
    irs_cem_launch_candidates(T, m, total, CemSource::draw(u_mean, std, seed, iter, sample_offset), u_cand,
                              static_cast<hipStream_t>(stream));
    return launched(__func__);
}

int irs_cem_rollout_costs_drawn(int model, const double* params, int n_params, int T, int B, const double* u_mean,
                                const double* std, uint64_t seed, uint32_t iter, uint64_t sample_offset,
                                const double* x0, const double* Q, const double* R, const double* xd_trj,
                                double* costs, void* stream) {
    return cem_cost_call(__func__, CemCost::Plain, model, params, n_params, T, B,
                         CemSource::draw(u_mean, std, seed, iter, sample_offset), x0, Q, nullptr, R, xd_trj, costs, stream);
}

int irs_cem_rollout_costs_quasistatic_drawn(int model, const double* params, int n_params, int T, int B,
                                            const double* u_mean, const double* std, uint64_t seed, uint32_t iter,
                                            uint64_t sample_offset, const double* x0, const double* Q,
                                            const double* Qd, const double* R, const double* xd_trj, double* costs,
                                            void* stream) {
    return cem_cost_call(__func__, CemCost::Quasistatic, model, params, n_params, T, B,
                         CemSource::draw(u_mean, std, seed, iter, sample_offset), x0, Q, Qd, R, xd_trj, costs, stream);
}

int irs_cem_refit_drawn(int T, int m, int B, int n_elite, const double* u_mean, const double* std, uint64_t seed,
                        uint32_t iter, uint64_t sample_offset, const double* costs, int* elite_idx, double* u_new,
                        double* std_new, void* stream) {
    return cem_refit_call(__func__, T, m, B, n_elite, CemSource::draw(u_mean, std, seed, iter, sample_offset), costs,
                          elite_idx, u_new, std_new, stream);
}

// ---- model-free rollout: one stage per call, the caller steps the plant between calls ---------------------------

int irs_cem_values_stage(int n, int m, int T, int B, int t, const double* x, const double* u_cand, const double* Q,
                         const double* R, const double* xd_trj, double* u_t, double* costs, void* stream) {
    return cem_stage_call(__func__, n, m, T, B, t, CemSource::supplied(u_cand), x, Q, R, xd_trj, u_t, costs, stream);
}

int irs_cem_values_stage_drawn(int n, int m, int T, int B, int t, const double* x, const double* u_mean,
                               const double* std, uint64_t seed, uint32_t iter, uint64_t sample_offset, const double* Q,
                               const double* R, const double* xd_trj, double* u_t, double* costs, void* stream) {
    return cem_stage_call(__func__, n, m, T, B, t, CemSource::draw(u_mean, std, seed, iter, sample_offset), x, Q, R,
                          xd_trj, u_t, costs, stream);
}

// ---- n_descents descents in one call --------------------------------------------------------------------------

// costs (B) | elite_idx (n_elite) | the plain cost of the mean's rollout where the quasistatic one is reported
size_t irs_cem_iterate_scratch_bytes(int T, int m, int B, int n_elite) {
    if (T <= 0 || m <= 0 || B <= 0 || n_elite <= 0) return 0;
    return round256((size_t)B * sizeof(double)) + round256((size_t)n_elite * sizeof(int)) + 256;
}

int irs_cem_iterate(const irs_cem_iterate_call* c, void* stream) {
    IRS_CHECK_ARG(c != nullptr, "null call struct");
    IRS_CHECK_ARG(c->T > 0 && c->B > 0 && c->n_descents > 0, "T, B and n_descents must be positive");
    IRS_CHECK_ARG(c->n_elite > 0 && c->n_elite <= c->B, "need 0 < n_elite <= B");
    IRS_CHECK_ARG(c->Q && c->R && c->xd_trj && c->x0 && c->u_trj0 && c->std0, "null problem pointer");
    IRS_CHECK_ARG(!c->quasistatic || c->Qd, "the quasistatic cost needs Qd");
    IRS_CHECK_ARG(c->u_hist && c->std_hist && c->x_hist && c->cost_hist && c->scratch, "null output / scratch pointer");
    int n, m, np;
    int rc = irs_model_info(c->model, &n, &m, &np);
    if (rc != IRS_OK) return rc;
    ModelParams p;
    rc = irs_load_params(c->model, c->params, c->n_params, &p);
    if (rc != IRS_OK) return rc;
    if (c->quasistatic && position_controlled(c->model) != IRS_OK) {
        irs_set_error("irs_cem_iterate: model %d is not position controlled", c->model);
        return IRS_ERR_UNSUPPORTED;
    }
    const int T = c->T, B = c->B;
    const size_t need = irs_cem_iterate_scratch_bytes(T, m, B, c->n_elite);
    if (c->scratch_bytes < need) {
        irs_set_error("irs_cem_iterate: scratch %zu < %zu bytes", c->scratch_bytes, need);
        return IRS_ERR_INVALID_ARG;
    }
    char* sp = static_cast<char*>(c->scratch);
    double* costs = reinterpret_cast<double*>(sp);
    int* elite_idx = reinterpret_cast<int*>(sp + round256((size_t)B * sizeof(double)));
    double* plain_cost = reinterpret_cast<double*>(sp + need - 256);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const CemCost cost = c->quasistatic ? CemCost::Quasistatic : CemCost::Plain;
    const size_t us = (size_t)T * m, xs = (size_t)(T + 1) * n;
    for (int i = 0; i < c->n_descents; ++i) {
        // draw around the previous descent's refit (std is always carried; the caller decides what "adopted" means)
        const CemSource src = CemSource::draw(i == 0 ? c->u_trj0 : c->u_hist + (size_t)(i - 1) * us,
                                              i == 0 ? c->std0 : c->std_hist + (size_t)(i - 1) * us, c->seed,
                                              c->iter0 + (uint32_t)i, 0);
        double* u_new = c->u_hist + (size_t)i * us;
        rc = irs_cem_launch_rollout(cost, c->model, p, T, B, src, c->x0, c->Q, c->Qd, c->R, c->xd_trj, costs, st);
        if (rc != IRS_OK) return rc;
        irs_cem_launch_refit(T, m, B, c->n_elite, src, costs, elite_idx, u_new, c->std_hist + (size_t)i * us, st);
        // the mean's rollout (cem.py:182), priced like the candidates
        rc = irs_rollout_cost(c->model, c->params, c->n_params, T, c->x0, u_new, c->Q, c->R, c->xd_trj,
                              c->x_hist + (size_t)i * xs, c->quasistatic ? plain_cost : c->cost_hist + i, stream);
        if (rc != IRS_OK) return rc;
        if (c->quasistatic) {
            rc = irs_cem_launch_rollout(cost, c->model, p, T, 1, CemSource::supplied(u_new), c->x0, c->Q, c->Qd, c->R,
                                        c->xd_trj, c->cost_hist + i, st);
            if (rc != IRS_OK) return rc;
        }
    }
    IRS_CHECK_LAUNCH();
    return IRS_OK;
}

}  // extern "C"
