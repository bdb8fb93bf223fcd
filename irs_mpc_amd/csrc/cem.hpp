// The cross-entropy-method kernels (cem.hip) as their entries (cem_api.hip) see them: where the candidates of an
// operation come from, and the launches the family offers.  No launch here checks an argument or a HIP error.
#pragma once
#include "irs_common.hpp"

// Where the B candidate sequences of a CEM operation come from.  `drawn` tells the two kinds apart:
//   false  the caller's tensor u_cand (B,T,m); nothing else is read;
//   true   candidate b, step t, component j is mean[t,j] + std[t,j] z with z the standard normal of the counter-based
//          stream at (seed, iter, sample_offset + b, t, j) (cem.hip: CemDrawn); u_cand is not read.
struct CemSource {
    bool drawn;
    const double* u_cand;
    const double *mean, *std;           // (T,m)
    uint64_t seed, sample_offset;
    uint32_t iter;

    static CemSource supplied(const double* u_cand) { return {false, u_cand, nullptr, nullptr, 0, 0, 0}; }
    static CemSource draw(const double* mean, const double* std, uint64_t seed, uint32_t iter, uint64_t sample_offset) {
        return {true, nullptr, mean, std, seed, sample_offset, iter};
    }
    // a pointer its kind reads is null
    bool has_null() const { return drawn ? !mean || !std : !u_cand; }
};

// Which cost a rollout prices its candidates with: CrossEntropyMethod's (cem_rollout_kernel) or IrsLqrQuasistatic's
// (cem_rollout_quasistatic_kernel: needs Qd and a position-controlled model).
enum class CemCost { Plain, Quasistatic };

// What the stage kernel takes at run time (torch_system.MAX_DIM_X / MAX_DIM_U)
constexpr int kCemStageMaxN = 32, kCemStageMaxM = 16;

// costs (B) of the B candidates of `src` rolled out on `model` from x0.  Qd is read by the quasistatic cost only.
// IRS_ERR_UNSUPPORTED, nothing launched, when that cost is asked of a model that is not position controlled.
int irs_cem_launch_rollout(CemCost cost, int model, const ModelParams& p, int T, int B, const CemSource& src,
                           const double* x0, const double* Q, const double* Qd, const double* R, const double* xd_trj,
                           double* costs, hipStream_t st);

// Selection (elite_idx: the n_elite cheapest of costs (B), in index order) and the refit over them, two launches.
// Drawn: the elites are regenerated from their indices, and u_new / std_new must not overlap src.mean / src.std.
void irs_cem_launch_refit(int T, int m, int B, int n_elite, const CemSource& src, const double* costs, int* elite_idx,
                          double* u_new, double* std_new, hipStream_t st);

// Stage t of the model-free rollout: x (B,n) the states at step t; costs (B) written at t = 0, added to after; u_t (B,m)
// gets the controls of step t (not touched at t == T).  n <= kCemStageMaxN, m <= kCemStageMaxM.
void irs_cem_launch_stage(int n, int m, int T, int B, int t, const CemSource& src, const double* x, const double* Q,
                          const double* R, const double* xd_trj, double* u_t, double* costs, hipStream_t st);

// The candidate writer: the `total` = B T m elements a drawn source stands for, into u_cand (B,T,m).  At most
// 2^31 - 1 blocks of 256.
void irs_cem_launch_candidates(int T, int m, size_t total, const CemSource& src, double* u_cand, hipStream_t st);
