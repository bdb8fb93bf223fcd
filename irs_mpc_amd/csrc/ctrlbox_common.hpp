// What the two active-set descent kernels (ctrlbox.hip: lanes + LDS; ctrlbox_mfma.hip: matrix-core tiles) state once
// beyond the wave helpers of wave.hpp: the kinds of bound, the cap of the primal-dual phase, and the small rules of
// their setup.  ctrlbox.hip has the derivation of the method.  Everything here is inlined into its kernel.
#pragma once
#include "boxqp.hpp"
#include "wave.hpp"

constexpr int KIND_ABS = 0, KIND_REL = 1;      // the box is on u_t (a.ulo / a.uhi) | on u_t - u_{t-1} (a.dlo / a.dhi)
// Phase 1 updates the active set primal-dual style, which usually ends in a few iterations but may cycle; after
// kPdasIter of them the lanes kernel goes on with the primal method, the tiles kernel with its damped rule first.
constexpr int kPdasIter = 10;

// the bound rows of the launch's kind: row t at ptr + t * stride; null = unbounded
template <int KIND>
__device__ __forceinline__ void ctrlbox_bounds_of(const BoxArgs& a, const double*& blo, const double*& bhi, int& stride) {
    blo = KIND == KIND_ABS ? a.ulo : a.dlo;
    bhi = KIND == KIND_ABS ? a.uhi : a.dhi;
    stride = KIND == KIND_ABS ? a.su : a.sd;
}

// A launch that does not reach its epilogue must not leave a previous launch's values behind: info = -1 is rejected
// by the host like any other failure (the cost's sentinel, NaN, is the plant wave's).
__device__ __forceinline__ void ctrlbox_info_sentinel(int* info, int lane) {
    if (lane == 0) {
        info[0] = -1; info[1] = -1; info[2] = -1;
    }
}

// warm start of the first tail (the previous iLQR iteration's converged set), cleaned: {-1, 0, +1}, and nothing
// pinned at an infinite bound
__device__ __forceinline__ double ctrlbox_clean_warm(double a0, double lo, double hi) {
    constexpr double INF = __builtin_huge_val();
    return a0 < 0.0 ? (lo > -INF ? -1.0 : 0.0) : (a0 > 0.0 ? (hi < INF ? 1.0 : 0.0) : 0.0);
}
