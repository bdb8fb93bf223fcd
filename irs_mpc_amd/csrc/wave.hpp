// Wave-level primitives of the descent kernels (tvlqr.hip, boxqp.hip, ctrlbox.hip, ctrlbox_mfma.hip, iterate.hip).
// Every one of these kernels is one 64-lane wave walking a latency-bound chain (the active-set descents: one solver
// wave plus one plant wave, meeting at wg_barrier); the helpers below are what such a wave needs between its lanes.
// (The sample pass has its own set in smooth_common.hpp.)
#pragma once
#include <hip/hip_runtime.h>

typedef double v4d __attribute__((ext_vector_type(4)));      // operand / accumulator of v_mfma_f64_16x16x4_f64

// Orders ONE wave's LDS traffic: the LDS executes a wave's operations in issue order,
// so this only has to stop the compiler from moving them; it deliberately does not
// wait for outstanding global loads (the prefetches stay in flight).
__device__ __forceinline__ void wave_sync() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

// Workgroup barrier between the solver wave and the plant wave of the active-set descents: everything this wave has
// written (LDS and global) is complete before it arrives, and nothing of what follows is moved ahead of it.
__device__ __forceinline__ void wg_barrier() {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// 1/d to ~1 ulp: hardware reciprocal + two Newton steps (a correctly rounded f64 divide
// is ~40 dependent instructions on the critical path of every backward step).
__device__ __forceinline__ double fast_rcp(double d) {
    double r = __builtin_amdgcn_rcp(d);
    r = fma(fma(-d, r, 1.0), r, r);
    r = fma(fma(-d, r, 1.0), r, r);
    return r;
}

// The verdicts of the descents (`info`) must not depend on how a floating-point compare treats a NaN -- one of these
// translation units is compiled with -fno-honor-nans, where `!(x > 0.0)` may be folded as if x were a number -- so
// they are decided on the bit pattern, in integer arithmetic.
// expo_bits: the exponent field of v in place (bits 20..30 of its high word); all ones <=> v is +-Inf or a NaN.
// An accumulator `e = max(e, expo_bits(v))` over the values a kernel stores is all ones at the end iff one of them
// was not finite: two integer operations per value, no compare, no branch.
// (expo_bits is for the units compiled with IEEE semantics -- tvlqr, boxqp, boxqp_values: it sits in their step loops
// and stays transparent to the scheduler.  Under -fno-honor-nans the compiler knows a double "is no NaN", sees through
// the cast and folds the test to "is infinite"; the two predicates below therefore pass the bits through an opaque
// register move first, as the sample pass does under -ffinite-math-only (smooth_common.hpp), and hold in every unit.)
constexpr unsigned kExpoOnes = 0x7ff00000u;
__device__ __forceinline__ unsigned expo_bits(double v) { return (unsigned)__double2hiint(v) & kExpoOnes; }
__device__ __forceinline__ bool nonfinite_bits(double v) {
    unsigned hi = (unsigned)__double2hiint(v);
    asm("" : "+v"(hi));
    return (hi & kExpoOnes) == kExpoOnes;
}

// The same test for SEVERAL pivots at one compare (the matrix-core active-set kernel tests two to four per backward
// step, on a lone wave that pays for every instruction): pivot_word(v) < kPivotBad <=> v is a positive, finite, NORMAL
// number -- the high word minus the smallest normal exponent wraps zero and denormals (a pivot below 2.2e-308 is no
// pivot) to the top of the unsigned range, where the negative numbers, the infinities and the NaNs already are -- so
// max over the pivots' words < kPivotBad <=> all of them are good: a subtraction and a maximum per pivot.
constexpr unsigned kPivotBad = 0x7fe00000u;
__device__ __forceinline__ unsigned pivot_word(double v) {
    unsigned hi = (unsigned)__double2hiint(v);
    asm("" : "+v"(hi));
    return hi - 0x00100000u;
}

// lane `src_lane` (wave-uniform) to every lane
__device__ __forceinline__ double readlane_f64(double v, int src_lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src_lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src_lane);
    return __hiloint2double(hi, lo);
}

// lane N of every 16-lane row to all lanes of that row (DPP row_newbcast; checked on gfx950: tools/microbench)
template <int N>
__device__ __forceinline__ double row_bcast_f64(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    // (bound_ctrl set: every lane has a valid source, and with it the compiler need not initialise the destination --
    // it emitted a v_mov of zero per word and broadcast otherwise)
    lo = __builtin_amdgcn_update_dpp(0, lo, 0x150 + N, 0xf, 0xf, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, 0x150 + N, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

// wave-wide maximum / minimum, the result in every lane (six shuffles through the LDS crossbar)
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = fmax(v, __shfl_xor(v, s, 64));
    return v;
}
__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = fmin(v, __shfl_xor(v, s, 64));
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = max(v, __shfl_xor(v, s, 64));
    return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = min(v, __shfl_xor(v, s, 64));
    return v;
}

// dst = half_scale (src + src'), n x n row major, the elements dealt over the wave's lanes: only the symmetric part
// of a weight enters a quadratic form.  half_scale = 0.5, or 0.5 alpha where the weight carries a factor.
__device__ __forceinline__ void sym_part(double* dst, const double* src, int n, double half_scale, int lane) {
    for (int q = lane; q < n * n; q += 64) {
        const int i = q / n, j = q % n;
        dst[q] = half_scale * (src[q] + src[j * n + i]);
    }
}
