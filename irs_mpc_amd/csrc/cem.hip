// Cross-entropy-method baseline: CrossEntropyMethod.local_descent (irs_lqr/cem.py:151-184).
//   1. roll out every candidate control sequence u_cand[b] (B of them) for T steps on the
//      true dynamics and evaluate its cost            (cem.py:163-168; the ONLY place the
//      reference batches multi-step rollouts)         -> cem_rollout_kernel, one lane per b
//   2. keep the n_elite cheapest (np.argpartition, :173) -> cem_select_kernel: radix select
//      on order-preserving 64-bit keys + ordered compaction (deterministic)
//   3. refit mean / std over the elites (:178-180)      -> cem_refit_kernel
//   4. roll out the mean (:182)                          -> rollout_kernel (tvlqr.hip)
// All arithmetic in f64: rollout costs only rank the candidates, but ties broken by f32
// noise would change the elite set and hence the refit.
//
// Device-resident form (irs_cem_*_drawn, irs_cem_iterate): the candidate tensor is never stored.  Candidate b,
// step t, component j is a pure function of (seed, iter, sample_offset + b, t, j) -- cem_candidate below -- so the
// rollout draws its candidate in the lane as it goes and the refit regenerates only the n_elite winners from their
// indices.  The stream is the `du` stream of oracle.irs_oracle.device_gaussian_samples(T, B, 0, m, [], ones(m), seed,
// iter, sample_offset) with axes (T, B, m) -> (B, T, m), scaled by std and shifted by mean in f64.  It deliberately
// REUSES the counters of the smoothing generator (csrc/philox.hpp): no program here runs CEM and a smoothing pass
// with the same (seed, iter), so there is no second keying.  It is that generator with the radius of the rare pairs
// with u1 -> 1 formed from 1 - u1 (philox_normal4<true>): the candidates are held to the f64 restatement element by
// element (std (2e-5 |z| + 2e-6)), which the f32 rounding of u1 next to 1 misses about once in 3e4 pairs.
//
// Model-free form (irs_cem_values_stage[_drawn]): for a system that is a torch callable, step 1 is T + 1 launches of
// cem_values_stage_kernel -- the time-loop body of cem_rollout_kernel without the dynamics -- with the callable
// stepping all B states between them; steps 2-3 are the kernels above, which never see a Model.
//
// This file holds the kernels and, at its end, the launches cem.hpp declares; the extern "C" entries and their checks
// are cem_api.hip.
#include "boxqp.hpp"      // has_u_into_x
#include "cem.hpp"
#include "philox.hpp"

namespace {

// The one statement of the candidate stream.  An explicit fma: the rollout, the refit and the debug writer get the
// same bits whatever the compiler contracts around it.
__device__ __forceinline__ double cem_candidate(double mean, double std, float z) { return fma(std, (double)z, mean); }

// Where a rollout lane gets its candidate from.  Supplied: the (B,T,m) tensor of the host-draw path.
// lane(b, T, m): what the lane keeps across the time loop; row<m>(lane, t, u): its controls of step t.
struct CemSupplied {
    const double* __restrict__ u_cand;
    using Lane = const double*;
    __device__ __forceinline__ Lane lane(int b, int T, int m) const { return u_cand + (size_t)b * T * m; }
    template <int m>
    __device__ __forceinline__ void row(Lane ub, int t, double* u) const {
#pragma unroll
        for (int j = 0; j < m; ++j) u[j] = ub[(size_t)t * m + j];
    }
};

// Drawn: ceil(m/4) Philox calls per (b, t); mean / std rows are uniform addresses (scalar loads), no per-candidate
// memory is read.
struct CemDrawn {
    const double* __restrict__ mean;   // (T,m)
    const double* __restrict__ std;    // (T,m)
    uint64_t seed, sample_offset;
    uint32_t iter;
    using Lane = uint64_t;             // the candidate's global index
    __device__ __forceinline__ Lane lane(int b, int, int) const { return sample_offset + (uint64_t)b; }
    template <int m>
    __device__ __forceinline__ void row(Lane gidx, int t, double* u) const {
#pragma unroll
        for (int blk = 0; blk < (m + 3) / 4; ++blk) {
            float z[4];
            philox_normal4<true>(gidx, (uint32_t)t, (uint32_t)blk, iter, seed, z);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int j = 4 * blk + c;
                if (j < m) u[j] = cem_candidate(mean[(size_t)t * m + j], std[(size_t)t * m + j], z[c]);
            }
        }
    }
    // one component, m known at run time (refit, debug writer)
    __device__ __forceinline__ double at(int m, int b, int t, int j) const {
        float z[4];
        philox_normal4<true>(sample_offset + (uint64_t)b, (uint32_t)t, (uint32_t)(j >> 2), iter, seed, z);
        const int c = j & 3;
        const float zc = c == 0 ? z[0] : c == 1 ? z[1] : c == 2 ? z[2] : z[3];
        return cem_candidate(mean[(size_t)t * m + j], std[(size_t)t * m + j], zc);
    }
};

template <class Model, class Src>
__global__ __launch_bounds__(256) void cem_rollout_kernel(ModelParams p, int T, int B, Src src,
                                                          const double* __restrict__ x0,
                                                          const double* __restrict__ Q,
                                                          const double* __restrict__ R,
                                                          const double* __restrict__ xd_trj,
                                                          double* __restrict__ costs) {
    constexpr int n = Model::NX, m = Model::NU;
    __shared__ double Qs[n * n];
    __shared__ double Rs[m * m];
    for (int q = threadIdx.x; q < n * n; q += blockDim.x) Qs[q] = Q[q];
    for (int q = threadIdx.x; q < m * m; q += blockDim.x) Rs[q] = R[q];
    __syncthreads();
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double x[n], u[m], xn[n];
#pragma unroll
    for (int i = 0; i < n; ++i) x[i] = x0[i];
    const typename Src::Lane ub = src.lane(b, T, m);
    double cost = 0.0;
    unsigned warm_set = ~0u;          // active set of the previous contact step (exact step QPs only)
    for (int t = 0; t <= T; ++t) {
        // (x_t - xd_t)' Q (x_t - xd_t); the terminal term also uses Q (cem.py:138-139)
        const double* xd = xd_trj + (size_t)t * n;      // uniform address: scalar loads
        double e[n];
#pragma unroll
        for (int i = 0; i < n; ++i) e[i] = x[i] - xd[i];
#pragma unroll
        for (int i = 0; i < n; ++i) {
            double r = 0.0;
#pragma unroll
            for (int j = 0; j < n; ++j) r += Qs[i * n + j] * e[j];
            cost += e[i] * r;
        }
        if (t == T) break;
        src.template row<m>(ub, t, u);
#pragma unroll
        for (int i = 0; i < m; ++i) {
            double r = 0.0;
#pragma unroll
            for (int j = 0; j < m; ++j) r += Rs[i * m + j] * u[j];
            cost += u[i] * r;
        }
        irs_step_along<Model>(p, x, u, xn, &warm_set);
#pragma unroll
        for (int i = 0; i < n; ++i) x[i] = xn[i];
    }
    costs[b] = cost;
}

// CrossEntropyMethodQuasistatic.local_descent steps 1-2 (irs_lqr/cem_quasistatic.py:186-200): the
// candidate cost is IrsLqrQuasistatic's eval_cost (:124-165) -- state error with Q, TERMINAL Qd,
// input cost on du_t = u_t - u_{t-1} with du_0 = u_0 - x_0[indices_u_into_x].
template <class Model, class Src>
__global__ __launch_bounds__(64) void cem_rollout_quasistatic_kernel(ModelParams p, int T, int B, Src src,
                                                                     const double* __restrict__ x0,
                                                                     const double* __restrict__ Q,
                                                                     const double* __restrict__ Qd,
                                                                     const double* __restrict__ R,
                                                                     const double* __restrict__ xd_trj,
                                                                     double* __restrict__ costs) {
    constexpr int n = Model::NX, m = Model::NU;
    __shared__ double Qs[n * n];
    __shared__ double Qds[n * n];
    __shared__ double Rs[m * m];
    for (int q = threadIdx.x; q < n * n; q += blockDim.x) { Qs[q] = Q[q]; Qds[q] = Qd[q]; }
    for (int q = threadIdx.x; q < m * m; q += blockDim.x) Rs[q] = R[q];
    __syncthreads();
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double x[n], u[m], up[m], xn[n];
#pragma unroll
    for (int i = 0; i < n; ++i) x[i] = x0[i];
#pragma unroll
    for (int j = 0; j < m; ++j) up[j] = x0[Model::u_into_x(j)];
    const typename Src::Lane ub = src.lane(b, T, m);
    double cost = 0.0;
    unsigned warm_set = ~0u;          // active set of the previous contact step (exact step QPs only)
    for (int t = 0; t <= T; ++t) {
        const double* xd = xd_trj + (size_t)t * n;
        const double* W = t == T ? Qds : Qs;
        double e[n];
#pragma unroll
        for (int i = 0; i < n; ++i) e[i] = x[i] - xd[i];
#pragma unroll
        for (int i = 0; i < n; ++i) {
            double r = 0.0;
#pragma unroll
            for (int j = 0; j < n; ++j) r += W[i * n + j] * e[j];
            cost += e[i] * r;
        }
        if (t == T) break;
        double dv[m];
        src.template row<m>(ub, t, u);
#pragma unroll
        for (int j = 0; j < m; ++j) { dv[j] = u[j] - up[j]; up[j] = u[j]; }
#pragma unroll
        for (int i = 0; i < m; ++i) {
            double r = 0.0;
#pragma unroll
            for (int j = 0; j < m; ++j) r += Rs[i * m + j] * dv[j];
            cost += dv[i] * r;
        }
        irs_step_along<Model>(p, x, u, xn, &warm_set);
#pragma unroll
        for (int i = 0; i < n; ++i) x[i] = xn[i];
    }
    costs[b] = cost;
}

// ---- model-free rollout: one stage of B candidate rollouts, the plant stepped by the caller between launches ----
// cem_rollout_kernel with the dynamics taken out (TorchDeviceModel.cem_rollout_costs: the torch callable steps all B
// states between two stages).  Stage t of candidate b: costs[b] (+)= e' Q e + u' R u with e = x[b] - xd_t and u the
// candidate's control of step t, which is also written to u_t[b] for the callable; the terms are added in the order
// of cem_rollout_kernel's time loop, so equal states give equal bits.  Stage 0 writes costs, stage T has no control.
//
// One lane per candidate, n <= 32 and m <= 16 at run time.  A lane's row of x is n doubles at stride n: read by the
// lane itself, a wave's load would touch 64 rows with 8 bytes of each.  The workgroup's kStageBlock rows are one
// contiguous range of x, so the workgroup reads that range linearly -- lane i at base + 8 i, 512 bytes a wave and
// instruction -- into an LDS tile and every lane then works on its row there; u_t leaves the same way.  Rows are
// pitched to an odd number of doubles: the 32 lanes of an LDS access group then sit on 32 distinct bank pairs.
// Eight bytes a lane, not sixteen: the range starts at row b0 of a tensor the C ABI only knows to be 8-byte aligned,
// and the stage is bound by its launch, not its loads (B (n + m + 2) doubles: 1.6 MB at B = 50 000, n = 2, m = 1).
constexpr int kStageBlock = 128;

__host__ __device__ constexpr int stage_pitch(int w) { return w | 1; }

// Q (n n) | R (m m) | xd_t (n) | e tile (kStageBlock, pitch n) | u tile (kStageBlock, pitch m): 61 696 bytes at most
size_t stage_lds_bytes(int n, int m) {
    return sizeof(double) * (size_t)(n * n + m * m + n + kStageBlock * (stage_pitch(n) + stage_pitch(m)));
}

// The controls of step t of candidates b0 .. b0 + rows into the tile us (pitch mp) and out to u_t (B,m).
// Supplied: a row is m consecutive doubles at stride T m; thread q takes element q of the (rows, m) block, so a
// wave reads whole rows and writes u_t linearly -- the value stored is the value loaded.
__device__ __forceinline__ void stage_controls(const CemSupplied& src, int m, int mp, int T, int t, int b0, int rows,
                                               double* __restrict__ us, double* __restrict__ u_t) {
    for (int q = threadIdx.x; q < rows * m; q += kStageBlock) {
        const int r = q / m, j = q - r * m;
        const double v = src.u_cand[((size_t)(b0 + r) * T + t) * m + j];
        us[r * mp + j] = v;
        u_t[(size_t)b0 * m + q] = v;
    }
}

// Drawn: the lane draws its own row (ceil(m/4) Philox calls, as CemDrawn::row with m known at run time: the same
// counters, the same cem_candidate), the workgroup then writes the tile out linearly.
__device__ __forceinline__ void stage_controls(const CemDrawn& src, int m, int mp, int, int t, int b0, int rows,
                                               double* __restrict__ us, double* __restrict__ u_t) {
    const int r = threadIdx.x;
    if (r < rows) {
        const uint64_t gidx = src.lane(b0 + r, 0, 0);
        for (int blk = 0; 4 * blk < m; ++blk) {
            float z[4];
            philox_normal4<true>(gidx, (uint32_t)t, (uint32_t)blk, src.iter, src.seed, z);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int j = 4 * blk + c;
                if (j < m) us[r * mp + j] = cem_candidate(src.mean[(size_t)t * m + j], src.std[(size_t)t * m + j], z[c]);
            }
        }
    }
    __syncthreads();
    for (int q = threadIdx.x; q < rows * m; q += kStageBlock) {
        const int rr = q / m;
        u_t[(size_t)b0 * m + q] = us[rr * mp + (q - rr * m)];
    }
}

template <class Src>
__global__ __launch_bounds__(kStageBlock) void cem_values_stage_kernel(int n, int m, int T, int B, int t, Src src,
                                                                       const double* __restrict__ x,
                                                                       const double* __restrict__ Q,
                                                                       const double* __restrict__ R,
                                                                       const double* __restrict__ xd_trj,
                                                                       double* __restrict__ u_t,
                                                                       double* __restrict__ costs) {
    extern __shared__ double stage_lds[];
    const int np = stage_pitch(n), mp = stage_pitch(m);
    double* Qs = stage_lds;
    double* Rs = Qs + n * n;
    double* xds = Rs + m * m;
    double* es = xds + n;
    double* us = es + kStageBlock * np;
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * kStageBlock;
    const int rows = min(kStageBlock, B - b0);
    for (int q = tid; q < n * n; q += kStageBlock) Qs[q] = Q[q];
    for (int q = tid; q < m * m; q += kStageBlock) Rs[q] = R[q];
    for (int q = tid; q < n; q += kStageBlock) xds[q] = xd_trj[(size_t)t * n + q];
    const double* xb = x + (size_t)b0 * n;
    for (int q = tid; q < rows * n; q += kStageBlock) {
        const int r = q / n;
        es[r * np + (q - r * n)] = xb[q];
    }
    if (t < T) stage_controls(src, m, mp, T, t, b0, rows, us, u_t);      // t is uniform: every thread or none
    __syncthreads();
    if (tid >= rows) return;
    double* e = es + tid * np;
    const double* u = us + tid * mp;
    double cost = t == 0 ? 0.0 : costs[b0 + tid];
    for (int j = 0; j < n; ++j) e[j] -= xds[j];
    // (x_t - xd_t)' Q (x_t - xd_t); the terminal term also uses Q (cem.py:138-139).  No min / max, no compare: a
    // non-finite state makes this candidate's cost non-finite and no other's.
    for (int i = 0; i < n; ++i) {
        double r = 0.0;
        for (int j = 0; j < n; ++j) r += Qs[i * n + j] * e[j];
        cost += e[i] * r;
    }
    if (t < T) {
        for (int i = 0; i < m; ++i) {
            double r = 0.0;
            for (int j = 0; j < m; ++j) r += Rs[i * m + j] * u[j];
            cost += u[i] * r;
        }
    }
    costs[b0 + tid] = cost;
}

// Order-preserving map f64 -> u64 (NaN sorts last: a diverged rollout is never elite).
__device__ __forceinline__ unsigned long long cost_key(double c) {
    if (c != c) return ~0ull;
    unsigned long long b = (unsigned long long)__double_as_longlong(c);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

constexpr int kSelBlock = 1024;

// Single workgroup.  Finds the n_elite smallest costs; writes their indices in increasing
// index order (ties at the threshold: lowest indices first) -> elite_idx[0..n_elite).
__global__ __launch_bounds__(kSelBlock) void cem_select_kernel(const double* __restrict__ costs, int B,
                                                               int n_elite, int* __restrict__ elite_idx) {
    __shared__ unsigned int hist[256];
    __shared__ unsigned long long s_prefix;
    __shared__ int s_k, s_binc;
    __shared__ int scan[kSelBlock];
    __shared__ int s_less_total;
    const int tid = threadIdx.x;
    if (tid == 0) { s_prefix = 0ull; s_k = n_elite; }
    __syncthreads();
    // MSB-first radix select of the n_elite-th smallest key
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        if (tid < 256) hist[tid] = 0u;
        __syncthreads();
        const unsigned long long prefix = s_prefix;
        const unsigned long long mask = pass == 0 ? 0ull : (~0ull << (shift + 8));
        for (int i = tid; i < B; i += kSelBlock) {
            unsigned long long key = cost_key(costs[i]);
            if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 0xFF], 1u);
        }
        __syncthreads();
        if (tid < 64) {
            // the bin holding the k-th smallest candidate: inclusive prefix sums of the 256 counts, four per lane
            // (one wave; the serial scan by one lane was 8 x 256 dependent LDS reads of the kernel's 74 us)
            const int k = s_k;
            int c[4], run = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) { c[j] = (int)hist[4 * tid + j]; run += c[j]; }
            int incl = run;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int v = __shfl_up(incl, off, 64);
                if (tid >= off) incl += v;
            }
            int before = incl - run;                   // candidates in the bins of lower lanes
            const bool mine = before < k && k <= incl; // exactly one lane
            if (mine) {
                int bin = 4 * tid, kk = k - before;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (kk > c[j] && j < 3) { kk -= c[j]; ++bin; } else break;
                }
                s_k = kk;                              // rank inside the chosen bin
                s_prefix = prefix | ((unsigned long long)bin << shift);
                s_binc = (int)hist[bin];
            }
        }
        __syncthreads();
        // every key of the chosen bin is elite: no need to refine further -- the largest key of the bin is a valid
        // threshold (keys equal to it, if any, all belong)
        const bool whole_bin = s_k == s_binc && pass < 7;
        __syncthreads();                               // everyone has read the pair before lane 0 rewrites it
        if (whole_bin) {
            if (tid == 0) {
                s_prefix |= (1ull << shift) - 1ull;
                s_k = 0x7fffffff;
            }
            __syncthreads();
            break;
        }
    }
    const unsigned long long thr = s_prefix;           // key of the n_elite-th smallest cost (or the top of its bin)
    const int need_equal = s_k;                        // how many keys == thr belong to the elite
    // ordered compaction: thread owns a contiguous chunk of indices
    const int chunk = (B + kSelBlock - 1) / kSelBlock;
    const int lo = tid * chunk, hi = min(B, lo + chunk);
    int n_less = 0, n_eq = 0;
    for (int i = lo; i < hi; ++i) {
        unsigned long long key = cost_key(costs[i]);
        n_less += key < thr;
        n_eq += key == thr;
    }
    // exclusive scans of n_less and n_eq over the threads (two passes through one buffer)
    auto block_exclusive_scan = [&](int v, int* total) {
        scan[tid] = v;
        __syncthreads();
        for (int off = 1; off < kSelBlock; off <<= 1) {
            int add = tid >= off ? scan[tid - off] : 0;
            __syncthreads();
            scan[tid] += add;
            __syncthreads();
        }
        int incl = scan[tid];
        if (total != nullptr && tid == kSelBlock - 1) *total = incl;
        __syncthreads();
        return incl - v;
    };
    const int less_before = block_exclusive_scan(n_less, &s_less_total);
    const int eq_before = block_exclusive_scan(n_eq, nullptr);
    const int less_total = s_less_total;               // == n_elite - need_equal
    int wl = less_before, we = eq_before;
    for (int i = lo; i < hi; ++i) {
        unsigned long long key = cost_key(costs[i]);
        if (key < thr) {
            elite_idx[wl++] = i;                        // provisional slot; merged below
        } else if (key == thr) {
            if (we < need_equal) elite_idx[less_total + we] = i;
            ++we;
        }
    }
}

// u_new = mean over elites, std_new = population std over elites (np.mean / np.std, axis 0: two passes).
// One workgroup per 64 consecutive outputs q: lane = q (an elite's row is contiguous in q: coalesced), the 16 waves
// split the elites and meet in LDS, partial sums added in wave order (deterministic).  (One lane per q looping over
// all elites alone -- 2 x n_elite dependent loads -- took 118 us for 312 elites.)
// term(b, q) = component q of candidate b; called for q < Tm only.
constexpr int kRefitWaves = 16;
template <class Term>
__device__ __forceinline__ void cem_refit_body(Term term, const int* __restrict__ elite_idx, int n_elite, int Tm,
                                               double* __restrict__ u_new, double* __restrict__ std_new) {
    __shared__ double part[kRefitWaves][64];
    __shared__ double mean_s[64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = blockIdx.x * 64 + lane;
    const bool on = q < Tm;
    double s = 0.0;
    for (int e = wave; e < n_elite; e += kRefitWaves)
        s += on ? term(elite_idx[e], q) : 0.0;
    part[wave][lane] = s;
    __syncthreads();
    if (wave == 0) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < kRefitWaves; ++w) t += part[w][lane];
        mean_s[lane] = t / n_elite;
    }
    __syncthreads();
    const double mean = mean_s[lane];
    double v = 0.0;
    for (int e = wave; e < n_elite; e += kRefitWaves) {
        const double d = on ? term(elite_idx[e], q) - mean : 0.0;
        v += d * d;
    }
    __syncthreads();
    part[wave][lane] = v;
    __syncthreads();
    if (wave == 0 && on) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < kRefitWaves; ++w) t += part[w][lane];
        u_new[q] = mean;
        std_new[q] = sqrt(t / n_elite);
    }
}

__global__ __launch_bounds__(64 * kRefitWaves) void cem_refit_kernel(const double* __restrict__ u_cand,
                                                                     const int* __restrict__ elite_idx, int n_elite,
                                                                     int Tm, double* __restrict__ u_new,
                                                                     double* __restrict__ std_new) {
    cem_refit_body([=](int b, int q) { return u_cand[(size_t)b * Tm + q]; }, elite_idx, n_elite, Tm, u_new, std_new);
}

// The same sums with every term regenerated from (elite_idx[e], t, j) instead of loaded: one Philox call per term
// and pass.  Reads the OLD mean / std (src) and writes the new ones: u_new / std_new must not alias them.
__global__ __launch_bounds__(64 * kRefitWaves) void cem_refit_drawn_kernel(CemDrawn src, int m,
                                                                           const int* __restrict__ elite_idx,
                                                                           int n_elite, int Tm,
                                                                           double* __restrict__ u_new,
                                                                           double* __restrict__ std_new) {
    cem_refit_body([=](int b, int q) { return src.at(m, b, q / m, q % m); }, elite_idx, n_elite, Tm, u_new, std_new);
}

// Debug writer: the (B,T,m) tensor the drawn rollout and the drawn refit see (as irs_rng_samples for the smoothing
// stream).  One thread per element.
__global__ __launch_bounds__(256) void cem_candidates_kernel(CemDrawn src, int m, int Tm, size_t total,
                                                             double* __restrict__ u_cand) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int b = (int)(i / Tm), q = (int)(i - (size_t)b * Tm);
    u_cand[i] = src.at(m, b, q / m, q % m);
}

// ---- the launches of cem.hpp: a CemSource becomes the Src its kernels are compiled for, here and nowhere else ----
CemDrawn drawn(const CemSource& s) { return {s.mean, s.std, s.seed, s.sample_offset, s.iter}; }

// f(CemSupplied) or f(CemDrawn)
template <class F>
auto with_source(const CemSource& s, F f) {
    if (!s.drawn) return f(CemSupplied{s.u_cand});
    return f(drawn(s));
}

template <CemCost COST, class Src>
int launch_rollout(int model, const ModelParams& p, int T, int B, const Src& src, const double* x0, const double* Q,
                   const double* Qd, const double* R, const double* xd_trj, double* costs, hipStream_t st) {
    int rc = IRS_ERR_UNSUPPORTED;
    IRS_DISPATCH_MODEL(model, {
        if constexpr (COST == CemCost::Plain) {
            hipLaunchKernelGGL((cem_rollout_kernel<Model, Src>), dim3((B + 255) / 256), dim3(256), 0, st, p, T, B, src,
                               x0, Q, R, xd_trj, costs);
            rc = IRS_OK;
        } else if constexpr (has_u_into_x<Model>::value) {
            // one wave per workgroup: the contact step holds hundreds of f64 registers per lane
            hipLaunchKernelGGL((cem_rollout_quasistatic_kernel<Model, Src>), dim3((B + 63) / 64), dim3(64), 0, st, p,
                               T, B, src, x0, Q, Qd, R, xd_trj, costs);
            rc = IRS_OK;
        }
    });
    return rc;
}

}  // namespace

int irs_cem_launch_rollout(CemCost cost, int model, const ModelParams& p, int T, int B, const CemSource& src,
                           const double* x0, const double* Q, const double* Qd, const double* R, const double* xd_trj,
                           double* costs, hipStream_t st) {
    return with_source(src, [&](const auto& s) {
        return cost == CemCost::Plain
                   ? launch_rollout<CemCost::Plain>(model, p, T, B, s, x0, Q, nullptr, R, xd_trj, costs, st)
                   : launch_rollout<CemCost::Quasistatic>(model, p, T, B, s, x0, Q, Qd, R, xd_trj, costs, st);
    });
}

void irs_cem_launch_refit(int T, int m, int B, int n_elite, const CemSource& src, const double* costs, int* elite_idx,
                          double* u_new, double* std_new, hipStream_t st) {
    hipLaunchKernelGGL(cem_select_kernel, dim3(1), dim3(kSelBlock), 0, st, costs, B, n_elite, elite_idx);
    const int Tm = T * m;
    const dim3 grid((Tm + 63) / 64), block(64 * kRefitWaves);
    if (src.drawn)
        hipLaunchKernelGGL(cem_refit_drawn_kernel, grid, block, 0, st, drawn(src), m, elite_idx, n_elite, Tm, u_new,
                           std_new);
    else
        hipLaunchKernelGGL(cem_refit_kernel, grid, block, 0, st, src.u_cand, elite_idx, n_elite, Tm, u_new, std_new);
}

void irs_cem_launch_stage(int n, int m, int T, int B, int t, const CemSource& src, const double* x, const double* Q,
                          const double* R, const double* xd_trj, double* u_t, double* costs, hipStream_t st) {
    with_source(src, [&](const auto& s) {
        using Src = std::decay_t<decltype(s)>;
        hipLaunchKernelGGL((cem_values_stage_kernel<Src>), dim3((B + kStageBlock - 1) / kStageBlock), dim3(kStageBlock),
                           stage_lds_bytes(n, m), st, n, m, T, B, t, s, x, Q, R, xd_trj, u_t, costs);
    });
}

void irs_cem_launch_candidates(int T, int m, size_t total, const CemSource& src, double* u_cand, hipStream_t st) {
    hipLaunchKernelGGL(cem_candidates_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, drawn(src), m,
                       T * m, total, u_cand);
}

