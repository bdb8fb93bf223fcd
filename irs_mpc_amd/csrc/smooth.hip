// Randomised-smoothing linearisation: get_TV_matrices of
//   irs_lqr/irs_lqr_zero_order.py:38-63   (ZERO_ORDER_AB)
//   irs_lqr/irs_lqr_first_order.py:28-54  (FIRST_ORDER)
//   irs_lqr/quasistatic_dynamics.py:242-266 (ZERO_ORDER_B, u-only noise)
//   irs_lqr/irs_lqr_exact.py:15-31        (exact)
// as ONE launch: a streaming map-reduce over the (T x N) grid of independent one-step
// samples whose last-arriving workgroup per timestep finishes the job.
//
//   smooth_kernel   grid (nblk, T) x 256 threads.
//     1. every lane streams its samples' z=[dx|du] (f32, vector loads, consecutive
//        lanes read consecutive records), evaluates the model functor in f32 and
//        accumulates the P sufficient statistics of its timestep in registers;
//     2. the workgroup transpose-reduces them with wave shuffles + one LDS hop and
//        publishes its P partial sums (write-through stores), then takes a ticket on
//        the timestep's arrival counter;
//     3. the workgroup that draws the last ticket of timestep t re-reads the nblk
//        partials in a FIXED order (f64) -> sums[t][P]   (deterministic: no float
//        atomics, the arrival order never changes the summation order);
//     4. (single-GPU path) its first wave solves the Jacobi-scaled normal equations
//        by Cholesky in f64 -> A_t, B_t and c_t = f(x_t,u_t) - A_t x_t - B_t u_t.
//   With several GPUs step 4 is a separate launch (smooth_finalize_kernel) after the
//   all-reduce of `sums`.
//
// Which lane reads which sample is planned on the host in ONE place, smooth_geometry() of smooth_api.hip (reported by
// irs_smooth_geometry, restated loop by loop in oracle/smooth_cases.py).  This file holds the kernels and their
// launches (the interface at its end, declared in smooth_common.hpp); every entry point, check and plan is there.
// smooth_kernel itself is smooth_kernel.inc, which smooth_batch.hip compiles a second time for B problems per launch.
//
// Inter-workgroup hand-off follows cdna_hip_programming.md Guideline 16: partials are
// stored sc1 (agent-scope relaxed atomic stores), every storing wave drains vmcnt, the
// workgroup barriers, one lane adds to the counter; the consumer does one agent-scope
// acquire + vmcnt(0) + barrier before any load of the partials.
#include "smooth_common.hpp"

namespace {

#include "smooth_kernel.inc"

// Stand-alone solve (after an all-reduce of `sums`): one wave per timestep.
template <class Model, int MODE>
__global__ __launch_bounds__(64) void smooth_finalize_kernel(SmoothArgs a) {
    __shared__ FinalizeLds<Model, MODE> fin;
    const int t = blockIdx.x;
    // a.fnom (optional): the f64 nominal steps a preceding irs_smooth_accumulate left in its workspace
    const double* fnom = (nominal_in_wg0<Model, MODE>() && a.fnom) ? a.fnom + (size_t)t * SmoothTraits<Model, MODE>::n
                                                                    : nullptr;
    finalize_timestep<Model, MODE>(a.p, a.x_trj, a.u_trj, a.sums + (size_t)t * SmoothTraits<Model, MODE>::P,
                                   a.n_total, t, threadIdx.x, fin, a.At, a.Bt, a.ct, a.info, fnom);
}

template <class Model>
__global__ __launch_bounds__(64) void exact_linearize_kernel(ModelParams p, const double* x_trj,
                                                             const double* u_trj, double* At, double* Bt,
                                                             double* ct, int T) {
    constexpr int n = Model::NX, m = Model::NU, d = n + m;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    double x[n], u[m], f[n], J[n * d];
#pragma unroll
    for (int i = 0; i < n; ++i) x[i] = x_trj[(size_t)t * n + i];
#pragma unroll
    for (int j = 0; j < m; ++j) u[j] = u_trj[(size_t)t * m + j];
    model_jacobian<Model, double>(p, x, u, f, J);
#pragma unroll
    for (int i = 0; i < n; ++i) {
        double c = f[i];
#pragma unroll
        for (int k = 0; k < n; ++k) {
            At[((size_t)t * n + i) * n + k] = J[i * d + k];
            c -= J[i * d + k] * x[k];
        }
#pragma unroll
        for (int k = 0; k < m; ++k) {
            Bt[((size_t)t * n + i) * m + k] = J[i * d + n + k];
            c -= J[i * d + n + k] * u[k];
        }
        ct[(size_t)t * n + i] = c;
    }
}

template <int n, int m>
__global__ void rng_samples_kernel(float* dx, float* du, SmoothArgs a) {
    constexpr int d = n + m;
    const int t = blockIdx.y;
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.N) return;
    const unsigned long long gidx = a.sample_offset + (unsigned long long)s;
    float z[(d + 3) / 4 * 4];
#pragma unroll
    for (int j = 0; j < (d + 3) / 4; ++j) philox_normal4(gidx, (unsigned)t, (unsigned)j, a.iter, a.seed, z + 4 * j);
    const size_t row = (size_t)t * a.N + s;
#pragma unroll
    for (int i = 0; i < n; ++i) dx[row * n + i] = z[i] * a.std[i];
#pragma unroll
    for (int j = 0; j < m; ++j) du[row * m + j] = z[n + j] * a.std[n + j];
}

template <class Model, int MODE, int BLOCK>
void launch_smooth_b(const SmoothArgs& a, bool rng, bool fuse, hipStream_t st) {
    dim3 grid(a.nblk, a.T), block(BLOCK);
    if (rng) {
        if (fuse) hipLaunchKernelGGL((smooth_kernel<Model, MODE, true, true, BLOCK>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((smooth_kernel<Model, MODE, true, false, BLOCK>), grid, block, 0, st, a);
    } else {
        if (fuse) hipLaunchKernelGGL((smooth_kernel<Model, MODE, false, true, BLOCK>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((smooth_kernel<Model, MODE, false, false, BLOCK>), grid, block, 0, st, a);
    }
}

template <class Model, int MODE>
void launch_smooth_m(const SmoothArgs& a, bool rng, bool fuse, hipStream_t st) {
    if constexpr (SmoothTraits<Model, MODE>::LIGHT) {
        if (a.block == kBigBlock) { launch_smooth_b<Model, MODE, kBigBlock>(a, rng, fuse, st); return; }
    }
    launch_smooth_b<Model, MODE, kBlock>(a, rng, fuse, st);
}

}  // namespace

// ---- the launch interface (smooth_common.hpp): what smooth_api.hip calls once a call is checked and planned ----------

int irs_smooth_launch(int model, int mode, const SmoothArgs& a, bool rng, bool fuse, hipStream_t st) {
    int rc = IRS_ERR_UNSUPPORTED;
    IRS_DISPATCH_MODEL(model, IRS_DISPATCH_MODE(mode, { launch_smooth_m<Model, MODE>(a, rng, fuse, st); rc = IRS_OK; }));
    return rc;
}

// every registered model's (NX, NU) in turn; the macro's refusal of the first id past the last model ends the search
int irs_rng_samples_launch(int n, int m, float* dx, float* du, const SmoothArgs& a, hipStream_t st) {
    for (int model = 0;; ++model) {
        IRS_DISPATCH_MODEL(model, {
            if (Model::NX == n && Model::NU == m) {
                hipLaunchKernelGGL((rng_samples_kernel<Model::NX, Model::NU>), dim3((a.N + 255) / 256, a.T), dim3(256), 0, st,
                                   dx, du, a);
                return IRS_OK;
            }
        });
    }
}

int irs_smooth_finalize_launch(int model, int mode, const SmoothArgs& a, hipStream_t st) {
    int rc = IRS_ERR_UNSUPPORTED;
    IRS_DISPATCH_MODEL(model, IRS_DISPATCH_MODE(mode, {
        hipLaunchKernelGGL((smooth_finalize_kernel<Model, MODE>), dim3(a.T), dim3(64), 0, st, a);
        rc = IRS_OK;
    }));
    return rc;
}

int irs_exact_linearize_launch(int model, const ModelParams& p, const double* x_trj, const double* u_trj, double* At,
                               double* Bt, double* ct, int T, hipStream_t st) {
    IRS_DISPATCH_MODEL(model, {
        hipLaunchKernelGGL((exact_linearize_kernel<Model>), dim3((T + 63) / 64), dim3(64), 0, st, p, x_trj, u_trj, At, Bt,
                           ct, T);
    });
    return IRS_OK;
}
