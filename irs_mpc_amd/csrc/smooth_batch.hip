// The general sample pass (smooth_kernel.inc) over B problems in ONE launch: grid (nblk, B T), row b T + t is time step
// t of problem b.  Served: the analytic models (pendulum, quadrotor, bicycle, three cart) in the modes that perturb x
// and u, with device-drawn samples and the fused solve -- what IrsLqrBatch needs.  Every row gets the single call's
// launch geometry, Philox counters and fixed summation order (SmoothRow, smooth_common.hpp); the results equal the
// single call's up to f32 rounding, not by contract bit for bit: this unit is built with smooth.o's flags (SLP
// vectorisation under -ffp-contract=fast), and the row's view in front of the body may change which products fuse.
// A translation unit of its own so that smooth.o's single-problem kernels stay the code they were.
#define IRS_SMOOTH_KERNEL_BATCH
#include "smooth_common.hpp"

namespace {

#include "smooth_kernel.inc"

// device-drawn samples, fused solve, the 256-thread workgroups the planner gives every drawn pass
template <class Model>
int launch_batch(int mode, const SmoothArgs& a, const SmoothBatch& bat, int B, hipStream_t st) {
    const dim3 grid(a.nblk, B * a.T), block(kBlock);
    if (mode == IRS_SMOOTH_ZERO_ORDER_AB)
        hipLaunchKernelGGL((smooth_kernel<Model, IRS_SMOOTH_ZERO_ORDER_AB, true, true, kBlock>), grid, block, 0, st, a, bat);
    else
        hipLaunchKernelGGL((smooth_kernel<Model, IRS_SMOOTH_FIRST_ORDER, true, true, kBlock>), grid, block, 0, st, a, bat);
    return IRS_OK;
}

}  // namespace

int irs_smooth_launch_batch(int model, int mode, const SmoothArgs& a, const SmoothBatch& bat, int B, hipStream_t st) {
    if (a.block != kBlock || (mode != IRS_SMOOTH_ZERO_ORDER_AB && mode != IRS_SMOOTH_FIRST_ORDER)) return IRS_ERR_UNSUPPORTED;
    switch (model) {
        case IRS_MODEL_PENDULUM: return launch_batch<PendulumModel>(mode, a, bat, B, st);
        case IRS_MODEL_QUADROTOR: return launch_batch<QuadrotorModel>(mode, a, bat, B, st);
        case IRS_MODEL_BICYCLE: return launch_batch<BicycleModel>(mode, a, bat, B, st);
        case IRS_MODEL_THREE_CART: return launch_batch<ThreeCartModel>(mode, a, bat, B, st);
        default: return IRS_ERR_UNSUPPORTED;
    }
}
