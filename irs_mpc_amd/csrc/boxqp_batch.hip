// The ADMM kernel of the bounded TV-LQR (boxqp_kernel.inc) over B problems in ONE launch: grid B, one 64-lane workgroup
// per problem, blockIdx.x = b.  Served: the plain fixed-penalty form (DU = false, ADAPT = false) of the analytic models
// (pendulum, quadrotor, bicycle, three cart), with the records on chip or in slice b of a workspace -- what IrsLqrBatch
// needs.  Same source, same flags, one wave, f64: problem b's x_new, u_new, cost and info are the bits of the single
// kernel on problem b's inputs (tests/test_box_batch_gpu.py holds it to that).  A translation unit of its own so that
// boxqp.o's single-problem kernels stay the code they were.
#define IRS_BOX_KERNEL_BATCH
#include "boxqp.hpp"
#include "boxqp_layout.hpp"
#include "wave.hpp"

namespace {

#include "boxqp_kernel.inc"

template <class Model, bool HBM>
int launch_batch_kernel(const BoxArgs& a, double* recs, size_t bytes, int B, size_t rec_stride, hipStream_t st) {
    constexpr auto kern = box_descent_kernel<Model, false, HBM, false>;
    const int rc = irs_raise_lds_limit<kern>(bytes, "irs_tvlqr_box_descent_batch");
    if (rc != IRS_OK) return rc;
    hipLaunchKernelGGL(kern, dim3(B), dim3(64), bytes, st, a, recs, BoxAdapt{}, rec_stride);
    return IRS_OK;
}

template <class Model>
int launch_batch(const BoxArgs& a, const BoxPlan& p, double* ws, int B, size_t ws_stride, hipStream_t st) {
    return p.place == BoxPlace::AdmmHbm
               ? launch_batch_kernel<Model, true>(a, ws, p.lds, B, ws_stride / sizeof(double), st)
               : launch_batch_kernel<Model, false>(a, nullptr, p.lds, B, 0, st);
}

}  // namespace

int irs_box_admm_launch_batch(int model, const BoxArgs& a, const BoxPlan& p, double* ws, int B, size_t ws_stride,
                              hipStream_t st) {
    if (p.place != BoxPlace::AdmmLds && p.place != BoxPlace::AdmmHbm) return IRS_ERR_UNSUPPORTED;
    switch (model) {
        case IRS_MODEL_PENDULUM: return launch_batch<PendulumModel>(a, p, ws, B, ws_stride, st);
        case IRS_MODEL_QUADROTOR: return launch_batch<QuadrotorModel>(a, p, ws, B, ws_stride, st);
        case IRS_MODEL_BICYCLE: return launch_batch<BicycleModel>(a, p, ws, B, ws_stride, st);
        case IRS_MODEL_THREE_CART: return launch_batch<ThreeCartModel>(a, p, ws, B, ws_stride, st);
        default: return IRS_ERR_UNSUPPORTED;
    }
}
