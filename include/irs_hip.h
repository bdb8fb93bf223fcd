/*
 * irs_hip.h -- C ABI of libirs_hip.so, the MI355X (gfx950) implementation of the
 * iRS-LQR inner loop of hjsuh94/irs_mpc.
 *
 * The reference has no FFI: its hot path is Python calling NumPy / Drake.  Each
 * entry point below names the reference interface (file:line, relative to the
 * reference repo root) it replaces; INTEGRATION.md shows the ctypes stub a
 * reference maintainer would add.
 *
 * Conventions
 *  - Plain C: pointers and sizes only.  No allocation, no retained pointers, no
 *    host synchronisation inside any call: every call enqueues kernels on
 *    `stream` (a hipStream_t passed as void*; NULL = the default stream) and
 *    returns.  All calls are hipGraph-capturable.
 *  - Pointers marked DEV are device (HBM) pointers owned by the caller; pointers
 *    marked HOST are read during the call and not retained.
 *  - All matrices are C-contiguous row-major.  Trajectories, matrices, gains and
 *    costs are float64 (the reference computes in float64); the sample tensors
 *    dx/du, which carry all the bytes, are float32 and the per-sample dynamics
 *    evaluation runs in float32 (`dtype` of the path: f32).
 *  - The cost weights Q, Qd (n x n) and R (m x m) are dense and need not be symmetric:
 *    every entry point uses the symmetric part (W + W')/2, as Drake's quadratic costs do.
 *  - Return value: IRS_OK (0) or a negative irs_status; irs_last_error() returns
 *    a thread-local message.  Numerical failures inside kernels (non-SPD Gram or
 *    Hessian) are reported through the DEV `info` arrays, LAPACK style.
 *  - `params` HOST: model constants, params[0] = h (step size); see irs_model_info.
 *  - The verdict of a TV-LQR entry is its `info`, and the host classes trust that word alone.  Two rules hold at every
 *    descent entry and at irs_tvlqr_riccati (tests/test_descent_verdicts_gpu.py):
 *    V1, the step.  If exactly one step t* has a control Hessian that is not positive definite in the backward sweep --
 *      the Hessians being those of the P computed from the steps after t*, in the form the kernel factors (alpha R +
 *      B'PB; with the ADMM's rho/2 on the bounded components; [x; u_prev] for the position-controlled form) -- then
 *      info[0] == t* + 1: for every position of t*, every position of the failing pivot, every problem of a batch; a
 *      failing problem's neighbours keep their bits.  The first failure of the sweep is the one reported.
 *    V2, non-finite data.  A call that is handed a NaN or +-Inf in an element of At, Bt, ct, xd_trj or x0 that reaches
 *      one of its outputs never returns an all-clear.  Unbounded entries (irs_tvlqr_riccati, irs_tvlqr_descent,
 *      irs_tvlqr_descent_batch): 1 <= info[0] <= T + 1 -- t + 1 where a pivot caught it, T + 1 ("no such step:
 *      non-finite data", as irs_least_squares uses n + m + 1) where the pivots were fine but a stored gain or the
 *      realised cost is not finite.  Bounded entries (the ADMM, active-set, batch, lazy, adaptive and box_values
 *      descents): info[0] != 0 or info[2] != 0, the two words the host classes read -- a tail whose first control is not
 *      finite counts as not converged in info[2] (a clipped control can make the realised trajectory finite again; what
 *      never happens is three zero words), and a realised cost that is not finite gives info[0] = T + 1.  (Row 0 of
 *      xd_trj reaches the cost only: irs_tvlqr_riccati, which returns no cost, does not see it.  NOT covered: a bounded
 *      descent in which every tail that reads the poisoned step has its FIRST control pinned before the poison can reach
 *      it -- a caller-supplied active set (act_io) or enforced set that pins step 0 of those tails: the first control is
 *      then a finite bound, the multiplier tests are ordered compares a NaN fails, the tail reads as converged, and if
 *      the plant keeps the realised trajectory and cost finite the three words are zero.  The tests are made on the
 *      tail's first control and on the cost, not on its whole plan or its multipliers.)  Every test is made on
 *      bit patterns, in integer arithmetic: it does not depend on how a floating-point compare treats a NaN.
 */
#ifndef IRS_HIP_H
#define IRS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IRS_ABI_VERSION 1

typedef enum irs_status {
    IRS_OK = 0,
    IRS_ERR_INVALID_ARG = -1,
    IRS_ERR_HIP = -2,
    IRS_ERR_UNSUPPORTED = -3,
    IRS_ERR_WORKSPACE = -4
} irs_status;

/* Device models = the reference's DynamicalSystem plugins that exist as device
 * functors (irs_lqr/dynamical_system.py:1-66).                                  */
typedef enum irs_model_id {
    IRS_MODEL_PENDULUM = 0,   /* examples/pendulum/pendulum_dynamics.py:8-127; params = {h}            */
    IRS_MODEL_QUADROTOR = 1,  /* examples/quadrotor/quadrotor_dynamics.py:15-231;
                                 params = {h, m, L, g, Ixx, Iyy, Izz, kF, kM}                          */
    IRS_MODEL_BICYCLE = 2,    /* examples/bicycle/bicycle_dynamics.py:8-132; params = {h}              */
    IRS_MODEL_THREE_CART = 3, /* examples/three_cart/three_cart_dynamics.py:8-107 (scalar `dynamics`:
                                 contact by branching); params = {h, d}                                */
    IRS_MODEL_PLANAR_HAND = 4, /* examples/planar_hand (QuasistaticDynamics over the external simulator,
                                 irs_lqr/quasistatic_dynamics.py:136-164): planar quasi-dynamic contact,
                                 Anitescu convex step; x = [xo, ql1, qr1, yo, ql2, qr2, th] (the reference's order,
                                 planar_hand_analysis.py:61-67), u = [ql1, ql2, qr1, qr2] joint commands;
                                 params = {h, g, mass, R, mu, kp1, kp2, l1, l2, r_link, base_x, pgs_iters};
                                 Jacobian = the step QP's active-set derivative (the simulator's Dq_nextDq |
                                 Dq_nextDqa_cmd, quasistatic_dynamics.py:184-191); the sample-pass modes
                                 ZERO_ORDER_B / FIRST_ORDER perturb u only and return the decoupled (A,B) of
                                 irs_lqr_quasistatic.py:275-284.  PARITY UNPINNED.                       */
    IRS_MODEL_BOX_PIVOT = 5   /* examples/box_pivoting: a 1 m square box on the ground pivoted by a position-
                                 controlled disc; x = [x_h, x_b, y_h, y_b, th_b] (box_pivoting_analysis.py:53-64),
                                 u = commanded hand position; params = {h, g, mass, half, mu, kp, r_hand,
                                 pgs_iters}; same contact scheme and restrictions as the planar hand.       */
    , IRS_MODEL_BOX_ON_BOX = 6 /* examples/box_pushing/analysis/box_on_box.py:11-20: the reference's 1-D
                                 statement of the quasi-dynamic step (x = [x_a, x_u], u = commanded x_a;
                                 params = {h, m, k, pgs_iters}); pins the contact QP code the functors share */
    , IRS_MODEL_BOX_PUSH = 7  /* examples/box_pushing (box_pushing_setup.py:6-19): the box and disc of
                                 box_pivoting seen from above (no gravity, no ground, Kp = 500); x, u as there;
                                 params = {h, mass, inertia, half, mu, kp, r_hand, pgs_iters}.  PINNED by the
                                 simulator data examples/box_pushing/analysis/{xu,dxdu}_quasistatic.npy        */
    , IRS_MODEL_PLANAR_HAND_EXACT = 8 /* IRS_MODEL_PLANAR_HAND with the step QP solved EXACTLY (dual active-set
                                 method, csrc/contact_models.hpp) -- what the reference's simulator does (Gurobi) --
                                 instead of by pgs_iters projected sweeps; same params (pgs_iters ignored)      */
    , IRS_MODEL_BOX_PIVOT_EXACT = 9 /* IRS_MODEL_BOX_PIVOT with the step QP solved exactly, likewise           */
    , IRS_MODEL_BOX_PUSH_EXACT = 10 /* IRS_MODEL_BOX_PUSH with the step QP solved exactly, likewise            */
} irs_model_id;

/* Smoothing estimators.                                                         */
typedef enum irs_smooth_mode {
    IRS_SMOOTH_ZERO_ORDER_AB = 0, /* irs_lqr/irs_lqr_zero_order.py:38-63 (LSQ fit through N one-step evals) */
    IRS_SMOOTH_FIRST_ORDER = 1,   /* irs_lqr/irs_lqr_first_order.py:28-54 (mean of N sampled Jacobians); on a
                                     contact model: calc_AB_first_order, irs_lqr/quasistatic_dynamics.py:193-208
                                     (u-only noise, dx may be NULL; sums = (T, n*m): the B blocks; decoupled)  */
    IRS_SMOOTH_ZERO_ORDER_B = 2   /* irs_lqr/quasistatic_dynamics.py:242-266 (u-only noise: B by LSQ,
                                     A = exact Jacobian at the nominal point)                               */
} irs_smooth_mode;

int irs_abi_version(void);
const char *irs_last_error(void);

/* dim_x, dim_u and the number of model constants (`h, dim_x, dim_u` attributes of
 * irs_lqr/dynamical_system.py:8-10).                                             */
int irs_model_info(int model, int *dim_x, int *dim_u, int *n_params);

/* ---- DynamicalSystem plugin surface (irs_lqr/dynamical_system.py:12-66) ------ */

/* dynamics_batch (:24-38): Xn[b] = f(X[b], U[b]).  X (B,n), U (B,m), Xn (B,n) DEV f64. */
int irs_dynamics_batch(int model, const double *params, int n_params,
                       const double *X, const double *U, int B, double *Xn, void *stream);

/* jacobian_xu_batch (:53-66): J[b] = df/d[x,u] at (X[b],U[b]); J (B,n,n+m) DEV f64.
 * Forward-mode AD of the device functor, like the reference's forwarddiff/symbolic
 * Jacobians (quadrotor_dynamics.py:136-148, pendulum_dynamics.py:110-127); contact models:
 * the derivative of the step QP through its active constraints, contact geometry fixed =
 * QuasistaticDynamics.jacobian_xu (irs_lqr/quasistatic_dynamics.py:184-191).           */
int irs_jacobian_xu_batch(int model, const double *params, int n_params,
                          const double *X, const double *U, int B, double *J, void *stream);

/* Per-sample view of calc_AB_first_order on a contact model (irs_lqr/quasistatic_dynamics.py:193-208: the loop
 * body, one u-perturbation per lane): from the nominal x (n), u (m) DEV f64 and du (B,m) DEV f32, exactly what a
 * lane of the FIRST_ORDER sample pass evaluates in f32 -- Xn (B,n) the step from ((float)x, (float)u + du[b]),
 * Bs (B,n,m) the block Dq_nextDqa_cmd of its active-set derivative, active_mask (B) i32 bit i = contact row i
 * active.  Diagnostics: lets a test separate the samples whose active set differs between the f32 lanes and an
 * f64 evaluation from the rest.  IRS_ERR_UNSUPPORTED for analytic models.                                   */
int irs_contact_samples_f32(int model, const double *params, int n_params, const double *x, const double *u,
                            const float *du, int B, float *Xn, float *Bs, int *active_mask, void *stream);

/* IrsLqr.rollout + evaluate_cost (irs_lqr/irs_lqr.py:105-119, :121-137).
 * x0 (n), u_trj (T,m), Q (n,n), R (m,m), xd_trj (T+1,n) DEV f64 in;
 * x_trj (T+1,n), cost (1) DEV f64 out.  Terminal term uses Q (reference :135-136). */
int irs_rollout_cost(int model, const double *params, int n_params, int T,
                     const double *x0, const double *u_trj, const double *Q,
                     const double *R, const double *xd_trj, double *x_trj,
                     double *cost, void *stream);

/* IrsLqr.evaluate_cost (irs_lqr/irs_lqr.py:121-137) of a GIVEN (x_trj, u_trj) pair:
 * sum_t (x_t-xd_t)'Q(x_t-xd_t) + u_t'R u_t  +  (x_T-xd_T)'Q(x_T-xd_T).  Any n<=32, m<=16. */
int irs_evaluate_cost(int n, int m, int T, const double *x_trj, const double *u_trj,
                      const double *Q, const double *R, const double *xd_trj,
                      double *cost, void *stream);

/* ---- Randomised-smoothing linearisation (get_TV_matrices) -------------------- */

/* Length P of one timestep's sufficient statistics (z = the perturbed components, d = n+m):
 *   ZERO_ORDER_AB: d(d+1)/2 (upper Gram of z=[dx,du]) + d*n (z (f(x+dx,u+du)-f(x,u))')
 *   FIRST_ORDER  : n*d      (sum of Jacobians)
 *   ZERO_ORDER_B : m(m+1)/2 + m*n                                  (z = du)
 * Contact models (IRS_MODEL_PLANAR_HAND, IRS_MODEL_BOX_PIVOT; expensive step) use the layout
 *   [Gram | z (f(x+dx,u+du) - xb)' | sum of z],  P as above + d (resp. m),
 * xb = the f32-rounded x_t: the finalize step subtracts (sum z)(f(x,u) - xb)' with f(x,u) in f64, so
 * no lane of the sample pass evaluates the nominal step.  Sums of shards add in either layout.    */
int irs_sums_len(int model, int mode);

/* Bytes of DEV scratch the irs_smooth* calls need for (T, N) (T <= 1024).        */
size_t irs_smooth_workspace_bytes(int model, int mode, int T, int N);

/* The launch geometry the irs_smooth* calls use for (model, mode, T, N); rng != 0: device-drawn samples.  Makes
 * no launch and needs no device.  The sample pass launches exactly what this reports (one planner, csrc/smooth_api.hip:
 * smooth_geometry); like the launch it honours IRS_UG, read per call.  out[]:
 *   [0] family (irs_smooth_family): which sample loop runs
 *   [1] block   threads per workgroup        [2] nblk  workgroups per timestep (grid = nblk x T)
 *   [3] chunk0  samples of workgroup 0       [4] chunk samples of every later workgroup: workgroup b >= 1 owns
 *       [chunk0 + (b-1) chunk, chunk0 + b chunk) cut at N -- possibly empty.  Both 0 for the uniform-geometry
 *       family, which deals 64-sample blocks round robin to the nblk x 8 waves of a timestep instead
 *   [5] wg0_rr  trips of workgroup 0 dealt to all four of its waves before the last one sits out (INT_MAX: never)
 *   [6] branch (irs_smooth_plan): which contact re-planning set chunk0 / chunk      [7] 0 (reserved)           */
typedef enum {
    IRS_SMOOTH_FAMILY_LANES_LIGHT = 0,       /* strided lanes; 1024 threads and four samples per lane per trip when
                                                the samples are supplied and N is small                          */
    IRS_SMOOTH_FAMILY_LANES_HEAVY = 1,       /* strided lanes, one sample per trip, next row prefetched          */
    IRS_SMOOTH_FAMILY_GRAM_MATRIX_CORE = 2,  /* a wave per 64 samples, Gram by MFMA                              */
    IRS_SMOOTH_FAMILY_CONTACT_WAVE_DEALT = 3,/* contact step per lane, 64-sample blocks dealt to waves           */
    IRS_SMOOTH_FAMILY_CONTACT_PARKED = 4,    /* the same deal + unfinished samples parked in a per-wave ring     */
    IRS_SMOOTH_FAMILY_UNIFORM_GEOMETRY = 5   /* csrc/smooth_ug.hip                                               */
} irs_smooth_family;
typedef enum {
    IRS_SMOOTH_PLAN_NONE = 0,   /* chunk0 == chunk                                                               */
    IRS_SMOOTH_PLAN_TRIPS = 1,  /* balanced by 64-sample wave trips (wg0_rr finite)                              */
    IRS_SMOOTH_PLAN_COST = 2    /* workgroup 0 gives up a fixed number of samples per lane                       */
} irs_smooth_plan;
int irs_smooth_geometry(int model, int mode, int T, int N, int rng, int out[8]);

/* Zeroes the arrival counters at the head of a freshly allocated workspace.  Call
 * once per allocation; every irs_smooth* call leaves them zero again.  One call in
 * flight per workspace at a time.                                                */
int irs_workspace_init(void *workspace, size_t workspace_bytes, void *stream);

/* Whole get_TV_matrices in ONE launch (single-GPU path): sample pass + reduction +
 * least-squares solve.  Samples SUPPLIED: dx (T,N,n), du (T,N,m) DEV f32 -- what the
 * reference's `sampling(x_t,u_t,iter)` closure returned at each t, e.g.
 * examples/pendulum/pendulum_zero_order.py:38-43 ("identical seeds").
 * Outputs as irs_smooth_accumulate (sums) + irs_smooth_finalize (At,Bt,ct,info).
 * Kernels: csrc/smooth.hip (general sample pass), except IRS_MODEL_PLANAR_HAND_EXACT in the u-only modes
 * (IRS_SMOOTH_ZERO_ORDER_B, IRS_SMOOTH_FIRST_ORDER) -- quasistatic_dynamics.py:193-266, the state is not perturbed --
 * which run csrc/smooth_ug.hip: one dual Hessian per timestep, all 2^8 active-set maps tabulated in LDS, every
 * sample's step QP solved exactly by table rows.  Same arguments, statistics layout and results (to f32 rounding);
 * the environment variable IRS_UG=0 (read per call) selects the general kernel for comparison runs.             */
int irs_smooth(int model, const double *params, int n_params, int mode, int T, int N,
               const double *x_trj, const double *u_trj, const float *dx, const float *du,
               double *sums, double *At, double *Bt, double *ct, int *info,
               void *workspace, size_t workspace_bytes, void *stream);

/* Same with on-device Philox draws (see irs_smooth_accumulate_rng).              */
int irs_smooth_rng(int model, const double *params, int n_params, int mode, int T, int N,
                   const double *x_trj, const double *u_trj, const double *std_x,
                   const double *std_u, uint64_t seed, uint32_t iter, double *sums,
                   double *At, double *Bt, double *ct, int *info,
                   void *workspace, size_t workspace_bytes, void *stream);

/* The sample passes of B independent problems in ONE launch: irs_smooth_rng with a problem index, grid (nblk, B T).
 * Row (b, t) executes the instructions of the single call on problem b's inputs, so problem b's outputs are, bit for
 * bit, those of irs_smooth_rng(model, ..., T, N, x_trj_b, u_trj_b, NULL, std_u_b, seed_b, iter, ...):
 *   - every row gets the launch geometry irs_smooth_geometry(model, mode, T, N, 1) reports for the PER-PROBLEM (T, N)
 *     (nblk, block, chunk0, chunk, wg0_rr; IRS_UG is honoured per call, like the single entry); samples are dealt to
 *     waves in the same order and the partial sums are added in the same fixed order;
 *   - the Philox counters take the time step WITHIN the problem, problem b's seed, the shared `iter`, sample_offset 0;
 *   - every draw is scaled by problem b's std_u, converted f64 -> f32 by the round-to-nearest conversion the single
 *     entry applies on the host.
 * Served: what the uniform-geometry kernel (csrc/smooth_ug.hip) serves -- IRS_MODEL_PLANAR_HAND_EXACT in
 * IRS_SMOOTH_ZERO_ORDER_B and IRS_SMOOTH_FIRST_ORDER, the u-only modes (std_x does not exist), while IRS_UG is not 0.
 * The general kernel (csrc/smooth.hip: the other contact models, and the planar hand under IRS_UG=0) has no batched
 * form: its translation unit is SLP-vectorised under -ffp-contract=fast, and a problem index in front of its body
 * changed which products the compiler fuses, i.e. the last bits of the f32 sums.  (The analytic models
 * have a batched form of that kernel under another contract: irs_smooth_rng_general_batch below.)
 * In:  x_trj DEV f64, problem b's nominal states from x_trj + b x_stride (ELEMENTS), T rows of n read: x_stride =
 *      (T+1) n takes a (B,T+1,n) trajectory tensor as it is, T n stacked nominal points; u_trj likewise with u_stride
 *      >= T m; std_u (B,m) DEV f64; seed (B) DEV; iter shared by the problems.
 * Out: B contiguous blocks of the single call's outputs: sums (B,T,P), At (B,T,n,n), Bt (B,T,n,m), ct (B,T,n) DEV
 *      f64, info (B,T) DEV int.
 * Workspace (DEV, 256-byte aligned): B slices of the single-problem layout, each with its own arrival counters,
 * nominal steps and partial sums; problem b owns the bytes from b * round256(irs_smooth_workspace_bytes(model, mode,
 * T, N)), and irs_smooth_batch_workspace_bytes is B times that (0: model / mode not served, or B <= 0).
 * irs_smooth_batch_workspace_init zeroes the whole buffer, once per allocation -- and again before the buffer serves
 * another (model, mode, T, N), whose slices start elsewhere; every call leaves all counters zero again.  One call in
 * flight per workspace at a time.  No allocation, no host synchronisation: the call enqueues one
 * launch on `stream`.  Every argument error is decided before the first HIP call:
 *   IRS_ERR_INVALID_ARG  B, T or N <= 0; T > 1024; B T > 65535 (grid rows); a problem's partial sums beyond 4 GiB; a
 *                        null pointer; x_stride < T n or u_stride < T m; wrong n_params
 *   IRS_ERR_UNSUPPORTED  IRS_SMOOTH_ZERO_ORDER_AB, an analytic model (one with a Jacobian), an unknown model, a model
 *                        or setting (IRS_UG=0) that runs the general kernel
 *   IRS_ERR_WORKSPACE    workspace null, too small or not 256-byte aligned                                        */
size_t irs_smooth_batch_workspace_bytes(int model, int mode, int T, int N, int B);   /* no GPU is touched */
int irs_smooth_batch_workspace_init(void *workspace, size_t workspace_bytes, void *stream);
int irs_smooth_rng_batch(int model, const double *params, int n_params, int mode, int T, int N, int B,
                         const double *x_trj, long long x_stride, const double *u_trj, long long u_stride,
                         const double *std_u, const uint64_t *seed, uint32_t iter,
                         double *sums, double *At, double *Bt, double *ct, int *info,
                         void *workspace, size_t workspace_bytes, void *stream);

/* The same for the ANALYTIC models (pendulum, quadrotor, bicycle, three cart) in IRS_SMOOTH_ZERO_ORDER_AB and
 * IRS_SMOOTH_FIRST_ORDER: the general kernel (csrc/smooth.hip) over B T rows, grid (nblk, B T), device-drawn samples
 * and the fused solve.  Row (b, t) gets the geometry irs_smooth_geometry(model, mode, T, N, 1) plans for the
 * per-problem (T, N); its Philox counters take t within the problem, problem b's seed, the shared `iter` and
 * sample_offset 0, so problem b's DRAWS are those of irs_smooth_rng(model, ..., x_trj_b, u_trj_b, std_x_b, std_u_b,
 * seed_b, iter, ...); std_x (B,n) and std_u (B,m) DEV f64 are converted to f32 as the single entry converts them.
 * The contract is NOT bit equality with the single call: that translation unit is SLP-vectorised under
 * -ffp-contract=fast and a problem index in front of the body may change which f32 products fuse.  Problem b's sums,
 * At, Bt and ct equal the single call's up to f32 rounding and meet the tolerance against the f64 oracle on identical
 * samples that the single entry meets (tests/test_irs_lqr_batch_gpu.py).
 * Strides, outputs, workspace (B slices of the single layout, 256-byte aligned, zeroed once per allocation by
 * irs_smooth_general_batch_workspace_init; every call leaves all counters zero again) and the order of the checks:
 * as irs_smooth_rng_batch.  irs_smooth_general_batch_workspace_bytes = B * round256(irs_smooth_workspace_bytes(model,
 * mode, T, N)); 0: model / mode not served, or B <= 0.  Every argument error is decided before the first HIP call:
 *   IRS_ERR_INVALID_ARG  B, T or N <= 0; T > 1024; B T > 65535; a null pointer (std_x included); short strides; wrong
 *                        n_params
 *   IRS_ERR_UNSUPPORTED  a contact model (irs_smooth_rng_batch serves the planar hand), an unknown model,
 *                        IRS_SMOOTH_ZERO_ORDER_B
 *   IRS_ERR_WORKSPACE    workspace null, too small or not 256-byte aligned                                        */
size_t irs_smooth_general_batch_workspace_bytes(int model, int mode, int T, int N, int B);   /* no GPU is touched */
int irs_smooth_general_batch_workspace_init(void *workspace, size_t workspace_bytes, void *stream);
int irs_smooth_rng_general_batch(int model, const double *params, int n_params, int mode, int T, int N, int B,
                                 const double *x_trj, long long x_stride, const double *u_trj, long long u_stride,
                                 const double *std_x, const double *std_u, const uint64_t *seed, uint32_t iter,
                                 double *sums, double *At, double *Bt, double *ct, int *info,
                                 void *workspace, size_t workspace_bytes, void *stream);

/* Sample pass, samples SUPPLIED (parity mode; "identical seeds" = the host draws
 * them exactly as the reference's `sampling(x_t,u_t,iter)` closure does, e.g.
 * examples/pendulum/pendulum_zero_order.py:38-43).
 *   x_trj (T+1,n), u_trj (T,m) DEV f64; dx (T,N,n), du (T,N,m) DEV f32
 *   (dx may be NULL for ZERO_ORDER_B); sums (T,P) DEV f64 out.
 * N is the number of samples per timestep held by THIS device; sums of several
 * devices add (one all-reduce of `sums` replaces zmq_parallel_cmp/array_io.py:6-26). */
int irs_smooth_accumulate(int model, const double *params, int n_params, int mode,
                          int T, int N, const double *x_trj, const double *u_trj,
                          const float *dx, const float *du, double *sums,
                          void *workspace, size_t workspace_bytes, void *stream);

/* Sample pass with on-device Philox4x32-10 + Box-Muller draws (throughput mode):
 * z_c ~ N(0, std_c), std = [std_x | std_u] HOST (n+m); the stream is a pure function
 * of (seed, iter, t, sample_offset + i), so results do not depend on how samples
 * are split over devices.  Specification: oracle/irs_oracle.py:device_gaussian_samples. */
int irs_smooth_accumulate_rng(int model, const double *params, int n_params, int mode,
                              int T, int N, const double *x_trj, const double *u_trj,
                              const double *std_x, const double *std_u, uint64_t seed,
                              uint32_t iter, uint64_t sample_offset, double *sums,
                              void *workspace, size_t workspace_bytes, void *stream);

/* Debug/verification: writes the samples irs_smooth_accumulate_rng would draw.   */
int irs_rng_samples(int n, int m, int T, int N, const double *std_x, const double *std_u,
                    uint64_t seed, uint32_t iter, uint64_t sample_offset,
                    float *dx, float *du, void *stream);

/* Solve: sums (T,P) -> At (T,n,n), Bt (T,n,m), ct (T,n) DEV f64,
 * c_t = f(x_t,u_t) - A_t x_t - B_t u_t (irs_lqr_zero_order.py:59-62).
 * N_total = samples per timestep summed over all devices.
 * info (T) DEV int32: 0 ok, j>0 = Gram matrix not positive definite at pivot j.
 * ZERO_ORDER_AB solves the normal equations of compute_least_squares
 * (irs_lqr_zero_order.py:27-36) by Jacobi-scaled Cholesky in f64.                */
int irs_smooth_finalize(int model, const double *params, int n_params, int mode,
                        int T, long long N_total, const double *x_trj, const double *u_trj,
                        const double *sums, double *At, double *Bt, double *ct,
                        int *info, void *stream);

/* irs_smooth_finalize that may reuse work of the preceding irs_smooth_accumulate[_rng] call:
 * `workspace` = the workspace that call was given (same model, mode, T, x_trj, u_trj), or NULL.  For
 * contact models the accumulate launch leaves f(x_t,u_t) (f64, 400 serial PGS updates each) there,
 * evaluated by workgroup 0 of every timestep while the others sample; finalize then skips them.    */
int irs_smooth_finalize_ws(int model, const double *params, int n_params, int mode, int T,
                           long long N_total, const double *x_trj, const double *u_trj,
                           const double *sums, double *At, double *Bt, double *ct, int *info,
                           const void *workspace, size_t workspace_bytes, void *stream);

/* IrsLqrExact.get_TV_matrices (irs_lqr/irs_lqr_exact.py:15-31).                  */
int irs_exact_linearize(int model, const double *params, int n_params, int T,
                        const double *x_trj, const double *u_trj,
                        double *At, double *Bt, double *ct, void *stream);

/* ---- TV-LQR (irs_lqr/tv_lqr.py:30-145, bounds inactive) ---------------------- */

/* Backward Riccati pass of the QP solve_tvlqr poses:
 *   min sum_t (x_t-xd_t)'Q(x_t-xd_t) + alpha_R u_t'R u_t + (x_T-xd_T)'Qd(x_T-xd_T)
 *   s.t. x_{t+1} = A_t x_t + B_t u_t + c_t
 * alpha_R = 0.5 reproduces Drake's AddQuadraticCost (tv_lqr.py:110).
 * Any n <= 32, m <= 16.  K (T,m,n), k (T,m) DEV f64 out: u_t = K_t x_t + k_t.
 * info (1) DEV int32: 0 ok, t+1 = Hessian not positive definite at step t -- the FIRST such step of the sweep, which
 * runs from T-1 down (rule V1 above) -- or T+1: every pivot was fine but a stored gain is not finite (rule V2: a NaN or
 * Inf in ct or xd_trj never meets a pivot).                                                                         */
int irs_tvlqr_riccati(int n, int m, int T, const double *At, const double *Bt,
                      const double *ct, const double *Q, const double *Qd,
                      const double *R, double alpha_R, const double *xd_trj,
                      double *K, double *k, int *info, void *stream);

/* solve_tvlqr's return value (x*, u*): the policy rolled out on the LINEAR model
 * from x0.  x_star (T+1,n), u_star (T,m) DEV f64 out.                            */
int irs_tvlqr_linear_rollout(int n, int m, int T, const double *At, const double *Bt,
                             const double *ct, const double *K, const double *k,
                             const double *x0, double *x_star, double *u_star,
                             void *stream);

/* The forward loop of IrsLqr.local_descent (irs_lqr/irs_lqr.py:169-184): u_t =
 * K_t x_t + k_t (== the re-solved QP's first control), x_{t+1} = f(x_t,u_t) on the
 * TRUE dynamics, plus evaluate_cost of the result.                                */
int irs_closed_loop_rollout(int model, const double *params, int n_params, int T,
                            const double *K, const double *k, const double *x0,
                            const double *Q, const double *R, const double *xd_trj,
                            double *x_new, double *u_new, double *cost, void *stream);

/* irs_tvlqr_riccati + irs_closed_loop_rollout in ONE launch: everything
 * IrsLqr.local_descent does after get_TV_matrices (irs_lqr/irs_lqr.py:169-184) plus
 * evaluate_cost (:121-137) of the new trajectory.  x0 (n) DEV.
 * info (1): as irs_tvlqr_riccati (V1: t+1 of the first Hessian that is not positive definite); T+1 also when the
 * pivots and gains were fine but the realised cost is not finite (V2: x0, a rollout that left the range of f64).  */
int irs_tvlqr_descent(int model, const double *params, int n_params, int T,
                      const double *At, const double *Bt, const double *ct,
                      const double *Q, const double *Qd, const double *R, double alpha_R,
                      const double *xd_trj, const double *x0, double *K, double *k,
                      double *x_new, double *u_new, double *cost, int *info, void *stream);

/* B descents of the analytic models in ONE launch: irs_tvlqr_descent with a problem index, grid B, one 64-lane
 * workgroup per problem.  Problem b's outputs are, bit for bit, those of irs_tvlqr_descent on problem b's inputs, on
 * every Riccati path (the model and T choose it as in the single call).
 * In (DEV f64, B contiguous blocks): At (B,T,n,n), Bt (B,T,n,m), ct (B,T,n), xd_trj (B,T+1,n), x0 (B,n); shared by
 *      the problems: the model and its params, T, Q, Qd, R, alpha_R.
 * Out: K (B,T,m,n), k (B,T,m), x_new (B,T+1,n), u_new (B,T,m), cost (B) DEV f64, info (B) DEV int: problem b's
 *      verdict, by the rules V1 and V2 of the single entry; a failing or poisoned problem changes no bit of another's.
 * Every argument error is decided before the first HIP call:
 *   IRS_ERR_INVALID_ARG  B <= 0, T <= 0, a null pointer, wrong n_params
 *   IRS_ERR_UNSUPPORTED  an unknown model; a contact model (irs_quasistatic_box_descent_batch is its batched descent) */
int irs_tvlqr_descent_batch(int model, const double *params, int n_params, int T, int B,
                            const double *At, const double *Bt, const double *ct,
                            const double *Q, const double *Qd, const double *R, double alpha_R,
                            const double *xd_trj, const double *x0, double *K, double *k,
                            double *x_new, double *u_new, double *cost, int *info, void *stream);

/* IrsLqr.local_descent (irs_lqr/irs_lqr.py:148-186) with ACTIVE absolute box bounds
 * (solve_tvlqr's x_bound_abs / u_bound_abs, irs_lqr/tv_lqr.py:112-123): T tail QPs, each
 * re-solved from the realised state, first control applied to the true dynamics.  The QPs
 * (OSQP in the reference) are solved by ADMM on the box around one shared Riccati
 * factorisation, warm started from tail to tail.  xlo,xhi (n), ulo,uhi (m) DEV f64, +-inf =
 * unbounded, applied to x_1..x_T and u_0..u_{T-1}.  rho > 0 ADMM penalty, 0 < relax < 2
 * over-relaxation, stop at max(primal, dual residual) < eps or max_iter.
 * info (3) DEV int32: [0] t+1 of a non-PD Hessian (0 ok; V1: the first one of the sweep, the Hessians carrying the
 * rho/2 of the bounded components; T+1: the realised cost is not finite), [1] most ADMM iterations any tail
 * needed, [2] number of tails that stopped at max_iter or whose first control is not finite (V2: the residuals are
 * maxima, which drop a NaN -- a poisoned tail is never "converged").  The lazy, adaptive, workspace and batch entries
 * and irs_tvlqr_box_solve report by the same rules.  One launch; the factorisation lives
 * in LDS, so T is limited (irs_tvlqr_box_lds_bytes(model,T) <= ~160 KB); irs_tvlqr_box_descent_wsx
 * runs longer horizons with the factor records in a workspace in HBM.                      */
int irs_tvlqr_box_descent(int model, const double *params, int n_params, int T,
                          const double *At, const double *Bt, const double *ct,
                          const double *Q, const double *Qd, const double *R, double alpha_R,
                          const double *xd_trj, const double *x0,
                          const double *xlo, const double *xhi, const double *ulo, const double *uhi,
                          double rho, double relax, int max_iter, double eps,
                          double *x_new, double *u_new, int *info, void *stream);
size_t irs_tvlqr_box_lds_bytes(int model, int T);

/* The bounded TV-LQR beyond the LDS horizon.  The kernel keeps one factor record per time step (the Riccati
 * factorisation every ADMM iteration sweeps) and the ADMM vectors.  With the records in a caller workspace in HBM
 * only the vectors stay in LDS: the horizon is limited by irs_tvlqr_box_hbm_lds_bytes(model, T, du) <= ~160 KB
 * instead (irs_box_horizon_limit: quadrotor T <= 357, bicycle T <= 867; position-controlled form, du = 1: planar
 * hand T <= 383, box pivoting T <= 679).  The sweeps stage the records back through LDS two steps ahead of use; the results are
 * bit-identical to the on-chip path.
 * irs_tvlqr_box_workspace_bytes: the record bytes when the records do not fit LDS, 0 when they do (or when the
 * model has no such form).  du = 0: the plain form of irs_tvlqr_box_descent; du = 1: the position-controlled
 * form (irs_quasistatic_box_descent solver 1, irs_tvlqr_box_solve with position_controlled = 1).  Neither query
 * touches the GPU.                                                                                             */
size_t irs_tvlqr_box_workspace_bytes(int model, int T, int du);
size_t irs_tvlqr_box_hbm_lds_bytes(int model, int T, int du);
/* The longest horizon a bounded-descent kind runs on `model`, with a workspace where the kind takes one; 0 when the
 * model has no such form, INT_MAX for the matrix-core tiles (no cap).  One planner in csrc/boxqp.hip decides every
 * placement, LDS size and cap of the bounded descents; this and the size queries above read it.  No GPU.
 *   IRS_BOX_ADMM             irs_tvlqr_box_descent / _solve, plain form (records in HBM)
 *   IRS_BOX_ADMM_DU          the position-controlled form: irs_quasistatic_box_descent solver 1 (records in HBM)
 *   IRS_BOX_ACTIVE_SET       irs_quasistatic_box_descent solver 2 (on chip only)
 *   IRS_BOX_ACTIVE_SET_MFMA  irs_quasistatic_box_descent solver 3                                               */
typedef enum irs_box_kind {
    IRS_BOX_ADMM = 0,
    IRS_BOX_ADMM_DU = 1,
    IRS_BOX_ACTIVE_SET = 2,
    IRS_BOX_ACTIVE_SET_MFMA = 3
} irs_box_kind;
int irs_box_horizon_limit(int model, int kind);
/* The bytes of per-step records the kernel of `kind` keeps for horizon T when they are placed in a workspace: what
 * the planner sizes the workspace entries by, at ANY horizon (the *_workspace_bytes queries answer 0 while the records
 * fit on chip).  0 for T <= 0, an unknown model or kind, a model without that form, and IRS_BOX_ACTIVE_SET (on chip
 * only: nothing to place).  No GPU.                                                                             */
size_t irs_box_records_bytes(int model, int T, int kind);
/* irs_tvlqr_box_descent / irs_tvlqr_box_solve with a workspace: DEV, 256-byte aligned, >= the record bytes of
 * this horizon (irs_box_records_bytes: BoxLayout stride x T, rounded up to 256; irs_tvlqr_box_workspace_bytes where
 * the records do not fit LDS).  A workspace that is given is used, even where the records would fit on chip; NULL =
 * the entry without it.  IRS_ERR_WORKSPACE if it is too small.                                                 */
int irs_tvlqr_box_descent_wsx(int model, const double *params, int n_params, int T,
                              const double *At, const double *Bt, const double *ct,
                              const double *Q, const double *Qd, const double *R, double alpha_R,
                              const double *xd_trj, const double *x0,
                              const double *xlo, const double *xhi, const double *ulo, const double *uhi,
                              double rho, double relax, int max_iter, double eps,
                              double *x_new, double *u_new, int *info, void *workspace, size_t workspace_bytes,
                              void *stream);

/* IrsLqrQuasistatic.local_descent after get_TV_matrices (irs_lqr/irs_lqr_quasistatic.py:286-345)
 * for a position-controlled model (one with indices_u_into_x, e.g. IRS_MODEL_PLANAR_HAND): T tail
 * re-solves of solve_tvlqr(..., indices_u_into_x, x_bound_abs, u_bound_abs, u_bound_rel)
 * (irs_lqr/tv_lqr.py:30-137), first control applied to the true dynamics, plus eval_cost
 * (:153-194) of the new trajectory.  The input cost is du_t'R du_t with du_t = u_t - u_{t-1},
 * du_0 = u_0 - x_0[indices_u_into_x] (tv_lqr.py:98-108); inside each tail re-solve "u_{-1}" is
 * the realised actuated position.  Solved as the box-LQR of the augmented state [x; u_prev] with
 * the ADMM of irs_tvlqr_box_descent.
 * Bounds, all DEV f64, NULL = absent, +-inf entries allowed:
 *   x_lo,x_hi (T+1,n): ABSOLUTE bounds on x_t   (the caller adds the nominal trajectory to the
 *   u_lo,u_hi (T,m)  : ABSOLUTE bounds on u_t    reference's trust-region offsets, :303-314)
 *   du_lo,du_hi (T,m): bounds on u_t - u_{t-1}  (u_bounds_rel, :321-325)
 * x_bound_rel is not supported ("should be rarely used", :315-319).
 * solver: 1 = the ADMM of irs_tvlqr_box_descent on the augmented problem (any combination of
 *   bounds; rho, relax, max_iter, eps as there);
 *   2 = exact active-set method (primal-dual active set with a primal active-set safeguard) on the
 *   control-box form of the QP: needs x_lo == NULL and at most ONE of the u / du pairs (every
 *   example of the reference); the active set and the backward sweep are carried from tail to
 *   tail; eps = tolerance on bounds and multipliers, max_iter = cap on safeguard iterations per
 *   tail, rho/relax unused; one wave, every quantity of all T steps in LDS (planar hand: T <= 52);
 *   3 = the same method with every step riding in one 16 x 16 matrix-core tile of homogeneous
 *   coordinates (csrc/ctrlbox_mfma.hip; models with n + 2 m + 1 <= 16 after padding: all contact
 *   models here): ~5x faster, and no horizon limit -- per-step records stay in LDS when they fit (planar
 *   hand T <= 53, box pivoting T <= 123) and
 *   otherwise live in the workspace of irs_quasistatic_box_descent_wsx;
 *   0 = 3 where it applies (on chip, or a workspace was given), else 2 where it fits LDS, else 1.
 * cost (1) DEV (may be NULL); info (3): [0] t+1 of a non-PD Hessian (V1: the first one of the first backward sweep,
 * which starts from the empty active set and factors the full Hessian of every step; T+1: the realised cost is not
 * finite), [1] most iterations any tail needed, [2] number of tails that did not converge -- a tail whose first
 * control is not finite has not (V2), whichever solver ran.  The verdict of solver 3, whose translation unit is
 * compiled with -fno-honor-nans, is decided on bit patterns like every other.  _ws, _wsx, _set, _lazy, _batch: the same.  */
int irs_quasistatic_box_descent(int model, const double *params, int n_params, int T,
                                const double *At, const double *Bt, const double *ct,
                                const double *Q, const double *Qd, const double *R,
                                const double *xd_trj, const double *x0,
                                const double *x_lo, const double *x_hi,
                                const double *u_lo, const double *u_hi,
                                const double *du_lo, const double *du_hi,
                                int solver, double rho, double relax, int max_iter, double eps,
                                double *x_new, double *u_new, double *cost, int *info, void *stream);
/* The same with the active set of the FIRST tail handed from one iLQR iteration to the next.
 * act_io (T,m) DEV f64 in {-1: at the lower bound, 0: free, +1: at the upper bound}, may be NULL
 * (= irs_quasistatic_box_descent).  In: the set the first tail's solve starts from (all zeros = cold
 * start; any content is valid, the QP's solution does not depend on it); out: the set that tail
 * converged to.  Consecutive iterations of IrsLqrQuasistatic.iterate (irs_lqr_quasistatic.py:349-385)
 * bind nearly the same bounds, so the cold start of tail 0 -- up to 40 % of a descent -- shrinks to a
 * few sweeps.  Used by the active-set solver only (ADMM ignores it).                                  */
int irs_quasistatic_box_descent_ws(int model, const double *params, int n_params, int T,
                                   const double *At, const double *Bt, const double *ct,
                                   const double *Q, const double *Qd, const double *R,
                                   const double *xd_trj, const double *x0,
                                   const double *x_lo, const double *x_hi,
                                   const double *u_lo, const double *u_hi,
                                   const double *du_lo, const double *du_hi,
                                   int solver, double rho, double relax, int max_iter, double eps,
                                   double *x_new, double *u_new, double *cost, int *info,
                                   double *act_io, void *stream);
size_t irs_quasistatic_box_lds_bytes(int model, int T, int solver);
/* solve_tvlqr stand-alone (irs_lqr/tv_lqr.py:30-145): ONE QP, possibly bounded, its plan returned -- what a
 * caller outside the MPC loops gets from the reference function.  `model` only selects the compiled (n, m)
 * (and, position_controlled = 1: indices_u_into_x, tv_lqr.py:96-108, cost on du_t = u_t - u_{t-1} with
 * du_0 = u_0 - x0[idx], full R); its dynamics are not used.  Bounds: per-time rows, DEV f64, NULL = absent,
 * +-inf allowed: x_lo,x_hi (T+1,n) [x_bound_abs, :112-115; row 0 is not enforced: x_0 is data], u_lo,u_hi (T,m)
 * [u_bound_abs, :116-118], du_lo,du_hi (T,m) [u_bound_rel, :122-125; position-controlled form only].
 * x_bound_rel (:119-121) is not supported.  alpha_R: 1/2 for the plain branch (Drake's AddQuadraticCost(R, 0, u),
 * :110), 1 for the position-controlled one (:107).  ADMM around one Riccati factorisation (csrc/boxqp.hip);
 * x_star (T+1,n), u_star (T,m) DEV out; info (3) as for irs_tvlqr_box_descent.                              */
int irs_tvlqr_box_solve(int model, const double *params, int n_params, int T,
                        const double *At, const double *Bt, const double *ct,
                        const double *Q, const double *Qd, const double *R, double alpha_R,
                        const double *xd_trj, const double *x0, int position_controlled,
                        const double *x_lo, const double *x_hi, const double *u_lo, const double *u_hi,
                        const double *du_lo, const double *du_hi,
                        double rho, double relax, int max_iter, double eps,
                        double *x_star, double *u_star, int *info, void *stream);
int irs_tvlqr_box_solve_wsx(int model, const double *params, int n_params, int T,
                            const double *At, const double *Bt, const double *ct,
                            const double *Q, const double *Qd, const double *R, double alpha_R,
                            const double *xd_trj, const double *x0, int position_controlled,
                            const double *x_lo, const double *x_hi, const double *u_lo, const double *u_hi,
                            const double *du_lo, const double *du_hi,
                            double rho, double relax, int max_iter, double eps,
                            double *x_star, double *u_star, int *info, void *workspace, size_t workspace_bytes,
                            void *stream);
/* The ADMM settings of the bounded TV-LQR as one struct, with the adaptive penalty: OSQP, which the reference calls,
 * adapts its rho by itself, and the speed of the ADMM depends strongly on rho relative to the problem's scale.
 * rho, relax, eps, max_iter: as the positional arguments of the entries above (rho: the penalty the launch starts from).
 * adaptive != 0: after every check_every-th iteration of a tail QP that has not converged the residuals are
 * balanced (the quantities are maxima over the tail's bounded components; y: the scaled duals):
 *     ratio = sqrt((rp / pn) / (rd / dn)), clipped to [1e-2, 1e2],   rp = |z - w|, rd = rho |w - w_prev|,
 *                                                                    pn = max(|z|, |w|), dn = rho |y|;
 * when ratio > trigger or ratio < 1 / trigger: rho <- rho ratio, y <- y / ratio (the multipliers rho y stay), and the
 * kernel rebuilds its Riccati factor -- at most max_refactor times per tail.  The new rho stays for the following
 * warm-started tails of the launch.  The stopping test is unchanged: max(rp, rd) < eps with the current rho.
 * adaptive == 0: check_every, trigger and max_refactor are not read, and the launch is that of the positional entry.
 * IRS_ADMM_CHECK_EVERY, _TRIGGER, _MAX_REFACTOR: the constants the Python classes pass.           */
#define IRS_ADMM_CHECK_EVERY 1000
#define IRS_ADMM_TRIGGER 5.0
#define IRS_ADMM_MAX_REFACTOR 4
typedef struct {
    double rho, relax, eps;
    int max_iter;
    int adaptive;
    int check_every;
    double trigger;
    int max_refactor;
} irs_admm_settings;
/* irs_tvlqr_box_descent_wsx, irs_tvlqr_box_solve_wsx and the ADMM form (solver 1; any other solver is refused) of
 * irs_quasistatic_box_descent_wsx with `settings` in place of (rho, relax, max_iter, eps); every other argument as
 * there.  adapt_out (3) DEV f64, may be NULL, written by the adaptive form only: [0] the Riccati factorisations of the
 * launch (1 = rho never moved), [1] the rho it ended with, [2] its ADMM iterations, all tails.  info keeps its meaning.  Records on chip or in the
 * workspace: bit-identical results, as for the fixed penalty.                                                      */
int irs_tvlqr_box_descent_set(int model, const double *params, int n_params, int T,
                              const double *At, const double *Bt, const double *ct,
                              const double *Q, const double *Qd, const double *R, double alpha_R,
                              const double *xd_trj, const double *x0,
                              const double *xlo, const double *xhi, const double *ulo, const double *uhi,
                              const irs_admm_settings *settings,
                              double *x_new, double *u_new, int *info, double *adapt_out,
                              void *workspace, size_t workspace_bytes, void *stream);
int irs_tvlqr_box_solve_set(int model, const double *params, int n_params, int T,
                            const double *At, const double *Bt, const double *ct,
                            const double *Q, const double *Qd, const double *R, double alpha_R,
                            const double *xd_trj, const double *x0, int position_controlled,
                            const double *x_lo, const double *x_hi, const double *u_lo, const double *u_hi,
                            const double *du_lo, const double *du_hi,
                            const irs_admm_settings *settings,
                            double *x_star, double *u_star, int *info, double *adapt_out,
                            void *workspace, size_t workspace_bytes, void *stream);
int irs_quasistatic_box_descent_set(int model, const double *params, int n_params, int T,
                                    const double *At, const double *Bt, const double *ct,
                                    const double *Q, const double *Qd, const double *R,
                                    const double *xd_trj, const double *x0,
                                    const double *x_lo, const double *x_hi,
                                    const double *u_lo, const double *u_hi,
                                    const double *du_lo, const double *du_hi,
                                    int solver, const irs_admm_settings *settings,
                                    double *x_new, double *u_new, double *cost, int *info, double *adapt_out,
                                    void *workspace, size_t workspace_bytes, void *stream);
/* The three entries above with the box bounds enforced lazily (constraint generation inside the kernel).  A component
 * -- of [x (n) | u (m)], or in the position-controlled form of [x (n) | u abs (m) | du (m)] -- carries the ADMM's rho
 * term and is projected only while it is in the enforced set S.  When a tail QP has converged, every component with a
 * finite bound outside S is compared with its bounds on the tail's rows of the plan (plain < / >, no tolerance); those
 * that leave them join S (their w = clip(z), y = 0), the kernel rebuilds its Riccati factor from the tail's first step
 * and the same tail goes on, its iterations running on against max_iter.  Exactness: a converged plan that keeps every
 * dropped bound is feasible for the full QP and optimal for a relaxation of it, hence the full QP's solution, to the
 * ADMM's tolerance.  S only grows (at most one factorisation per component) and stays for the launch's following
 * warm-started tails; a tail that ends at max_iter is not checked and counts in info[2]; the first control of a tail
 * is clipped to all bounds, as ever.  Scripts that write "no bound" as a large finite number keep the rho term off
 * those components this way -- on them it only damps the iteration.  Works with the fixed and the adaptive penalty.
 * enforced_io DEV int, (n + m) or position controlled (n + 2 m), may be NULL.  In: nonzero = in S from the start
 * (ignored where the component has no finite bound; NULL: S starts empty).  Out: 1 where in S when the launch ends,
 * else 0 -- what the next descent over the same bounds should start from.
 * lazy_out (3) DEV f64, may be NULL: [0] activation events (one extra factorisation each), [1] the last tail that
 * activated something, -1 if none, [2] the ADMM iterations of the launch, all tails.
 * adapt_out as above, written with adaptive == 0 too; its [0] counts the lazy factorisations as well.  The two new
 * arguments stand before `stream`, which stays last as in every entry.  Results need not equal the _set entries' bit
 * for bit (the iteration differs); records on chip or in the workspace give identical bits.                          */
int irs_tvlqr_box_descent_lazy(int model, const double *params, int n_params, int T,
                               const double *At, const double *Bt, const double *ct,
                               const double *Q, const double *Qd, const double *R, double alpha_R,
                               const double *xd_trj, const double *x0,
                               const double *xlo, const double *xhi, const double *ulo, const double *uhi,
                               const irs_admm_settings *settings,
                               double *x_new, double *u_new, int *info, double *adapt_out,
                               void *workspace, size_t workspace_bytes,
                               int *enforced_io, double *lazy_out, void *stream);
int irs_tvlqr_box_solve_lazy(int model, const double *params, int n_params, int T,
                             const double *At, const double *Bt, const double *ct,
                             const double *Q, const double *Qd, const double *R, double alpha_R,
                             const double *xd_trj, const double *x0, int position_controlled,
                             const double *x_lo, const double *x_hi, const double *u_lo, const double *u_hi,
                             const double *du_lo, const double *du_hi,
                             const irs_admm_settings *settings,
                             double *x_star, double *u_star, int *info, double *adapt_out,
                             void *workspace, size_t workspace_bytes,
                             int *enforced_io, double *lazy_out, void *stream);
int irs_quasistatic_box_descent_lazy(int model, const double *params, int n_params, int T,
                                     const double *At, const double *Bt, const double *ct,
                                     const double *Q, const double *Qd, const double *R,
                                     const double *xd_trj, const double *x0,
                                     const double *x_lo, const double *x_hi,
                                     const double *u_lo, const double *u_hi,
                                     const double *du_lo, const double *du_hi,
                                     int solver, const irs_admm_settings *settings,
                                     double *x_new, double *u_new, double *cost, int *info, double *adapt_out,
                                     void *workspace, size_t workspace_bytes,
                                     int *enforced_io, double *lazy_out, void *stream);
/* IrsLqrZeroOrder.compute_least_squares (irs_lqr/irs_lqr_zero_order.py:27-36) stand-alone: dxdu (N, n+m),
 * deltaf (N, n) DEV f64 -> A (n,n), B (n,m) with [A | B] = lstsq(dxdu, deltaf)[0]'.  Normal equations in f64,
 * Jacobi-scaled Cholesky (the solve the sample pass ends with).  info (1): 0, the failed pivot (1-based: a
 * rank-deficient design), or n+m+1 for non-finite data.  n <= 32, m <= 16.                                   */
int irs_least_squares(int n, int m, int N, const double *dxdu, const double *deltaf, double *A, double *B,
                      int *info, void *stream);

/* ---- The values pass: the zero-order sample pass of a system WITHOUT a device functor ------------------------
 * The caller evaluated its own dynamics; these entries evaluate no model.  All T timesteps at once:
 *   dx (T,N,n), du (T,N,m), fz (T,N,n) DEV f32, 16-byte aligned: the samples and fz = f(x_t + dx, u_t + du);
 *   f0 (T,n) DEV f32: f(x_t, u_t) from the same code in the same precision (dF = fz - f0 is formed in f32);
 *   fnom (T,n) DEV f64: the nominal step c_t is measured from; x_trj (>= T rows of n), u_trj (T,m) DEV f64.
 * 1 <= n <= 32, 1 <= m <= 16 (the generic Riccati kernel's limits), 1 <= T <= 1024, N >= 1.
 * sums (T,P) DEV f64, P = irs_values_sums_len(n, m) = d(d+1)/2 + d n, d = n + m: the IRS_SMOOTH_ZERO_ORDER_AB
 * layout of irs_sums_len -- upper triangle of Z'Z row-major, then Z'dF (d,n).  Sums of sample shards add
 * (all-reduce them, then finalize with N_total).  The Gram products run on the matrix cores in f32, moved to f64
 * every 1024 samples per wave; every summation order is a function of (T, N) alone, so a call is bit-reproducible.
 * The solve is irs_least_squares' (Jacobi-scaled Cholesky of the normal equations, f64): At (T,n,n), Bt (T,n,m),
 * ct (T,n) = fnom_t - A_t x_t - B_t u_t, info (T): 0, the failed pivot (1-based), or n+m+1 where a statistic of
 * that timestep is not finite; a bad timestep leaves the others alone.  N_total < n+m samples cannot span the
 * design (rank Z'Z <= N_total): pivot N_total + 1 is reported failed whatever rounding left on it.
 * workspace: DEV, 256-byte aligned, >= irs_smooth_values_workspace_bytes(n, m, T, N), uninitialised scratch (the
 * workgroups' partial sums; no counters, nothing to zero).  One call in flight per workspace at a time.  No
 * allocation, no host synchronisation: accumulate and irs_smooth_values enqueue two launches, finalize one.
 * Every argument error is decided before the first HIP call:
 *   IRS_ERR_INVALID_ARG  a size out of range, a null pointer, dx / du / fz not 16-byte aligned
 *   IRS_ERR_WORKSPACE    workspace null, too small or not 256-byte aligned                                      */
int irs_values_sums_len(int n, int m);
/* No GPU is touched; 0 for invalid sizes.  Non-decreasing in n, m, T and N (an upper bound of the partials, not their
 * exact size): a workspace sized for a caller's largest (n, m, T, N) -- the largest shard, say -- serves every
 * smaller call.                                                                                                 */
size_t irs_smooth_values_workspace_bytes(int n, int m, int T, int N);
/* the launch geometry for (T, N) -- it does not depend on (n, m): out = {threads per workgroup, workgroups per
 * timestep (nblk), samples per workgroup (a multiple of 256; the last one of a timestep may be ragged), trips
 * between f64 flushes}                                                                                          */
int irs_smooth_values_geometry(int T, int N, long long out[4]);
/* irs_rng_samples for ANY 1 <= n <= 32, 1 <= m <= 16 (that entry serves the compiled models' sizes): the same
 * Philox stream -- counter (sample_offset + i, t, block, iter), key seed; oracle/irs_oracle.py:device_gaussian_samples --
 * written as dx (T,N,n), du (T,N,m) DEV f32.  std_x (n), std_u (m) HOST.                                        */
int irs_values_rng_samples(int n, int m, int T, int N, const double *std_x, const double *std_u, uint64_t seed,
                           uint32_t iter, uint64_t sample_offset, float *dx, float *du, void *stream);
int irs_smooth_values_accumulate(int n, int m, int T, int N, const float *dx, const float *du, const float *fz,
                                 const float *f0, double *sums, void *workspace, size_t workspace_bytes,
                                 void *stream);
int irs_smooth_values_finalize(int n, int m, int T, long long N_total, const double *x_trj, const double *u_trj,
                               const double *fnom, const double *sums, double *At, double *Bt, double *ct,
                               int *info, void *stream);
int irs_smooth_values(int n, int m, int T, int N, const double *x_trj, const double *u_trj, const float *dx,
                      const float *du, const float *fz, const float *f0, const double *fnom, double *sums,
                      double *At, double *Bt, double *ct, int *info, void *workspace, size_t workspace_bytes,
                      void *stream);

/* ---- Bounded TV-LQR of ANY size, resumable from tail to tail (csrc/boxqp_values.hip) --------------------------
 * irs_tvlqr_box_descent is compiled per model and keeps the plant step inside its launch.  These entries evaluate no
 * model: the same ADMM (one Riccati factorisation, w <- clip(a z + (1-a) w + y), a rho term only on components with
 * a finite bound at any time, stop at max(primal, dual residual) < eps; fixed penalty only) for runtime
 * 1 <= n <= 32, 1 <= m <= 16, split at the plant.  `begin` factorises the whole horizon once per descent; `tail`
 * solves the tail QP t..T from a given state, warm started from the previous tail; the caller's plant runs between
 * the launches on the same stream.  Each entry is ONE launch of one wave; nothing waits on the host.
 *   At (T,n,n), Bt (T,n,m), ct (T,n), Q, Qd (n,n), R (m,m), xd_trj (T+1,n) DEV f64; alpha_R as irs_tvlqr_riccati.
 *   x_lo, x_hi: DEV, x_rows = 1 (one row of n, every step) or T + 1 (row t bounds x_t; row 0 is not enforced: x_t of
 *   a tail is data); u_lo, u_hi: DEV, u_rows = 1 or T.  NULL = absent; +-inf allowed.
 *   workspace: DEV, 256-byte aligned, >= irs_box_values_workspace_bytes(n, m, T).  It holds the state of a descent --
 *   a header, the masks, the T factor records, the warm start (w, y) -- from `begin` to the last `tail`; one descent
 *   at a time per workspace.  It need not be initialised: `begin` writes all of it, the header last.
 *   info (3) DEV: begin writes [t+1 of a non-PD Hessian or 0, 0, 0] -- V1: the first such step of the sweep; V2: T+1
 *   where the pivots were fine but an entry of a factor record is not finite (c_t and xd_t reach the records, never a
 *   pivot); each tail updates [1] = most ADMM iterations of any tail so far, [2] += 1 if it stopped at max_iter or its
 *   first control is not finite (V2: x_t).  A tail whose workspace header does not match (n, m, T, begun) writes
 *   info[0] = -1 and nothing else.
 * Every argument error is decided before the first HIP call:
 *   IRS_ERR_INVALID_ARG  n, m, T or t out of range; a null pointer; x_rows / u_rows not as above; rho <= 0; relax
 *                        outside (0, 2); max_iter <= 0; eps <= 0
 *   IRS_ERR_UNSUPPORTED  T > irs_box_values_horizon_limit(n, m)
 *   IRS_ERR_WORKSPACE    workspace null, too small or not 256-byte aligned                                      */
typedef struct irs_box_values_call {
    int n, m, T;
    const double *At, *Bt, *ct, *Q, *Qd, *R;
    double alpha_R;
    const double *xd_trj;
    const double *x_lo, *x_hi;
    int x_rows;
    const double *u_lo, *u_hi;
    int u_rows;
    double rho, relax;
    void *workspace;
    size_t workspace_bytes;
    int *info;
} irs_box_values_call;
/* No GPU is touched; 0 for invalid sizes.  Non-decreasing in n, m and T: a buffer sized for the largest call serves
 * every smaller one.                                                                                            */
size_t irs_box_values_workspace_bytes(int n, int m, int T);
/* The longest horizon a tail launch serves: its ADMM vectors -- wx, yx, zx (T+1,n), wu, yu, zu, k (T,m) -- stay in
 * LDS beside the 3-slot record ring.  0 for invalid sizes.  Decided by the planner the launch reads.           */
int irs_box_values_horizon_limit(int n, int m);
/* dynamic LDS bytes of a tail launch at horizon T (0 for invalid sizes); <= ~160 KB up to the horizon limit      */
size_t irs_box_values_lds_bytes(int n, int m, int T);
int irs_box_values_begin(const irs_box_values_call *call, void *stream);
/* x_t (n) DEV: the realised state.  u_t (m) DEV: the tail's first control, clipped to its bounds.  x_plan
 * (T+1-t, n), u_plan (T-t, m) DEV or NULL: the tail's plan (the linear-model rollout of the final iterate); with
 * t = 0 that is solve_tvlqr's result.  `call` is checked as in `begin`; the launch reads its bounds, sizes, workspace
 * and info -- the matrices are in the records, and rho and relax are those `begin` wrote to the header.         */
int irs_box_values_tail(const irs_box_values_call *call, int t, const double *x_t, int max_iter, double eps,
                        double *u_t, double *x_plan, double *u_plan, void *stream);
/* The same with a device workspace for horizons whose per-step records do not fit the 160 KB of LDS
 * (solver 3 / 0, and solver 1: the ADMM's factor records, up to irs_tvlqr_box_hbm_lds_bytes(model, T, 1)
 * <= ~160 KB): `workspace` DEV, 256-byte aligned, at least irs_quasistatic_descent_workspace_bytes(model, T,
 * solver) bytes (0 = none needed: pass NULL); uninitialised scratch, no state is kept in it between calls.
 * Where the records fit LDS the workspace is not used.  The reference has no horizon limit
 * (irs_lqr_quasistatic.py:325-345).                                                                    */
int irs_quasistatic_box_descent_wsx(int model, const double *params, int n_params, int T,
                                    const double *At, const double *Bt, const double *ct,
                                    const double *Q, const double *Qd, const double *R,
                                    const double *xd_trj, const double *x0,
                                    const double *x_lo, const double *x_hi,
                                    const double *u_lo, const double *u_hi,
                                    const double *du_lo, const double *du_hi,
                                    int solver, double rho, double relax, int max_iter, double eps,
                                    double *x_new, double *u_new, double *cost, int *info,
                                    double *act_io, void *workspace, size_t workspace_bytes, void *stream);
size_t irs_quasistatic_descent_workspace_bytes(int model, int T, int solver);

/* B independent quasistatic descents in ONE launch: solver 3's method (the active-set solver on matrix-core tiles),
 * one workgroup per problem -- the same program as irs_quasistatic_box_descent_wsx(solver = 3) with a problem index,
 * so problem b's outputs are, bit for bit, those of the single call on problem b's inputs.  What users of a
 * contact-rich optimiser run anyway (several initial guesses, start states or goals) then fills the device's compute
 * units side by side instead of queueing on one.
 * Per problem, B contiguous blocks, all DEV f64: At (B,T,n,n), Bt (B,T,n,m), ct (B,T,n), xd_trj (B,T+1,n), x0 (B,n),
 * the bound rows (B,T,m) -- EXACTLY ONE of the pairs u_lo,u_hi (absolute) / du_lo,du_hi (on u_t - u_{t-1}), the other
 * NULL; +-inf entries allowed -- and the outputs x_new (B,T+1,n), u_new (B,T,m), cost (B) (may be NULL), info (B,3)
 * int, act_io (B,T,m) (may be NULL; in/out as for irs_quasistatic_box_descent_ws).  Shared by all problems: the
 * model and its params, T, Q, Qd, R, the kind of bound, max_iter, eps.  State bounds are not served.
 * Records: in LDS where they fit (irs_quasistatic_descent_batch_workspace_bytes == 0: pass NULL); otherwise in
 * `workspace` (DEV, 256-byte aligned, uninitialised scratch), where problem b owns the bytes from b * round256(
 * irs_quasistatic_descent_workspace_bytes(model, T, 3)).  A non-NULL workspace puts the records there at ANY horizon
 * (as irs_tvlqr_box_descent_wsx does; same results, bit for bit).
 * IRS_ERR_UNSUPPORTED: the model does not fit the tile; IRS_ERR_INVALID_ARG: B <= 0, both bound pairs or neither;
 * IRS_ERR_WORKSPACE: no or too small a workspace.                                                            */
size_t irs_quasistatic_descent_batch_workspace_bytes(int model, int T, int B);   /* no GPU is touched */
int irs_quasistatic_box_descent_batch(int model, const double *params, int n_params, int T, int B,
                                      const double *At, const double *Bt, const double *ct,
                                      const double *Q, const double *Qd, const double *R,
                                      const double *xd_trj, const double *x0,
                                      const double *u_lo, const double *u_hi,
                                      const double *du_lo, const double *du_hi,
                                      int max_iter, double eps,
                                      double *x_new, double *u_new, double *cost, int *info,
                                      double *act_io, void *workspace, size_t workspace_bytes, void *stream);
/* The trust-region rows of B problems in one launch (irs_lqr_quasistatic.py:303-325): lo, hi (B,T,m) DEV f64 out,
 * entry (b,t,j) = x_trj[b,t,indices_u_into_x[j]] + offset (rel = 0: rows for u_lo,u_hi; x_trj (B,T+1,n) DEV f64,
 * indices_u_into_x (m) DEV int32) or the offset alone (rel = 1: rows for du_lo,du_hi; x_trj and the indices are
 * not read).  offsets DEV f64: (B,2,m) -- lower then upper -- or (B,2,T,m) if per_time.  One f64 add per entry.   */
int irs_quasistatic_bound_rows_batch(int n, int m, int T, int B, const double *x_trj, const int *indices_u_into_x,
                                     const double *offsets, int per_time, int rel, double *lo, double *hi,
                                     void *stream);

/* ---- Cross-entropy-method baseline (irs_lqr/cem.py:151-184) -------------------- */

/* Steps 1-2 of CrossEntropyMethod.local_descent (cem.py:163-168): roll out each of the
 * B candidate control sequences u_cand (B,T,m) DEV f64 from x0 on the true dynamics and
 * evaluate its cost (evaluate_cost, cem.py:121-140) -> costs (B) DEV f64.             */
int irs_cem_rollout_costs(int model, const double *params, int n_params, int T, int B,
                          const double *u_cand, const double *x0, const double *Q,
                          const double *R, const double *xd_trj, double *costs, void *stream);

/* Steps 1-2 of CrossEntropyMethodQuasistatic.local_descent (irs_lqr/cem_quasistatic.py:186-200)
 * for a position-controlled model: as irs_cem_rollout_costs, but every candidate is priced with
 * the quasistatic eval_cost (:124-165): state error with Q, TERMINAL Qd, input cost on
 * u_t - u_{t-1} (u_{-1} = x_0[indices_u_into_x]).                                              */
int irs_cem_rollout_costs_quasistatic(int model, const double *params, int n_params, int T, int B,
                                      const double *u_cand, const double *x0, const double *Q,
                                      const double *Qd, const double *R, const double *xd_trj,
                                      double *costs, void *stream);

/* Steps 3-4 (cem.py:173-180): the n_elite cheapest candidates (np.argpartition) ->
 * elite_idx (n_elite) DEV int32 (cheaper-than-threshold candidates in increasing index
 * order, then threshold ties, lowest index first: deterministic), their mean -> u_new (T,m) and
 * population standard deviation -> std_new (T,m), DEV f64.  Any m, T.               */
int irs_cem_refit(int T, int m, int B, int n_elite, const double *u_cand, const double *costs,
                  int *elite_idx, double *u_new, double *std_new, void *stream);

/* ---- Device-resident CEM: the candidates are drawn inside the kernels ------------
 * The draw of cem.py:159-161 / cem_quasistatic.py:170-173 (np.random.normal(u_trj, std_trj, (B,T,m)))
 * replaced by a counter-based stream, so the (B,T,m) tensor is never stored:
 *   u_cand[b,t,j] = fma(std[t,j], (double) z, u_mean[t,j]),
 *   z = component j % 4 of the four normals of Philox counter (sample_offset + b, t, block j / 4, iter), key seed
 * -- the `du` stream of the smoothing generator (irs_rng_samples) with n = 0 and unit std, axes (T,B,m) ->
 * (B,T,m).  It shares that generator's counters on purpose: no caller runs CEM and a smoothing pass with
 * the same (seed, iter).  One refinement: where a Box-Muller pair has u1 within 2^-6 of 1 its radius is
 * formed from 1 - u1, which f32 holds exactly there, so that every candidate agrees with the f64
 * statement of the stream to std (2e-5 |z| + 2e-6); such draws differ from irs_rng_samples' by up to
 * 1e-5, all others are bit-equal.  u_mean, std (T,m) DEV f64.                                          */

/* Debug/verification: writes the candidates u_cand (B,T,m) DEV f64 the calls below draw.               */
int irs_cem_candidates(int T, int m, int B, const double *u_mean, const double *std, uint64_t seed,
                       uint32_t iter, uint64_t sample_offset, double *u_cand, void *stream);

/* irs_cem_rollout_costs (cem.py:163-168) on drawn candidates: ceil(m/4) generator calls per (b,t) in
 * the lane, no per-candidate memory read.                                                              */
int irs_cem_rollout_costs_drawn(int model, const double *params, int n_params, int T, int B,
                                const double *u_mean, const double *std, uint64_t seed, uint32_t iter,
                                uint64_t sample_offset, const double *x0, const double *Q,
                                const double *R, const double *xd_trj, double *costs, void *stream);

/* irs_cem_rollout_costs_quasistatic (cem_quasistatic.py:175-186) on drawn candidates.                  */
int irs_cem_rollout_costs_quasistatic_drawn(int model, const double *params, int n_params, int T, int B,
                                            const double *u_mean, const double *std, uint64_t seed,
                                            uint32_t iter, uint64_t sample_offset, const double *x0,
                                            const double *Q, const double *Qd, const double *R,
                                            const double *xd_trj, double *costs, void *stream);

/* irs_cem_refit (cem.py:173-180, cem_quasistatic.py:188-197) with every elite regenerated from its index
 * instead of loaded: same selection, same summation order.  Reads the OLD u_mean / std while it writes
 * u_new / std_new: IRS_ERR_INVALID_ARG if they alias.                                                  */
int irs_cem_refit_drawn(int T, int m, int B, int n_elite, const double *u_mean, const double *std,
                        uint64_t seed, uint32_t iter, uint64_t sample_offset, const double *costs,
                        int *elite_idx, double *u_new, double *std_new, void *stream);

/* ---- Model-free CEM rollout: one stage per call, the caller steps the plant ----------------------------
 * irs_cem_rollout_costs[_drawn] for a system that has no device functor (a TorchDynamicalSystem): the time
 * loop is the caller's.  For t = 0 .. T the caller makes one call with x (B,n) DEV f64 holding the B states
 * at step t -- x0 in every row at t = 0, afterwards whatever its dynamics returned for (x, u_t) of the call
 * before.  Stage t of candidate b
 *   - adds (x[b] - xd_trj[t])' Q (x[b] - xd_trj[t]) to costs[b]; t = T is the terminal stage and also uses Q
 *     (cem.py:138-139); at t = 0 costs[b] is WRITTEN, so costs (B) DEV f64 needs no clearing;
 *   - for t < T writes the candidate's control of step t -- u_cand[b,t,:] of the supplied (B,T,m) tensor, or
 *     the drawn one (the stream of irs_cem_candidates: same counters, same bits) -- to u_t[b,:] (B,m) DEV f64
 *     out, and adds u' R u.  At t = T u_t is not touched and may be NULL.
 * Q (n,n), R (m,m) dense, xd_trj (T+1,n).  1 <= n <= 32, 1 <= m <= 16.  All arithmetic f64, the terms added in
 * the order irs_cem_rollout_costs adds them; a non-finite state gives a non-finite cost for that candidate
 * only.  After stage T costs holds what irs_cem_rollout_costs returns for the same dynamics; selection and
 * refit are irs_cem_refit / irs_cem_refit_drawn.  One launch on `stream`, no allocation, no host
 * synchronisation.  Decided before any HIP call:
 *   IRS_ERR_INVALID_ARG  n outside 1..32, m outside 1..16; T or B <= 0; t outside 0..T; a null pointer (u_t
 *                        only while t < T)                                                               */
int irs_cem_values_stage(int n, int m, int T, int B, int t, const double *x, const double *u_cand,
                         const double *Q, const double *R, const double *xd_trj,
                         double *u_t, double *costs, void *stream);
int irs_cem_values_stage_drawn(int n, int m, int T, int B, int t, const double *x, const double *u_mean,
                               const double *std, uint64_t seed, uint32_t iter, uint64_t sample_offset,
                               const double *Q, const double *R, const double *xd_trj,
                               double *u_t, double *costs, void *stream);

/* CrossEntropyMethod.iterate (cem.py:186-216) / CrossEntropyMethodQuasistatic.iterate
 * (cem_quasistatic.py:200-258) as ONE call: n_descents x (price B drawn candidates, select, refit, roll
 * out the new mean (cem.py:182) and price it with the cost the candidates got), enqueued back to back on
 * `stream`; the caller reads the histories back once.  Descent i draws around u_hist[i-1] / std_hist[i-1]
 * (descent 0: u_trj0 / std0) with generator iteration iter0 + i and sample_offset 0 -- the chain of the
 * reference's loop, where every descent but the last is adopted and std_trj is always carried.
 * quasistatic 0: the cost of cem.py:124-140 (terminal Q; Qd unused, may be NULL); 1: eval_cost of
 * cem_quasistatic.py:122-160 (terminal Qd, input cost on u_t - u_{t-1}), position-controlled models only
 * (IRS_ERR_UNSUPPORTED otherwise).  scratch: DEV, >= irs_cem_iterate_scratch_bytes(T, m, B, n_elite);
 * IRS_ERR_INVALID_ARG if it is smaller.                                                                 */
typedef struct irs_cem_iterate_call {
    int model, n_params;
    double params[12];
    int T, B, n_elite, n_descents, quasistatic;
    uint64_t seed;
    uint32_t iter0;
    const double *Q, *Qd, *R, *xd_trj, *x0;   /* DEV (n,n), (n,n), (m,m), (T+1,n), (n) */
    const double *u_trj0, *std0;               /* DEV (T,m): mean and std of descent 0 */
    double *u_hist, *std_hist;                 /* DEV out (n_descents, T, m) */
    double *x_hist, *cost_hist;                /* DEV out (n_descents, T+1, n), (n_descents) */
    void *scratch;
    size_t scratch_bytes;
} irs_cem_iterate_call;

size_t irs_cem_iterate_scratch_bytes(int T, int m, int B, int n_elite);
int irs_cem_iterate(const irs_cem_iterate_call *call, void *stream);

/* ---- Pre-marshalled calls ------------------------------------------------------
 * The same operations with their arguments packed in a caller-owned struct, so that a
 * host loop (IrsLqr.iterate, irs_lqr/irs_lqr.py:188-218) pays one pointer-sized FFI
 * call per launch instead of marshalling ~20 scalars.  Fields have the meaning of the
 * like-named parameters above.                                                      */
typedef struct irs_smooth_call {
    int model, n_params;
    double params[12];
    int mode, T, N;
    const double *x_trj, *u_trj;     /* DEV */
    const float *dx, *du;            /* DEV; used when use_rng == 0 */
    int use_rng;                     /* 1: draw on device from std/seed/iter/sample_offset */
    uint32_t iter;
    double std_x[32], std_u[16];
    uint64_t seed, sample_offset;
    double *sums;                    /* DEV (T,P) out */
    double *At, *Bt, *ct;            /* DEV out; all NULL = accumulate only */
    int *info;                       /* DEV (T) out (when At != NULL) */
    long long n_total;               /* samples per timestep over all devices (solve) */
    void *workspace;
    size_t workspace_bytes;
} irs_smooth_call;

/* irs_smooth / irs_smooth_rng / irs_smooth_accumulate[_rng], by struct.           */
int irs_smooth_run(const irs_smooth_call *call, void *stream);

typedef struct irs_descent_call {
    int model, n_params;
    double params[12];
    int T;
    double alpha_R;
    const double *At, *Bt, *ct, *Q, *Qd, *R, *xd_trj, *x0;   /* DEV */
    double *K, *k, *x_new, *u_new, *cost;                     /* DEV out */
    int *info;                                                /* DEV (1) out */
} irs_descent_call;

/* irs_tvlqr_descent, by struct.                                                    */
int irs_descent_run(const irs_descent_call *call, void *stream);

/* ---- IrsLqr.iterate as one call (csrc/iterate.hip) ---------------------------------------------------------
 * irs_lqr/irs_lqr.py:188-218: `n_descents` descents (iterate(k) performs k + 1), each = get_TV_matrices (device-drawn
 * samples: irs_smooth_rng; or IRS_ITERATE_EXACT: irs_exact_linearize) -> irs_tvlqr_descent -> with box bounds:
 * irs_tvlqr_plan_within_bounds and, behind its device-side flag, irs_tvlqr_box_descent_if -- all enqueued back to back
 * on `stream`, no host synchronisation between phases or iterations.  Descent i linearises around the trajectory
 * descent i-1 wrote into x_hist / u_hist (descent 0: x_trj0 / u_trj0); the caller reads the histories back once.
 * std_x (n_descents, n) / std_u (n_descents, m): HOST, the sampling schedule evaluated by the caller (e.g.
 * sigma / iter^p, examples/pendulum/pendulum_zero_order.py:38-43); Philox iteration counter of descent i = iter0 + i.
 * info_hist (n_descents, 8) DEV int32 per descent: [0] Riccati info (t+1 of a non-PD Hessian), [1] number of
 * timesteps whose smoothing solve failed, [2] 1 = some tail's unconstrained plan left the box (the bounded descent
 * ran), [3..5] its info (irs_tvlqr_box_descent), [6] 1 = it was needed but the horizon does not fit its kernel
 * (beyond the LDS horizon its factor records live at the end of the scratch; [6] only past the HBM form's limit).
 * scratch: DEV, >= irs_iterate_scratch_bytes(model, mode, T, N).  timing (optional, HOST out): per-phase device
 * time summed over the descents -- timing mode synchronises after every descent; NULL = fully asynchronous.   */
#define IRS_ITERATE_EXACT 3
typedef struct irs_iterate_call {
    int model, n_params;
    double params[12];
    int mode, T, N, n_descents;
    const double *std_x, *std_u;               /* HOST (n_descents, n) / (n_descents, m); std_x NULL in u-only modes */
    uint64_t seed;
    uint32_t iter0;
    const double *Q, *Qd, *R, *xd_trj;         /* DEV */
    double alpha_R;
    const double *xlo, *xhi, *ulo, *uhi;       /* DEV (n) / (m), all four or none */
    double qp_rho, qp_relax, qp_eps;           /* bounded descent (ADMM); <= 0: defaults 10, 1.6, 1e-8 */
    int qp_max_iter;                           /* <= 0: 5000 */
    const double *x_trj0, *u_trj0;             /* DEV (T+1, n), (T, m): the nominal trajectory of descent 0 */
    double *x_hist, *u_hist, *cost_hist;       /* DEV out (n_descents, T+1, n), (n_descents, T, m), (n_descents) */
    int *info_hist;                            /* DEV out (n_descents, 8) */
    void *scratch;
    size_t scratch_bytes;
} irs_iterate_call;

/* what SURVEY 8(b) calls irs_get_timing: filled by irs_iterate when asked for */
typedef struct irs_timing {
    double linearise_ms, descent_ms, bounds_ms;   /* device time per phase, summed over the descents */
    int descents;
    double sample_steps;                          /* N x T x descents one-step evaluations */
    double sample_bytes;                          /* the f32 perturbations those would stream if supplied */
} irs_timing;

size_t irs_iterate_scratch_bytes(int model, int mode, int T, int N);
int irs_iterate(const irs_iterate_call *call, irs_timing *timing, void *stream);

/* *flag (DEV int32) = 1 iff the unconstrained plan of SOME tail QP (start t, realised state x_new[t], policy K, k rolled
 * out on the linear model) violates the box xlo <= x <= xhi (n), ulo <= u <= uhi (m): only then do the bounded QPs
 * of irs_lqr/tv_lqr.py:112-123 differ from the Riccati descent.  n <= 32, m <= 16.                              */
int irs_tvlqr_plan_within_bounds(int n, int m, int T, const double *At, const double *Bt, const double *ct,
                                 const double *K, const double *k, const double *x_new,
                                 const double *xlo, const double *xhi, const double *ulo, const double *uhi,
                                 int *flag, void *stream);

/* The same test for B problems in one launch (one workgroup per problem): flag (B) DEV int32, flag[b] = the single
 * entry's decision on problem b's blocks of irs_tvlqr_descent_batch -- At (B,T,n,n), Bt (B,T,n,m), ct (B,T,n),
 * K (B,T,m,n), k (B,T,m), x_new (B,T+1,n) -- and ITS box: xlo, xhi (B,n), ulo, uhi (B,m) DEV f64, +-inf allowed.
 * IRS_ERR_INVALID_ARG: sizes out of range, B <= 0, a null pointer.                                              */
int irs_tvlqr_plan_within_bounds_batch(int n, int m, int T, int B, const double *At, const double *Bt, const double *ct,
                                       const double *K, const double *k, const double *x_new,
                                       const double *xlo, const double *xhi, const double *ulo, const double *uhi,
                                       int *flag, void *stream);

/* irs_tvlqr_box_descent that (a) also returns evaluate_cost of its result (cost, may be NULL) and (b) returns at
 * once, writing nothing, when *run_flag (DEV int32, may be NULL = always run) is 0.                            */
int irs_tvlqr_box_descent_if(int model, const double *params, int n_params, int T,
                             const double *At, const double *Bt, const double *ct,
                             const double *Q, const double *Qd, const double *R, double alpha_R,
                             const double *xd_trj, const double *x0,
                             const double *xlo, const double *xhi, const double *ulo, const double *uhi,
                             double rho, double relax, int max_iter, double eps,
                             double *x_new, double *u_new, double *cost, int *info, const int *run_flag,
                             void *stream);

/* B bounded descents of the analytic models (pendulum, quadrotor, bicycle, three cart) in ONE launch: the kernel of
 * irs_tvlqr_box_descent_if with a problem index, grid B, one 64-lane workgroup per problem (fixed penalty, every
 * finite bound enforced).  Problem b's x_new, u_new, cost and info are, bit for bit, those of irs_tvlqr_box_descent_if
 * (records on chip) / irs_tvlqr_box_descent_wsx (records in the workspace) on problem b's inputs.
 * In (DEV f64, B contiguous blocks): At (B,T,n,n), Bt (B,T,n,m), ct (B,T,n), xd_trj (B,T+1,n), x0 (B,n), and each
 *      problem's box xlo, xhi (B,n), ulo, uhi (B,m) (+-inf allowed: the shapes of irs_tvlqr_plan_within_bounds_batch);
 *      shared: the model and its params, T, Q, Qd, R, alpha_R, rho, relax, max_iter, eps.
 * Out: x_new (B,T+1,n), u_new (B,T,m), cost (B, may be NULL) DEV f64, info (B,3) DEV int32.
 * run_flag (B) DEV int32, may be NULL = all run: workgroup b returns at once when run_flag[b] == 0, and nothing of
 *      problem b is read or written.  A problem that fails (info[0] or info[2]) leaves its neighbours' bits alone.
 * workspace: NULL = records on chip (the horizon must fit LDS, as for irs_tvlqr_box_descent); given (DEV, 256-byte
 *      aligned), it is used at any horizon, as irs_tvlqr_box_descent_wsx does: problem b's records at
 *      workspace + b * stride, stride = irs_box_records_bytes(model, T, IRS_BOX_ADMM) rounded up to 256.
 * irs_tvlqr_box_descent_batch_workspace_bytes: B * stride; 0 for B <= 0, T <= 0, a model the batch does not serve,
 *      and a horizon beyond irs_box_horizon_limit(model, IRS_BOX_ADMM).  No GPU.
 * Every argument error is decided before the first HIP call:
 *   IRS_ERR_INVALID_ARG  B <= 0, T <= 0, a null pointer (all but cost, run_flag, workspace), a bad ADMM parameter,
 *                        wrong n_params
 *   IRS_ERR_WORKSPACE    the workspace is smaller than B slices, or not 256-byte aligned
 *   IRS_ERR_UNSUPPORTED  any other model; no workspace at a horizon whose records do not fit LDS; a horizon beyond
 *                        the limit (the single entry's texts)                                                     */
size_t irs_tvlqr_box_descent_batch_workspace_bytes(int model, int T, int B);
int irs_tvlqr_box_descent_batch(int model, const double *params, int n_params, int T, int B,
                                const double *At, const double *Bt, const double *ct,
                                const double *Q, const double *Qd, const double *R, double alpha_R,
                                const double *xd_trj, const double *x0,
                                const double *xlo, const double *xhi, const double *ulo, const double *uhi,
                                double rho, double relax, int max_iter, double eps,
                                double *x_new, double *u_new, double *cost, int *info, const int *run_flag,
                                void *workspace, size_t workspace_bytes, void *stream);

/* ---- the multi-GPU smoothing step inside the library (csrc/collective.hip) ------------------------------
 * One process per GPU; samples sharded over the ranks; per step: sample pass -> ONE all-reduce of the
 * (T,P) f64 statistics (RCCL over xGMI) -> solve (every rank, redundantly).  Replaces the reference's ZeroMQ
 * worker pool (zmq_parallel_cmp/array_io.py:6-26, irs_lqr/irs_lqr_quasistatic.py:245-263).  RCCL is bound at
 * run time (the copy torch.distributed's "nccl" backend loaded, if any).
 *   irs_comm_available   a rank-local, non-collective pre-check a launcher makes before the collective create
 *   irs_comm_unique_id   rank 0 fills 128 bytes (ncclGetUniqueId); the host distributes them to all ranks
 *   irs_comm_create      collective: every rank, with its device current (ncclCommInitRank)
 *   irs_allreduce_sums   in-place f64 SUM all-reduce of `count` doubles on `stream`
 *   irs_smooth_step_collective   the three enqueues (accumulate, all-reduce, solve) on `stream`; `call` must
 *                        carry sums AND At/Bt/ct/info, n_total = samples per timestep over all ranks, and, for
 *                        device-drawn samples, sample_offset = this rank's first global sample; comm may be NULL
 *                        (one rank: no collective)
 *   irs_step_graph_*     the same three enqueues captured ONCE into a HIP graph (on `stream`, which must not be
 *                        the default stream) and replayed with one call per step: the step is ~70-100 us of
 *                        device work in three launches, which a host issuing them one by one cannot keep fed */
int irs_comm_available(void);   /* 1 if RCCL could be bound in this process (no communicator is made), else 0 */
int irs_comm_unique_id(void *id128);
int irs_comm_create(const void *id128, int nranks, int rank, void **comm);
int irs_comm_destroy(void *comm);
int irs_allreduce_sums(void *comm, double *sums, size_t count, void *stream);
int irs_smooth_step_collective(const irs_smooth_call *call, void *comm, void *stream);
int irs_step_graph_create(const irs_smooth_call *call, void *comm, void *stream, void **graph_exec);
int irs_step_graph_launch(void *graph_exec, void *stream);
int irs_step_graph_destroy(void *graph_exec);

/* ---- the same step with the exchange done WITHOUT a collective library (csrc/collective.hip; opt-in) ----------
 * Replaces the same ZeroMQ fan-in as above.  Every rank publishes its (T,P) statistics in an exchange region of
 * its own device memory and reads the other ranks' regions, mapped by IPC handle, directly over xGMI: one small
 * launch between the sample pass and the solve (publish with system-scope stores -> release the step flag -> wait,
 * bounded, for every rank's flag -> sum the blocks in RANK ORDER: the same bits on every rank).  Two alternating
 * slots per region; a peer that does not arrive within IRS_PEER_TIMEOUT_MS (default 2000) poisons the statistics
 * (NaN), which the solve reports through `info` -- the job fails, the GPU does not hang.
 *   irs_peer_alloc       `region` = device memory for `count` doubles per slot (zeroed), `handle64` = its 64-byte
 *                        IPC handle; the host gathers the handles of all ranks (any rendezvous)
 *   irs_peer_create      maps the other ranks' regions; handles = nranks x 64 bytes in rank order (own entry unused)
 *   irs_peer_allreduce_sums   the exchange launch alone: `sums` (count doubles) in place
 *   irs_smooth_step_peer / irs_step_graph_create_peer   as irs_smooth_step_collective / irs_step_graph_create
 *   irs_peer_status      launches and timeouts so far (synchronising read)
 *   irs_peer_destroy     unmaps, frees the counters and, if given, the region (call on every rank after a barrier)
 * Every rank must issue the same sequence of exchange launches.  Not yet run on more than one physical GPU. */
int irs_peer_alloc(size_t count, void **region, void *handle64);
int irs_peer_create(int nranks, int rank, void *region, size_t count, const void *handles, void **peer);
int irs_peer_destroy(void *peer, void *region);
int irs_peer_status(void *peer, unsigned long long *launches, unsigned long long *timeouts);
int irs_peer_allreduce_sums(void *peer, double *sums, size_t count, void *stream);
int irs_smooth_step_peer(const irs_smooth_call *call, void *peer, void *stream);
int irs_step_graph_create_peer(const irs_smooth_call *call, void *peer, void *stream, void **graph_exec);

#ifdef __cplusplus
}
#endif
#endif /* IRS_HIP_H */
