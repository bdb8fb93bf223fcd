// The host side of the sample pass (get_TV_matrices): every extern "C" entry of the smoothing kernels, the planner
// that chooses their launch geometry, and the workspace layout.  No kernel is compiled here: smooth.hip and
// smooth_ug.hip hold them behind the launch interface of smooth_common.hpp.
//
// Every single-problem entry -- by struct (irs_smooth_run) or positional -- states its call as a SmoothEntry and
// goes through smooth_common: the checks in one order, the model constants, the plan (smooth_geometry), the
// workspace carve and SmoothArgs (fill_args), one launch.  The two batched entries state theirs as a SmoothBatchCall and
// go through smooth_batch_common: the checks only B problems have, what tells the two apart as data (SmoothBatchKind),
// fill_args for problem 0, one launch.  The refusal texts carry the names of the entries -- IRS_CHECK_ARG prints
// __func__, the batched path the record's fn: tests/test_smooth_entries_cpu.py pins them, call by call.
#include "smooth_common.hpp"

namespace {

// ---- the workspace: arrival counters, then T rows of f64 nominal steps (n <= 32), then (T, nblk, P4) partial sums ----
constexpr size_t kCounterBytes = 4096;
constexpr int kMaxT = kCounterBytes / sizeof(int);

struct SmoothWorkspace {
    int* counters;
    double* fnom;
    float* partial;
};
constexpr size_t partial_offset(int T) { return kCounterBytes + (size_t)T * 32 * sizeof(double); }
// `rows` rows of partial sums per timestep, P statistics each, padded to 16-byte stores
constexpr size_t partial_bytes(int T, int rows, int P) { return (size_t)T * rows * ((P + 3) / 4 * 4) * sizeof(float); }

SmoothWorkspace smooth_workspace(void* workspace, int T) {
    char* base = static_cast<char*>(workspace);
    return {reinterpret_cast<int*>(base), reinterpret_cast<double*>(base + kCounterBytes),
            reinterpret_cast<float*>(base + partial_offset(T))};
}
// the bytes of a workspace with `rows` partial rows per timestep (rows = 0: what the stand-alone solve reads)
constexpr size_t smooth_workspace_size(int T, int rows, int P) { return partial_offset(T) + partial_bytes(T, rows, P); }

// Planner knobs (environment overrides are for tuning experiments only).
int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    int v = e ? atoi(e) : dflt;
    return v < 1 ? 1 : v;
}
int tune_spt() { static int v = env_int("IRS_SPT", 32); return v; }                 // samples per lane aimed for
int tune_single_max() { static int v = env_int("IRS_SINGLE_MAX", 16384); return v; } // <= : one WG per t
int tune_max_wg() { static int v = env_int("IRS_MAX_WG", 1024); return v; }         // grid cap, light kernels
int tune_max_wg_heavy() { static int v = env_int("IRS_MAX_WG_HEAVY", 256); return v; }  // 1 wave/SIMD kernels
int tune_min_wg() { static int v = env_int("IRS_MIN_WG", 256); return v; }          // fill the CUs

// Chooses the launch geometry for (T, N).  `light` = the kernel's accumulators fit a
// 1024-thread workgroup (SmoothTraits::LIGHT).  Measured on MI355X (profiles/): every extra
// workgroup costs more (its hand-off: write-through stores + ticket) than it gains in
// streaming parallelism once the CUs are covered, so grids stay SMALL:
//  * light, samples supplied, N <= tune_single_max(): ONE 1024-thread workgroup per
//    timestep -- no inter-workgroup hand-off at all;
//  * otherwise 256-thread workgroups, ~tune_spt() samples per lane, at least enough
//    workgroups to cover the CUs (while each lane still has >= 4 samples) and at most
//    ~4 per CU (light kernels) or 1 per CU (kernels that hold 1 wave per SIMD).
void plan_grid(int T, int N, bool light, bool rng, int* chunk, int* nblk, int* block, bool contact = false) {
    if (light && !rng && N <= tune_single_max()) {
        *block = kBigBlock;
        *nblk = 1;
        *chunk = (N + kBigBlock - 1) / kBigBlock * kBigBlock;
        return;
    }
    *block = kBlock;
    if (T < 1) T = 1;
    const int spt = tune_spt();
    int nb = (N + kBlock * spt - 1) / (kBlock * spt);
    int fill = (tune_min_wg() + T - 1) / T;               // blocks per t that cover the CUs
    // ... keeping >= 4 samples per lane -- 1 for a contact kernel, whose sample costs more than a workgroup's
    // hand-off (planar hand N = 1000: one workgroup per time step 51 us, four 2x faster)
    int by4 = contact ? (N + kBlock - 1) / kBlock : (N + kBlock * 4 - 1) / (kBlock * 4);
    if (fill > by4) fill = by4;
    if (nb < fill) nb = fill;
    // heavy kernels: 1 workgroup per CU, 2 once there is enough work to hide the tail.  Contact
    // kernels never: since the active-set polish they need more than 256 registers (VGPRs + AGPRs), one
    // wave per SIMD is all a CU can hold, and a second workgroup per CU would only queue behind the first
    // (before the polish, two per CU won 7 % from N = 1e5 on and lost below that: profiles/).
    const long long two_per_cu = contact ? (1LL << 62) : 2000000;
    const int heavy_cap = tune_max_wg_heavy() * ((long long)N * T >= two_per_cu ? 2 : 1);
    int max_blk = (light ? tune_max_wg() : heavy_cap) / T;
    if (max_blk < 1) max_blk = 1;
    if (nb > max_blk) nb = max_blk;
    if (nb < 1) nb = 1;
    int c = (N + nb - 1) / nb;
    c = (c + kBlock - 1) / kBlock * kBlock;
    *chunk = c;
    *nblk = (N + c - 1) / c;
    if (*nblk < 1) *nblk = 1;
}

// ---- what the kernels of a (model, mode) are compiled to, for runtime ids ---------------------------------------
bool is_light(int model, int mode) {
    bool r = false;
    IRS_DISPATCH_MODEL(model, IRS_DISPATCH_MODE(mode, r = SmoothTraits<Model, MODE>::LIGHT));
    return r;
}

// contact models, in every smoothing mode (nominal_in_wg0<Model, MODE>)
bool has_nominal_in_wg0(int model, int /*mode*/) {
    bool r = false;
    IRS_DISPATCH_MODEL(model, { r = !Model::HAS_JACOBIAN; });
    return r;
}

// smooth_kernel's DEFER path (defer_samples<Model, MODE>)
bool uses_parked_samples(int model, int mode) {
    bool r = false;
    IRS_DISPATCH_MODEL(model, IRS_DISPATCH_MODE(mode, r = defer_samples<Model, MODE>()));
    return r;
}

bool uses_matrix_cores(int model, int mode) {
    bool r = false;
    IRS_DISPATCH_MODEL(model, IRS_DISPATCH_MODE(mode, r = gram_on_matrix_cores<Model, MODE>()));
    return r;
}

// what the f64 nominal step costs the wave of workgroup 0 that evaluates it, in 64-sample trips of the same kernel
// (IRS_NOMINAL_TRIPS overrides for tuning)
int nominal_trips() {
    static int ov = env_int("IRS_NOMINAL_TRIPS", -1);      // (env_int clamps to >= 1: unset, this is 1 -- DESIGN section 7)
    if (ov >= 0) return ov;
    return kNominalTrips;      // measured: 1-3 trips are equal for every contact kernel (planar hand exact / sweeps /
                               // first-order, box pivoting); 4 and more lose a trip
}

// The launch geometry of one sample pass: the ONE statement of which kernel family runs (T, N) and how its samples
// are split over workgroups.  smooth_common launches what this returns; irs_smooth_geometry reports it.
struct SmoothGeometry {
    int family;      // IRS_SMOOTH_FAMILY_*
    int block, nblk; // threads per workgroup, workgroups per timestep
    int chunk0, chunk, wg0_rr;   // SmoothArgs (0, 0, INT_MAX for the uniform-geometry family: it deals 64-sample blocks)
    int branch;      // IRS_SMOOTH_PLAN_*: which contact re-planning set chunk0 / chunk
};

int smooth_geometry(int model, int mode, int T, int N, bool rng, SmoothGeometry* g) {
    IRS_CHECK_ARG(T > 0 && N > 0, "T and N must be positive");
    IRS_CHECK_ARG(mode >= 0 && mode <= 2, "unknown smoothing mode");
    if (irs_sums_len(model, mode) <= 0) return IRS_ERR_UNSUPPORTED;
    g->branch = IRS_SMOOTH_PLAN_NONE;
    g->wg0_rr = 0x7fffffff;
    if (irs_smooth_ug_supported(model, mode)) {
        // exact 8-row contact model, u-only mode: the uniform-geometry pass (smooth_ug.hip)
        g->family = IRS_SMOOTH_FAMILY_UNIFORM_GEOMETRY;
        g->nblk = irs_smooth_ug_nblk(T, N);
        g->block = 512;
        g->chunk = g->chunk0 = 0;
        return IRS_OK;
    }
    const bool contact = has_nominal_in_wg0(model, mode);
    plan_grid(T, N, is_light(model, mode), rng, &g->chunk, &g->nblk, &g->block, contact);
    g->chunk0 = g->chunk;
    g->family = is_light(model, mode) ? IRS_SMOOTH_FAMILY_LANES_LIGHT      // four samples per lane per trip when supplied
                : uses_matrix_cores(model, mode) ? IRS_SMOOTH_FAMILY_GRAM_MATRIX_CORE
                : uses_parked_samples(model, mode) ? IRS_SMOOTH_FAMILY_CONTACT_PARKED
                : contact ? IRS_SMOOTH_FAMILY_CONTACT_WAVE_DEALT : IRS_SMOOTH_FAMILY_LANES_HEAVY;
    bool planned = false;
    if (g->nblk >= 2 && g->block == kBlock && contact) {
        // contact kernels balance by WAVE trips (64 samples): B blocks plus the nominal step's kNominalTrips
        // over 4 nblk waves -> tt trips each; workgroup 0: tt - kNominalTrips rounds over its four waves, then
        // kNominalTrips rounds over three.  (Chunks rounded to whole workgroup trips, as below, left three of the
        // five workgroups of the benchmark's N = 1e4 with 9 trips and one with 5 + the nominal step.)
        const int NW = kBlock / 64, B = (N + 63) / 64, nw = g->nblk * NW;
        const int kNom = nominal_trips();
        const int tt = (B + kNom + nw - 1) / nw, rr = tt - kNom;
        if (rr >= 1) {
            const int c0b = NW * rr + (NW - 1) * kNom;
            const int restb = B > c0b ? (B - c0b + (g->nblk - 1) - 1) / (g->nblk - 1) : 0;
            if (restb <= NW * tt) {
                g->chunk0 = c0b * 64;
                g->chunk = restb > 0 ? restb * 64 : 64;
                g->wg0_rr = rr;
                g->branch = IRS_SMOOTH_PLAN_TRIPS;
                planned = true;
            }
        }
    }
    if (!planned && g->nblk >= 2 && g->block == kBlock && contact) {
        // workgroup 0 gives up kNominalCost samples per lane and evaluates the f64 nominal step
        int c0 = g->chunk - kNominalCost * kBlock;
        if (c0 < kBlock) c0 = kBlock;
        int rest = (N - c0 + (g->nblk - 1) - 1) / (g->nblk - 1);
        rest = (rest + kBlock - 1) / kBlock * kBlock;
        if (c0 < g->chunk && c0 + (long long)(g->nblk - 1) * rest >= N && rest <= g->chunk + kBlock) {
            g->chunk0 = c0;
            g->chunk = rest;
            g->branch = IRS_SMOOTH_PLAN_COST;
        }
    }
    return IRS_OK;
}

// modes that perturb u only never read dx / std_x
bool u_noise_only(int model, int mode) {
    if (mode == IRS_SMOOTH_ZERO_ORDER_B) return true;
    bool contact = false;
    IRS_DISPATCH_MODEL(model, { contact = !Model::HAS_JACOBIAN; });
    return contact && mode == IRS_SMOOTH_FIRST_ORDER;
}

int fill_rng(int model, int mode, const double* std_x, const double* std_u, uint64_t seed, uint32_t iter,
             uint64_t sample_offset, SmoothArgs& a) {
    IRS_CHECK_ARG(std_u != nullptr, "std_u is null");
    IRS_CHECK_ARG(std_x != nullptr || u_noise_only(model, mode), "std_x is null");
    int n, m, np;
    int rc = irs_model_info(model, &n, &m, &np);
    if (rc != IRS_OK) return rc;
    for (int i = 0; i < n; ++i) a.std[i] = std_x ? (float)std_x[i] : 0.f;
    for (int j = 0; j < m; ++j) a.std[n + j] = (float)std_u[j];
    a.seed = seed; a.iter = iter; a.sample_offset = sample_offset;
    return IRS_OK;
}

int check_samples(const float* dx, const float* du, int model, int mode) {
    IRS_CHECK_ARG(du != nullptr, "du is null");
    IRS_CHECK_ARG(dx != nullptr || u_noise_only(model, mode), "dx is null");
    IRS_CHECK_ARG((reinterpret_cast<uintptr_t>(dx) & 15) == 0 && (reinterpret_cast<uintptr_t>(du) & 15) == 0,
                  "dx/du must be 16-byte aligned");
    return IRS_OK;
}

// One single-problem sample pass as an entry states it: the public record, and what the positional entries pass
// differently from it -- arrays of the caller's (std_x may then be null in a u-only mode), and the fused form whatever
// the output pointers are (by struct, a null At asks for the sums alone).
struct SmoothEntry {
    const irs_smooth_call& c;
    const double* params;
    const double* std_x;
    const double* std_u;
    bool fuse;
};

// What an accepted call puts into SmoothArgs, single or batched (then: problem 0's): the trajectories, the plan, the
// workspace carve, the outputs.  IRS_DIAG (timing experiments only) is read here, per call.
void fill_args(SmoothArgs& a, const irs_smooth_call& c, const SmoothGeometry& g, bool fuse) {
    a.x_trj = c.x_trj; a.u_trj = c.u_trj;
    a.T = c.T; a.N = c.N;
    a.block = g.block; a.nblk = g.nblk; a.chunk0 = g.chunk0; a.chunk = g.chunk; a.wg0_rr = g.wg0_rr;
    const char* diag = getenv("IRS_DIAG");
    a.diag = diag ? atoi(diag) : 0;
    const SmoothWorkspace w = smooth_workspace(c.workspace, c.T);
    a.counters = w.counters; a.fnom = w.fnom; a.partial = w.partial;
    a.sums = c.sums;
    if (fuse) {
        a.At = c.At; a.Bt = c.Bt; a.ct = c.ct; a.info = c.info;
        a.n_total = (double)c.n_total;
    }
}

int smooth_common(const SmoothEntry& e, void* stream) {
    const irs_smooth_call& c = e.c;
    SmoothArgs a;
    memset(&a, 0, sizeof(a));
    int rc;
    if (c.use_rng) {
        rc = fill_rng(c.model, c.mode, e.std_x, e.std_u, c.seed, c.iter, c.sample_offset, a);
    } else {
        rc = check_samples(c.dx, c.du, c.model, c.mode);
        a.dx = c.dx; a.du = c.du;
    }
    if (rc != IRS_OK) return rc;
    IRS_CHECK_ARG(c.T > 0 && c.N > 0, "T and N must be positive");
    IRS_CHECK_ARG(c.x_trj && c.u_trj && c.sums && c.workspace, "null pointer");
    IRS_CHECK_ARG(c.mode >= 0 && c.mode <= 2, "unknown smoothing mode");
    IRS_CHECK_ARG(c.T <= kMaxT, "T too large for the arrival counters (max 1024)");
    rc = irs_load_params(c.model, e.params, c.n_params, &a.p);
    if (rc != IRS_OK) return rc;
    const size_t need = irs_smooth_workspace_bytes(c.model, c.mode, c.T, c.N);
    if (c.workspace_bytes < need) {
        irs_set_error("irs_smooth: workspace %zu < %zu bytes", c.workspace_bytes, need);
        return IRS_ERR_WORKSPACE;
    }
    SmoothGeometry g;
    rc = smooth_geometry(c.model, c.mode, c.T, c.N, c.use_rng != 0, &g);
    if (rc != IRS_OK) return rc;
    if (e.fuse) IRS_CHECK_ARG(c.At && c.Bt && c.ct && c.info && c.n_total > 0, "null output pointer");
    fill_args(a, c, g, e.fuse);
    hipStream_t st = static_cast<hipStream_t>(stream);
    rc = g.family == IRS_SMOOTH_FAMILY_UNIFORM_GEOMETRY ? irs_smooth_ug_launch(c.model, c.mode, a, c.use_rng != 0, e.fuse, st)
                                                        : irs_smooth_launch(c.model, c.mode, a, c.use_rng != 0, e.fuse, st);
    if (rc != IRS_OK) return rc;
    IRS_CHECK_LAUNCH();
    return IRS_OK;
}

// the fields every positional single-problem entry passes (the arrays of the record stay empty: SmoothEntry points at
// the caller's)
irs_smooth_call positional_call(int model, int n_params, int mode, int T, int N, const double* x_trj, const double* u_trj,
                                double* sums, void* workspace, size_t workspace_bytes) {
    irs_smooth_call c{};
    c.model = model; c.n_params = n_params; c.mode = mode; c.T = T; c.N = N;
    c.x_trj = x_trj; c.u_trj = u_trj; c.sums = sums;
    c.n_total = N;
    c.workspace = workspace; c.workspace_bytes = workspace_bytes;
    return c;
}

// ---- B problems per launch --------------------------------------------------------------------------------
size_t round256(size_t bytes) { return (bytes + 255) / 256 * 256; }

// what the general kernel's batched form serves of a registered model: the analytic ones (those with a Jacobian) in
// the modes that perturb x and u
bool smooth_general_batch_serves(int model, int mode) {
    return !has_nominal_in_wg0(model, mode) && (mode == IRS_SMOOTH_ZERO_ORDER_AB || mode == IRS_SMOOTH_FIRST_ORDER);
}

// What tells the two batched passes apart, as data: the rest of smooth_batch_common is the same for both.
struct SmoothBatchKind {
    bool (*serves_model)(int model, int mode);       // of a registered model (the uniform-geometry one reads IRS_UG per call)
    const char* serves;              // the refusal of a (model, mode) that is not served, after "<fn>: model %d, mode %d: "
    bool takes_std_x;                // std_x is an argument, and a null one is refused (else: the entry has none)
    bool uniform_geometry_only;      // the planned family must be IRS_SMOOTH_FAMILY_UNIFORM_GEOMETRY, refused by number
    int (*launch)(int model, int mode, const SmoothArgs& a, const SmoothBatch& bat, int B, hipStream_t st);
    const char* launch_refusal;      // what a launcher's refusal is reworded to (fn, model, mode); null: its own text stands
};

const SmoothBatchKind kUniformGeometryBatch{
    irs_smooth_ug_supported,
    "the batched sample pass serves the uniform-geometry kernel (IRS_MODEL_PLANAR_HAND_EXACT in IRS_SMOOTH_ZERO_ORDER_B and "
    "IRS_SMOOTH_FIRST_ORDER, IRS_UG not 0)",
    false, true, irs_smooth_ug_launch_batch, nullptr};
const SmoothBatchKind kGeneralBatch{
    smooth_general_batch_serves,
    "the general batched sample pass serves the analytic models (pendulum, quadrotor, bicycle, three cart) in "
    "IRS_SMOOTH_ZERO_ORDER_AB and IRS_SMOOTH_FIRST_ORDER",
    true, false, irs_smooth_launch_batch, "%s: no batched kernel for model %d, mode %d"};

// One batched sample pass as its entry states it: the kind, and the entry's arguments in the order it takes them.
struct SmoothBatchCall {
    const char* fn;                  // the name the checks word their errors with
    const SmoothBatchKind& kind;
    int model; const double* params; int n_params, mode, T, N, B;
    const double* x_trj; long long x_stride; const double* u_trj; long long u_stride;
    const double* std_x;             // DEV (B, n); null for the uniform-geometry form
    const double* std_u; const uint64_t* seed; uint32_t iter;      // DEV (B, m), DEV (B)
    double *sums, *At, *Bt, *ct; int* info;
    void* workspace; size_t workspace_bytes;
};

// whether the kind serves (model, mode), and then the model's sizes
int smooth_batch_supported(const SmoothBatchKind& k, int model, int mode, int* n, int* m, int* np) {
    const int rc = irs_model_info(model, n, m, np);
    if (rc != IRS_OK) return rc;
    return k.serves_model(model, mode) ? IRS_OK : IRS_ERR_UNSUPPORTED;
}

// B slices of the single-problem workspace, 256-byte aligned; 0 where the kind does not serve (model, mode)
size_t smooth_batch_workspace_size(const SmoothBatchKind& k, int model, int mode, int T, int N, int B) {
    int n, m, np;
    if (B <= 0 || smooth_batch_supported(k, model, mode, &n, &m, &np) != IRS_OK) return 0;
    return (size_t)B * round256(irs_smooth_workspace_bytes(model, mode, T, N));
}

// zeroes a batch workspace: every slice's arrival counters, once per allocation
int smooth_batch_workspace_init(const char* fn, void* workspace, size_t workspace_bytes, void* stream) {
    if (workspace == nullptr || workspace_bytes == 0) { irs_set_error("%s: no workspace", fn); return IRS_ERR_INVALID_ARG; }
    hipError_t e = hipMemsetAsync(workspace, 0, workspace_bytes, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) { irs_set_error("%s: %s", fn, hipGetErrorString(e)); return IRS_ERR_HIP; }
    return IRS_OK;
}

// The one path of both batched entries: the checks in one order, worded with the entry's name, then SmoothArgs for
// problem 0 (fill_args), the strides and per-problem arrays (SmoothBatch), one launch.
int smooth_batch_common(const SmoothBatchCall& c, void* stream) {
    const SmoothBatchKind& k = c.kind;
    const auto refuse = [&c](const char* msg) { irs_set_error("%s: %s", c.fn, msg); return IRS_ERR_INVALID_ARG; };
    // every argument error is decided before the first HIP call
    if (!(c.B > 0 && c.T > 0 && c.N > 0)) return refuse("B, T and N must be positive");
    if (c.T > kMaxT) return refuse("T too large for the arrival counters (max 1024)");
    if ((long long)c.B * c.T > 65535) return refuse("B * T beyond the grid's 65535 rows");
    if (!(c.x_trj && c.u_trj && (c.std_x || !k.takes_std_x) && c.std_u && c.seed && c.sums && c.At && c.Bt && c.ct &&
          c.info))
        return refuse("null pointer");
    if (c.mode < 0 || c.mode > 2) return refuse("unknown smoothing mode");
    int n = 0, m = 0, np = 0;
    int rc = smooth_batch_supported(k, c.model, c.mode, &n, &m, &np);
    if (rc != IRS_OK) {
        irs_set_error("%s: model %d, mode %d: %s", c.fn, c.model, c.mode, k.serves);
        return IRS_ERR_UNSUPPORTED;
    }
    if (c.params == nullptr || c.n_params != np) {
        irs_set_error("%s: model %d expects %d params, got %d", c.fn, c.model, np, c.n_params);
        return IRS_ERR_INVALID_ARG;
    }
    if (c.x_stride < (long long)c.T * n || c.u_stride < (long long)c.T * m)
        return refuse("x_stride / u_stride shorter than a problem's T rows");
    SmoothArgs a;
    memset(&a, 0, sizeof(a));
    rc = irs_load_params(c.model, c.params, c.n_params, &a.p);
    if (rc != IRS_OK) return rc;
    SmoothGeometry g;
    rc = smooth_geometry(c.model, c.mode, c.T, c.N, true, &g);
    if (rc != IRS_OK) return rc;
    if (partial_bytes(c.T, g.nblk, irs_sums_len(c.model, c.mode)) > 0xffffffffull)
        return refuse("a problem's partial sums exceed the hand-off's 32-bit buffer size");
    if (k.uniform_geometry_only && g.family != IRS_SMOOTH_FAMILY_UNIFORM_GEOMETRY) {
        irs_set_error("%s: no batched kernel for the planned kernel family %d", c.fn, g.family);
        return IRS_ERR_UNSUPPORTED;
    }
    const size_t stride = round256(irs_smooth_workspace_bytes(c.model, c.mode, c.T, c.N)), need = (size_t)c.B * stride;
    if (c.workspace == nullptr || c.workspace_bytes < need) {
        irs_set_error("%s: workspace %zu < %zu bytes (%d slices of %zu)", c.fn, c.workspace_bytes, need, c.B, stride);
        return IRS_ERR_WORKSPACE;
    }
    if ((reinterpret_cast<uintptr_t>(c.workspace) & 255) != 0) {
        irs_set_error("%s: the workspace must be 256-byte aligned", c.fn);
        return IRS_ERR_WORKSPACE;
    }
    // problem 0's call; the kernel's entry moves its arguments to the row's problem (SmoothRow)
    irs_smooth_call p0 = positional_call(c.model, c.n_params, c.mode, c.T, c.N, c.x_trj, c.u_trj, c.sums, c.workspace,
                                         c.workspace_bytes);
    p0.At = c.At; p0.Bt = c.Bt; p0.ct = c.ct; p0.info = c.info;
    fill_args(a, p0, g, true);
    a.iter = c.iter;
    const SmoothBatch bat{c.x_stride, c.u_stride, (long long)stride, reinterpret_cast<const unsigned long long*>(c.seed),
                          c.std_u, c.std_x};
    rc = k.launch(c.model, c.mode, a, bat, c.B, static_cast<hipStream_t>(stream));
    if (rc != IRS_OK) {
        if (k.launch_refusal) irs_set_error(k.launch_refusal, c.fn, c.model, c.mode);
        return rc;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { irs_set_error("%s: HIP error %s", c.fn, hipGetErrorString(e)); return IRS_ERR_HIP; }
    return IRS_OK;
}

}  // namespace

extern "C" {

size_t irs_smooth_batch_workspace_bytes(int model, int mode, int T, int N, int B) {
    return smooth_batch_workspace_size(kUniformGeometryBatch, model, mode, T, N, B);
}

size_t irs_smooth_general_batch_workspace_bytes(int model, int mode, int T, int N, int B) {
    return smooth_batch_workspace_size(kGeneralBatch, model, mode, T, N, B);
}

int irs_smooth_batch_workspace_init(void* workspace, size_t workspace_bytes, void* stream) {
    return smooth_batch_workspace_init(__func__, workspace, workspace_bytes, stream);
}

int irs_smooth_general_batch_workspace_init(void* workspace, size_t workspace_bytes, void* stream) {
    return smooth_batch_workspace_init(__func__, workspace, workspace_bytes, stream);
}

int irs_smooth_rng_batch(int model, const double* params, int n_params, int mode, int T, int N, int B,
                         const double* x_trj, long long x_stride, const double* u_trj, long long u_stride,
                         const double* std_u, const uint64_t* seed, uint32_t iter,
                         double* sums, double* At, double* Bt, double* ct, int* info,
                         void* workspace, size_t workspace_bytes, void* stream) {
    return smooth_batch_common({__func__, kUniformGeometryBatch, model, params, n_params, mode, T, N, B, x_trj, x_stride,
                                u_trj, u_stride, nullptr, std_u, seed, iter, sums, At, Bt, ct, info, workspace,
                                workspace_bytes}, stream);
}

int irs_smooth_rng_general_batch(int model, const double* params, int n_params, int mode, int T, int N, int B,
                                 const double* x_trj, long long x_stride, const double* u_trj, long long u_stride,
                                 const double* std_x, const double* std_u, const uint64_t* seed, uint32_t iter,
                                 double* sums, double* At, double* Bt, double* ct, int* info,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    return smooth_batch_common({__func__, kGeneralBatch, model, params, n_params, mode, T, N, B, x_trj, x_stride,
                                u_trj, u_stride, std_x, std_u, seed, iter, sums, At, Bt, ct, info, workspace,
                                workspace_bytes}, stream);
}

int irs_sums_len(int model, int mode) {
    if (mode < 0 || mode > 2) { irs_set_error("irs_sums_len: unknown mode %d", mode); return IRS_ERR_INVALID_ARG; }
    IRS_DISPATCH_MODEL(model, IRS_DISPATCH_MODE(mode, return (SmoothTraits<Model, MODE>::P)));
    return IRS_ERR_UNSUPPORTED;
}

size_t irs_smooth_workspace_bytes(int model, int mode, int T, int N) {
    int P = irs_sums_len(model, mode);
    if (P <= 0 || T <= 0 || N <= 0) return 0;
    int chunk, nblk, block;
    plan_grid(T, N, is_light(model, mode), /*rng=*/true, &chunk, &nblk, &block,       // the larger grid
              has_nominal_in_wg0(model, mode));
    if (irs_smooth_ug_supported(model, mode)) {
        const int ug = irs_smooth_ug_nblk(T, N);
        if (ug > nblk) nblk = ug;
    }
    return smooth_workspace_size(T, nblk, P);
}

int irs_smooth_geometry(int model, int mode, int T, int N, int rng, int out[8]) {
    IRS_CHECK_ARG(out != nullptr, "null pointer");
    SmoothGeometry g;
    int rc = smooth_geometry(model, mode, T, N, rng != 0, &g);
    if (rc != IRS_OK) return rc;
    out[0] = g.family; out[1] = g.block; out[2] = g.nblk; out[3] = g.chunk0; out[4] = g.chunk; out[5] = g.wg0_rr;
    out[6] = g.branch; out[7] = 0;
    return IRS_OK;
}

int irs_workspace_init(void* workspace, size_t workspace_bytes, void* stream) {
    IRS_CHECK_ARG(workspace != nullptr && workspace_bytes >= kCounterBytes, "workspace too small");
    hipError_t e = hipMemsetAsync(workspace, 0, kCounterBytes, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) { irs_set_error("irs_workspace_init: %s", hipGetErrorString(e)); return IRS_ERR_HIP; }
    return IRS_OK;
}

int irs_smooth_accumulate(int model, const double* params, int n_params, int mode, int T, int N,
                          const double* x_trj, const double* u_trj, const float* dx,
                          const float* du, double* sums, void* workspace,
                          size_t workspace_bytes, void* stream) {
    irs_smooth_call c = positional_call(model, n_params, mode, T, N, x_trj, u_trj, sums, workspace, workspace_bytes);
    c.dx = dx; c.du = du;
    return smooth_common({c, params, nullptr, nullptr, false}, stream);
}

int irs_smooth_accumulate_rng(int model, const double* params, int n_params, int mode, int T, int N,
                              const double* x_trj, const double* u_trj, const double* std_x,
                              const double* std_u, uint64_t seed, uint32_t iter,
                              uint64_t sample_offset, double* sums, void* workspace,
                              size_t workspace_bytes, void* stream) {
    irs_smooth_call c = positional_call(model, n_params, mode, T, N, x_trj, u_trj, sums, workspace, workspace_bytes);
    c.use_rng = 1; c.seed = seed; c.iter = iter; c.sample_offset = sample_offset;
    return smooth_common({c, params, std_x, std_u, false}, stream);
}

int irs_smooth(int model, const double* params, int n_params, int mode, int T, int N,
               const double* x_trj, const double* u_trj, const float* dx, const float* du,
               double* sums, double* At, double* Bt, double* ct, int* info, void* workspace,
               size_t workspace_bytes, void* stream) {
    irs_smooth_call c = positional_call(model, n_params, mode, T, N, x_trj, u_trj, sums, workspace, workspace_bytes);
    c.dx = dx; c.du = du;
    c.At = At; c.Bt = Bt; c.ct = ct; c.info = info;
    return smooth_common({c, params, nullptr, nullptr, true}, stream);
}

int irs_smooth_rng(int model, const double* params, int n_params, int mode, int T, int N,
                   const double* x_trj, const double* u_trj, const double* std_x, const double* std_u,
                   uint64_t seed, uint32_t iter, double* sums, double* At, double* Bt, double* ct,
                   int* info, void* workspace, size_t workspace_bytes, void* stream) {
    irs_smooth_call c = positional_call(model, n_params, mode, T, N, x_trj, u_trj, sums, workspace, workspace_bytes);
    c.use_rng = 1; c.seed = seed; c.iter = iter;
    c.At = At; c.Bt = Bt; c.ct = ct; c.info = info;
    return smooth_common({c, params, std_x, std_u, true}, stream);
}

int irs_smooth_run(const irs_smooth_call* c, void* stream) {
    IRS_CHECK_ARG(c != nullptr, "null call struct");
    return smooth_common({*c, c->params, c->std_x, c->std_u, c->At != nullptr}, stream);
}

int irs_rng_samples(int n, int m, int T, int N, const double* std_x, const double* std_u,
                    uint64_t seed, uint32_t iter, uint64_t sample_offset, float* dx, float* du,
                    void* stream) {
    IRS_CHECK_ARG(T > 0 && N > 0 && dx && du && std_x && std_u, "bad argument");
    SmoothArgs a;
    memset(&a, 0, sizeof(a));
    for (int i = 0; i < n; ++i) a.std[i] = (float)std_x[i];
    for (int j = 0; j < m; ++j) a.std[n + j] = (float)std_u[j];
    a.seed = seed; a.iter = iter; a.sample_offset = sample_offset; a.T = T; a.N = N;
    if (irs_rng_samples_launch(n, m, dx, du, a, static_cast<hipStream_t>(stream)) != IRS_OK) {
        irs_set_error("irs_rng_samples: unsupported (n,m)=(%d,%d)", n, m);
        return IRS_ERR_UNSUPPORTED;
    }
    IRS_CHECK_LAUNCH();
    return IRS_OK;
}

int irs_smooth_finalize(int model, const double* params, int n_params, int mode, int T,
                        long long N_total, const double* x_trj, const double* u_trj,
                        const double* sums, double* At, double* Bt, double* ct, int* info,
                        void* stream) {
    return irs_smooth_finalize_ws(model, params, n_params, mode, T, N_total, x_trj, u_trj, sums, At, Bt, ct, info,
                                  nullptr, 0, stream);
}

int irs_smooth_finalize_ws(int model, const double* params, int n_params, int mode, int T,
                           long long N_total, const double* x_trj, const double* u_trj,
                           const double* sums, double* At, double* Bt, double* ct, int* info,
                           const void* workspace, size_t workspace_bytes, void* stream) {
    IRS_CHECK_ARG(T > 0 && N_total > 0, "T and N_total must be positive");
    IRS_CHECK_ARG(workspace == nullptr || workspace_bytes >= smooth_workspace_size(T, 0, 0),
                  "workspace too small to hold the nominal steps");
    IRS_CHECK_ARG(x_trj && u_trj && sums && At && Bt && ct && info, "null pointer");
    IRS_CHECK_ARG(mode >= 0 && mode <= 2, "unknown smoothing mode");
    SmoothArgs a;
    memset(&a, 0, sizeof(a));
    int rc = irs_load_params(model, params, n_params, &a.p);
    if (rc != IRS_OK) return rc;
    a.x_trj = x_trj; a.u_trj = u_trj; a.sums = const_cast<double*>(sums);
    a.At = At; a.Bt = Bt; a.ct = ct; a.info = info;
    a.n_total = (double)N_total; a.T = T;
    if (workspace != nullptr) a.fnom = smooth_workspace(const_cast<void*>(workspace), T).fnom;
    rc = irs_smooth_finalize_launch(model, mode, a, static_cast<hipStream_t>(stream));
    if (rc != IRS_OK) return rc;
    IRS_CHECK_LAUNCH();
    return IRS_OK;
}

int irs_exact_linearize(int model, const double* params, int n_params, int T, const double* x_trj,
                        const double* u_trj, double* At, double* Bt, double* ct, void* stream) {
    IRS_CHECK_ARG(T > 0 && x_trj && u_trj && At && Bt && ct, "bad argument");
    ModelParams p;
    int rc = irs_load_params(model, params, n_params, &p);
    if (rc != IRS_OK) return rc;
    rc = irs_exact_linearize_launch(model, p, x_trj, u_trj, At, Bt, ct, T, static_cast<hipStream_t>(stream));
    if (rc != IRS_OK) return rc;
    IRS_CHECK_LAUNCH();
    return IRS_OK;
}

}  // extern "C"
