// The values pass: the zero-order sample pass of irs_lqr/irs_lqr_zero_order.py:38-63 for a system that has NO device
// functor.  The caller evaluated its own dynamics -- fz = f(x_t + dx, u_t + du) for every sample, f0 = f(x_t, u_t),
// both in f32 by the same code -- and this unit turns the values into the per-timestep statistics
//     sums[t] = [ upper(Z'Z) row-major (d(d+1)/2) | Z'dF (d n) ],   z = [dx | du],  dF = fz - f0 (formed here, in f32)
// (the IRS_SMOOTH_ZERO_ORDER_AB layout of irs_sums_len, for runtime 1 <= n <= 32, 1 <= m <= 16) and solves
//     [A_t | B_t] = lstsq(Z, dF)',   c_t = fnom_t - A_t x_t - B_t u_t
// by the Jacobi-scaled Cholesky of the normal equations in f64 that lstsq_kernel (tvlqr.hip) and finalize_timestep
// (smooth_common.hpp) use.
//
//   values_kernel<DT, NT>   grid (nblk, T) x 256 threads; DT = ceil(d/16), NT = ceil(n/16) 16-wide tiles.
//     A wave takes 64-sample blocks of its workgroup's chunk.  A block of a (T,N,cols) tensor is ONE contiguous span
//     of 64 cols floats: the wave loads it flat, one aligned 16-byte load per lane per trip, and scatters the words to
//     rows [z | 0.. | dF | 0..] of its LDS tile (zero padding up to the tile widths; slots beyond N are zero rows).
//     It re-reads the tile in operand layout and contracts four samples per v_mfma_f32_16x16x4_f32: the DT(DT+1)/2
//     upper tiles of Z'Z and the DT NT tiles of Z'dF (at most 6 + 6) stay in registers.  Every kFlushTrips trips the
//     f32 accumulators are added into f64 ones and cleared.  The four waves add their f64 accumulators into one LDS
//     image in wave order, and the workgroup stores its partial (P f64) to the workspace with plain stores.
//   values_finish_kernel<REDUCE, SOLVE>   grid T x 256 threads.
//     REDUCE: the nblk partials of the timestep are added in index order -> sums[t].  SOLVE: the workgroup solves
//     from the sums.  The launch boundary is the hand-off: no counters, no atomics, nothing to zero in the workspace.
//
//   values_rng_kernel   the compiled models' Philox sample stream written out for runtime (n, m) (irs_rng_samples
//     serves the compiled sizes only).
//
// Every summation order is fixed by (T, N) alone (values_plan), so the same inputs give the same bits on every run.
#include "irs_common.hpp"
#include "philox.hpp"
#include "wave.hpp"

namespace {

constexpr int kMaxN = 32;           // the limits of the generic Riccati kernel (tvlqr.hip)
constexpr int kMaxM = 16;
constexpr int kMaxT = 1024;
constexpr int kBlock = 256;         // 4 waves
constexpr int kFlushTrips = 16;     // f32 accumulators hold at most 16 x 64 samples before they move to f64
constexpr int kSamplesPerWg = 2048; // 8 trips per wave where N allows
constexpr int kFillWgs = 512;       // workgroups that cover the device twice
constexpr int kMaxWgs = 4096;       // ... and bound the partials in the workspace

typedef float v4f __attribute__((ext_vector_type(4)));

// row stride of a wave's tile in dwords: == 16 (mod 32), so that the four sample rows one operand read touches fall
// on disjoint banks (ds_read_b32: 32 banks per 32-lane half), and a multiple of 4 (16-byte rows)
constexpr int tile_stride(int width) { return width % 32 == 16 ? width : width + 16; }

struct ValuesArgs {
    const float* dx; const float* du; const float* fz; const float* f0;
    double* partial;            // (T, nblk, P)
    int n, m, T, N, nblk;
    long long chunk;            // samples per workgroup, a multiple of kBlock
};

struct FinishArgs {
    const double* partial;      // REDUCE
    double* sums;               // written (REDUCE) or read
    const double* x_trj; const double* u_trj; const double* fnom;
    double* At; double* Bt; double* ct; int* info;
    long long n_total;          // samples per timestep behind the sums (SOLVE)
    int n, m, T, nblk;
};

__host__ __device__ inline int values_sums_len(int n, int m) { return (n + m) * (n + m + 1) / 2 + (n + m) * n; }

// workgroups per timestep and samples per workgroup, from (T, N) only
void values_plan(int T, int N, int* nblk, long long* chunk) {
    const long long by_wg = ((long long)N + kBlock - 1) / kBlock;             // one trip per wave at least
    long long nb = ((long long)N + kSamplesPerWg - 1) / kSamplesPerWg;
    long long fill = (kFillWgs + T - 1) / T;
    if (fill > by_wg) fill = by_wg;
    if (nb < fill) nb = fill;
    long long cap = kMaxWgs / T;
    if (cap < 1) cap = 1;
    if (nb > cap) nb = cap;
    if (nb < 1) nb = 1;
    long long c = ((long long)N + nb - 1) / nb;
    c = (c + kBlock - 1) / kBlock * kBlock;
    *chunk = c;
    *nblk = (int)(((long long)N + c - 1) / c);
}

// `count` floats from element e0 of `src` (total floats in the tensor: `total`; base 16-byte aligned) -> columns
// col_off.. of the tile rows, `cols` per row; `sub` (LDS, cols floats) is subtracted column-wise where given.
// Aligned 16-byte loads; the words of the first and last load that lie outside the span are dropped, and a load that
// would cross the tensor's end is done word by word.
template <int TS>
__device__ __forceinline__ void load_span(const float* __restrict__ src, size_t total, size_t e0, int count, int cols,
                                          float* tile, int col_off, const float* sub, int lane) {
    const size_t q0 = e0 >> 2, q1 = (e0 + (size_t)count + 3) >> 2;
    for (size_t q = q0 + lane; q < q1; q += 64) {
        const size_t e = q << 2;
        float v[4];
        if (e + 4 <= total) {
            const float4 w = *reinterpret_cast<const float4*>(src + e);
            v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = e + c < total ? src[e + c] : 0.f;
        }
        const int l = (int)((long long)e - (long long)e0);           // >= -3
        const int lr = l < 0 ? 0 : l;
        int row = lr / cols, cc = lr - row * cols;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (l + c >= 0 && l + c < count) {
                tile[row * TS + col_off + cc] = sub != nullptr ? v[c] - sub[cc] : v[c];
                if (++cc == cols) { cc = 0; ++row; }
            }
        }
    }
}

template <int DT, int NT>
__global__ __launch_bounds__(kBlock) void values_kernel(ValuesArgs a) {
    constexpr int W = (DT + NT) * 16, TS = tile_stride(W), NG = DT * (DT + 1) / 2, NH = DT * NT, NA = NG + NH;
    constexpr int NW = kBlock / 64;
    static_assert((size_t)NW * 64 * TS * sizeof(float) >= (size_t)(8 * DT * (16 * DT + 1) + 256 * DT * NT) * sizeof(double),
                  "the tiles hold the workgroup's f64 image of the statistics");
    __shared__ __attribute__((aligned(16))) float tiles[NW * 64 * TS];
    __shared__ float f0s[kMaxN];

    const int n = a.n, m = a.m, d = n + m;
    const int t = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6, col = lane & 15, rg = lane >> 4;
    float* my = tiles + wave * 64 * TS;
    if (tid < kMaxN) f0s[tid] = tid < n ? a.f0[(size_t)t * n + tid] : 0.f;
    for (int q = lane; q < 64 * TS; q += 64) my[q] = 0.f;            // the padding columns stay zero from here on
    __syncthreads();

    v4f acc[NA];
    double acc64[NA][4];
#pragma unroll
    for (int q = 0; q < NA; ++q) {
        acc[q] = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < 4; ++r) acc64[q][r] = 0.0;
    }
    auto flush = [&]() {
#pragma unroll
        for (int q = 0; q < NA; ++q) {
#pragma unroll
            for (int r = 0; r < 4; ++r) acc64[q][r] += (double)acc[q][r];
            acc[q] = v4f{0.f, 0.f, 0.f, 0.f};
        }
    };

    const long long s_begin = (long long)blk * a.chunk;
    const long long s_end = s_begin + a.chunk < (long long)a.N ? s_begin + a.chunk : (long long)a.N;
    const size_t total_x = (size_t)a.T * (size_t)a.N * n, total_u = (size_t)a.T * (size_t)a.N * m;
    int trip = 0;
    for (long long s0 = s_begin + wave * 64; s0 < s_end; s0 += kBlock, ++trip) {
        const int cnt = s_end - s0 < 64 ? (int)(s_end - s0) : 64;
        if (cnt < 64) {                                              // the ragged end of the timestep: zero rows
            for (int q = lane; q < 64 * TS; q += 64) my[q] = 0.f;
            wave_sync();
        }
        const size_t row0 = (size_t)t * (size_t)a.N + (size_t)s0;
        load_span<TS>(a.dx, total_x, row0 * n, cnt * n, n, my, 0, nullptr, lane);
        load_span<TS>(a.du, total_u, row0 * m, cnt * m, m, my, n, nullptr, lane);
        load_span<TS>(a.fz, total_x, row0 * n, cnt * n, n, my, 16 * DT, f0s, lane);
        wave_sync();
#pragma unroll 4
        for (int kk = 0; kk < 16; ++kk) {
            // lane (i = l & 15, k = l >> 4) <- sample row 4 kk + k, column 16 c + i of tile column c
            float v[DT + NT];
#pragma unroll
            for (int c = 0; c < DT + NT; ++c) v[c] = my[(4 * kk + rg) * TS + 16 * c + col];
            int q = 0;
#pragma unroll
            for (int ti = 0; ti < DT; ++ti)
#pragma unroll
                for (int tj = ti; tj < DT; ++tj) { acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(v[ti], v[tj], acc[q], 0, 0, 0); ++q; }
#pragma unroll
            for (int ti = 0; ti < DT; ++ti)
#pragma unroll
                for (int tk = 0; tk < NT; ++tk) { acc[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(v[ti], v[DT + tk], acc[q], 0, 0, 0); ++q; }
        }
        wave_sync();
        if ((trip & (kFlushTrips - 1)) == kFlushTrips - 1) flush();
    }
    flush();

    // the four waves' accumulators -> one f64 image of the P statistics, added in wave order (the tiles are done with)
    __syncthreads();
    double* red = reinterpret_cast<double*>(tiles);
    const int P = values_sums_len(n, m), PG = d * (d + 1) / 2;
    for (int w = 0; w < NW; ++w) {
        if (wave == w) {
            // accumulator (row = 4 (l >> 4) + reg, col = l & 15) of tile (ti, tj)
            int q = 0;
#pragma unroll
            for (int ti = 0; ti < DT; ++ti)
#pragma unroll
                for (int tj = ti; tj < DT; ++tj) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int i = 16 * ti + 4 * rg + r, j = 16 * tj + col;
                        if (j < d && i <= j) {
                            const int idx = i * d - i * (i - 1) / 2 + (j - i);
                            red[idx] = w == 0 ? acc64[q][r] : red[idx] + acc64[q][r];
                        }
                    }
                    ++q;
                }
#pragma unroll
            for (int ti = 0; ti < DT; ++ti)
#pragma unroll
                for (int tk = 0; tk < NT; ++tk) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int i = 16 * ti + 4 * rg + r, k = 16 * tk + col;
                        if (i < d && k < n) {
                            const int idx = PG + i * n + k;
                            red[idx] = w == 0 ? acc64[q][r] : red[idx] + acc64[q][r];
                        }
                    }
                    ++q;
                }
        }
        __syncthreads();
    }
    double* out = a.partial + ((size_t)t * a.nblk + blk) * P;
    for (int q = tid; q < P; q += kBlock) out[q] = red[q];
}

__device__ __forceinline__ bool nonfinite_f64(double v) {
    return ((unsigned long long)__double_as_longlong(v) & 0x7ff0000000000000ull) == 0x7ff0000000000000ull;
}

template <bool REDUCE, bool SOLVE>
__global__ __launch_bounds__(kBlock) void values_finish_kernel(FinishArgs a) {
    constexpr int D = kMaxN + kMaxM;
    __shared__ double G[SOLVE ? D : 1][D + 1];
    __shared__ double H[SOLVE ? D : 1][kMaxN];
    __shared__ double sc[D];
    __shared__ int nonfin, bad;
    const int n = a.n, m = a.m, d = n + m, t = blockIdx.x, tid = threadIdx.x;
    const int P = values_sums_len(n, m), PG = d * (d + 1) / 2;
    if (tid == 0) { nonfin = 0; bad = 0; }
    __syncthreads();
    // statistic q of this timestep: the partials added in index order (and stored), or the supplied sum
    auto stat = [&](int q) {
        if constexpr (REDUCE) {
            double s = 0.0;
            for (int b = 0; b < a.nblk; ++b) s += a.partial[((size_t)t * a.nblk + b) * P + q];
            a.sums[(size_t)t * P + q] = s;
            return s;
        } else {
            return a.sums[(size_t)t * P + q];
        }
    };
    if constexpr (!SOLVE) {
        for (int q = tid; q < P; q += kBlock) stat(q);
        return;
    } else {
        for (int e = tid; e < d * d; e += kBlock) {
            const int i = e / d, j = e % d;
            if (j < i) continue;
            const double s = stat(i * d - i * (i - 1) / 2 + (j - i));
            if (nonfinite_f64(s)) nonfin = 1;
            G[i][j] = s;
            G[j][i] = s;
        }
        for (int e = tid; e < d * n; e += kBlock) {
            const double s = stat(PG + e);
            if (nonfinite_f64(s)) nonfin = 1;
            H[e / n][e % n] = s;
        }
        __syncthreads();
        // ---- lstsq_kernel's solve (tvlqr.hip): Jacobi scaling, right-looking Cholesky with the forward substitution
        // folded in, back substitution -- dealt over the whole workgroup: thread (r = tid & 63, cg = tid >> 6) owns
        // row r (d <= 48 < 64) and every fourth column from cg on, so a pivot step is d / 4 + n / 4 updates per
        // thread without an index division (one wave walking all d d + d n entries took 380 us at d = 48)
        const int r = tid & 63, cg = tid >> 6;
        if (tid < 64) {
            const double g = r < d ? G[r][r] : 1.0;
            const int first = wave_min(g > 0.0 ? 0x7fffffff : r + 1);
            if (tid == 0 && first != 0x7fffffff) bad = first;
            if (r < d) sc[r] = g > 0.0 ? 1.0 / sqrt(g) : 0.0;
        }
        __syncthreads();
        for (int q = tid; q < d * d; q += kBlock) G[q / d][q % d] *= sc[q / d] * sc[q % d];
        for (int q = tid; q < d * n; q += kBlock) H[q / n][q % n] *= sc[q / n];
        __syncthreads();
        for (int j = 0; j < d; ++j) {
            double djj = G[j][j];
            // (rank(Z'Z) <= N_total: from pivot N_total + 1 on the exact pivot is zero, whatever sign the rounding of
            // the f32 statistics left on the computed one)
            if (!(djj > 1e-14) || j >= a.n_total) {
                if (tid == 0 && bad == 0) bad = j + 1;
                djj = 1.0;
            }
            const double il = 1.0 / sqrt(djj);
            __syncthreads();                                 // every thread holds the pivot
            if (tid == j) G[j][j] = il;
            if (cg == 0 && r > j && r < d) G[r][j] *= il;
            if (cg == 1 && r < n) H[j][r] *= il;
            __syncthreads();
            if (r > j && r < d) {                            // column j and row j of H are only read here
                const double lrj = G[r][j];
                for (int c = j + 1 + cg; c <= r; c += kBlock / 64) G[r][c] -= lrj * G[c][j];
                for (int k = cg; k < n; k += kBlock / 64) H[r][k] -= lrj * H[j][k];
            }
            __syncthreads();
        }
        for (int i = d - 1; i >= 0; --i) {                   // L' w = y, column oriented
            if (tid < n) H[i][tid] *= G[i][i];
            __syncthreads();
            if (r < i) {
                const double g = G[i][r];
                for (int k = cg; k < n; k += kBlock / 64) H[r][k] -= g * H[i][k];
            }
            __syncthreads();
        }
        // [A | B][k][i] = X[i][k] / scale_i;   c = fnom - A x - B u
        double* A = a.At + (size_t)t * n * n;
        double* B = a.Bt + (size_t)t * n * m;
        for (int q = tid; q < n * n; q += kBlock) A[q] = H[q % n][q / n] * sc[q % n];
        for (int q = tid; q < n * m; q += kBlock) B[q] = H[n + q % m][q / m] * sc[n + q % m];
        if (tid < n) {
            double c = a.fnom[(size_t)t * n + tid];
            for (int i = 0; i < n; ++i) c -= H[i][tid] * sc[i] * a.x_trj[(size_t)t * n + i];
            for (int j = 0; j < m; ++j) c -= H[n + j][tid] * sc[n + j] * a.u_trj[(size_t)t * m + j];
            a.ct[(size_t)t * n + tid] = c;
        }
        if (tid == 0) a.info[t] = nonfin ? d + 1 : bad;
    }
}

// The sample stream of the compiled models' sample pass (philox.hpp; smooth.hip rng_samples_kernel) for runtime
// (n, m): thread (s, t, j) draws block j of sample s at timestep t -- components 4j .. 4j+3 of z = [dx | du] -- and
// writes each as the f32 product with its std, the value a supplied f32 sample would hold.
struct RngArgs {
    float std[kMaxN + kMaxM];
    unsigned long long seed, sample_offset;
    unsigned iter;
    int n, m, N;
};

__global__ __launch_bounds__(kBlock) void values_rng_kernel(float* dx, float* du, RngArgs a) {
    const int t = blockIdx.y, j = blockIdx.z;
    const long long s = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (s >= a.N) return;
    float z[4];
    philox_normal4(a.sample_offset + (unsigned long long)s, (unsigned)t, (unsigned)j, a.iter, a.seed, z);
    const size_t row = (size_t)t * a.N + (size_t)s;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = 4 * j + k;
        if (c < a.n) dx[row * a.n + c] = __fmul_rn(z[k], a.std[c]);
        else if (c < a.n + a.m) du[row * a.m + (c - a.n)] = __fmul_rn(z[k], a.std[c]);
    }
}

template <int DT, int NT>
void launch_values_t(const ValuesArgs& a, hipStream_t st) {
    hipLaunchKernelGGL((values_kernel<DT, NT>), dim3(a.nblk, a.T), dim3(kBlock), 0, st, a);
}

void launch_values(const ValuesArgs& a, hipStream_t st) {
    const int DT = (a.n + a.m + 15) / 16, NT = (a.n + 15) / 16;     // NT <= DT
    if (DT == 1) launch_values_t<1, 1>(a, st);
    else if (DT == 2 && NT == 1) launch_values_t<2, 1>(a, st);
    else if (DT == 2) launch_values_t<2, 2>(a, st);
    else if (NT == 1) launch_values_t<3, 1>(a, st);
    else launch_values_t<3, 2>(a, st);
}

bool sizes_ok(int n, int m, int T, long long N) {
    return n >= 1 && n <= kMaxN && m >= 1 && m <= kMaxM && T >= 1 && T <= kMaxT && N >= 1 && N <= 0x7fffffffLL;
}
const char* kSizesMsg = "need 1<=n<=32, 1<=m<=16, 1<=T<=1024, N>=1";

size_t round256(size_t b) { return (b + 255) / 256 * 256; }

// An upper bound of T * nblk that does not decrease in T or in N, so that a workspace sized for a caller's largest
// (T, N) serves every smaller call.  (T * nblk itself saws: nblk is recounted after the chunk is rounded up to whole
// trips, and T * ceil(512 / T), T * floor(4096 / T) are not monotone in T.)  values_plan's nblk is at most
// nb = max(1, min(cap, max(by_samples, min(fill, by_wg)))) with T * fill <= 511 + T and T * cap <= 4096 (T <= 1024);
// every term below is non-decreasing in T and in N, and so are their minima and maxima.
long long partials_bound(int T, int N) {
    const long long by_wg = ((long long)N + kBlock - 1) / kBlock;
    const long long by_samples = ((long long)N + kSamplesPerWg - 1) / kSamplesPerWg;
    long long w = kFillWgs - 1 + T;
    if (w > (long long)T * by_wg) w = (long long)T * by_wg;
    if (w < (long long)T * by_samples) w = (long long)T * by_samples;
    if (w > kMaxWgs) w = kMaxWgs;
    if (w < T) w = T;
    return w;
}

size_t workspace_bytes(int n, int m, int T, int N) {
    return round256((size_t)partials_bound(T, N) * values_sums_len(n, m) * sizeof(double));
}

// the argument checks of the two entries that run the sample pass; nothing here calls HIP
int check_pass(const char* fn, int n, int m, int T, int N, const float* dx, const float* du, const float* fz,
               const float* f0, const double* sums, const void* workspace, size_t bytes) {
    if (!sizes_ok(n, m, T, N)) { irs_set_error("%s: %s", fn, kSizesMsg); return IRS_ERR_INVALID_ARG; }
    if (!(dx && du && fz && f0 && sums)) { irs_set_error("%s: null pointer", fn); return IRS_ERR_INVALID_ARG; }
    if (((reinterpret_cast<uintptr_t>(dx) | reinterpret_cast<uintptr_t>(du) | reinterpret_cast<uintptr_t>(fz)) & 15) != 0) {
        irs_set_error("%s: dx / du / fz must be 16-byte aligned", fn);
        return IRS_ERR_INVALID_ARG;
    }
    const size_t need = workspace_bytes(n, m, T, N);
    if (workspace == nullptr || bytes < need) {
        irs_set_error("%s: workspace %zu < %zu bytes", fn, workspace ? bytes : (size_t)0, need);
        return IRS_ERR_WORKSPACE;
    }
    if ((reinterpret_cast<uintptr_t>(workspace) & 255) != 0) {
        irs_set_error("%s: the workspace must be 256-byte aligned", fn);
        return IRS_ERR_WORKSPACE;
    }
    return IRS_OK;
}

ValuesArgs pass_args(int n, int m, int T, int N, const float* dx, const float* du, const float* fz, const float* f0,
                     void* workspace) {
    ValuesArgs a{dx, du, fz, f0, static_cast<double*>(workspace), n, m, T, N, 0, 0};
    values_plan(T, N, &a.nblk, &a.chunk);
    return a;
}

}  // namespace

extern "C" {

int irs_values_sums_len(int n, int m) {
    IRS_CHECK_ARG(n >= 1 && n <= kMaxN && m >= 1 && m <= kMaxM, "need 1<=n<=32, 1<=m<=16");
    return values_sums_len(n, m);
}

size_t irs_smooth_values_workspace_bytes(int n, int m, int T, int N) {
    if (!sizes_ok(n, m, T, N)) return 0;
    return workspace_bytes(n, m, T, N);
}

int irs_smooth_values_geometry(int T, int N, long long out[4]) {
    IRS_CHECK_ARG(T >= 1 && T <= kMaxT && N >= 1, "need 1<=T<=1024, N>=1");
    IRS_CHECK_ARG(out != nullptr, "null pointer");
    int nblk; long long chunk;
    values_plan(T, N, &nblk, &chunk);
    out[0] = kBlock; out[1] = nblk; out[2] = chunk; out[3] = kFlushTrips;
    return IRS_OK;
}

int irs_values_rng_samples(int n, int m, int T, int N, const double* std_x, const double* std_u, uint64_t seed,
                           uint32_t iter, uint64_t sample_offset, float* dx, float* du, void* stream) {
    IRS_CHECK_ARG(sizes_ok(n, m, T, N), kSizesMsg);
    IRS_CHECK_ARG(std_x && std_u && dx && du, "null pointer");
    RngArgs a;
    memset(&a, 0, sizeof(a));
    for (int i = 0; i < n; ++i) a.std[i] = (float)std_x[i];
    for (int j = 0; j < m; ++j) a.std[n + j] = (float)std_u[j];
    a.seed = seed; a.sample_offset = sample_offset; a.iter = iter; a.n = n; a.m = m; a.N = N;
    const dim3 grid((unsigned)(((long long)N + kBlock - 1) / kBlock), T, (n + m + 3) / 4);
    hipLaunchKernelGGL(values_rng_kernel, grid, dim3(kBlock), 0, static_cast<hipStream_t>(stream), dx, du, a);
    IRS_CHECK_LAUNCH();
    return IRS_OK;
}

int irs_smooth_values_accumulate(int n, int m, int T, int N, const float* dx, const float* du, const float* fz,
                                 const float* f0, double* sums, void* workspace, size_t workspace_bytes,
                                 void* stream) {
    int rc = check_pass(__func__, n, m, T, N, dx, du, fz, f0, sums, workspace, workspace_bytes);
    if (rc != IRS_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const ValuesArgs a = pass_args(n, m, T, N, dx, du, fz, f0, workspace);
    launch_values(a, st);
    IRS_CHECK_LAUNCH();
    FinishArgs f{a.partial, sums, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, n, m, T, a.nblk};
    hipLaunchKernelGGL((values_finish_kernel<true, false>), dim3(T), dim3(kBlock), 0, st, f);
    IRS_CHECK_LAUNCH();
    return IRS_OK;
}

int irs_smooth_values_finalize(int n, int m, int T, long long N_total, const double* x_trj, const double* u_trj,
                               const double* fnom, const double* sums, double* At, double* Bt, double* ct, int* info,
                               void* stream) {
    IRS_CHECK_ARG(sizes_ok(n, m, T, 1) && N_total >= 1, "need 1<=n<=32, 1<=m<=16, 1<=T<=1024, N_total>=1");
    IRS_CHECK_ARG(x_trj && u_trj && fnom && sums && At && Bt && ct && info, "null pointer");
    FinishArgs f{nullptr, const_cast<double*>(sums), x_trj, u_trj, fnom, At, Bt, ct, info, N_total, n, m, T, 0};
    hipLaunchKernelGGL((values_finish_kernel<false, true>), dim3(T), dim3(kBlock), 0, static_cast<hipStream_t>(stream), f);
    IRS_CHECK_LAUNCH();
    return IRS_OK;
}

int irs_smooth_values(int n, int m, int T, int N, const double* x_trj, const double* u_trj, const float* dx,
                      const float* du, const float* fz, const float* f0, const double* fnom, double* sums, double* At,
                      double* Bt, double* ct, int* info, void* workspace, size_t workspace_bytes, void* stream) {
    int rc = check_pass(__func__, n, m, T, N, dx, du, fz, f0, sums, workspace, workspace_bytes);
    if (rc != IRS_OK) return rc;
    IRS_CHECK_ARG(x_trj && u_trj && fnom && At && Bt && ct && info, "null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const ValuesArgs a = pass_args(n, m, T, N, dx, du, fz, f0, workspace);
    launch_values(a, st);
    IRS_CHECK_LAUNCH();
    FinishArgs f{a.partial, sums, x_trj, u_trj, fnom, At, Bt, ct, info, N, n, m, T, a.nblk};
    hipLaunchKernelGGL((values_finish_kernel<true, true>), dim3(T), dim3(kBlock), 0, st, f);
    IRS_CHECK_LAUNCH();
    return IRS_OK;
}

}  // extern "C"
