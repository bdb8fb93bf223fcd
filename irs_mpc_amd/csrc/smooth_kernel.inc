// smooth_kernel, the general sample pass: included by smooth.hip (one problem, grid (nblk, T)) and, with
// IRS_SMOOTH_KERNEL_BATCH defined, by smooth_batch.hip (B problems, grid (nblk, B T): `a` is then the row's view of the
// arguments and t the time step within the row's problem -- smooth_common.hpp, SmoothRow).  Two translation units
// rather than one template parameter: this code is SLP-vectorised under -ffp-contract=fast, and a batch parameter in
// front of the single-problem instantiations moved the compiled code of the contact models' kernels.
constexpr int kDeferRing = 128;     // entries per wave: < 64 waiting + <= 64 new ones

template <class Model, int MODE, bool RNG, bool FUSE, int BLOCK>
#ifdef IRS_SMOOTH_KERNEL_BATCH
__global__ __launch_bounds__(BLOCK, (smooth_min_waves<Model, MODE>())) void smooth_kernel(SmoothArgs args, SmoothBatch bat) {
#else
__global__ __launch_bounds__(BLOCK, (smooth_min_waves<Model, MODE>())) void smooth_kernel(SmoothArgs a) {
#endif
    using TR = SmoothTraits<Model, MODE>;
    constexpr int n = TR::n, m = TR::m, d = TR::d, NZ = TR::NZ, Z0 = TR::Z0, P = TR::P;
    constexpr int NW = BLOCK / 64;
    constexpr bool USE_MFMA = gram_on_matrix_cores<Model, MODE>() && BLOCK == kBlock;
    // exact contact models in the lane path: unfinished samples wait in a per-wave ring (see the DEFER branch)
    // Used by the u-only modes of the 8-row models (planar hand, T = 50: zero-order-B 102 -> 79 us at N = 1e4 and
    // 820 -> 606 us at 1e5; first-order 112 -> 76 us).  Measured and left on the plain path: the 12-row box models --
    // 39 % of their samples are unfinished after the first attempt, and W (144) + its factor live across the loop
    // spill 200 VGPRs: 123 -> 225 us.
    constexpr bool DEFER = defer_samples<Model, MODE>();
    // perturbed components of a sample in the u-only modes (NOT TR::NZ: that is the width of the least-squares design,
    // d for the first-order statistics) + the warm set
    constexpr int NPERT = d - Z0;
    constexpr int QE = NPERT + 1;
    __shared__ float defer_ring[DEFER ? NW * kDeferRing * QE : 1];
    __shared__ float red[NW * TR::PP];
    __shared__ float tile[USE_MFMA ? NW * 64 * 36 : 1];
    __shared__ double red64[TR::NGRP * P];
    __shared__ double tot[P];
    __shared__ FinalizeLds<Model, MODE> fin;
    __shared__ int s_ticket;

#ifdef IRS_SMOOTH_KERNEL_BATCH
    const SmoothRow a = smooth_batch_row<Model, MODE>(args, bat, (int)blockIdx.y);
    const int t = a.t, blk = blockIdx.x, tid = threadIdx.x;
#else
    const int t = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
#endif

    // nominal point of this timestep (every lane keeps its own copy in registers)
    float xb[n], ub[m], f0[n];
#pragma unroll
    for (int i = 0; i < n; ++i) xb[i] = (float)a.x_trj[(size_t)t * n + i];
#pragma unroll
    for (int j = 0; j < m; ++j) ub[j] = (float)a.u_trj[(size_t)t * m + j];
    // what the samples' f(x+dx,u+du) is measured from: the nominal step, or (TR::SUMZ) just xb
    if constexpr (MODE != IRS_SMOOTH_FIRST_ORDER && !TR::SUMZ) Model::template step<float>(a.p, xb, ub, f0);
    else {
#pragma unroll
        for (int i = 0; i < n; ++i) f0[i] = xb[i];
    }

    // workgroup 0 owns [0, chunk0), workgroup b >= 1 owns chunk0 + [(b-1) chunk, b chunk)
    const int s_begin = blk == 0 ? 0 : a.chunk0 + (blk - 1) * a.chunk;
    const int s_end = min(a.N, blk == 0 ? a.chunk0 : a.chunk0 + blk * a.chunk);
    constexpr bool NB = nominal_in_wg0<Model, MODE>();
    if constexpr (USE_MFMA) {
        // ---- matrix-core Gram accumulation (zero-order, d <= 16, many statistics) -------
        // The P = d(d+1)/2 + d n statistics are the products Z'Z and Z'dF over the sample
        // axis: exactly what v_mfma_f32_16x16x4_f32 contracts (k = 4 samples per issue),
        // with the accumulators in 8 registers per WAVE instead of P per LANE.  Each lane
        // evaluates one sample, stages [z | df] as a row of its wave's LDS tile (row stride
        // 36 dwords: conflict-free 16-byte writes), and the wave re-reads the tile in
        // operand layout (lane (i = l&15, k = l>>4) <- row 4 kk + k, column i); Z serves as
        // both the A and the B operand of Z'Z.  f32 MFMA is an exact k-ordered fmaf chain.
        typedef float v4f __attribute__((ext_vector_type(4)));
        constexpr int TS = 36;
        const int lane = tid & 63, wave = tid >> 6, col = lane & 15, rg = lane >> 4;
        float* my = tile + wave * 64 * TS;
        v4f aG = {0.f, 0.f, 0.f, 0.f}, aH = {0.f, 0.f, 0.f, 0.f};
        for (int s0 = s_begin + wave * 64; s0 < s_end; s0 += BLOCK) {
            const int s = s0 + lane;
            const bool valid = s < s_end;
            float z[16], dfp[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) { z[i] = 0.f; dfp[i] = 0.f; }
            if constexpr (RNG) {
                const unsigned long long gidx = a.sample_offset + (unsigned long long)s;
#pragma unroll
                for (int j = 0; j < (d + 3) / 4; ++j) {
                    float g[4];
                    philox_normal4(gidx, (unsigned)t, (unsigned)j, a.iter, a.seed, g);
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (4 * j + c < d) z[4 * j + c] = __fmul_rn(g[c], a.std[4 * j + c]);   // rounded like a supplied f32 sample (no fma with the nominal point)
                }
            } else {
                const size_t row = (size_t)t * a.N + (valid ? s : s_end - 1);
                load_row<n>(a.dx + row * n, z);
                load_row<m>(a.du + row * m, z + n);
            }
#pragma unroll
            for (int i = 0; i < d; ++i) z[i] = valid ? z[i] : 0.f;
            float xs[n], us[m], fx[n];
#pragma unroll
            for (int i = 0; i < n; ++i) xs[i] = xb[i] + z[i];
#pragma unroll
            for (int j = 0; j < m; ++j) us[j] = ub[j] + z[n + j];
            Model::template step<float>(a.p, xs, us, fx);
#pragma unroll
            for (int k = 0; k < n; ++k) dfp[k] = fx[k] - f0[k];      // (!SUMZ: 0 for a zeroed slot)
            if constexpr (TR::SUMZ) {
                static_assert(!TR::SUMZ || n < 16, "column n of the dF tile carries the ones that sum z");
                dfp[n < 16 ? n : 0] = 1.f;                           // z of an invalid slot is 0
            }
            float4* rowp = reinterpret_cast<float4*>(my + lane * TS);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                rowp[q] = make_float4(z[4 * q], z[4 * q + 1], z[4 * q + 2], z[4 * q + 3]);
                rowp[4 + q] = make_float4(dfp[4 * q], dfp[4 * q + 1], dfp[4 * q + 2], dfp[4 * q + 3]);
            }
            wave_sync();
#pragma unroll
            for (int kk = 0; kk < 16; ++kk) {
                const float av = my[(4 * kk + rg) * TS + col];
                const float bv = my[(4 * kk + rg) * TS + 16 + col];
                aG = __builtin_amdgcn_mfma_f32_16x16x4f32(av, av, aG, 0, 0, 0);
                aH = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, aH, 0, 0, 0);
            }
            wave_sync();
        }
        // accumulator (row = 4 (l>>4) + reg, col = l&15) -> this wave's row of `red`, P-order
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = 4 * rg + r, j = col;
            if (i < d && j < d && i <= j) red[wave * TR::PP + i * d - i * (i - 1) / 2 + (j - i)] = aG[r];
            if (i < d && j < n) red[wave * TR::PP + TR::NG + i * n + j] = aH[r];
            if constexpr (TR::SUMZ) {
                if (i < d && j == n) red[wave * TR::PP + TR::NH + i] = aH[r];
            }
        }
    } else if constexpr (DEFER) {
        // ---- exact contact models: finished samples accumulate at once, unfinished ones are parked ----------
        // irs_contact_step_try (contact_models.hpp) settles ~90 % of the samples with straight-line code; the
        // rest -- those whose guessed active set needs repair rounds or active-set steps, loops that run as long
        // as a wave's slowest lane -- are parked in this wave's LDS ring (the perturbation + the warm set, m + 1
        // dwords) and finished 64 at a time with every lane busy: as soon as 64 are waiting, and once more after
        // the wave's last sample.  Everything is wave-private and in lane order (ballot prefix, wave-uniform
        // head/tail): no barrier, no atomic, and the same sample lands in the same lane's accumulator in every
        // run -- the fixed-order sums stay bit-reproducible.
        float acc[TR::PP];
#pragma unroll
        for (int i = 0; i < TR::PP; ++i) acc[i] = 0.f;
        const int lane = tid & 63, wave = tid >> 6;
        float* ring = defer_ring + wave * (kDeferRing * QE);
        int qhead = 0, qtail = 0;                           // wave-uniform
        auto accumulate = [&](const float* z, const float* fx, const float* Bs, bool on) {
            if constexpr (TR::FIRST_B) {
#pragma unroll
                for (int q = 0; q < n * m; ++q) acc[q] += on ? Bs[q] : 0.f;
                // the derivative of a step whose command is NaN / Inf is finite (no row tests active): mark it
                bool nf = false;
#pragma unroll
                for (int j = 0; j < m; ++j) nf = nf || irs_nonfinite_bits(z[n + j]);
                if (on && nf) acc[0] = irs_poison();
            } else {
                float zz[NZ], df[n];
#pragma unroll
                for (int i = 0; i < NZ; ++i) zz[i] = on ? z[Z0 + i] : 0.f;
#pragma unroll
                for (int k = 0; k < n; ++k) df[k] = fx[k] - f0[k];
                int q = 0;
#pragma unroll
                for (int i = 0; i < NZ; ++i)
#pragma unroll
                    for (int j = i; j < NZ; ++j) { acc[q] = fmaf(zz[i], zz[j], acc[q]); ++q; }
#pragma unroll
                for (int i = 0; i < NZ; ++i)
#pragma unroll
                    for (int k = 0; k < n; ++k) { acc[q] = fmaf(zz[i], df[k], acc[q]); ++q; }
                if constexpr (TR::SUMZ) {
#pragma unroll
                    for (int i = 0; i < NZ; ++i) { acc[q] += zz[i]; ++q; }
                }
            }
        };
        // One loop, two kinds of trips (the choice is wave-uniform): a FRESH trip takes the wave's next 64 samples
        // through the first attempt; a FLUSH trip takes up to 64 parked samples through the full method.  Both share
        // the assembly of the step QP in front and the primal recovery / derivative / accumulation behind, so the
        // kernel holds one copy of each (two complete inlined steps cost the first-order kernel 137 spilled VGPRs).
        constexpr int NC = Model::NC;
        // trip k of wave w takes 64-sample block 4 k + w of the workgroup; in workgroup 0 the last wave sits out
        // after a.wg0_rr trips (it evaluates the f64 nominal step instead) and the other three share the rest
        int kt = 0;                                         // wave-uniform
        const int rr = blk == 0 ? a.wg0_rr : 0x7fffffff;
        auto block_of = [&](int k) {
            if (k < rr) return NW * k + wave;
            return wave == NW - 1 ? 0x3fffffff : NW * rr + (NW - 1) * (k - rr) + wave;
        };
        int sb = s_begin + 64 * block_of(0);
        constexpr bool HOIST = !TR::FIRST_B;
        float q[n], b0[n], J[NC][n], phi[NC], Dinv[n];
        if constexpr (HOIST) Model::template assemble<float>(a.p, xb, ub, q, Dinv, b0, J, phi);
        while (true) {
            const bool fresh = sb < s_end;
            const int pending = qtail - qhead;
            const bool flush = pending >= 64 || (!fresh && pending > 0);
            if (!fresh && !flush) break;
            float z[d];
            bool on;
            unsigned wm = 0u;
            int take = 0;
            if (flush) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                take = min(64, pending);
                on = lane < take;
                const int slot = (qhead + (on ? lane : 0)) & (kDeferRing - 1);
#pragma unroll
                for (int i = 0; i < Z0; ++i) z[i] = 0.f;
#pragma unroll
                for (int i = 0; i < NPERT; ++i) z[Z0 + i] = ring[slot * QE + i];
                wm = __float_as_uint(ring[slot * QE + NPERT]);
            } else {
                const int sidx = sb + lane;
                on = sidx < s_end;
                if constexpr (RNG) {
                    constexpr int j0 = Z0 / 4;
                    const unsigned long long gidx = a.sample_offset + (unsigned long long)sidx;
#pragma unroll
                    for (int j = j0; j < (d + 3) / 4; ++j) {
                        float g[4];
                        philox_normal4(gidx, (unsigned)t, (unsigned)j, a.iter, a.seed, g);
#pragma unroll
                        for (int c = 0; c < 4; ++c)
                            if (4 * j + c < d) z[4 * j + c] = __fmul_rn(g[c], a.std[4 * j + c]);   // rounded like a supplied f32 sample (no fma with the nominal point)
                    }
#pragma unroll
                    for (int i = 0; i < Z0; ++i) z[i] = 0.f;
                } else {
                    static_assert(Z0 == n && NPERT == m, "the parked-sample loop serves the u-only modes");
#pragma unroll
                    for (int i = 0; i < n; ++i) z[i] = 0.f;
                    // (a register prefetch of the next trip's sample and staging 8 trips through LDS were both measured:
                    // no change -- the load at the head of a trip is not what a trip waits for)
                    const size_t row = (size_t)t * a.N + (on ? sidx : s_end - 1);
                    load_row<NPERT>(a.du + row * NPERT, z + n);
                }
            }
            float xs[n], us[m], fx[n], Bs[TR::FIRST_B ? n * m : 1];
#pragma unroll
            for (int i = 0; i < n; ++i) xs[i] = xb[i] + z[i];
#pragma unroll
            for (int j = 0; j < m; ++j) us[j] = ub[j] + z[n + j];
            // the state is not perturbed in these modes: geometry (q, D, J, phi) assembled ONCE, before the loop; per
            // sample only the actuated entries of b -- the same expression the model's assemble evaluates
            // (zero-order-B: the compiler left ~1 900 cycles of assembly in every trip -- 69.6 -> 63.1 us; in the
            // first-order kernel it hoists by itself and the explicit form costs registers: 68.7 -> 71.3 us, so there
            // the model's assemble stays in the loop)
            float qn[n], bq[n], W[NC][NC], lam[NC];
            if constexpr (HOIST) {
#pragma unroll
                for (int k = 0; k < n; ++k) bq[k] = b0[k];
#pragma unroll
                for (int j = 0; j < m; ++j) bq[Model::act(j)] = Model::template stiffness<float>(a.p, j) * (q[Model::act(j)] - us[j]);
            } else {
                Model::template assemble<float>(a.p, xs, us, q, Dinv, bq, J, phi);
            }
            bool fin_ = true;
            if (flush) {
                irs_contact_qp_dual_exact<float, n, NC>(Dinv, bq, J, phi, W, lam, &wm);
                qhead += take;
            } else {
                unsigned mask = 0u;
                fin_ = irs_contact_qp_dual_exact_try<float, n, NC>(Dinv, bq, J, phi, W, lam, &mask);
                const bool hard = on && !fin_;
                const unsigned long long bal = __ballot(hard);
                if (hard) {
                    const int slot = (qtail + __popcll(bal & ((1ull << lane) - 1ull))) & (kDeferRing - 1);
#pragma unroll
                    for (int i = 0; i < NPERT; ++i) ring[slot * QE + i] = z[Z0 + i];
                    ring[slot * QE + NPERT] = __uint_as_float(mask);
                }
                qtail += __popcll(bal);
                ++kt;
                const int nb_ = block_of(kt);
                sb = nb_ >= 0x3fffffff ? s_end : s_begin + 64 * nb_;
            }
            irs_contact_qp_primal<float, n, NC>(q, Dinv, bq, J, lam, qn);
#pragma unroll
            for (int k = 0; k < n; ++k) fx[Model::perm(k)] = qn[k];
            if constexpr (TR::FIRST_B) {
                int actc[m];
#pragma unroll
                for (int j = 0; j < m; ++j) actc[j] = Model::act(j);
                float Bint[n][m], Aint[1][n];
                irs_contact_qp_grad<float, n, NC, m, false>(Dinv, J, W, lam, actc, Bint, Aint);
#pragma unroll
                for (int k = 0; k < n; ++k)
#pragma unroll
                    for (int j = 0; j < m; ++j) Bs[Model::perm(k) * m + j] = Bint[k][j];
            }
            accumulate(z, fx, Bs, on && fin_);
        }
        block_reduce_lds<P, NW>(acc, red);
    } else {
        float acc[TR::PP];
#pragma unroll
        for (int i = 0; i < TR::PP; ++i) acc[i] = 0.f;
        constexpr int NJC = compact_jac_len<Model>();      // 0: the model has no hand-derived compact Jacobian
        float accj[irs_reduce_pad(NJC + 1)];                // + the number of samples this lane summed
#pragma unroll
        for (int i = 0; i < irs_reduce_pad(NJC + 1); ++i) accj[i] = 0.f;

        // Sample loop.  U samples per lane are loaded together (independent loads in
        // flight), then evaluated; out-of-range slots are clamped to a valid address and
        // zeroed (a zero perturbation contributes exactly nothing to the zero-order sums).
        constexpr int U = (TR::LIGHT && !RNG) ? 4 : 1;
        // kernels whose workgroup 0 evaluates the f64 nominal step deal 64-sample blocks to WAVES (block_of, as in
        // the parked-sample loop above): trip k of wave w takes block NW k + w; in workgroup 0 the last wave sits out
        // after a.wg0_rr trips.  Everything else: the plain strided loop.
        const int rr_ = (NB && blk == 0) ? a.wg0_rr : 0x7fffffff;
        auto next_s0 = [&](int k) {
            if constexpr (NB) {
                if (k < rr_) return s_begin + tid + k * BLOCK;
                if ((tid >> 6) == NW - 1) return s_end;
                return s_begin + 64 * (NW * rr_ + (NW - 1) * (k - rr_)) + tid;
            } else {
                return s_begin + tid + k * BLOCK;
            }
        };
        // One sample per trip and supplied samples (the 16-dimensional analytic models): the NEXT trip's row is requested
        // before this trip's arithmetic starts (quadrotor first-order, N = 1e5: 93 -> 85 us.  Two rows ahead: 92 us --
        // the 16 extra registers and moves cost more than the second request in flight gains)
        constexpr bool PREF = !RNG && !NB && U == 1;
        float zpre[PREF ? d : 1];
        auto request_row = [&](int s) {
            if constexpr (PREF) {
                const size_t row = (size_t)t * a.N + (s < s_end ? s : s_end - 1);
                if constexpr (Z0 == 0) load_row<n>(a.dx + row * n, zpre);
                else {
#pragma unroll
                    for (int i = 0; i < n; ++i) zpre[i] = 0.f;
                }
                load_row<m>(a.du + row * m, zpre + n);
            }
        };
        if (s_begin < s_end) request_row(s_begin + tid);
        int kt_ = 0;
        for (int s0 = s_begin + tid; s0 < s_end; s0 = (NB && U == 1) ? next_s0(++kt_) : s0 + BLOCK * U) {
            float zz[U][d];
            bool valid[U];
#pragma unroll
            for (int uu = 0; uu < U; ++uu) {
                const int s = s0 + uu * BLOCK;
                valid[uu] = s < s_end;
                if constexpr (RNG) {
                    constexpr int j0 = Z0 / 4;
                    const unsigned long long gidx = a.sample_offset + (unsigned long long)s;
#pragma unroll
                    for (int j = j0; j < (d + 3) / 4; ++j) {
                        float g[4];
                        philox_normal4(gidx, (unsigned)t, (unsigned)j, a.iter, a.seed, g);
#pragma unroll
                        for (int c = 0; c < 4; ++c)
                            if (4 * j + c < d) zz[uu][4 * j + c] = __fmul_rn(g[c], a.std[4 * j + c]);   // rounded like a supplied f32 sample (no fma with the nominal point)
                    }
#pragma unroll
                    for (int i = 0; i < Z0; ++i) zz[uu][i] = 0.f;
                } else if constexpr (PREF) {
#pragma unroll
                    for (int i = 0; i < d; ++i) zz[uu][i] = zpre[i];
                    request_row(s0 + BLOCK);
                } else {
                    const size_t row = (size_t)t * a.N + (valid[uu] ? s : s_end - 1);
                    if constexpr (Z0 == 0) load_row<n>(a.dx + row * n, zz[uu]);
                    else {
#pragma unroll
                        for (int i = 0; i < n; ++i) zz[uu][i] = 0.f;
                    }
                    load_row<m>(a.du + row * m, zz[uu] + n);
                }
            }
#pragma unroll
            for (int uu = 0; uu < U; ++uu) {
                float z[d];
#pragma unroll
                for (int i = 0; i < d; ++i) z[i] = (U == 1 || valid[uu]) ? zz[uu][i] : 0.f;
                float xs[n], us[m], fx[n];
#pragma unroll
                for (int i = 0; i < n; ++i) xs[i] = xb[i] + z[i];
#pragma unroll
                for (int j = 0; j < m; ++j) us[j] = ub[j] + z[n + j];

                if constexpr (TR::FIRST_B) {
                    float Bs[n * m];
                    irs_contact_step_grad<Model, float, false>(a.p, xs, us, fx, Bs, nullptr);
#pragma unroll
                    for (int q = 0; q < n * m; ++q) acc[q] += Bs[q];
                    bool nf = false;
#pragma unroll
                    for (int j = 0; j < m; ++j) nf = nf || irs_nonfinite_bits(z[n + j]);
                    if (nf) acc[0] = irs_poison();
                } else if constexpr (MODE == IRS_SMOOTH_FIRST_ORDER && has_compact_jac<Model>::value) {
                    // hand-derived Jacobian, only its sample-dependent entries (models.hpp, step_jac): the full n x d
                    // sum is put together once per workgroup after the loop
                    float Jc[NJC];
                    Model::template step_jac<float>(a.p, xs, us, fx, Jc);
                    const float w = (U == 1 || valid[uu]) ? 1.f : 0.f;
#pragma unroll
                    for (int q = 0; q < NJC; ++q) accj[q] = fmaf(w, Jc[q], accj[q]);
                    accj[NJC] += w;
                } else if constexpr (MODE == IRS_SMOOTH_FIRST_ORDER) {
                    float J[n * d];
                    model_jacobian<Model, float>(a.p, xs, us, fx, J);
                    const float w = (U == 1 || valid[uu]) ? 1.f : 0.f;
#pragma unroll
                    for (int q = 0; q < n * d; ++q) acc[q] = fmaf(w, J[q], acc[q]);
                } else {
                    Model::template step<float>(a.p, xs, us, fx);
                    float df[n];
#pragma unroll
                    for (int k = 0; k < n; ++k) df[k] = fx[k] - f0[k];
                    int q = 0;
#pragma unroll
                    for (int i = 0; i < NZ; ++i)
#pragma unroll
                        for (int j = i; j < NZ; ++j) { acc[q] = fmaf(z[Z0 + i], z[Z0 + j], acc[q]); ++q; }
#pragma unroll
                    for (int i = 0; i < NZ; ++i)
#pragma unroll
                        for (int k = 0; k < n; ++k) { acc[q] = fmaf(z[Z0 + i], df[k], acc[q]); ++q; }
                    if constexpr (TR::SUMZ) {
#pragma unroll
                        for (int i = 0; i < NZ; ++i) { acc[q] += z[Z0 + i]; ++q; }
                    }
                }
            }
        }

        if constexpr (MODE == IRS_SMOOTH_FIRST_ORDER && has_compact_jac<Model>::value) {
            // the workgroup reduces the COMPACT sums (34 numbers, not 192), adds the waves' rows in a fixed order, and
            // only then lays the n x d sum out as `red`'s row 0 (the other rows zero)
            constexpr int PC = irs_reduce_pad(NJC + 1);
            __shared__ float redc[NW * PC + PC];
            block_reduce_lds<NJC + 1, NW>(accj, redc);
            __syncthreads();
            if (tid <= NJC) {
                float tsum = 0.f;
#pragma unroll
                for (int w = 0; w < NW; ++w) tsum += redc[w * PC + tid];
                redc[NW * PC + tid] = tsum;
            }
            __syncthreads();
            for (int q = tid; q < NW * TR::PP; q += BLOCK) {
                const int w = q / TR::PP, e = q - w * TR::PP;
                red[q] = (w == 0 && e < P) ? Model::template expand_entry<float>(a.p, redc + NW * PC, redc[NW * PC + NJC], e) : 0.f;
            }
        } else {
            // ---- workgroup reduction: registers -> shuffles -> LDS ---------------------
            block_reduce_lds<P, NW>(acc, red);
        }
    }
    if constexpr (NB) {
        // (a lone fused workgroup lets its solve evaluate the step itself: same cost, no round trip)
        constexpr int NOMW = NW - 1;                        // the wave that evaluates it: the one that is dealt fewer
                                                           // sample trips (a.wg0_rr)
        if (blk == 0 && (a.nblk > 1 || !FUSE) && (tid >> 6) == NOMW) {
            double x64[n], u64[m], f64[n];
#pragma unroll
            for (int i = 0; i < n; ++i) x64[i] = a.x_trj[(size_t)t * n + i];
#pragma unroll
            for (int j = 0; j < m; ++j) u64[j] = a.u_trj[(size_t)t * m + j];
            Model::template step<double>(a.p, x64, u64, f64);
            if ((tid & 63) == 0) {
#pragma unroll
                for (int i = 0; i < n; ++i)
                    __hip_atomic_store(a.fnom + (size_t)t * n + i, f64[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    smooth_finish<Model, MODE, FUSE, BLOCK>(a, red, red64, tot, fin, s_ticket, t, blk, tid,
                                            (NB && a.nblk > 1) ? a.fnom + (size_t)t * n : nullptr);
}
