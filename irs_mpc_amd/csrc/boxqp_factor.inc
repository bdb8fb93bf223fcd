// The factorisation of box_descent_kernel (boxqp.hip), as text: included there once for the whole horizon and, in the
// adaptive kernel, once more where a new rho asks for it -- with BOX_FACTOR_FROM the first step to factorise (a record
// depends on the later steps only).  Text and not a function or a lambda, because either changes the registers and
// the schedule the compiler gives the fixed-rho kernel, which has to stay the code it was.  Reads the kernel's
// locals (a, lane, T, hr, the LDS pointers, the accessors), writes P, the records and `bad`.
    // P_T = Qd + rho/2 Mx ; qx_T = Qd xd_T
    for (int q = lane; q < N * N; q += 64) {
        int i = q / N, j = q % N;
        P[q] = qs(a.Qd, i, j) + (i == j ? hr * mxv[i] : 0.0);
    }
    if (lane < N) {
        double s = 0.0;
        for (int j = 0; j < N; ++j) s += qs(a.Qd, lane, j) * xd_(T, j);
        qxT[lane] = s;
    }
    wave_sync();

    // ---- backward Riccati with Q^ = Q + rho/2 Mx, R^ = alpha R + rho/2 Mu --
    for (int t = T - 1; t >= BOX_FACTOR_FROM; --t) {
        // HBM: records T-1 and T-2 are built in the ring slots the first sweep reads them from, the rest in the third
        double* rec = HBM ? F + (size_t)((t >= T - 2 ? t : T - 3) % L::RING) * L::SP : F + (size_t)t * L::S;
        for (int q = lane; q < N * N; q += 64) Am[q] = A_(t, q / N, q % N);
        for (int q = lane; q < N * M; q += 64) rec[L::oB + q] = B_(t, q / M, q % M);
        if (lane < N) {
            rec[L::oC + lane] = c_(t, lane);
            double s = 0.0;
            for (int j = 0; j < N; ++j) s += qs(a.Q, lane, j) * xd_(t, j);
            rec[L::oQx + lane] = s;
        }
        wave_sync();
        const double* B = rec + L::oB;
        // PB = P B ; d = P c
        for (int q = lane; q < N * M; q += 64) {
            int i = q / M, j = q % M;
            double s = 0.0;
            for (int l = 0; l < N; ++l) s += P[i * N + l] * B[l * M + j];
            PB[q] = s;
        }
        if (lane < N) {
            double s = 0.0;
            for (int l = 0; l < N; ++l) s += P[lane * N + l] * rec[L::oC + l];
            rec[L::oD + lane] = s;
        }
        wave_sync();
        // H = R^ + B'PB
        for (int q = lane; q < M * M; q += 64) {
            int i = q / M, j = q % M;
            double s = 0.5 * a.alpha * (a.R[i * M + j] + a.R[j * M + i]) + (i == j ? hr * muv[i] : 0.0);
            for (int l = 0; l < N; ++l) s += B[l * M + i] * PB[l * M + j];
            Hs[q] = s;
        }
        wave_sync();
        // H^-1 by LDL' in registers (every lane), lane j < M keeps column j
        {
            double Lm[M][M], Dg[M], Dinv[M];
#pragma unroll
            for (int j = 0; j < M; ++j) {
                double dj = Hs[j * M + j];
#pragma unroll
                for (int l = 0; l < j; ++l) dj -= Lm[j][l] * Lm[j][l] * Dg[l];
                if (!(dj > 0.0) && bad == 0) bad = t + 1;
                Dg[j] = dj;
                Dinv[j] = 1.0 / dj;
#pragma unroll
                for (int i = j + 1; i < M; ++i) {
                    double s = Hs[i * M + j];
#pragma unroll
                    for (int l = 0; l < j; ++l) s -= Lm[i][l] * Lm[j][l] * Dg[l];
                    Lm[i][j] = s * Dinv[j];
                }
            }
            if (lane < M) {
                double y[M];
#pragma unroll
                for (int i = 0; i < M; ++i) {
                    double s = (i == lane) ? 1.0 : 0.0;
#pragma unroll
                    for (int l = 0; l < i; ++l) s -= Lm[i][l] * y[l];
                    y[i] = s;
                }
#pragma unroll
                for (int i = M - 1; i >= 0; --i) {
                    double s = y[i] * Dinv[i];
#pragma unroll
                    for (int l = i + 1; l < M; ++l) s -= Lm[l][i] * y[l];
                    y[i] = s;
                }
#pragma unroll
                for (int i = 0; i < M; ++i) rec[L::oHinv + i * M + lane] = y[i];
            }
        }
        wave_sync();
        // Minv = H^-1 B' (M x N)
        for (int q = lane; q < M * N; q += 64) {
            int i = q / N, j = q % N;
            double s = 0.0;
            for (int l = 0; l < M; ++l) s += rec[L::oHinv + i * M + l] * B[j * M + l];
            rec[L::oMinv + q] = s;
        }
        // W = P A
        for (int q = lane; q < N * N; q += 64) {
            int i = q / N, j = q % N;
            double s = 0.0;
            for (int l = 0; l < N; ++l) s += P[i * N + l] * Am[l * N + j];
            Wm[q] = s;
        }
        wave_sync();
        // K = -Minv W  (= -H^-1 B'P A)
        for (int q = lane; q < M * N; q += 64) {
            int i = q / N, j = q % N;
            double s = 0.0;
            for (int l = 0; l < N; ++l) s -= rec[L::oMinv + i * N + l] * Wm[l * N + j];
            rec[L::oK + q] = s;
        }
        wave_sync();
        // Acl = A + B K
        for (int q = lane; q < N * N; q += 64) {
            int i = q / N, j = q % N;
            double s = Am[q];
            for (int l = 0; l < M; ++l) s += B[i * M + l] * rec[L::oK + l * N + j];
            rec[L::oAcl + q] = s;
        }
        wave_sync();
        // P <- Q^ + sym(W' Acl)   (W' Acl = A'P Acl)
        double pn[(N * N + 63) / 64];
#pragma unroll
        for (int r = 0; r < (N * N + 63) / 64; ++r) {
            int q = lane + 64 * r;
            pn[r] = 0.0;
            if (q < N * N) {
                int i = q / N, j = q % N;
                double s = 0.0, s2 = 0.0;
                for (int l = 0; l < N; ++l) {
                    s += Wm[l * N + i] * rec[L::oAcl + l * N + j];
                    s2 += Wm[l * N + j] * rec[L::oAcl + l * N + i];
                }
                pn[r] = qs(a.Q, i, j) + (i == j ? hr * mxv[i] : 0.0) + 0.5 * (s + s2);
            }
        }
        wave_sync();
#pragma unroll
        for (int r = 0; r < (N * N + 63) / 64; ++r) {
            int q = lane + 64 * r;
            if (q < N * N) P[q] = pn[r];
        }
        if constexpr (HBM) {                             // the finished record, once, to the workspace
            const v2d* src = reinterpret_cast<const v2d*>(rec);
            gv2d* dst = (gv2d*)(recs + (size_t)t * L::SP);
            for (int c = lane; c < L::SP / 2; c += 64) dst[c] = src[c];
        }
        wave_sync();
    }
    if constexpr (HBM) {                                 // the sweeps read them back: the stores are done first
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
    }
