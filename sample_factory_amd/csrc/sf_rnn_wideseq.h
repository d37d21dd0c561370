// Persistent sequence passes at H = 1024 (included by sf_rnn.hip, inside its anonymous namespace).
//
// The 16-unit W_hh slice of k_lstm_seq_fwd is 64 x 1028 floats = 263 KB at this width: more than LDS.  Here a
// work-group owns 8 hidden units, so both slices fit (forward 32 gate columns x 1028 floats = 131.6 KB, backward
// 8 rows x 4100 floats = 131.2 KB), and 128 work-groups form a row group (2 groups on 256 CUs, 512 rows per launch).
// Everything else is the scheme of sf_rnn.hip: W_hh resident in LDS for all R steps, exact-f32 MFMAs
// (v_mfma_f32_16x16x4_f32) in one k-order per output element (the start block depends on the hidden unit only), state and
// carries in registers, h_t / gate gradients handed to the other work-groups of the row group through L2 with
// seq_arrive / seq_wait.  KIND 0 = GRU (torch gate order r, z, n), 1 = LSTM (i, f, g, o); the cell arithmetic is
// sf_rnn_cell.h, i.e. that of the per-step kernels.
//
// Forward accumulator layout.  A 16-column MFMA tile holds two gates of the 8 units: tile 0 = [gate 0 | gate 1],
// tile 1 = [gate 2 | gate 3] (GRU: [n | zero columns]).  After the k-loop lane (c, g) holds, for rows 4g .. 4g+3, gates
// hi and 2 + hi of unit c & 7 (hi = c >> 3).  Lanes c and c ^ 8 swap four values, after which a lane has all four gates of
// unit c & 7 for the two rows 4g + 2 hi + {0, 1} and runs the cell for them.
// Backward: the output tile of phase B is 16 rows x 8 units; lanes c and c ^ 8 read the same W_hh row, so both hold the
// unit's four rows and each keeps its two — no exchange.
constexpr int WIDE_H = 1024, WIDE_JB = 8, WIDE_NCOL = WIDE_H / WIDE_JB;

struct WideSeqFwd {
    const float *gx, *whh, *bhh, *keep;
    float *gates, *hprev, *hout, *cprev, *cout;
    unsigned *sync;
    int R, Cn, ngroups, rows_per_group, row0, row_end;  // rows [row0, row_end) of the Cn-row buffers
    int64_t ho_rs, ho_ts;
};

template <int KIND, int NSUB>
__global__ __launch_bounds__(256, 1) void k_wideseq_fwd(WideSeqFwd p) {
    constexpr int H = WIDE_H, JB = WIDE_JB, NG = KIND ? 4 : 3, GH = NG * H, G4 = 4 * H, NC = 4 * JB, NT = 2, LDW = H + 4;
    constexpr int KU = 8, NKB = H / 16 / KU;
    constexpr int NBUF = SF_SEQ_NBUF;
    constexpr int STG = 16 * JB;
    static_assert(NKB * KU * 16 == H && NKB >= NBUF, "shape");
    __shared__ __attribute__((aligned(16))) float lds[NC * LDW + 4 * STG + 4];
    float *wt = lds, *flag = lds + NC * LDW + 4 * STG;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
    const int hi = c >> 3, u = c & 7, lr0 = 4 * g + 2 * hi;  // this lane's cell elements: rows lr0, lr0 + 1 of unit u
    float *stg = lds + NC * LDW + wave * STG;
    const int group = blockIdx.x % p.ngroups, j0 = (blockIdx.x / p.ngroups) * JB, j = j0 + u;
    const unsigned ncol = WIDE_NCOL;
    const int Cn = p.Cn, R = p.R;
    const int rot = (int)(blockIdx.x / p.ngroups) % NKB;
    unsigned *counter = p.sync + group * SEQ_SYNC_STRIDE, *abort_flag = p.sync + SEQ_ABORT_SLOT;
    // ---- W_hh slice, transposed into LDS: wt[q*JB + u][k] = whh[k][q*H + j0 + u] (GRU: the columns of q = 3 are zero)
    for (int idx = tid; idx < NC * H; idx += 256) {
        const int lc = idx % NC, k = idx / NC, q = lc / JB, uu = lc % JB;
        wt[lc * LDW + k] = q < NG ? p.whh[(int64_t)k * GH + q * H + j0 + uu] : 0.0f;
    }
    float bias[NG];
#pragma unroll
    for (int q = 0; q < NG; ++q) bias[q] = p.bhh[q * H + j];
    __syncthreads();
    const auto h_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)p.hprev, 0, (int)((int64_t)(R + 1) * Cn * H * 4), 0x00020000);
    const int g_row0 = p.row0 + group * p.rows_per_group;
    const int g_rows_end = min(p.row_end, g_row0 + p.rows_per_group);

    // masked state entering the step for this lane's elements (LSTM: c, GRU: h)
    float st[NSUB][2];
#pragma unroll
    for (int sub = 0; sub < NSUB; ++sub)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int row = g_row0 + sub * 64 + wave * 16 + lr0 + e, r = row < g_rows_end ? row : g_rows_end - 1;
            st[sub][e] = (KIND ? p.cprev : p.hprev)[(int64_t)r * H + j];
        }
    float xg[NSUB][2][NG], kp[NSUB][2];
    auto prefetch = [&](int t) {
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub)
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int row = g_row0 + sub * 64 + wave * 16 + lr0 + e, r = row < g_rows_end ? row : g_rows_end - 1;
                const int64_t tr = (int64_t)t * Cn + r;
                kp[sub][e] = p.keep[tr];
#pragma unroll
                for (int q = 0; q < NG; ++q) xg[sub][e][q] = p.gx[tr * GH + q * H + j];
            }
    };
    prefetch(0);

    for (int t = 0; t < R; ++t) {
        if (t > 0 && !seq_wait(counter, ncol * (unsigned)t, abort_flag, flag)) return;
        float sv[NSUB][2][6];  // LSTM: i, f, g, o, h, c; GRU: r, z, n, hn, h
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub) {
            const int row0 = g_row0 + sub * 64 + wave * 16;
            if (row0 >= g_rows_end) continue;  // (wave-uniform)
            // ---- gh = h_{t-1} W_hh: A rows from L2 (sc1 loads of the hand-off payload), B from the resident LDS slice
            f32x4 acc[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
            const int arow = row0 + c;
            const uint32_t abase = arow < g_rows_end ? (uint32_t)((((int64_t)t * Cn + arow) * H + 4 * g) * 4) : OOB;
            i32x4 abuf[NBUF][KU];
            auto load_block = [&](int kb, i32x4 (&dst)[KU]) {
#pragma unroll
                for (int ku = 0; ku < KU; ++ku)
                    dst[ku] = __builtin_amdgcn_raw_buffer_load_b128(h_rsrc, abase + (uint32_t)((kb * KU + ku) * 64), 0, SF_SEQ_LOAD_AUX);
            };
            auto kbe = [&](int kb) { const int k = kb + rot; return k >= NKB ? k - NKB : k; };  // staggered start (k_lstm_seq_fwd)
#pragma unroll
            for (int b = 0; b < NBUF - 1; ++b) load_block(kbe(b), abuf[b]);
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) {
                if (kb + NBUF - 1 < NKB) load_block(kbe(kb + NBUF - 1), abuf[(kb + NBUF - 1) % NBUF]);
                const float *bpk = wt + c * LDW + kbe(kb) * (KU * 16) + 4 * g;
#pragma unroll
                for (int ku = 0; ku < KU; ++ku) {
                    const f32x4 a4 = __builtin_bit_cast(f32x4, abuf[kb % NBUF][ku]);
                    const float *bp = bpk + ku * 16;
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        const f32x4 b4 = *reinterpret_cast<const f32x4 *>(bp + nt * 16 * LDW);
#pragma unroll
                        for (int jj = 0; jj < 4; ++jj)
                            acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[jj], b4[jj], acc[nt], 0, 0, 0);
                    }
                }
            }
            // ---- lanes c and c ^ 8 swap the halves they do not keep; then all four gates of (rows lr0 + e, unit u) are here
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const float own_a = hi ? acc[0][2 + e] : acc[0][e], own_b = hi ? acc[1][2 + e] : acc[1][e];
                const float snd_a = hi ? acc[0][e] : acc[0][2 + e], snd_b = hi ? acc[1][e] : acc[1][2 + e];
                const float rcv_a = __shfl_xor(snd_a, 8), rcv_b = __shfl_xor(snd_b, 8);
                const float gh0 = hi ? rcv_a : own_a, gh1 = hi ? own_a : rcv_a, gh2 = hi ? rcv_b : own_b, gh3 = hi ? own_b : rcv_b;
                float hm;  // the masked state handed to step t + 1
                if constexpr (KIND == 1) {
                    float ig, fg, gg, og, cn, h;
                    sf_lstm_cell_fwd(xg[sub][e][0] + (gh0 + bias[0]), xg[sub][e][1] + (gh1 + bias[1]),
                                     xg[sub][e][2] + (gh2 + bias[2]), xg[sub][e][KIND ? 3 : 0] + (gh3 + bias[KIND ? 3 : 0]),
                                     st[sub][e], ig, fg, gg, og, cn, h);
                    st[sub][e] = cn * kp[sub][e];
                    hm = h * kp[sub][e];
                    sv[sub][e][0] = ig; sv[sub][e][1] = fg; sv[sub][e][2] = gg; sv[sub][e][3] = og; sv[sub][e][4] = h; sv[sub][e][5] = cn;
                } else {
                    float r, z, n, h;
                    const float hn = gh2 + bias[2];
                    sf_gru_cell_fwd(xg[sub][e][0] + (gh0 + bias[0]), xg[sub][e][1] + (gh1 + bias[1]), xg[sub][e][2], hn,
                                    st[sub][e], r, z, n, h);
                    hm = st[sub][e] = h * kp[sub][e];
                    sv[sub][e][0] = r; sv[sub][e][1] = z; sv[sub][e][2] = n; sv[sub][e][3] = hn; sv[sub][e][4] = h;
                }
                stg[(lr0 + e) * JB + u] = hm;
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            // state_t * keep -> hprev[t+1]: 16 rows x 8 floats as 16-byte write-through stores (the hand-off payload)
            {
                const int r = lane >> 1, c4 = lane & 1, row = row0 + r;
                const f32x4 val = *reinterpret_cast<const f32x4 *>(stg + (r & 15) * JB + c4 * 4);
                const uint32_t off = (lane < 32 && row < g_rows_end)
                    ? (uint32_t)((((int64_t)(t + 1) * Cn + row) * H + j0 + c4 * 4) * 4) : OOB;
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4, val), h_rsrc, off, 0, 16);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        if (t + 1 < R) {
            seq_arrive(counter);
            prefetch(t + 1);
        }
        // ---- saves for the backward pass (plain stores: they drain while this work-group waits for the others)
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub)
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int row = g_row0 + sub * 64 + wave * 16 + lr0 + e;
                if (row < g_rows_end) {
                    const int64_t tr = (int64_t)t * Cn + row;
                    float *go = p.gates + tr * G4 + j;
                    go[0] = sv[sub][e][0]; go[H] = sv[sub][e][1]; go[2 * H] = sv[sub][e][2]; go[3 * H] = sv[sub][e][3];
                    p.hout[(int64_t)row * p.ho_rs + (int64_t)t * p.ho_ts + j] = sv[sub][e][4];
                    if constexpr (KIND == 1) {
                        p.cout[tr * H + j] = sv[sub][e][5];
                        p.cprev[(tr + Cn) * H + j] = st[sub][e];
                    }
                }
            }
    }
}

struct WideSeqBwd {
    const float *dout, *gates, *hprev, *cprev, *cout, *keep, *whh;
    float *dgx, *dgh;  // LSTM: dgh == dgx (one gate-gradient array)
    unsigned *sync;
    int R, Cn, ngroups, rows_per_group, row0, row_end;
    int64_t do_rs, do_ts;
};

template <int KIND, int NSUB>
__global__ __launch_bounds__(256, 1) void k_wideseq_bwd(WideSeqBwd p) {
    constexpr int H = WIDE_H, JB = WIDE_JB, NG = KIND ? 4 : 3, GH = NG * H, G4 = 4 * H, NC = NG * JB, LDK = GH + 4;
    constexpr int KU = 8, NKB = GH / 16 / KU;
    constexpr int NBUF = SF_SEQ_NBUF;
    constexpr int STG = 16 * NC, NV = (STG / 4 + 63) / 64;
    static_assert(NKB * KU * 16 == GH && NKB % NBUF == 0, "shape");
    __shared__ __attribute__((aligned(16))) float lds[JB * LDK + 4 * STG + 4];
    float *wk = lds, *flag = lds + JB * LDK + 4 * STG;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
    const int hi = c >> 3, u = c & 7, lr0 = 4 * g + 2 * hi;  // this lane's cell elements: rows lr0, lr0 + 1 of unit u
    float *stg = lds + JB * LDK + wave * STG;
    const int group = blockIdx.x % p.ngroups, j0 = (blockIdx.x / p.ngroups) * JB, j = j0 + u;
    const unsigned ncol = WIDE_NCOL;
    const int Cn = p.Cn, R = p.R;
    const int rot = (int)(blockIdx.x / p.ngroups) % NKB;
    unsigned *counter = p.sync + group * SEQ_SYNC_STRIDE, *abort_flag = p.sync + SEQ_ABORT_SLOT;
    // ---- W_hh rows j0 .. j0+7 (all gate columns of this work-group's hidden units): wk[kk][n] = whh[j0 + kk][n]
    for (int idx = tid; idx < JB * (GH / 4); idx += 256) {
        const int kk = idx / (GH / 4), n4 = idx % (GH / 4);
        *reinterpret_cast<f32x4 *>(wk + kk * LDK + n4 * 4) = *reinterpret_cast<const f32x4 *>(p.whh + (int64_t)(j0 + kk) * GH + n4 * 4);
    }
    __syncthreads();
    const auto d_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)p.dgh, 0, (int)((int64_t)R * Cn * GH * 4), 0x00020000);
    const int g_row0 = p.row0 + group * p.rows_per_group;
    const int g_rows_end = min(p.row_end, g_row0 + p.rows_per_group);

    float car_h[NSUB][2], car_c[NSUB][2];
#pragma unroll
    for (int sub = 0; sub < NSUB; ++sub)
#pragma unroll
        for (int e = 0; e < 2; ++e) car_h[sub][e] = car_c[sub][e] = 0.0f;
    // operands of the cell backward of the NEXT step: issued right after this step's hand-off
    float pg[NSUB][2][4], pdo[NSUB][2], pa[NSUB][2], pb[NSUB][2], pkp[NSUB][2];  // pa: cout (LSTM) / hprev (GRU); pb: cprev
    auto prefetch = [&](int t) {
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub)
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int row = g_row0 + sub * 64 + wave * 16 + lr0 + e, r = row < g_rows_end ? row : g_rows_end - 1;
                const int64_t tr = (int64_t)t * Cn + r;
                pkp[sub][e] = t > 0 ? p.keep[tr - Cn] : 0.0f;
                const float *go = p.gates + tr * G4 + j;
                pg[sub][e][0] = go[0]; pg[sub][e][1] = go[H]; pg[sub][e][2] = go[2 * H]; pg[sub][e][3] = go[3 * H];
                pdo[sub][e] = p.dout[(int64_t)r * p.do_rs + (int64_t)t * p.do_ts + j];
                if constexpr (KIND == 1) {
                    pa[sub][e] = p.cout[tr * H + j];
                    pb[sub][e] = p.cprev[tr * H + j];
                } else {
                    pa[sub][e] = p.hprev[tr * H + j];
                    pb[sub][e] = 0.0f;
                }
            }
    };
    prefetch(R - 1);

    for (int s = 0; s < R; ++s) {
        const int t = R - 1 - s;
        float dir[NSUB][2];  // GRU: dL/dh_prev that does not go through W_hh (dh * z)
        // ---- phase A: cell backward of this lane's elements; the gate gradients of step t are the hand-off payload
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub) {
            const int row0 = g_row0 + sub * 64 + wave * 16;
            if (row0 >= g_rows_end) continue;  // (wave-uniform)
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                float d = pdo[sub][e];
                if (s > 0) d = d + car_h[sub][e];
                float *sp = stg + (lr0 + e) * NC + u;
                if constexpr (KIND == 1) {
                    float di, df, dg, dob, dcp;
                    sf_lstm_cell_bwd(d, s > 0 ? car_c[sub][e] : 0.0f, pg[sub][e][0], pg[sub][e][1], pg[sub][e][2], pg[sub][e][3],
                                     pa[sub][e], pb[sub][e], di, df, dg, dob, dcp);
                    sp[0] = di; sp[JB] = df; sp[2 * JB] = dg; sp[(KIND ? 3 : 0) * JB] = dob;
                    car_c[sub][e] = dcp * pkp[sub][e];
                    dir[sub][e] = 0.0f;
                } else {
                    float dr, dz, dn, dnr, dhd;
                    sf_gru_cell_bwd(d, pg[sub][e][0], pg[sub][e][1], pg[sub][e][2], pg[sub][e][3], pa[sub][e], dr, dz, dn, dnr, dhd);
                    sp[0] = dr; sp[JB] = dz; sp[2 * JB] = dnr;
                    dir[sub][e] = dhd;
                    const int row = row0 + lr0 + e;
                    if (row < g_rows_end) {
                        float *x = p.dgx + ((int64_t)t * Cn + row) * GH + j;
                        x[0] = dr; x[H] = dz; x[2 * H] = dn;
                    }
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int v = 0; v < NV; ++v) {  // 16 rows x NC floats as 16-byte write-through stores
                const int f = v * 64 + lane, fr = f < STG / 4 ? f : 0, r = fr / (NC / 4), c4 = fr % (NC / 4), row = row0 + r;
                const int q = c4 >> 1, u4 = (c4 & 1) * 4;
                const f32x4 val = *reinterpret_cast<const f32x4 *>(stg + r * NC + c4 * 4);
                const uint32_t off = (f < STG / 4 && row < g_rows_end)
                    ? (uint32_t)((((int64_t)t * Cn + row) * GH + q * H + j0 + u4) * 4) : OOB;
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4, val), d_rsrc, off, 0, 16);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        if (t == 0) break;  // no state in front of step 0
        seq_arrive(counter);
        float kcur[NSUB][2];
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub)
#pragma unroll
            for (int e = 0; e < 2; ++e) kcur[sub][e] = pkp[sub][e];  // keep[t-1] of THIS step (prefetch overwrites pkp)
        prefetch(t - 1);
        if (!seq_wait(counter, ncol * (unsigned)(s + 1), abort_flag, flag)) return;
        // ---- phase B: dL/dh_{t-1}[rows, own units] = (gate gradients_t[rows, :] W_hh[own units, :]^T (+ dh * z)) * keep[t-1]
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub) {
            const int row0 = g_row0 + sub * 64 + wave * 16;
            if (row0 >= g_rows_end) continue;
            f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
            const int arow = row0 + c;
            const uint32_t abase = arow < g_rows_end ? (uint32_t)((((int64_t)t * Cn + arow) * GH + 4 * g) * 4) : OOB;
            i32x4 abuf[NBUF][KU];
            auto load_block = [&](int kb, i32x4 (&dst)[KU]) {
#pragma unroll
                for (int ku = 0; ku < KU; ++ku)
                    dst[ku] = __builtin_amdgcn_raw_buffer_load_b128(d_rsrc, abase + (uint32_t)((kb * KU + ku) * 64), 0, SF_SEQ_LOAD_AUX);
            };
            auto mma_block = [&](int kb, const i32x4 (&src)[KU]) {
                const float *bp = wk + u * LDK + kb * (KU * 16) + 4 * g;  // (lanes c and c ^ 8: the same unit's row)
#pragma unroll
                for (int ku = 0; ku < KU; ++ku) {
                    const f32x4 a4 = __builtin_bit_cast(f32x4, src[ku]);
                    const f32x4 b4 = *reinterpret_cast<const f32x4 *>(bp + ku * 16);
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[jj], b4[jj], acc, 0, 0, 0);
                }
            };
            auto kbe = [&](int kb) { const int k = kb + rot; return k >= NKB ? k - NKB : k; };
            // block n lives in slot n % NBUF; NBUF - 1 blocks are in flight behind the one in the matrix pipe
#pragma unroll
            for (int b = 0; b < NBUF - 1; ++b) load_block(kbe(b), abuf[b]);
            for (int kb = 0; kb < NKB; kb += NBUF) {
#pragma unroll
                for (int b = 0; b < NBUF; ++b) {
                    if (kb + b + NBUF - 1 < NKB) load_block(kbe(kb + b + NBUF - 1), abuf[(b + NBUF - 1) % NBUF]);
                    mma_block(kbe(kb + b), abuf[b]);
                }
            }
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const float a = hi ? acc[2 + e] : acc[e];
                car_h[sub][e] = (KIND ? a : a + dir[sub][e]) * kcur[sub][e];
            }
        }
    }
}

// row groups of one launch: 128 work-groups each, at most 8 (the counters in front of the abort word)
int wide_groups_max() { return row_groups_max(WIDE_NCOL, 8); }
// the plan of ONE launch over n rows (seq_plan's rule with 128 work-groups per group)
RowGroupPlan wide_plan(int n) { return row_group_plan(n, WIDE_NCOL, 8, 16, 64 * SEQ_MAX_SUB); }
