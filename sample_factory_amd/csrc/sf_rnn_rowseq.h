// Row-owned sequence passes for narrow recurrent cores, H in {32, 64, 128} (included by sf_rnn.hip, inside its anonymous
// namespace).
//
// The persistent passes of sf_rnn.hip split the HIDDEN UNITS of a 256 / 512 wide core across work-groups, because one
// W_hh slice is all a work-group's LDS holds; the work-groups then hand h_t to each other through L2 every step.  At
// these widths the whole W_hh fits one work-group (GRU-64: 48 KB, LSTM-64: 64 KB), so the split goes the other way: a
// work-group owns a tile of CHUNK ROWS and walks all R steps of them alone.  No counters, no polling, no abort word,
// no limit on Cn, and every loop has a trip count known at launch.
//
//   * 256 threads = 4 waves, arranged WR row tiles (16 rows each) x WC unit groups; a wave multiplies its 16 rows by
//     the gate columns of its NU 16-unit tiles (all G gates of them), so that the MFMA accumulator layout hands every
//     lane all gates of its (row, unit) elements: the cell runs in registers, as in the persistent passes.
//     H = 64, 128: WC = 4, tile = 16 rows (a 2048-chunk minibatch is 128 work-groups); H = 32: WC = 2, tile = 32 rows.
//   * W_hh [H][G*H] is copied to LDS once (H <= 64) and read as it lies by the forward pass (B = W_hh) and with
//     transposed fragment indexing by the backward pass (B = W_hh^T); the row pitch (20 mod 64 floats) keeps both
//     fragment shapes clear of systematic bank conflicts.  At H = 128 (192 / 256 KB) the fragments stream from L2.
//   * h_t (forward) / the gate gradients (backward) go from the accumulator layout to the A-fragment layout of the
//     next product through a double-buffered LDS tile: one block barrier per step.  h, c and the dL/dh, dL/dc carries
//     stay in registers; hprev / cprev are written for the weight gradient and the backward pass and never read back.
//   * the operands of step t+1 (gx, keep; backward: dout, gates, states of step t-1) are requested before the products
//     of step t are issued.
//   * ONE accumulation order: v_mfma_f32_16x16x4_f32 over k ascending in steps of 4, whatever Cn: a row's results do
//     not depend on the tile or lane it lands in, nor on its neighbours.  Rows past Cn compute on a copy of the last
//     row and store nothing.
// The cell expressions are those of k_rnn_cell_fwd / k_rnn_cell_bwd (sf_rnn_cell.h).

struct RowSeqFwd {
    const float *gx, *whh, *bhh, *keep;
    float *gates, *hprev, *hout, *cprev, *cout;
    int R, Cn;
    int64_t ho_rs, ho_ts;  // hout element (row, t) lives at row*ho_rs + t*ho_ts (+ unit)
};
struct RowSeqBwd {
    const float *dout, *gates, *hprev, *cprev, *cout, *keep, *whh;
    float *dgx, *dgh;
    int R, Cn;
    int64_t do_rs, do_ts;
};

template <int KIND, int H>
struct RowSeqCfg {
    static constexpr int G = KIND ? 4 : 3, GH = G * H;
    static constexpr int WC = H / 16 < 4 ? H / 16 : 4;  // waves across the unit tiles
    static constexpr int WR = 4 / WC;                    // 16-row tiles per work-group
    static constexpr int ROWS = 16 * WR;
    static constexpr int NU = H / 16 / WC;               // 16-unit tiles per wave
    static constexpr bool WLDS = H <= 64;                // W_hh resident in LDS
    static constexpr int LDW = GH + (84 - GH % 64) % 64;  // = 20 mod 64 floats
    static constexpr int LDH = H + 4, LDG = GH + 4;
    static constexpr int WFLOATS = WLDS ? H * LDW : 0;
};

template <int KIND, int H>
__device__ __forceinline__ void rowseq_load_w(float *wl, const float *whh, int tid) {
    using C = RowSeqCfg<KIND, H>;
    if constexpr (C::WLDS) {
        for (int idx = tid; idx < H * (C::GH / 4); idx += 256) {
            const int k = idx / (C::GH / 4), c4 = idx % (C::GH / 4);
            *reinterpret_cast<f32x4 *>(wl + k * C::LDW + 4 * c4) = *reinterpret_cast<const f32x4 *>(whh + (int64_t)k * C::GH + 4 * c4);
        }
    }
}

template <int KIND, int H>
__global__ __launch_bounds__(256) void k_rowseq_fwd(RowSeqFwd p) {
    using C = RowSeqCfg<KIND, H>;
    constexpr int G = C::G, GH = C::GH, NU = C::NU, NT = G * NU, LDW = C::LDW, LDH = C::LDH, ROWS = C::ROWS;
    __shared__ __attribute__((aligned(16))) float lds[C::WFLOATS + 2 * ROWS * LDH];
    float *wl = lds, *hs = lds + C::WFLOATS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
    const int wr = wave / C::WC, wc = wave % C::WC;
    const int Cn = p.Cn, R = p.R;
    const int row0 = (int)blockIdx.x * ROWS;
    rowseq_load_w<KIND, H>(wl, p.whh, tid);
    for (int idx = tid; idx < ROWS * H; idx += 256) {  // chunk-start h rows -> A staging of step 0
        const int r = idx / H, k = idx % H;
        hs[r * LDH + k] = p.hprev[(int64_t)min(row0 + r, Cn - 1) * H + k];
    }
    // this lane's elements: rows row0 + 16*wr + 4*g + i, units 16*(wc*NU + u) + c
    int rowi[4];
    int64_t rc[4];
    float hp[4][NU], cs[4][NU], bias[G][NU];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        rowi[i] = row0 + 16 * wr + 4 * g + i;
        rc[i] = min(rowi[i], Cn - 1);
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int j = 16 * (wc * NU + u) + c;
            hp[i][u] = p.hprev[rc[i] * H + j];
            cs[i][u] = KIND ? p.cprev[rc[i] * H + j] : 0.0f;
        }
    }
#pragma unroll
    for (int q = 0; q < G; ++q)
#pragma unroll
        for (int u = 0; u < NU; ++u) bias[q][u] = p.bhh[q * H + 16 * (wc * NU + u) + c];
    float xg[4][G][NU], kp[4], xg_n[4][G][NU], kp_n[4];
    auto prefetch = [&](int t, float (&x)[4][G][NU], float (&k)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t tr = (int64_t)t * Cn + rc[i];
            k[i] = p.keep[tr];
#pragma unroll
            for (int q = 0; q < G; ++q)
#pragma unroll
                for (int u = 0; u < NU; ++u) x[i][q][u] = p.gx[tr * GH + q * H + 16 * (wc * NU + u) + c];
        }
    };
    prefetch(0, xg, kp);
    __syncthreads();

    for (int t = 0; t < R; ++t) {
        prefetch(t + 1 < R ? t + 1 : t, xg_n, kp_n);  // lands while the products of this step run
        // ---- gh = h_{t-1} W_hh: A from the staging tile (lane (c, g): row c, k = 4*kk + g), B = W_hh[k][gate column]
        f32x4 acc[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        const float *ap = hs + (t & 1) * ROWS * LDH + (16 * wr + c) * LDH + g;
#pragma unroll
        for (int kk = 0; kk < H / 4; ++kk) {
            const float a = ap[4 * kk];
#pragma unroll
            for (int q = 0; q < G; ++q)
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    const int col = q * H + 16 * (wc * NU + u) + c;
                    const float b = C::WLDS ? wl[(4 * kk + g) * LDW + col] : p.whh[(4 * kk + g) * GH + col];
                    acc[q * NU + u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc[q * NU + u], 0, 0, 0);
                }
        }
        // ---- cell; masked state -> registers, the other staging tile and hprev / cprev [t+1]
        float *hn_s = hs + ((t + 1) & 1) * ROWS * LDH;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool live = rowi[i] < Cn;
            const int64_t tr = (int64_t)t * Cn + rc[i];
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int j = 16 * (wc * NU + u) + c;
                float gate[4], h;
                if constexpr (KIND == 0) {
                    gate[3] = acc[2 * NU + u][i] + bias[2][u];
                    sf_gru_cell_fwd(xg[i][0][u] + (acc[0 * NU + u][i] + bias[0][u]), xg[i][1][u] + (acc[1 * NU + u][i] + bias[1][u]),
                                    xg[i][2][u], gate[3], hp[i][u], gate[0], gate[1], gate[2], h);
                } else {
                    float cn;
                    sf_lstm_cell_fwd(xg[i][0][u] + (acc[0 * NU + u][i] + bias[0][u]), xg[i][1][u] + (acc[1 * NU + u][i] + bias[1][u]),
                                     xg[i][2][u] + (acc[2 * NU + u][i] + bias[2][u]), xg[i][3][u] + (acc[3 * NU + u][i] + bias[3][u]),
                                     cs[i][u], gate[0], gate[1], gate[2], gate[3], cn, h);
                    cs[i][u] = cn * kp[i];
                    if (live) {
                        p.cout[tr * H + j] = cn;
                        p.cprev[(tr + Cn) * H + j] = cs[i][u];
                    }
                }
                hp[i][u] = h * kp[i];
                hn_s[(16 * wr + 4 * g + i) * LDH + j] = hp[i][u];
                if (live) {
                    float *go = p.gates + tr * 4 * H + j;
                    go[0] = gate[0]; go[H] = gate[1]; go[2 * H] = gate[2]; go[3 * H] = gate[3];
                    p.hout[rc[i] * p.ho_rs + (int64_t)t * p.ho_ts + j] = h;
                    p.hprev[(tr + Cn) * H + j] = hp[i][u];
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            kp[i] = kp_n[i];
#pragma unroll
            for (int q = 0; q < G; ++q)
#pragma unroll
                for (int u = 0; u < NU; ++u) xg[i][q][u] = xg_n[i][q][u];
        }
        __syncthreads();  // h_t visible to every wave of the tile; the tile read in this step is free for step t+1's h
    }
}

template <int KIND, int H>
__global__ __launch_bounds__(256) void k_rowseq_bwd(RowSeqBwd p) {
    using C = RowSeqCfg<KIND, H>;
    constexpr int G = C::G, GH = C::GH, NU = C::NU, LDW = C::LDW, LDG = C::LDG, ROWS = C::ROWS;
    __shared__ __attribute__((aligned(16))) float lds[C::WFLOATS + 2 * ROWS * LDG];
    float *wl = lds, *dgs = lds + C::WFLOATS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
    const int wr = wave / C::WC, wc = wave % C::WC;
    const int Cn = p.Cn, R = p.R;
    const int row0 = (int)blockIdx.x * ROWS;
    rowseq_load_w<KIND, H>(wl, p.whh, tid);
    int rowi[4];
    int64_t rc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        rowi[i] = row0 + 16 * wr + 4 * g + i;
        rc[i] = min(rowi[i], Cn - 1);
    }
    // operands of one step's cell backward for this lane's elements: gates, dout, the states, keep of the step before
    struct Ops {
        float gate[4][4][NU], d[4][NU], s0[4][NU], s1[4][NU], km[4];  // s0 = hprev (GRU) / cprev (LSTM), s1 = cout (LSTM)
    };
    Ops cur, nxt;
    auto prefetch = [&](int t, Ops &o) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t tr = (int64_t)t * Cn + rc[i];
            o.km[i] = p.keep[t > 0 ? tr - Cn : tr];
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int j = 16 * (wc * NU + u) + c;
#pragma unroll
                for (int q = 0; q < 4; ++q) o.gate[i][q][u] = p.gates[tr * 4 * H + q * H + j];
                o.d[i][u] = p.dout[rc[i] * p.do_rs + (int64_t)t * p.do_ts + j];
                if constexpr (KIND == 0) {
                    o.s0[i][u] = p.hprev[tr * H + j];
                    o.s1[i][u] = 0.0f;
                } else {
                    o.s0[i][u] = p.cprev[tr * H + j];
                    o.s1[i][u] = p.cout[tr * H + j];
                }
            }
        }
    };
    float carry_h[4][NU], carry_c[4][NU];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int u = 0; u < NU; ++u) carry_h[i][u] = carry_c[i][u] = 0.0f;
    prefetch(R - 1, cur);
    __syncthreads();

    for (int t = R - 1; t >= 0; --t) {
        prefetch(t > 0 ? t - 1 : 0, nxt);
        // ---- cell backward; gate gradients -> dgx / dgh [t] and the A staging tile of the product below
        float *dg_s = dgs + (t & 1) * ROWS * LDG;
        float direct[4][NU];  // the part of dL/dh_prev (GRU) / dL/dc_prev (LSTM) that does not go through W_hh
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool live = rowi[i] < Cn;
            const int64_t tr = (int64_t)t * Cn + rc[i];
            float *sr = dg_s + (16 * wr + 4 * g + i) * LDG;
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int j = 16 * (wc * NU + u) + c;
                const float d = cur.d[i][u] + carry_h[i][u];
                if constexpr (KIND == 0) {
                    float dr, dz, dn, dnr;
                    sf_gru_cell_bwd(d, cur.gate[i][0][u], cur.gate[i][1][u], cur.gate[i][2][u], cur.gate[i][3][u], cur.s0[i][u], dr, dz,
                                    dn, dnr, direct[i][u]);
                    sr[j] = dr; sr[H + j] = dz; sr[2 * H + j] = dnr;
                    if (live) {
                        float *x = p.dgx + tr * GH + j, *gg = p.dgh + tr * GH + j;
                        x[0] = dr; x[H] = dz; x[2 * H] = dn;
                        gg[0] = dr; gg[H] = dz; gg[2 * H] = dnr;
                    }
                } else {
                    float di, df, dg, dob;
                    sf_lstm_cell_bwd(d, carry_c[i][u], cur.gate[i][0][u], cur.gate[i][1][u], cur.gate[i][2][u], cur.gate[i][3][u],
                                     cur.s1[i][u], cur.s0[i][u], di, df, dg, dob, direct[i][u]);
                    sr[j] = di; sr[H + j] = df; sr[2 * H + j] = dg; sr[3 * H + j] = dob;
                    if (live) {
                        float *x = p.dgx + tr * GH + j;
                        x[0] = di; x[H] = df; x[2 * H] = dg; x[3 * H] = dob;
                    }
                }
            }
        }
        if (t == 0) break;  // (uniform) no state in front of the first step
        __syncthreads();  // the gate gradients of the whole tile are staged; the other tile is free for step t-1
        // ---- dL/dh_{t-1} through W_hh: A = dgh_t (lane (c, g): row c, k = 16*kb + 4*g + j), B = W_hh^T[k][unit]
        f32x4 acc[NU];
#pragma unroll
        for (int u = 0; u < NU; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        const float *ap = dg_s + (16 * wr + c) * LDG + 4 * g;
#pragma unroll
        for (int kb = 0; kb < GH / 16; ++kb) {
            const f32x4 a4 = *reinterpret_cast<const f32x4 *>(ap + 16 * kb);
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                const int n = 16 * (wc * NU + u) + c;
                const f32x4 b4 = C::WLDS ? *reinterpret_cast<const f32x4 *>(wl + n * LDW + 16 * kb + 4 * g)
                                         : *reinterpret_cast<const f32x4 *>(p.whh + n * GH + 16 * kb + 4 * g);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[j], b4[j], acc[u], 0, 0, 0);
            }
        }
        // ---- carries into step t-1, masked by keep[t-1] (the state was zeroed after a done / invalid step)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int u = 0; u < NU; ++u) {
                if constexpr (KIND == 0) {
                    carry_h[i][u] = (acc[u][i] + direct[i][u]) * cur.km[i];
                } else {
                    // (+ 0.0f: what sf_rows_add_scale computes with no second operand — the per-step path's carry; it only
                    // turns a -0 into +0, and keeps the two paths' bits equal there too)
                    carry_h[i][u] = (acc[u][i] + 0.0f) * cur.km[i];
                    carry_c[i][u] = (direct[i][u] + 0.0f) * cur.km[i];
                }
            }
        cur = nxt;
    }
}

// every width is one tile height, so the plan is the template's own constants
inline int rowseq_width_ok(int H) { return H == 32 || H == 64 || H == 128; }
