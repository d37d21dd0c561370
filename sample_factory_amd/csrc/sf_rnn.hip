// libsf_hip.so — persistent LSTM sequence kernels for gfx950 (one launch per BPTT pass instead of ~6 launches per step).
//
// Reference path: model/core.py:19-64 (nn.LSTM over a PackedSequence) + algo/learning/rnn_utils.py:114-158; here the
// masked time loop over recurrence-length chunks (state zeroed after done/invalid steps), the loop form the reference's
// tests/algo/test_rnn.py proves equal to its packed path.
//
// The per-step recurrent GEMM of config 5 (512 chunk rows x 512 hidden x 2048 gate columns, 1.07 GFLOP) is too small
// to fill the chip as a launch of its own: measured 31 us forward / 65 us backward per step at 15-27 TFLOP/s, plus the
// cell and carry kernels (profiles/r02_c5_a_kernel_stats.csv).  Instead ONE launch walks all R steps:
//   * a work-group owns JB hidden units (= 4*JB gate columns; JB = 16 for H = 512) of one ROW GROUP of chunks and keeps
//     its slice of W_hh RESIDENT IN LDS for the whole pass (64 x 516 floats = 129 KB forward, 16 x 2052 backward);
//   * per step only the h (forward: 128 KB per group) / gate-gradient (backward: 512 KB) rows come from L2; the
//     products run on v_mfma_f32_16x16x4_f32 (exact f32), one ds_read_b128 + one 16-byte global load per 4 MFMAs;
//   * the cell non-linearity, the done/invalid masking, the carries of dL/dh and dL/dc and all saves for the backward
//     pass are fused into the epilogue (the MFMA accumulator layout hands every lane all four gates of its (row, unit));
//   * the work-groups of a row group (H/JB of them; block b -> group b % ngroups, i.e. one XCD per group under the
//     observed round-robin dispatch — a speed bonus only) exchange h_t / dgates_t through L2 with the placement-
//     independent write-through protocol of MI355X_MICROARCH.md (16-byte sc1 stores -> s_waitcnt vmcnt(0) -> barrier ->
//     relaxed agent-scope counter; consumer: relaxed poll -> sc1 loads), one hand-off per step, no grid-wide barrier.
// Work-groups spin on the counter, so all of them must be co-resident: the grid is ngroups * H/JB <= #CUs with one
// work-group per CU (LDS-limited).  A bounded spin turns a lost work-group (GPU shared with another process) into an
// error flag instead of a hang.
#include <limits.h>
#include <stdlib.h>
#include <algorithm>
#include <initializer_list>
#include <type_traits>

#include "sf_common.h"
#include "sf_rnn_cell.h"

#define STREAM(s) reinterpret_cast<hipStream_t>(s)

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((__vector_size__(16)));

namespace {

constexpr int SEQ_SYNC_STRIDE = 16;       // one counter per 64-byte line
constexpr int SEQ_ABORT_SLOT = 8 * SEQ_SYNC_STRIDE;
constexpr uint32_t SEQ_SPIN_LIMIT = 1u << 22;
constexpr int SEQ_MAX_SUB = 4;             // 64-row sub-tiles per work-group (register-resident state): Cn <= ngroups * 256
#ifndef SF_SEQ_NBUF
#define SF_SEQ_NBUF 2
#endif
#ifndef SF_SEQ_LOAD_AUX
#define SF_SEQ_LOAD_AUX 16  // cache policy of the hand-off payload loads: 16 = sc1 (served by L2), 0 = through the CU's L1
#endif
constexpr uint32_t OOB = 0x7FFFFFF0u;     // byte offset past every buffer: loads return 0, stores are dropped

// Cell transcendentals of the fused sequence passes.  SF_FAST_CELL = 1 (NOT the default; -DSF_FAST_CELL=1 through
// tools/build_variant.sh): hardware v_exp_f32 / v_rcp_f32 forms — ~4 instructions instead of the ~15 (expf) /
// ~25 (tanhf) of the accurate library code; absolute error <= 2e-7 (the relative error of tanh grows as 6e-8 / |x| near
// 0).  Vector instructions do not overlap with MFMAs on a SIMD, so they are matrix-pipe time: forward
// pass 0.440 -> 0.415 ms, configs[4] step 16.36 -> 16.09 ms over three alternations, the configs[4] LSTM / GRU replays
// against the reference and its float64 loop still within their bounds (profiles/r05_i_fastcell_ab.log) — but the GRU replay's
// distance from the float64 loop doubles (1.2e-4 -> 2.4e-4 of the largest weight delta; the reference's own fp32 run:
// 0.5e-4), and 1.6 % of a secondary line does not buy that: the accurate library forms stay the default.
#ifndef SF_FAST_CELL
#define SF_FAST_CELL 0
#endif
#if SF_FAST_CELL
__device__ __forceinline__ float sigm(float x) { return __frcp_rn(1.0f + __expf(-x)); }
__device__ __forceinline__ float tanh_c(float x) {
    const float t = __expf(-2.0f * fabsf(x));
    return copysignf((1.0f - t) * __frcp_rn(1.0f + t), x);
}
#else
__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float tanh_c(float x) { return tanhf(x); }
#endif

// arrive: every wave has drained its write-through stores, then one relaxed agent-scope increment
__device__ __forceinline__ void seq_arrive(unsigned *counter) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// wait until `counter` >= target; returns false if the pass was aborted (bounded spin)
__device__ __forceinline__ bool seq_wait(unsigned *counter, unsigned target, unsigned *abort_flag, float *lds_flag) {
    if (threadIdx.x == 0) {
        uint32_t spins = 0;
        bool ok = true;
        while (__hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
            __builtin_amdgcn_s_sleep(4);
            if ((++spins & 1023u) == 0 &&
                (spins >= SEQ_SPIN_LIMIT || __hip_atomic_load(abort_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))) {
                __hip_atomic_store(abort_flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                ok = false;
                break;
            }
        }
        *lds_flag = ok ? 1.0f : 0.0f;
    }
    __syncthreads();
    if (SF_SEQ_LOAD_AUX == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // drop the CU's L1 copies of older payload lines
    const bool ok = *lds_flag != 0.0f;
    __syncthreads();  // the flag word may be rewritten by the next wait
    return ok;
}

struct LstmSeqFwd {
    const float *gx, *whh, *bhh, *keep;
    float *gates, *hprev, *hout, *cprev, *cout;
    unsigned *sync;
    int R, Cn, ngroups, rows_per_group;
    int64_t ho_rs, ho_ts;  // hout element (row, t) lives at row*ho_rs + t*ho_ts (+ unit): [R][Cn][H] or [Cn][R][H]
    // KXB > 0 (sf_lstm_seq_fwd_x): gx is not given but computed here, x [R][Cn][16*KXB] (time-major), wih_t [4H][16*KXB]
    // (gate-column-major copy of W_ih), bih [4H]
    const float *x, *wih_t, *bih;
    int row0, row_end;  // this launch covers rows [row0, row_end) of the Cn-row buffers (Cn stays the row pitch)
};

// H hidden units, JB of them per work-group (JB = 16: the W_hh slice is 64 x (H + 4) floats of LDS — 129 KB at H = 512,
// 66.5 KB at H = 256; H = 1024 would need 263 KB: that width runs with JB = 8 and its own accumulator-to-lane mapping,
// k_wideseq_fwd in sf_rnn_wideseq.h).
// KXB > 0: the input projection gx_t = x_t W_ih^T + b_ih (KXB 16-column blocks of x) is computed HERE instead of by a GEMM
// launch that writes [R][Cn][4H] floats for this kernel to read back: the W_ih fragments of the work-group's 64 gate
// columns live in registers, the x fragments of step t+1 are fetched behind step t's hand-off, and the 16*KXB MFMAs run
// while the first h rows of the step are on their way from L2 (placed between the hand-off and the wait they delayed
// every work-group alike: +1.8 us per step, measured).
template <int H, int JB, int NSUB, int KXB>
__global__ __launch_bounds__(256, 1) void k_lstm_seq_fwd(LstmSeqFwd p) {
    constexpr int G4 = 4 * H, NC = 4 * JB, NT = NC / 16, NU = JB / 16, LDW = H + 4, KX = 16 * KXB;
    constexpr int KU = 8, NKB = H / 16 / KU;
    constexpr int NBUF = NKB < SF_SEQ_NBUF ? NKB : SF_SEQ_NBUF;  // k-blocks of 8 x 16-byte loads per lane in flight (+ the one in the matrix pipe)
    constexpr int STG = 16 * JB;  // floats of one wave's staging tile
    static_assert(NKB * KU * 16 == H && NU >= 1, "shape");
    __shared__ __attribute__((aligned(16))) float lds[NC * LDW + 4 * STG + 4];
    float *wt = lds, *flag = lds + NC * LDW + 4 * STG;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
    float *stg = lds + NC * LDW + wave * STG;
    const int group = blockIdx.x % p.ngroups, j0 = (blockIdx.x / p.ngroups) * JB;
    const unsigned ncol = H / JB;
    const int Cn = p.Cn, R = p.R;
    const int rot = (int)(blockIdx.x / p.ngroups) % NKB;
    unsigned *counter = p.sync + group * SEQ_SYNC_STRIDE, *abort_flag = p.sync + SEQ_ABORT_SLOT;
    // ---- W_hh slice, transposed into LDS: wt[q*JB + u][k] = whh[k][q*H + j0 + u]
    for (int idx = tid; idx < NC * H; idx += 256) {
        const int lc = idx % NC, k = idx / NC, q = lc / JB, u = lc % JB;
        wt[lc * LDW + k] = p.whh[(int64_t)k * G4 + q * H + j0 + u];
    }
    float bias[4][NU], bih[4][NU];
    f32x4 bx[KXB > 0 ? KXB : 1][NT];  // lane (c, g): W_ih^T[gate column of tile nt, lane c][16*blk + 4*g ..]
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            bias[q][u] = p.bhh[q * H + j0 + u * 16 + c];
            bih[q][u] = KXB > 0 ? p.bih[q * H + j0 + u * 16 + c] : 0.0f;
            if (KXB > 0) {
#pragma unroll
                for (int blk = 0; blk < KXB; ++blk)
                    bx[blk][q * NU + u] = *reinterpret_cast<const f32x4 *>(p.wih_t + (int64_t)(q * H + j0 + u * 16 + c) * KX + 16 * blk + 4 * g);
            }
        }
    __syncthreads();
    const auto h_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)p.hprev, 0, (int)((int64_t)(R + 1) * Cn * H * 4), 0x00020000);
    const int g_row0 = p.row0 + group * p.rows_per_group;  // [row0, row_end): the slab of rows this launch covers
    const int g_rows_end = min(p.row_end, g_row0 + p.rows_per_group);

    // the cell state of this lane's (row, unit) elements stays in registers across the steps (the masked copy is also
    // stored to cprev[t+1] for the backward pass); sub-tiles are unrolled so that the register arrays index statically
    float cst[NSUB][4][NU];
#pragma unroll
    for (int sub = 0; sub < NSUB; ++sub) {
        const int row0 = g_row0 + sub * 64 + wave * 16;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = row0 + 4 * g + i, r = row < g_rows_end ? row : g_rows_end - 1;
#pragma unroll
            for (int u = 0; u < NU; ++u) cst[sub][i][u] = p.cprev[(int64_t)r * H + j0 + u * 16 + c];
        }
    }

    // operands of the cell epilogue for the next step: issued right after this step's hand-off, so they fly during the
    // wait for the other work-groups and the MFMA phase
    float xg[KXB > 0 ? 1 : NSUB][4][4][NU], kp[NSUB][4];
    f32x4 xa[NSUB][KXB > 0 ? KXB : 1];   // KXB > 0: x fragments of the NEXT projection (lane (c, g): row c, k = 16*blk + 4*g ..)
    f32x4 xacc[NSUB][KXB > 0 ? NT : 1];  // KXB > 0: x_t W_ih^T of the step about to run
    auto prefetch = [&](int t) {
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub) {
            const int row0 = g_row0 + sub * 64 + wave * 16;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = row0 + 4 * g + i, r = row < g_rows_end ? row : g_rows_end - 1;
                const int64_t tr = (int64_t)t * Cn + r;
                kp[sub][i] = p.keep[tr];
                if constexpr (KXB == 0) {
#pragma unroll
                    for (int u = 0; u < NU; ++u)
#pragma unroll
                        for (int q = 0; q < 4; ++q) xg[sub][i][q][u] = p.gx[tr * G4 + q * H + j0 + u * 16 + c];
                }
            }
        }
    };
    auto load_x = [&](int t) {  // fragments of x_t
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub) {
            const int row = g_row0 + sub * 64 + wave * 16 + c, r = row < g_rows_end ? row : g_rows_end - 1;
#pragma unroll
            for (int blk = 0; blk < KXB; ++blk)
                xa[sub][blk] = *reinterpret_cast<const f32x4 *>(p.x + ((int64_t)t * Cn + r) * KX + 16 * blk + 4 * g);
        }
    };
    auto project_x = [&](int sub) {  // xacc = xa W_ih^T (this work-group's gate columns)
#pragma unroll
        for (int nt = 0; nt < (KXB > 0 ? NT : 1); ++nt) xacc[sub][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int blk = 0; blk < KXB; ++blk)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    xacc[sub][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[sub][blk][j], bx[blk][nt][j], xacc[sub][nt], 0, 0, 0);
    };
    prefetch(0);
    if (KXB > 0) load_x(0);

    for (int t = 0; t < R; ++t) {
        if (t > 0 && !seq_wait(counter, ncol * (unsigned)t, abort_flag, flag)) return;
        float sv[NSUB][4][NU][6];  // i, f, g, o, h, c of this step: stored AFTER the hand-off (nobody waits for them)
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub) {
            const int row0 = g_row0 + sub * 64 + wave * 16;
            if (row0 >= g_rows_end) continue;  // (wave-uniform; no block barrier inside the sub-tile body)
            // ---- gh = h_{t-1} W_hh: A rows from L2 (write-through hand-off: sc1 loads), B from the resident LDS slice
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
            // every work-group of the row group reads the SAME h rows: each starts its reduction at a different k-block
            // so that at any moment they pull different lines (different L2 channels) instead of all the same one
            auto kbe = [&](int kb) { const int k = kb + rot; return k >= NKB ? k - NKB : k; };
#pragma unroll
            for (int b = 0; b < NBUF - 1; ++b) load_block(kbe(b), abuf[b]);
            if constexpr (KXB > 0) {  // x_t W_ih^T while the first h rows are on their way from L2
                __builtin_amdgcn_sched_barrier(0);
                project_x(sub);
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) {
                if (kb + NBUF - 1 < NKB) load_block(kbe(kb + NBUF - 1), abuf[(kb + NBUF - 1) % NBUF]);
                if constexpr (KXB > 0) __builtin_amdgcn_sched_barrier(0);  // (with the projection's registers live hipcc sinks these loads to their use)
                const float *bpk = wt + c * LDW + kbe(kb) * (KU * 16) + 4 * g;
#pragma unroll
                for (int ku = 0; ku < KU; ++ku) {
                    const f32x4 a4 = __builtin_bit_cast(f32x4, abuf[kb % NBUF][ku]);
                    const float *bp = bpk + ku * 16;
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        const f32x4 b4 = *reinterpret_cast<const f32x4 *>(bp + nt * 16 * LDW);
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[j], b4[j], acc[nt], 0, 0, 0);
                    }
                }
            }
            // ---- LSTM cell (k_rnn_cell_fwd's arithmetic); masked state for step t+1 into the staging tile
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    float gxv[4];  // gx of this (row, unit): given, or the projection computed behind the last hand-off
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        gxv[q] = KXB > 0 ? xacc[sub][KXB > 0 ? q * NU + u : 0][i] + bih[q][u] : xg[KXB > 0 ? 0 : sub][i][q][u];
                    const float ig = sigm(gxv[0] + (acc[0 * NU + u][i] + bias[0][u]));
                    const float fg = sigm(gxv[1] + (acc[1 * NU + u][i] + bias[1][u]));
                    const float gg = tanh_c(gxv[2] + (acc[2 * NU + u][i] + bias[2][u]));
                    const float og = sigm(gxv[3] + (acc[3 * NU + u][i] + bias[3][u]));
                    const float cn = fg * cst[sub][i][u] + ig * gg;
                    const float h = og * tanh_c(cn);
                    cst[sub][i][u] = cn * kp[sub][i];
                    stg[(4 * g + i) * JB + u * 16 + c] = h * kp[sub][i];
                    sv[sub][i][u][0] = ig; sv[sub][i][u][1] = fg; sv[sub][i][u][2] = gg; sv[sub][i][u][3] = og;
                    sv[sub][i][u][4] = h; sv[sub][i][u][5] = cn;
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            // h_t * keep -> hprev[t+1]: 16-byte write-through stores (the hand-off payload)
#pragma unroll
            for (int v = 0; v < NU; ++v) {
                const int f = v * 64 + lane, r = f / (JB / 4), c4 = f % (JB / 4), row = row0 + r;
                const f32x4 val = *reinterpret_cast<const f32x4 *>(stg + r * JB + c4 * 4);
                const uint32_t off = row < g_rows_end ? (uint32_t)((((int64_t)(t + 1) * Cn + row) * H + j0 + c4 * 4) * 4) : OOB;
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4, val), h_rsrc, off, 0, 16);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        if (t + 1 < R) {
            seq_arrive(counter);
            prefetch(t + 1);
            if (KXB > 0) load_x(t + 1);  // fragments of the next step's input
        }
        // ---- saves for the backward pass (plain stores: they drain while this work-group waits for the others)
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub) {
            const int row0 = g_row0 + sub * 64 + wave * 16;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = row0 + 4 * g + i;
                if (row < g_rows_end) {
                    const int64_t tr = (int64_t)t * Cn + row;
#pragma unroll
                    for (int u = 0; u < NU; ++u) {
                        const int j = j0 + u * 16 + c;
                        float *go = p.gates + tr * G4 + j;
                        go[0] = sv[sub][i][u][0]; go[H] = sv[sub][i][u][1]; go[2 * H] = sv[sub][i][u][2]; go[3 * H] = sv[sub][i][u][3];
                        p.hout[(int64_t)row * p.ho_rs + (int64_t)t * p.ho_ts + j] = sv[sub][i][u][4];
                        p.cout[tr * H + j] = sv[sub][i][u][5];
                        p.cprev[(tr + Cn) * H + j] = cst[sub][i][u];
                    }
                }
            }
        }
    }
}

struct LstmSeqBwd {
    const float *dout, *gates, *cprev, *cout, *keep, *whh;
    float *dgx;
    unsigned *sync;
    int R, Cn, ngroups, rows_per_group;
    int64_t do_rs, do_ts;  // dout element (row, t) lives at row*do_rs + t*do_ts (+ unit)
    int ablate;  // timing experiments only (SF_LSTM_ABLATE, tools/lstm_bench.py): 1 no hand-off wait, 2 no phase-B loads,
                 // 4 no phase-B MFMAs, 8 no phase A — results are wrong with any bit set
    int row0, row_end;  // (see LstmSeqFwd)
};

template <int H, int JB, int NSUB>
__global__ __launch_bounds__(256, 1) void k_lstm_seq_bwd(LstmSeqBwd p) {
    constexpr int G4 = 4 * H, NC = 4 * JB, NU = JB / 16, LDK = G4 + 4;
    constexpr int KU = 8, NKB = G4 / 16 / KU;
    constexpr int NBUF = SF_SEQ_NBUF;  // k-blocks of 8 x 16-byte loads per lane: NBUF - 1 in flight behind the one in the matrix pipe
    constexpr int STG = 16 * NC;
    static_assert(NKB * KU * 16 == G4 && NKB >= NBUF - 1, "shape");
    __shared__ __attribute__((aligned(16))) float lds[JB * LDK + 4 * STG + 4];
    float *wk = lds, *flag = lds + JB * LDK + 4 * STG;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
    float *stg = lds + JB * LDK + wave * STG;
    const int group = blockIdx.x % p.ngroups, j0 = (blockIdx.x / p.ngroups) * JB;
    const unsigned ncol = H / JB;
    const int Cn = p.Cn, R = p.R;
    const int rot = (int)(blockIdx.x / p.ngroups) % NKB;  // staggered reduction start (see k_lstm_seq_fwd)
    unsigned *counter = p.sync + group * SEQ_SYNC_STRIDE, *abort_flag = p.sync + SEQ_ABORT_SLOT;
    // ---- W_hh rows j0 .. j0+JB-1 (all 4H gate columns of this group's hidden units): wk[kk][n] = whh[j0 + kk][n]
    for (int idx = tid; idx < JB * (G4 / 4); idx += 256) {
        const int kk = idx / (G4 / 4), n4 = idx % (G4 / 4);
        *reinterpret_cast<f32x4 *>(wk + kk * LDK + n4 * 4) =
            *reinterpret_cast<const f32x4 *>(p.whh + (int64_t)(j0 + kk) * G4 + n4 * 4);
    }
    __syncthreads();
    const auto d_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)p.dgx, 0, (int)((int64_t)R * Cn * G4 * 4), 0x00020000);
    const int g_row0 = p.row0 + group * p.rows_per_group;  // [row0, row_end): the slab of rows this launch covers
    const int g_rows_end = min(p.row_end, g_row0 + p.rows_per_group);

    // dL/dh and dL/dc carried from step t+1 to step t for this lane's (row, unit) elements: registers
    float car_h[NSUB][4][NU], car_c[NSUB][4][NU];
#pragma unroll
    for (int sub = 0; sub < NSUB; ++sub)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int u = 0; u < NU; ++u) car_h[sub][i][u] = car_c[sub][i][u] = 0.0f;

    // operands of the cell backward of the NEXT step (t-1): issued right after this step's hand-off, so they fly during
    // the wait and the MFMA phase (only the carry of dL/dh links phase A of step t-1 to phase B of step t)
    float pg[NSUB][4][NU][4], pdo[NSUB][4][NU], pco[NSUB][4][NU], pcp[NSUB][4][NU], pkp[NSUB][4];
    auto prefetch = [&](int t) {
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub) {
            const int row0 = g_row0 + sub * 64 + wave * 16;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = row0 + 4 * g + i, r = row < g_rows_end ? row : g_rows_end - 1;
                const int64_t tr = (int64_t)t * Cn + r;
                pkp[sub][i] = t > 0 ? p.keep[tr - Cn] : 0.0f;
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    const int j = j0 + u * 16 + c;
                    const float *go = p.gates + tr * G4 + j;
                    pg[sub][i][u][0] = go[0]; pg[sub][i][u][1] = go[H]; pg[sub][i][u][2] = go[2 * H]; pg[sub][i][u][3] = go[3 * H];
                    pdo[sub][i][u] = p.dout[(int64_t)r * p.do_rs + (int64_t)t * p.do_ts + j];
                    pco[sub][i][u] = p.cout[tr * H + j];
                    pcp[sub][i][u] = p.cprev[tr * H + j];
                }
            }
        }
    };
    prefetch(R - 1);

    for (int s = 0; s < R; ++s) {
        const int t = R - 1 - s;
        // ---- phase A: cell backward (k_rnn_cell_bwd's arithmetic) for this group's (rows, units); dgates -> dgx[t]
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub) {
            const int row0 = g_row0 + sub * 64 + wave * 16;
            if (row0 >= g_rows_end || (p.ablate & 8)) continue;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float kprev = pkp[sub][i];
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    const float ig = pg[sub][i][u][0], fg = pg[sub][i][u][1], gg = pg[sub][i][u][2], og = pg[sub][i][u][3];
                    float d = pdo[sub][i][u];
                    float dc_in = 0.0f;
                    if (s > 0) {
                        d = d + car_h[sub][i][u];
                        dc_in = car_c[sub][i][u];
                    }
                    const float tc = tanh_c(pco[sub][i][u]);
                    const float dc = d * og * (1.0f - tc * tc) + dc_in;
                    const float di = (dc * gg) * (ig * (1.0f - ig)), df = (dc * pcp[sub][i][u]) * (fg * (1.0f - fg));
                    const float dg = (dc * ig) * (1.0f - gg * gg), dob = (d * tc) * (og * (1.0f - og));
                    float *sp = stg + (4 * g + i) * NC + u * 16 + c;
                    sp[0] = di; sp[JB] = df; sp[2 * JB] = dg; sp[3 * JB] = dob;
                    car_c[sub][i][u] = (dc * fg) * kprev;
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int v = 0; v < STG / 4 / 64; ++v) {  // 16 rows x NC floats as 16-byte write-through stores
                const int f = v * 64 + lane, r = f / (NC / 4), c4 = f % (NC / 4), row = row0 + r;
                const int q = (c4 * 4) / JB, u4 = (c4 * 4) % JB;
                const f32x4 val = *reinterpret_cast<const f32x4 *>(stg + r * NC + c4 * 4);
                const uint32_t off = row < g_rows_end ? (uint32_t)((((int64_t)t * Cn + row) * G4 + q * H + j0 + u4) * 4) : OOB;
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4, val), d_rsrc, off, 0, 16);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        if (t == 0) break;  // no state in front of step 0
        seq_arrive(counter);
        prefetch(t - 1);
        if (!(p.ablate & 1) && !seq_wait(counter, ncol * (unsigned)(s + 1), abort_flag, flag)) return;
        // ---- phase B: dL/dh_{t-1}[rows, own units] = dgates_t[rows, :] W_hh[own units, :]^T, masked by keep[t-1]
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub) {
            const int row0 = g_row0 + sub * 64 + wave * 16;
            if (row0 >= g_rows_end) continue;
            f32x4 acc[NU];
#pragma unroll
            for (int u = 0; u < NU; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            const int arow = row0 + c;
            const uint32_t abase = (arow < g_rows_end && !(p.ablate & 2)) ? (uint32_t)((((int64_t)t * Cn + arow) * G4 + 4 * g) * 4) : OOB;
            i32x4 abuf[NBUF][KU];
            auto load_block = [&](int kb, i32x4 (&dst)[KU]) {
#pragma unroll
                for (int ku = 0; ku < KU; ++ku)
                    dst[ku] = __builtin_amdgcn_raw_buffer_load_b128(d_rsrc, abase + (uint32_t)((kb * KU + ku) * 64), 0, SF_SEQ_LOAD_AUX);
            };
            auto mma_block = [&](int kb, const i32x4 (&src)[KU]) {
                if (p.ablate & 4) return;
#pragma unroll
                for (int ku = 0; ku < KU; ++ku) {
                    const f32x4 a4 = __builtin_bit_cast(f32x4, src[ku]);
                    const float *bp = wk + c * LDK + (kb * KU + ku) * 16 + 4 * g;
#pragma unroll
                    for (int u = 0; u < NU; ++u) {
                        const f32x4 b4 = *reinterpret_cast<const f32x4 *>(bp + u * 16 * LDK);
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[j], b4[j], acc[u], 0, 0, 0);
                    }
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
                    if (kb + b < NKB) mma_block(kbe(kb + b), abuf[b]);
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = row0 + 4 * g + i, r = row < g_rows_end ? row : g_rows_end - 1;
                const float kprev = p.keep[(int64_t)(t - 1) * Cn + r];
#pragma unroll
                for (int u = 0; u < NU; ++u) car_h[sub][i][u] = acc[u][i] * kprev;
            }
        }
    }
}


// ================================================================================================ GRU (torch gate order r, z, n)
// The reference's DEFAULT core (cfg rnn_type = gru, rnn_size = 512).  Same decomposition and hand-off protocol as the
// LSTM passes; a work-group's 16 hidden units are 48 gate columns (r, z, n), the candidate gate needs the recurrent part
// hn = h W_hn + b_hn separately (n = tanh(x_n + r * hn)), so the MFMA result is NOT pre-added to gx, and the backward
// pass has two gate-gradient arrays: dgx (for W_ih and the encoder) and dgh = {dr, dz, dn * r} (for W_hh; it is the
// hand-off payload), plus the direct path dL/dh_prev += dh * z.
struct GruSeqFwd {
    const float *gx, *whh, *bhh, *keep;
    float *gates, *hprev, *hout;
    unsigned *sync;
    int R, Cn, ngroups, rows_per_group;
    int64_t ho_rs, ho_ts;
    const float *x, *wih_t, *bih;  // KXB > 0 (sf_gru_seq_fwd_x): see LstmSeqFwd
    int row0, row_end;
};

template <int H, int JB, int NSUB, int KXB>
__global__ __launch_bounds__(256, 1) void k_gru_seq_fwd(GruSeqFwd p) {
    constexpr int G3 = 3 * H, G4 = 4 * H, NC = 3 * JB, NT = NC / 16, NU = JB / 16, LDW = H + 4, KX = 16 * KXB;
    constexpr int KU = 8, NKB = H / 16 / KU;
    constexpr int NBUF = NKB < SF_SEQ_NBUF ? NKB : SF_SEQ_NBUF;  // k-blocks of 8 x 16-byte loads per lane in flight (+ the one in the matrix pipe)
    constexpr int STG = 16 * JB;
    static_assert(NKB * KU * 16 == H && NU >= 1, "shape");
    __shared__ __attribute__((aligned(16))) float lds[NC * LDW + 4 * STG + 4];
    float *wt = lds, *flag = lds + NC * LDW + 4 * STG;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
    float *stg = lds + NC * LDW + wave * STG;
    const int group = blockIdx.x % p.ngroups, j0 = (blockIdx.x / p.ngroups) * JB;
    const unsigned ncol = H / JB;
    const int Cn = p.Cn, R = p.R;
    const int rot = (int)(blockIdx.x / p.ngroups) % NKB;
    unsigned *counter = p.sync + group * SEQ_SYNC_STRIDE, *abort_flag = p.sync + SEQ_ABORT_SLOT;
    for (int idx = tid; idx < NC * H; idx += 256) {  // wt[q*JB + u][k] = whh[k][q*H + j0 + u]
        const int lc = idx % NC, k = idx / NC, q = lc / JB, u = lc % JB;
        wt[lc * LDW + k] = p.whh[(int64_t)k * G3 + q * H + j0 + u];
    }
    float bias[3][NU], bih[3][NU];
    f32x4 bx[KXB > 0 ? KXB : 1][NT];
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            bias[q][u] = p.bhh[q * H + j0 + u * 16 + c];
            bih[q][u] = KXB > 0 ? p.bih[q * H + j0 + u * 16 + c] : 0.0f;
            if (KXB > 0) {
#pragma unroll
                for (int blk = 0; blk < KXB; ++blk)
                    bx[blk][q * NU + u] = *reinterpret_cast<const f32x4 *>(p.wih_t + (int64_t)(q * H + j0 + u * 16 + c) * KX + 16 * blk + 4 * g);
            }
        }
    __syncthreads();
    const auto h_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)p.hprev, 0, (int)((int64_t)(R + 1) * Cn * H * 4), 0x00020000);
    const int g_row0 = p.row0 + group * p.rows_per_group;  // [row0, row_end): the slab of rows this launch covers
    const int g_rows_end = min(p.row_end, g_row0 + p.rows_per_group);
    float hst[NSUB][4][NU];  // masked state entering the step, for this lane's (row, unit) elements
#pragma unroll
    for (int sub = 0; sub < NSUB; ++sub) {
        const int row0 = g_row0 + sub * 64 + wave * 16;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = row0 + 4 * g + i, r = row < g_rows_end ? row : g_rows_end - 1;
#pragma unroll
            for (int u = 0; u < NU; ++u) hst[sub][i][u] = p.hprev[(int64_t)r * H + j0 + u * 16 + c];
        }
    }
    float xg[KXB > 0 ? 1 : NSUB][4][3][NU], kp[NSUB][4];
    f32x4 xa[NSUB][KXB > 0 ? KXB : 1], xacc[NSUB][KXB > 0 ? NT : 1];  // (see k_lstm_seq_fwd)
    auto prefetch = [&](int t) {
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub) {
            const int row0 = g_row0 + sub * 64 + wave * 16;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = row0 + 4 * g + i, r = row < g_rows_end ? row : g_rows_end - 1;
                const int64_t tr = (int64_t)t * Cn + r;
                kp[sub][i] = p.keep[tr];
                if constexpr (KXB == 0) {
#pragma unroll
                    for (int u = 0; u < NU; ++u)
#pragma unroll
                        for (int q = 0; q < 3; ++q) xg[sub][i][q][u] = p.gx[tr * G3 + q * H + j0 + u * 16 + c];
                }
            }
        }
    };
    auto load_x = [&](int t) {
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub) {
            const int row = g_row0 + sub * 64 + wave * 16 + c, r = row < g_rows_end ? row : g_rows_end - 1;
#pragma unroll
            for (int blk = 0; blk < KXB; ++blk)
                xa[sub][blk] = *reinterpret_cast<const f32x4 *>(p.x + ((int64_t)t * Cn + r) * KX + 16 * blk + 4 * g);
        }
    };
    auto project_x = [&](int sub) {
#pragma unroll
        for (int nt = 0; nt < (KXB > 0 ? NT : 1); ++nt) xacc[sub][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int blk = 0; blk < KXB; ++blk)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    xacc[sub][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[sub][blk][j], bx[blk][nt][j], xacc[sub][nt], 0, 0, 0);
    };
    prefetch(0);
    if (KXB > 0) load_x(0);

    for (int t = 0; t < R; ++t) {
        if (t > 0 && !seq_wait(counter, ncol * (unsigned)t, abort_flag, flag)) return;
        float sv[NSUB][4][NU][5];  // r, z, n, hn, h
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub) {
            const int row0 = g_row0 + sub * 64 + wave * 16;
            if (row0 >= g_rows_end) continue;
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
            auto kbe = [&](int kb) { const int k = kb + rot; return k >= NKB ? k - NKB : k; };
#pragma unroll
            for (int b = 0; b < NBUF - 1; ++b) load_block(kbe(b), abuf[b]);
            if constexpr (KXB > 0) {  // x_t W_ih^T while the first h rows are on their way from L2
                __builtin_amdgcn_sched_barrier(0);
                project_x(sub);
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) {
                if (kb + NBUF - 1 < NKB) load_block(kbe(kb + NBUF - 1), abuf[(kb + NBUF - 1) % NBUF]);
                if constexpr (KXB > 0) __builtin_amdgcn_sched_barrier(0);  // (with the projection's registers live hipcc sinks these loads to their use)
                const float *bpk = wt + c * LDW + kbe(kb) * (KU * 16) + 4 * g;
#pragma unroll
                for (int ku = 0; ku < KU; ++ku) {
                    const f32x4 a4 = __builtin_bit_cast(f32x4, abuf[kb % NBUF][ku]);
                    const float *bp = bpk + ku * 16;
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        const f32x4 b4 = *reinterpret_cast<const f32x4 *>(bp + nt * 16 * LDW);
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[j], b4[j], acc[nt], 0, 0, 0);
                    }
                }
            }
            // ---- GRU cell (k_rnn_cell_fwd's arithmetic)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    float gxv[3];
#pragma unroll
                    for (int q = 0; q < 3; ++q)
                        gxv[q] = KXB > 0 ? xacc[sub][KXB > 0 ? q * NU + u : 0][i] + bih[q][u] : xg[KXB > 0 ? 0 : sub][i][q][u];
                    const float r = sigm(gxv[0] + (acc[0 * NU + u][i] + bias[0][u]));
                    const float z = sigm(gxv[1] + (acc[1 * NU + u][i] + bias[1][u]));
                    const float hn = acc[2 * NU + u][i] + bias[2][u];
                    const float n = tanh_c(gxv[2] + r * hn);
                    const float h = (1.0f - z) * n + z * hst[sub][i][u];
                    hst[sub][i][u] = h * kp[sub][i];
                    stg[(4 * g + i) * JB + u * 16 + c] = hst[sub][i][u];
                    sv[sub][i][u][0] = r; sv[sub][i][u][1] = z; sv[sub][i][u][2] = n; sv[sub][i][u][3] = hn; sv[sub][i][u][4] = h;
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int v = 0; v < NU; ++v) {
                const int f = v * 64 + lane, r = f / (JB / 4), c4 = f % (JB / 4), row = row0 + r;
                const f32x4 val = *reinterpret_cast<const f32x4 *>(stg + r * JB + c4 * 4);
                const uint32_t off = row < g_rows_end ? (uint32_t)((((int64_t)(t + 1) * Cn + row) * H + j0 + c4 * 4) * 4) : OOB;
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4, val), h_rsrc, off, 0, 16);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        if (t + 1 < R) {
            seq_arrive(counter);
            prefetch(t + 1);
            if (KXB > 0) load_x(t + 1);  // fragments of the next step's input
        }
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub) {
            const int row0 = g_row0 + sub * 64 + wave * 16;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = row0 + 4 * g + i;
                if (row < g_rows_end) {
                    const int64_t tr = (int64_t)t * Cn + row;
#pragma unroll
                    for (int u = 0; u < NU; ++u) {
                        const int j = j0 + u * 16 + c;
                        float *go = p.gates + tr * G4 + j;
                        go[0] = sv[sub][i][u][0]; go[H] = sv[sub][i][u][1]; go[2 * H] = sv[sub][i][u][2]; go[3 * H] = sv[sub][i][u][3];
                        p.hout[(int64_t)row * p.ho_rs + (int64_t)t * p.ho_ts + j] = sv[sub][i][u][4];
                    }
                }
            }
        }
    }
}

struct GruSeqBwd {
    const float *dout, *gates, *hprev, *keep, *whh;
    float *dgx, *dgh;
    unsigned *sync;
    int R, Cn, ngroups, rows_per_group;
    int64_t do_rs, do_ts;
    int row0, row_end;
};

template <int H, int JB, int NSUB>
__global__ __launch_bounds__(256, 1) void k_gru_seq_bwd(GruSeqBwd p) {
    constexpr int G3 = 3 * H, G4 = 4 * H, NC = 3 * JB, NU = JB / 16, LDK = G3 + 4;
    constexpr int KU = 8, NKB = G3 / 16 / KU;
    constexpr int NBUF = SF_SEQ_NBUF;
    constexpr int STG = 16 * NC;
    static_assert(NKB * KU * 16 == G3 && NKB >= NBUF - 1, "shape");
    __shared__ __attribute__((aligned(16))) float lds[JB * LDK + 4 * STG + 4];
    float *wk = lds, *flag = lds + JB * LDK + 4 * STG;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
    float *stg = lds + JB * LDK + wave * STG;
    const int group = blockIdx.x % p.ngroups, j0 = (blockIdx.x / p.ngroups) * JB;
    const unsigned ncol = H / JB;
    const int Cn = p.Cn, R = p.R;
    const int rot = (int)(blockIdx.x / p.ngroups) % NKB;
    unsigned *counter = p.sync + group * SEQ_SYNC_STRIDE, *abort_flag = p.sync + SEQ_ABORT_SLOT;
    for (int idx = tid; idx < JB * (G3 / 4); idx += 256) {  // wk[kk][n] = whh[j0 + kk][n]
        const int kk = idx / (G3 / 4), n4 = idx % (G3 / 4);
        *reinterpret_cast<f32x4 *>(wk + kk * LDK + n4 * 4) =
            *reinterpret_cast<const f32x4 *>(p.whh + (int64_t)(j0 + kk) * G3 + n4 * 4);
    }
    __syncthreads();
    const auto d_rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)p.dgh, 0, (int)((int64_t)R * Cn * G3 * 4), 0x00020000);
    const int g_row0 = p.row0 + group * p.rows_per_group;  // [row0, row_end): the slab of rows this launch covers
    const int g_rows_end = min(p.row_end, g_row0 + p.rows_per_group);
    float car_h[NSUB][4][NU];
#pragma unroll
    for (int sub = 0; sub < NSUB; ++sub)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int u = 0; u < NU; ++u) car_h[sub][i][u] = 0.0f;
    float pg[NSUB][4][NU][4], pdo[NSUB][4][NU], php[NSUB][4][NU], pkp[NSUB][4];
    auto prefetch = [&](int t) {
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub) {
            const int row0 = g_row0 + sub * 64 + wave * 16;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = row0 + 4 * g + i, r = row < g_rows_end ? row : g_rows_end - 1;
                const int64_t tr = (int64_t)t * Cn + r;
                pkp[sub][i] = t > 0 ? p.keep[tr - Cn] : 0.0f;
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    const int j = j0 + u * 16 + c;
                    const float *go = p.gates + tr * G4 + j;
                    pg[sub][i][u][0] = go[0]; pg[sub][i][u][1] = go[H]; pg[sub][i][u][2] = go[2 * H]; pg[sub][i][u][3] = go[3 * H];
                    pdo[sub][i][u] = p.dout[(int64_t)r * p.do_rs + (int64_t)t * p.do_ts + j];
                    php[sub][i][u] = p.hprev[tr * H + j];
                }
            }
        }
    };
    prefetch(R - 1);

    for (int s = 0; s < R; ++s) {
        const int t = R - 1 - s;
        float dir[NSUB][4][NU];  // dL/dh_prev that does not go through W_hh: dh * z
        // ---- phase A: GRU cell backward (k_rnn_cell_bwd's arithmetic); dgx plain, dgh = the hand-off payload
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub) {
            const int row0 = g_row0 + sub * 64 + wave * 16;
            if (row0 >= g_rows_end) continue;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = row0 + 4 * g + i;
                const bool ok = row < g_rows_end;
                const int64_t tr = (int64_t)t * Cn + (ok ? row : g_rows_end - 1);
#pragma unroll
                for (int u = 0; u < NU; ++u) {
                    const float r = pg[sub][i][u][0], z = pg[sub][i][u][1], n = pg[sub][i][u][2], hn = pg[sub][i][u][3];
                    float d = pdo[sub][i][u];
                    if (s > 0) d = d + car_h[sub][i][u];
                    const float dn_pre = (d * (1.0f - z)) * (1.0f - n * n);
                    const float dz_pre = (d * (php[sub][i][u] - n)) * (z * (1.0f - z));
                    const float dr_pre = (dn_pre * hn) * (r * (1.0f - r));
                    float *sp = stg + (4 * g + i) * NC + u * 16 + c;
                    sp[0] = dr_pre; sp[JB] = dz_pre; sp[2 * JB] = dn_pre * r;
                    dir[sub][i][u] = d * z;
                    if (ok) {
                        float *x = p.dgx + tr * G3 + j0 + u * 16 + c;
                        x[0] = dr_pre; x[H] = dz_pre; x[2 * H] = dn_pre;
                    }
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int v = 0; v < STG / 4 / 64; ++v) {  // 16 rows x NC floats as 16-byte write-through stores
                const int f = v * 64 + lane, r = f / (NC / 4), c4 = f % (NC / 4), row = row0 + r;
                const int q = (c4 * 4) / JB, u4 = (c4 * 4) % JB;
                const f32x4 val = *reinterpret_cast<const f32x4 *>(stg + r * NC + c4 * 4);
                const uint32_t off = row < g_rows_end ? (uint32_t)((((int64_t)t * Cn + row) * G3 + q * H + j0 + u4) * 4) : OOB;
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4, val), d_rsrc, off, 0, 16);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        if (t == 0) break;
        seq_arrive(counter);
        float kcur[NSUB][4];
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub)
#pragma unroll
            for (int i = 0; i < 4; ++i) kcur[sub][i] = pkp[sub][i];  // keep[t-1] of THIS step (prefetch overwrites pkp)
        prefetch(t - 1);
        if (!seq_wait(counter, ncol * (unsigned)(s + 1), abort_flag, flag)) return;
        // ---- phase B: dL/dh_{t-1}[rows, own units] = (dgh_t[rows, :] W_hh[own units, :]^T + dh * z) * keep[t-1]
#pragma unroll
        for (int sub = 0; sub < NSUB; ++sub) {
            const int row0 = g_row0 + sub * 64 + wave * 16;
            if (row0 >= g_rows_end) continue;
            f32x4 acc[NU];
#pragma unroll
            for (int u = 0; u < NU; ++u) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            const int arow = row0 + c;
            const uint32_t abase = arow < g_rows_end ? (uint32_t)((((int64_t)t * Cn + arow) * G3 + 4 * g) * 4) : OOB;
            i32x4 abuf[NBUF][KU];
            auto load_block = [&](int kb, i32x4 (&dst)[KU]) {
#pragma unroll
                for (int ku = 0; ku < KU; ++ku)
                    dst[ku] = __builtin_amdgcn_raw_buffer_load_b128(d_rsrc, abase + (uint32_t)((kb * KU + ku) * 64), 0, SF_SEQ_LOAD_AUX);
            };
            auto mma_block = [&](int kb, const i32x4 (&src)[KU]) {
#pragma unroll
                for (int ku = 0; ku < KU; ++ku) {
                    const f32x4 a4 = __builtin_bit_cast(f32x4, src[ku]);
                    const float *bp = wk + c * LDK + (kb * KU + ku) * 16 + 4 * g;
#pragma unroll
                    for (int u = 0; u < NU; ++u) {
                        const f32x4 b4 = *reinterpret_cast<const f32x4 *>(bp + u * 16 * LDK);
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            acc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[j], b4[j], acc[u], 0, 0, 0);
                    }
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
                    if (kb + b < NKB) mma_block(kbe(kb + b), abuf[b]);
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int u = 0; u < NU; ++u) car_h[sub][i][u] = (acc[u][i] + dir[sub][i][u]) * kcur[sub][i];
        }
    }
}

// ---- launch plans.  Every persistent pass splits the rows of ONE launch into row groups by the same rule: as many groups
// as the CUs hold (`wgs_per_group` co-resident work-groups each), at most `max_groups` (the hand-off counters) and at most
// one per `row_tile` rows; a group's rows are rounded up to the tile and must not exceed `max_rows_per_group`.
struct RowGroupPlan {
    int ngroups = 0, rows_per_group = 0;  // ngroups == 0: no plan
    explicit operator bool() const { return ngroups > 0; }
};

int device_cus() {  // of the current device; 0 on error
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
        return 0;
    return cus;
}

int row_groups_max(int wgs_per_group, int max_groups) {
    const int ng = device_cus() / wgs_per_group;
    return ng > max_groups ? max_groups : ng;
}

RowGroupPlan row_group_plan(int rows, int wgs_per_group, int max_groups, int row_tile, int max_rows_per_group) {
    int ng = row_groups_max(wgs_per_group, max_groups);
    const int need = (rows + row_tile - 1) / row_tile;
    if (ng > need) ng = need;
    if (ng < 1) return {};
    const int rpg = ((rows + ng - 1) / ng + row_tile - 1) / row_tile * row_tile;
    if (rpg > max_rows_per_group) return {};
    return {ng, rpg};
}

// The LDS passes: 16 hidden units per work-group, at most 8 row groups of at most 64 * SEQ_MAX_SUB rows.
// Widths with a compiled instantiation: 256 and 512 (the k-blocking needs H % 128 == 0 forward, an even number of
// 128-column blocks backward; both hold for LSTM and GRU); 32 / 64 / 128 take the row-owned passes (sf_rnn_rowseq.h),
// 1024 the 8-unit passes of sf_rnn_wideseq.h, every other width the per-step path.
constexpr int SEQ_JB = 16;
RowGroupPlan seq_plan(int Cn, int H) {
    if (H != 512 && H != 256) return {};
    return row_group_plan(Cn, H / SEQ_JB, 8, 16, 64 * SEQ_MAX_SUB);
}

// Rows of a pass are independent, so a call with more rows than one launch serves runs as consecutive launches over row
// slabs [r0, r1) of the same buffers (seq_run_slabs below).  Rows of one slab = the largest Cn seq_plan accepts on this
// device (2048 on 256 CUs); 0: no fused pass at this width.
// Both passes use it: a backward slab of this height runs k_*_seq_bwd (LDS), a shorter tail whatever seq_plan_r /
// seq_plan give a call of its size.  (1024-row slabs on the register-resident backward would make a 1025..2048-row call,
// one LDS launch today, differ from its own first slab; DESIGN.md 3.4 has the timing of both heights, taken with
// tools/experiments/sf_rnn_bwd_slab_regw_not_kept.patch.)
// The kernels address a whole [slot][Cn][width] tensor through ONE 32-bit buffer resource, so a call is limited to 2 GiB per
// hand-off tensor whatever the slabs; the forward entry points check the backward pass's tensor as well.
int seq_slab_rows(int H) {
    if (H != 512 && H != 256) return 0;
    return row_groups_max(H / SEQ_JB, 8) * 64 * SEQ_MAX_SUB;
}

#include "sf_rnn_regw.h"
#include "sf_rnn_rowseq.h"
#include "sf_rnn_wideseq.h"

// One launch of a fused pass: `family` as sf_rnn_seq_kernel_name numbers them
enum { FAM_PERSISTENT = 0, FAM_ROW_OWNED = 1, FAM_WIDE = 2 };
struct SeqLaunch {
    int targ[4] = {0, 0, 0, 0}, ntarg = 0;  // the chosen instantiation: its template arguments, as the dispatch tables list them
    unsigned grid = 0;
    int ngroups = 0, rows_per_group = 0;     // (row-owned: none)
    void set(std::initializer_list<int> a) { ntarg = (int)a.size(); std::copy(a.begin(), a.end(), targ); }
    bool is(std::initializer_list<int> a) const { return (int)a.size() == ntarg && std::equal(a.begin(), a.end(), targ); }
};

// rows ONE launch of the family serves at this width on this device; 0: the family has no pass at this width
int seq_family_slab_rows(int family, int H) {
    if (family == FAM_PERSISTENT) return seq_slab_rows(H);
    if (family == FAM_ROW_OWNED) return rowseq_width_ok(H) ? INT_MAX : 0;
    if (family == FAM_WIDE) return H == WIDE_H ? wide_groups_max() * 64 * SEQ_MAX_SUB : 0;
    return 0;
}

// The plan of ONE launch of (family, kind, pass) over `rows` rows; Kx != 0: the forward pass with the input projection
// fused in.  false: no such launch.
bool seq_launch(int family, int kind, int pass, int rows, int H, int Kx, SeqLaunch *L) {
    if ((kind != 0 && kind != 1) || (pass != 0 && pass != 1) || rows <= 0 || (Kx && (family != FAM_PERSISTENT || pass))) return false;
    // 64-row sub-tiles per work-group, unrolled at compile time (register-resident state): 1, 2 or 4 are compiled, 3 runs on 4
    auto nsub_of = [](const RowGroupPlan &g) { const int n = (g.rows_per_group + 63) / 64; return n == 3 ? 4 : n; };
    RowGroupPlan g;
    if (family == FAM_ROW_OWNED) {  // a work-group owns a tile of rows: grid = ceil(rows / tile rows of the instantiation)
        static_assert(RowSeqCfg<0, 32>::ROWS == RowSeqCfg<1, 32>::ROWS && RowSeqCfg<0, 64>::ROWS == RowSeqCfg<1, 64>::ROWS &&
                      RowSeqCfg<0, 128>::ROWS == RowSeqCfg<1, 128>::ROWS, "the tile depends on the width only");
        if (!rowseq_width_ok(H)) return false;
        const int tile = H == 32 ? RowSeqCfg<0, 32>::ROWS : H == 64 ? RowSeqCfg<0, 64>::ROWS : RowSeqCfg<0, 128>::ROWS;
        L->set({kind, H});
        L->grid = (unsigned)((rows + tile - 1) / tile);
    } else if (family == FAM_WIDE) {
        if (H != WIDE_H || !(g = wide_plan(rows))) return false;
        L->set({kind, nsub_of(g)});
        L->grid = (unsigned)(g.ngroups * WIDE_NCOL);
    } else if (family == FAM_PERSISTENT) {
        if (pass == 1 && (g = seq_plan_r(rows, H))) {  // 32 hidden units per work-group, W_hh slice in registers
            L->set({H, g.rows_per_group / 16});
            L->grid = (unsigned)(g.ngroups * (H / 32));
        } else {
            if (!(g = seq_plan(rows, H))) return false;
            const int nsub = nsub_of(g);
            if (Kx && (Kx != 64 || nsub > 2)) return false;  // x has 64 columns; register budget: one or two sub-tiles
            if (pass == 0) L->set({H, SEQ_JB, nsub, Kx / 16});
            else L->set({H, SEQ_JB, nsub});
            L->grid = (unsigned)(g.ngroups * (H / SEQ_JB));
        }
    } else {
        return false;
    }
    L->ngroups = g.ngroups;
    L->rows_per_group = g.rows_per_group;
    return true;
}
// the fused input projection is a one-launch feature: the whole call must have a plan
bool seq_fwd_x_plan(int Cn, int H, int Kx) {
    SeqLaunch L;
    return Kx != 0 && seq_launch(FAM_PERSISTENT, 0, 0, Cn, H, Kx, &L);
}

// ---- dispatch tables: how the plan's runtime choice reaches a template argument.  A row is one compiled instantiation;
// the row that matches the plan launches it (p != nullptr) and returns its name as rocprofv3 prints it, from the same tokens.
#define SEQ_ROW(KERN, ...)                                                         \
    if (L.is({__VA_ARGS__})) {                                                     \
        if (p) KERN<__VA_ARGS__><<<dim3(L.grid), dim3(256), 0, stream>>>(*p);      \
        return #KERN "<" #__VA_ARGS__ ">";                                         \
    }
// <prefix..., X>, <prefix..., Y>, <prefix..., Z>
#define SEQ_ROWS3(KERN, X, Y, Z, ...) SEQ_ROW(KERN, __VA_ARGS__, X) SEQ_ROW(KERN, __VA_ARGS__, Y) SEQ_ROW(KERN, __VA_ARGS__, Z)
// forward <H, JB, sub-tiles, 16-column blocks of x>: without the input projection, then with it
#define SEQ_ROWS_FWD(KERN)                                                                                     \
    SEQ_ROW(KERN, 512, 16, 1, 0) SEQ_ROW(KERN, 512, 16, 2, 0) SEQ_ROW(KERN, 512, 16, 4, 0)                     \
    SEQ_ROW(KERN, 256, 16, 1, 0) SEQ_ROW(KERN, 256, 16, 2, 0) SEQ_ROW(KERN, 256, 16, 4, 0)                     \
    SEQ_ROW(KERN, 512, 16, 1, 4) SEQ_ROW(KERN, 512, 16, 2, 4) SEQ_ROW(KERN, 256, 16, 1, 4) SEQ_ROW(KERN, 256, 16, 2, 4)

const char *seq_dispatch(const SeqLaunch &L, const LstmSeqFwd *p, hipStream_t stream) { SEQ_ROWS_FWD(k_lstm_seq_fwd) return nullptr; }
const char *seq_dispatch(const SeqLaunch &L, const LstmSeqBwd *p, hipStream_t stream) {
    // <H, row tiles per group>: the weights in registers (sf_rnn_regw.h); <H, JB, sub-tiles>: in LDS
    SEQ_ROW(k_lstm_seq_bwd_r, 512, 2) SEQ_ROW(k_lstm_seq_bwd_r, 512, 4) SEQ_ROW(k_lstm_seq_bwd_r, 256, 2) SEQ_ROW(k_lstm_seq_bwd_r, 256, 4)
    SEQ_ROWS3(k_lstm_seq_bwd, 1, 2, 4, 512, 16) SEQ_ROWS3(k_lstm_seq_bwd, 1, 2, 4, 256, 16)
    return nullptr;
}
const char *seq_dispatch(const SeqLaunch &L, const GruSeqFwd *p, hipStream_t stream) { SEQ_ROWS_FWD(k_gru_seq_fwd) return nullptr; }
const char *seq_dispatch(const SeqLaunch &L, const GruSeqBwd *p, hipStream_t stream) {
    SEQ_ROW(k_gru_seq_bwd_r, 512, 2) SEQ_ROW(k_gru_seq_bwd_r, 512, 4) SEQ_ROW(k_gru_seq_bwd_r, 256, 2) SEQ_ROW(k_gru_seq_bwd_r, 256, 4)
    SEQ_ROWS3(k_gru_seq_bwd, 1, 2, 4, 512, 16) SEQ_ROWS3(k_gru_seq_bwd, 1, 2, 4, 256, 16)
    return nullptr;
}
const char *seq_dispatch(const SeqLaunch &L, const RowSeqFwd *p, hipStream_t stream) {  // <kind, H>
    SEQ_ROWS3(k_rowseq_fwd, 32, 64, 128, 0) SEQ_ROWS3(k_rowseq_fwd, 32, 64, 128, 1)
    return nullptr;
}
const char *seq_dispatch(const SeqLaunch &L, const RowSeqBwd *p, hipStream_t stream) {
    SEQ_ROWS3(k_rowseq_bwd, 32, 64, 128, 0) SEQ_ROWS3(k_rowseq_bwd, 32, 64, 128, 1)
    return nullptr;
}
const char *seq_dispatch(const SeqLaunch &L, const WideSeqFwd *p, hipStream_t stream) {  // <kind, sub-tiles>
    SEQ_ROWS3(k_wideseq_fwd, 1, 2, 4, 0) SEQ_ROWS3(k_wideseq_fwd, 1, 2, 4, 1)
    return nullptr;
}
const char *seq_dispatch(const SeqLaunch &L, const WideSeqBwd *p, hipStream_t stream) {
    SEQ_ROWS3(k_wideseq_bwd, 1, 2, 4, 0) SEQ_ROWS3(k_wideseq_bwd, 1, 2, 4, 1)
    return nullptr;
}
#undef SEQ_ROWS_FWD
#undef SEQ_ROWS3
#undef SEQ_ROW

// the printed name of the instantiation L selects, from the table that launches it
const char *seq_kernel_name(const SeqLaunch &L, int family, int kind, int pass) {
    if (family == FAM_ROW_OWNED)
        return pass ? seq_dispatch(L, (const RowSeqBwd *)nullptr, nullptr) : seq_dispatch(L, (const RowSeqFwd *)nullptr, nullptr);
    if (family == FAM_WIDE)
        return pass ? seq_dispatch(L, (const WideSeqBwd *)nullptr, nullptr) : seq_dispatch(L, (const WideSeqFwd *)nullptr, nullptr);
    if (kind)
        return pass ? seq_dispatch(L, (const LstmSeqBwd *)nullptr, nullptr) : seq_dispatch(L, (const LstmSeqFwd *)nullptr, nullptr);
    return pass ? seq_dispatch(L, (const GruSeqBwd *)nullptr, nullptr) : seq_dispatch(L, (const GruSeqFwd *)nullptr, nullptr);
}

// hout / dout element (row, t) lives at row * rs + t * ts (+ unit): [R][Cn][H] (time-major) or, env_major, [Cn][R][H] = the
// row order of the minibatch itself (no transpose copy)
struct SeqStrides {
    int64_t rs, ts;
    SeqStrides(int env_major, int R, int Cn, int H) : rs(env_major ? (int64_t)R * H : (int64_t)H), ts(env_major ? (int64_t)H : (int64_t)Cn * H) {}
};

// The slab loop of the persistent entry points: one launch per row slab [r0, r1) of `slab` rows (a single one up to `slab`
// rows, the last one shorter).  Every slab gets the plan of a stand-alone call on r1 - r0 rows, which makes its results
// those of that call bit for bit; the hand-off counters are cleared before each launch, the abort word never.
template <class P>
int seq_run_slabs(const char *what, int family, int kind, int pass, int H, int Kx, int slab, P p, void *stream) {
    char memset_what[64];
    snprintf(memset_what, sizeof(memset_what), "%s memset", what);
    for (int r0 = 0; r0 < p.Cn; r0 += slab) {
        const int r1 = p.Cn - r0 < slab ? p.Cn : r0 + slab;
        SeqLaunch L;
        SF_REQUIRE(seq_launch(family, kind, pass, r1 - r0, H, Kx, &L), family == FAM_WIDE ? "%s: no plan for %d rows" : "%s: no plan for %d rows at H=%d",
                   what, r1 - r0, H);
        int rc = sf_hip_status(hipMemsetAsync(p.sync, 0, SEQ_ABORT_SLOT * sizeof(uint32_t), STREAM(stream)), memset_what);
        if (rc) return rc;
        p.ngroups = L.ngroups;
        p.rows_per_group = L.rows_per_group;
        p.row0 = r0;
        p.row_end = r1;
        SF_REQUIRE(seq_dispatch(L, &p, STREAM(stream)), "%s: no kernel for the plan", what);
        rc = sf_launch_status(what);
        if (rc) return rc;
    }
    return 0;
}

}  // namespace

extern "C" int sf_lstm_seq_supported(int Cn, int H) {
    // the OFFER ends at one launch, as before row slabs: on them Learner.train measured 1.09 - 1.55 x the per-step time at
    // 4096 / 8192 chunks (tools/wideseq_bench.py; nothing was measured in between).  The passes themselves run
    // any Cn > 0 as slabs; a caller that wants them beyond the offer calls the entry points.
    return Cn > 0 && Cn <= seq_slab_rows(H);
}

// the forward pass of both kinds (cprev / cout: LSTM only), on gx or, gx == nullptr, with the input projection x W_ih^T + b_ih
static int seq_fwd_impl(int kind, const float *gx, const float *x, const float *wih_t, const float *bih, int Kx, const float *whh,
                        const float *bhh, const float *keep, float *gates, float *hprev, float *hout, float *cprev, float *cout,
                        uint32_t *sync, int R, int Cn, int H, int env_major, void *stream) {
    const char *what = kind ? "sf_lstm_seq_fwd" : "sf_gru_seq_fwd";
    SF_REQUIRE((gx || (x && wih_t && bih)) && whh && bhh && keep && gates && hprev && hout && (!kind || (cprev && cout)) && sync && R > 0 &&
                   Cn > 0, "%s: bad args", what);
    const int slab = seq_slab_rows(H);
    SF_REQUIRE(slab > 0, "%s: unsupported shape Cn=%d H=%d (see sf_lstm_seq_supported)", what, Cn, H);
    SF_REQUIRE((int64_t)(R + 1) * Cn * H * 4 < 0x7FFFFFF0LL, "%s: state buffer exceeds 2 GiB", what);
    // (the backward pass's limit, checked HERE too: a pass pair is refused before its forward half runs)
    SF_REQUIRE((int64_t)R * Cn * (kind ? 4 : 3) * H * 4 < 0x7FFFFFF0LL, "%s: the backward pass's gate-gradient buffer would exceed 2 GiB", what);
    SF_REQUIRE(gx || (seq_fwd_x_plan(Cn, H, Kx) && (((uintptr_t)x | (uintptr_t)wih_t) & 15) == 0),
               "%s_x: unsupported shape Cn=%d H=%d Kx=%d (see sf_seq_fwd_x_supported)", what, Cn, H, Kx);
    const SeqStrides ho(env_major, R, Cn, H);
    if (kind)
        return seq_run_slabs(what, FAM_PERSISTENT, 1, 0, H, gx ? 0 : Kx, slab, LstmSeqFwd{gx, whh, bhh, keep, gates, hprev, hout, cprev, cout, sync,
                             R, Cn, 0, 0, ho.rs, ho.ts, x, wih_t, bih, 0, 0}, stream);
    return seq_run_slabs(what, FAM_PERSISTENT, 0, 0, H, gx ? 0 : Kx, slab, GruSeqFwd{gx, whh, bhh, keep, gates, hprev, hout, sync,
                         R, Cn, 0, 0, ho.rs, ho.ts, x, wih_t, bih, 0, 0}, stream);
}
extern "C" int sf_lstm_seq_fwd(const float *gx, const float *whh, const float *bhh, const float *keep, float *gates,
                               float *hprev, float *hout, float *cprev, float *cout, uint32_t *sync, int R, int Cn, int H,
                               int env_major, void *stream) {
    SF_REQUIRE(gx, "sf_lstm_seq_fwd: bad args");
    return seq_fwd_impl(1, gx, nullptr, nullptr, nullptr, 0, whh, bhh, keep, gates, hprev, hout, cprev, cout, sync, R, Cn, H,
                        env_major, stream);
}
extern "C" int sf_seq_fwd_x_supported(int Cn, int H, int Kx) {
    static const int on = getenv("SF_SEQ_FWD_X") ? atoi(getenv("SF_SEQ_FWD_X")) : 1;
    return on && seq_fwd_x_plan(Cn, H, Kx);
}
extern "C" int sf_lstm_seq_fwd_x(const float *x, const float *wih_t, const float *bih, int Kx, const float *whh,
                                 const float *bhh, const float *keep, float *gates, float *hprev, float *hout, float *cprev,
                                 float *cout, uint32_t *sync, int R, int Cn, int H, int env_major, void *stream) {
    SF_REQUIRE(x && wih_t && bih, "sf_lstm_seq_fwd_x: bad args");
    return seq_fwd_impl(1, nullptr, x, wih_t, bih, Kx, whh, bhh, keep, gates, hprev, hout, cprev, cout, sync, R, Cn, H,
                        env_major, stream);
}

extern "C" int sf_lstm_seq_bwd(const float *dout, const float *gates, const float *cprev, const float *cout,
                               const float *keep, const float *whh, float *dgx, uint32_t *sync, int R, int Cn, int H,
                               int env_major, void *stream) {
    SF_REQUIRE(dout && gates && cprev && cout && keep && whh && dgx && sync && R > 0 && Cn > 0,
               "sf_lstm_seq_bwd: bad args");
    const int slab = seq_slab_rows(H);
    SF_REQUIRE(slab > 0, "sf_lstm_seq_bwd: unsupported shape Cn=%d H=%d (see sf_lstm_seq_supported)", Cn, H);
    SF_REQUIRE((int64_t)R * Cn * 4 * H * 4 < 0x7FFFFFF0LL, "sf_lstm_seq_bwd: gate-gradient buffer exceeds 2 GiB");
    static const int ablate = getenv("SF_LSTM_ABLATE") ? atoi(getenv("SF_LSTM_ABLATE")) : 0;
    const SeqStrides d(env_major, R, Cn, H);
    LstmSeqBwd p{dout, gates, cprev, cout, keep, whh, dgx, sync, R, Cn, 0, 0, d.rs, d.ts, ablate, 0, 0};
    return seq_run_slabs("sf_lstm_seq_bwd", FAM_PERSISTENT, 1, 1, H, 0, slab, p, stream);
}

extern "C" int sf_gru_seq_fwd(const float *gx, const float *whh, const float *bhh, const float *keep, float *gates,
                              float *hprev, float *hout, uint32_t *sync, int R, int Cn, int H, int env_major,
                              void *stream) {
    SF_REQUIRE(gx, "sf_gru_seq_fwd: bad args");
    return seq_fwd_impl(0, gx, nullptr, nullptr, nullptr, 0, whh, bhh, keep, gates, hprev, hout, nullptr, nullptr, sync, R, Cn, H,
                        env_major, stream);
}
extern "C" int sf_gru_seq_fwd_x(const float *x, const float *wih_t, const float *bih, int Kx, const float *whh,
                                const float *bhh, const float *keep, float *gates, float *hprev, float *hout, uint32_t *sync,
                                int R, int Cn, int H, int env_major, void *stream) {
    SF_REQUIRE(x && wih_t && bih, "sf_gru_seq_fwd_x: bad args");
    return seq_fwd_impl(0, nullptr, x, wih_t, bih, Kx, whh, bhh, keep, gates, hprev, hout, nullptr, nullptr, sync, R, Cn, H,
                        env_major, stream);
}

extern "C" int sf_gru_seq_bwd(const float *dout, const float *gates, const float *hprev, const float *keep,
                              const float *whh, float *dgx, float *dgh, uint32_t *sync, int R, int Cn, int H,
                              int env_major, void *stream) {
    SF_REQUIRE(dout && gates && hprev && keep && whh && dgx && dgh && sync && R > 0 && Cn > 0, "sf_gru_seq_bwd: bad args");
    const int slab = seq_slab_rows(H);
    SF_REQUIRE(slab > 0, "sf_gru_seq_bwd: unsupported shape Cn=%d H=%d (see sf_lstm_seq_supported)", Cn, H);
    SF_REQUIRE((int64_t)R * Cn * 3 * H * 4 < 0x7FFFFFF0LL, "sf_gru_seq_bwd: gate-gradient buffer exceeds 2 GiB");
    const SeqStrides d(env_major, R, Cn, H);
    GruSeqBwd p{dout, gates, hprev, keep, whh, dgx, dgh, sync, R, Cn, 0, 0, d.rs, d.ts, 0, 0};
    return seq_run_slabs("sf_gru_seq_bwd", FAM_PERSISTENT, 0, 1, H, 0, slab, p, stream);
}

// ---- row-owned sequence passes (sf_rnn_rowseq.h): a work-group owns a tile of chunk rows for all R steps, one launch
extern "C" int sf_rnn_rowseq_supported(int kind, int Cn, int H) {
    return (kind == 0 || kind == 1) && Cn > 0 && rowseq_width_ok(H);
}

template <class P>
static int rowseq_run(const char *what, int kind, int pass, int H, const P &p, void *stream) {
    SeqLaunch L;
    SF_REQUIRE(seq_launch(FAM_ROW_OWNED, kind, pass, p.Cn, H, 0, &L) && seq_dispatch(L, &p, STREAM(stream)), "%s: no plan for %d rows at H=%d",
               what, p.Cn, H);
    return sf_launch_status(what);
}

extern "C" int sf_rnn_rowseq_fwd(int kind, const float *gx, const float *whh, const float *bhh, const float *keep, float *gates,
                                 float *hprev, float *hout, float *cprev, float *cout, int R, int Cn, int H, int env_major,
                                 void *stream) {
    SF_REQUIRE(sf_rnn_rowseq_supported(kind, Cn, H), "sf_rnn_rowseq_fwd: unsupported kind=%d Cn=%d H=%d (see sf_rnn_rowseq_supported)",
               kind, Cn, H);
    SF_REQUIRE(gx && whh && bhh && keep && gates && hprev && hout && R > 0, "sf_rnn_rowseq_fwd: bad args");
    SF_REQUIRE(kind == 0 || (cprev && cout), "sf_rnn_rowseq_fwd: LSTM needs cprev and cout");
    SF_REQUIRE(((uintptr_t)whh & 15) == 0 && (((uintptr_t)gx | (uintptr_t)bhh | (uintptr_t)keep | (uintptr_t)gates | (uintptr_t)hprev |
                                                (uintptr_t)hout | (uintptr_t)cprev | (uintptr_t)cout) & 3) == 0,
               "sf_rnn_rowseq_fwd: whh must be 16-byte aligned, every other operand 4-byte aligned");
    const SeqStrides ho(env_major, R, Cn, H);
    return rowseq_run("sf_rnn_rowseq_fwd", kind, 0, H, RowSeqFwd{gx, whh, bhh, keep, gates, hprev, hout, cprev, cout, R, Cn, ho.rs, ho.ts},
                      stream);
}

extern "C" int sf_rnn_rowseq_bwd(int kind, const float *dout, const float *gates, const float *hprev, const float *cprev,
                                 const float *cout, const float *keep, const float *whh, float *dgx, float *dgh, int R, int Cn,
                                 int H, int env_major, void *stream) {
    SF_REQUIRE(sf_rnn_rowseq_supported(kind, Cn, H), "sf_rnn_rowseq_bwd: unsupported kind=%d Cn=%d H=%d (see sf_rnn_rowseq_supported)",
               kind, Cn, H);
    SF_REQUIRE(dout && gates && keep && whh && dgx && R > 0, "sf_rnn_rowseq_bwd: bad args");
    SF_REQUIRE(kind == 1 || (hprev && dgh), "sf_rnn_rowseq_bwd: GRU needs hprev and dgh");
    SF_REQUIRE(kind == 0 || (cprev && cout), "sf_rnn_rowseq_bwd: LSTM needs cprev and cout");
    SF_REQUIRE(((uintptr_t)whh & 15) == 0 && (((uintptr_t)dout | (uintptr_t)gates | (uintptr_t)hprev | (uintptr_t)cprev | (uintptr_t)cout |
                                                (uintptr_t)keep | (uintptr_t)dgx | (uintptr_t)dgh) & 3) == 0,
               "sf_rnn_rowseq_bwd: whh must be 16-byte aligned, every other operand 4-byte aligned");
    const SeqStrides d(env_major, R, Cn, H);
    return rowseq_run("sf_rnn_rowseq_bwd", kind, 1, H, RowSeqBwd{dout, gates, hprev, cprev, cout, keep, whh, dgx, dgh, R, Cn, d.rs, d.ts},
                      stream);
}

// ---- persistent passes at H = 1024 (sf_rnn_wideseq.h): 8 hidden units per work-group, row slabs as above
// what the wide kernels can run: any Cn > 0 (row slabs beyond one launch)
static int wideseq_shape_ok(int kind, int Cn, int H) {
    return (kind == 0 || kind == 1) && Cn > 0 && H == WIDE_H && wide_groups_max() >= 1;
}
// what they are OFFERED for: the chunk range in which Learner.train measured faster than on the per-step launches
// by more than the spread (tools/wideseq_bench.py).  Measured at 64 / 512 / 2048 chunks: 0.40 / 0.99 / 1.91 of
// the per-step time for the GRU, 0.41 / 0.96 / 1.77 for the LSTM — the pass pulls rows x 1024 floats of h per work-group and
// step through L2 whatever the batch, the per-step GEMMs gain with it.  The GRU's 1 % at 512 chunks is inside the spread (it
// was outside in an earlier run), so the GRU is offered up to the largest chunk count that was SHOWN faster, 64; nothing
// between 64 and 512 was measured.
constexpr int WIDE_OFFER_MAX_CN[2] = {64, 512};  // GRU, LSTM
extern "C" int sf_rnn_wideseq_supported(int kind, int Cn, int H) {
    return wideseq_shape_ok(kind, Cn, H) && Cn <= WIDE_OFFER_MAX_CN[kind];
}

extern "C" int sf_rnn_seq_slab_rows(int kind, int H, int pass) {
    if ((kind != 0 && kind != 1) || (pass != 0 && pass != 1)) return 0;
    return seq_family_slab_rows(H == WIDE_H ? FAM_WIDE : FAM_PERSISTENT, H);
}

extern "C" int sf_rnn_wideseq_fwd(int kind, const float *gx, const float *whh, const float *bhh, const float *keep, float *gates,
                                  float *hprev, float *hout, float *cprev, float *cout, uint32_t *sync, int R, int Cn, int H,
                                  int env_major, void *stream) {
    SF_REQUIRE(wideseq_shape_ok(kind, Cn, H), "sf_rnn_wideseq_fwd: unsupported kind=%d Cn=%d H=%d (see sf_rnn_wideseq_supported)",
               kind, Cn, H);
    SF_REQUIRE(gx && whh && bhh && keep && gates && hprev && hout && sync && R > 0, "sf_rnn_wideseq_fwd: bad args");
    SF_REQUIRE(kind == 0 || (cprev && cout), "sf_rnn_wideseq_fwd: LSTM needs cprev and cout");
    SF_REQUIRE(((uintptr_t)hprev & 15) == 0 && (((uintptr_t)gx | (uintptr_t)whh | (uintptr_t)bhh | (uintptr_t)keep | (uintptr_t)gates |
                                                  (uintptr_t)hout | (uintptr_t)cprev | (uintptr_t)cout | (uintptr_t)sync) & 3) == 0,
               "sf_rnn_wideseq_fwd: hprev must be 16-byte aligned, every other operand 4-byte aligned");
    SF_REQUIRE((int64_t)(R + 1) * Cn * H * 4 < 0x7FFFFFF0LL, "sf_rnn_wideseq_fwd: state buffer exceeds 2 GiB");
    SF_REQUIRE((int64_t)R * Cn * (kind ? 4 : 3) * H * 4 < 0x7FFFFFF0LL,
               "sf_rnn_wideseq_fwd: the backward pass's gate-gradient buffer would exceed 2 GiB");
    const SeqStrides ho(env_major, R, Cn, H);
    WideSeqFwd p{gx, whh, bhh, keep, gates, hprev, hout, cprev, cout, sync, R, Cn, 0, 0, 0, 0, ho.rs, ho.ts};
    return seq_run_slabs("sf_rnn_wideseq_fwd", FAM_WIDE, kind, 0, H, 0, seq_family_slab_rows(FAM_WIDE, H), p, stream);
}

extern "C" int sf_rnn_wideseq_bwd(int kind, const float *dout, const float *gates, const float *hprev, const float *cprev,
                                  const float *cout, const float *keep, const float *whh, float *dgx, float *dgh, uint32_t *sync,
                                  int R, int Cn, int H, int env_major, void *stream) {
    SF_REQUIRE(wideseq_shape_ok(kind, Cn, H), "sf_rnn_wideseq_bwd: unsupported kind=%d Cn=%d H=%d (see sf_rnn_wideseq_supported)",
               kind, Cn, H);
    SF_REQUIRE(dout && gates && keep && whh && dgx && sync && R > 0, "sf_rnn_wideseq_bwd: bad args");
    SF_REQUIRE(kind == 1 || (hprev && dgh), "sf_rnn_wideseq_bwd: GRU needs hprev and dgh");
    SF_REQUIRE(kind == 0 || (cprev && cout), "sf_rnn_wideseq_bwd: LSTM needs cprev and cout");
    float *pay = kind == 0 ? dgh : dgx;  // the hand-off payload: 16-byte stores and loads
    SF_REQUIRE((((uintptr_t)pay | (uintptr_t)whh) & 15) == 0 &&
                   (((uintptr_t)dout | (uintptr_t)gates | (uintptr_t)hprev | (uintptr_t)cprev | (uintptr_t)cout | (uintptr_t)keep |
                     (uintptr_t)dgx | (uintptr_t)sync) & 3) == 0,
               "sf_rnn_wideseq_bwd: whh and the gate-gradient payload must be 16-byte aligned, every other operand 4-byte aligned");
    SF_REQUIRE((int64_t)R * Cn * (kind ? 4 : 3) * H * 4 < 0x7FFFFFF0LL, "sf_rnn_wideseq_bwd: gate-gradient buffer exceeds 2 GiB");
    const SeqStrides d(env_major, R, Cn, H);
    WideSeqBwd p{dout, gates, hprev, cprev, cout, keep, whh, dgx, pay, sync, R, Cn, 0, 0, 0, 0, d.rs, d.ts};
    return seq_run_slabs("sf_rnn_wideseq_bwd", FAM_WIDE, kind, 1, H, 0, seq_family_slab_rows(FAM_WIDE, H), p, stream);
}

// The name of the kernel a pass runs, as rocprofv3 prints it, from the plan and the table the entry points launch from.  A
// call of more than one slab is named by its first, full slab (a shorter tail may run another instantiation).
extern "C" int sf_rnn_seq_kernel_name(int family, int kind, int pass, int Cn, int H, int Kx, char *out, int cap) {
    SF_REQUIRE(out && cap >= 48 && (kind == 0 || kind == 1) && (pass == 0 || pass == 1) && Cn > 0,
               "sf_rnn_seq_kernel_name: bad args (kind=%d pass=%d Cn=%d)", kind, pass, Cn);
    const int slab = seq_family_slab_rows(family, H);
    SF_REQUIRE(slab > 0, "sf_rnn_seq_kernel_name: unsupported family=%d H=%d", family, H);
    SF_REQUIRE(Kx == 0 || (family == FAM_PERSISTENT && pass == 0 && seq_fwd_x_plan(Cn, H, Kx)),
               "sf_rnn_seq_kernel_name: unsupported shape Cn=%d H=%d Kx=%d (see sf_seq_fwd_x_supported)", Cn, H, Kx);
    SeqLaunch L;
    const int rows = Cn < slab ? Cn : slab;
    SF_REQUIRE(seq_launch(family, kind, pass, rows, H, Kx, &L), "sf_rnn_seq_kernel_name: no plan for %d rows at H=%d", rows, H);
    const char *name = seq_kernel_name(L, family, kind, pass);
    SF_REQUIRE(name, "sf_rnn_seq_kernel_name: no kernel for the plan");
    snprintf(out, (size_t)cap, "%s", name);
    return 0;
}

// ---- rollout state store that honours is_active.  sf_rnn_store_state (sf_rl.hip) with one more choice
// per row: a step recorded with policy_id < 0 was not the agent's to act on, so the row keeps the state it had
// (non_batched_sampling.py:605-612); the done mask applies either way.  out row b = [h | c] (c: LSTM)
// One thread per V floats of a row: V = 4 (one 16-byte load and store) where H, the row strides and the bases allow
// it, else 1.  A thread's floats lie on one side of the h | c seam because H % V == 0.
template <int V>
__global__ __launch_bounds__(256) void k_rnn_store_state_held(const float *__restrict__ h, const float *__restrict__ c,
                                                              const uint8_t *__restrict__ dones, int64_t done_stride,
                                                              const float *__restrict__ prev, int64_t prev_stride,
                                                              const int32_t *__restrict__ pid, int64_t pid_stride,
                                                              float *__restrict__ out, int64_t out_stride, int64_t B, int H) {
    using vec = typename std::conditional<V == 4, float4, float>::type;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int WV = (c ? 2 * H : H) / V;
    if (i >= B * WV) return;
    const int64_t b = i / WV;
    const int j = (int)(i - b * WV) * V;
    // the new state is loaded whatever policy_id says, as in the plain kernel: its load, the flag's and the done's are in
    // flight together, and only a held row waits for one more (prev)
    vec v = *reinterpret_cast<const vec *>(j < H ? h + b * H + j : c + b * H + j - H);
    if (pid[b * pid_stride] < 0) v = *reinterpret_cast<const vec *>(prev + b * prev_stride + j);
    if (dones[b * done_stride]) v = vec{};
    *reinterpret_cast<vec *>(out + b * out_stride + j) = v;
}

// do the row sets {a + b * sa + [0, W)} and {o + b * so + [0, W)}, b < B, share an element?  (units: floats.)  Exact for
// equal strides — columns t and t + 1 of one slab interleave without touching —, by extent otherwise
static bool rows_overlap(const float *a, int64_t sa, const float *o, int64_t so, int64_t B, int64_t W) {
    const intptr_t d = ((intptr_t)o - (intptr_t)a) / (intptr_t)sizeof(float);  // (both 4-byte aligned: checked by the caller)
    if (sa != so) return d < (B - 1) * sa + W && -d < (B - 1) * so + W;
    const intptr_t r = ((d % sa) + sa) % sa, k = (d - r) / sa;  // d = k * sa + r, 0 <= r < sa: o's row 0 starts r into a's row k
    return (r < W && k > -B && k < B) || (sa - r < W && k + 1 > -B && k + 1 < B);
}

extern "C" int sf_rnn_store_state_held(const float *h, const float *c, const uint8_t *dones, int64_t done_stride,
                                       const float *prev, int64_t prev_stride, const int32_t *policy_id,
                                       int64_t pid_stride, float *out, int64_t out_stride, int64_t B, int H,
                                       void *stream) {
    SF_REQUIRE(h && dones && out && B > 0 && H > 0, "sf_rnn_store_state_held: bad args");
    SF_REQUIRE(prev && policy_id, "sf_rnn_store_state_held: null prev / policy_id");
    const int64_t W = c ? 2 * (int64_t)H : H;
    SF_REQUIRE(prev_stride >= W && out_stride >= W, "sf_rnn_store_state_held: row stride below the row width %lld",
               (long long)W);
    SF_REQUIRE((((uintptr_t)prev | (uintptr_t)out) & 3) == 0, "sf_rnn_store_state_held: prev / out not 4-byte aligned");
    SF_REQUIRE(!rows_overlap(prev, prev_stride, out, out_stride, B, W), "sf_rnn_store_state_held: out overlaps prev");
    const bool v4 = H % 4 == 0 && prev_stride % 4 == 0 && out_stride % 4 == 0 &&
                    (((uintptr_t)h | (uintptr_t)c | (uintptr_t)prev | (uintptr_t)out) & 15) == 0;
    const int64_t n = B * W / (v4 ? 4 : 1);
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (v4)
        k_rnn_store_state_held<4><<<grid, block, 0, STREAM(stream)>>>(h, c, dones, done_stride, prev, prev_stride, policy_id,
                                                                     pid_stride, out, out_stride, B, H);
    else
        k_rnn_store_state_held<1><<<grid, block, 0, STREAM(stream)>>>(h, c, dones, done_stride, prev, prev_stride, policy_id,
                                                                     pid_stride, out, out_stride, B, H);
    return sf_launch_status("sf_rnn_store_state_held");
}
