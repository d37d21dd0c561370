// LDS-image WEIGHT GRADIENT for the convolutions behind conv1 with Cout = 64 and Cin in {32, 64} (Nature-CNN conv2:
// 32 x 20 x 20, 4x4 stride 2; conv3: 64 x 9 x 9, 3x3 stride 1):
//   dW[(kh, kw, c)][n] = sum_{sample, oh, ow} X[sample][S*oh + kh][S*ow + kw][c] * dY[sample][oh][ow][n]
//
// The im2col DMA kernel (k_wgrad_glds) moves every input element KS*KS/S^2 times through the vector-memory path and the
// dY rows once per weight-row tile (conv3: 5 tiles for K = 576): 4.55 GB per launch at n = 32768 against 1.09 GB of
// operands (profiles/r02_b_traffic.json) at 0.63 of the f32-MFMA peak.  Here
//   * work-groups are PERSISTENT over a contiguous run of samples; a sample's X image and dY image enter LDS exactly once
//     (LDS-DMA, two stages, one sample ahead): vector-memory traffic == the operands;
//   * per sample the gradient is ONE small GEMM [K rows] x [64 cols] with the OH*OW output pixels as the reduction index
//     (padded to a multiple of 4: 4 pixels per v_mfma_f32_16x16x4_f32).  The whole K x 64 accumulator lives in registers
//     for the whole launch: wave (nt, ks) owns output columns 16nt .. 16nt+15 and the row tiles of tap group ks
//     (conv3: 4 waves x 144 accumulator registers, two work-groups per CU; conv2: 8 waves x 64, one work-group per CU),
//     one partial per work-group, summed in fixed order by k_reduce_partials;
//   * im2col happens in the LDS ADDRESS: lane (i = row-in-tile, g = pixel-in-quad) reads the CT = Cin/16 channels
//     CT*i .. CT*i+CT-1 of its pixel at tap (kh, kw) with one ds_read_b128 / b64 whose tap part is an immediate — one LDS
//     read per CT MFMAs (the CT channel tiles: row i of tile j is channel CT*i + j), no VALU, no vector memory in the
//     pixel loop; the dY operand of a pixel quad is one ds_read_b32 reused by all row tiles; its running sum is the bias
//     gradient.  (The 8-wave conv2 form spreads the next sample's DMA pieces through the pixel loop and reads a quad ahead:
//     see its body.)
// Padded pixels: the dY slot is zero there (the DMA lanes past the image fetch a zero page), the X reads land in the
// zero-filled tail of the X slot or in the dY slot behind it (finite): 0 * finite = 0.
#pragma once

template <int CIN, int HH, int WW, int KS, int ST, int KSPLIT>
struct WimgGeom {
    static constexpr int OH = (HH - KS) / ST + 1, OW = (WW - KS) / ST + 1, P = OH * OW, STEPS = (P + 3) / 4, TAPS = KS * KS;
    static constexpr int CT = CIN / 16, TAPS_W = TAPS / KSPLIT, NW = 4 * KSPLIT;
    static constexpr int XB = HH * WW * CIN * 4, YB = P * 64 * 4;                 // image bytes
    static constexpr int XI = (XB + 1023) / 1024, YI = (4 * STEPS * 256 + 1023) / 1024;  // 1-KiB DMA instructions
    static constexpr int XSLOT = XI * 1024, YSLOT = YI * 1024, STAGE = XSLOT + YSLOT;
    static constexpr int NI = (XI + YI + NW - 1) / NW;                             // DMA instructions per wave and sample
    // furthest X byte a padded pixel can touch: pixel 4*STEPS-1 at the last tap, + one channel row
    static constexpr int PMAX = 4 * STEPS - 1;
    static constexpr int XREACH = (((ST * (PMAX / OW) + KS - 1) * WW + ST * (PMAX % OW) + KS - 1) * CIN + CIN) * 4;
    static_assert(CT == 2 || CT == 4, "Cin = 32 or 64: one float2 / float4 per lane");
    static_assert(TAPS % KSPLIT == 0 && TAPS_W % KS == 0, "a wave's tap group is whole filter rows");
    static_assert(XREACH <= STAGE, "padded-pixel reads must stay inside the stage");
    static_assert(2 * STAGE <= 160 * 1024 / (KSPLIT == 1 ? 2 : 1), "LDS: two work-groups per CU (4 waves) or one (8 waves)");
    // DMA instruction j of EVERY wave (q = wave + NW*j) lies inside its image with all 64 lanes: no zero-page lanes
    static constexpr bool piece_is_whole(int j) {
        for (int w = 0; w < NW; ++w) {
            const int q = w + NW * j;
            if (q < XI ? (q + 1) * 1024 > XB : (q - XI + 1) * 1024 > YB) return false;
        }
        return true;
    }
    static constexpr bool pieces_whole_but_last() {
        for (int j = 0; j + 1 < NI; ++j)
            if (!piece_is_whole(j)) return false;
        return true;
    }
};

// One 1-KiB LDS-DMA piece with ALL lanes or NONE (`on` != 0 / == 0, wave-uniform): EXEC is narrowed around the instruction
// instead of branching around it, so the piece stays where it is written inside a straight-line MFMA block (hipcc moves
// a conditional block of DMA instructions to the head of the loop body: the burst this is there to avoid).  hipcc does
// not see the load: the caller waits with vmcnt itself.  Form 1: uniform 64-bit base + 32-bit lane offset (no VALU);
// form 2: a 64-bit address per lane.
__device__ __forceinline__ void wimg_glds16_on(const void *ubase, uint32_t voff, uint32_t lds_byte_addr, uint32_t on) {
    uint64_t keep;
    asm volatile("s_mov_b64 %0, exec\n\ts_cmp_lg_u32 %4, 0\n\ts_cselect_b64 exec, exec, 0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %1, %2\n\ts_mov_b64 exec, %0"
                 : "=&s"(keep) : "v"(voff), "s"(ubase), "s"(lds_byte_addr), "s"(on) : "memory", "m0", "scc");
}
__device__ __forceinline__ void wimg_glds16_on(const void *src, uint32_t lds_byte_addr, uint32_t on) {
    uint64_t keep;
    asm volatile("s_mov_b64 %0, exec\n\ts_cmp_lg_u32 %3, 0\n\ts_cselect_b64 exec, exec, 0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %1, off\n\ts_mov_b64 exec, %0"
                 : "=&s"(keep) : "v"(src), "s"(lds_byte_addr), "s"(on) : "memory", "m0", "scc");
}

template <int CIN, int HH, int WW, int KS, int ST, int KSPLIT>
__global__ __launch_bounds__(256 * KSPLIT, 2) void k_wgrad_img(const float *__restrict__ in, int64_t in_stride,
                                                               const float *__restrict__ dy, float *__restrict__ partial,
                                                               float *__restrict__ partial_b, int nsamples) {
    typedef WimgGeom<CIN, HH, WW, KS, ST, KSPLIT> G;
    constexpr int OW = G::OW, STEPS = G::STEPS, TAPS_W = G::TAPS_W, CT = G::CT, NW = G::NW, N = 64, K = G::TAPS * CIN;
    constexpr int XB = G::XB, YB = G::YB, XI = G::XI, NI = G::NI, XSLOT = G::XSLOT, STAGE = G::STAGE;
    typedef float fvec __attribute__((ext_vector_type(CT)));
    __shared__ __attribute__((aligned(1024))) char lds[2 * STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i16 = lane & 15, kg = lane >> 4;
    const int nt = wave & 3, ks = wave >> 2;  // column tile, tap group
    // ---- this work-group's samples: a contiguous run
    const int per = (nsamples + (int)gridDim.x - 1) / (int)gridDim.x;
    const int s_beg = (int)blockIdx.x * per, s_end = min(nsamples, s_beg + per);
    f32x4 acc[TAPS_W][CT];
#pragma unroll
    for (int t = 0; t < TAPS_W; ++t)
#pragma unroll
        for (int j = 0; j < CT; ++j) acc[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;
    if (s_beg < s_end) {
        // ---- loader: instruction q = wave + NW*j of a sample; q < XI: 1 KiB of the X image, else of the dY image.  Lanes
        // past the image fetch zeros (the slot tails must be zero: padded pixels).
        int doff[NI];       // byte offset inside the sample's image, or -1: zero page
        bool is_y[NI];
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int q = wave + NW * j;
            is_y[j] = q >= XI;
            const int b = (is_y[j] ? q - XI : q) * 1024 + lane * 16;
            doff[j] = (b < (is_y[j] ? YB : XB)) ? b : -1;
        }
        const char *inb = reinterpret_cast<const char *>(in), *dyb = reinterpret_cast<const char *>(dy);
        const char *zero = reinterpret_cast<const char *>(sf_zero_page) + (lane & 7) * 16;
        auto issue = [&](int s, int stage) {
            const char *xs = inb + (int64_t)s * in_stride * 4, *ys = dyb + (int64_t)s * YB;
            char *st = lds + stage * STAGE;
#pragma unroll
            for (int j = 0; j < NI; ++j) {
                const int q = wave + NW * j;
                if (q < XI + G::YI) {
                    const char *src = doff[j] < 0 ? zero : (is_y[j] ? ys : xs) + doff[j];
                    GLDS16(src, st + (is_y[j] ? XSLOT + (q - XI) * 1024 : q * 1024));
                }
            }
        };
        // ---- fragment addresses: X of pixel p = 4*step + kg at this wave's first tap (channels CT*i16 ..), dY of
        // (pixel, column)
        const int tapbase = ks * (TAPS_W / KS) * WW * CIN * 4;
        int xo[STEPS];
#pragma unroll
        for (int st = 0; st < STEPS; ++st) {
            const int p = 4 * st + kg, oh = p / OW, ow = p - oh * OW;
            xo[st] = ((ST * oh * WW + ST * ow) * CIN + CT * i16) * 4 + tapbase;
        }
        const int yo = XSLOT + kg * 256 + (16 * nt + i16) * 4;

        if constexpr (KSPLIT == 2) {
            // ---- 8 waves, ONE work-group per CU: the two waves of a SIMD (ks = 0 / 1) run HALF A SAMPLE apart, one barrier
            // per half sample (phase).  In phase p set 0 multiplies half p & 1 of sample p >> 1 and set 1 what set 0 did in
            // phase p - 1: at every barrier one wave of each SIMD stands at a sample boundary and the other in mid-sample, so
            // the two never restart their LDS pipelines together.  Nobody bursts DMA: sample i + 1 goes into the stage that
            // sample i - 1 left with the barrier in front of phase 2i + 1 (set 1 read it last in phase 2i); every wave issues
            // its NI pieces of it two per pixel quad between that phase's first MFMAs and waits for them (vmcnt) before the
            // barrier in front of phase 2i + 2, whose first reader is set 0.  Each wave still sees samples ascending and
            // pixels ascending: every accumulator gets the same operands in the same order as with one barrier per sample
            // (bit-identical; the bias sum too).
            // Fragment bases: one register per (stage, filter row, quad), opaque to hipcc.  As a compile-time offset stage 1
            // lay beyond the 16-bit DS offset field (one v_add per ds_read_b64, no read2 pairing), and from one base per quad
            // hipcc pairs taps into ds_read2_b64 whose 8-bit offsets it reaches with more v_adds.  Here every tap of a row is
            // an immediate in both stages.  A quad's fragments (TAPS_W taps x CT channels + the dY word) are read into a
            // second register set between the two halves of the previous quad's MFMAs: the wait in front of a quad's first
            // MFMA has TAPS_W * CT / 2 MFMAs (256 matrix-pipe cycles) behind its youngest read.
            constexpr int H0 = (STEPS + 1) / 2, ROWS = TAPS_W / KS;  // pixel quads of half 0; filter rows of a wave
            static_assert(XB % 1024 == 0 && NW * (NI - 1) >= XI && G::pieces_whole_but_last(),
                          "only a wave's last piece, a dY piece, has zero-page lanes");
            const int cnt = s_end - s_beg;
            const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char *)lds;
            int xb[2][ROWS][STEPS], yb[2];
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                yb[g] = g * STAGE + yo;
                asm("" : "+v"(yb[g]));
#pragma unroll
                for (int r = 0; r < ROWS; ++r)
#pragma unroll
                    for (int st = 0; st < STEPS; ++st) {
                        xb[g][r][st] = g * STAGE + xo[st] + r * WW * CIN * 4;
                        asm("" : "+v"(xb[g][r][st]));
                    }
            }
            // the one piece with lanes past the dY image (if this wave has it): address = zy + sample * zs per lane, zs = 0
            // on the zero-page lanes (one v_mad_u64_u32 instead of an add and two selects per sample)
            const char *zy = doff[NI - 1] < 0 ? zero : dyb + doff[NI - 1];
            const uint32_t zs = doff[NI - 1] < 0 ? 0u : (uint32_t)YB;
            auto half = [&](auto hc, auto gc, int i) {
                constexpr int HF = decltype(hc)::value, STG = decltype(gc)::value, Q0 = HF ? H0 : 0, Q1 = HF ? STEPS : H0;
                static_assert(2 * (Q1 - Q0) >= NI, "two DMA pieces per quad cover a wave's share of the next sample");
                // this phase is 2i + 1 for the set with ks != HF: the other stage is free
                const uint32_t load = __builtin_amdgcn_readfirstlane(ks != HF && i + 1 < cnt ? 1 : 0);
                const uint32_t load_last = __builtin_amdgcn_readfirstlane(load && wave + NW * (NI - 1) < XI + G::YI ? 1 : 0);
                const uint32_t sn = (uint32_t)(s_beg + i + 1);
                const char *xs = inb + (int64_t)sn * in_stride * 4, *ys = dyb + (int64_t)sn * YB;
                const uint32_t dst = lds0 + (1 - STG) * STAGE;
                fvec a[2][TAPS_W];
                float b[2];
                auto fetch = [&](int st, int slot) {
                    b[slot] = *reinterpret_cast<const float *>(lds + yb[STG] + st * 1024);
#pragma unroll
                    for (int t = 0; t < TAPS_W; ++t)
                        a[slot][t] = *reinterpret_cast<const fvec *>(
                            __builtin_assume_aligned(lds + xb[STG][t / KS][st] + (t % KS) * CIN * 4, 4 * CT));
                };
                // (the empty asm ties an accumulator into the order of the volatile statements: the MFMAs are pure, and
                // without it hipcc sinks all of them below the reads and the DMA pieces of the whole phase)
                auto mfmas = [&](int slot, int t0, int t1) {
#pragma unroll
                    for (int t = t0; t < t1; ++t)
#pragma unroll
                        for (int j = 0; j < CT; ++j) {
                            acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[slot][t][j], b[slot], acc[t][j], 0, 0, 0);
                            asm volatile("" : "+v"(acc[t][j]));
                        }
                };
                fetch(Q0, 0);
#pragma unroll
                for (int st = Q0; st < Q1; ++st) {
                    const int slot = (st - Q0) & 1;
                    bsum += b[slot];
                    mfmas(slot, 0, TAPS_W / 2);
                    __builtin_amdgcn_sched_barrier(0);  // keep the next quad's reads ABOVE the second half of this quad
                    if (st + 1 < Q1) fetch(st + 1, slot ^ 1);
#pragma unroll
                    for (int j = 2 * (st - Q0); j < 2 * (st - Q0) + 2 && j < NI; ++j) {
                        const int q = wave + NW * j;
                        const uint32_t to = dst + (is_y[j] ? XSLOT + (q - XI) * 1024 : q * 1024);
                        if (G::piece_is_whole(j)) wimg_glds16_on(is_y[j] ? ys : xs, (uint32_t)doff[j], to, load);
                        else {
                            wimg_glds16_on(zy + (uint64_t)sn * zs, to, load_last);
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    mfmas(slot, TAPS_W / 2, TAPS_W);
                    __builtin_amdgcn_sched_barrier(0);
                }
            };
            // (own DMA pieces landed) + barrier: what was issued in the phase before is visible to every wave, and the stage
            // that the phase after the barrier overwrites has no reader left
            auto phase_barrier = [&]() {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
            };
            std::integral_constant<int, 0> c0;
            std::integral_constant<int, 1> c1;
            issue(s_beg, 0);
            if (ks == 1) phase_barrier();  // the lag: set 1 sits out phase 0 (and set 0 the last one)
            for (int i = 0; i < cnt; i += 2) {
                phase_barrier();
                half(c0, c0, i);
                phase_barrier();
                half(c1, c0, i);
                if (i + 1 < cnt) {
                    phase_barrier();
                    half(c0, c1, i + 1);
                    phase_barrier();
                    half(c1, c1, i + 1);
                }
            }
            if (ks == 0) phase_barrier();  // set 1's last phase
        } else {
            // ---- 4 waves, two work-groups per CU: one barrier per sample, the next sample's DMA right behind it
            auto sample = [&](auto stage_c) {
                constexpr int SOFF = decltype(stage_c)::value * STAGE;
#pragma unroll
                for (int st = 0; st < STEPS; ++st) {
                    const float b = *reinterpret_cast<const float *>(lds + SOFF + yo + st * 1024);
                    bsum += b;
#pragma unroll
                    for (int t = 0; t < TAPS_W; ++t) {
                        const int imm = SOFF + ((t / KS) * WW + (t % KS)) * CIN * 4;
                        const fvec a = *reinterpret_cast<const fvec *>(__builtin_assume_aligned(lds + xo[st] + imm, 4 * CT));
#pragma unroll
                        for (int j = 0; j < CT; ++j)
                            acc[t][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], b, acc[t][j], 0, 0, 0);
                    }
                }
            };
            issue(s_beg, 0);
            for (int s = s_beg; s < s_end; s += 2) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();  // sample s has landed in stage 0; everybody is done reading stage 1 (sample s-1)
                if (s + 1 < s_end) issue(s + 1, 1);
                sample(std::integral_constant<int, 0>{});
                if (s + 1 < s_end) {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __syncthreads();
                    if (s + 2 < s_end) issue(s + 2, 0);
                    sample(std::integral_constant<int, 1>{});
                }
            }
        }
    }
    // ---- this work-group's partial: row k = tap*CIN + CT*(4*kg + r) + j, column 16*nt + i16 (blocks without samples
    // write zeros: the reduction reads every partial)
    float *dst = partial + (int64_t)blockIdx.x * K * N + 16 * nt + i16;
#pragma unroll
    for (int t = 0; t < TAPS_W; ++t)
#pragma unroll
        for (int j = 0; j < CT; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) dst[((ks * TAPS_W + t) * CIN + CT * (4 * kg + r) + j) * N] = acc[t][j][r];
    if (partial_b && ks == 0) {
        bsum += __shfl_xor(bsum, 16, 64);
        bsum += __shfl_xor(bsum, 32, 64);
        if (kg == 0) partial_b[(int64_t)blockIdx.x * N + 16 * nt + i16] = bsum;
    }
}
