// sf_conv_bf16.hip — the inner conv layers of convnet_simple / convnet_atari on v_mfma_f32_16x16x32_bf16
// (cfg.encoder_conv_bf16): dense f32 NHWC layers without padding, (kernel, stride) in {(4, 2), (3, 1), (3, 2)}, Cin in
// {32, 64}, Cout in {32, 64, 128}.  Reached by name only (sf_conv_*_bf16); the plain sf_conv_* never route here.
//
// Arithmetic (the resnet family's, sf_resnet_bf16.hip): both MFMA operands are rounded to bf16 once per element, to nearest
// even: bf16(x), bf16(w), bf16(dout).  Accumulation is fp32; bias, activation and activation derivative are fp32 on
// unrounded values; db is the sum of the rounded dout.  The weights stay the fp32 [K*K*Cin, Cout] block and are converted
// inside the launch, on their way into the B registers: no bf16 copy outlives a launch.
//
// Forward and data gradient are ONE kernel (k_conv_bf16), an implicit GEMM with M = pixels, N = the produced channels, 32
// reduced channels of one tap per MFMA.
//   * A work-group (4 waves) stages its source once in LDS as bf16: S whole samples where S * pixels <= 128 and they fit,
//     else one sample, else a band of rows of one sample.  A pixel's channels are contiguous and the pixel stride is Cr + 8
//     elements, an odd number of 16-byte words, so that under stride 2 the 16 pixels of a lane group still spread over the
//     banks.
//   * M fragments run across the samples of the tile: pixel m of the tile is (m / P, m % P), so 81, 49, 16 or 18 pixels
//     per sample pad the LAST fragment of a tile only.  Fragments go round-robin to the MW wave groups; a wave holds FW of
//     them at a time and walks further chunks of FW * MW fragments with the LDS image in place.
//   * A wave owns TWO 16-column slices of N: one ds_read_b128 (pixel l % 16, channels 8 * (l / 16) .. + 7 of the chunk)
//     feeds two MFMAs.
//   * The weights stream from L2 as fp32 one (tap, chunk) ahead of the MFMAs and are rounded when the buffers swap.
//   * Data gradient under stride s: the input pixels with (h % s, w % s) = (ph, pw) are touched only by the taps
//     kh = ph + s*i, kw = pw + s*j, so each parity class is a stride-1 conv over dout with ceil((K-ph)/s) x ceil((K-pw)/s)
//     taps: input pixel (ph + s*a, pw + s*b) reads dout (a - i, b - j).  dout is staged with a zero halo of
//     ceil(K/s) - 1 pixels in front and zeros behind its last row / column; an M tile is the pixels of ONE class; the
//     classes are walked with the staged dout in place.  No structural zero is multiplied, and the input rows and columns
//     that no window covers come out as exact zeros (all their taps read the halo).
//   * An output element's reduction order is (tap row, tap column, chunk, the MFMA's own k order): it depends on neither
//     the batch size nor the sample's place in a tile, and there is no split-K.
//
// Weight gradient (k_conv_wgrad_bf16): M = 16 input channels of one tap, N = 16 output channels, K = 32 output pixels per
// MFMA, a lane holding 8 consecutive pixels of one channel.  The output pixels of the WHOLE batch are one flat sequence
// g = sample * OH*OW + pixel, cut into tiles of PT pixels (a multiple of 32) that ignore sample and row boundaries: nothing
// is padded but the end of the batch.  For a tile, the input is staged channel-major as one copy per tap (copy (kh, kw),
// position p = x[pixel p's window origin + (kh, kw)]), dout channel-major once, so every operand of every tap is one
// aligned ds_read_b128 at the same offset.  Grid = pixel parts x 16-channel Cin blocks; a part walks its tiles in order,
// partials go to [parts][K*K*Cin*Cout + Cout] and k_res_conv_wgrad_sum (sf_resnet.hip) adds them in part order: no float
// atomics.  The bias gradient is one more MFMA against ones.
//
// Compiled with -ffp-contract=off like its siblings: the epilogues round after each op.
#include "sf_common.h"
#include "sf_resnet_shared.h"
#include "sf_bf16.h"

#define STREAM(s) reinterpret_cast<hipStream_t>(s)

namespace {

constexpr int CB_CHUNK = 8;                // M fragments the four waves hold at a time
constexpr int CB_TILE_M = 16 * CB_CHUNK;   // ... = 128 pixels: the samples of a tile are chosen to fill them
constexpr int CB_LDS_BUDGET = 64 * 1024;   // dynamic LDS of one work-group
constexpr int CB_MIN_PARTS = 64;
constexpr int CB_GRID_TARGET = 1024;       // work-groups the weight gradient aims at: parts x Cin blocks

extern __shared__ float4 cb_lds4[];

inline bool cb_served(const sf_conv_desc *d) {
    if (!d || d->in_u8 != 0 || d->traj_T != 0 || d->KH != d->KW) return false;
    const int K = d->KH, s = d->stride;
    if (!((K == 4 && s == 2) || (K == 3 && s == 1) || (K == 3 && s == 2))) return false;
    if (!(d->Cin == 32 || d->Cin == 64) || !(d->Cout == 32 || d->Cout == 64 || d->Cout == 128)) return false;
    if (d->H < K || d->W < K || d->H > 4096 || d->W > 4096) return false;
    if (d->OH != (d->H - K) / s + 1 || d->OW != (d->W - K) / s + 1) return false;
    return d->relu >= 0 && d->relu <= 3;
}

// ------------------------------------------------------------------------------------------------ forward / dgrad
struct CbGeo {
    int H, W, OH, OW, K, st, Cin, Cout;
};

struct CbTile {
    int S;        // samples of a tile
    int TR, nrt;  // rows of a tile (forward: output rows; data gradient: class rows a, input row = ph + st*a); tiles per image
    int LH, LW;   // staged rows and columns of one sample
    int T;        // data gradient: ceil(K / st), the most taps of a class per dimension (halo = T - 1)
    int cs;       // bf16 elements per staged pixel: Cr + 8
};

// false: one row band of this layer does not fit the LDS budget (the image is too wide)
bool cb_tile(const CbGeo &g, bool dgrad, int64_t n, CbTile *out) {
    CbTile t;
    t.T = ceil_div(g.K, g.st);
    t.cs = (dgrad ? g.Cout : g.Cin) + 8;
    const int rows = dgrad ? ceil_div(g.H, g.st) : g.OH, cols = dgrad ? ceil_div(g.W, g.st) : g.OW;
    t.LW = dgrad ? cols + t.T - 1 : (g.OW - 1) * g.st + g.K;
    auto lh = [&](int TR) { return dgrad ? TR + t.T - 1 : (TR - 1) * g.st + g.K; };
    auto bytes = [&](int S, int TR) { return (int64_t)S * lh(TR) * t.LW * t.cs * 2; };
    int TR = rows;
    while (TR > 1 && bytes(1, TR) > CB_LDS_BUDGET) --TR;
    if (bytes(1, TR) > CB_LDS_BUDGET) return false;
    t.nrt = ceil_div(rows, TR);
    t.TR = ceil_div(rows, t.nrt);
    t.S = 1;
    if (t.nrt == 1)
        while (t.S < n && (t.S + 1) * rows * cols <= CB_TILE_M && bytes(t.S + 1, t.TR) <= CB_LDS_BUDGET) ++t.S;
    t.LH = lh(t.TR);
    *out = t;
    return true;
}

// NP: pairs of 16-column slices of the produced channels Cn = 32 * NP; MW: wave groups that share a pair and split the fragments.
// DGRAD = false: src = x [n,H,W,Cin] (samples src_stride apart), out = act(conv + bias) [n,OH,OW,Cout].
// DGRAD = true:  src = dout [n,OH,OW,Cout] dense, out = din [n,H,W,Cin] = conv_transpose * act'(in_act).
template <int NP, int MW, bool DGRAD>
__global__ __launch_bounds__(256) void k_conv_bf16(const float *__restrict__ src, const float *__restrict__ w,
                                                   const float *__restrict__ bias, const float *__restrict__ in_act,
                                                   float *__restrict__ out, int act, int64_t n, int64_t src_stride,
                                                   int64_t src_offset, CbGeo g, CbTile t) {
    static_assert(NP * MW == 4, "four waves");
    constexpr int Cn = 32 * NP, FW = CB_CHUNK / MW;
    __bf16 *lds = reinterpret_cast<__bf16 *>(cb_lds4);
    const int K = g.K, st = g.st, Cr = DGRAD ? g.Cout : g.Cin;
    const int LH = t.LH, LW = t.LW, LP = LH * LW, cs = t.cs, halo = t.T - 1;
    const int rt = blockIdx.x % t.nrt, r0 = rt * t.TR;  // first output row (forward) / class row (data gradient) of the tile
    const int64_t s0 = (int64_t)(blockIdx.x / t.nrt) * t.S;
    const int ns = (int)min((int64_t)t.S, n - s0);
    // ---- source -> LDS as bf16, exact zeros outside the source image and past the last sample
    const int SH = DGRAD ? g.OH : g.H, SW = DGRAD ? g.OW : g.W;
    const int q8 = Cr >> 3;
    for (int i = threadIdx.x; i < t.S * LP * q8; i += 256) {
        const int q = i % q8, lp = i / q8, s = lp / LP, rr = (lp - s * LP) / LW, cc = lp - s * LP - rr * LW;
        const int h = DGRAD ? r0 + rr - halo : r0 * st + rr, ww = DGRAD ? cc - halo : cc;
        float4 v0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), v1 = v0;
        if (s < ns && h >= 0 && h < SH && ww >= 0 && ww < SW) {
            const float4 *p = reinterpret_cast<const float4 *>(src + (src_offset + s0 + s) * src_stride + ((int64_t)h * SW + ww) * Cr + 8 * q);
            v0 = p[0];
            v1 = p[1];
        }
        *reinterpret_cast<bf16x8 *>(lds + lp * cs + 8 * q) = bf16_pack(v0, v1);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, pair = wave % NP, wg = wave / NP;
    const int lr = lane & 15, lg = lane >> 4;
    const int nch = Cr >> 5;
    const int ncls = DGRAD ? st * st : 1;
    for (int cls = 0; cls < ncls; ++cls) {
        const int ph = DGRAD ? cls / st : 0, pw = DGRAD ? cls % st : 0;
        // rows and columns of this class in the tile, taps of the class
        int rows_c, cols_c, ntr, ntc;
        if (DGRAD) {
            rows_c = max(0, min(t.TR, (g.H - ph + st - 1) / st - r0));
            cols_c = max(0, (g.W - pw + st - 1) / st);
            ntr = (K - ph + st - 1) / st;
            ntc = (K - pw + st - 1) / st;
        } else {
            rows_c = min(t.TR, g.OH - r0);
            cols_c = g.OW;
            ntr = ntc = K;
        }
        const int PC = rows_c * cols_c, M = t.S * PC;
        if (M <= 0) continue;
        const int nfr = (M + 15) >> 4, steps = ntr * ntc * nch;
        for (int c0 = 0; (c0 * FW) * MW + wg < nfr; ++c0) {  // (wave-uniform; no barrier below)
            int hb[FW];  // LDS offset of the lane's pixel at tap (0, 0), its channel group added
            floatx4 acc[FW][2];
#pragma unroll
            for (int f = 0; f < FW; ++f) {
                int m = ((c0 * FW + f) * MW + wg) * 16 + lr;
                if (m >= M) m = 0;  // a lane past the tile reads a real pixel; its rows are never stored
                const int s = m / PC, r = (m - s * PC) / cols_c, c = m - s * PC - r * cols_c;
                hb[f] = (DGRAD ? (s * LH + r + halo) * LW + c + halo : (s * LH + r * st) * LW + c * st) * cs + 8 * lg;
                acc[f][0] = acc[f][1] = (floatx4){0.0f, 0.0f, 0.0f, 0.0f};
            }
            // fp32 B operands of step (tap, 32-channel chunk): lane (column lr of slice u, group lg) holds k-rows 8*lg .. + 7
            float4 braw[2][2];
            auto load_b = [&](int tr, int tc, int ch) {
                const int wtap = DGRAD ? (ph + st * tr) * K + pw + st * tc : tr * K + tc;
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int col = (pair * 2 + u) * 16 + lr;
                    if (DGRAD) {  // B[o][c] = W[wtap*Cin + c][o]: the lane's row c, eight consecutive o
                        const float4 *p = reinterpret_cast<const float4 *>(w + ((int64_t)wtap * Cn + col) * Cr + ch * 32 + 8 * lg);
                        braw[u][0] = p[0];
                        braw[u][1] = p[1];
                    } else {      // B[k][o] = W[wtap*Cin + k][o]: eight rows down the lane's column
                        const float *p = w + ((int64_t)wtap * Cr + ch * 32 + 8 * lg) * Cn + col;
                        braw[u][0] = make_float4(p[0], p[Cn], p[2 * Cn], p[3 * Cn]);
                        braw[u][1] = make_float4(p[4 * Cn], p[5 * Cn], p[6 * Cn], p[7 * Cn]);
                    }
                }
            };
            load_b(0, 0, 0);
            int tr = 0, tc = 0, ch = 0;
            for (int it = 0; it < steps; ++it) {
                const bf16x8 b0 = bf16_pack(braw[0][0], braw[0][1]), b1 = bf16_pack(braw[1][0], braw[1][1]);
                const int aoff = (DGRAD ? -(tr * LW + tc) : tr * LW + tc) * cs + ch * 32;
                if (++ch == nch) {
                    ch = 0;
                    if (++tc == ntc) { tc = 0; ++tr; }
                }
                if (it + 1 < steps) load_b(tr, tc, ch);
#pragma unroll
                for (int f = 0; f < FW; ++f) {
                    if ((c0 * FW + f) * MW + wg < nfr) {
                        const bf16x8 a = *reinterpret_cast<const bf16x8 *>(lds + hb[f] + aoff);
                        acc[f][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b0, acc[f][0], 0, 0, 0);
                        acc[f][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b1, acc[f][1], 0, 0, 0);
                    }
                }
            }
            // ---- epilogue: accumulator j of fragment f, slice u is pixel 16*fragment + 4*lg + j, channel (2*pair + u)*16 + lr
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int o = (pair * 2 + u) * 16 + lr;
                const float bo = DGRAD ? 0.0f : bias[o];
#pragma unroll
                for (int f = 0; f < FW; ++f) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int m = ((c0 * FW + f) * MW + wg) * 16 + 4 * lg + j;
                        if (m >= M) continue;
                        const int s = m / PC, r = (m - s * PC) / cols_c, c = m - s * PC - r * cols_c;
                        if (s >= ns) continue;
                        float v = acc[f][u][j];
                        if (DGRAD) {
                            const int64_t idx = (((s0 + s) * g.H + ph + st * (r0 + r)) * g.W + pw + st * c) * Cn + o;
                            if (act) v = v * act_bwd_out(act, in_act[idx]);
                            out[idx] = v;
                        } else {
                            const int64_t idx = (((s0 + s) * g.OH + r0 + r) * g.OW + c) * Cn + o;
                            v = v + bo;
                            out[idx] = act_fwd(act, v);
                        }
                    }
                }
            }
        }
    }
}

template <bool DGRAD>
void cb_launch(int Cn, dim3 grid, size_t lds, hipStream_t s, const float *src, const float *w, const float *bias,
               const float *in_act, float *out, int act, int64_t n, int64_t src_stride, int64_t src_offset, const CbGeo &g,
               const CbTile &t) {
#define CB_GO(NP, MW)                                                                                                  \
    hipLaunchKernelGGL((k_conv_bf16<NP, MW, DGRAD>), grid, dim3(256), lds, s, src, w, bias, in_act, out, act, n,        \
                       src_stride, src_offset, g, t)
    if (Cn == 32) CB_GO(1, 4);
    else if (Cn == 64) CB_GO(2, 2);
    else CB_GO(4, 1);
#undef CB_GO
}

// ------------------------------------------------------------------------------------------------ weight gradient
struct CbBand {
    int PT;           // output pixels of a tile, a multiple of 32
    int cs;           // bf16 elements per staged channel row: PT or PT + 8, an odd number of 16-byte words
    int blocks;       // 16-channel Cin blocks = grid.y
    int64_t NPX, NT;  // output pixels of the batch, tiles
    int64_t tpp, parts;  // tiles per part, parts = grid.x
    int64_t lds_bytes;
};

CbBand cb_band(const sf_conv_desc &d, int64_t n) {
    CbBand t;
    const int rows = d.KH * d.KW * 16 + d.Cout;
    t.PT = 256;
    while (t.PT > 32 && (int64_t)rows * odd8(t.PT) * 2 > CB_LDS_BUDGET) t.PT -= 32;
    t.cs = odd8(t.PT);
    t.lds_bytes = (int64_t)rows * t.cs * 2;
    t.blocks = d.Cin / 16;
    t.NPX = n * d.OH * d.OW;
    t.NT = (t.NPX + t.PT - 1) / t.PT;
    const int64_t target = std::max(CB_MIN_PARTS, CB_GRID_TARGET / t.blocks);
    t.tpp = std::max<int64_t>(1, (t.NT + target - 1) / target);
    t.parts = std::max<int64_t>(1, (t.NT + t.tpp - 1) / t.tpp);
    return t;
}

// KS x KS taps, stride ST; NCOG waves, wave cog owns the 16-column tiles cog*CT .. + CT-1 of Cout = 16 * NCOG * CT
template <int KS, int ST, int NCOG, int CT>
__global__ __launch_bounds__(64 * NCOG) void k_conv_wgrad_bf16(const float *__restrict__ x, const float *__restrict__ gy,
                                                              float *__restrict__ part, int64_t x_stride, int64_t x_offset,
                                                              int W, int OH, int OW, int Cin, CbBand t) {
    constexpr int TAPS = KS * KS, Cout = 16 * NCOG * CT, NTHR = 64 * NCOG;
    __bf16 *la = reinterpret_cast<__bf16 *>(cb_lds4);
    const int PT = t.PT, cs = t.cs, RUNS = PT >> 3, P = OH * OW;
    __bf16 *lgy = la + TAPS * 16 * cs;
    const int cbase = blockIdx.y * 16;
    const int lane = threadIdx.x & 63, cog = threadIdx.x >> 6, lr = lane & 15, lg = lane >> 4;
    const bool do_bias = blockIdx.y == 0;
    floatx4 acc[TAPS][CT], accb[CT];
#pragma unroll
    for (int u = 0; u < CT; ++u) {
        accb[u] = (floatx4){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int tap = 0; tap < TAPS; ++tap) acc[tap][u] = (floatx4){0.0f, 0.0f, 0.0f, 0.0f};
    }
    const bf16x8 ones8 = bf16_ones8();
    const int64_t t0 = (int64_t)blockIdx.x * t.tpp, t1 = min(t.NT, t0 + t.tpp);
    const __bf16 *xa = la + lr * cs, *ga = lgy + (cog * CT * 16 + lr) * cs;
    for (int64_t tile = t0; tile < t1; ++tile) {
        const int64_t g0 = tile * PT;
        const int64_t sb = g0 / P;                                 // sample of the tile's first pixel
        const int pb = (int)(g0 - sb * P);                         // ... and its pixel in that sample
        const int live = (int)min((int64_t)PT, t.NPX - g0);        // pixels of the tile inside the batch
        __syncthreads();  // the previous tile's fragments have been read
        // ---- input, channel-major, one copy per tap: copy (kh, kw), position p = x at pixel p's window origin + (kh, kw)
        for (int i = threadIdx.x; i < TAPS * RUNS * 4; i += NTHR) {
            const int q = i & 3, run = (i >> 2) % RUNS, tap = (i >> 2) / RUNS, kh = tap / KS, kw = tap - kh * KS;
            __bf16 v[8][4];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int p = 8 * run + e;
                float4 f = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (p < live) {
                    const int l = pb + p, s = l / P, pix = l - s * P, oh = pix / OW, ow = pix - oh * OW;
                    f = *reinterpret_cast<const float4 *>(x + (x_offset + sb + s) * x_stride +
                                                          ((int64_t)(oh * ST + kh) * W + ow * ST + kw) * Cin + cbase + 4 * q);
                }
                v[e][0] = (__bf16)f.x; v[e][1] = (__bf16)f.y; v[e][2] = (__bf16)f.z; v[e][3] = (__bf16)f.w;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                bf16x8 o;
#pragma unroll
                for (int k = 0; k < 8; ++k) o[k] = v[k][c];
                *reinterpret_cast<bf16x8 *>(la + (tap * 16 + 4 * q + c) * cs + 8 * run) = o;
            }
        }
        // ---- dout, channel-major; pixels past the batch are zeros
        for (int i = threadIdx.x; i < RUNS * (Cout >> 2); i += NTHR) {
            const int q = i % (Cout >> 2), run = i / (Cout >> 2);
            __bf16 v[8][4];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int p = 8 * run + e;
                float4 f = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (p < live) f = *reinterpret_cast<const float4 *>(gy + (g0 + p) * Cout + 4 * q);
                v[e][0] = (__bf16)f.x; v[e][1] = (__bf16)f.y; v[e][2] = (__bf16)f.z; v[e][3] = (__bf16)f.w;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                bf16x8 o;
#pragma unroll
                for (int k = 0; k < 8; ++k) o[k] = v[k][c];
                *reinterpret_cast<bf16x8 *>(lgy + (4 * q + c) * cs + 8 * run) = o;
            }
        }
        __syncthreads();
        // ---- 32 pixels per MFMA: lane group lg takes run 4*it + lg
        for (int it = 0; 32 * it < live; ++it) {
            const int ofs = 8 * (4 * it + lg);
            bf16x8 b[CT];
#pragma unroll
            for (int u = 0; u < CT; ++u) b[u] = *reinterpret_cast<const bf16x8 *>(ga + u * 16 * cs + ofs);
#pragma unroll
            for (int tap = 0; tap < TAPS; ++tap) {
                const bf16x8 a = *reinterpret_cast<const bf16x8 *>(xa + tap * 16 * cs + ofs);
#pragma unroll
                for (int u = 0; u < CT; ++u) acc[tap][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[u], acc[tap][u], 0, 0, 0);
            }
            if (do_bias) {
#pragma unroll
                for (int u = 0; u < CT; ++u) accb[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones8, b[u], accb[u], 0, 0, 0);
            }
        }
    }
    // accumulator j: input channel 4*lg + j of the block, output channel lr of Cout tile u
    const int KC = TAPS * Cin * Cout;
    float *pp = part + (int64_t)blockIdx.x * (KC + Cout);
#pragma unroll
    for (int u = 0; u < CT; ++u) {
        const int o = (cog * CT + u) * 16 + lr;
#pragma unroll
        for (int tap = 0; tap < TAPS; ++tap)
#pragma unroll
            for (int j = 0; j < 4; ++j) pp[(tap * Cin + cbase + 4 * lg + j) * Cout + o] = acc[tap][u][j];
        if (do_bias && lg == 0) pp[KC + o] = accb[u][0];
    }
}

template <int KS, int ST>
void cb_wgrad_launch(int Cout, dim3 grid, size_t lds, hipStream_t s, const float *x, const float *gy, float *part,
                     int64_t x_stride, int64_t x_offset, const sf_conv_desc &d, const CbBand &t) {
#define CB_WGO(NCOG, CT)                                                                                               \
    hipLaunchKernelGGL((k_conv_wgrad_bf16<KS, ST, NCOG, CT>), grid, dim3(64 * NCOG), lds, s, x, gy, part, x_stride,     \
                       x_offset, d.W, d.OH, d.OW, d.Cin, t)
    if (Cout == 32) CB_WGO(2, 1);
    else if (Cout == 64) CB_WGO(4, 1);
    else CB_WGO(4, 2);
#undef CB_WGO
}

CbGeo cb_geo(const sf_conv_desc &d) { return CbGeo{d.H, d.W, d.OH, d.OW, d.KH, d.stride, d.Cin, d.Cout}; }

int cb_check(const sf_conv_desc *d, const char *what) {
    SF_REQUIRE(d != nullptr, "%s: desc is NULL", what);
    if (!cb_served(d)) {
        snprintf(sf_err_buf, sizeof(sf_err_buf),
                 "%s: Cin=%d Cout=%d kernel=%dx%d stride=%d H=%d W=%d OH=%d OW=%d in_u8=%d traj_T=%d relu=%d (the bf16 family "
                 "serves dense f32 NHWC layers without padding, (kernel, stride) in {(4, 2), (3, 1), (3, 2)}, Cin in {32, 64}, "
                 "Cout in {32, 64, 128})", what, d->Cin, d->Cout, d->KH, d->KW, d->stride, d->H, d->W, d->OH, d->OW, d->in_u8,
                 d->traj_T, d->relu);
        return SF_ERR_UNSUPPORTED;
    }
    return SF_OK;
}

int cb_too_wide(const sf_conv_desc &d, const char *what) {
    snprintf(sf_err_buf, sizeof(sf_err_buf), "%s: one row band of a W=%d image (Cin=%d, Cout=%d, %dx%d stride %d) exceeds the "
             "%d-byte LDS budget", what, d.W, d.Cin, d.Cout, d.KH, d.KW, d.stride, CB_LDS_BUDGET);
    return SF_ERR_UNSUPPORTED;
}

}  // namespace

extern "C" int sf_conv_bf16_supported(int op, int64_t n, const sf_conv_desc *h_desc) {
    if (n < 0 || op < 0 || op > 2 || !cb_served(h_desc)) return 0;
    if (op == 1) return 1;  // the weight gradient's tiles are cut from the flat pixel sequence: any geometry fits
    CbTile t;
    return cb_tile(cb_geo(*h_desc), op == 2, n, &t) ? 1 : 0;
}

extern "C" int sf_conv_fwd_bf16(const void *in, int64_t in_sample_stride, const int32_t *index, int64_t offset, const float *w,
                                const float *bias, float *out, int64_t n, const sf_conv_desc *h_desc, void *workspace,
                                int64_t workspace_bytes, void *stream) {
    (void)workspace;
    (void)workspace_bytes;  // no split-K: an element's reduction order never depends on the launch
    int rc = cb_check(h_desc, "sf_conv_fwd_bf16");
    if (rc) return rc;
    const sf_conv_desc &d = *h_desc;
    SF_REQUIRE(in && w && bias && out, "sf_conv_fwd_bf16: NULL operand");
    if (index != nullptr) {
        snprintf(sf_err_buf, sizeof(sf_err_buf), "sf_conv_fwd_bf16: index addressing is not served (dense samples only)");
        return SF_ERR_UNSUPPORTED;
    }
    SF_REQUIRE(n >= 0 && offset >= 0, "sf_conv_fwd_bf16: n=%lld offset=%lld", (long long)n, (long long)offset);
    SF_REQUIRE(in_sample_stride >= (int64_t)d.Cin * d.H * d.W && (in_sample_stride & 3) == 0,
               "sf_conv_fwd_bf16: in_sample_stride %lld (at least Cin*H*W, a multiple of 4)", (long long)in_sample_stride);
    SF_REQUIRE(aligned16(in) && aligned16(w) && aligned16(out), "sf_conv_fwd_bf16: in, w and out must be 16-byte aligned");
    const CbGeo g = cb_geo(d);
    CbTile t;
    if (!cb_tile(g, false, n, &t)) return cb_too_wide(d, "sf_conv_fwd_bf16");
    if (n == 0) return SF_OK;
    const int64_t groups = ((n + t.S - 1) / t.S) * t.nrt;
    SF_REQUIRE(groups <= 0x7fffffffLL, "sf_conv_fwd_bf16: %lld work-groups", (long long)groups);
    cb_launch<false>(d.Cout, dim3((unsigned)groups), (size_t)t.S * t.LH * t.LW * t.cs * 2, STREAM(stream), (const float *)in, w,
                     bias, nullptr, out, d.relu, n, in_sample_stride, offset, g, t);
    return sf_launch_status("sf_conv_fwd_bf16");
}

extern "C" int sf_conv_dgrad_bf16(const float *dout, const float *w, const float *in_act, float *din, int64_t n,
                                  const sf_conv_desc *h_desc, void *stream) {
    int rc = cb_check(h_desc, "sf_conv_dgrad_bf16");
    if (rc) return rc;
    const sf_conv_desc &d = *h_desc;
    SF_REQUIRE(dout && w && din, "sf_conv_dgrad_bf16: NULL operand");
    SF_REQUIRE(!d.relu || in_act, "sf_conv_dgrad_bf16: relu=%d needs the stored input activation", d.relu);
    SF_REQUIRE(n >= 0, "sf_conv_dgrad_bf16: n=%lld", (long long)n);
    SF_REQUIRE(aligned16(w) && aligned16(dout), "sf_conv_dgrad_bf16: dout and w must be 16-byte aligned");
    const CbGeo g = cb_geo(d);
    CbTile t;
    if (!cb_tile(g, true, n, &t)) return cb_too_wide(d, "sf_conv_dgrad_bf16");
    if (n == 0) return SF_OK;
    const int64_t groups = ((n + t.S - 1) / t.S) * t.nrt;
    SF_REQUIRE(groups <= 0x7fffffffLL, "sf_conv_dgrad_bf16: %lld work-groups", (long long)groups);
    cb_launch<true>(d.Cin, dim3((unsigned)groups), (size_t)t.S * t.LH * t.LW * t.cs * 2, STREAM(stream), dout, w, nullptr,
                    d.relu ? in_act : nullptr, din, d.relu, n, (int64_t)d.OH * d.OW * d.Cout, 0, g, t);
    return sf_launch_status("sf_conv_dgrad_bf16");
}

extern "C" int64_t sf_conv_wgrad_bf16_workspace(int64_t n, const sf_conv_desc *h_desc) {
    if (n < 0 || !cb_served(h_desc)) return 0;
    const CbBand t = cb_band(*h_desc, n);
    return t.parts * ((int64_t)h_desc->KH * h_desc->KW * h_desc->Cin * h_desc->Cout + h_desc->Cout) * (int64_t)sizeof(float);
}

extern "C" int sf_conv_wgrad_bf16(const void *in, int64_t in_sample_stride, const int32_t *index, int64_t offset,
                                  const float *dout, float *dw, float *db, int64_t n, const sf_conv_desc *h_desc,
                                  void *workspace, int64_t workspace_bytes, void *stream) {
    int rc = cb_check(h_desc, "sf_conv_wgrad_bf16");
    if (rc) return rc;
    const sf_conv_desc &d = *h_desc;
    SF_REQUIRE(in && dout && dw && db, "sf_conv_wgrad_bf16: NULL operand");
    if (index != nullptr) {
        snprintf(sf_err_buf, sizeof(sf_err_buf), "sf_conv_wgrad_bf16: index addressing is not served (dense samples only)");
        return SF_ERR_UNSUPPORTED;
    }
    SF_REQUIRE(n >= 0 && offset >= 0, "sf_conv_wgrad_bf16: n=%lld offset=%lld", (long long)n, (long long)offset);
    SF_REQUIRE(in_sample_stride >= (int64_t)d.Cin * d.H * d.W && (in_sample_stride & 3) == 0,
               "sf_conv_wgrad_bf16: in_sample_stride %lld (at least Cin*H*W, a multiple of 4)", (long long)in_sample_stride);
    SF_REQUIRE(aligned16(in) && aligned16(dout) && aligned16(workspace),
               "sf_conv_wgrad_bf16: in, dout and workspace must be 16-byte aligned");
    const CbBand t = cb_band(d, n);
    const int KC = d.KH * d.KW * d.Cin * d.Cout;
    const int64_t need = t.parts * (KC + d.Cout) * (int64_t)sizeof(float);
    SF_REQUIRE(workspace && workspace_bytes >= need, "sf_conv_wgrad_bf16: workspace %lld bytes < %lld",
               (long long)workspace_bytes, (long long)need);
    hipStream_t s = STREAM(stream);
    float *part = static_cast<float *>(workspace);
    const dim3 grid((unsigned)t.parts, (unsigned)t.blocks);
    const float *x = static_cast<const float *>(in);
    if (d.KH == 4) cb_wgrad_launch<4, 2>(d.Cout, grid, (size_t)t.lds_bytes, s, x, dout, part, in_sample_stride, offset, d, t);
    else if (d.stride == 1) cb_wgrad_launch<3, 1>(d.Cout, grid, (size_t)t.lds_bytes, s, x, dout, part, in_sample_stride, offset, d, t);
    else cb_wgrad_launch<3, 2>(d.Cout, grid, (size_t)t.lds_bytes, s, x, dout, part, in_sample_stride, offset, d, t);
    rc = sf_launch_status("sf_conv_wgrad_bf16 (partials)");
    if (rc) return rc;
    return sf_res_wgrad_sum_launch(part, (int)t.parts, KC, d.Cout, dw, db, s);
}
