// sf_resnet_bf16.hip — the 3x3 / stride 1 / pad 1 conv family of the resnet_impala encoder on v_mfma_f32_16x16x32_bf16, for
// f32 NHWC layers with Cin, Cout in {32, 64, 128} (every pair): cfg.encoder_resnet_bf16.  Reached by name only
// (sf_res_conv_*_bf16); the plain entry points never route here.  The same entry points hand the pairs 16 -> 16 and
// 16 -> 32 to sf_resnet_bf16_c16.hip (kernels built for 16 channels, the same arithmetic); any other pair with a 16 is refused.
//
// Arithmetic: both MFMA operands are rounded to bf16 (round to nearest even, v_cvt_pk_bf16_f32) once per element, the input
// after its activation: bf16(act_in(x)), bf16(w), bf16(dout).  Accumulation is fp32 and everything outside the matrix
// product stays fp32 in the fp32 family's order: bias, residual, out, act_out copy; data gradient * act'(pre) on the
// unrounded pre, then g_add +.  Activations, gradients and the weights [9*Cin, Cout] stay fp32 in memory: the weights are
// converted inside the launch, on their way into the B registers, and no bf16 copy outlives a launch.
//
// Forward and data gradient are ONE kernel (k_res_conv_bf16): an implicit GEMM with M = output pixels, N = the produced
// channels, K = 9 taps x the reduced channels Cr, 32 k per MFMA.
//   * A work-group (4 waves) takes a tile of S samples x TH rows x TW columns (<= 128 pixels = 8 M fragments) and stages its
//     halo in LDS once as bf16, activated and rounded, exact zeros outside the image.  A pixel's channels are contiguous,
//     the pixel stride is Cr + 8 bf16 = an odd number of 16-byte words.
//   * A wave owns TWO 16-column slices of N and FW = 8 / MW of the M fragments: one ds_read_b128 (lane = pixel l % 16,
//     channels 8*(l/16) .. +7 of the 32-channel chunk) feeds two MFMAs, which halves the LDS traffic per MFMA against one
//     slice per wave.  (slice pairs, MW) = (1, 4), (2, 2), (4, 1) for N = 32, 64, 128.
//   * The weights stream from global memory (L2) as fp32, one (tap, chunk) ahead of the MFMAs, and are rounded when the
//     buffers swap.  Forward: B[k][n] = W[k, n], 8 dwords down the lane's column; data gradient: the mirrored-tap transpose
//     of the same block, B[o][c] = W[(8 - tap)*Cin + c][o], two float4 along o.
//   * An output element's reduction order is (tap, chunk, the MFMA's own k order): it depends on neither the batch size nor
//     the sample's place in the tile.
//
// The weight gradient (k_res_wgrad_bf16) reduces over pixels: M = 16 input channels, N = 16 output channels, K = pixels, 32
// per MFMA as four runs of 8 consecutive pixels of a row (one run per lane group).  A lane's operand is 8 consecutive pixels
// of ONE channel, so both bands are staged channel-major, rows padded with zeros to a multiple of 8 pixels.  The three
// column taps shift the input run by one 2-byte element, which a 16-byte LDS read cannot follow: the input halo is staged
// as three column-shifted copies (copy kw, run j = columns 8j + kw - 1 .. + 7), so every tap is one aligned ds_read_b128;
// the alternative, two reads and a funnel shift per tap, doubles the LDS reads of the loop that is bound by them, while
// the copies cost LDS space and writes that happen once per band.  Grid = pixel parts x Cin blocks; partials go to
// [parts][9*Cin*Cout + Cout] and k_res_conv_wgrad_sum (sf_resnet.hip) adds them in part order: no float atomics.  The bias
// gradient is one more MFMA against ones: the sum of the rounded dout.
//
// Compiled with -ffp-contract=off like sf_resnet_mfma.hip: the epilogues round after each op.
#include "sf_common.h"
#include "sf_resnet_shared.h"
#include "sf_bf16.h"

#define STREAM(s) reinterpret_cast<hipStream_t>(s)

namespace {

constexpr int RB_FRAGS = 8;                // M fragments of a forward / data-gradient tile
constexpr int RB_TILE_M = 16 * RB_FRAGS;   // ... = 128 output pixels
constexpr int RB_LDS_BUDGET = 64 * 1024;   // dynamic LDS of one work-group: two of them per CU
constexpr int RB_BAND_PIX = 256;           // pixels (padded columns counted) a weight-gradient band aims at
constexpr int RB_MIN_PARTS = 64;
constexpr int RB_GRID_TARGET = 1024;       // work-groups the weight gradient aims at: parts x Cin blocks

extern __shared__ float4 rb_lds4[];

inline bool rb_width(int c) { return c == 32 || c == 64 || c == 128; }
// a 16 on the input side goes to sf_resnet_bf16_c16.hip; any other pair with a 16 is refused
inline bool rb_served(int cin, int cout) { return (rb_width(cin) && rb_width(cout)) || sf_res_c16_pair(cin, cout); }

__device__ __forceinline__ float4 rb_act4(int act, const float4 &v) {
    return make_float4(act_fwd(act, v.x), act_fwd(act, v.y), act_fwd(act, v.z), act_fwd(act, v.w));
}

// ------------------------------------------------------------------------------------------------ forward / dgrad
struct RbTile {
    int S, TH, TW, nrt, nct;  // samples, rows, columns of a tile; row / column tiles of an image
    int cs;                   // bf16 elements per halo pixel: Cr + 8 (an odd number of 16-byte words: 16 pixels cover all banks)
};

int64_t rb_tile_bytes(const RbTile &t, int S, int TH) { return (int64_t)S * (TH + 2) * (t.TW + 2) * t.cs * 2; }

RbTile rb_tile(int H, int W, int Cr, int64_t n) {
    RbTile t;
    t.cs = Cr + 8;
    t.nct = (W + 31) / 32;
    t.TW = (W + t.nct - 1) / t.nct;
    int TH = std::max(1, std::min(H, RB_TILE_M / t.TW));
    while (TH > 1 && rb_tile_bytes(t, 1, TH) > RB_LDS_BUDGET) --TH;  // 128 pixels of 32 columns: 6 * 34 * 136 * 2 = 55 488 bytes
    t.nrt = (H + TH - 1) / TH;
    t.TH = (H + t.nrt - 1) / t.nrt;
    t.S = 1;
    if (t.nrt == 1 && t.nct == 1)
        while (t.S < n && (t.S + 1) * H * W <= RB_TILE_M && rb_tile_bytes(t, t.S + 1, t.TH) <= RB_LDS_BUDGET) ++t.S;
    return t;
}

// NP: pairs of 16-column slices of the produced channels Cn = 32 * NP; MW: waves that share a pair and split the M fragments.
// DGRAD = false: in = x [n,H,W,Cr] (strided samples), act_in on load, a1 = residual, out_act / act_out as sf_res_conv_fwd.
// DGRAD = true:  in = dout [n,H,W,Cr] dense, act = the activation whose derivative at a1 = pre multiplies, a2 = g_add.
template <int NP, int MW, bool DGRAD>
__global__ __launch_bounds__(256) void k_res_conv_bf16(const float *__restrict__ in, const float *__restrict__ w,
                                                       const float *__restrict__ bias, const float *__restrict__ a1,
                                                       const float *__restrict__ a2, float *__restrict__ out,
                                                       float *__restrict__ out_act, int act, int act_out, int64_t n,
                                                       int64_t in_stride, int64_t in_offset, int H, int W, int Cr, RbTile t) {
    static_assert(NP * MW == 4, "four waves");
    constexpr int Cn = 32 * NP, FW = RB_FRAGS / MW;
    __bf16 *lds = reinterpret_cast<__bf16 *>(rb_lds4);
    const int TH = t.TH, TW = t.TW, HW2 = TW + 2, HP = (TH + 2) * HW2, cs = t.cs;
    const int ct = blockIdx.x % t.nct, rt = (blockIdx.x / t.nct) % t.nrt;
    const int64_t s0 = (int64_t)(blockIdx.x / (t.nct * t.nrt)) * t.S;
    const int ns = (int)min((int64_t)t.S, n - s0), h0 = rt * TH, w0 = ct * TW;
    // ---- halo band -> LDS as bf16(act(x)); everything outside the image (or past the last sample) is an exact zero
    const int q8 = Cr >> 3;
    for (int i = threadIdx.x; i < t.S * HP * q8; i += 256) {
        const int q = i % q8, hp = i / q8, s = hp / HP, rr = (hp - s * HP) / HW2, cc = hp - s * HP - rr * HW2;
        const int h = h0 + rr - 1, ww = w0 + cc - 1;
        float4 v0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), v1 = v0;
        if (s < ns && h >= 0 && h < H && ww >= 0 && ww < W) {
            const float4 *p = reinterpret_cast<const float4 *>(in + (in_offset + s0 + s) * in_stride + ((int64_t)h * W + ww) * Cr + 8 * q);
            v0 = p[0];
            v1 = p[1];
            if (!DGRAD && act) { v0 = rb_act4(act, v0); v1 = rb_act4(act, v1); }
        }
        *reinterpret_cast<bf16x8 *>(lds + hp * cs + 8 * q) = bf16_pack(v0, v1);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, pair = wave % NP, f0 = (wave / NP) * FW;
    const int lr = lane & 15, lg = lane >> 4;
    const int M = t.S * TH * TW, nfr = (M + 15) >> 4;
    int hb[FW];  // LDS offset of the lane's pixel at tap (0, 0), its channel group added
    floatx4 acc[FW][2];
#pragma unroll
    for (int f = 0; f < FW; ++f) {
        int m = (f0 + f) * 16 + lr;
        if (m >= M) m = 0;  // a lane past the tile reads a real pixel; its rows are never stored
        const int s = m / (TH * TW), r = (m / TW) % TH, c = m % TW;
        hb[f] = ((s * (TH + 2) + r) * HW2 + c) * cs + 8 * lg;
        acc[f][0] = acc[f][1] = (floatx4){0.0f, 0.0f, 0.0f, 0.0f};
    }
    const int nch = Cr >> 5, steps = 9 * nch;
    // fp32 B operands of step (tap, 32-channel chunk): lane (column lr of slice u, group lg) holds k-rows 8*lg .. + 7
    float4 braw[2][2];
    auto load_b = [&](int tap, int ch) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int col = (pair * 2 + u) * 16 + lr;
            if (DGRAD) {  // B[o][c] = W[(8 - tap)*Cn + c][o]: the lane's row c, eight consecutive o
                const float4 *p = reinterpret_cast<const float4 *>(w + ((int64_t)(8 - tap) * Cn + col) * Cr + ch * 32 + 8 * lg);
                braw[u][0] = p[0];
                braw[u][1] = p[1];
            } else {
                const float *p = w + ((int64_t)(tap * Cr + ch * 32 + 8 * lg)) * Cn + col;
                braw[u][0] = make_float4(p[0], p[Cn], p[2 * Cn], p[3 * Cn]);
                braw[u][1] = make_float4(p[4 * Cn], p[5 * Cn], p[6 * Cn], p[7 * Cn]);
            }
        }
    };
    load_b(0, 0);
    int tap = 0, ch = 0;
    for (int it = 0; it < steps; ++it) {
        const bf16x8 b0 = bf16_pack(braw[0][0], braw[0][1]), b1 = bf16_pack(braw[1][0], braw[1][1]);
        const int aoff = ((tap / 3) * HW2 + tap % 3) * cs + ch * 32;
        if (++ch == nch) { ch = 0; ++tap; }
        if (it + 1 < steps) load_b(tap, ch);
#pragma unroll
        for (int f = 0; f < FW; ++f) {
            if (f0 + f < nfr) {
                const bf16x8 a = *reinterpret_cast<const bf16x8 *>(lds + hb[f] + aoff);
                acc[f][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b0, acc[f][0], 0, 0, 0);
                acc[f][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b1, acc[f][1], 0, 0, 0);
            }
        }
    }
    // ---- epilogue: accumulator j of fragment f, slice u is pixel 16*f + 4*lg + j, channel (2*pair + u)*16 + lr
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int o = (pair * 2 + u) * 16 + lr;
        const float bo = DGRAD ? 0.0f : bias[o];
#pragma unroll
        for (int f = 0; f < FW; ++f) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int m = (f0 + f) * 16 + 4 * lg + j;
                const int s = m / (TH * TW), r = (m / TW) % TH, c = m % TW;
                if (m >= M || s >= ns || h0 + r >= H || w0 + c >= W) continue;
                const int64_t idx = (((s0 + s) * H + h0 + r) * W + w0 + c) * Cn + o;
                float v = acc[f][u][j];
                if (DGRAD) {
                    if (act) v = v * act_grad(act, a1[idx]);
                    if (a2) v = a2[idx] + v;
                    out[idx] = v;
                } else {
                    v = v + bo;
                    if (a1) v = a1[idx] + v;
                    out[idx] = v;
                    if (out_act) out_act[idx] = act_fwd(act_out, v);
                }
            }
        }
    }
}

template <bool DGRAD>
void rb_launch(int Cn, dim3 grid, size_t lds, hipStream_t s, const float *in, const float *w, const float *bias,
               const float *a1, const float *a2, float *out, float *out_act, int act, int act_out, int64_t n,
               int64_t in_stride, int64_t in_offset, int H, int W, int Cr, const RbTile &t) {
#define RB_GO(NP, MW)                                                                                                  \
    hipLaunchKernelGGL((k_res_conv_bf16<NP, MW, DGRAD>), grid, dim3(256), lds, s, in, w, bias, a1, a2, out, out_act,    \
                       act, act_out, n, in_stride, in_offset, H, W, Cr, t)
    if (Cn == 32) RB_GO(1, 4);
    else if (Cn == 64) RB_GO(2, 2);
    else RB_GO(4, 1);
#undef RB_GO
}

// ------------------------------------------------------------------------------------------------ weight gradient
struct RbBand {
    int S, TH, nrt;    // samples and whole rows of a band; bands per image
    int WP8, RW;       // columns of a row padded to a multiple of 8; runs of 8 pixels per row
    int ciw, CW;       // 16-channel Cin tiles of a work-group, and their channels
    int csa, csg;      // bf16 elements per channel of one halo copy / of the dout band: an odd number of 16-byte words, so
                       // that the 16 channels a lane group reads fall on 16 different words modulo 16
    int blocks;        // Cin blocks = grid.y
    int64_t NB, bpp, parts;  // bands in the batch, bands per part, parts = grid.x
    int64_t lds_bytes;
};

// false: a single row of this layer does not fit the LDS budget
bool rb_band(int H, int W, int Cin, int Cout, int64_t n, RbBand *out) {
    RbBand t;
    const int ncog = std::min(Cout / 16, 4);
    t.ciw = std::min(Cin / 16, 4 / ncog);
    t.CW = 16 * t.ciw;
    t.blocks = (Cin / 16) / t.ciw;
    t.WP8 = (W + 7) & ~7;
    t.RW = t.WP8 >> 3;
    auto bytes = [&](int S, int TH) {
        return 2 * ((int64_t)3 * t.CW * odd8(S * (TH + 2) * t.WP8) + (int64_t)Cout * odd8(S * TH * t.WP8));
    };
    int TH = std::max(1, std::min(H, RB_BAND_PIX / t.WP8));
    while (TH > 1 && bytes(1, TH) > RB_LDS_BUDGET) --TH;
    if (bytes(1, TH) > RB_LDS_BUDGET) return false;
    t.nrt = (H + TH - 1) / TH;
    t.TH = (H + t.nrt - 1) / t.nrt;
    t.S = 1;
    if (t.nrt == 1)
        while (t.S < n && (t.S + 1) * H * t.WP8 <= RB_BAND_PIX && bytes(t.S + 1, t.TH) <= RB_LDS_BUDGET) ++t.S;
    t.csa = odd8(t.S * (t.TH + 2) * t.WP8);
    t.csg = odd8(t.S * t.TH * t.WP8);
    t.lds_bytes = bytes(t.S, t.TH);
    t.NB = ((n + t.S - 1) / t.S) * t.nrt;
    const int64_t target = std::max(RB_MIN_PARTS, RB_GRID_TARGET / t.blocks);
    t.bpp = std::max<int64_t>(1, (t.NB + target - 1) / target);
    t.parts = std::max<int64_t>(1, (t.NB + t.bpp - 1) / t.bpp);
    *out = t;
    return true;
}

// NCOG x CT 16-column tiles of Cout: wave (cit, cog) owns Cin tile cit of the block and Cout tiles cog*CT .. +CT-1
template <int NCOG, int CT>
__global__ __launch_bounds__(256) void k_res_wgrad_bf16(const float *__restrict__ x, const float *__restrict__ gy,
                                                        float *__restrict__ part, int act, int64_t n, int64_t in_stride,
                                                        int64_t in_offset, int H, int W, int Cin, RbBand t) {
    constexpr int Cout = 16 * NCOG * CT;
    __bf16 *la = reinterpret_cast<__bf16 *>(rb_lds4);
    const int TH = t.TH, WP8 = t.WP8, RW = t.RW, CW = t.CW, csa = t.csa, csg = t.csg;
    __bf16 *lgy = la + 3 * CW * csa;
    const int nthr = blockDim.x, cbase = blockIdx.y * CW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, cog = wave % NCOG, cit = wave / NCOG;
    const int lr = lane & 15, lg = lane >> 4;
    const bool do_bias = blockIdx.y == 0 && cit == 0;
    floatx4 acc[9][CT], accb[CT];
#pragma unroll
    for (int u = 0; u < CT; ++u) {
        accb[u] = (floatx4){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) acc[tap][u] = (floatx4){0.0f, 0.0f, 0.0f, 0.0f};
    }
    const bf16x8 ones8 = bf16_ones8();
    bf16x8 zero8;
#pragma unroll
    for (int k = 0; k < 8; ++k) zero8[k] = (__bf16)0.0f;
    const int64_t b0 = (int64_t)blockIdx.x * t.bpp, b1 = min(t.NB, b0 + t.bpp);
    const int qa = CW >> 2, qg = Cout >> 2;
    const __bf16 *xa = la + (cit * 16 + lr) * csa, *ga = lgy + (cog * CT * 16 + lr) * csg;
    for (int64_t band = b0; band < b1; ++band) {
        const int64_t s0 = (band / t.nrt) * t.S;
        const int ns = (int)min((int64_t)t.S, n - s0), h0 = (int)(band % t.nrt) * TH;
        __syncthreads();  // the previous band's fragments have been read
        // ---- input halo, channel-major, three column-shifted copies: copy kw, run j = columns 8j + kw - 1 .. + 7
        for (int i = threadIdx.x; i < t.S * (TH + 2) * RW * qa; i += nthr) {
            const int q = i % qa, rest = i / qa, j = rest % RW, hp = rest / RW, s = hp / (TH + 2), rr = hp - s * (TH + 2);
            const int h = h0 + rr - 1;
            __bf16 v[10][4];
#pragma unroll
            for (int e = 0; e < 10; ++e) {
                const int col = 8 * j - 1 + e;
                float4 f = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (s < ns && h >= 0 && h < H && col >= 0 && col < W) {
                    f = *reinterpret_cast<const float4 *>(x + (in_offset + s0 + s) * in_stride + ((int64_t)h * W + col) * Cin + cbase + 4 * q);
                    if (act) f = rb_act4(act, f);
                }
                v[e][0] = (__bf16)f.x; v[e][1] = (__bf16)f.y; v[e][2] = (__bf16)f.z; v[e][3] = (__bf16)f.w;
            }
#pragma unroll
            for (int kw = 0; kw < 3; ++kw)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    bf16x8 o;
#pragma unroll
                    for (int k = 0; k < 8; ++k) o[k] = v[kw + k][c];
                    *reinterpret_cast<bf16x8 *>(la + (kw * CW + 4 * q + c) * csa + hp * WP8 + 8 * j) = o;
                }
        }
        // ---- dout band, channel-major; padding columns, rows past the image and samples past the batch are zeros
        for (int i = threadIdx.x; i < t.S * TH * RW * qg; i += nthr) {
            const int q = i % qg, rest = i / qg, j = rest % RW, gp = rest / RW, s = gp / TH, r = gp - s * TH;
            __bf16 v[8][4];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int col = 8 * j + e;
                float4 f = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (s < ns && h0 + r < H && col < W)
                    f = *reinterpret_cast<const float4 *>(gy + (((s0 + s) * H + h0 + r) * W + col) * Cout + 4 * q);
                v[e][0] = (__bf16)f.x; v[e][1] = (__bf16)f.y; v[e][2] = (__bf16)f.z; v[e][3] = (__bf16)f.w;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                bf16x8 o;
#pragma unroll
                for (int k = 0; k < 8; ++k) o[k] = v[k][c];
                *reinterpret_cast<bf16x8 *>(lgy + (4 * q + c) * csg + gp * WP8 + 8 * j) = o;
            }
        }
        __syncthreads();
        // ---- 32 pixels per MFMA: lane group lg takes run 4*it + lg of the band's ns * TH * RW runs, (sample, row, run) order
        const int NR = ns * TH * RW;
        int rho = lg, s = lg / (TH * RW), r = (lg / RW) % TH, j = lg % RW;
        for (int it = 0; 4 * it < NR; ++it) {
            const bool live = rho < NR;  // past the band: a zero dout run against any finite input run
            const int gofs = live ? (s * TH + r) * WP8 + 8 * j : 0, aofs = live ? (s * (TH + 2) + r) * WP8 + 8 * j : 0;
            bf16x8 b[CT];
#pragma unroll
            for (int u = 0; u < CT; ++u) b[u] = live ? *reinterpret_cast<const bf16x8 *>(ga + u * 16 * csg + gofs) : zero8;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const bf16x8 a = *reinterpret_cast<const bf16x8 *>(xa + (tap % 3) * CW * csa + aofs + (tap / 3) * WP8);
#pragma unroll
                for (int u = 0; u < CT; ++u) acc[tap][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[u], acc[tap][u], 0, 0, 0);
            }
            if (do_bias) {
#pragma unroll
                for (int u = 0; u < CT; ++u) accb[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones8, b[u], accb[u], 0, 0, 0);
            }
            rho += 4;
            j += 4;
            while (j >= RW) { j -= RW; ++r; }
            while (r >= TH) { r -= TH; ++s; }
        }
    }
    // accumulator j: input channel 4*lg + j of the wave's Cin tile, output channel lr of Cout tile u
    const int KC = 9 * Cin * Cout;
    float *pp = part + (int64_t)blockIdx.x * (KC + Cout);
#pragma unroll
    for (int u = 0; u < CT; ++u) {
        const int o = (cog * CT + u) * 16 + lr;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int j = 0; j < 4; ++j) pp[(tap * Cin + cbase + cit * 16 + 4 * lg + j) * Cout + o] = acc[tap][u][j];
        if (do_bias && lg == 0) pp[KC + o] = accb[u][0];
    }
}

int rb_check(const sf_res_desc *d, const char *what) {
    SF_REQUIRE(d != nullptr, "%s: desc is NULL", what);
    SF_REQUIRE(d->H >= 1 && d->W >= 1, "%s: bad geometry H=%d W=%d", what, d->H, d->W);
    SF_REQUIRE(d->act_in >= 0 && d->act_in <= 3, "%s: act_in=%d not in 0..3", what, d->act_in);
    if (d->in_u8 || d->traj_T != 0 || !rb_served(d->Cin, d->Cout)) {
        snprintf(sf_err_buf, sizeof(sf_err_buf),
                 "%s: Cin=%d Cout=%d in_u8=%d traj_T=%d (the bf16 family serves dense f32 NHWC layers with Cin and Cout in "
                 "{32, 64, 128}, and the pairs 16 -> 16 and 16 -> 32)", what, d->Cin, d->Cout, d->in_u8, d->traj_T);
        return SF_ERR_UNSUPPORTED;
    }
    return SF_OK;
}

}  // namespace

extern "C" int sf_res_conv_fwd_bf16(const void *in, int64_t in_sample_stride, const int32_t *index, int64_t offset,
                                    const float *w, const float *bias, const float *residual, float *out, float *out_act,
                                    int act_out, int64_t n, const sf_res_desc *h_desc, void *stream) {
    int rc = rb_check(h_desc, "sf_res_conv_fwd_bf16");
    if (rc) return rc;
    const sf_res_desc &d = *h_desc;
    SF_REQUIRE(in && w && bias && out, "sf_res_conv_fwd_bf16: NULL operand");
    SF_REQUIRE(index == nullptr, "sf_res_conv_fwd_bf16: index addressing is for the raw u8 frames only");
    SF_REQUIRE(n >= 0 && offset >= 0, "sf_res_conv_fwd_bf16: n=%lld offset=%lld", (long long)n, (long long)offset);
    SF_REQUIRE(act_out >= 0 && act_out <= 3, "sf_res_conv_fwd_bf16: act_out=%d", act_out);
    SF_REQUIRE(in_sample_stride >= (int64_t)d.Cin * d.H * d.W && (in_sample_stride & 3) == 0,
               "sf_res_conv_fwd_bf16: in_sample_stride %lld (at least Cin*H*W, a multiple of 4)", (long long)in_sample_stride);
    SF_REQUIRE(aligned16(in) && aligned16(w) && aligned16(out) && (!out_act || aligned16(out_act)) &&
                   (!residual || aligned16(residual)),
               "sf_res_conv_fwd_bf16: in, w, out, out_act and residual must be 16-byte aligned");
    if (n == 0) return SF_OK;
    if (sf_res_c16_pair(d.Cin, d.Cout))
        return sf_res_c16_conv_launch(false, (const float *)in, in_sample_stride, offset, w, bias, residual, nullptr, out, out_act,
                                      d.act_in, act_out, n, d.H, d.W, d.Cin, d.Cout, STREAM(stream));
    const RbTile t = rb_tile(d.H, d.W, d.Cin, n);
    const int64_t groups = ((n + t.S - 1) / t.S) * t.nrt * t.nct;
    SF_REQUIRE(groups <= 0x7fffffffLL, "sf_res_conv_fwd_bf16: %lld work-groups", (long long)groups);
    rb_launch<false>(d.Cout, dim3((unsigned)groups), (size_t)rb_tile_bytes(t, t.S, t.TH), STREAM(stream), (const float *)in, w,
                     bias, residual, nullptr, out, out_act, d.act_in, act_out, n, in_sample_stride, offset, d.H, d.W, d.Cin, t);
    return sf_launch_status("sf_res_conv_fwd_bf16");
}

extern "C" int sf_res_conv_dgrad_bf16(const float *dout, const float *w, const float *pre, const float *g_add, float *din,
                                      int64_t n, const sf_res_desc *h_desc, void *stream) {
    int rc = rb_check(h_desc, "sf_res_conv_dgrad_bf16");
    if (rc) return rc;
    const sf_res_desc &d = *h_desc;
    SF_REQUIRE(dout && w && din, "sf_res_conv_dgrad_bf16: NULL operand");
    SF_REQUIRE(!d.act_in || pre, "sf_res_conv_dgrad_bf16: act_in=%d needs the pre-activation input", d.act_in);
    SF_REQUIRE(n >= 0, "sf_res_conv_dgrad_bf16: n=%lld", (long long)n);
    SF_REQUIRE(aligned16(w) && aligned16(dout), "sf_res_conv_dgrad_bf16: w and dout must be 16-byte aligned");
    if (n == 0) return SF_OK;
    if (sf_res_c16_pair(d.Cin, d.Cout))
        return sf_res_c16_conv_launch(true, dout, (int64_t)d.H * d.W * d.Cout, 0, w, nullptr, pre, g_add, din, nullptr, d.act_in, 0,
                                      n, d.H, d.W, d.Cout, d.Cin, STREAM(stream));
    const RbTile t = rb_tile(d.H, d.W, d.Cout, n);
    const int64_t groups = ((n + t.S - 1) / t.S) * t.nrt * t.nct;
    SF_REQUIRE(groups <= 0x7fffffffLL, "sf_res_conv_dgrad_bf16: %lld work-groups", (long long)groups);
    rb_launch<true>(d.Cin, dim3((unsigned)groups), (size_t)rb_tile_bytes(t, t.S, t.TH), STREAM(stream), dout, w, nullptr, pre,
                    g_add, din, nullptr, d.act_in, 0, n, (int64_t)d.H * d.W * d.Cout, 0, d.H, d.W, d.Cout, t);
    return sf_launch_status("sf_res_conv_dgrad_bf16");
}

extern "C" int64_t sf_res_conv_wgrad_bf16_workspace(int64_t n, const sf_res_desc *h_desc) {
    if (!h_desc || n < 0 || h_desc->in_u8 || h_desc->traj_T != 0 || !rb_served(h_desc->Cin, h_desc->Cout) ||
        h_desc->H < 1 || h_desc->W < 1)
        return 0;
    if (sf_res_c16_pair(h_desc->Cin, h_desc->Cout))
        return sf_res_c16_wgrad_parts(h_desc->H, h_desc->W, h_desc->Cout, n) * (9LL * 16 * h_desc->Cout + h_desc->Cout) *
               (int64_t)sizeof(float);
    RbBand t;
    if (!rb_band(h_desc->H, h_desc->W, h_desc->Cin, h_desc->Cout, n, &t)) return 0;
    return t.parts * (9LL * h_desc->Cin * h_desc->Cout + h_desc->Cout) * (int64_t)sizeof(float);
}

extern "C" int sf_res_conv_wgrad_bf16(const void *in, int64_t in_sample_stride, const int32_t *index, int64_t offset,
                                      const float *dout, float *dw, float *db, int64_t n, const sf_res_desc *h_desc,
                                      void *workspace, int64_t workspace_bytes, void *stream) {
    int rc = rb_check(h_desc, "sf_res_conv_wgrad_bf16");
    if (rc) return rc;
    const sf_res_desc &d = *h_desc;
    SF_REQUIRE(in && dout && dw && db, "sf_res_conv_wgrad_bf16: NULL operand");
    SF_REQUIRE(index == nullptr, "sf_res_conv_wgrad_bf16: index addressing is for the raw u8 frames only");
    SF_REQUIRE(n >= 0 && offset >= 0, "sf_res_conv_wgrad_bf16: n=%lld offset=%lld", (long long)n, (long long)offset);
    SF_REQUIRE(in_sample_stride >= (int64_t)d.Cin * d.H * d.W && (in_sample_stride & 3) == 0,
               "sf_res_conv_wgrad_bf16: in_sample_stride %lld (at least Cin*H*W, a multiple of 4)", (long long)in_sample_stride);
    SF_REQUIRE(aligned16(in) && aligned16(dout), "sf_res_conv_wgrad_bf16: in and dout must be 16-byte aligned");
    if (sf_res_c16_pair(d.Cin, d.Cout)) {
        const int KC = 9 * d.Cin * d.Cout;
        const int64_t parts = sf_res_c16_wgrad_parts(d.H, d.W, d.Cout, n), need = parts * (KC + d.Cout) * (int64_t)sizeof(float);
        SF_REQUIRE(parts == 0 || (workspace && workspace_bytes >= need), "sf_res_conv_wgrad_bf16: workspace %lld bytes < %lld",
                   (long long)workspace_bytes, (long long)need);
        rc = sf_res_c16_wgrad_launch((const float *)in, in_sample_stride, offset, dout, static_cast<float *>(workspace), d.act_in,
                                     n, d.H, d.W, d.Cout, STREAM(stream));  // parts == 0: refuses, the row does not fit
        if (rc) return rc;
        return sf_res_wgrad_sum_launch(static_cast<const float *>(workspace), (int)parts, KC, d.Cout, dw, db, STREAM(stream));
    }
    RbBand t;
    if (!rb_band(d.H, d.W, d.Cin, d.Cout, n, &t)) {
        snprintf(sf_err_buf, sizeof(sf_err_buf), "sf_res_conv_wgrad_bf16: a row of W=%d pixels x (Cin=%d, Cout=%d) exceeds the "
                 "%d-byte LDS band", d.W, d.Cin, d.Cout, RB_LDS_BUDGET);
        return SF_ERR_UNSUPPORTED;
    }
    const int KC = 9 * d.Cin * d.Cout, E = KC + d.Cout;
    const int64_t need = t.parts * E * (int64_t)sizeof(float);
    SF_REQUIRE(workspace && workspace_bytes >= need, "sf_res_conv_wgrad_bf16: workspace %lld bytes < %lld",
               (long long)workspace_bytes, (long long)need);
    hipStream_t s = STREAM(stream);
    float *part = static_cast<float *>(workspace);
    const dim3 grid((unsigned)t.parts, (unsigned)t.blocks);
    const int ncog = d.Cout >= 64 ? 4 : d.Cout / 16;
    const dim3 block((unsigned)(t.ciw * ncog * 64));
#define RB_WGO(NCOG, CT)                                                                                                \
    hipLaunchKernelGGL((k_res_wgrad_bf16<NCOG, CT>), grid, block, (size_t)t.lds_bytes, s, (const float *)in, dout, part,  \
                       d.act_in, n, in_sample_stride, offset, d.H, d.W, d.Cin, t)
    if (d.Cout == 32) RB_WGO(2, 1);
    else if (d.Cout == 64) RB_WGO(4, 1);
    else RB_WGO(4, 2);
#undef RB_WGO
    rc = sf_launch_status("sf_res_conv_wgrad_bf16 (partials)");
    if (rc) return rc;
    return sf_res_wgrad_sum_launch(part, (int)t.parts, KC, d.Cout, dw, db, s);
}
