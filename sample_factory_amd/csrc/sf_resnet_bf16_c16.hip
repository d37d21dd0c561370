// sf_resnet_bf16_c16.hip — the bf16 family (sf_resnet_bf16.hip, cfg.encoder_resnet_bf16) for the 16-channel layers of the
// width-1 resnet_impala tower: 16 -> 16 and 16 -> 32, every pass.  Reached through sf_res_conv_*_bf16 only; the arithmetic
// contract is the family's: bf16(act_in(x)), bf16(w), bf16(dout) rounded once to nearest even, fp32 accumulation, fp32
// epilogues in the fp32 family's order, fp32 tensors and [9*Cin, Cout] weights in memory, -ffp-contract=off.
//
// Forward and data gradient are ONE kernel, k_res_conv_bf16_c16<CR, CN, DGRAD>, CR reduced and CN produced channels:
// <16, 16> (forward and data gradient of 16 -> 16), <16, 32> (forward of 16 -> 32), <32, 16> (data gradient of 16 -> 32).
//   * K packing at CR = 16: one v_mfma_f32_16x16x32_bf16 reduces TWO taps.  Lane groups 0-1 carry channels 0..7 / 8..15 of
//     tap 2p, groups 2-3 the same of tap 2p + 1: still one ds_read_b128 per fragment, whose tap offset is a per-lane
//     constant.  Nine taps = four pairs + the odd tap 8 in a half-filled fifth step: there groups 2-3 hold zeros in B AND
//     read their A from a zeroed 16-byte word of LDS, so the unused half adds an exact zero whatever the data (an inf or
//     NaN pixel against a zero weight would not).  The odd tap on v_mfma_f32_16x16x16_bf16 was tried first: on the
//     device accumulators 0 and 1 came out wrong exactly for the chains in which the compiler had issued it directly
//     behind the 16x16x32 whose result it accumulates onto; one opcode per chain avoids the question.
//     At CR = 32 a step is one tap.  An output element's reduction order is (step, the MFMA's k order) and nothing else.
//   * The layer's whole B operand is loaded from global memory and rounded ONCE per wave and stays in registers:
//     5 x 4 = 20 VGPRs per 16-column slice at CR = 16 (20 / 40 for CN = 16 / 32), 9 x 4 = 36 at <32, 16>.  The
//     data gradient's B is the mirrored-tap transpose, B[(tap, o)][c] = W[(8 - tap)*Cin + c][o].
//   * The grid is at most RC_GRID work-groups; a work-group walks tiles blockIdx.x, + gridDim.x, ... with those registers,
//     so the weight traffic from L2 per output pixel falls by the number of tiles walked.
//   * A tile is S samples x TH rows x TW <= 32 columns of up to 512 pixels = 32 M fragments (the halo pixel is 48 bytes
//     at CR = 16, 80 at CR = 32: 18 x 24 pixels of a 36 x 48 image need 20 x 26 x 48 = 24 960 / 41 600 bytes).  The four
//     waves split the M fragments, two at a time per wave (two independent MFMA chains); a fragment's accumulators live
//     only until its epilogue, so the tile size is not bound by registers.
//   * Where a pixel of the tile lies (sample, row, column) is geometry that does not change from tile to tile: a table
//     in LDS, written once per work-group, replaces the integer divisions per fragment and per stored pixel.
//
// The weight gradient, k_res_wgrad_bf16_c16<CT> (Cout = 16 * CT), keeps the family's staging (both bands channel-major,
// rows padded to 8 pixels, three column-shifted copies of the input halo so that every tap is one aligned ds_read_b128,
// K = 32 pixels per MFMA as four runs of 8) but there is ONE Cin tile, so the four waves split K: the 32-pixel steps of
// the bands a work-group walks are dealt to the waves round-robin, the deal running on from band to band.  Every wave
// holds all 9 * CT + CT accumulators; at the end they are added through LDS in the fixed order (w0 + w2) + (w1 + w3) and
// wave 0 writes the part's partial.  k_res_conv_wgrad_sum adds the parts in part order: no float atomics.  The band takes
// as many rows as 64 KB holds (six rows of 48 pixels at 16 -> 32).
#include "sf_common.h"
#include "sf_resnet_shared.h"
#include "sf_bf16.h"

namespace {

constexpr int RC_TILE_M = 512;              // output pixels of a forward / data-gradient tile: 32 M fragments
constexpr int RC_TBL_BYTES = RC_TILE_M * 4 + 16;  // the pixel table and one zeroed 16-byte word in front of the halo band
constexpr int RC_LDS_BUDGET = 64 * 1024;    // dynamic LDS of one work-group
constexpr int RC_GRID = 1024;               // work-groups of a launch: more tiles (or bands) than this are walked
constexpr int RC_BAND_SAMPLE_PIX = 1024;    // padded pixels up to which a weight-gradient band packs whole samples

extern __shared__ float4 rc_lds4[];

__device__ __forceinline__ float4 rc_act4(int act, const float4 &v) {
    return make_float4(act_fwd(act, v.x), act_fwd(act, v.y), act_fwd(act, v.z), act_fwd(act, v.w));
}

// ------------------------------------------------------------------------------------------------ forward / dgrad
struct RcTile {
    int S, TH, TW, nrt, nct;  // samples, rows, columns of a tile; row / column tiles of an image
    int cs;                   // bf16 elements per halo pixel: CR + 8, i.e. 3 or 5 sixteen-byte words (odd)
    int M;                    // pixels of a tile, at most RC_TILE_M
    int64_t tiles;
};

int64_t rc_tile_bytes(const RcTile &t, int S, int TH) { return RC_TBL_BYTES + (int64_t)S * (TH + 2) * (t.TW + 2) * t.cs * 2; }

RcTile rc_tile(int H, int W, int Cr, int64_t n) {
    RcTile t;
    t.cs = Cr + 8;
    t.nct = (W + 31) / 32;
    t.TW = (W + t.nct - 1) / t.nct;
    int TH = std::max(1, std::min(H, RC_TILE_M / t.TW));
    while (TH > 1 && rc_tile_bytes(t, 1, TH) > RC_LDS_BUDGET) --TH;  // one row of 32 columns: 3 * 34 * 80 bytes, always fits
    t.nrt = (H + TH - 1) / TH;
    t.TH = (H + t.nrt - 1) / t.nrt;
    t.S = 1;
    if (t.nrt == 1 && t.nct == 1)
        while (t.S < n && (t.S + 1) * H * W <= RC_TILE_M && rc_tile_bytes(t, t.S + 1, t.TH) <= RC_LDS_BUDGET) ++t.S;
    t.M = t.S * t.TH * t.TW;
    t.tiles = ((n + t.S - 1) / t.S) * t.nrt * t.nct;
    return t;
}

// DGRAD = false: in = x [n,H,W,CR] (strided samples), act_in on load, a1 = residual, out_act / act_out as sf_res_conv_fwd.
// DGRAD = true:  in = dout [n,H,W,CR] dense, act = the activation whose derivative at a1 = pre multiplies, a2 = g_add.
// Pixel table entry of tile pixel m: column | row << 6 | sample << 16; bit 31: m is past the tile.
template <int CR, int CN, bool DGRAD>
__global__ __launch_bounds__(256) void k_res_conv_bf16_c16(const float *__restrict__ in, const float *__restrict__ w,
                                                           const float *__restrict__ bias, const float *__restrict__ a1,
                                                           const float *__restrict__ a2, float *__restrict__ out,
                                                           float *__restrict__ out_act, int act, int act_out, int64_t n,
                                                           int64_t in_stride, int64_t in_offset, int H, int W, RcTile t) {
    static_assert((CR == 16 || CR == 32) && (CN == 16 || CN == 32), "16-channel layers");
    constexpr int NS = CN / 16;             // 16-column slices of the produced channels
    constexpr int NQ = CR == 16 ? 5 : 9;    // 32-deep steps: four tap pairs and the half-filled odd tap, or taps
    uint32_t *tbl = reinterpret_cast<uint32_t *>(rc_lds4);
    __bf16 *lds = reinterpret_cast<__bf16 *>(rc_lds4) + RC_TBL_BYTES / 2;
    const int TH = t.TH, TW = t.TW, HW2 = TW + 2, HP = (TH + 2) * HW2, cs = t.cs, M = t.M, nfr = (M + 15) >> 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lg = lane >> 4;
    for (int m = threadIdx.x; m < nfr * 16; m += 256) {
        uint32_t e = 0x80000000u;
        if (m < M) {
            const int s = m / (TH * TW), rem = m - s * TH * TW, r = rem / TW;
            e = (uint32_t)(rem - r * TW) | (uint32_t)r << 6 | (uint32_t)s << 16;
        }
        tbl[m] = e;
    }
    if (threadIdx.x < 4) tbl[RC_TILE_M + threadIdx.x] = 0u;  // what the dead half of the odd step reads as A
    // ---- the layer's B operand, rounded once, resident: lane (column lr of slice sl, group lg)
    auto wv = [&](int tap, int cr, int col) -> float {
        return DGRAD ? w[((8 - tap) * CN + col) * CR + cr] : w[(tap * CR + cr) * CN + col];
    };
    bf16x8 bq[NQ][NS];
    int offq[NQ];  // halo offset of the lane's 8 channels at step q, relative to the pixel at tap (0, 0)
    const bool dead = CR == 16 && lg >= 2;  // in the odd step: tap 9 does not exist
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const bool zero = dead && q == NQ - 1;
        const int tap = zero ? 8 : CR == 16 ? 2 * q + (lg >> 1) : q, c0 = CR == 16 ? 8 * (lg & 1) : 8 * lg;
        offq[q] = ((tap / 3) * HW2 + tap % 3) * cs + c0;
#pragma unroll
        for (int sl = 0; sl < NS; ++sl)
#pragma unroll
            for (int i = 0; i < 8; ++i) bq[q][sl][i] = zero ? (__bf16)0.0f : (__bf16)wv(tap, c0 + i, sl * 16 + lr);
    }
    float bv[NS];
#pragma unroll
    for (int sl = 0; sl < NS; ++sl) bv[sl] = DGRAD ? 0.0f : bias[sl * 16 + lr];
    constexpr int q8 = CR >> 3;
    for (int64_t tile = blockIdx.x; tile < t.tiles; tile += gridDim.x) {
        const int ct = (int)(tile % t.nct), rt = (int)((tile / t.nct) % t.nrt);
        const int64_t s0 = (tile / (t.nct * t.nrt)) * t.S;
        const int ns = (int)min((int64_t)t.S, n - s0), h0 = rt * TH, w0 = ct * TW;
        __syncthreads();  // the previous tile's fragments have been read
        // ---- halo band -> LDS as bf16(act(x)); everything outside the image (or past the last sample) is an exact zero
        for (int i = threadIdx.x; i < t.S * HP * q8; i += 256) {
            const int q = i % q8, hp = i / q8, s = hp / HP, rr = (hp - s * HP) / HW2, cc = hp - s * HP - rr * HW2;
            const int h = h0 + rr - 1, ww = w0 + cc - 1;
            float4 v0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), v1 = v0;
            if (s < ns && h >= 0 && h < H && ww >= 0 && ww < W) {
                const float4 *p = reinterpret_cast<const float4 *>(in + (in_offset + s0 + s) * in_stride + ((int64_t)h * W + ww) * CR + 8 * q);
                v0 = p[0];
                v1 = p[1];
                if (!DGRAD && act) { v0 = rc_act4(act, v0); v1 = rc_act4(act, v1); }
            }
            *reinterpret_cast<bf16x8 *>(lds + hp * cs + 8 * q) = bf16_pack(v0, v1);
        }
        __syncthreads();
        for (int fb = wave * 2; fb < nfr; fb += 8) {
            int hb[2];
            floatx4 acc[2][NS];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const uint32_t e = tbl[min(fb + u, nfr - 1) * 16 + lr];  // a lane past the tile reads pixel 0; never stored
                hb[u] = (((int)((e >> 16) & 1023) * (TH + 2) + (int)((e >> 6) & 1023)) * HW2 + (int)(e & 63)) * cs;
#pragma unroll
                for (int sl = 0; sl < NS; ++sl) acc[u][sl] = (floatx4){0.0f, 0.0f, 0.0f, 0.0f};
            }
#pragma unroll
            for (int q = 0; q < NQ; ++q)
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int ao = (q == NQ - 1 && dead) ? -8 : hb[u] + offq[q];  // -8: the zeroed word in front of the band
                    const bf16x8 a = *reinterpret_cast<const bf16x8 *>(lds + ao);
#pragma unroll
                    for (int sl = 0; sl < NS; ++sl)
                        acc[u][sl] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, bq[q][sl], acc[u][sl], 0, 0, 0);
                }
            // ---- epilogue: accumulator j of fragment f, slice sl is tile pixel 16*f + 4*lg + j, channel 16*sl + lr
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if (fb + u >= nfr) break;
                const uint4 e4 = *reinterpret_cast<const uint4 *>(tbl + (fb + u) * 16 + 4 * lg);
                const uint32_t ej[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int s = (int)((ej[j] >> 16) & 1023), r = (int)((ej[j] >> 6) & 1023), c = (int)(ej[j] & 63);
                    if ((ej[j] >> 31) || s >= ns || h0 + r >= H || w0 + c >= W) continue;
                    const int64_t base = (((s0 + s) * H + h0 + r) * W + w0 + c) * CN + lr;
#pragma unroll
                    for (int sl = 0; sl < NS; ++sl) {
                        const int64_t idx = base + sl * 16;
                        float v = acc[u][sl][j];
                        if (DGRAD) {
                            if (act) v = v * act_grad(act, a1[idx]);
                            if (a2) v = a2[idx] + v;
                            out[idx] = v;
                        } else {
                            v = v + bv[sl];
                            if (a1) v = a1[idx] + v;
                            out[idx] = v;
                            if (out_act) out_act[idx] = act_fwd(act_out, v);
                        }
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ weight gradient
struct RcBand {
    int S, TH, nrt;    // samples and whole rows of a band; bands per image
    int WP8, RW;       // columns of a row padded to a multiple of 8; runs of 8 pixels per row
    int csa, csg;      // bf16 elements per channel of one halo copy / of the dout band: an odd number of 16-byte words
    int64_t NB, bpp, parts;  // bands in the batch, bands per part, parts = grid.x
    int64_t lds_bytes;
};

// false: a single row of this layer does not fit the LDS budget (W > 200 at 16 -> 16, W > 184 at 16 -> 32)
bool rc_band(int H, int W, int Cout, int64_t n, RcBand *out) {
    RcBand t;
    t.WP8 = (W + 7) & ~7;
    t.RW = t.WP8 >> 3;
    auto bytes = [&](int64_t S, int TH) {
        return 2 * ((int64_t)3 * 16 * odd8((int)(S * (TH + 2) * t.WP8)) + (int64_t)Cout * odd8((int)(S * TH * t.WP8)));
    };
    if (bytes(1, 1) > RC_LDS_BUDGET) return false;
    int TH = std::max<int64_t>(1, std::min<int64_t>(H, RC_LDS_BUDGET / (2 * (48 + Cout) * (int64_t)t.WP8)));
    while (TH > 1 && bytes(1, TH) > RC_LDS_BUDGET) --TH;
    t.nrt = (H + TH - 1) / TH;
    t.TH = (H + t.nrt - 1) / t.nrt;
    t.S = 1;
    if (t.nrt == 1)
        while (t.S < n && (int64_t)(t.S + 1) * H * t.WP8 <= RC_BAND_SAMPLE_PIX && bytes(t.S + 1, t.TH) <= RC_LDS_BUDGET) ++t.S;
    t.csa = odd8(t.S * (t.TH + 2) * t.WP8);
    t.csg = odd8(t.S * t.TH * t.WP8);
    // the waves' accumulators meet in two slots of (9 + 1) * CT float4 per lane
    t.lds_bytes = std::max<int64_t>(bytes(t.S, t.TH), 2LL * 10 * (Cout / 16) * 64 * 16);
    t.NB = ((n + t.S - 1) / t.S) * t.nrt;
    t.bpp = std::max<int64_t>(1, (t.NB + RC_GRID - 1) / RC_GRID);
    t.parts = std::max<int64_t>(1, (t.NB + t.bpp - 1) / t.bpp);
    *out = t;
    return true;
}

template <int CT>
__global__ __launch_bounds__(256) void k_res_wgrad_bf16_c16(const float *__restrict__ x, const float *__restrict__ gy,
                                                            float *__restrict__ part, int act, int64_t n, int64_t in_stride,
                                                            int64_t in_offset, int H, int W, RcBand t) {
    constexpr int Cin = 16, Cout = 16 * CT, NA = 10 * CT;
    __bf16 *la = reinterpret_cast<__bf16 *>(rc_lds4);
    const int TH = t.TH, WP8 = t.WP8, RW = t.RW, csa = t.csa, csg = t.csg;
    __bf16 *lgy = la + 3 * Cin * csa;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lg = lane >> 4;
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
    constexpr int qa = Cin >> 2, qg = Cout >> 2;
    const __bf16 *xa = la + lr * csa, *ga = lgy + lr * csg;
    // a wave's next step is 16 runs on: 16 = ds * (TH * RW) + dr * RW + dj
    const int ds = 16 / (TH * RW), dr = (16 - ds * TH * RW) / RW, dj = 16 - ds * TH * RW - dr * RW;
    unsigned dealt = 0;  // steps dealt so far: step g of the walk belongs to wave g % 4
    for (int64_t band = b0; band < b1; ++band) {
        const int64_t s0 = (band / t.nrt) * t.S;
        const int ns = (int)min((int64_t)t.S, n - s0), h0 = (int)(band % t.nrt) * TH;
        __syncthreads();  // the previous band's fragments have been read
        // ---- input halo, channel-major, three column-shifted copies: copy kw, run j = columns 8j + kw - 1 .. + 7
        for (int i = threadIdx.x; i < t.S * (TH + 2) * RW * qa; i += 256) {
            const int q = i % qa, rest = i / qa, j = rest % RW, hp = rest / RW, s = hp / (TH + 2), rr = hp - s * (TH + 2);
            const int h = h0 + rr - 1;
            __bf16 v[10][4];
#pragma unroll
            for (int e = 0; e < 10; ++e) {
                const int col = 8 * j - 1 + e;
                float4 f = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (s < ns && h >= 0 && h < H && col >= 0 && col < W) {
                    f = *reinterpret_cast<const float4 *>(x + (in_offset + s0 + s) * in_stride + ((int64_t)h * W + col) * Cin + 4 * q);
                    if (act) f = rc_act4(act, f);
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
                    *reinterpret_cast<bf16x8 *>(la + (kw * Cin + 4 * q + c) * csa + hp * WP8 + 8 * j) = o;
                }
        }
        // ---- dout band, channel-major; padding columns, rows past the image and samples past the batch are zeros
        for (int i = threadIdx.x; i < t.S * TH * RW * qg; i += 256) {
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
        // ---- 32 pixels per MFMA: in step `it` lane group lg takes run 4*it + lg of the band's ns * TH * RW runs
        const int NR = ns * TH * RW, nst = (NR + 3) >> 2;
        int it = (int)((wave - dealt) & 3u);
        dealt += (unsigned)nst;
        int rho = 4 * it + lg, s = rho / (TH * RW), r = (rho - s * TH * RW) / RW, j = rho - s * TH * RW - r * RW;
        for (; it < nst; it += 4) {
            const bool live = rho < NR;  // past the band: a zero dout run against any finite input run
            const int gofs = live ? (s * TH + r) * WP8 + 8 * j : 0, aofs = live ? (s * (TH + 2) + r) * WP8 + 8 * j : 0;
            bf16x8 b[CT];
#pragma unroll
            for (int u = 0; u < CT; ++u) b[u] = live ? *reinterpret_cast<const bf16x8 *>(ga + u * 16 * csg + gofs) : zero8;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const bf16x8 a = *reinterpret_cast<const bf16x8 *>(xa + (tap % 3) * Cin * csa + aofs + (tap / 3) * WP8);
#pragma unroll
                for (int u = 0; u < CT; ++u) acc[tap][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[u], acc[tap][u], 0, 0, 0);
            }
#pragma unroll
            for (int u = 0; u < CT; ++u) accb[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones8, b[u], accb[u], 0, 0, 0);
            rho += 16;
            j += dj;
            if (j >= RW) { j -= RW; ++r; }
            r += dr;
            if (r >= TH) { r -= TH; ++s; }
            s += ds;
        }
    }
    // ---- the four waves' sums, in the fixed order (w0 + w2) + (w1 + w3)
    floatx4 *red = reinterpret_cast<floatx4 *>(rc_lds4);
    auto put = [&](int slot) {
#pragma unroll
        for (int u = 0; u < CT; ++u) {
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) red[(slot * NA + u * 10 + tap) * 64 + lane] = acc[tap][u];
            red[(slot * NA + u * 10 + 9) * 64 + lane] = accb[u];
        }
    };
    auto add = [&](int slot) {
#pragma unroll
        for (int u = 0; u < CT; ++u) {
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) acc[tap][u] = acc[tap][u] + red[(slot * NA + u * 10 + tap) * 64 + lane];
            accb[u] = accb[u] + red[(slot * NA + u * 10 + 9) * 64 + lane];
        }
    };
    __syncthreads();  // the last band's fragments have been read
    if (wave >= 2) put(wave - 2);
    __syncthreads();
    if (wave < 2) add(wave);
    __syncthreads();
    if (wave == 1) put(0);
    __syncthreads();
    if (wave != 0) return;
    add(0);
    // accumulator j: input channel 4*lg + j, output channel lr of Cout tile u
    constexpr int KC = 9 * Cin * Cout;
    float *pp = part + (int64_t)blockIdx.x * (KC + Cout);
#pragma unroll
    for (int u = 0; u < CT; ++u) {
        const int o = u * 16 + lr;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int j = 0; j < 4; ++j) pp[(tap * Cin + 4 * lg + j) * Cout + o] = acc[tap][u][j];
        if (lg == 0) pp[KC + o] = accb[u][0];
    }
}

}  // namespace

bool sf_res_c16_pair(int Cin, int Cout) { return Cin == 16 && (Cout == 16 || Cout == 32); }

int sf_res_c16_conv_launch(bool dgrad, const float *in, int64_t in_stride, int64_t in_offset, const float *w, const float *bias,
                           const float *a1, const float *a2, float *out, float *out_act, int act, int act_out, int64_t n,
                           int H, int W, int Cr, int Cn, hipStream_t s) {
    const RcTile t = rc_tile(H, W, Cr, n);
    const dim3 grid((unsigned)std::min<int64_t>(t.tiles, RC_GRID));
    const size_t lds = (size_t)rc_tile_bytes(t, t.S, t.TH);
#define RC_GO(CR, CN, DG)                                                                                              \
    hipLaunchKernelGGL((k_res_conv_bf16_c16<CR, CN, DG>), grid, dim3(256), lds, s, in, w, bias, a1, a2, out, out_act,   \
                       act, act_out, n, in_stride, in_offset, H, W, t)
    if (!dgrad && Cn == 16) RC_GO(16, 16, false);
    else if (!dgrad) RC_GO(16, 32, false);
    else if (Cr == 16) RC_GO(16, 16, true);
    else RC_GO(32, 16, true);
#undef RC_GO
    return sf_launch_status(dgrad ? "sf_res_conv_dgrad_bf16" : "sf_res_conv_fwd_bf16");
}

int64_t sf_res_c16_wgrad_parts(int H, int W, int Cout, int64_t n) {
    RcBand t;
    return rc_band(H, W, Cout, n, &t) ? t.parts : 0;
}

int sf_res_c16_wgrad_launch(const float *x, int64_t in_stride, int64_t in_offset, const float *gy, float *part, int act,
                            int64_t n, int H, int W, int Cout, hipStream_t s) {
    RcBand t;
    if (!rc_band(H, W, Cout, n, &t)) {
        snprintf(sf_err_buf, sizeof(sf_err_buf), "sf_res_conv_wgrad_bf16: a row of W=%d pixels x (Cin=16, Cout=%d) exceeds the "
                 "%d-byte LDS band (200 pixels at 16 -> 16, 184 at 16 -> 32)", W, Cout, RC_LDS_BUDGET);
        return SF_ERR_UNSUPPORTED;
    }
    const dim3 grid((unsigned)t.parts);
    if (Cout == 16)
        hipLaunchKernelGGL((k_res_wgrad_bf16_c16<1>), grid, dim3(256), (size_t)t.lds_bytes, s, x, gy, part, act, n, in_stride,
                           in_offset, H, W, t);
    else
        hipLaunchKernelGGL((k_res_wgrad_bf16_c16<2>), grid, dim3(256), (size_t)t.lds_bytes, s, x, gy, part, act, n, in_stride,
                           in_offset, H, W, t);
    return sf_launch_status("sf_res_conv_wgrad_bf16 (partials)");
}
