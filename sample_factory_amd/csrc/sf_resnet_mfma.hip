// sf_resnet_mfma.hip — the 3x3 / stride 1 / pad 1 conv family of the resnet_impala encoder on v_mfma_f32_16x16x4_f32, for
// f32 NHWC layers with Cin, Cout in {16, 32, 64, 128} (every pair): the wide towers of cfg.encoder_resnet_width = 2 and 4.
// Weights stay K-major [9*Cin, Cout], k = (kh*3 + kw)*Cin + c; no second weight layout is kept anywhere.
//
// Forward and data gradient are ONE kernel (k_res_conv_mfma): an implicit GEMM with M = output pixels, N = the produced
// channels (NS slices of 16), K = 9 taps x the reduced channels Cr.
//   * A work-group takes a tile of S samples x TH rows x TW columns (<= 128 pixels = 8 M fragments; several whole samples
//     when the image is small) and stages its halo, rows -1 .. TH and columns -1 .. TW, in LDS once, already activated;
//     positions outside the image are written as exact zeros.  A pixel's channels are contiguous, the pixel stride is
//     Cr + 4 floats.
//   * A wave owns one 16-column slice of N and FW = 8 / MW of the M fragments (MW waves share a slice when N is narrow:
//     N = 16 -> the four waves split M).  Per tap and 16-channel chunk it reads each A fragment with one ds_read_b128: lane
//     (pixel l % 16, group l / 16) gets channels 4*(l/16) .. +3 of the chunk, which are its k-rows of four consecutive
//     MFMAs — the k order inside a chunk is (4g + j) for MFMA j, the same on the B side.
//   * The weights stream: the wave loads its B fragments of the next (tap, chunk) from global memory (L2) while the MFMAs of
//     the current one run, and every fragment is reused by all FW M fragments.  Forward reads B[k][n] = W[k, n] as four
//     dwords (rows 4g + j); the data gradient reads the transpose of the same block, B[o][c] = W[(2-kh, 2-kw), c][o], as
//     one float4 along o (row c = the lane's column), taps mirrored.
//   * Epilogue from the accumulators, rounding after each op in the FMA kernels' order: forward bias, residual, activation;
//     data gradient act'(pre), g_add.
//
// The weight gradient (k_res_wgrad_mfma) reduces over pixels: M = 16 input channels, N = 16 output channels, K = pixels in
// steps of 4 along a row.  Grid = pixel parts x Cin blocks.  A work-group walks its part band by band (S samples x TH
// whole rows), stages the activated input halo of its Cin block and the dout band in LDS (rows padded to a multiple of 4
// columns with zeros) and keeps 9 taps x CT output tiles per wave in registers; the bias gradient is one more MFMA
// against a fragment of ones.  Partials go to the workspace [parts][9*Cin*Cout + Cout]; k_res_conv_wgrad_sum (in
// sf_resnet.hip, the FMA weight gradient's second stage) adds them in part order: deterministic, no float atomics.
//
// Compiled with -ffp-contract=off like sf_resnet.hip: the epilogues round after each op.
#include "sf_common.h"
#include "sf_resnet_shared.h"

#define STREAM(s) reinterpret_cast<hipStream_t>(s)

namespace {

typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr int RM_FRAGS = 8;                // M fragments of a forward / data-gradient tile
constexpr int RM_TILE_M = 16 * RM_FRAGS;   // ... = 128 output pixels
constexpr int RM_LDS_BUDGET = 64 * 1024;   // dynamic LDS of one work-group: two of them per CU
constexpr int RW_BAND_PIX = 128;           // pixels (padded columns counted) of one weight-gradient band
constexpr int RW_MIN_PARTS = 64;
constexpr int RW_GRID_TARGET = 1024;       // work-groups the weight gradient aims at: parts x Cin blocks

extern __shared__ float4 rm_lds4[];

// ------------------------------------------------------------------------------------------------ forward / dgrad
struct RmTile {
    int S, TH, TW, nrt, nct;  // samples, rows, columns of a tile; row / column tiles of an image
    int cs;                   // LDS floats per halo pixel: Cr + 4 (odd multiple of 4 -> 16 pixels cover all banks)
};

int64_t rm_tile_bytes(const RmTile &t, int S, int TH) { return (int64_t)S * (TH + 2) * (t.TW + 2) * t.cs * 4; }

RmTile rm_tile(int H, int W, int Cr, int64_t n) {
    RmTile t;
    t.cs = Cr + 4;
    t.nct = (W + 31) / 32;
    t.TW = (W + t.nct - 1) / t.nct;
    int TH = std::max(1, std::min(H, RM_TILE_M / t.TW));
    while (TH > 1 && rm_tile_bytes(t, 1, TH) > RM_LDS_BUDGET) --TH;  // TH = 1: 3 * 34 * 132 * 4 = 53 856 bytes at most
    t.nrt = (H + TH - 1) / TH;
    t.TH = (H + t.nrt - 1) / t.nrt;
    t.S = 1;
    if (t.nrt == 1 && t.nct == 1)
        while (t.S < n && (t.S + 1) * H * W <= RM_TILE_M && rm_tile_bytes(t, t.S + 1, t.TH) <= RM_LDS_BUDGET) ++t.S;
    return t;
}

// NS: 16-column slices of the produced channels Cn = 16 * NS; MW: waves that share a slice and split the M fragments.
// DGRAD = false: in = x [n,H,W,Cr] (strided samples), act_in on load, a1 = residual, out_act / act_out as sf_res_conv_fwd.
// DGRAD = true:  in = dout [n,H,W,Cr] dense, act = the activation whose derivative at a1 = pre multiplies, a2 = g_add.
template <int NS, int MW, bool DGRAD>
__global__ __launch_bounds__(NS * MW * 64) void k_res_conv_mfma(const float *__restrict__ in, const float *__restrict__ w,
                                                                const float *__restrict__ bias, const float *__restrict__ a1,
                                                                const float *__restrict__ a2, float *__restrict__ out,
                                                                float *__restrict__ out_act, int act, int act_out, int64_t n,
                                                                int64_t in_stride, int64_t in_offset, int H, int W, int Cr,
                                                                RmTile t) {
    constexpr int Cn = 16 * NS, FW = RM_FRAGS / MW;
    float *lds = reinterpret_cast<float *>(rm_lds4);
    const int TH = t.TH, TW = t.TW, HW2 = TW + 2, HP = (TH + 2) * HW2, cs = t.cs;
    const int ct = blockIdx.x % t.nct, rt = (blockIdx.x / t.nct) % t.nrt;
    const int64_t s0 = (int64_t)(blockIdx.x / (t.nct * t.nrt)) * t.S;
    const int ns = (int)min((int64_t)t.S, n - s0), h0 = rt * TH, w0 = ct * TW;
    // ---- halo band -> LDS, activated; everything outside the image (or past the last sample) is an exact zero
    const int q4 = Cr >> 2;
    for (int i = threadIdx.x; i < t.S * HP * q4; i += NS * MW * 64) {
        const int q = i % q4, hp = i / q4, s = hp / HP, rr = (hp - s * HP) / HW2, cc = hp - s * HP - rr * HW2;
        const int h = h0 + rr - 1, ww = w0 + cc - 1;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (s < ns && h >= 0 && h < H && ww >= 0 && ww < W) {
            v = *reinterpret_cast<const float4 *>(in + (in_offset + s0 + s) * in_stride + ((int64_t)h * W + ww) * Cr + 4 * q);
            if (!DGRAD && act) v = make_float4(act_fwd(act, v.x), act_fwd(act, v.y), act_fwd(act, v.z), act_fwd(act, v.w));
        }
        *reinterpret_cast<float4 *>(lds + hp * cs + 4 * q) = v;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, slice = wave % NS, f0 = (wave / NS) * FW;
    const int lr = lane & 15, lg = lane >> 4;
    const int M = t.S * TH * TW, nfr = (M + 15) >> 4;
    int hb[FW];  // LDS offset of the lane's pixel at tap (0, 0), its channel group added
    floatx4 acc[FW];
#pragma unroll
    for (int f = 0; f < FW; ++f) {
        int m = (f0 + f) * 16 + lr;
        if (m >= M) m = 0;  // a lane past the tile reads a real pixel; its rows are never stored
        const int s = m / (TH * TW), r = (m / TW) % TH, c = m % TW;
        hb[f] = ((s * (TH + 2) + r) * HW2 + c) * cs + 4 * lg;
        acc[f] = (floatx4){0.0f, 0.0f, 0.0f, 0.0f};
    }
    const int nch = Cr >> 4, steps = 9 * nch;
    // B fragments of step it = (tap, 16-channel chunk): lane (column lr, group lg) holds k-rows 4*lg + j, j = 0..3
    auto load_b = [&](int tap, int ch) -> floatx4 {
        if (DGRAD) {  // B[o][c] = W[(8 - tap)*Cn + c][o]: the lane's row c, four consecutive o
            const float4 v = *reinterpret_cast<const float4 *>(w + ((int64_t)(8 - tap) * Cn + slice * 16 + lr) * Cr + ch * 16 + 4 * lg);
            return (floatx4){v.x, v.y, v.z, v.w};
        }
        const float *p = w + ((int64_t)(tap * Cr + ch * 16 + 4 * lg)) * Cn + slice * 16 + lr;
        return (floatx4){p[0], p[Cn], p[2 * Cn], p[3 * Cn]};
    };
    floatx4 bc = load_b(0, 0), bn = bc;
    int tap = 0, ch = 0;
    for (int it = 0; it < steps; ++it) {
        const int aoff = ((tap / 3) * HW2 + tap % 3) * cs + ch * 16;
        if (++ch == nch) { ch = 0; ++tap; }
        if (it + 1 < steps) bn = load_b(tap, ch);
#pragma unroll
        for (int f = 0; f < FW; ++f) {
            if (f0 + f < nfr) {
                const floatx4 a = *reinterpret_cast<const floatx4 *>(lds + hb[f] + aoff);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j], bc[j], acc[f], 0, 0, 0);
            }
        }
        bc = bn;
    }
    // ---- epilogue: accumulator j of fragment f is pixel 16*f + 4*lg + j, channel slice*16 + lr
    const int o = slice * 16 + lr;
    const float bo = DGRAD ? 0.0f : bias[o];
#pragma unroll
    for (int f = 0; f < FW; ++f) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int m = (f0 + f) * 16 + 4 * lg + j;
            const int s = m / (TH * TW), r = (m / TW) % TH, c = m % TW;
            if (m >= M || s >= ns || h0 + r >= H || w0 + c >= W) continue;
            const int64_t idx = (((s0 + s) * H + h0 + r) * W + w0 + c) * Cn + o;
            float v = acc[f][j];
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

template <bool DGRAD>
void rm_launch(int Cn, dim3 grid, size_t lds, hipStream_t s, const float *in, const float *w, const float *bias,
               const float *a1, const float *a2, float *out, float *out_act, int act, int act_out, int64_t n,
               int64_t in_stride, int64_t in_offset, int H, int W, int Cr, const RmTile &t) {
#define RM_GO(NS, MW)                                                                                                  \
    hipLaunchKernelGGL((k_res_conv_mfma<NS, MW, DGRAD>), grid, dim3(NS * MW * 64), lds, s, in, w, bias, a1, a2, out,    \
                       out_act, act, act_out, n, in_stride, in_offset, H, W, Cr, t)
    if (Cn == 16) RM_GO(1, 4);
    else if (Cn == 32) RM_GO(2, 2);
    else if (Cn == 64) RM_GO(4, 1);
    else RM_GO(8, 1);
#undef RM_GO
}

// ------------------------------------------------------------------------------------------------ weight gradient
struct RwBand {
    int S, TH, nrt;    // samples and whole rows of a band; bands per image
    int WP4, WPH;      // columns of a dout row padded to a multiple of 4; of a halo row (+2)
    int ciw, CW;       // 16-channel Cin tiles of a work-group, and their channels
    int csa, cso;      // LDS floats per halo pixel / per dout pixel: = 16 or 48 (mod 64), so that the four pixel groups of
                       // a fragment read (16 channels each) fall on disjoint banks
    int blocks;        // Cin blocks = grid.y
    int64_t NB, bpp, parts;  // bands in the batch, bands per part, parts = grid.x
    int64_t lds_bytes;
};

int rw_pad(int c) { return c == 16 ? 16 : c + 16; }

// false: a single row of this layer does not fit the LDS budget
bool rw_band(int H, int W, int Cin, int Cout, int64_t n, RwBand *out) {
    RwBand t;
    const int ncog = std::min(Cout / 16, 4);
    t.ciw = std::min(Cin / 16, 4 / ncog);
    t.CW = 16 * t.ciw;
    t.blocks = (Cin / 16) / t.ciw;
    t.csa = rw_pad(t.CW);
    t.cso = rw_pad(Cout);
    t.WP4 = (W + 3) & ~3;
    t.WPH = t.WP4 + 2;
    auto bytes = [&](int S, int TH) {
        return 4 * ((int64_t)S * (TH + 2) * t.WPH * t.csa + (int64_t)S * TH * t.WP4 * t.cso);
    };
    int TH = std::max(1, std::min(H, RW_BAND_PIX / t.WP4));
    while (TH > 1 && bytes(1, TH) > RM_LDS_BUDGET) --TH;
    if (bytes(1, TH) > RM_LDS_BUDGET) return false;
    t.nrt = (H + TH - 1) / TH;
    t.TH = (H + t.nrt - 1) / t.nrt;
    t.S = 1;
    if (t.nrt == 1)
        while (t.S < n && (t.S + 1) * H * t.WP4 <= RW_BAND_PIX && bytes(t.S + 1, t.TH) <= RM_LDS_BUDGET) ++t.S;
    t.lds_bytes = bytes(t.S, t.TH);
    t.NB = ((n + t.S - 1) / t.S) * t.nrt;
    const int64_t target = std::max(RW_MIN_PARTS, RW_GRID_TARGET / t.blocks);
    t.bpp = std::max<int64_t>(1, (t.NB + target - 1) / target);
    t.parts = std::max<int64_t>(1, (t.NB + t.bpp - 1) / t.bpp);
    *out = t;
    return true;
}

// NCOG x CT 16-column tiles of Cout: wave (cit, cog) owns Cin tile cit of the block and Cout tiles cog*CT .. +CT-1
template <int NCOG, int CT>
__global__ __launch_bounds__(256) void k_res_wgrad_mfma(const float *__restrict__ x, const float *__restrict__ gy,
                                                        float *__restrict__ part, int act, int64_t n, int64_t in_stride,
                                                        int64_t in_offset, int H, int W, int Cin, RwBand t) {
    constexpr int Cout = 16 * NCOG * CT;
    float *la = reinterpret_cast<float *>(rm_lds4);
    const int TH = t.TH, WP4 = t.WP4, WPH = t.WPH, csa = t.csa, cso = t.cso, HP = (TH + 2) * WPH, GP = TH * WP4;
    float *lg_ = la + t.S * HP * csa;
    const int nthr = blockDim.x, cbase = blockIdx.y * t.CW;
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
    const int64_t b0 = (int64_t)blockIdx.x * t.bpp, b1 = min(t.NB, b0 + t.bpp);
    const int qa = t.CW >> 2, qg = Cout >> 2;
    for (int64_t band = b0; band < b1; ++band) {
        const int64_t s0 = (band / t.nrt) * t.S;
        const int ns = (int)min((int64_t)t.S, n - s0), h0 = (int)(band % t.nrt) * TH;
        __syncthreads();  // the previous band's fragments have been read
        for (int i = threadIdx.x; i < t.S * HP * qa; i += nthr) {
            const int q = i % qa, hp = i / qa, s = hp / HP, rr = (hp - s * HP) / WPH, cc = hp - s * HP - rr * WPH;
            const int h = h0 + rr - 1, ww = cc - 1;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (s < ns && h >= 0 && h < H && ww >= 0 && ww < W) {
                v = *reinterpret_cast<const float4 *>(x + (in_offset + s0 + s) * in_stride + ((int64_t)h * W + ww) * Cin + cbase + 4 * q);
                if (act) v = make_float4(act_fwd(act, v.x), act_fwd(act, v.y), act_fwd(act, v.z), act_fwd(act, v.w));
            }
            *reinterpret_cast<float4 *>(la + hp * csa + 4 * q) = v;
        }
        for (int i = threadIdx.x; i < t.S * GP * qg; i += nthr) {
            const int q = i % qg, gp = i / qg, s = gp / GP, r = (gp - s * GP) / WP4, c = gp - s * GP - r * WP4;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (s < ns && h0 + r < H && c < W)
                v = *reinterpret_cast<const float4 *>(gy + (((s0 + s) * H + h0 + r) * W + c) * Cout + 4 * q);
            *reinterpret_cast<float4 *>(lg_ + gp * cso + 4 * q) = v;
        }
        __syncthreads();
        for (int s = 0; s < ns; ++s) {
            for (int r = 0; r < TH; ++r) {
                const float *ga = lg_ + ((s * TH + r) * WP4 + lg) * cso + cog * CT * 16 + lr;
                const float *xa = la + ((s * (TH + 2) + r) * WPH + lg) * csa + cit * 16 + lr;
                for (int ks = 0; ks < WP4; ks += 4) {  // four pixels of the row per MFMA: the lane's is column ks + lg
                    float b[CT];
#pragma unroll
                    for (int u = 0; u < CT; ++u) b[u] = ga[ks * cso + u * 16];
#pragma unroll
                    for (int tap = 0; tap < 9; ++tap) {
                        const float a = xa[((tap / 3) * WPH + tap % 3 + ks) * csa];
#pragma unroll
                        for (int u = 0; u < CT; ++u) acc[tap][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[u], acc[tap][u], 0, 0, 0);
                    }
                    if (do_bias) {
#pragma unroll
                        for (int u = 0; u < CT; ++u) accb[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(1.0f, b[u], accb[u], 0, 0, 0);
                    }
                }
            }
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

int rm_check(const sf_res_desc *d, const char *what) {
    SF_REQUIRE(d != nullptr, "%s: desc is NULL", what);
    SF_REQUIRE(d->H >= 1 && d->W >= 1, "%s: bad geometry H=%d W=%d", what, d->H, d->W);
    SF_REQUIRE(d->act_in >= 0 && d->act_in <= 3, "%s: act_in=%d not in 0..3", what, d->act_in);
    if (d->in_u8 || d->traj_T != 0 || !res_mfma_width(d->Cin) || !res_mfma_width(d->Cout)) {
        snprintf(sf_err_buf, sizeof(sf_err_buf),
                 "%s: Cin=%d Cout=%d in_u8=%d traj_T=%d (the MFMA family serves dense f32 NHWC layers with Cin and Cout in "
                 "{16, 32, 64, 128})", what, d->Cin, d->Cout, d->in_u8, d->traj_T);
        return SF_ERR_UNSUPPORTED;
    }
    return SF_OK;
}

}  // namespace

extern "C" int sf_res_conv_fwd_mfma(const void *in, int64_t in_sample_stride, const int32_t *index, int64_t offset,
                                    const float *w, const float *bias, const float *residual, float *out, float *out_act,
                                    int act_out, int64_t n, const sf_res_desc *h_desc, void *stream) {
    int rc = rm_check(h_desc, "sf_res_conv_fwd_mfma");
    if (rc) return rc;
    const sf_res_desc &d = *h_desc;
    SF_REQUIRE(in && w && bias && out, "sf_res_conv_fwd_mfma: NULL operand");
    SF_REQUIRE(index == nullptr, "sf_res_conv_fwd_mfma: index addressing is for the raw u8 frames only");
    SF_REQUIRE(n >= 0 && offset >= 0, "sf_res_conv_fwd_mfma: n=%lld offset=%lld", (long long)n, (long long)offset);
    SF_REQUIRE(act_out >= 0 && act_out <= 3, "sf_res_conv_fwd_mfma: act_out=%d", act_out);
    SF_REQUIRE(in_sample_stride >= (int64_t)d.Cin * d.H * d.W && (in_sample_stride & 3) == 0,
               "sf_res_conv_fwd_mfma: in_sample_stride %lld (at least Cin*H*W, a multiple of 4)", (long long)in_sample_stride);
    SF_REQUIRE(aligned16(in) && aligned16(w) && aligned16(out) && (!out_act || aligned16(out_act)) &&
                   (!residual || aligned16(residual)),
               "sf_res_conv_fwd_mfma: in, w, out, out_act and residual must be 16-byte aligned");
    if (n == 0) return SF_OK;
    const RmTile t = rm_tile(d.H, d.W, d.Cin, n);
    const int64_t groups = ((n + t.S - 1) / t.S) * t.nrt * t.nct;
    SF_REQUIRE(groups <= 0x7fffffffLL, "sf_res_conv_fwd_mfma: %lld work-groups", (long long)groups);
    rm_launch<false>(d.Cout, dim3((unsigned)groups), (size_t)rm_tile_bytes(t, t.S, t.TH), STREAM(stream), (const float *)in, w,
                     bias, residual, nullptr, out, out_act, d.act_in, act_out, n, in_sample_stride, offset, d.H, d.W, d.Cin, t);
    return sf_launch_status("sf_res_conv_fwd_mfma");
}

extern "C" int sf_res_conv_dgrad_mfma(const float *dout, const float *w, const float *pre, const float *g_add, float *din,
                                      int64_t n, const sf_res_desc *h_desc, void *stream) {
    int rc = rm_check(h_desc, "sf_res_conv_dgrad_mfma");
    if (rc) return rc;
    const sf_res_desc &d = *h_desc;
    SF_REQUIRE(dout && w && din, "sf_res_conv_dgrad_mfma: NULL operand");
    SF_REQUIRE(!d.act_in || pre, "sf_res_conv_dgrad_mfma: act_in=%d needs the pre-activation input", d.act_in);
    SF_REQUIRE(n >= 0, "sf_res_conv_dgrad_mfma: n=%lld", (long long)n);
    SF_REQUIRE(aligned16(w) && aligned16(dout), "sf_res_conv_dgrad_mfma: w and dout must be 16-byte aligned");
    if (n == 0) return SF_OK;
    const RmTile t = rm_tile(d.H, d.W, d.Cout, n);
    const int64_t groups = ((n + t.S - 1) / t.S) * t.nrt * t.nct;
    SF_REQUIRE(groups <= 0x7fffffffLL, "sf_res_conv_dgrad_mfma: %lld work-groups", (long long)groups);
    rm_launch<true>(d.Cin, dim3((unsigned)groups), (size_t)rm_tile_bytes(t, t.S, t.TH), STREAM(stream), dout, w, nullptr, pre,
                    g_add, din, nullptr, d.act_in, 0, n, (int64_t)d.H * d.W * d.Cout, 0, d.H, d.W, d.Cout, t);
    return sf_launch_status("sf_res_conv_dgrad_mfma");
}

extern "C" int64_t sf_res_conv_wgrad_mfma_workspace(int64_t n, const sf_res_desc *h_desc) {
    if (!h_desc || n < 0 || !res_mfma_width(h_desc->Cin) || !res_mfma_width(h_desc->Cout) || h_desc->H < 1 || h_desc->W < 1)
        return 0;
    RwBand t;
    if (!rw_band(h_desc->H, h_desc->W, h_desc->Cin, h_desc->Cout, n, &t)) return 0;
    return t.parts * (9LL * h_desc->Cin * h_desc->Cout + h_desc->Cout) * (int64_t)sizeof(float);
}

extern "C" int sf_res_conv_wgrad_mfma(const void *in, int64_t in_sample_stride, const int32_t *index, int64_t offset,
                                      const float *dout, float *dw, float *db, int64_t n, const sf_res_desc *h_desc,
                                      void *workspace, int64_t workspace_bytes, void *stream) {
    int rc = rm_check(h_desc, "sf_res_conv_wgrad_mfma");
    if (rc) return rc;
    const sf_res_desc &d = *h_desc;
    SF_REQUIRE(in && dout && dw && db, "sf_res_conv_wgrad_mfma: NULL operand");
    SF_REQUIRE(index == nullptr, "sf_res_conv_wgrad_mfma: index addressing is for the raw u8 frames only");
    SF_REQUIRE(n >= 0 && offset >= 0, "sf_res_conv_wgrad_mfma: n=%lld offset=%lld", (long long)n, (long long)offset);
    SF_REQUIRE(in_sample_stride >= (int64_t)d.Cin * d.H * d.W && (in_sample_stride & 3) == 0,
               "sf_res_conv_wgrad_mfma: in_sample_stride %lld (at least Cin*H*W, a multiple of 4)", (long long)in_sample_stride);
    SF_REQUIRE(aligned16(in) && aligned16(dout), "sf_res_conv_wgrad_mfma: in and dout must be 16-byte aligned");
    RwBand t;
    if (!rw_band(d.H, d.W, d.Cin, d.Cout, n, &t)) {
        snprintf(sf_err_buf, sizeof(sf_err_buf), "sf_res_conv_wgrad_mfma: a row of W=%d pixels x (Cin=%d, Cout=%d) exceeds the "
                 "%d-byte LDS band", d.W, d.Cin, d.Cout, RM_LDS_BUDGET);
        return SF_ERR_UNSUPPORTED;
    }
    const int KC = 9 * d.Cin * d.Cout, E = KC + d.Cout;
    const int64_t need = t.parts * E * (int64_t)sizeof(float);
    SF_REQUIRE(workspace && workspace_bytes >= need, "sf_res_conv_wgrad_mfma: workspace %lld bytes < %lld",
               (long long)workspace_bytes, (long long)need);
    hipStream_t s = STREAM(stream);
    float *part = static_cast<float *>(workspace);
    const dim3 grid((unsigned)t.parts, (unsigned)t.blocks);
    const int ncog = d.Cout >= 64 ? 4 : d.Cout / 16;
    const dim3 block((unsigned)(t.ciw * ncog * 64));
#define RW_GO(NCOG, CT)                                                                                                 \
    hipLaunchKernelGGL((k_res_wgrad_mfma<NCOG, CT>), grid, block, (size_t)t.lds_bytes, s, (const float *)in, dout, part,  \
                       d.act_in, n, in_sample_stride, offset, d.H, d.W, d.Cin, t)
    if (d.Cout == 16) RW_GO(1, 1);
    else if (d.Cout == 32) RW_GO(2, 1);
    else if (d.Cout == 64) RW_GO(4, 1);
    else RW_GO(4, 2);
#undef RW_GO
    rc = sf_launch_status("sf_res_conv_wgrad_mfma (partials)");
    if (rc) return rc;
    return sf_res_wgrad_sum_launch(part, (int)t.parts, KC, d.Cout, dw, db, s);
}
