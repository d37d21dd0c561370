// sf_conv1_bf16.hip — the raw-frame conv layer of convnet_simple / convnet_atari / convnet_impala on
// v_mfma_f32_16x16x32_bf16 (cfg.encoder_conv1_bf16): u8 or f32 NCHW frames (sf_conv_desc.in_u8 = 1 / 2), 8x8 stride 4,
// Cin 1 .. 16, Cout in {16, 32}, with or without the observation normaliser's tables.  Reached by name only
// (sf_conv1_*_bf16); sf_conv_fwd, sf_conv_wgrad, sf_conv_*_norm and sf_conv_kernel_name never route here.
//
// Arithmetic (DESIGN.md 3.23's contract): x' = clamp(((float(px) - sub_mean) * inv_scale - mu[d]) * rstd[d], +-5), without
// tables (float(px) - sub_mean) * inv_scale; every operation rounded to fp32 (-ffp-contract=off), x' rounded ONCE to bf16
// (nearest even) where the pixel enters LDS.  bf16(w) and bf16(dout) are rounded once; accumulation, bias and activation are
// fp32; db is the sum of the rounded dout.  The vector and the scalar loader run the same operations per pixel.
//
// Forward (k_conv1_fwd_bf16): implicit GEMM, M = output pixels, N = Cout, reduction Cin * 64.  With the frame weight order
// k = (c*8 + kh)*8 + kw, the 8 consecutive k of a lane are one tap row, i.e. 8 contiguous pixels of one input row, and the
// four lane groups are four consecutive tap rows: one channel is two MFMAs per 16 pixels and 16-column slice.
//   * A work-group (4 waves) is persistent over bands.  A band is TR output rows of one sample (4*TR + 4 input rows of every
//     channel), or S whole samples where S * OH*OW <= 256.  It is staged as bf16 [sample][c][row][P]; x' is formed once per
//     staged pixel.  P is an odd multiple of 32 elements: the four tap rows of a lane group start 64 bytes apart mod 128.
//   * A pixel's window starts at column 4*ow: 8-byte aligned.  A fragment is two 8-byte LDS reads (one ds_read2_b64).
//   * The weights are converted once per work-group and stay in LDS in fragment order: block ((c*2 + h)*NS + u) holds, for
//     lane l, W[c*64 + (4h + l/16)*8 + 0..7][u*16 + l%16]: one conflict-free ds_read_b128, shared by the FW = 4 fragments a
//     wave holds at a time.
//   * The MFMA is issued transposed (weights as A, pixels as B): a lane then holds 4 consecutive channels of one pixel and
//     the output leaves as 16-byte stores.
//   * An element's reduction order is (c, tap-row half, the MFMA's own order): it depends on neither n nor the sample's
//     place in a band.  No split-K.
//
// Weight gradient (k_conv1_wgrad_bf16): M = k, N = Cout, reduction over the output pixels of the batch, 32 per MFMA; a lane
// holds 8 consecutive output pixels (a "run") of one (c, kh, kw).  In the raw row that is a stride-4 walk, so the band is
// staged de-interleaved: copy kw of input row r holds x'[r][4*j + kw] at position j, rows padded with zeros to OWp (an
// odd multiple of 8).  A thread loads 36 consecutive pixels (9 words on the vector path), forms x' once for each and writes
// the 8 runs they make, one 16-byte store per kw.  dout is staged channel-major and rounded once per band, zeros behind the
// end of every output row: a ragged run never reaches into another row.  Wave w owns tap rows 2w, 2w+1 (16 k) of every
// channel: acc[c][slice]; the four lane groups take four runs.  db is one more MFMA against ones (wave 0).  Bands are
// dealt to parts in order; partials go to [parts][Cin*64*Cout + Cout] and k_res_conv_wgrad_sum adds them in part order: no
// float atomics.  A part holds at least C1_PART_PIXELS output pixels, so a small layer at large n does not pay for
// hundreds of partials.
#include "sf_common.h"
#include "sf_resnet_shared.h"
#include "sf_bf16.h"

#include <algorithm>

#define STREAM(s) reinterpret_cast<hipStream_t>(s)

namespace {

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

constexpr int C1_K = 8, C1_ST = 4;
constexpr int C1_FW = 4;                    // fragments a wave holds at a time (forward)
constexpr int C1_TILE_M = 256;              // output pixels of a multi-sample band
constexpr int C1_LDS_SMALL = 64 * 1024;     // two work-groups per CU
constexpr int C1_LDS_LARGE = 128 * 1024;    // one work-group per CU: 16-channel weights, wide images
constexpr int C1_GRID = 512;                // persistent work-groups of the forward
constexpr int C1_MAX_PARTS = 512;
constexpr int C1_PART_PIXELS = 4096;        // floor on the output pixels of a weight-gradient part

extern __shared__ float4 c1_lds4[];

struct C1Geo {
    int Cin, H, W, OH, OW, Cout, traj_T, act;
    float sub_mean, inv_scale;
};

struct C1Tile {
    int S, TR, nrt;   // samples of a band; output rows of a band; bands per image
    int LH;           // staged input rows of a sample: 4*TR + 4
    int P;            // forward: elements per staged row.  weight gradient: OWp, elements per (row, kw) copy
    int RPR, GP;      // weight gradient: runs per output row; elements per staged dout channel
    int wbytes;       // forward: bytes of the resident weights
    int lds;          // dynamic LDS bytes
    int64_t nb;       // bands of the launch
    int64_t bpp, parts;  // weight gradient: bands per part, parts
    FastDiv dcols, dLH, dCin, dRPR, dTR;
};

inline int c1_odd(int x, int unit) { x = ceil_div(x, unit); return (x | 1) * unit; }  // smallest odd multiple of unit >= x

inline bool c1_served(const sf_conv_desc *d) {
    if (!d || (d->in_u8 != 1 && d->in_u8 != 2) || d->KH != C1_K || d->KW != C1_K || d->stride != C1_ST) return false;
    if (d->Cin < 1 || d->Cin > 16 || !(d->Cout == 16 || d->Cout == 32)) return false;
    if (d->H < C1_K || d->W < C1_K || (int64_t)d->Cin * d->H * d->W >= (1LL << 31)) return false;
    if (d->OH != (d->H - C1_K) / C1_ST + 1 || d->OW != (d->W - C1_K) / C1_ST + 1) return false;
    return d->relu >= 0 && d->relu <= 3 && d->traj_T >= 0;
}

// false: a band of one output row does not fit LDS (the image is too wide)
bool c1_tile(const sf_conv_desc &d, bool wgrad, int64_t n, C1Tile *out) {
    C1Tile t = {};
    const int NS = d.Cout / 16;
    t.wbytes = wgrad ? 0 : d.Cin * 2 * NS * 1024;
    t.P = wgrad ? c1_odd(d.OW, 8) : c1_odd(d.W, 32);
    t.RPR = t.P / 8;
    auto lh = [](int TR) { return C1_ST * TR + C1_K - C1_ST; };
    auto bytes = [&](int S, int TR) {
        if (!wgrad) return (int64_t)t.wbytes + (int64_t)S * d.Cin * lh(TR) * t.P * 2;
        return (int64_t)S * d.Cin * lh(TR) * C1_K * t.P * 2 + (int64_t)d.Cout * c1_odd(S * TR * t.P, 8) * 2;
    };
    int budget = C1_LDS_SMALL;
    if (bytes(1, 1) > budget) budget = C1_LDS_LARGE;
    if (bytes(1, 1) > budget) return false;
    int TR = d.OH;
    while (TR > 1 && bytes(1, TR) > budget) --TR;
    t.nrt = ceil_div(d.OH, TR);
    t.TR = ceil_div(d.OH, t.nrt);
    t.S = 1;
    if (t.nrt == 1)
        while (t.S < n && (t.S + 1) * d.OH * d.OW <= C1_TILE_M && bytes(t.S + 1, t.TR) <= budget) ++t.S;
    t.LH = lh(t.TR);
    t.GP = c1_odd(t.S * t.TR * t.P, 8);
    t.lds = (int)bytes(t.S, t.TR);
    t.nb = ((n + t.S - 1) / t.S) * t.nrt;
    // parts: at most C1_MAX_PARTS, each at least C1_PART_PIXELS output pixels
    const int64_t band_px = (int64_t)t.S * t.TR * d.OW;
    t.bpp = std::max<int64_t>({1, (t.nb + C1_MAX_PARTS - 1) / C1_MAX_PARTS, (C1_PART_PIXELS + band_px - 1) / band_px});
    t.parts = std::max<int64_t>(1, (t.nb + t.bpp - 1) / t.bpp);
    t.dLH = make_fastdiv((uint32_t)t.LH);
    t.dCin = make_fastdiv((uint32_t)d.Cin);
    t.dRPR = make_fastdiv((uint32_t)t.RPR);
    t.dTR = make_fastdiv((uint32_t)t.TR);
    *out = t;
    return true;
}

// the input value of the contract, every operation rounded to fp32
__device__ __forceinline__ float c1_x(float px, const C1Geo &g, bool norm, float mu, float rstd) {
    float v = px - g.sub_mean;
    v = v * g.inv_scale;
    if (norm) {
        v = v - mu;
        v = v * rstd;
        v = fminf(fmaxf(v, -5.0f), 5.0f);
    }
    return v;
}

__device__ __forceinline__ int64_t c1_sample(const C1Geo &g, const int32_t *__restrict__ index, int64_t offset, int64_t stride,
                                             int64_t smp) {
    int64_t d = index ? (int64_t)index[smp] : offset + smp;
    if (g.traj_T > 0) d += d / g.traj_T;
    return d * stride;
}

// four consecutive pixels of one frame row, from element offset e (vector path: e is a multiple of 4 and the base aligned)
template <bool U8>
__device__ __forceinline__ void c1_load4(const void *__restrict__ in, int64_t e, float (&px)[4]) {
    if (U8) {
        const uint32_t wd = *reinterpret_cast<const uint32_t *>(static_cast<const uint8_t *>(in) + e);
        px[0] = (float)(wd & 255u); px[1] = (float)((wd >> 8) & 255u); px[2] = (float)((wd >> 16) & 255u); px[3] = (float)(wd >> 24);
    } else {
        const float4 f = *reinterpret_cast<const float4 *>(static_cast<const float *>(in) + e);
        px[0] = f.x; px[1] = f.y; px[2] = f.z; px[3] = f.w;
    }
}
template <bool U8>
__device__ __forceinline__ float c1_load1(const void *__restrict__ in, int64_t e) {
    return U8 ? (float)static_cast<const uint8_t *>(in)[e] : static_cast<const float *>(in)[e];
}

// ------------------------------------------------------------------------------------------------ forward
template <int NS, bool U8>
__global__ __launch_bounds__(256) void k_conv1_fwd_bf16(const void *__restrict__ in, int64_t stride,
                                                        const int32_t *__restrict__ index, int64_t offset,
                                                        const float *__restrict__ mu, const float *__restrict__ rstd,
                                                        const float *__restrict__ w, const float *__restrict__ bias,
                                                        float *__restrict__ out, int64_t n, int vec, C1Geo g, C1Tile t) {
    __bf16 *wl = reinterpret_cast<__bf16 *>(c1_lds4);
    __bf16 *xl = wl + (t.wbytes >> 1);
    const int Cin = g.Cin, H = g.H, W = g.W, OH = g.OH, OW = g.OW, LH = t.LH, P = t.P;
    constexpr int Cout = 16 * NS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lg = lane >> 4;
    const bool norm = mu != nullptr;
    // ---- weights -> LDS as bf16, in fragment order, once per work-group
    for (int i = threadIdx.x; i < Cin * 2 * NS * 64; i += 256) {
        const int l = i & 63, blk = i >> 6, u = blk % NS, ch = blk / NS, h = ch & 1, c = ch >> 1;
        const float *p = w + (c * 64 + (4 * h + (l >> 4)) * 8) * Cout + u * 16 + (l & 15);
        bf16x8 r;
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = (__bf16)p[j * Cout];
        *reinterpret_cast<bf16x8 *>(wl + i * 8) = r;
    }
    float4 b4[NS];
#pragma unroll
    for (int u = 0; u < NS; ++u)
        b4[u] = make_float4(bias[u * 16 + 4 * lg], bias[u * 16 + 4 * lg + 1], bias[u * 16 + 4 * lg + 2], bias[u * 16 + 4 * lg + 3]);
    const int cols = vec ? W >> 2 : W;  // staged items of a row
    const int items = t.S * Cin * LH * cols;
    for (int64_t band = blockIdx.x; band < t.nb; band += gridDim.x) {
        const int rt = (int)(band % t.nrt), r0 = rt * t.TR;
        const int64_t s0 = (band / t.nrt) * t.S;
        const int ns = (int)min((int64_t)t.S, n - s0), rows_c = min(t.TR, OH - r0);
        __syncthreads();  // the previous band's fragments have been read
        // ---- frame rows -> LDS as bf16: x' formed once per pixel; zeros past the image and past the last sample
        for (int i = threadIdx.x; i < items; i += 256) {
            const uint32_t r1 = fdiv((uint32_t)i, t.dcols), q = (uint32_t)i - r1 * (uint32_t)cols;
            const uint32_t r2 = fdiv(r1, t.dLH), row = r1 - r2 * (uint32_t)LH;
            const uint32_t s = fdiv(r2, t.dCin), c = r2 - s * (uint32_t)Cin;
            const int h = C1_ST * r0 + (int)row;
            const bool live = (int)s < ns && h < H;
            __bf16 *dst = xl + ((s * Cin + c) * LH + row) * P;
            if (vec) {
                bf16x4 o = {(__bf16)0.0f, (__bf16)0.0f, (__bf16)0.0f, (__bf16)0.0f};
                if (live) {
                    const int d = ((int)c * H + h) * W + 4 * (int)q;
                    float px[4];
                    c1_load4<U8>(in, c1_sample(g, index, offset, stride, s0 + s) + d, px);
                    float4 m4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r4 = m4;
                    if (norm) {
                        m4 = *reinterpret_cast<const float4 *>(mu + d);
                        r4 = *reinterpret_cast<const float4 *>(rstd + d);
                    }
                    o[0] = (__bf16)c1_x(px[0], g, norm, m4.x, r4.x);
                    o[1] = (__bf16)c1_x(px[1], g, norm, m4.y, r4.y);
                    o[2] = (__bf16)c1_x(px[2], g, norm, m4.z, r4.z);
                    o[3] = (__bf16)c1_x(px[3], g, norm, m4.w, r4.w);
                }
                *reinterpret_cast<bf16x4 *>(dst + 4 * q) = o;
            } else {
                __bf16 o = (__bf16)0.0f;
                if (live) {
                    const int d = ((int)c * H + h) * W + (int)q;
                    const float px = c1_load1<U8>(in, c1_sample(g, index, offset, stride, s0 + s) + d);
                    o = (__bf16)c1_x(px, g, norm, norm ? mu[d] : 0.0f, norm ? rstd[d] : 0.0f);
                }
                dst[q] = o;
            }
        }
        __syncthreads();
        // ---- fragments round-robin over the waves, FW at a time against one read of the weights
        const int PC = rows_c * OW, M = ns * PC, nfr = (M + 15) >> 4;
        for (int c0 = 0; c0 * C1_FW * 4 + wave < nfr; ++c0) {  // (wave-uniform; no barrier below)
            int hb[C1_FW];
            floatx4 acc[C1_FW][NS];
#pragma unroll
            for (int f = 0; f < C1_FW; ++f) {
                int m = ((c0 * C1_FW + f) * 4 + wave) * 16 + lr;
                if (m >= M) m = 0;  // a lane past the band reads a real pixel; its column is never stored
                const int s = m / PC, r = (m - s * PC) / OW, ow = m - s * PC - r * OW;
                hb[f] = (s * Cin * LH + C1_ST * r + lg) * P + C1_ST * ow;
#pragma unroll
                for (int u = 0; u < NS; ++u) acc[f][u] = (floatx4){0.0f, 0.0f, 0.0f, 0.0f};
            }
            for (int ch = 0; ch < 2 * Cin; ++ch) {  // (c, h): tap rows 4h .. 4h + 3 of channel c
                const int aoff = ((ch >> 1) * LH + 4 * (ch & 1)) * P;
                bf16x8 bw[NS];
#pragma unroll
                for (int u = 0; u < NS; ++u) bw[u] = *reinterpret_cast<const bf16x8 *>(wl + ((ch * NS + u) * 64 + lane) * 8);
#pragma unroll
                for (int f = 0; f < C1_FW; ++f) {
                    if ((c0 * C1_FW + f) * 4 + wave < nfr) {
                        const bf16x4 lo = *reinterpret_cast<const bf16x4 *>(xl + hb[f] + aoff);
                        const bf16x4 hi = *reinterpret_cast<const bf16x4 *>(xl + hb[f] + aoff + 4);
                        const bf16x8 a = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
                        for (int u = 0; u < NS; ++u) acc[f][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bw[u], a, acc[f][u], 0, 0, 0);
                    }
                }
            }
            // ---- epilogue: accumulator j of fragment f, slice u is channel u*16 + 4*lg + j of pixel 16*fragment + lr
#pragma unroll
            for (int f = 0; f < C1_FW; ++f) {
                const int m = ((c0 * C1_FW + f) * 4 + wave) * 16 + lr;
                if (m >= M) continue;
                const int s = m / PC, r = (m - s * PC) / OW, ow = m - s * PC - r * OW;
                float *po = out + (((s0 + s) * OH + r0 + r) * OW + ow) * Cout + 4 * lg;
#pragma unroll
                for (int u = 0; u < NS; ++u) {
                    float4 v;
                    v.x = act_fwd(g.act, acc[f][u][0] + b4[u].x);
                    v.y = act_fwd(g.act, acc[f][u][1] + b4[u].y);
                    v.z = act_fwd(g.act, acc[f][u][2] + b4[u].z);
                    v.w = act_fwd(g.act, acc[f][u][3] + b4[u].w);
                    *reinterpret_cast<float4 *>(po + u * 16) = v;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ weight gradient
// CB: channels the accumulators are sized for (Cin <= CB)
template <int NS, int CB, bool U8>
__global__ __launch_bounds__(256) void k_conv1_wgrad_bf16(const void *__restrict__ in, int64_t stride,
                                                          const int32_t *__restrict__ index, int64_t offset,
                                                          const float *__restrict__ mu, const float *__restrict__ rstd,
                                                          const float *__restrict__ gy, float *__restrict__ part, int64_t n,
                                                          int vec, C1Geo g, C1Tile t) {
    constexpr int Cout = 16 * NS;
    const int Cin = g.Cin, H = g.H, W = g.W, OH = g.OH, OW = g.OW, LH = t.LH, OWp = t.P, RPR = t.RPR, GP = t.GP, TR = t.TR;
    __bf16 *xl = reinterpret_cast<__bf16 *>(c1_lds4);
    __bf16 *gl = xl + t.S * Cin * LH * C1_K * OWp;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lg = lane >> 4;
    const bool norm = mu != nullptr;
    const __bf16 zero = (__bf16)0.0f;
    floatx4 acc[CB][NS], accb[NS];
#pragma unroll
    for (int u = 0; u < NS; ++u) {
        accb[u] = (floatx4){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int c = 0; c < CB; ++c) acc[c][u] = (floatx4){0.0f, 0.0f, 0.0f, 0.0f};
    }
    const bf16x8 ones8 = bf16_ones8();
    bf16x8 zero8;
#pragma unroll
    for (int k = 0; k < 8; ++k) zero8[k] = zero;
    // the lane's A row: k = c*64 + 16*wave + lr, i.e. tap row 2*wave + lr/8, tap column lr%8
    const int arow = ((2 * wave + (lr >> 3)) * C1_K + (lr & 7)) * OWp;
    const int64_t b0 = (int64_t)blockIdx.x * t.bpp, b1 = min(t.nb, b0 + t.bpp);
    const int xitems = t.S * Cin * LH * RPR, gitems = t.S * TR * RPR * (Cout >> 2);
    for (int64_t band = b0; band < b1; ++band) {
        const int rt = (int)(band % t.nrt), r0 = rt * TR;
        const int64_t s0 = (band / t.nrt) * t.S;
        const int ns = (int)min((int64_t)t.S, n - s0), rows_c = min(TR, OH - r0);
        __syncthreads();  // the previous band's fragments have been read
        // ---- frame rows -> LDS, de-interleaved: 36 consecutive pixels make run rq of the 8 copies of their row
        for (int i = threadIdx.x; i < xitems; i += 256) {
            const uint32_t r1 = fdiv((uint32_t)i, t.dRPR), rq = (uint32_t)i - r1 * (uint32_t)RPR;
            const uint32_t r2 = fdiv(r1, t.dLH), row = r1 - r2 * (uint32_t)LH;
            const uint32_t s = fdiv(r2, t.dCin), c = r2 - s * (uint32_t)Cin;
            const int h = C1_ST * r0 + (int)row, q0 = 8 * (int)rq;
            __bf16 pb[36];
#pragma unroll
            for (int e = 0; e < 36; ++e) pb[e] = zero;
            if ((int)s < ns && h < H) {
                const int d0 = ((int)c * H + h) * W + 4 * q0;
                const int64_t e0 = c1_sample(g, index, offset, stride, s0 + s) + d0;
#pragma unroll
                for (int qq = 0; qq < 9; ++qq) {
                    const int col = 4 * (q0 + qq);
                    if (vec) {
                        if (col < W) {
                            float px[4];
                            c1_load4<U8>(in, e0 + 4 * qq, px);
                            float4 m4 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r4 = m4;
                            if (norm) {
                                m4 = *reinterpret_cast<const float4 *>(mu + d0 + 4 * qq);
                                r4 = *reinterpret_cast<const float4 *>(rstd + d0 + 4 * qq);
                            }
                            pb[4 * qq + 0] = (__bf16)c1_x(px[0], g, norm, m4.x, r4.x);
                            pb[4 * qq + 1] = (__bf16)c1_x(px[1], g, norm, m4.y, r4.y);
                            pb[4 * qq + 2] = (__bf16)c1_x(px[2], g, norm, m4.z, r4.z);
                            pb[4 * qq + 3] = (__bf16)c1_x(px[3], g, norm, m4.w, r4.w);
                        }
                    } else {
#pragma unroll
                        for (int p = 0; p < 4; ++p) {
                            if (col + p < W) {
                                const int d = d0 + 4 * qq + p;
                                pb[4 * qq + p] = (__bf16)c1_x(c1_load1<U8>(in, e0 + 4 * qq + p), g, norm, norm ? mu[d] : 0.0f,
                                                              norm ? rstd[d] : 0.0f);
                            }
                        }
                    }
                }
            }
            __bf16 *dst = xl + (((s * Cin + c) * LH + row) * C1_K) * OWp + q0;
#pragma unroll
            for (int kw = 0; kw < C1_K; ++kw) {
                bf16x8 o;
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = q0 + e < OW ? pb[4 * e + kw] : zero;  // position j reads column 4*j + kw
                *reinterpret_cast<bf16x8 *>(dst + kw * OWp) = o;
            }
        }
        // ---- dout -> LDS, channel-major, rounded once; zeros behind every row's end, past the image and the batch
        for (int i = threadIdx.x; i < gitems; i += 256) {
            const int oq = i % (Cout >> 2), run = i / (Cout >> 2);
            const uint32_t sr = fdiv((uint32_t)run, t.dRPR), rq = (uint32_t)run - sr * (uint32_t)RPR;
            const uint32_t s = fdiv(sr, t.dTR), r = sr - s * (uint32_t)TR;
            const bool live = (int)s < ns && (int)r < rows_c;
            const float *p = gy + (((s0 + s) * OH + r0 + r) * OW + 8 * rq) * Cout + 4 * oq;
            __bf16 v[8][4];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float4 f = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (live && 8 * (int)rq + e < OW) f = *reinterpret_cast<const float4 *>(p + e * Cout);
                v[e][0] = (__bf16)f.x; v[e][1] = (__bf16)f.y; v[e][2] = (__bf16)f.z; v[e][3] = (__bf16)f.w;
            }
#pragma unroll
            for (int cc = 0; cc < 4; ++cc) {
                bf16x8 o;
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = v[e][cc];
                *reinterpret_cast<bf16x8 *>(gl + (4 * oq + cc) * GP + run * 8) = o;
            }
        }
        __syncthreads();
        // ---- 4 runs (32 output pixels) per MFMA: lane group lg takes run 4*it + lg
        const int nruns = ((ns - 1) * TR + rows_c) * RPR;
        for (int it = 0; 4 * it < nruns; ++it) {
            const int run = 4 * it + lg;
            const bool ok = run < nruns;
            const uint32_t rr = ok ? (uint32_t)run : 0u;
            const uint32_t sr = fdiv(rr, t.dRPR), rq = rr - sr * (uint32_t)RPR;
            const uint32_t s = fdiv(sr, t.dTR), r = sr - s * (uint32_t)TR;
            bf16x8 b[NS];
#pragma unroll
            for (int u = 0; u < NS; ++u) {
                b[u] = *reinterpret_cast<const bf16x8 *>(gl + (u * 16 + lr) * GP + rr * 8);
                if (!ok) b[u] = zero8;
            }
            const __bf16 *xa = xl + ((s * Cin) * LH + C1_ST * r) * C1_K * OWp + arow + 8 * rq;
#pragma unroll
            for (int c = 0; c < CB; ++c) {
                if (c < Cin) {
                    bf16x8 a = *reinterpret_cast<const bf16x8 *>(xa + c * LH * C1_K * OWp);
                    if (!ok) a = zero8;
#pragma unroll
                    for (int u = 0; u < NS; ++u) acc[c][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[u], acc[c][u], 0, 0, 0);
                }
            }
            if (wave == 0) {
#pragma unroll
                for (int u = 0; u < NS; ++u) accb[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones8, b[u], accb[u], 0, 0, 0);
            }
        }
    }
    // accumulator j of (c, u): k = c*64 + 16*wave + 4*lg + j, output channel u*16 + lr
    const int KC = Cin * 64 * Cout;
    float *pp = part + (int64_t)blockIdx.x * (KC + Cout);
#pragma unroll
    for (int c = 0; c < CB; ++c) {
        if (c < Cin) {
#pragma unroll
            for (int u = 0; u < NS; ++u)
#pragma unroll
                for (int j = 0; j < 4; ++j) pp[(c * 64 + 16 * wave + 4 * lg + j) * Cout + u * 16 + lr] = acc[c][u][j];
        }
    }
    if (wave == 0 && lg == 0) {
#pragma unroll
        for (int u = 0; u < NS; ++u) pp[KC + u * 16 + lr] = accb[u][0];
    }
}

C1Geo c1_geo(const sf_conv_desc &d) {
    return C1Geo{d.Cin, d.H, d.W, d.OH, d.OW, d.Cout, d.traj_T, d.relu, d.sub_mean, d.inv_scale};
}

int c1_check(const sf_conv_desc *d, const char *what) {
    SF_REQUIRE(d != nullptr, "%s: desc is NULL", what);
    if (!c1_served(d)) {
        snprintf(sf_err_buf, sizeof(sf_err_buf),
                 "%s: Cin=%d Cout=%d kernel=%dx%d stride=%d H=%d W=%d OH=%d OW=%d in_u8=%d traj_T=%d relu=%d (the raw-frame bf16 "
                 "family serves u8 / f32 NCHW frames (in_u8 = 1, 2), 8x8 stride 4 without padding, Cin 1 .. 16, Cout in {16, 32})",
                 what, d->Cin, d->Cout, d->KH, d->KW, d->stride, d->H, d->W, d->OH, d->OW, d->in_u8, d->traj_T, d->relu);
        return SF_ERR_UNSUPPORTED;
    }
    return SF_OK;
}

int c1_too_wide(const sf_conv_desc &d, const char *what) {
    snprintf(sf_err_buf, sizeof(sf_err_buf), "%s: image too wide: one output row's band of a W=%d image (Cin=%d, Cout=%d) exceeds "
             "the %d-byte LDS budget", what, d.W, d.Cin, d.Cout, C1_LDS_LARGE);
    return SF_ERR_UNSUPPORTED;
}

// the operands both passes share; *vec: every load of the frames and the tables may be a vector load
int c1_operands(const char *what, const void *in, int64_t in_sample_stride, int64_t offset, const float *mu, const float *rstd,
                int64_t n, const sf_conv_desc &d, int *vec) {
    SF_REQUIRE(n >= 0 && offset >= 0, "%s: n=%lld offset=%lld", what, (long long)n, (long long)offset);
    SF_REQUIRE((mu == nullptr) == (rstd == nullptr), "%s: mu and rstd are both NULL or both set", what);
    SF_REQUIRE(in != nullptr, "%s: NULL operand", what);
    SF_REQUIRE(in_sample_stride >= (int64_t)d.Cin * d.H * d.W, "%s: in_sample_stride %lld < Cin*H*W", what,
               (long long)in_sample_stride);
    const bool u8 = d.in_u8 == 1;
    SF_REQUIRE(u8 || ((uintptr_t)in & 3) == 0, "%s: f32 frames must be 4-byte aligned", what);
    SF_REQUIRE(!mu || ((((uintptr_t)mu | (uintptr_t)rstd) & 3) == 0), "%s: the tables must be 4-byte aligned", what);
    const uintptr_t amask = u8 ? 3 : 15;
    *vec = d.W % 4 == 0 && ((uintptr_t)in & amask) == 0 && in_sample_stride % 4 == 0 &&
           (!mu || (((uintptr_t)mu | (uintptr_t)rstd) & 15) == 0);
    return SF_OK;
}

}  // namespace

extern "C" int sf_conv1_bf16_supported(int op, int64_t n, const sf_conv_desc *h_desc) {
    if (n < 0 || op < 0 || op > 1 || !c1_served(h_desc)) return 0;
    C1Tile t;
    return c1_tile(*h_desc, op == 1, n, &t) ? 1 : 0;
}

extern "C" int sf_conv1_fwd_bf16(const void *in, int64_t in_sample_stride, const int32_t *index, int64_t offset, const float *mu,
                                 const float *rstd, const float *w, const float *bias, float *out, int64_t n,
                                 const sf_conv_desc *h_desc, void *stream) {
    int rc = c1_check(h_desc, "sf_conv1_fwd_bf16");
    if (rc) return rc;
    const sf_conv_desc &d = *h_desc;
    C1Tile t;
    if (!c1_tile(d, false, n > 0 ? n : 1, &t)) return c1_too_wide(d, "sf_conv1_fwd_bf16");
    int vec = 0;
    rc = c1_operands("sf_conv1_fwd_bf16", in, in_sample_stride, offset, mu, rstd, n, d, &vec);
    if (rc) return rc;
    SF_REQUIRE(w && bias && out, "sf_conv1_fwd_bf16: NULL operand");
    SF_REQUIRE(((uintptr_t)w & 3) == 0 && aligned16(out), "sf_conv1_fwd_bf16: out must be 16-byte aligned");
    if (n == 0) return SF_OK;
    t.dcols = make_fastdiv((uint32_t)(vec ? d.W / 4 : d.W));
    const dim3 grid((unsigned)std::min<int64_t>(t.nb, t.lds > C1_LDS_SMALL ? C1_GRID / 2 : C1_GRID));
    const C1Geo g = c1_geo(d);
#define C1_FWD(NS, U8)                                                                                                 \
    hipLaunchKernelGGL((k_conv1_fwd_bf16<NS, U8>), grid, dim3(256), (size_t)t.lds, STREAM(stream), in, in_sample_stride, \
                       index, offset, mu, rstd, w, bias, out, n, vec, g, t)
    if (d.Cout == 16) { if (d.in_u8 == 1) C1_FWD(1, true); else C1_FWD(1, false); }
    else { if (d.in_u8 == 1) C1_FWD(2, true); else C1_FWD(2, false); }
#undef C1_FWD
    return sf_launch_status("sf_conv1_fwd_bf16");
}

extern "C" int64_t sf_conv1_wgrad_bf16_workspace(int64_t n, const sf_conv_desc *h_desc) {
    if (n < 0 || !c1_served(h_desc)) return 0;
    C1Tile t;
    if (!c1_tile(*h_desc, true, n > 0 ? n : 1, &t)) return 0;
    return t.parts * ((int64_t)h_desc->Cin * 64 * h_desc->Cout + h_desc->Cout) * (int64_t)sizeof(float);
}

extern "C" int sf_conv1_wgrad_bf16(const void *in, int64_t in_sample_stride, const int32_t *index, int64_t offset,
                                   const float *mu, const float *rstd, const float *dout, float *dw, float *db, int64_t n,
                                   const sf_conv_desc *h_desc, void *workspace, int64_t workspace_bytes, void *stream) {
    int rc = c1_check(h_desc, "sf_conv1_wgrad_bf16");
    if (rc) return rc;
    const sf_conv_desc &d = *h_desc;
    C1Tile t;
    if (!c1_tile(d, true, n > 0 ? n : 1, &t)) return c1_too_wide(d, "sf_conv1_wgrad_bf16");
    int vec = 0;
    rc = c1_operands("sf_conv1_wgrad_bf16", in, in_sample_stride, offset, mu, rstd, n, d, &vec);
    if (rc) return rc;
    SF_REQUIRE(dout && dw && db, "sf_conv1_wgrad_bf16: NULL operand");
    SF_REQUIRE(aligned16(dout) && aligned16(workspace), "sf_conv1_wgrad_bf16: dout and workspace must be 16-byte aligned");
    if (n == 0) return SF_OK;
    const int KC = d.Cin * 64 * d.Cout;
    const int64_t need = t.parts * (KC + d.Cout) * (int64_t)sizeof(float);
    SF_REQUIRE(workspace && workspace_bytes >= need, "sf_conv1_wgrad_bf16: workspace %lld bytes < %lld",
               (long long)workspace_bytes, (long long)need);
    hipStream_t s = STREAM(stream);
    float *part = static_cast<float *>(workspace);
    const dim3 grid((unsigned)t.parts);
    const C1Geo g = c1_geo(d);
#define C1_WG(NS, CB, U8)                                                                                              \
    hipLaunchKernelGGL((k_conv1_wgrad_bf16<NS, CB, U8>), grid, dim3(256), (size_t)t.lds, s, in, in_sample_stride, index, \
                       offset, mu, rstd, dout, part, n, vec, g, t)
#define C1_WG_CB(NS, U8)                                                                                               \
    do {                                                                                                               \
        if (d.Cin <= 4) C1_WG(NS, 4, U8);                                                                              \
        else if (d.Cin <= 8) C1_WG(NS, 8, U8);                                                                         \
        else C1_WG(NS, 16, U8);                                                                                        \
    } while (0)
    if (d.Cout == 16) { if (d.in_u8 == 1) C1_WG_CB(1, true); else C1_WG_CB(1, false); }
    else { if (d.in_u8 == 1) C1_WG_CB(2, true); else C1_WG_CB(2, false); }
#undef C1_WG_CB
#undef C1_WG
    rc = sf_launch_status("sf_conv1_wgrad_bf16 (partials)");
    if (rc) return rc;
    return sf_res_wgrad_sum_launch(part, (int)t.parts, KC, d.Cout, dw, db, s);
}
