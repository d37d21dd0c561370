// sf_resnet.hip — the resnet_impala encoder (model/encoder.py:153-221 of the reference) for gfx950: 3x3 same-padded
// conv forward / data gradient / weight gradient and the 3x3 / 2 / pad 1 max-pool forward / backward.
// Reference op sequences replaced by each entry point are cited in include/sf_hip.h.
//
// Layout as in the rest of the library: activations NHWC, weights K-major [9*Cin, Cout] with k = (kh*3 + kw)*Cin + c.
// The widths are the ones the architecture fixes (Cout in {16, 32}; the data gradient also needs Cin in {16, 32});
// the first layer takes any Cin <= 32 and reads the raw u8 NCHW frames in place.
//
// Compiled with -ffp-contract=off: the dot products use explicit fmaf (as every GEMM library does), every other op
// (bias, residual add, activation derivative, gradient add) rounds after each op in torch's order.
#include "sf_common.h"

#define STREAM(s) reinterpret_cast<hipStream_t>(s)

namespace {

constexpr int RES_BLOCK = 256;
constexpr int RES_MAX_K = 9 * 32;         // 3x3 taps x at most 32 input channels
constexpr int RES_WG_TILE = 16;           // output pixels staged per weight-gradient step
constexpr int RES_WG_MAX_PARTS = 1024;    // partial sums of the two-stage weight-gradient reduction

struct ResG {
    int Cin, H, W, Cout, act_in, traj_T;
    int64_t stride, offset;
    float sub_mean, inv_scale;
    const float *nmu, *nrstd;  // sf_res_conv_fwd_norm / _wgrad_norm: the observation normaliser's f32 tables [Cin*H*W], else NULL
};

__device__ __forceinline__ float act_fwd(int kind, float z) {
    switch (kind) {
        case 1: return fmaxf(z, 0.0f);
        case 2: return tanhf(z);
        case 3: return z > 0.0f ? z : expm1f(z);
        default: return z;
    }
}

// derivative of the activation at the PRE-activation value z (torch's elu_backward / tanh_backward / threshold_backward)
__device__ __forceinline__ float act_grad(int kind, float z) {
    switch (kind) {
        case 1: return z > 0.0f ? 1.0f : 0.0f;
        case 2: { const float t = tanhf(z); return 1.0f - t * t; }
        case 3: return z > 0.0f ? 1.0f : expf(z);
        default: return 1.0f;
    }
}

// element offset of sample `smp`'s first input element: dataset row index[smp] | offset + smp, slab row d + d / traj_T
__device__ __forceinline__ int64_t res_sample_base(const ResG &g, const int32_t *__restrict__ index, int64_t smp) {
    int64_t d = index ? (int64_t)index[smp] : g.offset + smp;
    if (g.traj_T > 0) d += d / g.traj_T;
    return d * g.stride;
}

// one input value in the NORMALISED, ACTIVATED domain; the zero padding belongs to that domain (torch pads the
// normalised f32 tensor), so an out-of-image tap is exactly 0 — also under the observation normaliser, whose
// clamp((v - mu) * rstd, +-5) (running_mean_std.py:108) is applied to in-image pixels only
template <bool U8>
__device__ __forceinline__ float res_load(const void *__restrict__ x, const ResG &g, int64_t base, int h, int w, int c) {
    if (h < 0 || h >= g.H || w < 0 || w >= g.W) return 0.0f;
    float v;
    if (U8) {
        const int e = (c * g.H + h) * g.W + w;
        const float raw = (float)((const uint8_t *)x)[base + e];
        v = (raw - g.sub_mean) * g.inv_scale;
        if (g.nmu) v = fminf(fmaxf((v - g.nmu[e]) * g.nrstd[e], -5.0f), 5.0f);
    } else {
        v = ((const float *)x)[base + ((int64_t)h * g.W + w) * g.Cin + c];
    }
    return act_fwd(g.act_in, v);
}

// ------------------------------------------------------------------------------------------------ conv forward
// One thread per output pixel, all COUT outputs in registers; the weights live in LDS (every lane of a wave reads the
// same row: broadcast).  out = [res +] (conv(act(x)) + bias); out_act (optional) = act_out(out).
template <int COUT, bool U8>
__global__ __launch_bounds__(RES_BLOCK) void k_res_conv_fwd(const void *__restrict__ x, const int32_t *__restrict__ index,
                                                            const float *__restrict__ w, const float *__restrict__ bias,
                                                            const float *__restrict__ res, float *__restrict__ out,
                                                            float *__restrict__ out_act, int act_out, int64_t n, ResG g) {
    __shared__ float4 sw[RES_MAX_K * COUT / 4];
    const int K = 9 * g.Cin;
    for (int i = threadIdx.x; i < K * COUT / 4; i += RES_BLOCK) sw[i] = reinterpret_cast<const float4 *>(w)[i];
    __syncthreads();
    const int64_t HW = (int64_t)g.H * g.W;
    const int64_t pix = (int64_t)blockIdx.x * RES_BLOCK + threadIdx.x;
    if (pix >= n * HW) return;
    const int64_t smp = pix / HW;
    const int r = (int)(pix - smp * HW), oh = r / g.W, ow = r - oh * g.W;
    const int64_t base = res_sample_base(g, index, smp);
    float acc[COUT];
#pragma unroll
    for (int o = 0; o < COUT; ++o) acc[o] = 0.0f;
    for (int kh = 0; kh < 3; ++kh) {
        for (int kw = 0; kw < 3; ++kw) {
            const int h = oh + kh - 1, ww = ow + kw - 1;
            const float4 *wrow = sw + (kh * 3 + kw) * g.Cin * (COUT / 4);
            for (int c = 0; c < g.Cin; ++c) {
                const float v = res_load<U8>(x, g, base, h, ww, c);
#pragma unroll
                for (int q = 0; q < COUT / 4; ++q) {
                    const float4 wv = wrow[c * (COUT / 4) + q];
                    acc[4 * q + 0] = fmaf(v, wv.x, acc[4 * q + 0]);
                    acc[4 * q + 1] = fmaf(v, wv.y, acc[4 * q + 1]);
                    acc[4 * q + 2] = fmaf(v, wv.z, acc[4 * q + 2]);
                    acc[4 * q + 3] = fmaf(v, wv.w, acc[4 * q + 3]);
                }
            }
        }
    }
    float4 *o4 = reinterpret_cast<float4 *>(out + pix * COUT);
    float4 *a4 = out_act ? reinterpret_cast<float4 *>(out_act + pix * COUT) : nullptr;
    const float4 *r4 = res ? reinterpret_cast<const float4 *>(res + pix * COUT) : nullptr;
#pragma unroll
    for (int q = 0; q < COUT / 4; ++q) {
        float4 y = make_float4(acc[4 * q] + bias[4 * q], acc[4 * q + 1] + bias[4 * q + 1], acc[4 * q + 2] + bias[4 * q + 2],
                               acc[4 * q + 3] + bias[4 * q + 3]);
        if (r4) {
            const float4 s = r4[q];
            y = make_float4(s.x + y.x, s.y + y.y, s.z + y.z, s.w + y.w);
        }
        o4[q] = y;
        if (a4) a4[q] = make_float4(act_fwd(act_out, y.x), act_fwd(act_out, y.y), act_fwd(act_out, y.z), act_fwd(act_out, y.w));
    }
}

// ------------------------------------------------------------------------------------------------ max-pool 3x3/2/1
// One thread per output element.  Padding is -inf; torch's rule: a tap replaces the running maximum when it is
// greater or NaN, so the first maximum in (kh, kw) order wins; the index starts at the first in-image tap.
__global__ __launch_bounds__(RES_BLOCK) void k_res_pool_fwd(const float *__restrict__ x, float *__restrict__ y,
                                                            uint8_t *__restrict__ arg, int64_t n, int H, int W, int C,
                                                            int OH, int OW) {
    const int64_t i = (int64_t)blockIdx.x * RES_BLOCK + threadIdx.x;
    if (i >= n * OH * OW * C) return;
    const int c = (int)(i % C);
    const int64_t p = i / C;
    const int ow = (int)(p % OW);
    const int64_t q = p / OW;
    const int oh = (int)(q % OH);
    const int64_t smp = q / OH;
    const float *xs = x + smp * H * W * C + c;
    float m = -INFINITY;
    int best = -1;
    for (int kh = 0; kh < 3; ++kh) {
        const int h = 2 * oh - 1 + kh;
        if (h < 0 || h >= H) continue;
        for (int kw = 0; kw < 3; ++kw) {
            const int w = 2 * ow - 1 + kw;
            if (w < 0 || w >= W) continue;
            const float v = xs[((int64_t)h * W + w) * C];
            if (best < 0) best = kh * 3 + kw;
            if (v > m || isnan(v)) {
                m = v;
                best = kh * 3 + kw;
            }
        }
    }
    y[i] = m;
    arg[i] = (uint8_t)best;
}

// One thread per INPUT element: it gathers from the <= 2x2 windows that can contain it, in (oh, ow) order.
__global__ __launch_bounds__(RES_BLOCK) void k_res_pool_bwd(const float *__restrict__ gy, const uint8_t *__restrict__ arg,
                                                            float *__restrict__ gx, int64_t n, int H, int W, int C,
                                                            int OH, int OW) {
    const int64_t i = (int64_t)blockIdx.x * RES_BLOCK + threadIdx.x;
    if (i >= n * H * W * C) return;
    const int c = (int)(i % C);
    const int64_t p = i / C;
    const int w = (int)(p % W);
    const int64_t q = p / W;
    const int h = (int)(q % H);
    const int64_t smp = q / H;
    const int64_t obase = smp * OH * OW;
    float s = 0.0f;
    for (int oh = h / 2; oh <= min((h + 1) / 2, OH - 1); ++oh) {
        for (int ow = w / 2; ow <= min((w + 1) / 2, OW - 1); ++ow) {
            const int64_t o = ((obase + (int64_t)oh * OW + ow) * C) + c;
            if (arg[o] == (h - 2 * oh + 1) * 3 + (w - 2 * ow + 1)) s += gy[o];
        }
    }
    gx[i] = s;
}

// ------------------------------------------------------------------------------------------------ conv data gradient
// gx[n,h,w,c] = sum_{kh,kw,o} gy[n, h+1-kh, w+1-kw, o] * W[(kh*3+kw)*CIN + c, o], times act'(pre[n,h,w,c]), plus g_add.
// One thread per input pixel, all CIN outputs in registers; weights in LDS.
template <int CIN, int COUT>
__global__ __launch_bounds__(RES_BLOCK) void k_res_conv_dgrad(const float *__restrict__ gy, const float *__restrict__ w,
                                                              const float *__restrict__ pre, const float *__restrict__ g_add,
                                                              float *__restrict__ gx, int act_kind, int64_t n, int H, int W) {
    __shared__ float4 sw[9 * CIN * COUT / 4];
    for (int i = threadIdx.x; i < 9 * CIN * COUT / 4; i += RES_BLOCK) sw[i] = reinterpret_cast<const float4 *>(w)[i];
    __syncthreads();
    const int64_t HW = (int64_t)H * W;
    const int64_t pix = (int64_t)blockIdx.x * RES_BLOCK + threadIdx.x;
    if (pix >= n * HW) return;
    const int64_t smp = pix / HW;
    const int r = (int)(pix - smp * HW), h = r / W, ww = r - h * W;
    float acc[CIN];
#pragma unroll
    for (int c = 0; c < CIN; ++c) acc[c] = 0.0f;
    for (int kh = 0; kh < 3; ++kh) {
        const int oh = h + 1 - kh;
        if (oh < 0 || oh >= H) continue;
        for (int kw = 0; kw < 3; ++kw) {
            const int ow = ww + 1 - kw;
            if (ow < 0 || ow >= W) continue;
            const float4 *g4 = reinterpret_cast<const float4 *>(gy + ((smp * HW) + (int64_t)oh * W + ow) * COUT);
            float gv[COUT];
#pragma unroll
            for (int q = 0; q < COUT / 4; ++q) {
                const float4 t = g4[q];
                gv[4 * q] = t.x; gv[4 * q + 1] = t.y; gv[4 * q + 2] = t.z; gv[4 * q + 3] = t.w;
            }
            const float4 *wrow = sw + (kh * 3 + kw) * CIN * (COUT / 4);
#pragma unroll
            for (int c = 0; c < CIN; ++c) {
                float a = acc[c];
#pragma unroll
                for (int q = 0; q < COUT / 4; ++q) {
                    const float4 wv = wrow[c * (COUT / 4) + q];
                    a = fmaf(gv[4 * q], wv.x, a);
                    a = fmaf(gv[4 * q + 1], wv.y, a);
                    a = fmaf(gv[4 * q + 2], wv.z, a);
                    a = fmaf(gv[4 * q + 3], wv.w, a);
                }
                acc[c] = a;
            }
        }
    }
    const int64_t o = pix * CIN;
#pragma unroll
    for (int c = 0; c < CIN; ++c) {
        float v = acc[c];
        if (act_kind) v = v * act_grad(act_kind, pre[o + c]);
        if (g_add) v = g_add[o + c] + v;
        gx[o + c] = v;
    }
}

// ------------------------------------------------------------------------------------------------ conv weight gradient
// Stage 1: block b reduces the output pixels [b*rows, (b+1)*rows) of the batch into partial[b][e], e = k*COUT + o
// (weights) and 9*Cin*COUT + o (bias); RES_WG_TILE pixels at a time are staged in LDS (input patches in the activated,
// normalised domain, and the output gradient rows).  Stage 2 sums the partials in block order: no float atomics, the
// result depends only on the shapes.
template <int COUT, bool U8>
__global__ __launch_bounds__(RES_BLOCK) void k_res_conv_wgrad_part(const void *__restrict__ x,
                                                                   const int32_t *__restrict__ index,
                                                                   const float *__restrict__ gy,
                                                                   float *__restrict__ part, int64_t n, int64_t rows,
                                                                   ResG g) {
    constexpr int EPT = (RES_MAX_K * COUT + COUT + RES_BLOCK - 1) / RES_BLOCK;
    __shared__ float sp[RES_WG_TILE][RES_MAX_K];
    __shared__ float sg[RES_WG_TILE][COUT];
    const int K = 9 * g.Cin, E = K * COUT + COUT;
    const int64_t HW = (int64_t)g.H * g.W, NP = n * HW;
    const int64_t p0 = (int64_t)blockIdx.x * rows;
    const int64_t p1 = min(p0 + rows, NP);
    float acc[EPT];
#pragma unroll
    for (int j = 0; j < EPT; ++j) acc[j] = 0.0f;
    for (int64_t t0 = p0; t0 < p1; t0 += RES_WG_TILE) {
        const int np = (int)min((int64_t)RES_WG_TILE, p1 - t0);
        __syncthreads();
        for (int i = threadIdx.x; i < np * K; i += RES_BLOCK) {
            const int pp = i / K, k = i - pp * K;
            const int tap = k / g.Cin, c = k - tap * g.Cin, kh = tap / 3, kw = tap - kh * 3;
            const int64_t pix = t0 + pp, smp = pix / HW;
            const int r = (int)(pix - smp * HW), oh = r / g.W, ow = r - oh * g.W;
            sp[pp][k] = res_load<U8>(x, g, res_sample_base(g, index, smp), oh + kh - 1, ow + kw - 1, c);
        }
        for (int i = threadIdx.x; i < np * COUT; i += RES_BLOCK) sg[i / COUT][i % COUT] = gy[t0 * COUT + i];
        __syncthreads();
#pragma unroll
        for (int j = 0; j < EPT; ++j) {
            const int e = threadIdx.x + j * RES_BLOCK;
            if (e < E) {
                const int k = e / COUT, o = e - k * COUT;
                float a = acc[j];
                if (k < K) {
                    for (int pp = 0; pp < np; ++pp) a = fmaf(sp[pp][k], sg[pp][o], a);
                } else {
                    for (int pp = 0; pp < np; ++pp) a = a + sg[pp][o];
                }
                acc[j] = a;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < EPT; ++j) {
        const int e = threadIdx.x + j * RES_BLOCK;
        if (e < E) part[(int64_t)blockIdx.x * E + e] = acc[j];
    }
}

__global__ __launch_bounds__(RES_BLOCK) void k_res_conv_wgrad_sum(const float *__restrict__ part, int parts, int KC, int Cout,
                                                                  float *__restrict__ gw, float *__restrict__ gb) {
    const int e = blockIdx.x * RES_BLOCK + threadIdx.x;
    const int E = KC + Cout;
    if (e >= E) return;
    float s = 0.0f;
    for (int b = 0; b < parts; ++b) s += part[(int64_t)b * E + e];
    if (e < KC) gw[e] = s;
    else gb[e - KC] = s;
}

int res_check(const sf_res_desc *d, bool need_inner) {
    SF_REQUIRE(d != nullptr, "sf_res_*: desc is NULL");
    SF_REQUIRE(d->H >= 1 && d->W >= 1 && d->Cin >= 1, "sf_res_*: bad geometry Cin=%d H=%d W=%d", d->Cin, d->H, d->W);
    SF_REQUIRE(d->act_in >= 0 && d->act_in <= 3, "sf_res_*: act_in=%d not in 0..3", d->act_in);
    SF_REQUIRE(d->traj_T >= 0, "sf_res_*: traj_T=%d", d->traj_T);
    if (d->Cout != 16 && d->Cout != 32) {
        snprintf(sf_err_buf, sizeof(sf_err_buf), "sf_res_*: Cout=%d (16 or 32 only)", d->Cout);
        return SF_ERR_UNSUPPORTED;
    }
    if (d->Cin > 32 || (need_inner && d->Cin != 16 && d->Cin != 32)) {
        snprintf(sf_err_buf, sizeof(sf_err_buf), "sf_res_*: Cin=%d unsupported here", d->Cin);
        return SF_ERR_UNSUPPORTED;
    }
    return SF_OK;
}

ResG res_geom(const sf_res_desc *d, int64_t stride, int64_t offset) {
    ResG g;
    g.Cin = d->Cin; g.H = d->H; g.W = d->W; g.Cout = d->Cout; g.act_in = d->act_in; g.traj_T = d->traj_T;
    g.stride = stride; g.offset = offset; g.sub_mean = d->sub_mean; g.inv_scale = d->inv_scale;
    g.nmu = nullptr; g.nrstd = nullptr;
    return g;
}

// partial sums of the weight gradient over np output pixels: at most RES_WG_MAX_PARTS, every one of them non-empty
int64_t res_wgrad_parts(int64_t np) {
    if (np <= 0) return 1;
    const int64_t parts = min((int64_t)RES_WG_MAX_PARTS, (np + 255) / 256);
    const int64_t rows = (np + parts - 1) / parts;
    return (np + rows - 1) / rows;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

// mu / rstd: the observation normaliser's tables (sf_res_conv_fwd_norm), else NULL
static int res_conv_fwd_impl(const void *in, int64_t in_sample_stride, const int32_t *index, int64_t offset,
                             const float *w, const float *bias, const float *residual, float *out, float *out_act,
                             int act_out, int64_t n, const sf_res_desc *h_desc, void *stream, const float *mu,
                             const float *rstd) {
    int rc = res_check(h_desc, false);
    if (rc) return rc;
    SF_REQUIRE(in && w && bias && out, "sf_res_conv_fwd: NULL operand");
    SF_REQUIRE(n >= 0 && offset >= 0, "sf_res_conv_fwd: n=%lld offset=%lld", (long long)n, (long long)offset);
    SF_REQUIRE(act_out >= 0 && act_out <= 3, "sf_res_conv_fwd: act_out=%d", act_out);
    const sf_res_desc &d = *h_desc;
    const int64_t elems = (int64_t)d.Cin * d.H * d.W;
    SF_REQUIRE(in_sample_stride >= elems, "sf_res_conv_fwd: in_sample_stride %lld < %lld", (long long)in_sample_stride,
               (long long)elems);
    SF_REQUIRE(d.in_u8 || (index == nullptr && d.traj_T == 0),
               "sf_res_conv_fwd: index / traj_T addressing is for the raw u8 frames only");
    SF_REQUIRE(aligned16(w) && aligned16(out) && (!out_act || aligned16(out_act)) && (!residual || aligned16(residual)),
               "sf_res_conv_fwd: w, out, out_act and residual must be 16-byte aligned");
    if (n == 0) return SF_OK;
    ResG g = res_geom(h_desc, in_sample_stride, offset);
    g.nmu = mu; g.nrstd = rstd;
    const dim3 grid((unsigned)((n * d.H * d.W + RES_BLOCK - 1) / RES_BLOCK));
    hipStream_t s = STREAM(stream);
#define RES_FWD(CO, U8)                                                                                             \
    hipLaunchKernelGGL((k_res_conv_fwd<CO, U8>), grid, dim3(RES_BLOCK), 0, s, in, index, w, bias, residual, out, out_act, \
                       act_out, n, g)
    if (d.Cout == 16) {
        if (d.in_u8) RES_FWD(16, true); else RES_FWD(16, false);
    } else {
        if (d.in_u8) RES_FWD(32, true); else RES_FWD(32, false);
    }
#undef RES_FWD
    return sf_launch_status("sf_res_conv_fwd");
}

extern "C" int sf_res_conv_fwd(const void *in, int64_t in_sample_stride, const int32_t *index, int64_t offset,
                               const float *w, const float *bias, const float *residual, float *out, float *out_act,
                               int act_out, int64_t n, const sf_res_desc *h_desc, void *stream) {
    return res_conv_fwd_impl(in, in_sample_stride, index, offset, w, bias, residual, out, out_act, act_out, n, h_desc,
                             stream, nullptr, nullptr);
}

// the raw-frame first layer with cfg.normalize_input: the u8 frames are normalised in the loader (res_load), the zero
// padding stays zero; mu / rstd: the normaliser's f32 tables [Cin*H*W] in the frame's NCHW order
extern "C" int sf_res_conv_fwd_norm(const void *in, int64_t in_sample_stride, const int32_t *index, int64_t offset,
                                    const float *mu, const float *rstd, const float *w, const float *bias, float *out,
                                    int64_t n, const sf_res_desc *h_desc, void *stream) {
    SF_REQUIRE(h_desc && h_desc->in_u8 && mu && rstd, "sf_res_conv_fwd_norm: the raw u8 frame layer and both tables are needed");
    SF_REQUIRE(((uintptr_t)mu & 3) == 0 && ((uintptr_t)rstd & 3) == 0, "sf_res_conv_fwd_norm: tables must be 4-byte aligned");
    return res_conv_fwd_impl(in, in_sample_stride, index, offset, w, bias, nullptr, out, nullptr, 0, n, h_desc, stream, mu,
                             rstd);
}

extern "C" int sf_res_pool_fwd(const float *in, float *out, uint8_t *argmax, int64_t n, int H, int W, int C,
                               void *stream) {
    SF_REQUIRE(in && out && argmax, "sf_res_pool_fwd: NULL operand");
    SF_REQUIRE(n >= 0 && H >= 1 && W >= 1 && C >= 1, "sf_res_pool_fwd: n=%lld H=%d W=%d C=%d", (long long)n, H, W, C);
    const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
    const int64_t total = n * OH * OW * C;
    if (total == 0) return SF_OK;
    hipLaunchKernelGGL(k_res_pool_fwd, dim3((unsigned)((total + RES_BLOCK - 1) / RES_BLOCK)), dim3(RES_BLOCK), 0,
                       STREAM(stream), in, out, argmax, n, H, W, C, OH, OW);
    return sf_launch_status("sf_res_pool_fwd");
}

extern "C" int sf_res_pool_bwd(const float *dout, const uint8_t *argmax, float *din, int64_t n, int H, int W, int C,
                               void *stream) {
    SF_REQUIRE(dout && argmax && din, "sf_res_pool_bwd: NULL operand");
    SF_REQUIRE(n >= 0 && H >= 1 && W >= 1 && C >= 1, "sf_res_pool_bwd: n=%lld H=%d W=%d C=%d", (long long)n, H, W, C);
    const int OH = (H - 1) / 2 + 1, OW = (W - 1) / 2 + 1;
    const int64_t total = n * H * W * C;
    if (total == 0) return SF_OK;
    hipLaunchKernelGGL(k_res_pool_bwd, dim3((unsigned)((total + RES_BLOCK - 1) / RES_BLOCK)), dim3(RES_BLOCK), 0,
                       STREAM(stream), dout, argmax, din, n, H, W, C, OH, OW);
    return sf_launch_status("sf_res_pool_bwd");
}

extern "C" int sf_res_conv_dgrad(const float *dout, const float *w, const float *pre, const float *g_add, float *din,
                                 int64_t n, const sf_res_desc *h_desc, void *stream) {
    int rc = res_check(h_desc, true);
    if (rc) return rc;
    SF_REQUIRE(dout && w && din, "sf_res_conv_dgrad: NULL operand");
    SF_REQUIRE(!h_desc->act_in || pre, "sf_res_conv_dgrad: act_in=%d needs the pre-activation input", h_desc->act_in);
    SF_REQUIRE(!h_desc->in_u8, "sf_res_conv_dgrad: the raw-frame layer has no data gradient");
    SF_REQUIRE(n >= 0, "sf_res_conv_dgrad: n=%lld", (long long)n);
    SF_REQUIRE(aligned16(w) && aligned16(dout), "sf_res_conv_dgrad: w and dout must be 16-byte aligned");
    if (n == 0) return SF_OK;
    const sf_res_desc &d = *h_desc;
    const dim3 grid((unsigned)((n * d.H * d.W + RES_BLOCK - 1) / RES_BLOCK));
    hipStream_t s = STREAM(stream);
#define RES_DG(CI, CO) \
    hipLaunchKernelGGL((k_res_conv_dgrad<CI, CO>), grid, dim3(RES_BLOCK), 0, s, dout, w, pre, g_add, din, d.act_in, n, d.H, d.W)
    if (d.Cin == 16 && d.Cout == 16) RES_DG(16, 16);
    else if (d.Cin == 16) RES_DG(16, 32);
    else if (d.Cout == 16) RES_DG(32, 16);
    else RES_DG(32, 32);
#undef RES_DG
    return sf_launch_status("sf_res_conv_dgrad");
}

extern "C" int64_t sf_res_conv_wgrad_workspace(int64_t n, const sf_res_desc *h_desc) {
    if (!h_desc || n < 0) return 0;
    const int64_t E = 9LL * h_desc->Cin * h_desc->Cout + h_desc->Cout;
    return res_wgrad_parts(n * h_desc->H * h_desc->W) * E * (int64_t)sizeof(float);
}

// mu / rstd: the observation normaliser's tables (sf_res_conv_wgrad_norm), else NULL
static int res_conv_wgrad_impl(const void *in, int64_t in_sample_stride, const int32_t *index, int64_t offset,
                               const float *dout, float *dw, float *db, int64_t n, const sf_res_desc *h_desc,
                               void *workspace, int64_t workspace_bytes, void *stream, const float *mu,
                               const float *rstd) {
    int rc = res_check(h_desc, false);
    if (rc) return rc;
    SF_REQUIRE(in && dout && dw && db, "sf_res_conv_wgrad: NULL operand");
    SF_REQUIRE(n >= 0 && offset >= 0, "sf_res_conv_wgrad: n=%lld offset=%lld", (long long)n, (long long)offset);
    const sf_res_desc &d = *h_desc;
    const int64_t elems = (int64_t)d.Cin * d.H * d.W;
    SF_REQUIRE(in_sample_stride >= elems, "sf_res_conv_wgrad: in_sample_stride %lld < %lld", (long long)in_sample_stride,
               (long long)elems);
    SF_REQUIRE(d.in_u8 || (index == nullptr && d.traj_T == 0),
               "sf_res_conv_wgrad: index / traj_T addressing is for the raw u8 frames only");
    const int64_t need = sf_res_conv_wgrad_workspace(n, h_desc);
    SF_REQUIRE(workspace && workspace_bytes >= need, "sf_res_conv_wgrad: workspace %lld bytes < %lld",
               (long long)workspace_bytes, (long long)need);
    const int KC = 9 * d.Cin * d.Cout, E = KC + d.Cout;
    hipStream_t s = STREAM(stream);
    const int64_t NP = n * d.H * d.W;
    const int64_t parts = res_wgrad_parts(NP);
    const int64_t rows = NP > 0 ? (NP + parts - 1) / parts : 0;
    float *part = static_cast<float *>(workspace);
    ResG g = res_geom(h_desc, in_sample_stride, offset);
    g.nmu = mu; g.nrstd = rstd;
#define RES_WG(CO, U8)                                                                                          \
    hipLaunchKernelGGL((k_res_conv_wgrad_part<CO, U8>), dim3((unsigned)parts), dim3(RES_BLOCK), 0, s, in, index, dout, \
                       part, n, rows, g)
    if (d.Cout == 16) {
        if (d.in_u8) RES_WG(16, true); else RES_WG(16, false);
    } else {
        if (d.in_u8) RES_WG(32, true); else RES_WG(32, false);
    }
#undef RES_WG
    rc = sf_launch_status("sf_res_conv_wgrad (partials)");
    if (rc) return rc;
    hipLaunchKernelGGL(k_res_conv_wgrad_sum, dim3((unsigned)((E + RES_BLOCK - 1) / RES_BLOCK)), dim3(RES_BLOCK), 0, s,
                       part, (int)parts, KC, d.Cout, dw, db);
    return sf_launch_status("sf_res_conv_wgrad");
}

extern "C" int sf_res_conv_wgrad(const void *in, int64_t in_sample_stride, const int32_t *index, int64_t offset,
                                 const float *dout, float *dw, float *db, int64_t n, const sf_res_desc *h_desc,
                                 void *workspace, int64_t workspace_bytes, void *stream) {
    return res_conv_wgrad_impl(in, in_sample_stride, index, offset, dout, dw, db, n, h_desc, workspace, workspace_bytes,
                               stream, nullptr, nullptr);
}

extern "C" int sf_res_conv_wgrad_norm(const void *in, int64_t in_sample_stride, const int32_t *index, int64_t offset,
                                      const float *mu, const float *rstd, const float *dout, float *dw, float *db,
                                      int64_t n, const sf_res_desc *h_desc, void *workspace, int64_t workspace_bytes,
                                      void *stream) {
    SF_REQUIRE(h_desc && h_desc->in_u8 && mu && rstd, "sf_res_conv_wgrad_norm: the raw u8 frame layer and both tables are needed");
    SF_REQUIRE(((uintptr_t)mu & 3) == 0 && ((uintptr_t)rstd & 3) == 0, "sf_res_conv_wgrad_norm: tables must be 4-byte aligned");
    return res_conv_wgrad_impl(in, in_sample_stride, index, offset, dout, dw, db, n, h_desc, workspace, workspace_bytes,
                               stream, mu, rstd);
}
