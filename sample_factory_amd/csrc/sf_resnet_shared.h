// sf_resnet_shared.h — what the two translation units of the resnet_impala encoder share: sf_resnet.hip (fp32 FMA kernels,
// pools, entry-point routing) and sf_resnet_mfma.hip (the 3x3 conv family on v_mfma_f32_16x16x4_f32).
#pragma once
#include "sf_common.h"

// stage 2 of both weight gradients (defined in sf_resnet.hip): partial sums part[parts][KC + Cout] added in part order
int sf_res_wgrad_sum_launch(const float *part, int parts, int KC, int Cout, float *gw, float *gb, hipStream_t s);

// the bf16 family's kernels for 16 -> 16 and 16 -> 32 layers (defined in sf_resnet_bf16_c16.hip), behind sf_res_conv_*_bf16.
// conv_launch: Cr reduced, Cn produced channels; a1 / a2 = residual / unused (forward), pre / g_add (data gradient).
// wgrad_parts: rows of the [parts][9*16*Cout + Cout] workspace the launch fills; 0: a row of W pixels does not fit the band.
bool sf_res_c16_pair(int Cin, int Cout);
int sf_res_c16_conv_launch(bool dgrad, const float *in, int64_t in_stride, int64_t in_offset, const float *w, const float *bias,
                           const float *a1, const float *a2, float *out, float *out_act, int act, int act_out, int64_t n,
                           int H, int W, int Cr, int Cn, hipStream_t s);
int64_t sf_res_c16_wgrad_parts(int H, int W, int Cout, int64_t n);
int sf_res_c16_wgrad_launch(const float *x, int64_t in_stride, int64_t in_offset, const float *gy, float *part, int act,
                            int64_t n, int H, int W, int Cout, hipStream_t s);

namespace {

constexpr int RES_BLOCK = 256;

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

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

inline bool res_mfma_width(int c) { return c == 16 || c == 32 || c == 64 || c == 128; }

}  // namespace
