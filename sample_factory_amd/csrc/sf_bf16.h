// sf_bf16.h — what the translation units of the bf16 matrix-pipe families share (sf_resnet_bf16.hip, sf_resnet_bf16_c16.hip,
// sf_conv_bf16.hip, sf_conv1_bf16.hip, sf_linear_bf16.hip): the MFMA operand types, the rounding of eight floats to one
// operand, the activation derivative of the data gradients' epilogues, and the host arithmetic of the tile plans.
#pragma once
#include "sf_common.h"

namespace {

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// eight floats rounded to nearest-even bf16: one A or B operand of v_mfma_f32_16x16x32_bf16
__device__ __forceinline__ bf16x8 bf16_pack(const float4 &a, const float4 &b) {
    bf16x8 r;
    r[0] = (__bf16)a.x; r[1] = (__bf16)a.y; r[2] = (__bf16)a.z; r[3] = (__bf16)a.w;
    r[4] = (__bf16)b.x; r[5] = (__bf16)b.y; r[6] = (__bf16)b.z; r[7] = (__bf16)b.w;
    return r;
}

// the operand of the bias gradient's MFMA: the sum of the rounded dout
__device__ __forceinline__ bf16x8 bf16_ones8() {
    bf16x8 r;
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = (__bf16)1.0f;
    return r;
}

// derivative of the activation through its OUTPUT y (sf_conv_dgrad's contract: in_act is the stored activation)
__device__ __forceinline__ float act_bwd_out(int kind, float y) {
    switch (kind) {
        case 1: return y > 0.0f ? 1.0f : 0.0f;
        case 2: return 1.0f - y * y;
        case 3: return y > 0.0f ? 1.0f : y + 1.0f;
        default: return 1.0f;
    }
}

template <typename T>  // int or int64_t: both operands of one type, the caller says which where they differ
inline T ceil_div(T a, T b) { return (a + b - 1) / b; }

// x (a multiple of 8) or x + 8, whichever is an ODD multiple of 8: an LDS pitch in bf16 elements that is an odd number of
// 16-byte words
inline int odd8(int x) { return ((x >> 3) & 1) ? x : x + 8; }

}  // namespace
