// sf_nn.hip — actor-critic network kernels for gfx950 (MI355X): one fp32-MFMA implicit-GEMM family
//   out[M,N] = epilogue( gather(A)[M,K] x B[K,N] )
// instantiated as conv/linear FORWARD, WEIGHT-GRADIENT (split over the reduction = sample/pixel axis, deterministic
// two-stage reduce) and DATA-GRADIENT (gather form, decomposed by stride-parity class so no MFMA work is spent on
// structurally-zero taps).  A dense layer is the 1x1 conv on a 1x1 image, so six reference ops share three kernels.
//
// Numerics: v_mfma_f32_32x32x2_f32 — f32 in, f32 accumulate, bit-equal to an fmaf chain (MI355X_MICROARCH.md), i.e.
// the same precision class as the reference's fp32 MIOpen/rocBLAS path.  No reduced precision anywhere.
//
// Data layout: activations NHWC ([sample][oh][ow][c] == row-major [M, C]); weights K-major [K, Cout] with
// k = (kh*KW + kw)*Cin + c (NHWC input) or k = (c*KH + kh)*KW + kw (raw NCHW observation frames, u8 or f32, so that
// four consecutive k are four consecutive pixels).  Observation frames are converted ((x - mean) * 1/scale) inside the
// loader: the f32 copy of the observations that the reference materialises (utils/normalize.py:40-70) never exists.
//
// Tile: 256 threads = 4 wavefronts (one per SIMD), block tile BM x BN x 32, LDS image As[32][BM+pad], Bs[32][BN+pad]
// (reduction-major => both MFMA fragment reads are 32 consecutive words, conflict-free), register prefetch of the next
// K-chunk while the current one is in the matrix pipe.
//
// Loaders are compile-time specialised (MODE) and BRANCH-FREE: out-of-range rows / columns / reduction indices load
// from a clamped, always-valid address and are zeroed with a select, so the compiler issues every global load of a
// chunk back-to-back and waits once (the first version branched per load and hipcc serialised them with vmcnt(0)).
#include "sf_common.h"
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>
#ifndef SF_GLDS_ABLATE
#define SF_GLDS_ABLATE 0  // timing experiments only (sf_nn_glds.h)
#endif
#include <type_traits>
#include <algorithm>

#define STREAM(s) reinterpret_cast<hipStream_t>(s)

typedef float f32x16 __attribute__((ext_vector_type(16)));

// (FastDiv / make_fastdiv / fdiv — exact n / d for n < 2^31 — live in sf_common.h: sf_ingest.hip divides with them too)
extern "C" int sf_selftest_host(void) {  // exercised by the CPU test-suite: the index math everything rests on
    const uint32_t ds[] = {1, 2, 3, 4, 6, 7, 9, 20, 32, 33, 49, 64, 81, 84, 128, 400, 512, 576, 3136, 7056, 28224, 65535, 1000003};
    for (uint32_t d : ds) {
        const FastDiv f = make_fastdiv(d);
        const uint32_t ns[] = {0, 1, d - 1, d, d + 1, 2 * d - 1, 2 * d, 12345678, 0x7FFFFFFFu, 0x7FFFFFFFu - d, 13107200, 13107199};
        for (uint32_t n : ns) if (fdiv(n, f) != n / d) return -1;
        for (uint32_t n = 0; n < 200000; n += 7) if (fdiv(n, f) != n / d) return -2;
        for (uint32_t n = 0x7FFFFFFFu; n > 0x7FFFFFFFu - 100000; n -= 13) if (fdiv(n, f) != n / d) return -3;
    }
    // sf_frame_resize (sf_ingest.hip) rounds its box average with them: (2 S + D) / (2 D) == (S + D / 2) / D for every
    // frame area D = H W <= 2^23 and every weighted sum S <= 255 D
    const uint32_t areas[] = {1, 2, 3, 35, 70, 96, 485, 5760, 19200, 33600, 76800, 921600, 8388607, 8388608};
    for (uint32_t D : areas) {
        const FastDiv f = make_fastdiv(D);
        for (uint64_t v = 0; v <= 255; ++v)
            for (int64_t off = -2; off <= 2; ++off) {  // sums around every tie v + 1/2 and around every whole v
                for (int tie = 0; tie < 2; ++tie) {
                    const int64_t S = (int64_t)((2 * v + tie) * D / 2) + off;
                    if (S < 0 || S > 255 * (int64_t)D) continue;
                    if (fdiv((uint32_t)S + D / 2, f) != (uint32_t)((2 * (uint64_t)S + D) / (2 * (uint64_t)D))) return -4;
                }
            }
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------- input formats
// sf_conv_desc.in_u8: 0 = f32 NHWC activations, 1 = u8 NCHW observation frames, 2 = f32 NCHW observation frames.
// Every test of the field goes through these two helpers (a plain truth test would take format 2 for u8).
constexpr int IN_F32_NHWC = 0, IN_U8_FRAME = 1, IN_F32_FRAME = 2;
__host__ __device__ __forceinline__ bool in_is_u8(int in_u8) { return in_u8 == IN_U8_FRAME; }
__host__ __device__ __forceinline__ bool in_is_frame(int in_u8) { return in_u8 == IN_U8_FRAME || in_u8 == IN_F32_FRAME; }

// ---------------------------------------------------------------------------------------------- geometry
struct ConvG {
    int Cin, H, W, Cout, KH, KW, S, OH, OW;
    int in_u8, relu, traj_T;
    float sub_mean, inv_scale;
    int K;          // KH*KW*Cin
    int vecA, vecB; // vector (16-byte / 4-byte-of-u8) loads legal for the activation / [*,Cout] operands
    const float *nmu, *nrstd;  // sf_conv_fwd_norm / sf_conv_wgrad_norm: the observation normaliser's f32 tables, else NULL
    FastDiv dOHOW, dOW, dCin, dKW, dKHKW, dT, dCout;
    FastDiv dHcWc[16], dWc[16], dKWs[16];  // data-gradient stride-parity classes (S*S <= 16)
};

static ConvG make_geom(const sf_conv_desc *d) {
    ConvG g;
    g.Cin = d->Cin; g.H = d->H; g.W = d->W; g.Cout = d->Cout; g.KH = d->KH; g.KW = d->KW; g.S = d->stride;
    g.OH = d->OH; g.OW = d->OW; g.in_u8 = d->in_u8; g.relu = d->relu; g.traj_T = d->traj_T;
    g.sub_mean = d->sub_mean; g.inv_scale = d->inv_scale;
    g.nmu = nullptr; g.nrstd = nullptr;
    g.K = d->KH * d->KW * d->Cin;
    // frames: four consecutive k are four consecutive pixels of one row, and every patch origin is a multiple of 4
    // pixels (4-byte words of u8, 16-byte float4 of f32 frames)
    g.vecA = in_is_frame(d->in_u8) ? (d->KW % 4 == 0 && d->stride % 4 == 0 && d->W % 4 == 0) : (d->Cin % 4 == 0);
    g.vecB = d->Cout % 4 == 0;
    g.dOHOW = make_fastdiv((uint32_t)(d->OH * d->OW));
    g.dOW = make_fastdiv((uint32_t)d->OW);
    g.dCin = make_fastdiv((uint32_t)d->Cin);
    g.dKW = make_fastdiv((uint32_t)d->KW);
    g.dKHKW = make_fastdiv((uint32_t)(d->KH * d->KW));
    g.dT = make_fastdiv((uint32_t)(d->traj_T > 0 ? d->traj_T : 1));
    g.dCout = make_fastdiv((uint32_t)d->Cout);
    for (int z = 0; z < 16; ++z) {
        const int S = d->stride, ph = z / S, pw = z % S;
        const int Hc = (d->H - ph + S - 1) / S, Wc = (d->W - pw + S - 1) / S, KWs = (d->KW - pw + S - 1) / S;
        const bool ok = z < S * S && Hc > 0 && Wc > 0;
        g.dHcWc[z] = make_fastdiv(ok ? (uint32_t)(Hc * Wc) : 1u);
        g.dWc[z] = make_fastdiv(ok ? (uint32_t)Wc : 1u);
        g.dKWs[z] = make_fastdiv(ok && KWs > 0 ? (uint32_t)KWs : 1u);
    }
    return g;
}

static int check_desc(const sf_conv_desc *d, const char *who) {
    SF_REQUIRE(d, "%s: null descriptor", who);
    SF_REQUIRE(d->Cin > 0 && d->H > 0 && d->W > 0 && d->Cout > 0 && d->KH > 0 && d->KW > 0 && d->stride > 0,
               "%s: bad geometry", who);
    SF_REQUIRE(d->OH == (d->H - d->KH) / d->stride + 1 && d->OW == (d->W - d->KW) / d->stride + 1,
               "%s: OH/OW do not match a VALID (no padding) convolution", who);
    SF_REQUIRE(d->in_u8 >= IN_F32_NHWC && d->in_u8 <= IN_F32_FRAME, "%s: in_u8 = %d is not an input format (0, 1, 2)",
               who, d->in_u8);
    return SF_OK;
}

// loader specialisations
constexpr int MODE_F32 = 0;      // f32 NHWC activations, Cin % 4 == 0, Cout % 4 == 0: 16-byte loads everywhere
constexpr int MODE_U8 = 1;       // raw u8 NCHW observation, KW/stride/W % 4 == 0: 4-byte loads of 4 pixels
constexpr int MODE_GENERIC = 2;  // any geometry: scalar, bounds-checked (slow; odd shapes only)
constexpr int MODE_F32F = 3;     // f32 NCHW observation frames, KW/stride/W % 4 == 0: 16-byte loads of 4 pixels
constexpr int MODE_F32F_NORM = 4;  // MODE_F32F + the observation normaliser's tables (sf_conv_fwd_norm / _wgrad_norm)
constexpr int MODE_U8_NORM = 5;    // MODE_U8 + the observation normaliser's tables: 4-byte load of 4 pixels, 16-byte loads of mu / rstd
// frames (u8 or f32): reduction index k = (c*KH + kh)*KW + kw over the NCHW frame, output rows fastest across lanes
template <int MODE>
constexpr bool frame_layout() {
    return MODE == MODE_U8 || MODE == MODE_F32F || MODE == MODE_F32F_NORM || MODE == MODE_U8_NORM;
}

// input-sample base offset (elements) of logical sample `smp`: optional index gather, optional dataset->trajectory
// slab row mapping (flat index e*T+t  ->  slab row e*(T+1)+t, learner.py:1005-1012 drops column T by *copy*; we
// read the slab in place instead).
__device__ __forceinline__ int64_t sample_base(const ConvG &g, const int32_t *__restrict__ index, int64_t offset,
                                               int64_t stride, uint32_t smp) {
    int64_t d = index ? (int64_t)index[smp] : offset + (int64_t)smp;
    if (g.traj_T > 0) d += (int64_t)fdiv((uint32_t)d, g.dT);  // e*(T+1) + (d - e*T)
    return d * stride;
}

// offset (elements) of im2col column k inside one input sample, relative to the patch origin
template <bool U8>
__device__ __forceinline__ int tap_offset(const ConvG &g, uint32_t k) {
    if (U8) {  // k = (c*KH + kh)*KW + kw over NCHW bytes
        const uint32_t c = fdiv(k, g.dKHKW), r = k - c * (uint32_t)(g.KH * g.KW);
        const uint32_t kh = fdiv(r, g.dKW), kw = r - kh * (uint32_t)g.KW;
        return (int)((c * (uint32_t)g.H + kh) * (uint32_t)g.W + kw);
    }
    const uint32_t tap = fdiv(k, g.dCin), c = k - tap * (uint32_t)g.Cin;  // k = (kh*KW + kw)*Cin + c over NHWC
    const uint32_t kh = fdiv(tap, g.dKW), kw = tap - kh * (uint32_t)g.KW;
    return (int)((kh * (uint32_t)g.W + kw) * (uint32_t)g.Cin + c);
}
// offset (elements) of output pixel `pix` patch origin inside one input sample
template <bool U8>
__device__ __forceinline__ int patch_origin(const ConvG &g, uint32_t pix) {
    const uint32_t oh = fdiv(pix, g.dOW), ow = pix - oh * (uint32_t)g.OW;
    const uint32_t o = oh * (uint32_t)g.S * (uint32_t)g.W + ow * (uint32_t)g.S;
    return (int)(U8 ? o : o * (uint32_t)g.Cin);
}

// activations (desc.relu carries the kind): 0 none, 1 ReLU, 2 tanh, 3 ELU(alpha=1) — model/model_utils.py:27-35
__device__ __forceinline__ float act_fwd(float x, int kind) {
    if (kind == 1) return fmaxf(x, 0.f);
    if (kind == 2) return tanhf(x);
    if (kind == 3) return x > 0.f ? x : expm1f(x);
    return x;
}
// derivative expressed through the activation OUTPUT y (what the backward chain has at hand)
__device__ __forceinline__ float act_bwd(float y, int kind) {
    if (kind == 1) return y > 0.f ? 1.f : 0.f;
    if (kind == 2) return 1.f - y * y;
    if (kind == 3) return y > 0.f ? 1.f : y + 1.f;
    return 1.f;
}

// v * act'(y) with the kind known at compile time (KIND 0: no activation, < 0: run-time kind)
template <int KIND>
__device__ __forceinline__ float act_bwd_mul(float v, float y, int kind) {
    if (KIND == 0) return v;
    if (KIND == 1) return y > 0.f ? v : 0.f;
    return v * act_bwd(y, kind);
}

// Raw (unconverted, unmasked) operand quads.  The value is NOT touched between the global load and the LDS store of
// the next iteration, so the loads stay in flight across the whole MFMA phase (a select right after the load made
// hipcc wait for the data before the first MFMA — no overlap at all).
template <int MODE>
struct ARaw {
    float4 v;
};
template <>
struct ARaw<MODE_U8> {
    uint32_t v;
};
template <>
struct ARaw<MODE_F32F_NORM> {
    float4 v, mu, rs;  // four pixels and their normaliser table entries
};
template <>
struct ARaw<MODE_U8_NORM> {
    uint32_t v;     // four u8 pixels
    float4 mu, rs;  // their normaliser table entries
};

// the observation normaliser applied to one converted pixel (running_mean_std.py:108: sub_(mu).mul_(1/sigma).clamp_(-5, 5))
__device__ __forceinline__ float obs_norm(float x, float mu, float rs) { return fminf(fmaxf((x - mu) * rs, -5.f), 5.f); }

// four consecutive im2col columns k..k+3 (k % 4 == 0, k < K) of the patch whose origin is `base`; po = that origin's
// offset inside its sample (frames with the normaliser: the index into the [Cin*H*W] tables)
template <int MODE>
__device__ __forceinline__ ARaw<MODE> load_act_raw(const ConvG &g, const void *__restrict__ in, int64_t base, int po,
                                                   uint32_t k, bool ok) {
    ARaw<MODE> r;
    if constexpr (MODE == MODE_U8) {
        r.v = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const uint8_t *>(in) + base + tap_offset<true>(g, k));
    } else if constexpr (MODE == MODE_U8_NORM) {
        const int t = tap_offset<true>(g, k);
        r.v = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const uint8_t *>(in) + base + t);
        r.mu = *reinterpret_cast<const float4 *>(g.nmu + po + t);
        r.rs = *reinterpret_cast<const float4 *>(g.nrstd + po + t);
    } else if constexpr (MODE == MODE_F32F || MODE == MODE_F32F_NORM) {
        const int t = tap_offset<true>(g, k);
        r.v = *reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(in) + base + t);
        if constexpr (MODE == MODE_F32F_NORM) {
            r.mu = *reinterpret_cast<const float4 *>(g.nmu + po + t);
            r.rs = *reinterpret_cast<const float4 *>(g.nrstd + po + t);
        }
    } else if constexpr (MODE == MODE_F32) {
        r.v = *reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(in) + base + tap_offset<false>(g, k));
    } else {
        float x[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool okj = ok && (k + j < (uint32_t)g.K);
            const uint32_t kj = okj ? k + j : 0u;
            if (in_is_frame(g.in_u8)) {
                const int t = tap_offset<true>(g, kj);
                const float raw = in_is_u8(g.in_u8) ? (float)reinterpret_cast<const uint8_t *>(in)[base + t]
                                                    : reinterpret_cast<const float *>(in)[base + t];
                x[j] = (raw - g.sub_mean) * g.inv_scale;
                if (g.nmu) x[j] = obs_norm(x[j], g.nmu[po + t], g.nrstd[po + t]);
            } else {
                x[j] = reinterpret_cast<const float *>(in)[base + tap_offset<false>(g, kj)];
            }
            x[j] = okj ? x[j] : 0.f;
        }
        r.v = make_float4(x[0], x[1], x[2], x[3]);
    }
    return r;
}
template <int MODE>
__device__ __forceinline__ float4 act_finish(const ConvG &g, const ARaw<MODE> &r, bool ok) {
    if constexpr (MODE == MODE_U8) {
        float x[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float t = ((float)((r.v >> (8 * j)) & 0xFFu) - g.sub_mean) * g.inv_scale;
            x[j] = ok ? t : 0.f;
        }
        return make_float4(x[0], x[1], x[2], x[3]);
    } else if constexpr (MODE == MODE_U8_NORM) {
        const float s = g.sub_mean, c = g.inv_scale;
        return make_float4(ok ? obs_norm(((float)(r.v & 0xFFu) - s) * c, r.mu.x, r.rs.x) : 0.f,
                           ok ? obs_norm(((float)((r.v >> 8) & 0xFFu) - s) * c, r.mu.y, r.rs.y) : 0.f,
                           ok ? obs_norm(((float)((r.v >> 16) & 0xFFu) - s) * c, r.mu.z, r.rs.z) : 0.f,
                           ok ? obs_norm(((float)(r.v >> 24) - s) * c, r.mu.w, r.rs.w) : 0.f);
    } else if constexpr (MODE == MODE_F32F) {
        const float s = g.sub_mean, c = g.inv_scale;
        return make_float4(ok ? (r.v.x - s) * c : 0.f, ok ? (r.v.y - s) * c : 0.f, ok ? (r.v.z - s) * c : 0.f,
                           ok ? (r.v.w - s) * c : 0.f);
    } else if constexpr (MODE == MODE_F32F_NORM) {
        const float s = g.sub_mean, c = g.inv_scale;
        return make_float4(ok ? obs_norm((r.v.x - s) * c, r.mu.x, r.rs.x) : 0.f,
                           ok ? obs_norm((r.v.y - s) * c, r.mu.y, r.rs.y) : 0.f,
                           ok ? obs_norm((r.v.z - s) * c, r.mu.z, r.rs.z) : 0.f,
                           ok ? obs_norm((r.v.w - s) * c, r.mu.w, r.rs.w) : 0.f);
    } else {
        return make_float4(ok ? r.v.x : 0.f, ok ? r.v.y : 0.f, ok ? r.v.z : 0.f, ok ? r.v.w : 0.f);
    }
}

// four consecutive columns n..n+3 of row `row` of a row-major [*, N] f32 matrix (row must be a valid row index even
// when the result is going to be masked).  VEC: N % 4 == 0 and n % 4 == 0 -> one 16-byte load; n >= N reads column 0.
template <bool VEC>
__device__ __forceinline__ float4 load_row_raw(const float *__restrict__ p, int64_t row, int n, int N) {
    if constexpr (VEC) {
        return *reinterpret_cast<const float4 *>(p + row * N + (n < N ? n : 0));
    } else {
        float x[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = p[row * N + (n + j < N ? n + j : 0)];
        return make_float4(x[0], x[1], x[2], x[3]);
    }
}
__device__ __forceinline__ float4 row_finish(const float4 &r, bool ok, int n, int N) {
    return make_float4((ok && n < N) ? r.x : 0.f, (ok && n + 1 < N) ? r.y : 0.f, (ok && n + 2 < N) ? r.z : 0.f,
                       (ok && n + 3 < N) ? r.w : 0.f);
}

// ---------------------------------------------------------------------------------------------- MFMA tile compute
// As: [32][LDA] (reduction-major), Bs: [32][LDB].  Wave (wm, wn) owns rows wm*TM*32.. and cols wn*TN*32..
template <int TM, int TN, int LDA, int LDB>
__device__ __forceinline__ void mma_chunk(const float *__restrict__ As, const float *__restrict__ Bs, int arow0,
                                          int bcol0, int lane, f32x16 (&acc)[TM][TN]) {
    // Fragments are double-buffered in registers, two k-steps ahead: the ds_reads of step kk+2 are issued before the
    // MFMAs of step kk, so the LDS latency hides under 2*TM*TN*64 cycles of matrix-pipe time instead of stalling
    // every MFMA pair behind an lgkmcnt(0) (what hipcc emitted for the naive loop).
    const int i = lane & 31, kh = lane >> 5;
    const float *ap = As + kh * LDA + arow0 + i;
    const float *bp = Bs + kh * LDB + bcol0 + i;
    float a[3][TM], b[3][TN];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) a[p][tm] = ap[(2 * p) * LDA + tm * 32];
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) b[p][tn] = bp[(2 * p) * LDB + tn * 32];
    }
#pragma unroll
    for (int st = 0; st < 16; ++st) {
        const int cur = st % 3, nxt = (st + 2) % 3;
        if (st + 2 < 16) {
#pragma unroll
            for (int tm = 0; tm < TM; ++tm) a[nxt][tm] = ap[(2 * (st + 2)) * LDA + tm * 32];
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) b[nxt][tn] = bp[(2 * (st + 2)) * LDB + tn * 32];
        }
        __builtin_amdgcn_sched_barrier(0);  // keep the prefetch reads ABOVE this step's MFMAs
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int tn = 0; tn < TN; ++tn)
                acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cur][tm], b[cur][tn], acc[tm][tn], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// C/D fragment: reg r of lane l holds (row = (r&3) + 8*(r>>2) + 4*(l>>5), col = l&31)  (cdna_hip_programming.md §3)
#define FRAG_ROW(r, lane) (((r) & 3) + 8 * ((r) >> 2) + 4 * ((lane) >> 5))

// act_fwd with the kind known at compile time (KIND < 0: run-time kind)
template <int KIND>
__device__ __forceinline__ float act_fwd_c(float x, int kind) {
    if (KIND == 0) return x;
    if (KIND == 1) return fmaxf(x, 0.f);
    return act_fwd(x, kind);
}

// Store one wave's TM x TN accumulator fragments (32x32x2 layout: row = (r&3) + 8*(r>>2) + 4*(lane>>5), col =
// lane&31) as act(acc + bias) into a row-major [rows][N] matrix.  ob = uniform pointer to the tile's (0, 0);
// voff = this lane's (4*(lane>>5))*N + (lane&31); rows_left / cols_left = number of existing rows / columns counted
// from THIS LANE's first row / column (FULL: the whole tile exists, no per-element test); bias0 = bias + tile column,
// lcol = lane&31.
template <int TM, int TN, int KIND, bool FULL>
__device__ __forceinline__ void store_fwd_tile(const f32x16 (&acc)[TM][TN], float *__restrict__ ob, uint32_t voff, int N,
                                               int rows_left, int cols_left, const float *__restrict__ bias0, int lcol,
                                               int kind) {
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
        const bool cok = FULL || tn * 32 < cols_left;
        const float bv = (bias0 && cok) ? bias0[tn * 32 + lcol] : 0.f;
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rr = tm * 32 + (r & 3) + 8 * (r >> 2);
                float *p = ob + (int64_t)rr * N + tn * 32;  // uniform
                const float v = act_fwd_c<KIND>(acc[tm][tn][r] + bv, kind);
#if SF_GLDS_ABLATE & 4
                if (v == 1.2345e30f) p[voff] = v;  // timing experiment: the value is computed, the store never happens
#else
                if (FULL || (cok && rr < rows_left)) p[voff] = v;
#endif
            }
    }
}

// store_fwd_tile with an output SAMPLE stride: row m of the flat row space belongs to sample m / OHOW, pixel m % OHOW, and goes
// to out + sample * out_ss + pixel * N (k_fwd_glds_zt_os).  mrow0 = this lane's first row, col = its column of tile 0.
template <int TM, int TN, int KIND>
__device__ __forceinline__ void store_fwd_tile_os(const f32x16 (&acc)[TM][TN], float *__restrict__ out, int64_t mrow0,
                                                  int64_t Mtot, const ConvG &g, int64_t out_ss, int col,
                                                  const float *__restrict__ bias, int kind) {
    const int N = g.Cout;
    const uint32_t OHOW = (uint32_t)(g.OH * g.OW);
    bool cok[TN];
    float bv[TN];
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
        cok[tn] = col + tn * 32 < N;
        bv[tn] = (bias && cok[tn]) ? bias[col + tn * 32] : 0.f;
    }
    // a lane's rows come in groups of four consecutive ones (r & 3): the (sample, pixel) split and the 64-bit address are
    // worked out once per group, a row that crosses into the next sample adds the distance between the two samples' ends
    // (OHOW >= 4: at most one boundary inside a group; the launcher keeps out_ss below 2^30)
    const int hop = (int)out_ss - (int)OHOW * N;
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t m0 = mrow0 + tm * 32 + 8 * q;
            const uint32_t smp = fdiv((uint32_t)(m0 < Mtot ? m0 : 0), g.dOHOW), pix = (uint32_t)m0 - smp * OHOW;
            float *p0 = out + (int64_t)smp * out_ss + (int64_t)pix * N + col;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int o = j * N + (pix + (uint32_t)j >= OHOW ? hop : 0);
#pragma unroll
                for (int tn = 0; tn < TN; ++tn) {
                    const float v = act_fwd_c<KIND>(acc[tm][tn][4 * q + j] + bv[tn], kind);
                    if (cok[tn] && m0 + j < Mtot) p0[o + tn * 32] = v;
                }
            }
        }
}

// The same tile as v * act'(y): the data gradient of a linear layer is this forward GEMM on dY with the (untransposed)
// weight matrix, finished with the derivative of the activation that produced the layer's input y (mk: pointer to the
// tile's (0, 0) inside y, same [rows][N] layout).  KIND 0: no mask, 1: ReLU, < 0: run-time kind.
template <int TM, int TN, int KIND, bool FULL>
__device__ __forceinline__ void store_dgrad_tile(const f32x16 (&acc)[TM][TN], float *__restrict__ ob,
                                                 const float *__restrict__ mk, uint32_t voff, int N, int rows_left,
                                                 int cols_left, int kind) {
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
        const bool cok = FULL || tn * 32 < cols_left;
#pragma unroll
        for (int tm = 0; tm < TM; ++tm) {
            float y[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {  // all 16 loads in flight before the first store
                const int rr = tm * 32 + (r & 3) + 8 * (r >> 2);
                const bool ok = FULL || (cok && rr < rows_left);
                y[r] = (KIND != 0 && ok) ? (mk + (int64_t)rr * N + tn * 32)[voff] : 1.f;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rr = tm * 32 + (r & 3) + 8 * (r >> 2);
                const float v = act_bwd_mul<KIND>(acc[tm][tn][r], y[r], kind);
                if (FULL || (cok && rr < rows_left)) (ob + (int64_t)rr * N + tn * 32)[voff] = v;
            }
        }
    }
}


template <int BM, int BN, int WM, int WN>
struct Tile {
    static constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    static constexpr int SA = BM / 32, SB = BN / 32;  // 16-byte load slots per thread per 32-deep chunk
    static_assert(WM * WN == 4 && TM >= 1 && TN >= 1, "4 waves per block");
};

#define ZERO_ACC(acc)                                                                                         \
    _Pragma("unroll") for (int a_ = 0; a_ < T::TM; ++a_) _Pragma("unroll") for (int b_ = 0; b_ < T::TN; ++b_) \
        _Pragma("unroll") for (int r_ = 0; r_ < 16; ++r_) acc[a_][b_][r_] = 0.f

// ============================================================================================== FORWARD
// rows m = (sample, oh, ow); A reduction-major loads (4 consecutive k per slot), B = weights free-axis-major.
template <int BM, int BN, int WM, int WN, int MODE>
__global__ __launch_bounds__(256) void k_conv_fwd(ConvG g, const void *__restrict__ in, int64_t in_stride,
                                                  const int32_t *__restrict__ index, int64_t offset,
                                                  const float *__restrict__ w, const float *__restrict__ bias,
                                                  float *__restrict__ out, int64_t Mtot, int k_per_split,
                                                  float *__restrict__ partial) {
    using T = Tile<BM, BN, WM, WN>;
    constexpr bool FR = frame_layout<MODE>();
    constexpr bool VECB = MODE != MODE_GENERIC;
    constexpr int LDA = BM + 1, LDB = BN + 4;
    __shared__ __attribute__((aligned(16))) float As[32 * LDA];
    __shared__ __attribute__((aligned(16))) float Bs[32 * LDB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int64_t m0 = (int64_t)blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;
    const int N = g.Cout, K = g.K;
    // split-K (small grids only): this block reduces k in [kbeg, kend) and writes a raw partial tile
    const int kbeg = blockIdx.z * k_per_split;
    const int kend = (kbeg + k_per_split < K) ? kbeg + k_per_split : K;

    // A slots.  f32 NHWC input: k-quad fastest across lanes (row = tid/8 + 32*s, k-quad = tid%8): 8 lanes read one
    // 128-byte run of channels.  Raw NCHW frames: row fastest (row = tid%32 + 32*s, k-quad = tid/32): consecutive
    // output pixels are `stride` pixels apart, so 32 lanes x 4 bytes cover one contiguous 128-byte span of a u8 frame
    // (f32 frames: 32 lanes x 16 bytes, `stride` floats apart).
    const int arow = FR ? (tid & 31) : (tid >> 3);
    const int kq = (FR ? (tid >> 5) : (tid & 7)) * 4;
    int64_t abase[T::SA];
    int apo[T::SA];
    bool aval[T::SA];
#pragma unroll
    for (int s = 0; s < T::SA; ++s) {
        const int64_t m = m0 + arow + 32 * s;
        aval[s] = m < Mtot;
        const uint32_t mm = aval[s] ? (uint32_t)m : 0u;
        const uint32_t smp = fdiv(mm, g.dOHOW), pix = mm - smp * (uint32_t)(g.OH * g.OW);
        const bool fr = MODE == MODE_GENERIC ? in_is_frame(g.in_u8) : FR;
        apo[s] = fr ? patch_origin<true>(g, pix) : patch_origin<false>(g, pix);
        abase[s] = sample_base(g, index, offset, in_stride, smp) + apo[s];
    }
    // B slots: F-major: column quad cg, reduction row kk0 + s*(1024/BN)
    constexpr int BG = BN / 4, BROWS = 256 / BG;
    const int bcg = (tid % BG) * 4, bkk0 = tid / BG;

    f32x16 acc[T::TM][T::TN];
    ZERO_ACC(acc);

    ARaw<MODE> ra[T::SA];
    float4 rb[T::SB];
    bool aok = false, bok[T::SB];
    auto gload = [&](int k0) {
        const int ka = k0 + kq;
        aok = ka < kend;
        const uint32_t kc = aok ? (uint32_t)ka : (uint32_t)kbeg;
#pragma unroll
        for (int s = 0; s < T::SA; ++s) ra[s] = load_act_raw<MODE>(g, in, abase[s], apo[s], kc, aok && aval[s]);
#pragma unroll
        for (int s = 0; s < T::SB; ++s) {
            const int k = k0 + bkk0 + s * BROWS;
            bok[s] = k < kend;
            rb[s] = load_row_raw<VECB>(w, bok[s] ? k : kbeg, n0 + bcg, N);
        }
    };
    // Rows >= Mtot and columns >= N only feed accumulator entries that are never stored, and the clamped addresses
    // read finite data, so with full K-chunks (every layer of the Nature CNN: K % 32 == 0) nothing needs masking.
    const bool kfull = ((kend - kbeg) & 31) == 0 && MODE != MODE_GENERIC;
    auto lstore = [&]() {
#pragma unroll
        for (int s = 0; s < T::SA; ++s) {
            const float4 v = act_finish<MODE>(g, ra[s], kfull || (aok && aval[s]));
            As[(kq + 0) * LDA + arow + 32 * s] = v.x;
            As[(kq + 1) * LDA + arow + 32 * s] = v.y;
            As[(kq + 2) * LDA + arow + 32 * s] = v.z;
            As[(kq + 3) * LDA + arow + 32 * s] = v.w;
        }
#pragma unroll
        for (int s = 0; s < T::SB; ++s)
            *reinterpret_cast<float4 *>(&Bs[(bkk0 + s * BROWS) * LDB + bcg]) =
                kfull ? rb[s] : row_finish(rb[s], bok[s], n0 + bcg, N);
    };
    gload(kbeg);
    for (int k0 = kbeg; k0 < kend; k0 += 32) {
        __syncthreads();  // every wave is done reading the previous chunk's LDS image
        lstore();         // first use of the prefetched registers: the loads had the whole MFMA phase to land
        __syncthreads();
        if (k0 + 32 < kend) gload(k0 + 32);
        mma_chunk<T::TM, T::TN, LDA, LDB>(As, Bs, wm * T::TM * 32, wn * T::TN * 32, lane, acc);
    }
    // epilogue: bias + ReLU, NHWC store (split-K: raw partial, finished by k_splitk_finish)
    float *dst = partial ? partial + (int64_t)blockIdx.z * Mtot * N : out;
    const bool fin = partial == nullptr;
    float *ob = dst + (m0 + wm * T::TM * 32) * N + (n0 + wn * T::TN * 32);
    const int rows_left = (int)min((int64_t)(T::TM * 32), Mtot - m0 - wm * T::TM * 32) - 4 * (lane >> 5);
    const int cols_left = N - (n0 + wn * T::TN * 32) - (lane & 31);
    const uint32_t voff = (uint32_t)(4 * (lane >> 5)) * (uint32_t)N + (uint32_t)(lane & 31);
    const bool full = m0 + BM <= Mtot && n0 + BN <= N;
    const float *b0 = (fin && bias) ? bias + n0 + wn * T::TN * 32 : nullptr;
    if (!fin) {
        if (full) store_fwd_tile<T::TM, T::TN, 0, true>(acc, ob, voff, N, rows_left, cols_left, nullptr, lane & 31, 0);
        else store_fwd_tile<T::TM, T::TN, 0, false>(acc, ob, voff, N, rows_left, cols_left, nullptr, lane & 31, 0);
    } else if (g.relu == 1) {
        if (full) store_fwd_tile<T::TM, T::TN, 1, true>(acc, ob, voff, N, rows_left, cols_left, b0, lane & 31, 1);
        else store_fwd_tile<T::TM, T::TN, 1, false>(acc, ob, voff, N, rows_left, cols_left, b0, lane & 31, 1);
    } else {
        store_fwd_tile<T::TM, T::TN, -1, false>(acc, ob, voff, N, rows_left, cols_left, b0, lane & 31, g.relu);
    }
}

// out[m][n] = act(sum_z partial[z][m][n] + bias[n]), z ascending (deterministic)
__global__ __launch_bounds__(256) void k_splitk_finish(const float *__restrict__ partial,
                                                       const float *__restrict__ bias, float *__restrict__ out,
                                                       int64_t MN, int N, int Z, int relu) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < MN; i += (int64_t)gridDim.x * blockDim.x) {
        float s = 0.f;
        for (int z = 0; z < Z; ++z) s += partial[(int64_t)z * MN + i];
        if (bias) s += bias[(int)(i % N)];
        out[i] = act_fwd(s, relu);
    }
}

// ============================================================================================== WEIGHT GRADIENT
// dW[k][n] = sum_m col(in)[m][k] * dY[m][n].  GEMM rows = k (BM), cols = n (BN), reduction = m, split over
// gridDim.z contiguous m-ranges; partial tiles go to workspace[z][K][N], k_reduce_partials sums them in fixed order.
// The bias gradient (column sums of dY) is accumulated from the staged dY tile by the blockIdx.x == 0 blocks.
template <int BN, int WM, int WN, int MODE>
__global__ __launch_bounds__(256) void k_conv_wgrad(ConvG g, const void *__restrict__ in, int64_t in_stride,
                                                    const int32_t *__restrict__ index, int64_t offset,
                                                    const float *__restrict__ dy, float *__restrict__ partial,
                                                    float *__restrict__ partial_b, int64_t Mtot,
                                                    int64_t m_per_split) {
    constexpr int BM = 128;
    using T = Tile<BM, BN, WM, WN>;
    constexpr bool FR = frame_layout<MODE>();
    constexpr bool VECB = MODE != MODE_GENERIC;
    constexpr int LDA = BM + 4, LDB = BN + 4;
    __shared__ __attribute__((aligned(16))) float As[32 * LDA];
    __shared__ __attribute__((aligned(16))) float Bs[32 * LDB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int k0row = blockIdx.x * BM;  // first weight row (im2col column) of this block
    const int n0 = blockIdx.y * BN;
    const int N = g.Cout, K = g.K;
    const int64_t mbeg = (int64_t)blockIdx.z * m_per_split;
    const int64_t mend = (mbeg + m_per_split < Mtot) ? mbeg + m_per_split : Mtot;

    // A' slots (free-axis-major): 4 consecutive weight rows k for one reduction index m.
    // f32 NHWC input: k-group fastest across lanes (32 lanes read 512 contiguous bytes of channels); slot s holds
    //   k-group tid%32 of reduction row tid/32 + 8*s.
    // raw NCHW frames: m fastest (32 consecutive output pixels = one contiguous 128-byte span of a u8 frame); slot s
    //   holds k-group tid/32 + 8*s of reduction row tid%32, so the m -> (sample, pixel) decomposition is done once per
    //   chunk.
    int kg[T::SA], tapo[T::SA];
    bool kval[T::SA];
#pragma unroll
    for (int s = 0; s < T::SA; ++s) {
        kg[s] = (FR ? (tid >> 5) + 8 * s : (tid & 31)) * 4;
        const int k = k0row + kg[s];
        kval[s] = k < K;
        const uint32_t kc = kval[s] ? (uint32_t)k : 0u;
        tapo[s] = MODE == MODE_GENERIC ? 0 : (FR ? tap_offset<true>(g, kc) : tap_offset<false>(g, kc));
    }
    constexpr int BG = BN / 4, BROWS = 256 / BG;
    const int bcg = (tid % BG) * 4, bkk0 = tid / BG;

    f32x16 acc[T::TM][T::TN];
    ZERO_ACC(acc);

    ARaw<MODE> ra[T::SA];
    float4 rb[T::SB];
    bool aok[T::SA], bok[T::SB];
    // base of the patch of reduction row m (sample base + patch origin); po = the patch origin alone
    auto patch_base = [&](int64_t m, bool ok, int &po) -> int64_t {
        const uint32_t mm = ok ? (uint32_t)m : (uint32_t)mbeg;
        const uint32_t smp = fdiv(mm, g.dOHOW), pix = mm - smp * (uint32_t)(g.OH * g.OW);
        const bool fr = MODE == MODE_GENERIC ? in_is_frame(g.in_u8) : FR;
        po = fr ? patch_origin<true>(g, pix) : patch_origin<false>(g, pix);
        return sample_base(g, index, offset, in_stride, smp) + po;
    };
    auto gload = [&](int64_t mc) {
        if constexpr (FR) {
            const int64_t m = mc + (tid & 31);
            const bool mok = m < mend;
            int po;
            const int64_t base = patch_base(m, mok, po);
#pragma unroll
            for (int s = 0; s < T::SA; ++s) {
                if constexpr (MODE == MODE_U8 || MODE == MODE_U8_NORM) {
                    ra[s].v = *reinterpret_cast<const uint32_t *>(reinterpret_cast<const uint8_t *>(in) + base + tapo[s]);
                    if constexpr (MODE == MODE_U8_NORM) {
                        ra[s].mu = *reinterpret_cast<const float4 *>(g.nmu + po + tapo[s]);
                        ra[s].rs = *reinterpret_cast<const float4 *>(g.nrstd + po + tapo[s]);
                    }
                } else {
                    ra[s].v = *reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(in) + base + tapo[s]);
                    if constexpr (MODE == MODE_F32F_NORM) {
                        ra[s].mu = *reinterpret_cast<const float4 *>(g.nmu + po + tapo[s]);
                        ra[s].rs = *reinterpret_cast<const float4 *>(g.nrstd + po + tapo[s]);
                    }
                }
                aok[s] = mok && kval[s];
            }
        } else {
#pragma unroll
            for (int s = 0; s < T::SA; ++s) {
                const int64_t m = mc + (tid >> 5) + 8 * s;
                const bool mok = m < mend;
                aok[s] = mok && kval[s];
                int po;
                const int64_t base = patch_base(m, mok, po);
                if constexpr (MODE == MODE_F32)
                    ra[s].v = *reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(in) + base + tapo[s]);
                else
                    ra[s] = load_act_raw<MODE_GENERIC>(g, in, base, po, (uint32_t)(k0row + kg[s]), aok[s]);
            }
        }
#pragma unroll
        for (int s = 0; s < T::SB; ++s) {
            const int64_t m = mc + bkk0 + s * BROWS;
            bok[s] = m < mend;
            rb[s] = load_row_raw<VECB>(dy, bok[s] ? m : mbeg, n0 + bcg, N);
        }
    };
    const bool do_colsum = partial_b != nullptr && blockIdx.x == 0 && tid < BN;  // bias gradient: column sums of dY
    float colacc = 0.f;
    if (mbeg < mend) gload(mbeg);
    for (int64_t mc = mbeg; mc < mend; mc += 32) {
        __syncthreads();
#pragma unroll
        for (int s = 0; s < T::SA; ++s) {
            const int lrow = FR ? (tid & 31) : (tid >> 5) + 8 * s;  // reduction index (m) inside the chunk
            // rows k >= K are never stored and reduction rows >= mend are annihilated by the zeroed dY rows below,
            // so the activation operand is stored unmasked on the vector paths (clamped loads read finite data)
            *reinterpret_cast<float4 *>(&As[lrow * LDA + kg[s]]) =
                act_finish<MODE>(g, ra[s], MODE != MODE_GENERIC || aok[s]);
        }
        const bool tail = mc + 32 > mend;
#pragma unroll
        for (int s = 0; s < T::SB; ++s)
            *reinterpret_cast<float4 *>(&Bs[(bkk0 + s * BROWS) * LDB + bcg]) =
                (VECB && !tail) ? rb[s] : row_finish(rb[s], bok[s], n0 + bcg, N);
        __syncthreads();
        if (mc + 32 < mend) gload(mc + 32);
        if (do_colsum) {
#pragma unroll 8
            for (int kk = 0; kk < 32; ++kk) colacc += Bs[kk * LDB + tid];
        }
        mma_chunk<T::TM, T::TN, LDA, LDB>(As, Bs, wm * T::TM * 32, wn * T::TN * 32, lane, acc);
    }
    if (do_colsum && n0 + tid < N) partial_b[(int64_t)blockIdx.z * N + n0 + tid] = colacc;
    float *dst = partial + (int64_t)blockIdx.z * K * N;
#pragma unroll
    for (int tm = 0; tm < T::TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < T::TN; ++tn) {
            const int n = n0 + wn * T::TN * 32 + tn * 32 + (lane & 31);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = k0row + wm * T::TM * 32 + tm * 32 + FRAG_ROW(r, lane);
                if (k < K && n < N) dst[(int64_t)k * N + n] = acc[tm][tn][r];
            }
        }
}

// out[i] = sum_z partial[z][i] in a FIXED order (deterministic): eight interleaved accumulators (z mod 8) keep eight
// loads in flight per lane — the single-accumulator loop was latency-bound (Z up to 1024 dependent loads per lane).
__global__ __launch_bounds__(256) void k_reduce_partials(const float *__restrict__ partial, float *__restrict__ out,
                                                         int64_t n, int Z) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        int z = 0;
        for (; z + 8 <= Z; z += 8) {
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] += partial[(int64_t)(z + j) * n + i];
        }
        for (int j = 0; z < Z; ++z, ++j) s[j] += partial[(int64_t)z * n + i];
        out[i] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
    }
}

// Many partials, few outputs (persistent weight-gradient kernels write one partial per work-group: 256 - 512 of them for
// a 27 x 64 ... 256 x 32 result): the loop above is then a handful of work-groups walking Z dependent rounds.  Here a
// work-group takes 32 outputs x 8 groups of consecutive partials; every thread sums its group as above (ascending z,
// eight interleaved accumulators), the eight group sums meet in LDS and are added in a fixed tree.  Deterministic.
__global__ __launch_bounds__(256) void k_reduce_partials_tree(const float *__restrict__ partial, float *__restrict__ out,
                                                              int64_t n, int Z) {
    __shared__ float sm[8][33];
    const int li = threadIdx.x & 31, zg = threadIdx.x >> 5;
    const int64_t i = (int64_t)blockIdx.x * 32 + li;
    const int zper = (Z + 7) / 8, z0 = zg * zper, z1 = z0 + zper < Z ? z0 + zper : Z;
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (i < n) {
        int z = z0;
        for (; z + 8 <= z1; z += 8) {
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] += partial[(int64_t)(z + j) * n + i];
        }
        for (int j = 0; z < z1; ++z, ++j) s[j] += partial[(int64_t)z * n + i];
    }
    sm[zg][li] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
    __syncthreads();
    if (zg == 0 && i < n)
        out[i] = ((sm[0][li] + sm[1][li]) + (sm[2][li] + sm[3][li])) + ((sm[4][li] + sm[5][li]) + (sm[6][li] + sm[7][li]));
}
// ============================================================================================== A/B switches
// Every SF_* environment variable this file reads, once per process; what each one does stands at the decision it steers.
#define SF_SWITCHES(X)                                                                                                  \
    X(reduce_tree, "SF_REDUCE_TREE", 1) X(conv1_bf16, "SF_CONV1_BF16", 1) X(conv1_img, "SF_CONV1_IMG", 1)              \
    X(conv1_wgs, "SF_CONV1_WGS", 2) X(conv1_wide, "SF_CONV1_WIDE", 1) X(conv1_norm, "SF_CONV1_NORM", 1)                \
    X(relu_mask, "SF_RELU_MASK", 1) X(fwd_img, "SF_FWD_IMG", 1) X(linear_narrow, "SF_LINEAR_NARROW", 1)                \
    X(linear_dual, "SF_LINEAR_DUAL", 1) X(glds_cfg, "SF_GLDS_CFG", 0) X(glds_splitk, "SF_GLDS_SPLITK", 1)              \
    X(glds_fc64, "SF_GLDS_FC64", 1) X(glds_wide_min, "SF_GLDS_WIDE_MIN", 384) X(glds_min_tiles, "SF_GLDS_MIN_TILES", 768) \
    X(glds_small64, "SF_GLDS_SMALL64", 256) X(glds_force64, "SF_GLDS_FORCE64", 0) X(glds_split64, "SF_GLDS_SPLIT64", 32) \
    X(glds_zl, "SF_GLDS_ZL", 2) X(glds_tailsplit, "SF_GLDS_TAILSPLIT", 1) X(glds_tall, "SF_GLDS_TALL", 0)              \
    X(glds_persist, "SF_GLDS_PERSIST", 0) X(xcd_raster, "SF_XCD_RASTER", 1) X(xcd_rows, "SF_XCD_ROWS", 0)              \
    X(tap_perm, "SF_TAP_PERM", 0) X(wgrad_glds, "SF_WGRAD_GLDS", 1) X(wgrad_glds_min, "SF_WGRAD_GLDS_MIN", -1)         \
    X(wgrad_glds_k64, "SF_WGRAD_GLDS_K64", 1) X(wgrad_img, "SF_WGRAD_IMG", 3) X(wgrad_zl, "SF_WGRAD_ZL", 1)            \
    X(dgrad_linear, "SF_DGRAD_LINEAR", 1) X(dgrad_linear64, "SF_DGRAD_LINEAR64", 1) X(dgrad_lpt, "SF_DGRAD_LPT", 1)    \
    X(dgrad_zl, "SF_DGRAD_ZL", 3) X(dgrad_pix, "SF_DGRAD_PIX", 1) X(debug_occ, "SF_DEBUG_OCC", 0)
struct Switches {
#define X(field, name, dflt) int64_t field;
    SF_SWITCHES(X)
#undef X
    bool debug_img;  // SF_DEBUG_IMG set at all
};
static int64_t env_num(const char *name, int64_t dflt) {
    const char *v = getenv(name);
    return v ? atoll(v) : dflt;
}
static Switches read_switches() {
    Switches s;
#define X(field, name, dflt) s.field = env_num(name, dflt);
    SF_SWITCHES(X)
#undef X
    s.debug_img = getenv("SF_DEBUG_IMG") != nullptr;
    return s;
}
static const Switches &sw() {
    static const Switches s = read_switches();
    return s;
}

static void launch_reduce_partials(const float *partial, float *out, int64_t n, int Z, hipStream_t st) {
    if (sw().reduce_tree && Z >= 64 && (n + 255) / 256 < 256)  // fewer loop work-groups than CUs and a long walk each
        k_reduce_partials_tree<<<dim3((unsigned)((n + 31) / 32)), dim3(256), 0, st>>>(partial, out, n, Z);
    else
        k_reduce_partials<<<dim3((unsigned)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048)), dim3(256), 0, st>>>(partial, out, n, Z);
}

// ============================================================================================== DATA GRADIENT
// din[sample, ih, iw, c] = mask * sum_{kh,kw,n} dY[sample, (ih-kh)/S, (iw-kw)/S, n] * W[(kh,kw,c), n], only taps with
// kh = ih mod S (+ a*S), kw = iw mod S (+ b*S) contribute -> one GEMM per parity class (ph, pw) = blockIdx.z:
// rows m' = (sample, ihh, iww) with ih = ihh*S+ph, cols = c, reduction k' = ((a*KWs + b)*Cout + n).
template <int BM, int BN, int WM, int WN, bool VEC>
__global__ __launch_bounds__(256) void k_conv_dgrad(ConvG g, const float *__restrict__ dy,
                                                    const float *__restrict__ w, const float *__restrict__ in_act,
                                                    float *__restrict__ din, int64_t nsamples) {
    using T = Tile<BM, BN, WM, WN>;
    constexpr int LDA = BM + 1, LDB = BN + 1;
    __shared__ __attribute__((aligned(16))) float As[32 * LDA];
    __shared__ __attribute__((aligned(16))) float Bs[32 * LDB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int ph = blockIdx.z / g.S, pw = blockIdx.z % g.S;
    const int Hc = (g.H - ph + g.S - 1) / g.S, Wc = (g.W - pw + g.S - 1) / g.S;
    const int KHs = (g.KH - ph + g.S - 1) / g.S, KWs = (g.KW - pw + g.S - 1) / g.S;
    const int64_t Mc = nsamples * Hc * Wc;
    const int64_t m0 = (int64_t)blockIdx.x * BM;
    if (m0 >= Mc || Hc <= 0 || Wc <= 0) return;
    const int n0 = blockIdx.y * BN;  // input-channel tile
    const int Cin = g.Cin, Cout = g.Cout;
    const int Kp = KHs * KWs * Cout;  // reduction length of this class (0 if the class has no taps)

    const int kq = (tid & 7) * 4;
    const FastDiv fHW = g.dHcWc[blockIdx.z], fW = g.dWc[blockIdx.z], fKWs = g.dKWs[blockIdx.z];
    // per-slot dY row of tap (0,0) as a 32-bit index (launcher guarantees rows*Cout < 2^31), plus (ihh, iww)
    int arow[T::SA], aih[T::SA], aiw[T::SA];
    bool aval[T::SA];
    const uint32_t HcWc = (uint32_t)(Hc * Wc);
#pragma unroll
    for (int s = 0; s < T::SA; ++s) {
        const int64_t m = m0 + (tid >> 3) + 32 * s;
        aval[s] = m < Mc;
        const uint32_t mm = aval[s] ? (uint32_t)m : 0u;
        const uint32_t smp = fdiv(mm, fHW), pix = mm - smp * HcWc;
        aih[s] = (int)fdiv(pix, fW);
        aiw[s] = (int)pix - aih[s] * Wc;
        arow[s] = (int)(smp * (uint32_t)(g.OH * g.OW)) + aih[s] * g.OW + aiw[s];
    }
    const bool kfull = (Kp & 31) == 0;  // every chunk full: the weight operand needs no masking
    f32x16 acc[T::TM][T::TN];
    ZERO_ACC(acc);

    float4 ra[T::SA], rb[T::SB];
    bool aok[T::SA], bok = true;
    int ncol = 0;
    auto gload = [&](int k0) {
        const int k = k0 + kq;
        const bool kval = k < Kp;
        const int kc = kval ? k : 0;
        const int tap = (int)fdiv((uint32_t)kc, g.dCout);
        const int n = kc - tap * Cout;
        ncol = n;
        const int a = (int)fdiv((uint32_t)tap, fKWs), b = tap - a * KWs;
        const int drow = a * g.OW + b;  // tap (a,b) reads dY pixel (ihh - a, iww - b)
#pragma unroll
        for (int s = 0; s < T::SA; ++s) {
            const int oh = aih[s] - a, ow = aiw[s] - b;
            aok[s] = kval && aval[s] && oh >= 0 && oh < g.OH && ow >= 0 && ow < g.OW;
            const int row = aok[s] ? arow[s] - drow : 0;
            ra[s] = load_row_raw<VEC>(dy, row, n, Cout);
        }
        const int wrow = ((ph + a * g.S) * g.KW + (pw + b * g.S)) * Cin;
        bok = kval;
#pragma unroll
        for (int s = 0; s < T::SB; ++s) {
            const int c = n0 + (tid >> 3) + 32 * s;
            rb[s] = load_row_raw<VEC>(w, wrow + (c < Cin ? c : 0), n, Cout);  // columns >= Cin are never stored
        }
    };
    if (Kp > 0) gload(0);
    for (int k0 = 0; k0 < Kp; k0 += 32) {
        __syncthreads();
#pragma unroll
        for (int s = 0; s < T::SA; ++s) {
            const float4 v = row_finish(ra[s], aok[s], ncol, Cout);
            As[(kq + 0) * LDA + (tid >> 3) + 32 * s] = v.x;
            As[(kq + 1) * LDA + (tid >> 3) + 32 * s] = v.y;
            As[(kq + 2) * LDA + (tid >> 3) + 32 * s] = v.z;
            As[(kq + 3) * LDA + (tid >> 3) + 32 * s] = v.w;
        }
#pragma unroll
        for (int s = 0; s < T::SB; ++s) {
            const float4 v = (VEC && kfull) ? rb[s] : row_finish(rb[s], bok, ncol, Cout);
            Bs[(kq + 0) * LDB + (tid >> 3) + 32 * s] = v.x;
            Bs[(kq + 1) * LDB + (tid >> 3) + 32 * s] = v.y;
            Bs[(kq + 2) * LDB + (tid >> 3) + 32 * s] = v.z;
            Bs[(kq + 3) * LDB + (tid >> 3) + 32 * s] = v.w;
        }
        __syncthreads();
        if (k0 + 32 < Kp) gload(k0 + 32);
        mma_chunk<T::TM, T::TN, LDA, LDB>(As, Bs, wm * T::TM * 32, wn * T::TN * 32, lane, acc);
    }
    const int akind = g.relu;
#pragma unroll
    for (int tm = 0; tm < T::TM; ++tm)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t m = m0 + wm * T::TM * 32 + tm * 32 + FRAG_ROW(r, lane);
            const bool mok = m < Mc;
            const uint32_t mm = mok ? (uint32_t)m : 0u;
            const uint32_t smp = fdiv(mm, fHW), pix = mm - smp * HcWc;
            const int ihh = (int)fdiv(pix, fW), iww = (int)pix - ihh * Wc;
            const int64_t obase = (((int64_t)smp * g.H + (ihh * g.S + ph)) * g.W + (iww * g.S + pw)) * Cin;
#pragma unroll
            for (int tn = 0; tn < T::TN; ++tn) {
                const int c = n0 + wn * T::TN * 32 + tn * 32 + (lane & 31);
                if (mok && c < Cin) {
                    float v = acc[tm][tn][r];
                    if (in_act) v *= act_bwd(in_act[obase + c], akind);  // kind of the activation that produced in_act
                    din[obase + c] = v;
                }
            }
        }
}

__global__ __launch_bounds__(256) void k_relu_mask(float *__restrict__ gsrc, const float *__restrict__ act, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        if (!(act[i] > 0.f)) gsrc[i] = 0.f;
}

__device__ __forceinline__ float clampf(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }
#include "sf_nn_glds.h"
#include "sf_nn_img.h"
#include "sf_nn_u8.h"
#include "sf_nn_wimg.h"
#include "sf_nn_narrow.h"

// ============================================================================================== host launchers
static inline unsigned cdiv64(int64_t a, int64_t b) { return (unsigned)((a + b - 1) / b); }

// resident blocks per CU of a 256-thread kernel (registers + static LDS), for grid-quantisation decisions
template <class KernelT>
static int occupancy_of(KernelT kern, int threads = 256, size_t dyn_lds = 0) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, threads, dyn_lds) != hipSuccess || nb < 1) nb = 2;
    (void)hipGetLastError();
    return nb;
}


static int num_cus() {
    static int v = 0;
    if (!v) {
        int dev = 0;
        hipDeviceProp_t p;
        v = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&p, dev) == hipSuccess) ? p.multiProcessorCount : 256;
    }
    return v;
}

// ---------------------------------------------------------------------------------------------- launch plans
// One plan per operation: plan_conv_fwd (sf_conv_fwd, sf_conv_fwd_norm), plan_conv_fwd_t, plan_conv_wgrad (sf_conv_wgrad,
// sf_conv_wgrad_norm) and plan_conv_dgrad decide WHICH kernel a launch runs and everything its <<<>>> needs.  The launchers
// validate their arguments and switch on plan.kernel; sf_conv_kernel_name, the workspace queries and the *_supported
// queries call the same functions, so a threshold or a switch lives in exactly one place.
enum ConvKernel {
    K_NONE,  // not a launch the entry point accepts
    K_CONV_FWD, K_CONV1_U8_BF16, K_CONV1_U8_BF16_W, K_CONV_U8_IMG, K_CONV_U8_IMG_NORM,
    K_LINEAR_NARROW, K_FWD_IMG, K_FWD_GLDS, K_FWD_GLDS_Z, K_FWD_GLDS_ZT, K_FWD_GLDS_ZP,
    K_CONV_WGRAD, K_CONV1_WGRAD_BF16, K_CONV1_WGRAD_IMG, K_CONV1_WGRAD_IMG_NORM, K_LINEAR_WGRAD_SMALL, K_WGRAD_IMG,
    K_WGRAD_GLDS, K_WGRAD_GLDS_Z,
    K_CONV_DGRAD, K_DGRAD_PIX, K_DGRAD_PIX_Z, K_DGRAD_QUADROW, K_DGRAD_QUADROW_Z,
};
struct TileArgs { int BM, BN, WM, WN; };  // the <BM, BN, WM, WN> of a tiled kernel (weight gradients: BM = reduction-free K rows)
struct ConvPlan {
    int kernel;           // ConvKernel
    char name[64];        // the instantiation as rocprofv3 spells it
    TileArgs t;
    int variant;          // the remaining template argument: loader MODE, bool (mean subtracted / vector loads), index into
                          // IMG_FWD_GEOMS, k_linear_narrow<1|2>, k_wgrad_img variant 1|2
    dim3 grid, block;
    unsigned lds;         // dynamic LDS bytes
    int splits;           // slices of the reduction (gridDim.z before rastering), 1 = unsplit
    int64_t per_split;    // k_per_split (forward) / m_per_split (weight gradient)
    int partials;         // weight gradient: partial results in the workspace; partial_b starts partials * K * N floats in
    int rx, ry, rtot;     // XCD-aware block order (sf_nn_glds.h): tiles per row / column, total (0 = plain grid)
    int main_tiles;       // k_fwd_glds_zt: 128-row tiles in front of the split last round
    QuadrowClasses qr;    // k_dgrad_quadrow / _z: the column classes and their tiles (sf_nn_glds.h)
    bool recommended;     // sf_conv_fwd_t_supported's answer
};
static ConvPlan plan_init() {
    ConvPlan p{};  // K_NONE, a grid of one work-group, no name
    p.block = dim3(256); p.splits = p.partials = 1;
    return p;
}
static void plan_kernel(ConvPlan &p, int kernel, const char *fmt, ...) {
    p.kernel = kernel;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(p.name, sizeof(p.name), fmt, ap);
    va_end(ap);
}
static void plan_tile(ConvPlan &p, int kernel, const char *base, TileArgs t, const char *tail = "") {
    p.t = t;
    plan_kernel(p, kernel, "%s<%d, %d, %d, %d%s>", base, t.BM, t.BN, t.WM, t.WN, tail);
}
// the strided-output twin of a planned kernel (sf_conv_fwd_relu_mask_os / sf_conv_fwd_t_os): "k_name<...>" -> "k_name_os<...>"
static void plan_os_name(ConvPlan &p) {
    char tmp[64];
    const char *lt = strchr(p.name, '<');
    if (!lt) return;
    snprintf(tmp, sizeof(tmp), "%.*s_os%s", (int)(lt - p.name), p.name, lt);
    memcpy(p.name, tmp, sizeof(tmp));
}
// 1-D launch whose block ids are re-mapped so that every XCD owns a contiguous run of tiles (sf_nn_glds.h)
static void plan_raster(ConvPlan &p, bool on) {
    p.rx = (int)p.grid.x; p.ry = (int)p.grid.y;
    p.rtot = on ? (int)(p.grid.x * p.grid.y * p.grid.z) : 0;
    if (p.rtot > 0) p.grid = dim3((unsigned)(8 * ((p.rtot + 7) / 8)), 1, 1);
}

// What a launcher knows about its operands beyond the descriptor; the plans test the alignments.  sf_conv_kernel_name and
// the queries ask for query_operands(): everything aligned (a null pointer is), dense samples, no index.
struct Operands {
    const void *in;
    int64_t stride;     // in_sample_stride
    bool index;         // samples gathered through an index
    const void *w, *dout, *out;
    int64_t ws_floats;  // sf_conv_fwd: floats of split-K workspace
};
static Operands query_operands(const sf_conv_desc *d, bool split_k_workspace) {
    return Operands{nullptr, (int64_t)d->H * d->W * d->Cin, false, nullptr, nullptr, nullptr, split_k_workspace ? (int64_t)1 << 60 : 0};
}
static bool aligned(const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
static const float TABLE_PROBE[4] __attribute__((aligned(16))) = {0.f, 0.f, 0.f, 0.f};  // stands for mu / rstd in the queries

// (g.nmu set: a launch of sf_conv_fwd_norm / sf_conv_wgrad_norm)
static int pick_mode(const ConvG &g) {
    if (!g.vecA || !g.vecB) return MODE_GENERIC;
    if (in_is_u8(g.in_u8)) return g.nmu ? MODE_U8_NORM : MODE_U8;
    if (g.in_u8 == IN_F32_FRAME) return g.nmu ? MODE_F32F_NORM : MODE_F32F;
    return MODE_F32;
}

// vector loads of the activation operand also need aligned bases (f32: 16 bytes; u8 frames: 4 bytes; the normaliser's
// tables of either frame format: 16 bytes)
static bool act_aligned(const ConvG &g, const void *in, int64_t in_sample_stride) {
    return aligned(in, in_is_u8(g.in_u8) ? 4 : 16) && in_sample_stride % 4 == 0 && aligned(g.nmu, 16) && aligned(g.nrstd, 16);
}

// frame base 4-byte aligned, sample stride a multiple of 4: what the Nature-CNN conv1 strip kernels ask of their input
static bool in4(const Operands &o) { return aligned(o.in, 4) && o.stride % 4 == 0; }
static bool tabs16(const ConvG &g) { return aligned(g.nmu, 16) && aligned(g.nrstd, 16); }

static bool nature_conv1_geom(const ConvG &g) {
    return g.Cin == 4 && g.H == 84 && g.W == 84 && g.KH == 8 && g.KW == 8 && g.S == 4;
}
// geometry contract of k_conv_u8_img<2, 4, 5, 16, *>
static bool conv1_img_ok(const ConvG &g, int mode, int64_t n) {
    return mode == MODE_U8 && n >= 256 && nature_conv1_geom(g) && g.Cout <= 32;
}

// k_conv1_u8_bf16: same geometry; the A operand must be exact in bf16: pixel - mean an integer of at most 8 bits
static bool conv1_bf16_ok(const ConvG &g, int mode, int64_t n) {
    return sw().conv1_bf16 && conv1_img_ok(g, mode, n) && g.sub_mean == floorf(g.sub_mean) && g.sub_mean >= 0.f &&
           g.sub_mean <= 255.f;
}

// ---- conv1 on raw u8 frames WITH the observation normaliser's running statistics applied in the loader (cfg.normalize_input
// on image observations: utils/normalize.py:51-70, running_mean_std.py:79-110, cfg/cfg.py:337-341 default True): no
// normalised f32 copy of the frames exists anywhere.  mu / rstd: the normaliser's f32 tables [Cin*H*W] in the frame's NCHW
// order (sf_obsnorm_update writes them).  sf_conv_norm_supported() accepts every frame descriptor (in_u8 = 1 or 2) that
// check_desc accepts.  Both frame formats take every geometry: the register-staged kernels (k_conv_fwd / k_conv_wgrad)
// form clamp(((x - sub_mean) * inv_scale - mu[d]) * rstd[d], +-5) in their loaders (MODE_U8_NORM / MODE_F32F_NORM), with
// vector loads of pixels and table entries where sf_conv_fwd would use them and the scalar loader otherwise.  The
// Nature-CNN conv1 on u8 frames (32 output channels, aligned operands) keeps the strip-image kernels it always had.
static bool conv_norm_ok(const sf_conv_desc *d, int64_t n) {
    return sw().conv1_norm && d && n > 0 && in_is_frame(d->in_u8);
}
// the strip kernels' compile-time geometry; ANY n (their n >= 256 dispatch threshold is a speed heuristic of the plain
// entry points, the kernels themselves are correct for every n >= 1)
static bool conv_norm_strip(const ConvG &g) {
    return in_is_u8(g.in_u8) && g.Cout == 32 && g.vecA && g.vecB && nature_conv1_geom(g);
}

// forward launch plan: tile config + optional split-K when the natural grid cannot fill 256 CUs several times over
struct FwdPlan {
    int cfg;  // 0: 128x32 (4x1 waves), 1: 128x64 (2x2), 2: 64x64 (2x2)
    int splits, k_per_split;
};
static FwdPlan plan_fwd(int64_t Mtot, int N, int K, int64_t ws_floats) {
    FwdPlan p;
    p.splits = 1;
    p.k_per_split = (K + 31) / 32 * 32;
    p.cfg = N <= 32 ? 0 : 1;
    const int BM = 128, BN = p.cfg == 0 ? 32 : 64;
    int64_t blocks = ((Mtot + BM - 1) / BM) * ((N + BN - 1) / BN);
    if (blocks < 768 && Mtot <= 64) { p.cfg = 2; blocks = ((Mtot + 63) / 64) * ((N + 63) / 64); }
    if (blocks < 768 && K >= 512) {
        int s = (int)((1024 + blocks - 1) / blocks);
        const int smax = K / 256;  // keep >= 8 chunks per split
        if (s > smax) s = smax;
        if (s > 16) s = 16;
        if (s > 1 && (int64_t)s * Mtot * N <= ws_floats) {
            const int chunks = (K + 31) / 32;
            p.k_per_split = ((chunks + s - 1) / s) * 32;
            p.splits = (K + p.k_per_split - 1) / p.k_per_split;
        }
    }
    return p;
}

// sf_conv_fwd and (g.nmu set) sf_conv_fwd_norm
static ConvPlan plan_conv_fwd(const sf_conv_desc *d, const ConvG &g, int64_t n, const Operands &o) {
    ConvPlan p = plan_init();
    const bool norm = g.nmu != nullptr;
    if (norm && !conv_norm_ok(d, n)) return p;
    const int64_t Mtot = n * g.OH * g.OW, npairs = cdiv64(n, 2);
    if (norm && conv_norm_strip(g) && in4(o) && tabs16(g)) {
        // the Nature-CNN conv1 on aligned u8 frames; every other normalising launch: the register-staged kernel below
        p.lds = (unsigned)(2 * 4 * 20 * 84 * sizeof(float));
        static const int bpc = occupancy_of(k_conv_u8_img_norm<2, 4, 5, 16>, 256, 2 * 4 * 20 * 84 * sizeof(float));
        const int64_t resident = (int64_t)num_cus() * (bpc > 0 ? bpc : 1);
        p.grid = dim3((unsigned)(npairs < resident ? npairs : resident));
        plan_kernel(p, K_CONV_U8_IMG_NORM, "k_conv_u8_img_norm<2, 4, 5, 16>");
        return p;
    }
    int mode = pick_mode(g);
    if (mode != MODE_GENERIC && (!act_aligned(g, o.in, o.stride) || !aligned(o.w, 16))) mode = MODE_GENERIC;
    p.variant = g.sub_mean != 0.f;
    // Nature-CNN conv1 on raw frames: strip-image kernel (bytes converted once into an f32 LDS image, im2col read
    // out of LDS).  Geometry contract of the <2,4,5,16> instantiation: K = 256, 2*4*OW rows = 10 fragments.
    // ... and on the bf16 matrix pipe with exact products (sf_nn_u8.h) when (pixel - mean) is an integer of <= 8 bits
    if (conv1_bf16_ok(g, mode, n) && in4(o)) {
        // [SMP][Cin][RS][WP] bf16 strip image + (whole-line stores) the staging tile [SMP][80][36] f32
        const unsigned img_bytes = 2u * 4u * 20u * (unsigned)SF_CONV1_WP * (unsigned)sizeof(uint16_t);
        // persistent grid: SF_CONV1_WGS work-groups per CU (default 2 = what the register budget of __launch_bounds__(256, 2) admits)
        const int64_t resident = (int64_t)num_cus() * sw().conv1_wgs;
        p.grid = dim3((unsigned)(npairs < resident ? npairs : resident));
        // SF_CONV1_WIDE (default 1): whole-line output stores through an LDS staging tile (sf_nn_u8.h) — N == 32, aligned output
        const bool wide = sw().conv1_wide && g.Cout == 32 && aligned(o.out, 16);
        p.lds = img_bytes + (wide ? 2u * 80u * 36u * (unsigned)sizeof(float) : 0u);
        plan_kernel(p, wide ? K_CONV1_U8_BF16_W : K_CONV1_U8_BF16, "k_conv1_u8_bf16%s<%s>", wide ? "_w" : "",
                    p.variant ? "true" : "false");
        return p;
    }
    if (sw().conv1_img && conv1_img_ok(g, mode, n) && in4(o)) {
        p.lds = (unsigned)(2 * 4 * 20 * 84 * sizeof(float));  // [SMP][Cin][RS][W] f32
        // persistent work-groups: as many as are resident at once (two per CU: 53.8 KB of LDS each), each walks the
        // sample pairs b, b + grid, ...
        static const int bpc = occupancy_of(k_conv_u8_img<2, 4, 5, 16, false>, 256, 2 * 4 * 20 * 84 * sizeof(float));
        const int64_t resident = (int64_t)num_cus() * bpc;
        p.grid = dim3((unsigned)(npairs < resident ? npairs : resident));
        plan_kernel(p, K_CONV_U8_IMG, "k_conv_u8_img<2, 4, 5, 16, %s>", p.variant ? "true" : "false");
        return p;
    }
    const FwdPlan f = plan_fwd(Mtot, g.Cout, g.K, norm ? 0 : o.ws_floats);  // (sf_conv_fwd_norm takes no workspace)
    // 256-row tiles: measured +5 % for N = 32 (conv1: twice the MFMAs per barrier), -3..-15 % for N = 64 (occupancy)
    const bool big32 = f.splits == 1 && Mtot >= 256 * 2048;
    const TileArgs t = f.cfg == 0 ? TileArgs{big32 ? 256 : 128, 32, 4, 1} : TileArgs{f.cfg == 1 ? 128 : 64, 64, 2, 2};
    p.variant = mode; p.splits = f.splits; p.per_split = f.k_per_split;
    p.grid = dim3(cdiv64(Mtot, t.BM), cdiv64(g.Cout, t.BN), (unsigned)f.splits);
    p.t = t;
    plan_kernel(p, K_CONV_FWD, "k_conv_fwd<%d, %d, %d, %d, %d>", t.BM, t.BN, t.WM, t.WN, mode);
    return p;
}

extern "C" int64_t sf_conv_fwd_workspace(int64_t n, const sf_conv_desc *h_desc) {
    if (!h_desc || n <= 0) return 0;
    const int K = h_desc->KH * h_desc->KW * h_desc->Cin, N = h_desc->Cout;
    const int64_t Mtot = n * h_desc->OH * h_desc->OW;
    const FwdPlan p = plan_fwd(Mtot, N, K, (int64_t)1 << 60);
    return p.splits > 1 ? (int64_t)sizeof(float) * p.splits * Mtot * N + 256 : 0;
}

#define TILE_IS(BM_, BN_) (p.t.BM == BM_ && p.t.BN == BN_)
static void launch_splitk_finish(const float *partial, const float *bias, float *out, int64_t MN, const ConvG &g, int Z, hipStream_t st) {
    k_splitk_finish<<<dim3(cdiv64(MN, 256) < 4096 ? cdiv64(MN, 256) : 4096), dim3(256), 0, st>>>(partial, bias, out, MN, g.Cout, Z, g.relu);
}
// the loader MODE of a plan as a template argument: L(..., MODE)
#define BY_MODE(L, ...)                                                          \
    switch (p.variant) {                                                         \
        case MODE_F32: L(__VA_ARGS__, MODE_F32); break;                          \
        case MODE_U8: L(__VA_ARGS__, MODE_U8); break;                            \
        case MODE_F32F: L(__VA_ARGS__, MODE_F32F); break;                        \
        case MODE_F32F_NORM: L(__VA_ARGS__, MODE_F32F_NORM); break;              \
        case MODE_U8_NORM: L(__VA_ARGS__, MODE_U8_NORM); break;                  \
        default: L(__VA_ARGS__, MODE_GENERIC);                                   \
    }
#define FWD_LAUNCH(BM, BN, WM, WN, MODE)                          \
    k_conv_fwd<BM, BN, WM, WN, MODE><<<p.grid, p.block, 0, st>>>( \
        g, in, in_sample_stride, index, offset, w, bias, out, Mtot, (int)p.per_split, partial)

// ReLU sign-bit masks (sf_conv_fwd_relu_mask / sf_conv_wgrad_relu_mask): the layers whose forward AND weight-gradient
// kernels can record / consume them — conv1 on raw u8 frames on the exact-product bf16 kernels, 32 output channels, ReLU.
// SF_RELU_MASK=0 switches the path off (A/B: the data gradient below reads the activation again).
static bool relu_mask_ok(const sf_conv_desc *d, int64_t n) {
    if (!sw().relu_mask || !in_is_u8(d->in_u8) || d->relu != 1 || d->Cout != 32) return false;
    const int k = plan_conv_fwd(d, make_geom(d), n, query_operands(d, false)).kernel;
    return k == K_CONV1_U8_BF16 || k == K_CONV1_U8_BF16_W;
}
extern "C" int sf_conv_relu_mask_supported(int64_t n, const sf_conv_desc *h_desc) {
    return h_desc && n > 0 && check_desc(h_desc, "sf_conv_relu_mask_supported") == 0 && relu_mask_ok(h_desc, n) ? 1 : 0;
}

// mu / rstd: the observation normaliser's tables (u8 / f32 frames through sf_conv_fwd_norm), else NULL
static int conv_fwd_impl(const void *in, int64_t in_sample_stride, const int32_t *index, int64_t offset, const float *w,
                         const float *bias, float *out, uint32_t *relu_mask, int64_t n, const sf_conv_desc *h_desc,
                         void *workspace, int64_t workspace_bytes, void *stream, const float *mu = nullptr,
                         const float *rstd = nullptr, bool os = false, int64_t out_ss = 0, int64_t mask_ss = 0,
                         float *out2 = nullptr, int64_t keep_n = -1) {
    int rc = check_desc(h_desc, "sf_conv_fwd");
    if (rc) return rc;
    SF_REQUIRE(in && w && out && n > 0, "sf_conv_fwd: bad args");
    SF_REQUIRE(((uintptr_t)workspace & 15) == 0, "sf_conv_fwd: workspace must be 16-byte aligned");
    ConvG g = make_geom(h_desc);
    g.nmu = mu; g.nrstd = rstd;
    const int64_t Mtot = n * g.OH * g.OW;
    SF_REQUIRE(Mtot < (1LL << 31), "sf_conv_fwd: M=%lld exceeds 2^31 rows; split the batch", (long long)Mtot);
    const Operands o = {in, in_sample_stride, index != nullptr, w, nullptr, out, workspace ? workspace_bytes / (int64_t)sizeof(float) : 0};
    const ConvPlan p = plan_conv_fwd(h_desc, g, n, o);
    hipStream_t st = STREAM(stream);
    const bool bf16 = p.kernel == K_CONV1_U8_BF16 || p.kernel == K_CONV1_U8_BF16_W;
    // only the bf16 kernels record ReLU sign bits: every other path would leave the mask unwritten for the
    // weight-gradient kernel to consume (misaligned operands drop to MODE_GENERIC without it)
    SF_REQUIRE(relu_mask == nullptr || bf16,
               "sf_conv_fwd_relu_mask: operands not eligible for the sign-bit kernel (sf_conv_relu_mask_supported, 4-byte "
               "aligned frames and sample stride, 16-byte aligned weights)");
    SF_REQUIRE(!os || p.kernel == K_CONV1_U8_BF16_W,
               "sf_conv_fwd_relu_mask_os: not a launch of the whole-line-store conv1 kernel (sf_conv_fwd_os_supported)");
    if (bf16 && sw().debug_occ) {
        const unsigned img_bytes = 2u * 4u * 20u * (unsigned)SF_CONV1_WP * (unsigned)sizeof(uint16_t);
        fprintf(stderr, "k_conv1_u8_bf16 occupancy: %d (dword stores, %u B LDS) / %d (whole-line stores, %u B LDS) work-groups per CU\n",
                occupancy_of(k_conv1_u8_bf16<false>, 256, img_bytes), img_bytes,
                occupancy_of(k_conv1_u8_bf16_w<false>, 256, img_bytes + 2u * 80u * 36u * 4u), img_bytes + 2u * 80u * 36u * 4u);
    }
    const uint8_t *in8 = reinterpret_cast<const uint8_t *>(in);
    float *partial = p.splits > 1 ? reinterpret_cast<float *>(workspace) : nullptr;
#define CONV1_LAUNCH(KERN, ...) \
    KERN<<<p.grid, p.block, p.lds, st>>>(g, in8, in_sample_stride, index, offset, w, bias, out, ##__VA_ARGS__, (int)n)
    switch (p.kernel) {
        case K_CONV1_U8_BF16_W:
            if (os) {
                const int kn = (int)(keep_n < 0 ? n : keep_n);  // samples of the strided segment (all of them: one segment)
                if (p.variant) k_conv1_u8_bf16_w_os<true><<<p.grid, p.block, p.lds, st>>>(g, in8, in_sample_stride, index, offset, w, bias, out, relu_mask, (int)n, out_ss, mask_ss, out2, kn);
                else k_conv1_u8_bf16_w_os<false><<<p.grid, p.block, p.lds, st>>>(g, in8, in_sample_stride, index, offset, w, bias, out, relu_mask, (int)n, out_ss, mask_ss, out2, kn);
                break;
            }
            if (p.variant) CONV1_LAUNCH(k_conv1_u8_bf16_w<true>, relu_mask); else CONV1_LAUNCH(k_conv1_u8_bf16_w<false>, relu_mask);
            break;
        case K_CONV1_U8_BF16:
            if (p.variant) CONV1_LAUNCH(k_conv1_u8_bf16<true>, relu_mask); else CONV1_LAUNCH(k_conv1_u8_bf16<false>, relu_mask);
            break;
        case K_CONV_U8_IMG:
            if (p.variant) CONV1_LAUNCH((k_conv_u8_img<2, 4, 5, 16, true>)); else CONV1_LAUNCH((k_conv_u8_img<2, 4, 5, 16, false>));
            break;
        default:  // K_CONV_FWD
            if (TILE_IS(256, 32)) { BY_MODE(FWD_LAUNCH, 256, 32, 4, 1) }
            else if (TILE_IS(128, 32)) { BY_MODE(FWD_LAUNCH, 128, 32, 4, 1) }
            else if (TILE_IS(128, 64)) { BY_MODE(FWD_LAUNCH, 128, 64, 2, 2) }
            else { BY_MODE(FWD_LAUNCH, 64, 64, 2, 2) }
            if (partial) launch_splitk_finish(partial, bias, out, Mtot * g.Cout, g, p.splits, st);
    }
#undef CONV1_LAUNCH
    return sf_launch_status("sf_conv_fwd");
}

extern "C" int sf_conv_fwd(const void *in, int64_t in_sample_stride, const int32_t *index, int64_t offset,
                           const float *w, const float *bias, float *out, int64_t n, const sf_conv_desc *h_desc,
                           void *workspace, int64_t workspace_bytes, void *stream) {
    return conv_fwd_impl(in, in_sample_stride, index, offset, w, bias, out, nullptr, n, h_desc, workspace, workspace_bytes,
                         stream);
}
extern "C" int sf_conv_fwd_relu_mask(const void *in, int64_t in_sample_stride, const int32_t *index, int64_t offset,
                                     const float *w, const float *bias, float *out, uint32_t *relu_mask, int64_t n,
                                     const sf_conv_desc *h_desc, void *stream) {
    SF_REQUIRE(relu_mask && ((uintptr_t)relu_mask & 3) == 0, "sf_conv_fwd_relu_mask: relu_mask must be a 4-byte aligned device buffer");
    SF_REQUIRE(h_desc && n > 0 && relu_mask_ok(h_desc, n) && ((uintptr_t)in & 3) == 0 && in_sample_stride % 4 == 0,
               "sf_conv_fwd_relu_mask: unsupported layer / launch (see sf_conv_relu_mask_supported)");
    return conv_fwd_impl(in, in_sample_stride, index, offset, w, bias, out, relu_mask, n, h_desc, nullptr, 0, stream);
}

// ---- forwards with an OUTPUT sample stride (floats; the sign-bit words: mask_sample_stride u32 words): sample s, pixel p goes
// to out + s * out_sample_stride + p * Cout.  A rollout step writes slot t of a buffer laid out [E, T, OH * OW, Cout] this way;
// the next layer reads it through its input stride, and rows [e * T + t] of that buffer are the dense activation of dataset
// rows e * T + t.  Only the launches whose dense kernel has a strided twin are accepted (sf_conv_fwd_os_supported).
static bool out_stride_ok(const sf_conv_desc *d, const void *out, int64_t out_ss) {
    return out_ss >= (int64_t)d->OH * d->OW * d->Cout && out_ss < (1LL << 30) && out_ss % 4 == 0 && aligned(out, 16);
}
extern "C" int sf_conv_fwd_relu_mask_os(const void *in, int64_t in_sample_stride, const int32_t *index, int64_t offset,
                                        const float *w, const float *bias, float *out, int64_t out_sample_stride,
                                        uint32_t *relu_mask, int64_t mask_sample_stride, int64_t n, const sf_conv_desc *h_desc,
                                        void *stream) {
    SF_REQUIRE(relu_mask && ((uintptr_t)relu_mask & 3) == 0, "sf_conv_fwd_relu_mask_os: relu_mask must be a 4-byte aligned device buffer");
    SF_REQUIRE(h_desc && n > 0 && relu_mask_ok(h_desc, n) && ((uintptr_t)in & 3) == 0 && in_sample_stride % 4 == 0,
               "sf_conv_fwd_relu_mask_os: unsupported layer / launch (see sf_conv_relu_mask_supported)");
    SF_REQUIRE(out_stride_ok(h_desc, out, out_sample_stride) && mask_sample_stride >= (int64_t)h_desc->OH * h_desc->OW,
               "sf_conv_fwd_relu_mask_os: output / mask sample stride shorter than a sample, or unaligned output");
    return conv_fwd_impl(in, in_sample_stride, index, offset, w, bias, out, relu_mask, n, h_desc, nullptr, 0, stream, nullptr,
                         nullptr, true, out_sample_stride, mask_sample_stride);
}
// ---- ... in TWO SEGMENTS of samples (a rollout launch of which only the first keep_n trajectories belong to the learner's
// first minibatch): samples s < keep_n are read and written as by the _os entry points (in / in_sample_stride, out /
// out_sample_stride, relu_mask / mask_sample_stride); samples s >= keep_n are read from in2 + (s - keep_n) * H*W*Cin and written
// to out2 + (s - keep_n) * OH*OW*Cout, both dense, and their sign-bit words are not stored.  0 <= keep_n <= n; the pointers of
// an empty segment are not looked at.  The same kernels as the _os entry points, which are their keep_n = n case.
static bool seg2_ok(const sf_conv_desc *d, const void *out, int64_t out_ss, const void *out2, int64_t keep_n, int64_t n) {
    if (keep_n < 0 || keep_n > n) return false;
    if (keep_n > 0 && !(out && out_stride_ok(d, out, out_ss))) return false;
    if (keep_n == 0 && !(out_ss >= 0 && out_ss < (1LL << 30) && out_ss % 4 == 0)) return false;
    return keep_n == n || (out2 && aligned(out2, 16));
}
extern "C" int sf_conv_fwd_relu_mask_os2(const void *in, int64_t in_sample_stride, const int32_t *index, int64_t offset,
                                         const float *w, const float *bias, float *out, int64_t out_sample_stride,
                                         uint32_t *relu_mask, int64_t mask_sample_stride, float *out2, int64_t keep_n,
                                         int64_t n, const sf_conv_desc *h_desc, void *stream) {
    SF_REQUIRE(h_desc && n > 0 && relu_mask_ok(h_desc, n) && ((uintptr_t)in & 3) == 0 && in_sample_stride % 4 == 0,
               "sf_conv_fwd_relu_mask_os2: unsupported layer / launch (see sf_conv_relu_mask_supported)");
    SF_REQUIRE(seg2_ok(h_desc, out, out_sample_stride, out2, keep_n, n),
               "sf_conv_fwd_relu_mask_os2: keep_n outside [0, n], output sample stride shorter than a sample, or unaligned output");
    SF_REQUIRE(keep_n == 0 || (relu_mask && ((uintptr_t)relu_mask & 3) == 0 && mask_sample_stride >= (int64_t)h_desc->OH * h_desc->OW),
               "sf_conv_fwd_relu_mask_os2: relu_mask must be a 4-byte aligned device buffer, its sample stride a sample long");
    float *o1 = keep_n > 0 ? out : out2;  // (an empty first segment: any valid pointer, never written through)
    return conv_fwd_impl(in, in_sample_stride, index, offset, w, bias, o1, keep_n > 0 ? relu_mask : nullptr, n, h_desc, nullptr, 0,
                         stream, nullptr, nullptr, true, out_sample_stride, mask_sample_stride, out2, keep_n);
}

// ---- LDS-image forward (sf_nn_img.h): compile-time geometries (Cin, H, W, K, S, fragments per step, wave sets, output
// rows per unit).  Nature-CNN conv3 (64 x 9 x 9, 3x3 stride 1, whole images): two independent persistent work-groups
// per CU, +5 % (n = 32768) / +8 % (n = 4096) over k_fwd_glds.  conv2 (32 x 20 x 20, 4x4 stride 2) was measured in two
// forms and stays on k_fwd_glds: whole 51 KB images — X(32, 20, 20, 4, 2, 2, 2, 9) — allow only ONE
// work-group per CU whose 8 waves all stop at the same block barrier (110 vs 117 TFLOP/s); strips of 3 output rows —
// X(32, 20, 20, 4, 2, 2, 1, 3), 20 KB per strip, two work-groups per CU — reach 115: a third more image bytes (strip
// overlap), 2-way bank conflicts where a fragment wraps to the next output row, fewer MFMAs per block step.
#ifndef SF_IMG_TMF
#define SF_IMG_TMF 2  // 16-row fragments per wave and block step of the conv3 LDS-image forward (experiment switch)
#endif
#define IMG_FWD_GEOMS(X) X(64, 9, 9, 3, 1, SF_IMG_TMF, 1, 7)
// index into IMG_FWD_GEOMS (-1: none); fills the plan's grid (persistent: as many work-groups as fit on the chip at once)
static int plan_img_fwd(ConvPlan &p, const ConvG &g, int64_t n, bool any_n = false) {
    if (!sw().fwd_img || g.Cout != 64 || g.KH != g.KW || (n < 512 && !any_n)) return -1;
    int idx = 0;
#define X(CIN, HH, WW, KS, ST, TMF, WS, R)                                                                         \
    if (g.Cin == CIN && g.H == HH && g.W == WW && g.KH == KS && g.S == ST) {                                       \
        static const int bpc = occupancy_of(k_fwd_img<CIN, HH, WW, KS, ST, TMF, WS, R>, 256 * WS);                 \
        p.variant = idx; p.grid = dim3(num_cus() * (bpc > 0 ? bpc : 1)); p.block = dim3(256 * WS);                 \
        plan_kernel(p, K_FWD_IMG, "k_fwd_img<%d, %d, %d, %d, %d, %d, %d, %d>", CIN, HH, WW, KS, ST, TMF, WS, R);   \
        return idx;                                                                                                \
    }                                                                                                              \
    ++idx;
    IMG_FWD_GEOMS(X)
#undef X
    return -1;
}

// ---- glds forward (pre-transposed weights)
static bool glds_fwd_ok(const sf_conv_desc *d) {
    return d->in_u8 == IN_F32_NHWC && d->Cin % 32 == 0 && d->traj_T == 0;
}
// Launch plan of the LDS-DMA forward.  Grids of >= 768 128x64 tiles run unsplit (tile width by grid quantisation).
// A wide layer with a long reduction and too few rows to fill the chip (the fc layer of a rollout step: 4096 x 512,
// K = 3136 -> 128 tiles of 128x128) is split along K so that ~2 blocks land on every CU; the slices go through
// k_splitk_finish (ascending z: deterministic).  Measured at n = 4096: register-staged split-K kernel 140 us, this
// plan 4 x 128 blocks 127 + 10 us.  Where 64x64 tiles alone give two work-groups per CU (>= 512 tiles: exactly that fc
// launch) the reduction runs unsplit on k_fwd_glds<64, 64>: 118-121 us and no partial sums (step -0.4 ms, three
// alternations on one box, profiles/r04_d_fc64_ab.log; 128x64 tiles x 2 slices and a third pipeline stage: +-0).  SF_GLDS_FC64=0: the split plan.
struct GldsFwdPlan {
    bool ok, wide, sq64;  // sq64: 64x64 tiles, unsplit
    int Z, k_per_split;
};
// slices of a reduction of K >= 1024 that turn `tiles` work-groups into about `want`: at least 8 chunks of 32 per slice, at
// most 16 slices (so more than one slice asked for is more than one slice made); returns Z and sets k_per_split
static int split_k(int K, int64_t want, int64_t tiles, int *k_per_split) {
    int z = (int)((want + tiles - 1) / tiles);
    z = z > K / 256 ? K / 256 : z;
    z = z > 16 ? 16 : z;
    if (z <= 1) return 1;
    *k_per_split = (((K + 31) / 32 + z - 1) / z) * 32;
    return (K + *k_per_split - 1) / *k_per_split;
}
static GldsFwdPlan plan_fwd_t(int64_t Mtot, int N, int K) {
    const Switches &s = sw();
    static const int occ64 = occupancy_of(k_fwd_glds<128, 64, 2, 2, 2>), occ128 = occupancy_of(k_fwd_glds<128, 128, 2, 2, 2>);
    GldsFwdPlan p;
    p.ok = false; p.wide = false; p.sq64 = false; p.Z = 1; p.k_per_split = (K + 31) / 32 * 32;
    const int64_t t64 = cdiv64(Mtot, 128) * (int64_t)cdiv64(N, 64), t128 = cdiv64(Mtot, 128) * (int64_t)cdiv64(N, 128);
    // SF_GLDS_WIDE_MIN (default 384): wide outputs of moderate height — the recurrent projection of one rollout step,
    // 2048 x 512 x 2048: 512 tiles, two per CU — also beat the register-staged kernel: 75 -> measured in
    // profiles/r02_c5_*; the GRU's 2048 x 512 x 1536 is 384 tiles.
    // Launches of a few hundred tiles — the per-split inference launches of a host-env run: conv2 at n = 512 is 324 tiles
    // of 128 x 64, the fc layer 4 x 8 tiles of 64 x 64 — used to fall to the register-staged kernel.  Measured at
    // n = 512 / 1024 (profiles/r05_b_kbench_small_n.log): conv2 47.6 / 84.3 us there, 40.1 / 61.4 us on 128 x 64 LDS-DMA
    // tiles, 34.4 / 61.7 us on 64 x 64 tiles (SF_GLDS_SMALL64 = rows/64 from which they are used; 0 = off); the fc layer
    // 170 / 52 us -> 26 / 39 us on 64 x 64 tiles split along K (SF_GLDS_SPLIT64 below).  SF_GLDS_MIN_TILES: 128 x 64
    // tiles from which the unsplit 128-row plan is used (unchanged: 768).  SF_GLDS_FORCE64: experiment switch.
    if (s.glds_force64 && N == 64 && t64 <= s.glds_force64) { p.ok = true; p.sq64 = true; return p; }
    if (s.glds_small64 && t64 < 768 && N == 64 && K >= 256 && cdiv64(Mtot, 64) >= s.glds_small64) {
        p.ok = true; p.sq64 = true;  // narrow layer, few rows: 64-row tiles double the work-groups on the chip
        return p;
    }
    if (t64 >= s.glds_min_tiles || (t64 >= s.glds_wide_min && N >= 512 && K >= 256)) {
        p.ok = true;
        if (N >= 128 && s.glds_cfg == 0) {  // efficiency = rounds / ceil(rounds) with the kernel's own occupancy
            const double u64 = (double)t64 / (256.0 * occ64), u128 = (double)t128 / (256.0 * occ128);
            const double e64 = u64 / (double)(int64_t)(u64 + 0.999999), e128 = u128 / (double)(int64_t)(u128 + 0.999999);
            p.wide = e128 * 1.03 >= e64;  // 64x64 wave tiles: fewer LDS reads and DMA instructions per MFMA
        }
        if (s.glds_cfg == 2) p.wide = true;
        return p;
    }
    if (s.glds_fc64 == 1 && N >= 128 && K >= 1024 && cdiv64(Mtot, 64) * (int64_t)cdiv64(N, 64) >= 512) {
        p.ok = true; p.sq64 = true;  // two 64x64 work-groups per CU, the whole reduction in one pass, no partial sums
        return p;
    }
    // a wide layer on very few rows (the fc layer of a 512-sample inference launch: 4 x 8 tiles of 64 x 64): 64 x 64
    // tiles split along K until ~2 work-groups per CU exist.  SF_GLDS_SPLIT64=<min 64x64 tiles> (0 = off)
    const int64_t t6464 = cdiv64(Mtot, 64) * (int64_t)cdiv64(N, 64);
    if (s.glds_split64 && s.glds_splitk && N >= 128 && K >= 1024 && t6464 >= s.glds_split64 && t6464 < 512) {
        p.Z = split_k(K, 512, t6464, &p.k_per_split);
        if (p.Z > 1) { p.ok = true; p.sq64 = true; return p; }
    }
    if (s.glds_splitk && N >= 128 && K >= 1024 && t128 >= 32) {
        p.Z = split_k(K, 256 * occ128, t128, &p.k_per_split);
        p.ok = p.wide = p.Z > 1;
    }
    return p;
}
static bool linear_1x1(const sf_conv_desc *d) {
    return d->in_u8 == IN_F32_NHWC && d->traj_T == 0 && d->KH == 1 && d->KW == 1 && d->H == 1 && d->W == 1;
}
static bool small_linear_wgrad_ok(const sf_conv_desc *d) {
    return sw().linear_narrow && linear_1x1(d) && d->Cout <= 64 && d->Cin <= 64;
}
// narrow linear layers (the heads): one wave per 16 rows, operands straight from memory (sf_nn_narrow.h)
static bool narrow_fwd_ok(const sf_conv_desc *d, int64_t n) {
    return sw().linear_narrow && linear_1x1(d) && d->Cout <= 32 && d->Cin % 16 == 0 && n < (1 << 30);
}
// SF_GLDS_TAILSPLIT (default 1): single-column unsplit 128 x 64 launches go through k_fwd_glds_zt, which runs a last round of
// work-groups that is at most half full as 64-row tiles.  Returns the number of 128-row tiles in front of that round (all of
// them when there is nothing to split), 0 = not such a launch (k_fwd_glds_z / k_fwd_glds).
static int fwd_tail_split(const ConvG &g, int64_t Mtot, int Z, bool zl_ok) {
    if (!sw().glds_tailsplit || !zl_ok || sw().glds_zl < 1 || Z != 1 || g.Cout > 64 || sw().xcd_rows) return 0;
    static const int occ = occupancy_of(k_fwd_glds_zt<128, 64, 2, 2>, 256, (128 + 64) * 32 * 2 * sizeof(float));
    const int64_t tiles = cdiv64(Mtot, 128), resident = (int64_t)num_cus() * occ, tail = tiles % resident;
    if (tiles <= resident || tail == 0 || 2 * tail > resident) return (int)tiles;
    return (int)(tiles - tail);
}
// Switches of the LDS-DMA forward launch:
// SF_XCD_RASTER (default 1; 0 = off): XCD-aware block order of the launches with more than one column tile (sf_nn_glds.h).
// SF_XCD_ROWS=1: the same re-mapping for launches with ONE column tile (conv2's forward): XCD c then owns a contiguous run
// of row tiles, so the image rows two neighbouring tiles share (a sample straddling a tile boundary, the 2-row halo of the
// 4x4 stride-2 window) are fetched into one L2 instead of two.
// SF_GLDS_ZL (default 2; 1 = wave tiles of at most two 32x32 blocks only, 0 = off): the LDS-DMA forward with no vector-ALU
// instruction in its k-loop (k_fwd_glds_z, sf_nn_glds.h).  Measured (profiles/r05_k_zl_ab.log, r05_k_zl128_ab.log, same box,
// alternating): conv2 forward 213 / 218 -> 192 / 195 us at n = 4096, 1491 / 1507 -> 1413 / 1406 us at n = 32768; fc forward
// of a rollout step (64 x 64 tiles) 110 / 113 -> 105 / 104 us; fc forward at n = 32768 (128 x 128 tiles) 832 / 837 -> 802 / 811 us.
// SF_TAP_PERM=1 (default 0): conv2's forward visits its 16 filter taps in groups of the four taps that read the same input
// elements (k_fwd_glds, sf_nn_glds.h).  Measured (profiles/r05_h_*): counter traffic of the dominant kernel 805.6 -> 544.1 MB
// per launch (1.56 -> 1.05 x algorithmic), launch time 1573 / 1591 vs 1591 / 1597 us at n = 32768 — the re-reads were being
// served by the Infinity Cache, so the time does not move.  It is a different fp32 summation order, though, and the
// normalised-input replay (train_cnn84_norm: inputs up to +-5, two SGD steps) lands on other ReLU flips with it and leaves the
// tolerance the replays are held to (profiles/r05_m_norm_bisect.log); with no time to gain, the natural order stays.
// SF_GLDS_TALL=<min 256-row tiles> (experiment): 256 x 64 tiles (waves 4 x 1, 64 x 64 wave tiles) for 64-column layers with
// many rows — half the per-tile fixed cost and a sixth less DMA per flop, at two work-groups per CU instead of three.
// SF_GLDS_PERSIST=1 (experiment): persistent row-tile walk (k_fwd_glds_zp).
// os: the plan of sf_conv_fwd_t_os — the twin of k_fwd_img (its geometries) or of k_fwd_glds_zt (one column tile, unsplit) at
// ANY n: the size thresholds of the dense dispatch are speed heuristics, the kernels are correct for every n, and whether a
// strided launch may stand in for a dense one is the caller's comparison of the two names.  The twins take their lane
// offsets from the tile's first sample, so only a TILE's span of the input has to fit 32 bits.  K_NONE: no twin.
// keep_n (os): samples of the strided segment, < 0 = all n; k_fwd_glds_zt_os cuts its row tiles per segment.
static ConvPlan plan_conv_fwd_t(const sf_conv_desc *d, int64_t n, int64_t in_sample_stride, ConvG *g_out = nullptr,
                                bool os = false, int64_t keep_n = -1) {
    ConvPlan p = plan_init();
    if (narrow_fwd_ok(d, n)) {
        p.recommended = true; p.variant = d->Cout <= 16 ? 1 : 2;
        p.grid = dim3((unsigned)cdiv64(n, 16)); p.block = dim3(64);
        plan_kernel(p, K_LINEAR_NARROW, "k_linear_narrow<%d>", p.variant);
        return p;
    }
    if (!glds_fwd_ok(d)) return p;
    const ConvG g = make_geom(d);
    if (g_out) *g_out = g;
    const int64_t Mtot = n * g.OH * g.OW;
    if (n * in_sample_stride < ((int64_t)1 << 40) && plan_img_fwd(p, g, n, os) >= 0) {
        p.recommended = true;
        if (os) plan_os_name(p);
        return p;
    }
    // small grids keep the split-K register-staged kernel (a 128-row tile grid must fill 256 CUs a few times over)
    GldsFwdPlan q = plan_fwd_t(Mtot, g.Cout, g.K);
    p.recommended = q.ok;
    if (!q.ok) { q.Z = 1; q.k_per_split = (g.K + 31) / 32 * 32; }  // not a grid sf_conv_fwd_t_supported recommends: still correct, one unsplit launch
    p.splits = q.Z; p.per_split = q.k_per_split;
    // zero-VALU k-loop form (k_fwd_glds_z): every per-lane operand offset must fit 32 bits
    const int64_t lane_span = os ? 127 / (g.OH * g.OW) + 1 : n - 1;  // samples between a lane's row and the DMA base
    const bool zl_ok = sw().glds_zl && lane_span * in_sample_stride + (int64_t)g.H * g.W * g.Cin < (1LL << 30) &&
                       (int64_t)g.Cout * g.K < (1LL << 30);
    const bool col64 = !q.sq64 && !q.wide && q.Z == 1 && g.Cout <= 64 && zl_ok;
    if (os && linear_1x1(d)) {
        // a linear layer (the fc behind conv3, whose output has the two segments): the twin of the unsplit 64 x 64 launch, at
        // any n like the conv twins (whether it may stand in for the dense launch of this n is the caller's comparison of the
        // names and of the workspace); its row tiles are cut per segment, each segment's lane offsets are taken from its base
        const int64_t nk = keep_n < 0 || keep_n > n ? n : keep_n;
        const bool zl2 = sw().glds_zl && (nk == 0 || (nk - 1) * in_sample_stride + g.K < (1LL << 30)) &&
                         (n - nk) * (int64_t)g.K < (1LL << 30) && (int64_t)g.Cout * g.K < (1LL << 30);
        if (!zl2 || g.K % 32 != 0 || g.Cout < 64) return plan_init();
        p.splits = 1; p.per_split = g.K;
        p.grid = dim3((unsigned)(cdiv64(nk, 64) + cdiv64(n - nk, 64)), cdiv64(g.Cout, 64), 1);
        plan_raster(p, sw().xcd_raster && p.grid.y > 1);
        plan_tile(p, K_FWD_GLDS_Z, "k_fwd_glds_z", TileArgs{64, 64, 2, 2});
        plan_os_name(p);
        return p;
    }
    if (os) {
        p.splits = 1; p.per_split = (g.K + 31) / 32 * 32;
        const int64_t Mkeep = (keep_n < 0 || keep_n > n ? n : keep_n) * g.OH * g.OW;
        const int64_t tiles = cdiv64(Mkeep, 128) + cdiv64(Mtot - Mkeep, 128);  // (one more than the flat count where the split is inside a tile)
        // the dense segment runs the body of k_fwd_glds_zt: its lane offsets are taken from in2, over the whole segment
        const bool seg2_zl = Mkeep == Mtot || (n - Mkeep / (g.OH * g.OW)) * (int64_t)g.H * g.W * g.Cin < (1LL << 30);
        p.main_tiles = g.K % 32 == 0 && g.OH * g.OW >= 4 && seg2_zl ? fwd_tail_split(g, tiles * 128, 1, zl_ok) : 0;  // (>= 4 pixels: store_fwd_tile_os)
        if (p.main_tiles <= 0) return plan_init();
        const int tail = (int)tiles - p.main_tiles;
        p.grid = dim3((unsigned)(p.main_tiles + 2 * tail));
        p.lds = (128 + 64) * 32 * 2 * sizeof(float);
        plan_tile(p, K_FWD_GLDS_ZT, "k_fwd_glds_zt", TileArgs{128, 64, 2, 2});
        plan_os_name(p);
        return p;
    }
    if (sw().glds_persist && col64) {
        static const int occp = occupancy_of(k_fwd_glds_zp<128, 64, 2, 2>);
        const int64_t tiles = cdiv64(Mtot, 128), slots = (int64_t)num_cus() * occp;
        p.grid = dim3((unsigned)(tiles < slots ? tiles : slots));
        plan_tile(p, K_FWD_GLDS_ZP, "k_fwd_glds_zp", TileArgs{128, 64, 2, 2});
        return p;
    }
    if (sw().glds_tall && col64 && cdiv64(Mtot, 256) >= (unsigned)sw().glds_tall) {
        p.grid = dim3(cdiv64(Mtot, 256), 1, 1);
        plan_tile(p, K_FWD_GLDS_Z, "k_fwd_glds_z", TileArgs{256, 64, 4, 1});
        return p;
    }
    if (!q.sq64 && !q.wide) {
        p.main_tiles = fwd_tail_split(g, Mtot, q.Z, zl_ok);
        if (p.main_tiles > 0) {
            const int tail = (int)cdiv64(Mtot, 128) - p.main_tiles;
            p.grid = dim3((unsigned)(p.main_tiles + 2 * tail));
            p.lds = (128 + 64) * 32 * 2 * sizeof(float);
            plan_tile(p, K_FWD_GLDS_ZT, "k_fwd_glds_zt", TileArgs{128, 64, 2, 2});
            return p;
        }
    }
    const TileArgs t = q.sq64 ? TileArgs{64, 64, 2, 2} : q.wide ? TileArgs{128, 128, 2, 2} : TileArgs{128, 64, 2, 2};
    p.grid = dim3(cdiv64(Mtot, t.BM), cdiv64(g.Cout, t.BN), (unsigned)q.Z);
    plan_raster(p, sw().xcd_raster && (p.grid.y > 1 || (sw().xcd_rows && p.grid.x >= 64)));
    // wave tiles of more than two 32x32 blocks (128 x 128) take the _z form from SF_GLDS_ZL=2 on
    if (zl_ok && ((t.BM / t.WM / 32) * (t.BN / t.WN / 32) <= 2 || sw().glds_zl >= 2)) plan_tile(p, K_FWD_GLDS_Z, "k_fwd_glds_z", t);
    else plan_tile(p, K_FWD_GLDS, "k_fwd_glds", t, ", 2");
    return p;
}
extern "C" int sf_conv_fwd_t_supported(int64_t n, const sf_conv_desc *h_desc) {
    return h_desc && n > 0 && plan_conv_fwd_t(h_desc, n, query_operands(h_desc, false).stride).recommended ? 1 : 0;
}
extern "C" int64_t sf_conv_fwd_t_workspace(int64_t n, const sf_conv_desc *h_desc) {
    if (!h_desc || n <= 0) return 0;
    const ConvPlan p = plan_conv_fwd_t(h_desc, n, query_operands(h_desc, false).stride);
    return p.splits > 1 ? (int64_t)sizeof(float) * p.splits * n * h_desc->OH * h_desc->OW * h_desc->Cout + 256 : 0;
}
#define GLDS_FWD_ARGS \
    g, in, in_sample_stride, wt, bias, out, Mtot, (int)p.per_split, partial, nullptr, 0, p.rx, p.ry, p.rtot, sw().tap_perm
#define GLDS_FWD(BM, BN, WM, WN)                                                                            \
    do {                                                                                                    \
        if (p.kernel == K_FWD_GLDS_Z) k_fwd_glds_z<BM, BN, WM, WN><<<p.grid, p.block, 0, st>>>(GLDS_FWD_ARGS); \
        else k_fwd_glds<BM, BN, WM, WN, 2><<<p.grid, p.block, 0, st>>>(GLDS_FWD_ARGS);                      \
    } while (0)
extern "C" int sf_conv_fwd_t(const float *in, int64_t in_sample_stride, const float *wt, const float *bias, float *out,
                             int64_t n, const sf_conv_desc *h_desc, void *workspace, int64_t workspace_bytes,
                             void *stream) {
    int rc = check_desc(h_desc, "sf_conv_fwd_t");
    if (rc) return rc;
    SF_REQUIRE(in && wt && out && n > 0, "sf_conv_fwd_t: bad args");
    SF_REQUIRE(((uintptr_t)in & 15) == 0 && ((uintptr_t)wt & 15) == 0 && in_sample_stride % 4 == 0,
               "sf_conv_fwd_t: operands must be 16-byte aligned");
    ConvG g;
    const ConvPlan p = plan_conv_fwd_t(h_desc, n, in_sample_stride, &g);
    hipStream_t st = STREAM(stream);
    if (p.kernel == K_LINEAR_NARROW) {
#define NARROW_ARGS in, in_sample_stride, wt, bias, out, (int)n, h_desc->Cout, h_desc->Cin, h_desc->relu
        if (p.variant == 1) k_linear_narrow<1><<<p.grid, p.block, 0, st>>>(NARROW_ARGS);
        else k_linear_narrow<2><<<p.grid, p.block, 0, st>>>(NARROW_ARGS);
#undef NARROW_ARGS
        return sf_launch_status("sf_conv_fwd_t");
    }
    SF_REQUIRE(glds_fwd_ok(h_desc), "sf_conv_fwd_t: needs f32 NHWC input with Cin %% 32 == 0 (use sf_conv_fwd)");
    const int64_t Mtot = n * g.OH * g.OW;
    SF_REQUIRE(Mtot < (1LL << 31), "sf_conv_fwd_t: M=%lld exceeds 2^31 rows; split the batch", (long long)Mtot);
    float *partial = nullptr;
    if (p.splits > 1) {
        SF_REQUIRE(workspace && ((uintptr_t)workspace & 15) == 0 &&
                       workspace_bytes >= (int64_t)sizeof(float) * p.splits * Mtot * g.Cout,
                   "sf_conv_fwd_t: this launch is split along K and needs sf_conv_fwd_t_workspace() bytes of workspace");
        partial = reinterpret_cast<float *>(workspace);
    }
    switch (p.kernel) {
        case K_FWD_IMG: {
            int idx = 0;
#define X(CIN, HH, WW, KS, ST, TMF, WS, R)                                                                           \
    if (p.variant == idx++) {                                                                                        \
        if (sw().debug_img) fprintf(stderr, "k_fwd_img R=%d: %d work-groups per CU\n", R, (int)p.grid.x / num_cus()); \
        k_fwd_img<CIN, HH, WW, KS, ST, TMF, WS, R><<<p.grid, p.block, 0, st>>>(in, in_sample_stride, wt, bias, out, (int)n, g.relu); \
    }
            IMG_FWD_GEOMS(X)
#undef X
            break;
        }
        case K_FWD_GLDS_ZP:
            k_fwd_glds_zp<128, 64, 2, 2><<<p.grid, p.block, 0, st>>>(g, in, in_sample_stride, wt, bias, out, Mtot, (int)p.per_split);
            break;
        case K_FWD_GLDS_ZT:
            k_fwd_glds_zt<128, 64, 2, 2><<<p.grid, p.block, p.lds, st>>>(g, in, in_sample_stride, wt, bias, out, Mtot, (int)p.per_split,
                                                                          p.main_tiles, sw().tap_perm);
            break;
        default:  // K_FWD_GLDS_Z / K_FWD_GLDS
            if (TILE_IS(256, 64)) k_fwd_glds_z<256, 64, 4, 1><<<p.grid, p.block, 0, st>>>(GLDS_FWD_ARGS);  // (_z form only)
            else if (TILE_IS(64, 64)) GLDS_FWD(64, 64, 2, 2);
            else if (TILE_IS(128, 128)) GLDS_FWD(128, 128, 2, 2);
            else GLDS_FWD(128, 64, 2, 2);
    }
    if (partial) launch_splitk_finish(partial, bias, out, Mtot * g.Cout, g, p.splits, st);
    return sf_launch_status("sf_conv_fwd_t");
}
// two linear layers into one accumulator (k_fwd_glds2): out = a1 w1t^T + a2 w2t^T + bias1 + bias2
// sf_conv_fwd_t with an output sample stride: the launches that resolve to k_fwd_glds_zt (conv2) or k_fwd_img (conv3)
static int conv_fwd_t_os_impl(const char *who, const float *in, int64_t in_sample_stride, const float *in2, const float *wt,
                              const float *bias, float *out, int64_t out_sample_stride, float *out2, int64_t keep_n, int64_t n,
                              const sf_conv_desc *h_desc, void *stream) {
    int rc = check_desc(h_desc, who);
    if (rc) return rc;
    SF_REQUIRE(wt && n > 0 && ((uintptr_t)wt & 15) == 0 && in_sample_stride % 4 == 0, "%s: bad args", who);
    SF_REQUIRE(seg2_ok(h_desc, out, out_sample_stride, out2, keep_n, n),
               "%s: keep_n outside [0, n], output sample stride shorter than a sample, or unaligned output", who);
    SF_REQUIRE((keep_n == 0 || (in && ((uintptr_t)in & 15) == 0)) && (keep_n == n || (in2 && ((uintptr_t)in2 & 15) == 0)),
               "%s: operands must be 16-byte aligned", who);
    ConvG g;
    const ConvPlan p = plan_conv_fwd_t(h_desc, n, in_sample_stride, &g, true, keep_n);
    SF_REQUIRE((p.kernel == K_FWD_IMG || p.kernel == K_FWD_GLDS_ZT || p.kernel == K_FWD_GLDS_Z) && p.splits == 1,
               "%s: this launch has no strided-output kernel (sf_conv_fwd_os_supported)", who);
    const int64_t Mtot = n * g.OH * g.OW;
    SF_REQUIRE(Mtot < (1LL << 31), "%s: M=%lld exceeds 2^31 rows; split the batch", who, (long long)Mtot);
    hipStream_t st = STREAM(stream);
    if (p.kernel == K_FWD_IMG) {
        int idx = 0;
#define X(CIN, HH, WW, KS, ST, TMF, WS, R)                                                                              \
    if (p.variant == idx++)                                                                                             \
        k_fwd_img_os<CIN, HH, WW, KS, ST, TMF, WS, R><<<p.grid, p.block, 0, st>>>(in, in_sample_stride, wt, bias, out, (int)n, \
                                                                                  g.relu, out_sample_stride, in2, out2, (int)keep_n);
        IMG_FWD_GEOMS(X)
#undef X
    } else if (p.kernel == K_FWD_GLDS_Z) {
        k_fwd_glds_z_os<64, 64, 2, 2><<<p.grid, p.block, 0, st>>>(g, in, in_sample_stride, wt, bias, out, Mtot, (int)p.per_split, p.rx,
                                                                   p.ry, p.rtot, out_sample_stride, in2, out2, keep_n);
    } else {
        k_fwd_glds_zt_os<128, 64, 2, 2><<<p.grid, p.block, p.lds, st>>>(g, in, in_sample_stride, wt, bias, out, Mtot, (int)p.per_split,
                                                                         p.main_tiles, sw().tap_perm, out_sample_stride, in2, out2,
                                                                         keep_n * g.OH * g.OW);
    }
    return sf_launch_status(who);
}
extern "C" int sf_conv_fwd_t_os(const float *in, int64_t in_sample_stride, const float *wt, const float *bias, float *out,
                                int64_t out_sample_stride, int64_t n, const sf_conv_desc *h_desc, void *stream) {
    SF_REQUIRE(in && out, "sf_conv_fwd_t_os: bad args");
    return conv_fwd_t_os_impl("sf_conv_fwd_t_os", in, in_sample_stride, nullptr, wt, bias, out, out_sample_stride, nullptr, n, n,
                              h_desc, stream);
}
extern "C" int sf_conv_fwd_t_os2(const float *in, int64_t in_sample_stride, const float *in2, const float *wt, const float *bias,
                                 float *out, int64_t out_sample_stride, float *out2, int64_t keep_n, int64_t n,
                                 const sf_conv_desc *h_desc, void *stream) {
    return conv_fwd_t_os_impl("sf_conv_fwd_t_os2", in, in_sample_stride, in2, wt, bias, out, out_sample_stride, out2, keep_n, n,
                              h_desc, stream);
}
// op: 0 sf_conv_fwd_relu_mask_os, 3 sf_conv_fwd_t_os (the numbers of their dense entry points in sf_conv_kernel_name)
static int conv_fwd_os_supported_impl(int op, int64_t n, int64_t keep_n, const sf_conv_desc *h_desc, int64_t in_sample_stride,
                                      int64_t out_sample_stride) {
    if (!h_desc || n <= 0 || keep_n < 0 || keep_n > n || check_desc(h_desc, "sf_conv_fwd_os_supported") != 0 ||
        in_sample_stride % 4 != 0 || !out_stride_ok(h_desc, nullptr, out_sample_stride) ||
        n * (int64_t)h_desc->OH * h_desc->OW >= (1LL << 31))
        return 0;
    if (op == 0) {
        if (!relu_mask_ok(h_desc, n)) return 0;
        Operands o = query_operands(h_desc, false);
        o.stride = in_sample_stride;
        return plan_conv_fwd(h_desc, make_geom(h_desc), n, o).kernel == K_CONV1_U8_BF16_W ? 1 : 0;
    }
    if (op != 3) return 0;
    const ConvPlan p = plan_conv_fwd_t(h_desc, n, in_sample_stride, nullptr, true, keep_n);
    return (p.kernel == K_FWD_IMG || p.kernel == K_FWD_GLDS_ZT || p.kernel == K_FWD_GLDS_Z) && p.splits == 1 ? 1 : 0;
}
extern "C" int sf_conv_fwd_os_supported(int op, int64_t n, const sf_conv_desc *h_desc, int64_t in_sample_stride,
                                        int64_t out_sample_stride) {
    return conv_fwd_os_supported_impl(op, n, n, h_desc, in_sample_stride, out_sample_stride);
}
// ... of the two-segment entry points with this split
extern "C" int sf_conv_fwd_os2_supported(int op, int64_t n, int64_t keep_n, const sf_conv_desc *h_desc, int64_t in_sample_stride,
                                         int64_t out_sample_stride) {
    return conv_fwd_os_supported_impl(op, n, keep_n, h_desc, in_sample_stride, out_sample_stride);
}

extern "C" int sf_linear_fwd_dual_supported(int64_t n, int N, int K1, int K2) {
    return sw().linear_dual && n > 0 && N >= 64 && K1 > 0 && K2 > 0 && K1 % 32 == 0 && K2 % 32 == 0 && n < (1LL << 31) &&
           cdiv64(n, 128) * (int64_t)cdiv64(N, 64) >= 256;
}
extern "C" int sf_linear_fwd_dual(const float *a1, int64_t lda1, const float *w1t, const float *bias1, int K1,
                                  const float *a2, int64_t lda2, const float *w2t, const float *bias2, int K2, float *out,
                                  int64_t n, int N, int gru_H, void *stream) {
    SF_REQUIRE(a1 && w1t && a2 && w2t && out && n > 0 && N > 0, "sf_linear_fwd_dual: bad args");
    SF_REQUIRE(K1 > 0 && K2 > 0 && K1 % 32 == 0 && K2 % 32 == 0 && lda1 % 4 == 0 && lda2 % 4 == 0 && n < (1LL << 31),
               "sf_linear_fwd_dual: K1, K2 must be multiples of 32 and the row strides multiples of 4 (K1=%d K2=%d)", K1, K2);
    SF_REQUIRE((((uintptr_t)a1 | (uintptr_t)a2 | (uintptr_t)w1t | (uintptr_t)w2t) & 15) == 0,
               "sf_linear_fwd_dual: operands must be 16-byte aligned");
    SF_REQUIRE(gru_H == 0 || (gru_H > 0 && gru_H % 64 == 0 && N == 4 * gru_H),
               "sf_linear_fwd_dual: the GRU column layout needs N == 4 * gru_H and gru_H %% 64 == 0 (N=%d gru_H=%d)", N, gru_H);
    k_fwd_glds2<128, 64, 2, 2><<<dim3(cdiv64(n, 128), cdiv64(N, 64)), dim3(256), 0, STREAM(stream)>>>(
        a1, lda1, w1t, bias1, K1, a2, lda2, w2t, bias2, K2, out, n, N, gru_H);
    return sf_launch_status("sf_linear_fwd_dual");
}
extern "C" int sf_transpose(const float *w, float *wt, int K, int N, void *stream) {
    SF_REQUIRE(w && wt && K > 0 && N > 0, "sf_transpose: bad args");
    k_transpose<<<dim3(cdiv64(K, 32), cdiv64(N, 32)), dim3(256), 0, STREAM(stream)>>>(w, wt, K, N);
    return sf_launch_status("sf_transpose");
}

// split plan shared by the workspace query and the launcher
struct SplitPlan {
    int Z;
    int64_t m_per_split;
};
// bpc = resident blocks per CU of the kernel that will run (hipOccupancy...), 0 = unknown (workspace query: return the
// largest split count any bpc can lead to).  The reduction is split so that the grid fills the chip in WHOLE rounds:
// 200 tiles x Z = 8 on 1024 slots is 1.56 rounds, i.e. 2 rounds at 78 % — Z = 5 (0.98 rounds) is 25 % faster.
static SplitPlan plan_splits(int64_t Mtot, int K, int N, int BM, int BN, int bpc = 0) {
    const int64_t tiles = (int64_t)((K + BM - 1) / BM) * ((N + BN - 1) / BN);
    const int64_t chunks = (Mtot + 31) / 32;
    int64_t zcap = (2304 + tiles - 1) / tiles;  // never more than ~9 blocks per CU
    const int64_t zmax = (chunks + 7) / 8;      // at least 8 chunks (256 reduction rows) per split
    if (zcap > zmax) zcap = zmax;
    if (zcap < 1) zcap = 1;
    if (zcap > 1024) zcap = 1024;
    int64_t Z = zcap;
    if (bpc > 0) {
        const double slots = 256.0 * bpc;
        double best = -1.0;
        for (int64_t z = 1; z <= zcap; ++z) {
            const double u = (double)(tiles * z) / slots, rounds = u <= 1.0 ? 1.0 : (double)(int64_t)(u + 0.999999);
            double eff = u / rounds;
            if (tiles * z < 256) eff *= 0.5;          // fewer blocks than CUs: strictly worse than the formula says
            if (eff > best + 0.02) { best = eff; Z = z; }  // ties / near-ties: the smaller split (less partial traffic)
        }
    }
    SplitPlan p;
    p.m_per_split = ((chunks + Z - 1) / Z) * 32;
    p.Z = (int)((Mtot + p.m_per_split - 1) / p.m_per_split);
    return p;
}
template <int BK, int BN, int WM, int WN>
static int occ_wgrad_glds() {
    static const int v = occupancy_of(k_wgrad_glds<BK, BN, WM, WN>);
    return v;
}
static inline int wgrad_bn(int N) { return N <= 32 ? 32 : 64; }
// partials sf_conv_wgrad_workspace always has room for: the register-staged kernel's largest split count
static int wgrad_ws_partials(int64_t Mtot, int K, int N) { return plan_splits(Mtot, K, N, 128, wgrad_bn(N)).Z; }
struct WgradGlds {
    int cfg;  // 0: 256x64 (waves 4x1), 1: 128x128 (2x2), 2: 128x64 (2x2), 3: 64x128 (2x2; K = 64: the recurrent input projection)
    int BK, BN, Z;
    int64_t m_per_split;
};
// SF_WGRAD_GLDS: 0 = the register-staged kernel instead, 1 = default, 2 + cfg = that tile config for every launch
static WgradGlds plan_wgrad_glds(int64_t Mtot, int K, int N, bool query_occupancy = false) {
    WgradGlds q;
    // 256-row weight tiles only when they do not add padded rows over 128-row tiles (K = 576: 768 vs 640 rows)
    const bool k256 = K >= 256 && (K + 255) / 256 * 256 <= (K + 127) / 128 * 128;
    q.cfg = N >= 128 ? 1 : (k256 ? 0 : 2);
    if (sw().wgrad_glds >= 2) q.cfg = sw().wgrad_glds - 2;
    if (K == 64 && N >= 128) q.cfg = 3;  // a 128-row weight tile would be half padding
    q.BK = q.cfg == 0 ? 256 : q.cfg == 3 ? 64 : 128;
    q.BN = (q.cfg == 1 || q.cfg == 3) ? 128 : 64;
    int bpc = 0;
    if (query_occupancy)
        bpc = q.cfg == 0 ? occ_wgrad_glds<256, 64, 4, 1>() : q.cfg == 1 ? occ_wgrad_glds<128, 128, 2, 2>()
              : q.cfg == 3 ? occ_wgrad_glds<64, 128, 2, 2>() : occ_wgrad_glds<128, 64, 2, 2>();
    const SplitPlan p = plan_splits(Mtot, K, N, q.BK, q.BN, bpc);
    q.Z = p.Z;
    q.m_per_split = p.m_per_split;
    return q;
}

// Which reductions go to the LDS-DMA weight-gradient kernel: long ones, and mid-sized ones with a large K x N (the fc
// layer at n = 32768: 1044 -> 911 us; the LSTM's 512 x 2048 recurrent matrix at 16384 chunk rows; the 8-column heads
// stay on the register-staged kernel).  SF_WGRAD_GLDS_MIN
// overrides the row threshold (A/B switch).
static bool wgrad_glds_wanted(int64_t Mtot, int K, int N) {
    if (sw().wgrad_glds_min >= 0) return Mtot >= sw().wgrad_glds_min;
    if (sw().wgrad_glds_k64 && Mtot >= 16384 && K == 64 && N >= 512) return true;  // W_ih of a recurrent core behind a 64-wide encoder
    return Mtot >= 65536 || (Mtot >= 16384 && N >= 64 && (K >= 1024 || (int64_t)K * N >= 512 * 1024));
}

// LDS-image weight gradient (sf_nn_wimg.h): Nature-CNN conv3 (variant 1: 4 waves, two work-groups per CU) and conv2
// (variant 2: 8 waves, one work-group per CU) geometries, launches that give every persistent work-group a few samples.
// SF_WGRAD_IMG=0: back on k_wgrad_glds; =1: conv3 only; default 3: both (A/B switch).
static int wgrad_img_variant(const sf_conv_desc *d, int64_t n) {
    const int on = sw().wgrad_img;
    if (!on || d->in_u8 != IN_F32_NHWC || d->traj_T != 0 || d->Cout != 64 || n < 512) return 0;
    if ((on & 1) && d->Cin == 64 && d->H == 9 && d->W == 9 && d->KH == 3 && d->KW == 3 && d->stride == 1) return 1;
    if ((on & 2) && d->Cin == 32 && d->H == 20 && d->W == 20 && d->KH == 4 && d->KW == 4 && d->stride == 2) return 2;
    return 0;
}
static int wgrad_img_blocks(const sf_conv_desc *d, int64_t n) {
    const int64_t nb = (wgrad_img_variant(d, n) == 1 ? 2 : 1) * (int64_t)num_cus();
    return (int)(n < nb ? n : nb);
}

// per-mode occupancy of the register-staged weight-gradient kernel
template <int BN, int WM, int WN>
static int occ_wgrad_mode(int mode) {
#define OCC(MODE) { static const int v = occupancy_of(k_conv_wgrad<BN, WM, WN, MODE>); return v; }
    switch (mode) {
        case MODE_F32: OCC(MODE_F32) case MODE_U8: OCC(MODE_U8) case MODE_F32F: OCC(MODE_F32F)
        case MODE_F32F_NORM: OCC(MODE_F32F_NORM) case MODE_U8_NORM: OCC(MODE_U8_NORM) default: OCC(MODE_GENERIC)
    }
#undef OCC
}

// sf_conv_wgrad and (g.nmu set) sf_conv_wgrad_norm.  Every kernel writes plan.partials partial results [K, N] (+ [N] for
// the bias, plan.partials * K * N floats in) that launch_reduce_partials sums; the strip kernels' persistent grids are
// cut to the partials sf_conv_wgrad_workspace sized for.
static ConvPlan plan_conv_wgrad(const sf_conv_desc *d, const ConvG &g, int64_t n, const Operands &o) {
    ConvPlan p = plan_init();
    const bool norm = g.nmu != nullptr;
    if (norm && !conv_norm_ok(d, n)) return p;
    const int K = g.K, N = g.Cout, BN = wgrad_bn(N);
    const int64_t Mtot = n * g.OH * g.OW;
    const int Zws = wgrad_ws_partials(Mtot, K, N), npairs = (int)((n + 1) / 2);
    int mode = pick_mode(g);
    if (mode != MODE_GENERIC && (!act_aligned(g, o.in, o.stride) || !aligned(o.dout, 16))) mode = MODE_GENERIC;
    const bool strip_ops = N == 32 && in4(o) && aligned(o.dout, 16);  // what the Nature-CNN conv1 strip kernels ask of their operands
    p.variant = g.sub_mean != 0.f;
    // persistent blocks over sample pairs, one partial per block, never more than the workspace was sized for
    auto strip = [&](int blocks, size_t lds) { p.partials = min(min(npairs, blocks), Zws); p.lds = (unsigned)lds; };
    if (norm && conv_norm_strip(g) && strip_ops && tabs16(g)) {
        strip(512, (160 * 32 + 2 * 4 * 20 * 84) * sizeof(float));
        plan_kernel(p, K_CONV1_WGRAD_IMG_NORM, "k_conv1_wgrad_img_norm<2, 4>");
    } else if (conv1_bf16_ok(g, mode, n) && strip_ops) {  // exact products on the bf16 matrix pipe (sf_nn_u8.h)
        strip(2 * num_cus(), (2 * 4 * 20 * 4 * 36 + 3 * 32 * 168) * sizeof(uint16_t));
        plan_kernel(p, K_CONV1_WGRAD_BF16, "k_conv1_wgrad_bf16<%s>", p.variant ? "true" : "false");
    } else if (sw().conv1_img && conv1_img_ok(g, mode, n) && strip_ops) {  // Nature-CNN conv1 on raw frames: strip-image kernel
        strip(512, (160 * 32 + 2 * 4 * 20 * 84) * sizeof(float));
        plan_kernel(p, K_CONV1_WGRAD_IMG, "k_conv1_wgrad_img<2, 4, %s>", p.variant ? "true" : "false");
    } else if (small_linear_wgrad_ok(d) && !o.index) {
        // 27 -> 64 -> 64 encoder layers: 64-row tiles through LDS, fmaf (sf_nn_narrow.h); one partial per work-group
        const int nb = (int)(cdiv64(Mtot, 64) < 256 ? cdiv64(Mtot, 64) : 256);  // (<= what sf_conv_wgrad_workspace sized for)
        p.per_split = cdiv64(cdiv64(Mtot, nb), 64) * 64;
        p.partials = (int)cdiv64(Mtot, p.per_split);
        plan_kernel(p, K_LINEAR_WGRAD_SMALL, "k_linear_wgrad_small");
    } else if (mode == MODE_F32 && !o.index && wgrad_img_variant(d, n)) {
        // conv2 / conv3: persistent LDS-image kernel, every operand byte fetched once, one partial per work-group
        p.variant = wgrad_img_variant(d, n); p.partials = wgrad_img_blocks(d, n); p.block = dim3(p.variant == 1 ? 256 : 512);
        plan_kernel(p, K_WGRAD_IMG, p.variant == 1 ? "k_wgrad_img<64, 9, 9, 3, 1, 1>" : "k_wgrad_img<32, 20, 20, 4, 2, 2>");
    } else if (sw().wgrad_glds && mode == MODE_F32 && !o.index && g.traj_T == 0 && wgrad_glds_wanted(Mtot, K, N) &&
               n * max(o.stride, (int64_t)g.H * g.W * g.Cin) < ((int64_t)1 << 30)) {  // 32-bit byte offsets in the kernel
        // gfx950 LDS-DMA kernel (dense f32 NHWC input): different tiles, so its own split plan and partial layout
        const WgradGlds q = plan_wgrad_glds(Mtot, K, N, true);
        p.partials = p.splits = q.Z; p.per_split = q.m_per_split;
        p.grid = dim3(cdiv64(K, q.BK), cdiv64(N, q.BN), (unsigned)q.Z);
        // XCD-aware block order (sf_nn_glds.h): a 1-D launch whose ids are re-mapped so that every XCD owns a contiguous
        // run of (row tile, column tile, slice) — only worth it when tiles share strips (more than one tile per slice)
        plan_raster(p, sw().xcd_raster && p.grid.x * p.grid.y > 1);
        // linear layers: the zero-VALU reduction loop (k_wgrad_glds_z); SF_WGRAD_ZL=0 switches it off
        const bool zl = sw().wgrad_zl && g.KH == 1 && g.KW == 1 && g.H == 1 && g.W == 1 && g.OH == 1 && g.OW == 1 &&
                        n * o.stride < (1LL << 30) && Mtot * N < (1LL << 30);
        const TileArgs t = {q.BK, q.BN, q.cfg == 0 ? 4 : 2, q.cfg == 0 ? 1 : 2};
        if (zl) plan_tile(p, K_WGRAD_GLDS_Z, "k_wgrad_glds_z", t);
        else plan_tile(p, K_WGRAD_GLDS, "k_wgrad_glds", t);
        return p;
    } else {
        const int bpc = BN == 32 ? occ_wgrad_mode<32, 4, 1>(mode) : occ_wgrad_mode<64, 2, 2>(mode);
        const SplitPlan s = plan_splits(Mtot, K, N, 128, BN, bpc);
        p.variant = mode; p.partials = p.splits = s.Z; p.per_split = s.m_per_split;
        p.grid = dim3(cdiv64(K, 128), cdiv64(N, BN), (unsigned)s.Z);
        p.t = BN == 32 ? TileArgs{128, 32, 4, 1} : TileArgs{128, 64, 2, 2};
        plan_kernel(p, K_CONV_WGRAD, "k_conv_wgrad<%d, %d, %d, %d>", BN, p.t.WM, p.t.WN, mode);
        return p;
    }
    p.grid = dim3((unsigned)p.partials);  // one partial per (persistent) work-group
    return p;
}

// the maximum over the operand facts the query cannot know (alignment, index, occupancy of the kernel that will run)
extern "C" int64_t sf_conv_wgrad_workspace(int64_t n, const sf_conv_desc *h_desc) {
    if (!h_desc || n <= 0) return 0;
    const int K = h_desc->KH * h_desc->KW * h_desc->Cin, N = h_desc->Cout;
    const int64_t Mtot = n * h_desc->OH * h_desc->OW;
    int Z = wgrad_ws_partials(Mtot, K, N);
    if (wgrad_img_variant(h_desc, n) && wgrad_img_blocks(h_desc, n) > Z) Z = wgrad_img_blocks(h_desc, n);  // one partial per work-group
    if (small_linear_wgrad_ok(h_desc)) {  // one partial per 64-row tile, at most 1024
        const int64_t zs = cdiv64(Mtot, 64) < 1024 ? cdiv64(Mtot, 64) : 1024;
        if (zs > Z) Z = (int)zs;
    }
    if (h_desc->in_u8 == IN_F32_NHWC) {  // the LDS-DMA kernel may pick other tiles (hence another split count)
        const WgradGlds q = plan_wgrad_glds(Mtot, K, N);
        if (q.Z > Z) Z = q.Z;
    }
    return (int64_t)sizeof(float) * Z * ((int64_t)K * N + N) + 256;
}

#define WGRAD_LAUNCH(BN, WM, WN, MODE)                                                                                  \
    k_conv_wgrad<BN, WM, WN, MODE><<<p.grid, p.block, 0, st>>>(g, in, in_sample_stride, index, offset, dout, partial_w, \
                                                               partial_b, Mtot, p.per_split)
#define WGRAD_GLDS_ARGS g, inf, in_sample_stride, dout, partial_w, partial_b, Mtot, p.per_split, p.rx, p.ry, p.rtot
#define WGRAD_GLDS(BK_, BN_, WM_, WN_)                                                                                    \
    do {                                                                                                                  \
        if (p.kernel == K_WGRAD_GLDS_Z) k_wgrad_glds_z<BK_, BN_, WM_, WN_><<<p.grid, p.block, 0, st>>>(WGRAD_GLDS_ARGS);  \
        else k_wgrad_glds<BK_, BN_, WM_, WN_><<<p.grid, p.block, 0, st>>>(WGRAD_GLDS_ARGS);                               \
    } while (0)
// the Nature-CNN conv1 strip kernels (dmask: the bf16 kernel alone)
#define WGRAD_STRIP(KERN, ...)                                                                                  \
    KERN<<<p.grid, p.block, p.lds, st>>>(g, reinterpret_cast<const uint8_t *>(in), in_sample_stride, index, offset, dout, \
                                         ##__VA_ARGS__, partial_w, partial_b, (int)n, (int)((n + 1) / 2))

// mu / rstd: the observation normaliser's tables (u8 / f32 frames through sf_conv_wgrad_norm), else NULL
static int conv_wgrad_impl(const void *in, int64_t in_sample_stride, const int32_t *index, int64_t offset,
                           const float *dout, const uint32_t *dmask, float *dw, float *db, int64_t n,
                           const sf_conv_desc *h_desc, void *workspace, void *stream, const float *mu = nullptr,
                           const float *rstd = nullptr) {
    int rc = check_desc(h_desc, "sf_conv_wgrad");
    if (rc) return rc;
    SF_REQUIRE(in && dout && dw && workspace && n > 0, "sf_conv_wgrad: bad args");
    SF_REQUIRE(((uintptr_t)workspace & 15) == 0, "sf_conv_wgrad: workspace must be 16-byte aligned");
    ConvG g = make_geom(h_desc);
    g.nmu = mu; g.nrstd = rstd;
    const int64_t Mtot = n * g.OH * g.OW;
    SF_REQUIRE(Mtot < (1LL << 31), "sf_conv_wgrad: M=%lld exceeds 2^31 rows; split the batch", (long long)Mtot);
    const int K = g.K, N = g.Cout;
    const ConvPlan p = plan_conv_wgrad(h_desc, g, n, Operands{in, in_sample_stride, index != nullptr, nullptr, dout, nullptr, 0});
    SF_REQUIRE(!dmask || p.kernel == K_CONV1_WGRAD_BF16,
               "sf_conv_wgrad_relu_mask: this launch does not resolve to the mask-consuming kernel");
    float *partial_w = reinterpret_cast<float *>(workspace);
    float *partial_b = db ? partial_w + (int64_t)p.partials * K * N : nullptr;
    hipStream_t st = STREAM(stream);
    const float *inf = reinterpret_cast<const float *>(in);
    switch (p.kernel) {
        case K_CONV1_WGRAD_BF16:
            if (p.variant) WGRAD_STRIP(k_conv1_wgrad_bf16<true>, dmask); else WGRAD_STRIP(k_conv1_wgrad_bf16<false>, dmask);
            break;
        case K_CONV1_WGRAD_IMG:
            if (p.variant) WGRAD_STRIP((k_conv1_wgrad_img<2, 4, true>)); else WGRAD_STRIP((k_conv1_wgrad_img<2, 4, false>));
            break;
        case K_LINEAR_WGRAD_SMALL:
            k_linear_wgrad_small<<<p.grid, p.block, 0, st>>>(inf, in_sample_stride, dout, partial_w, partial_b, Mtot, p.per_split, K, N);
            break;
        case K_WGRAD_IMG:
            if (p.variant == 1) k_wgrad_img<64, 9, 9, 3, 1, 1><<<p.grid, p.block, 0, st>>>(inf, in_sample_stride, dout, partial_w, partial_b, (int)n);
            else k_wgrad_img<32, 20, 20, 4, 2, 2><<<p.grid, p.block, 0, st>>>(inf, in_sample_stride, dout, partial_w, partial_b, (int)n);
            break;
        case K_WGRAD_GLDS:
        case K_WGRAD_GLDS_Z:
            if (TILE_IS(64, 128)) WGRAD_GLDS(64, 128, 2, 2);
            else if (TILE_IS(256, 64)) WGRAD_GLDS(256, 64, 4, 1);
            else if (TILE_IS(128, 128)) WGRAD_GLDS(128, 128, 2, 2);
            else WGRAD_GLDS(128, 64, 2, 2);
            break;
        default:  // K_CONV_WGRAD
            if (TILE_IS(128, 32)) { BY_MODE(WGRAD_LAUNCH, 32, 4, 1) }
            else { BY_MODE(WGRAD_LAUNCH, 64, 2, 2) }
    }
    launch_reduce_partials(partial_w, dw, (int64_t)K * N, p.partials, st);
    if (db) launch_reduce_partials(partial_b, db, N, p.partials, st);
    return sf_launch_status("sf_conv_wgrad");
}

extern "C" int sf_conv_wgrad(const void *in, int64_t in_sample_stride, const int32_t *index, int64_t offset,
                             const float *dout, float *dw, float *db, int64_t n, const sf_conv_desc *h_desc,
                             void *workspace, void *stream) {
    return conv_wgrad_impl(in, in_sample_stride, index, offset, dout, nullptr, dw, db, n, h_desc, workspace, stream);
}
extern "C" int sf_conv_wgrad_relu_mask(const void *in, int64_t in_sample_stride, const int32_t *index, int64_t offset,
                                       const float *dout, const uint32_t *relu_mask, float *dw, float *db, int64_t n,
                                       const sf_conv_desc *h_desc, void *workspace, void *stream) {
    SF_REQUIRE(relu_mask && ((uintptr_t)relu_mask & 7) == 0, "sf_conv_wgrad_relu_mask: relu_mask must be an 8-byte aligned device buffer");
    SF_REQUIRE(h_desc && n > 0 && relu_mask_ok(h_desc, n) && ((uintptr_t)in & 3) == 0 && in_sample_stride % 4 == 0 &&
                   ((uintptr_t)dout & 15) == 0,
               "sf_conv_wgrad_relu_mask: unsupported layer / launch (see sf_conv_relu_mask_supported)");
    return conv_wgrad_impl(in, in_sample_stride, index, offset, dout, relu_mask, dw, db, n, h_desc, workspace, stream);
}

extern "C" int sf_conv_norm_supported(int64_t n, const sf_conv_desc *h_desc) {
    return h_desc && check_desc(h_desc, "sf_conv_norm_supported") == 0 && conv_norm_ok(h_desc, n) ? 1 : 0;
}
extern "C" int sf_conv_fwd_norm(const void *in, int64_t in_sample_stride, const int32_t *index, int64_t offset,
                                const float *mu, const float *rstd, const float *w, const float *bias, float *out,
                                int64_t n, const sf_conv_desc *h_desc, void *stream) {
    int rc = check_desc(h_desc, "sf_conv_fwd_norm");
    if (rc) return rc;
    SF_REQUIRE(in && mu && rstd && w && out && n > 0, "sf_conv_fwd_norm: bad args");
    SF_REQUIRE(conv_norm_ok(h_desc, n) && ((uintptr_t)mu & 3) == 0 && ((uintptr_t)rstd & 3) == 0 &&
                   (in_is_u8(h_desc->in_u8) || ((uintptr_t)in & 3) == 0),
               "sf_conv_fwd_norm: unsupported launch (see sf_conv_norm_supported; f32 frames and tables 4-byte aligned)");
    ConvG g = make_geom(h_desc);
    g.nmu = mu; g.nrstd = rstd;
    const ConvPlan p = plan_conv_fwd(h_desc, g, n, Operands{in, in_sample_stride, index != nullptr, w, nullptr, out, 0});
    // every launch but the Nature-CNN conv1 on aligned u8 frames: the register-staged kernel with a normalising loader
    if (p.kernel != K_CONV_U8_IMG_NORM)
        return conv_fwd_impl(in, in_sample_stride, index, offset, w, bias, out, nullptr, n, h_desc, nullptr, 0, stream, mu,
                             rstd);
    SF_REQUIRE(n * g.OH * g.OW < (1LL << 31), "sf_conv_fwd_norm: M exceeds 2^31 rows; split the batch");
    k_conv_u8_img_norm<2, 4, 5, 16><<<p.grid, p.block, p.lds, STREAM(stream)>>>(
        g, reinterpret_cast<const uint8_t *>(in), in_sample_stride, index, offset, w, bias, out, (int)n);
    return sf_launch_status("sf_conv_fwd_norm");
}
extern "C" int sf_conv_wgrad_norm(const void *in, int64_t in_sample_stride, const int32_t *index, int64_t offset,
                                  const float *mu, const float *rstd, const float *dout, float *dw, float *db, int64_t n,
                                  const sf_conv_desc *h_desc, void *workspace, void *stream) {
    int rc = check_desc(h_desc, "sf_conv_wgrad_norm");
    if (rc) return rc;
    SF_REQUIRE(in && mu && rstd && dout && dw && workspace && n > 0, "sf_conv_wgrad_norm: bad args");
    SF_REQUIRE(conv_norm_ok(h_desc, n) && ((uintptr_t)mu & 3) == 0 && ((uintptr_t)rstd & 3) == 0 &&
                   (in_is_u8(h_desc->in_u8) || ((uintptr_t)in & 3) == 0),
               "sf_conv_wgrad_norm: unsupported launch (see sf_conv_norm_supported; f32 frames and tables 4-byte aligned)");
    ConvG g = make_geom(h_desc);
    g.nmu = mu; g.nrstd = rstd;
    const ConvPlan p = plan_conv_wgrad(h_desc, g, n, Operands{in, in_sample_stride, index != nullptr, nullptr, dout, nullptr, 0});
    if (p.kernel != K_CONV1_WGRAD_IMG_NORM)
        return conv_wgrad_impl(in, in_sample_stride, index, offset, dout, nullptr, dw, db, n, h_desc, workspace, stream, mu,
                               rstd);
    SF_REQUIRE(((uintptr_t)workspace & 15) == 0, "sf_conv_wgrad_norm: workspace must be 16-byte aligned");
    const int K = g.K, N = g.Cout;
    float *partial_w = reinterpret_cast<float *>(workspace), *partial_b = db ? partial_w + (int64_t)p.partials * K * N : nullptr;
    hipStream_t st = STREAM(stream);
    WGRAD_STRIP((k_conv1_wgrad_img_norm<2, 4>));
    launch_reduce_partials(partial_w, dw, (int64_t)K * N, p.partials, st);
    if (db) launch_reduce_partials(partial_b, db, N, p.partials, st);
    return sf_launch_status("sf_conv_wgrad_norm");
}

static sf_conv_desc linear_desc(int K, int N, int relu);
static bool linear_dgrad_glds_ok(const ConvG &g, int64_t n) {
    return g.H == 1 && g.W == 1 && g.KH == 1 && g.KW == 1 && g.Cout % 32 == 0 && g.Cin >= 128 &&
           cdiv64(n, 128) * (int64_t)cdiv64(g.Cin, 128) >= 512;
}
// ... and narrow ones (Cin == 64 behind a deep reduction: the data gradient of a recurrent core's input projection,
// 16384 x 2048 -> 64): 128-row tiles are 128 work-groups, half the chip; 64 x 64 tiles fill it
static bool linear_dgrad_glds64_ok(const ConvG &g, int64_t n) {
    return sw().dgrad_linear64 && g.H == 1 && g.W == 1 && g.KH == 1 && g.KW == 1 && g.Cout % 32 == 0 && g.Cout >= 512 &&
           g.Cin == 64 && n >= 8192;
}
// k_dgrad_pix_z (SF_DGRAD_ZL bit 1): per-lane dY / W offsets of the SADDR-form DMA must fit 32 bits, channels in whole 64s
static bool dgrad_pix_zl(const ConvG &g, int64_t n) {
    return (sw().dgrad_zl & 2) && g.Cout % 64 == 0 && n * (int64_t)g.OH * g.OW * g.Cout < (1LL << 30) &&
           (int64_t)g.K * g.Cout < (1LL << 30);
}
// k_dgrad_quadrow_z addresses dY / W lanes as 32-bit element offsets and the input-gradient / activation elements as
// 32-bit BYTE offsets from a uniform base: both tensors must stay below 2^30 elements
static bool dgrad_quadrow_zl(const ConvG &g, int64_t n) {
    return (sw().dgrad_zl & 1) && g.Cout % 64 == 0 && n * (int64_t)g.OH * g.OW * g.Cout < (1LL << 30) &&
           (int64_t)g.K * g.Cout < (1LL << 30) && n * (int64_t)g.H * g.W * g.Cin < (1LL << 30);
}
// Column classes of the row-walking strided data gradient (sf_nn_glds.h): runs of group columns iwc with the same tap
// columns b in [max(0, iwc - OW + 1), min(KW/S - 1, iwc)] inside dY, each padded to whole BM-row tiles.  Launch order:
// the classes with the most tap columns first (conv2 at n = 32768: 2048 interior tiles = four full rounds of the 512
// resident work-groups, then the 2 x 256 border tiles with half the chunks).  Returns the tile count.
static unsigned plan_quadrow_classes(QuadrowClasses &q, const ConvG &g, int64_t n, int BM) {
    const int Wg = g.W / g.S, KWs = g.KW / g.S;
    q.ncls = 0;
    q.n = (uint32_t)n;
    for (int iwc = 0; iwc < Wg; ++iwc) {
        const int lo = std::max(0, iwc - g.OW + 1), nb = std::max(0, std::min(KWs - 1, iwc) - lo + 1);
        QuadrowClass *last = q.ncls ? &q.c[q.ncls - 1] : nullptr;
        if (last && last->nb == nb && (nb == 0 || last->b_lo == lo)) { ++last->dw.d; continue; }
        QuadrowClass &c = q.c[q.ncls++];
        c.col0 = iwc; c.b_lo = lo; c.nb = nb; c.dw.d = 1;
    }
    std::stable_sort(q.c, q.c + q.ncls, [](const QuadrowClass &a, const QuadrowClass &b) {
        return a.nb != b.nb ? a.nb > b.nb : a.dw.d > b.dw.d;  // most chunks per step first
    });
    unsigned tiles = 0;
    for (int i = 0; i < q.ncls; ++i) {
        q.c[i].tile0 = tiles;
        tiles += cdiv64(n * (int64_t)q.c[i].dw.d, BM);
        q.c[i].dw = make_fastdiv(q.c[i].dw.d);
    }
    return tiles;
}
// sf_conv_dgrad.  plan.variant: k_conv_dgrad's VEC argument
static ConvPlan plan_conv_dgrad(const ConvG &g, int64_t n, const Operands &o) {
    ConvPlan p = plan_init();
    const bool al16 = aligned(o.dout, 16) && aligned(o.w, 16), vec = g.vecB && al16;
    p.per_split = (g.Cout + 31) / 32 * 32;  // the linear forms: the forward GEMM's k_per_split
    // Linear layer (1x1 on a 1x1 image): din[n, Cin] = dY[n, Cout] * W^T is the forward GEMM of the LDS-DMA kernel with
    // the canonical [Cin, Cout] weight array AS its Cout-major operand (no transpose needed) and a mask epilogue:
    // 128x128 tiles, 64x64 per wave (fc layer at n = 32768: 105 -> 120 TFLOP/s against the pixel-major kernel).
    const bool zl_fits = n * (int64_t)g.Cout < (1LL << 30) && (int64_t)g.Cin * g.Cout < (1LL << 30);
    if (sw().dgrad_linear && linear_dgrad_glds_ok(g, n) && al16) {
        p.grid = dim3(cdiv64(n, 128), cdiv64(g.Cin, 128), 1);
        // (measured slower for this launch — 950 vs 930 us at n = 32768: both orders re-read one operand from the Infinity
        // Cache, and the row-strip order sweeps the 6.4 MB weight matrix per strip — so only SF_XCD_RASTER=2 enables it here)
        plan_raster(p, sw().xcd_raster >= 2 && p.grid.y > 1);
        if (sw().glds_zl >= 2 && zl_fits) plan_tile(p, K_FWD_GLDS_Z, "k_fwd_glds_z", TileArgs{128, 128, 2, 2});
        else plan_tile(p, K_FWD_GLDS, "k_fwd_glds", TileArgs{128, 128, 2, 2}, ", 2");
        return p;
    }
    if (sw().dgrad_linear && linear_dgrad_glds64_ok(g, n) && al16) {
        p.grid = dim3(cdiv64(n, 64), 1, 1);
        if (sw().glds_zl && zl_fits) plan_tile(p, K_FWD_GLDS_Z, "k_fwd_glds_z", TileArgs{64, 64, 2, 2});
        else plan_tile(p, K_FWD_GLDS, "k_fwd_glds", TileArgs{64, 64, 2, 2}, ", 2");
        return p;
    }
    // pixel-major LDS-DMA kernel: needs enough samples to fill BM-sample row tiles and Cout % 32 == 0
    // (SF_DGRAD_PIX: 0 = off, 2 = 128-sample tiles for Cin <= 32, 3 = strided convs too instead of the row-walking kernel)
    const int pix_cfg = sw().dgrad_pix;
    if (pix_cfg && vec && g.Cout % 32 == 0 && n >= 1024) {
        // zero-VALU reduction loop (k_dgrad_pix_z / k_dgrad_quadrow_z): per-lane operand offsets must fit 32 bits
        // SF_DGRAD_ZL (default 3): bit 0 = k_dgrad_quadrow_z (conv2: 1918 / 1921 -> 1877 / 1892 us at n = 32768), bit 1 =
        // k_dgrad_pix_z with SADDR-form DMA only (conv3: 1308 / 1316 -> 1277 / 1297 us; the full form — pointer fragment reads,
        // two chunks per trip — costs hipcc 256 + 168 registers against 173 + 32 and the second wave per SIMD with them:
        // 1214 -> 1316 us, compile-time switch SF_DGRAD_PIX_ZL_LITE=0) — profiles/r05_k_dgrad_zl_ab.log, r05_n_dgrad_pix_lite_ab.log
        if (g.S > 1 && g.KH % g.S == 0 && g.KW % g.S == 0 && g.W % g.S == 0 && pix_cfg != 3 &&
            2 * (g.KW / g.S) - 1 <= SF_QUADROW_MAX_CLASSES) {
            // strided conv, row-walking tiles of (sample, group-column) rows: contiguous activation / gradient rows
            p.grid = dim3(plan_quadrow_classes(p.qr, g, n, 128), cdiv64(g.S * g.S * g.Cin, 128));
            if (dgrad_quadrow_zl(g, n)) plan_tile(p, K_DGRAD_QUADROW_Z, "k_dgrad_quadrow_z", TileArgs{128, 128, 2, 2});
            else plan_tile(p, K_DGRAD_QUADROW, "k_dgrad_quadrow", TileArgs{128, 128, 2, 2});
            return p;
        }
        const TileArgs t = g.Cin <= 32 ? TileArgs{pix_cfg == 2 ? 128 : 256, 32, 4, 1} : TileArgs{128, 64, 2, 2};
        const int ntiles = (int)((n + t.BM - 1) / t.BM), tiles8 = (ntiles + 7) / 8, ctiles = (g.Cin + t.BN - 1) / t.BN;
        p.rx = ntiles; p.ry = tiles8;  // (kernel arguments of the pixel-major kernel, not a raster)
        p.grid = dim3((unsigned)(tiles8 * 8 * g.H * ctiles));
        if (dgrad_pix_zl(g, n)) plan_tile(p, K_DGRAD_PIX_Z, "k_dgrad_pix_z", t);
        else plan_tile(p, K_DGRAD_PIX, "k_dgrad_pix", t);
        return p;
    }
    const int64_t Mc = n * ((g.H + g.S - 1) / g.S) * ((g.W + g.S - 1) / g.S);  // rows of the largest parity class
    const TileArgs t = g.Cin <= 32 ? TileArgs{128, 32, 4, 1} : Mc * ((g.Cin + 63) / 64) < 128LL * 1024 ? TileArgs{64, 64, 2, 2} : TileArgs{128, 64, 2, 2};
    p.variant = vec;
    p.grid = dim3(cdiv64(Mc, t.BM), cdiv64(g.Cin, t.BN), (unsigned)(g.S * g.S));
    plan_tile(p, K_CONV_DGRAD, "k_conv_dgrad", t, vec ? ", true" : ", false");
    return p;
}

#define DGRAD_LAUNCH(BM, BN, WM, WN)                                                                                \
    do {                                                                                                            \
        if (p.variant) k_conv_dgrad<BM, BN, WM, WN, true><<<p.grid, p.block, 0, st>>>(g, dout, w, in_act, din, n);  \
        else k_conv_dgrad<BM, BN, WM, WN, false><<<p.grid, p.block, 0, st>>>(g, dout, w, in_act, din, n);           \
    } while (0)
// SF_DGRAD_LPT (default 1): longest rows first (k_dgrad_pix block order, sf_nn_glds.h); 0: row-major block ids
#define DGRAD_PIX_ARGS g, dout, w, in_act, din, (int)n, p.rx, p.ry, sw().dgrad_lpt
#define DGRAD_PIX(BM, BN, WM, WN)                                                                                \
    do {                                                                                                         \
        if (p.kernel == K_DGRAD_PIX_Z) k_dgrad_pix_z<BM, BN, WM, WN><<<p.grid, p.block, 0, st>>>(DGRAD_PIX_ARGS); \
        else k_dgrad_pix<BM, BN, WM, WN><<<p.grid, p.block, 0, st>>>(DGRAD_PIX_ARGS);                            \
    } while (0)
// the linear forms: the masked forward GEMM on the transposed problem (reduction = Cout, columns = Cin, relu = kind of in_act)
#define DGRAD_LIN_ARGS g2, dout, g.Cout, w, nullptr, din, n, (int)p.per_split, nullptr, in_act, 1, p.rx, p.ry, p.rtot
#define DGRAD_LINEAR(BM, BN)                                                                                      \
    do {                                                                                                          \
        if (p.kernel == K_FWD_GLDS_Z) k_fwd_glds_z<BM, BN, 2, 2><<<p.grid, p.block, 0, st>>>(DGRAD_LIN_ARGS);     \
        else k_fwd_glds<BM, BN, 2, 2, 2><<<p.grid, p.block, 0, st>>>(DGRAD_LIN_ARGS);                             \
    } while (0)
extern "C" int sf_conv_dgrad(const float *dout, const float *w, const float *in_act, float *din, int64_t n,
                             const sf_conv_desc *h_desc, void *stream) {
    int rc = check_desc(h_desc, "sf_conv_dgrad");
    if (rc) return rc;
    SF_REQUIRE(dout && w && din && n > 0, "sf_conv_dgrad: bad args");
    SF_REQUIRE(!in_is_frame(h_desc->in_u8), "sf_conv_dgrad: the observation layer has no data gradient");
    SF_REQUIRE(h_desc->Cout % 4 == 0 || (h_desc->KH == 1 && h_desc->KW == 1),
               "sf_conv_dgrad: Cout must be a multiple of 4 for spatial kernels");
    const ConvG g = make_geom(h_desc);
    SF_REQUIRE(n * g.H * g.W < (1LL << 31) && n * g.OH * g.OW * (int64_t)g.Cout < (1LL << 31) &&
                   (int64_t)g.K * g.Cout < (1LL << 31),
               "sf_conv_dgrad: operand too large for 32-bit element offsets; split the batch");
    hipStream_t st = STREAM(stream);
    const ConvPlan p = plan_conv_dgrad(g, n, Operands{nullptr, 0, false, w, dout, nullptr, 0});
    switch (p.kernel) {
        case K_FWD_GLDS:
        case K_FWD_GLDS_Z: {
            const sf_conv_desc d2 = linear_desc(g.Cout, g.Cin, g.relu);
            const ConvG g2 = make_geom(&d2);
            if (TILE_IS(128, 128)) DGRAD_LINEAR(128, 128); else DGRAD_LINEAR(64, 64);
            break;
        }
#define QUADROW_ARGS g, dout, w, in_act, din, p.qr
        case K_DGRAD_QUADROW_Z: k_dgrad_quadrow_z<128, 128, 2, 2><<<p.grid, p.block, 0, st>>>(QUADROW_ARGS); break;
        case K_DGRAD_QUADROW: k_dgrad_quadrow<128, 128, 2, 2><<<p.grid, p.block, 0, st>>>(QUADROW_ARGS); break;
#undef QUADROW_ARGS
        case K_DGRAD_PIX:
        case K_DGRAD_PIX_Z:
            if (TILE_IS(128, 32)) DGRAD_PIX(128, 32, 4, 1);
            else if (TILE_IS(256, 32)) DGRAD_PIX(256, 32, 4, 1);
            else DGRAD_PIX(128, 64, 2, 2);
            break;
        default:  // K_CONV_DGRAD
            if (TILE_IS(128, 32)) DGRAD_LAUNCH(128, 32, 4, 1);
            else if (TILE_IS(64, 64)) DGRAD_LAUNCH(64, 64, 2, 2);
            else DGRAD_LAUNCH(128, 64, 2, 2);
    }
    return sf_launch_status("sf_conv_dgrad");
}

#if SF_CONV1_TRACE
// experiment builds only (tools/conv1_trace.py): read and clear the per-phase cycle sums of k_conv1_u8_bf16
extern "C" int sf_debug_conv1_trace(unsigned long long *host_out12) {
    hipDeviceSynchronize();
    if (hipMemcpyFromSymbol(host_out12, HIP_SYMBOL(sf_conv1_trace_acc), 12 * sizeof(unsigned long long)) != hipSuccess) return 1;
    unsigned long long z[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    return hipMemcpyToSymbol(HIP_SYMBOL(sf_conv1_trace_acc), z, sizeof(z)) == hipSuccess ? 0 : 1;
}
#endif
// Name of the kernel instantiation a launch with these arguments resolves to, spelled the way rocprofv3 prints it, so that
// bench.py can group its HIP-event timings exactly like the rocprof kernel stats: the name of the plan the launcher itself
// would run for query_operands() (aligned operands and tables, dense samples, no index; a split-K workspace if allowed).
// op: 0 sf_conv_fwd, 1 sf_conv_wgrad, 2 sf_conv_dgrad, 3 sf_conv_fwd_t, 4 sf_conv_fwd_norm, 5 sf_conv_wgrad_norm,
// 6 sf_conv_fwd_relu_mask_os, 7 sf_conv_fwd_t_os (the strided-output twins, the same for their two-segment entry points; a
// linear layer under op 7: k_fwd_glds_z_os<64, 64, 2, 2>)
extern "C" int sf_conv_kernel_name(int op, int64_t n, const sf_conv_desc *h_desc, int split_k_allowed, char *out,
                                   int cap) {
    int rc = check_desc(h_desc, "sf_conv_kernel_name");
    if (rc) return rc;
    SF_REQUIRE(out && cap >= 48 && n > 0 && op >= 0 && op <= 7, "sf_conv_kernel_name: bad args");
    const Operands o = query_operands(h_desc, split_k_allowed != 0);
    ConvG g = make_geom(h_desc);
    if (op == 4 || op == 5) g.nmu = g.nrstd = TABLE_PROBE;
    ConvPlan p = op == 3 ? plan_conv_fwd_t(h_desc, n, o.stride) : op == 2 ? plan_conv_dgrad(g, n, o)
                 : op == 7 ? plan_conv_fwd_t(h_desc, n, o.stride, nullptr, true)
                 : (op == 0 || op == 4 || op == 6) ? plan_conv_fwd(h_desc, g, n, o) : plan_conv_wgrad(h_desc, g, n, o);
    if (op == 6) {
        if (p.kernel == K_CONV1_U8_BF16_W && relu_mask_ok(h_desc, n)) plan_os_name(p);
        else p.kernel = K_NONE;
    }
    if (op == 7 && (p.kernel == K_LINEAR_NARROW || p.splits != 1)) p.kernel = K_NONE;
    SF_REQUIRE(p.kernel != K_NONE, "sf_conv_kernel_name: not a launch %s accepts",
               op >= 6 ? "sf_conv_fwd_os_supported" : op >= 4 ? "sf_conv_norm_supported" : "sf_conv_fwd_t");
    strncpy(out, p.name, (size_t)cap - 1);
    out[cap - 1] = 0;
    return SF_OK;
}

// ---- dense layers = 1x1 conv on a 1x1 image
static sf_conv_desc linear_desc(int K, int N, int relu) {
    sf_conv_desc d;
    d.Cin = K; d.H = 1; d.W = 1; d.Cout = N; d.KH = 1; d.KW = 1; d.stride = 1; d.OH = 1; d.OW = 1;
    d.in_u8 = 0; d.relu = relu; d.traj_T = 0; d.sub_mean = 0.f; d.inv_scale = 1.f;
    return d;
}

extern "C" int sf_linear_fwd(const float *in, const float *w, const float *bias, float *out, int64_t M, int K, int N,
                             int relu, void *stream) {
    SF_REQUIRE(M > 0 && K > 0 && N > 0, "sf_linear_fwd: bad shape");
    const sf_conv_desc d = linear_desc(K, N, relu);
    return sf_conv_fwd(in, K, nullptr, 0, w, bias, out, M, &d, nullptr, 0, stream);
}
extern "C" int64_t sf_linear_wgrad_workspace(int64_t M, int K, int N) {
    const sf_conv_desc d = linear_desc(K, N, 0);
    return sf_conv_wgrad_workspace(M, &d);
}
extern "C" int sf_linear_wgrad(const float *in, const float *dout, float *dw, float *db, int64_t M, int K, int N,
                               void *workspace, void *stream) {
    SF_REQUIRE(M > 0 && K > 0 && N > 0, "sf_linear_wgrad: bad shape");
    const sf_conv_desc d = linear_desc(K, N, 0);
    return sf_conv_wgrad(in, K, nullptr, 0, dout, dw, db, M, &d, workspace, stream);
}
extern "C" int sf_linear_dgrad(const float *dout, const float *w, const float *in_act, float *din, int64_t M, int K,
                               int N, void *stream) {
    SF_REQUIRE(M > 0 && K > 0 && N > 0, "sf_linear_dgrad: bad shape");
    const sf_conv_desc d = linear_desc(K, N, in_act ? 1 : 0);  // this wrapper's contract: ReLU mask of in_act
    return sf_conv_dgrad(dout, w, in_act, din, M, &d, stream);
}

extern "C" int sf_relu_mask(float *g, const float *act, int64_t n, void *stream) {
    SF_REQUIRE(g && act && n >= 0, "sf_relu_mask: bad args");
    if (n == 0) return SF_OK;
    const unsigned blocks = cdiv64(n, 256) < 4096 ? cdiv64(n, 256) : 4096;
    k_relu_mask<<<dim3(blocks), dim3(256), 0, STREAM(stream)>>>(g, act, n);
    return sf_launch_status("sf_relu_mask");
}
