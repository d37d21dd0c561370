// sf_linear_bf16.hip — the fully connected layers on v_mfma_f32_16x16x32_bf16 (cfg.mlp_bf16): dense f32 rows in [n, K],
// w [K, N], out / dout [n, N] with K % 8 == 0, N % 8 == 0, any n >= 1.  Reached by name only (sf_linear_*_bf16); the plain
// sf_linear_* / sf_conv_* never route here.
//
// Arithmetic (the conv family's, sf_conv_bf16.hip): both MFMA operands are rounded to bf16 once per element, to nearest even.
// Accumulation is fp32; bias, activation and activation derivative are fp32 on unrounded values; db is the sum of the
// rounded dout.  Tensors and weights stay fp32 in memory and are converted on their way into LDS: no bf16 copy outlives a
// launch.
//
// All three passes are C[I, J] = sum_r A[i][r] B[r][j] on one tile machine: a work-group (4 waves) owns 128 x 128 outputs
// and walks the reduction in stages of 64.  Both operand tiles live in LDS as bf16 with the REDUCTION index contiguous,
// T[128][64 + 8]: the row pitch of 144 bytes is an odd number of 16-byte words, so the 16 rows of a lane group's
// ds_read_b128 spread over the banks.  2 x 18432 bytes per work-group.  A wave owns 64 x 64 outputs: 4 A fragments and
// 4 B fragments (one ds_read_b128 each) feed 16 MFMAs per 32 reduction elements.  The next stage's global loads are issued
// into registers before the current stage's MFMAs and written to LDS behind them (one LDS buffer, two barriers a stage).
//
// An operand reaches LDS in one of two ways, both 16-byte global loads and 16-byte LDS stores:
//   * lb_load_rows: the reduction index is contiguous in memory (in rows for the forward, dout rows and w rows for the data
//     gradient).  A thread takes 8 consecutive floats of one row, four times, rounds and stores them.
//   * lb_load_cols: the reduction index is the ROW of the matrix in memory (w for the forward; in and dout for the weight
//     gradient, whose reduction runs over the samples).  A thread takes a float4 from each of 8 consecutive rows (32 lanes
//     cover 512 contiguous bytes of a row), transposes the 8 x 4 block in registers and stores four 8-element runs.
//   The forward transposes w [K, N] this way instead of reading a kept [N, K] copy: the model keeps such a copy only for
//   K % 32 == 0, N >= 32 layers and refreshes it after every update, so an entry point built on it would serve fewer shapes
//   and could read a stale copy; the transpose costs no extra global traffic.
//   Tails are zero-filled on load (rows past the matrix, reduction elements past its end) and guarded on store.
//
// k_linear_bf16 (forward and data gradient): tile (rt, ct) = 128 rows x 128 produced columns, the whole reduction, in stage
// order: an output element's value depends on its own row alone, never on n or on the row's place in the launch, and there
// is no split-K.  The column tiles of one row tile are consecutive logical work-groups, and logical work-group ids are
// dealt to the 8 XCDs in contiguous runs (hardware id h -> logical (h % 8) * runs + h / 8), so the tiles that re-read one
// A row tile meet in one L2.
//
// k_linear_wgrad_bf16: tile = 128 K-indices x 128 N-indices, the sample rows cut into chunks of 64 and the chunks into
// `parts` contiguous runs (lb_parts: as many as bring the grid to about 1024 work-groups).  Part p writes its fp32 tile to
// workspace [parts][K*N + N]; the bias gradient is one more MFMA against ones in the tiles of the first K block.
// k_res_conv_wgrad_sum (sf_resnet.hip) adds the parts in part order: no float atomics.
//
// Compiled with -ffp-contract=off like its siblings: the epilogues round after each op.
#include "sf_common.h"
#include "sf_resnet_shared.h"
#include "sf_bf16.h"

#define STREAM(s) reinterpret_cast<hipStream_t>(s)

namespace {

constexpr int LB_T = 128;             // outputs of a tile, both ways
constexpr int LB_KC = 64;             // reduction elements of a stage
constexpr int LB_PITCH = LB_KC + 8;   // bf16 elements of an LDS row
constexpr int LB_XCD = 8;
constexpr int LB_WGRAD_GRID = 1024;   // work-groups the weight gradient aims at: tiles x parts

// T[i][k] = X[(i0 + i) * ld + k0 + k], zero for i0 + i >= I or k0 + k >= R (R % 8 == 0: a run of 8 is in or out as a whole)
__device__ __forceinline__ void lb_load_rows(float4 (&v)[8], const float *__restrict__ X, int64_t ld, int64_t i0, int64_t I,
                                             int64_t k0, int64_t R) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int u = threadIdx.x + 256 * q, kq = u & 7, i = u >> 3;
        v[2 * q] = v[2 * q + 1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (i0 + i < I && k0 + 8 * kq < R) {
            const float4 *p = reinterpret_cast<const float4 *>(X + (i0 + i) * ld + k0 + 8 * kq);
            v[2 * q] = p[0];
            v[2 * q + 1] = p[1];
        }
    }
}

__device__ __forceinline__ void lb_store_rows(__bf16 *T, const float4 (&v)[8]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int u = threadIdx.x + 256 * q, kq = u & 7, i = u >> 3;
        bf16x8 r;
        r[0] = (__bf16)v[2 * q].x; r[1] = (__bf16)v[2 * q].y; r[2] = (__bf16)v[2 * q].z; r[3] = (__bf16)v[2 * q].w;
        r[4] = (__bf16)v[2 * q + 1].x; r[5] = (__bf16)v[2 * q + 1].y; r[6] = (__bf16)v[2 * q + 1].z; r[7] = (__bf16)v[2 * q + 1].w;
        *reinterpret_cast<bf16x8 *>(T + i * LB_PITCH + 8 * kq) = r;
    }
}

// T[i][k] = X[(k0 + k) * ld + i0 + i], zero for i0 + i >= I or k0 + k >= R (I % 4 == 0: a float4 is in or out as a whole)
__device__ __forceinline__ void lb_load_cols(float4 (&v)[8], const float *__restrict__ X, int64_t ld, int64_t i0, int64_t I,
                                             int64_t k0, int64_t R) {
    const int cg = threadIdx.x & 31, rg = threadIdx.x >> 5;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int64_t k = k0 + 8 * rg + e;
        v[e] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (i0 + 4 * cg < I && k < R) v[e] = *reinterpret_cast<const float4 *>(X + k * ld + i0 + 4 * cg);
    }
}

__device__ __forceinline__ void lb_store_cols(__bf16 *T, const float4 (&v)[8]) {
    const int cg = threadIdx.x & 31, rg = threadIdx.x >> 5;
    bf16x8 r[4];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        r[0][e] = (__bf16)v[e].x;
        r[1][e] = (__bf16)v[e].y;
        r[2][e] = (__bf16)v[e].z;
        r[3][e] = (__bf16)v[e].w;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) *reinterpret_cast<bf16x8 *>(T + (4 * cg + c) * LB_PITCH + 8 * rg) = r[c];
}

template <bool COLS>
__device__ __forceinline__ void lb_load(float4 (&v)[8], const float *__restrict__ X, int64_t ld, int64_t i0, int64_t I,
                                        int64_t k0, int64_t R) {
    if (COLS) lb_load_cols(v, X, ld, i0, I, k0, R);
    else lb_load_rows(v, X, ld, i0, I, k0, R);
}

template <bool COLS>
__device__ __forceinline__ void lb_store(__bf16 *T, const float4 (&v)[8]) {
    if (COLS) lb_store_cols(T, v);
    else lb_store_rows(T, v);
}

// One staged 128 x 128 x (32 * ksteps) product.  Wave (wm, wn) owns rows 64*wm .. + 63 of TA and 64*wn .. + 63 of TB;
// acc[f][u][j] is output (64*wm + 16*f + 4*lg + j, 64*wn + 16*u + lr).  BIAS: accb[u][0] of the lanes with lg == 0 gathers
// the column sums of TB (an A operand of ones).
template <bool BIAS>
__device__ __forceinline__ void lb_mma(const __bf16 *TA, const __bf16 *TB, floatx4 (&acc)[4][4], floatx4 (&accb)[4],
                                       int ksteps, int wm, int wn, int lr, int lg, bool bias_on) {
    for (int ks = 0; ks < ksteps; ++ks) {
        bf16x8 a[4], b[4];
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            a[f] = *reinterpret_cast<const bf16x8 *>(TA + (64 * wm + 16 * f + lr) * LB_PITCH + 32 * ks + 8 * lg);
            b[f] = *reinterpret_cast<const bf16x8 *>(TB + (64 * wn + 16 * f + lr) * LB_PITCH + 32 * ks + 8 * lg);
        }
#pragma unroll
        for (int f = 0; f < 4; ++f)
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[f][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[f], b[u], acc[f][u], 0, 0, 0);
        if (BIAS && bias_on) {
            const bf16x8 ones8 = bf16_ones8();
#pragma unroll
            for (int u = 0; u < 4; ++u) accb[u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones8, b[u], accb[u], 0, 0, 0);
        }
    }
}

__device__ __forceinline__ void lb_zero(floatx4 (&acc)[4][4], floatx4 (&accb)[4]) {
#pragma unroll
    for (int f = 0; f < 4; ++f) {
        accb[f] = (floatx4){0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[f][u] = (floatx4){0.0f, 0.0f, 0.0f, 0.0f};
    }
}

// DGRAD = false: A = in [M, R = K], W = w [R, Cn = N],  out = act(A W + bias) [M, Cn].
// DGRAD = true:  A = dout [M, R = N], W = w [Cn = K, R], out = din = (A W^T) * act'(in_act) [M, Cn].
template <bool DGRAD>
__global__ __launch_bounds__(256) void k_linear_bf16(const float *__restrict__ A, const float *__restrict__ W,
                                                     const float *__restrict__ bias, const float *__restrict__ in_act,
                                                     float *__restrict__ out, int act, int64_t M, int R, int Cn, int nct,
                                                     int64_t tiles) {
    __shared__ __attribute__((aligned(16))) __bf16 TA[LB_T * LB_PITCH];
    __shared__ __attribute__((aligned(16))) __bf16 TB[LB_T * LB_PITCH];
    const int64_t runs = gridDim.x / LB_XCD;  // (the grid is a multiple of LB_XCD)
    const int64_t tile = (int64_t)(blockIdx.x % LB_XCD) * runs + blockIdx.x / LB_XCD;
    if (tile >= tiles) return;  // (the whole work-group: no barrier is left waiting)
    const int64_t i0 = (tile / nct) * LB_T;
    const int c0 = (int)(tile % nct) * LB_T;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave & 1, wn = wave >> 1, lr = lane & 15, lg = lane >> 4;
    floatx4 acc[4][4], accb[4];
    lb_zero(acc, accb);
    float4 va[8], vb[8];
    lb_load<false>(va, A, R, i0, M, 0, R);
    lb_load<!DGRAD>(vb, W, DGRAD ? R : Cn, c0, Cn, 0, R);
    for (int k0 = 0; k0 < R; k0 += LB_KC) {
        __syncthreads();  // the previous stage's fragments have been read
        lb_store<false>(TA, va);
        lb_store<!DGRAD>(TB, vb);
        __syncthreads();
        if (k0 + LB_KC < R) {
            lb_load<false>(va, A, R, i0, M, k0 + LB_KC, R);
            lb_load<!DGRAD>(vb, W, DGRAD ? R : Cn, c0, Cn, k0 + LB_KC, R);
        }
        lb_mma<false>(TA, TB, acc, accb, R - k0 > 32 ? 2 : 1, wm, wn, lr, lg, false);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int col = c0 + 64 * wn + 16 * u + lr;
        if (col >= Cn) continue;
        const float bo = DGRAD ? 0.0f : bias[col];
#pragma unroll
        for (int f = 0; f < 4; ++f) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t row = i0 + 64 * wm + 16 * f + 4 * lg + j;
                if (row >= M) continue;
                const int64_t idx = row * Cn + col;
                float v = acc[f][u][j];
                if (DGRAD) {
                    if (in_act != nullptr) v = v * act_bwd_out(act, in_act[idx]);
                    out[idx] = v;
                } else {
                    v = v + bo;
                    out[idx] = act_fwd(act, v);
                }
            }
        }
    }
}

// grid (tiles of dw, parts).  Part p reduces the sample chunks [p * cpp, min(NT, (p + 1) * cpp)) of 64 rows each.
__global__ __launch_bounds__(256) void k_linear_wgrad_bf16(const float *__restrict__ in, const float *__restrict__ dout,
                                                           float *__restrict__ part, int64_t n, int K, int N, int nct,
                                                           int64_t cpp, int64_t NT) {
    __shared__ __attribute__((aligned(16))) __bf16 TA[LB_T * LB_PITCH];
    __shared__ __attribute__((aligned(16))) __bf16 TB[LB_T * LB_PITCH];
    const int kt = blockIdx.x / nct, i0 = kt * LB_T, c0 = (blockIdx.x % nct) * LB_T;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave & 1, wn = wave >> 1, lr = lane & 15, lg = lane >> 4;
    const bool do_bias = kt == 0 && wm == 0;
    floatx4 acc[4][4], accb[4];
    lb_zero(acc, accb);
    const int64_t ch0 = (int64_t)blockIdx.y * cpp, ch1 = min(NT, ch0 + cpp);
    float4 va[8], vb[8];
    lb_load<true>(va, in, K, i0, K, ch0 * LB_KC, n);
    lb_load<true>(vb, dout, N, c0, N, ch0 * LB_KC, n);
    for (int64_t ch = ch0; ch < ch1; ++ch) {
        const int64_t r0 = ch * LB_KC;
        __syncthreads();  // the previous chunk's fragments have been read
        lb_store<true>(TA, va);
        lb_store<true>(TB, vb);
        __syncthreads();
        if (ch + 1 < ch1) {
            lb_load<true>(va, in, K, i0, K, r0 + LB_KC, n);
            lb_load<true>(vb, dout, N, c0, N, r0 + LB_KC, n);
        }
        lb_mma<true>(TA, TB, acc, accb, n - r0 > 32 ? 2 : 1, wm, wn, lr, lg, do_bias);
    }
    const int64_t KN = (int64_t)K * N;
    float *pp = part + (int64_t)blockIdx.y * (KN + N);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int col = c0 + 64 * wn + 16 * u + lr;
        if (col >= N) continue;
#pragma unroll
        for (int f = 0; f < 4; ++f) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = i0 + 64 * wm + 16 * f + 4 * lg + j;
                if (row < K) pp[(int64_t)row * N + col] = acc[f][u][j];
            }
        }
        if (do_bias && lg == 0) pp[KN + col] = accb[u][0];
    }
}

// op 0 forward, 1 weight gradient, 2 data gradient
bool lb_served(int op, int64_t n, int K, int N) {
    if (op < 0 || op > 2 || n < 1 || K < 8 || N < 8 || (K & 7) || (N & 7)) return false;
    if ((int64_t)K * N + N > 0x7fffffffLL) return false;  // the parts' sum indexes a part with an int
    const int64_t tiles = op == 1 ? ceil_div<int64_t>(K, LB_T) * ceil_div<int64_t>(N, LB_T)
                                  : ceil_div<int64_t>(n, LB_T) * ceil_div<int64_t>(op == 0 ? N : K, LB_T);
    return tiles <= 0x7fffffffLL - LB_XCD;
}

struct LbParts {
    int64_t tiles, NT, cpp, parts;  // dw tiles, 64-row chunks, chunks per part, parts
};

LbParts lb_parts(int64_t n, int K, int N) {
    LbParts p;
    p.tiles = ceil_div<int64_t>(K, LB_T) * ceil_div<int64_t>(N, LB_T);
    p.NT = ceil_div<int64_t>(n, LB_KC);
    const int64_t target = std::max<int64_t>(1, LB_WGRAD_GRID / p.tiles);
    p.cpp = ceil_div<int64_t>(p.NT, target);
    p.parts = ceil_div<int64_t>(p.NT, p.cpp);
    return p;
}

int lb_check(int op, int64_t n, int K, int N, int act, const char *what) {
    if (!lb_served(op, n, K, N) || act < 0 || act > 3) {
        snprintf(sf_err_buf, sizeof(sf_err_buf), "%s: n=%lld K=%d N=%d act=%d (the bf16 linear family serves n >= 1, K %% 8 == 0, "
                 "N %% 8 == 0, K >= 8, N >= 8, activation kinds 0..3)", what, (long long)n, K, N, act);
        return SF_ERR_UNSUPPORTED;
    }
    return SF_OK;
}

template <bool DGRAD>
void lb_launch(hipStream_t s, const float *A, const float *W, const float *bias, const float *in_act, float *out, int act,
               int64_t M, int R, int Cn) {
    const int nct = (int)ceil_div<int64_t>(Cn, LB_T);
    const int64_t tiles = ceil_div<int64_t>(M, LB_T) * nct;
    const unsigned grid = (unsigned)(ceil_div<int64_t>(tiles, LB_XCD) * LB_XCD);
    hipLaunchKernelGGL((k_linear_bf16<DGRAD>), dim3(grid), dim3(256), 0, s, A, W, bias, in_act, out, act, M, R, Cn, nct, tiles);
}

}  // namespace

extern "C" int sf_linear_bf16_supported(int op, int64_t n, int K, int N) { return lb_served(op, n, K, N) ? 1 : 0; }

extern "C" int sf_linear_fwd_bf16(const float *in, const float *w, const float *bias, float *out, int64_t n, int K, int N,
                                  int act, void *stream) {
    int rc = lb_check(0, n, K, N, act, "sf_linear_fwd_bf16");
    if (rc) return rc;
    SF_REQUIRE(in && w && bias && out, "sf_linear_fwd_bf16: NULL operand");
    SF_REQUIRE(aligned16(in) && aligned16(w) && aligned16(out), "sf_linear_fwd_bf16: in, w and out must be 16-byte aligned");
    lb_launch<false>(STREAM(stream), in, w, bias, nullptr, out, act, n, K, N);
    return sf_launch_status("sf_linear_fwd_bf16");
}

extern "C" int sf_linear_dgrad_bf16(const float *dout, const float *w, const float *in_act, float *din, int64_t n, int K,
                                    int N, int act, void *stream) {
    int rc = lb_check(2, n, K, N, act, "sf_linear_dgrad_bf16");
    if (rc) return rc;
    SF_REQUIRE(dout && w && din, "sf_linear_dgrad_bf16: NULL operand");
    SF_REQUIRE(aligned16(dout) && aligned16(w) && aligned16(din), "sf_linear_dgrad_bf16: dout, w and din must be 16-byte aligned");
    lb_launch<true>(STREAM(stream), dout, w, nullptr, act ? in_act : nullptr, din, act, n, N, K);  // in_act NULL: unmasked
    return sf_launch_status("sf_linear_dgrad_bf16");
}

extern "C" int64_t sf_linear_wgrad_bf16_workspace(int64_t n, int K, int N) {
    if (!lb_served(1, n, K, N)) return 0;
    return lb_parts(n, K, N).parts * ((int64_t)K * N + N) * (int64_t)sizeof(float);
}

extern "C" int sf_linear_wgrad_bf16(const float *in, const float *dout, float *dw, float *db, int64_t n, int K, int N,
                                    void *workspace, int64_t workspace_bytes, void *stream) {
    int rc = lb_check(1, n, K, N, 0, "sf_linear_wgrad_bf16");
    if (rc) return rc;
    SF_REQUIRE(in && dout && dw && db, "sf_linear_wgrad_bf16: NULL operand");
    const LbParts p = lb_parts(n, K, N);
    const int64_t need = p.parts * ((int64_t)K * N + N) * (int64_t)sizeof(float);
    SF_REQUIRE(workspace && workspace_bytes >= need, "sf_linear_wgrad_bf16: workspace %lld bytes < %lld",
               (long long)workspace_bytes, (long long)need);
    SF_REQUIRE(aligned16(in) && aligned16(dout) && aligned16(workspace),
               "sf_linear_wgrad_bf16: in, dout and workspace must be 16-byte aligned");
    hipStream_t s = STREAM(stream);
    float *part = static_cast<float *>(workspace);
    hipLaunchKernelGGL(k_linear_wgrad_bf16, dim3((unsigned)p.tiles, (unsigned)p.parts), dim3(256), 0, s, in, dout, part, n, K, N,
                       (int)ceil_div<int64_t>(N, LB_T), p.cpp, p.NT);
    rc = sf_launch_status("sf_linear_wgrad_bf16 (partials)");
    if (rc) return rc;
    return sf_res_wgrad_sum_launch(part, (int)p.parts, K * N, N, dw, db, s);
}
