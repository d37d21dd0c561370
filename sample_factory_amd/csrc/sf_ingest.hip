// sf_ingest.hip — observation ingest helpers that run on the device (gfx950): the frame stack of image observations and
// the HWC -> CHW transpose of channel-last frames.
//
// A host env that delivers ONE new frame per step (--device_framestack=k) has its k-frame observation assembled in the
// trajectory slab: obs[:, t + 1] = the k - 1 newest frames of obs[:, t] followed by the new frame, or k copies of the new
// frame where an episode ended (gym.wrappers.FrameStack over an auto-resetting env).  An env whose frames are [H][W][C]
// (--hwc_observations) has them transposed to C planes on the way: alone (sf_hwc_to_chw) or inside the frame-stack launch
// (sf_framestack_step_hwc).  Contract: include/sf_hip.h.
#include "sf_common.h"

#define STREAM(s) reinterpret_cast<hipStream_t>(s)

namespace {

constexpr int FS_BLOCK = 256;
constexpr int FS_MAX_K = 16;

// One row of `next` per blockIdx.y (grid-strided), the row's units spread over blockIdx.x: the done flag is uniform per
// work-group, so neither branch diverges.  V is the access unit (uint4 / uint32_t / uint8_t); `fu` = units per frame.
//   running row:  next[0 .. (k-1) fu) = prev[fu .. k fu)  — ONE shifted contiguous copy — and, with a separate `frame`
//                 buffer, next[(k-1) fu .. k fu) = frame; with frame == NULL the last slot already holds the new frame
//                 (the DMA put it there) and is neither read nor written;
//   done / reset: every slot = the new frame: each unit of it is loaded once and stored to `nslots` slots.
// Two units per lane are in flight before the first store (loads first, stores after).  next is not __restrict__: with
// frame == NULL a done row reads its own last slot while it writes the others (disjoint bytes).
template <typename V>
__global__ __launch_bounds__(FS_BLOCK) void k_framestack_step(char *next, int64_t next_pitch, const char *__restrict__ prev,
                                                              int64_t prev_pitch, const char *frame, int64_t frame_pitch,
                                                              int64_t fu, int k, const uint8_t *__restrict__ terminated,
                                                              const uint8_t *__restrict__ truncated, int reset, int rows) {
    constexpr int64_t U = (int64_t)sizeof(V);
    const int nslots = frame ? k : k - 1;  // slots of `next` this launch writes
    const int64_t step = (int64_t)gridDim.x * FS_BLOCK;
    const int64_t u0 = (int64_t)blockIdx.x * FS_BLOCK + threadIdx.x;
    for (int b = blockIdx.y; b < rows; b += gridDim.y) {
        char *nrow = next + (int64_t)b * next_pitch;
        const char *frow = frame ? frame + (int64_t)b * frame_pitch : nrow + (int64_t)(k - 1) * fu * U;
        const bool done = reset || (terminated && terminated[b]) || (truncated && truncated[b]);
        if (done) {
            for (int64_t u = u0; u < fu; u += 2 * step) {
                const int64_t u2 = u + step;
                const V a = *reinterpret_cast<const V *>(frow + u * U);
                V c = a;
                if (u2 < fu) c = *reinterpret_cast<const V *>(frow + u2 * U);
                for (int j = 0; j < nslots; ++j) {
                    *reinterpret_cast<V *>(nrow + ((int64_t)j * fu + u) * U) = a;
                    if (u2 < fu) *reinterpret_cast<V *>(nrow + ((int64_t)j * fu + u2) * U) = c;
                }
            }
        } else {
            const char *prow = prev + (int64_t)b * prev_pitch + fu * U;  // prev's slot 1
            const int64_t shifted = (int64_t)(k - 1) * fu, total = (int64_t)nslots * fu;
            for (int64_t u = u0; u < total; u += 2 * step) {
                const int64_t u2 = u + step;
                const char *s1 = u < shifted ? prow + u * U : frow + (u - shifted) * U;
                const V a = *reinterpret_cast<const V *>(s1);
                V c = a;
                if (u2 < total) c = *reinterpret_cast<const V *>(u2 < shifted ? prow + u2 * U : frow + (u2 - shifted) * U);
                *reinterpret_cast<V *>(nrow + u * U) = a;
                if (u2 < total) *reinterpret_cast<V *>(nrow + u2 * U) = c;
            }
        }
    }
}

// do rows of `row_bytes` bytes at a + i * pa (i < rows) and b + j * pb (j < rows) share a byte?  (pitches >= row_bytes)
bool rows_overlap(uintptr_t a, int64_t pa, uintptr_t b, int64_t pb, int64_t row_bytes, int64_t rows) {
    const uintptr_t a_end = a + (uintptr_t)(rows - 1) * (uintptr_t)pa + (uintptr_t)row_bytes;
    const uintptr_t b_end = b + (uintptr_t)(rows - 1) * (uintptr_t)pb + (uintptr_t)row_bytes;
    if (a_end <= b || b_end <= a) return false;  // the whole ranges are apart: two slabs
    if (pa == pb) {  // columns of one slab: the rows interleave, all at the same offset modulo the pitch
        const uintptr_t d = a >= b ? (a - b) % (uintptr_t)pa : (uintptr_t)pa - 1 - ((b - a - 1) % (uintptr_t)pa);
        return d < (uintptr_t)row_bytes || d > (uintptr_t)pa - (uintptr_t)row_bytes;
    }
    for (int64_t i = 0; i < rows; ++i) {  // different pitches inside one range (nobody's layout): row by row
        const uintptr_t r = a + (uintptr_t)i * (uintptr_t)pa;
        if (r + (uintptr_t)row_bytes <= b || r >= b_end) continue;
        int64_t j = r >= b ? (int64_t)((r - b) / (uintptr_t)pb) : 0;
        for (int64_t jj = j; jj <= j + 1 && jj < rows; ++jj) {
            const uintptr_t q = b + (uintptr_t)jj * (uintptr_t)pb;
            if (r < q + (uintptr_t)row_bytes && q < r + (uintptr_t)row_bytes) return true;
        }
    }
    return false;
}

// ---- HWC frames ----------------------------------------------------------------------------------------------------
// A frame row is [P = H W][C] elements; a slot of `next` is C planes of P.  dst[c][p] = src[p][c], bit for bit.
constexpr int HWC_MAX_CT = 4;  // channel counts with a register path of their own (gray, gray + alpha, RGB, RGBA)

// the shifted contiguous copy of a running row: `units` units of V, two per lane in flight before the first store
template <typename V>
__device__ __forceinline__ void copy_units(char *dst, const char *src, int64_t units, int64_t u0, int64_t step) {
    constexpr int64_t U = (int64_t)sizeof(V);
    for (int64_t u = u0; u < units; u += 2 * step) {
        const int64_t u2 = u + step;
        const V a = *reinterpret_cast<const V *>(src + u * U);
        V c = a;
        if (u2 < units) c = *reinterpret_cast<const V *>(src + u2 * U);
        *reinterpret_cast<V *>(dst + u * U) = a;
        if (u2 < units) *reinterpret_cast<V *>(dst + u2 * U) = c;
    }
}

// u8: a lane holds the 4 CT interleaved bytes of 4 consecutive pixels in w[] (byte n = pixel n / CT, channel n % CT) and
// wants one dword per channel: o[c] = bytes c, CT + c, 2 CT + c, 3 CT + c.  Two v_perm_b32 gather a byte pair each (the
// selector's 0..3 address the second operand, 4..7 the first), a third joins the pairs.
template <int CT>
__device__ __forceinline__ void deinterleave(const uint32_t (&w)[CT], uint32_t (&o)[CT]) {
#pragma unroll
    for (int c = 0; c < CT; ++c) {
        const int n0 = c, n1 = CT + c, n2 = 2 * CT + c, n3 = 3 * CT + c;
        const uint32_t lo = __builtin_amdgcn_perm(w[n1 >> 2], w[n0 >> 2], 0x0c0c0000u | ((4u + (n1 & 3)) << 8) | (n0 & 3));
        const uint32_t hi = __builtin_amdgcn_perm(w[n3 >> 2], w[n2 >> 2], 0x0c0c0000u | ((4u + (n3 & 3)) << 8) | (n2 & 3));
        o[c] = __builtin_amdgcn_perm(hi, lo, 0x05040100u);
    }
}

// The dword path (every base and pitch a multiple of 4; u8: P % 4 == 0 as well).  Rows and the done flag as in
// k_framestack_step.  A lane owns one dword of every plane: 4 pixels (EB == 1) or one pixel (EB == 4).  Either way its
// source is the C consecutive dwords at frame + 4 C g — the lanes of a wave read one contiguous span — and it stores C
// dwords, one per plane, each contiguous across the lanes.  CT = C for C <= HWC_MAX_CT: the C loads of two such dwords
// are issued, the bytes are de-interleaved in registers (u8) and the stores follow, to slot k - 1 of a running row or to
// all k slots of a done one (each source element is loaded once).  CT = 0: any C, four channels at a time; u8 then gathers its bytes
// with byte loads (the stores stay dwords).  A running row with k > 1 also gets slots 1 .. k - 1 of prev as ONE shifted
// contiguous copy, 16 bytes per access where `copy16` says the addresses allow it.  k == 1 is the plain transpose
// (prev is not read).
template <int EB, int CT>
__global__ __launch_bounds__(FS_BLOCK) void k_framestack_hwc(char *next, int64_t next_pitch, const char *__restrict__ prev,
                                                             int64_t prev_pitch, const char *frame, int64_t frame_pitch,
                                                             int64_t P, int C, int k, int copy16,
                                                             const uint8_t *__restrict__ terminated,
                                                             const uint8_t *__restrict__ truncated, int reset, int rows) {
    constexpr int PX = EB == 1 ? 4 : 1;  // pixels per lane
    const int64_t G = P / PX, plane = P * EB, fbytes = plane * C;
    const int64_t step = (int64_t)gridDim.x * FS_BLOCK;
    const int64_t u0 = (int64_t)blockIdx.x * FS_BLOCK + threadIdx.x;
    for (int b = blockIdx.y; b < rows; b += gridDim.y) {
        char *nrow = next + (int64_t)b * next_pitch;
        const char *frow = frame + (int64_t)b * frame_pitch;
        const bool done = reset || (terminated && terminated[b]) || (truncated && truncated[b]);
        const int j0 = done ? 0 : k - 1;  // first slot that takes the new frame
        if constexpr (CT > 0) {
            for (int64_t g = u0; g < G; g += 2 * step) {  // two of its dwords per plane in flight before the first store
                const int64_t g2 = g + step < G ? g + step : g;
                uint32_t w[2][CT], o[2][CT];
#pragma unroll
                for (int c = 0; c < CT; ++c) w[0][c] = *reinterpret_cast<const uint32_t *>(frow + g * 4 * CT + 4 * c);
#pragma unroll
                for (int c = 0; c < CT; ++c) w[1][c] = *reinterpret_cast<const uint32_t *>(frow + g2 * 4 * CT + 4 * c);
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    if constexpr (EB == 1 && CT > 1) {
                        deinterleave<CT>(w[i], o[i]);
                    } else {
#pragma unroll
                        for (int c = 0; c < CT; ++c) o[i][c] = w[i][c];
                    }
                }
                for (int j = j0; j < k; ++j) {
#pragma unroll
                    for (int c = 0; c < CT; ++c) {
                        char *d = nrow + ((int64_t)j * CT + c) * plane;
                        *reinterpret_cast<uint32_t *>(d + g * 4) = o[0][c];
                        if (g2 != g) *reinterpret_cast<uint32_t *>(d + g2 * 4) = o[1][c];
                    }
                }
            }
        } else {
            for (int64_t g = u0; g < G; g += step) {
                const char *s = frow + g * 4 * C;
                char *d = nrow + g * 4;
                for (int c0 = 0; c0 < C; c0 += 4) {
                    uint32_t o[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int c = c0 + i < C ? c0 + i : C - 1;
                        if constexpr (EB == 4) {
                            o[i] = *reinterpret_cast<const uint32_t *>(s + 4 * c);
                        } else {
                            const uint8_t *sb = reinterpret_cast<const uint8_t *>(s) + c;
                            o[i] = (uint32_t)sb[0] | (uint32_t)sb[C] << 8 | (uint32_t)sb[2 * C] << 16 | (uint32_t)sb[3 * C] << 24;
                        }
                    }
                    for (int j = j0; j < k; ++j) {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (c0 + i < C) *reinterpret_cast<uint32_t *>(d + ((int64_t)j * C + c0 + i) * plane) = o[i];
                    }
                }
            }
        }
        if (!done && k > 1) {
            const char *prow = prev + (int64_t)b * prev_pitch + fbytes;  // prev's slot 1
            const int64_t shifted = (int64_t)(k - 1) * fbytes;
            if (copy16)
                copy_units<uint4>(nrow, prow, shifted / 16, u0, step);
            else
                copy_units<uint32_t>(nrow, prow, shifted / 4, u0, step);
        }
    }
}

// The byte path: any alignment, any P, either element size.  A lane owns byte `o` of every plane (element o / eb, byte
// o % eb of it), loads it for four channels and stores it to their planes; merely correct.
__global__ __launch_bounds__(FS_BLOCK) void k_framestack_hwc_bytes(char *next, int64_t next_pitch,
                                                                   const char *__restrict__ prev, int64_t prev_pitch,
                                                                   const char *frame, int64_t frame_pitch, int64_t P, int C,
                                                                   int eb, int k, const uint8_t *__restrict__ terminated,
                                                                   const uint8_t *__restrict__ truncated, int reset, int rows) {
    const int64_t plane = P * eb, fbytes = plane * C;
    const int64_t step = (int64_t)gridDim.x * FS_BLOCK;
    const int64_t u0 = (int64_t)blockIdx.x * FS_BLOCK + threadIdx.x;
    for (int b = blockIdx.y; b < rows; b += gridDim.y) {
        char *nrow = next + (int64_t)b * next_pitch;
        const char *frow = frame + (int64_t)b * frame_pitch;
        const bool done = reset || (terminated && terminated[b]) || (truncated && truncated[b]);
        const int j0 = done ? 0 : k - 1;
        for (int64_t o = u0; o < plane; o += step) {
            const int64_t p = o / eb;
            const char *s = frow + p * C * eb + (o - p * eb);
            for (int c0 = 0; c0 < C; c0 += 4) {
                char v[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = s[(int64_t)(c0 + i < C ? c0 + i : C - 1) * eb];
                for (int j = j0; j < k; ++j) {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (c0 + i < C) nrow[((int64_t)j * C + c0 + i) * plane + o] = v[i];
                }
            }
        }
        if (!done && k > 1) copy_units<uint8_t>(nrow, prev + (int64_t)b * prev_pitch + fbytes, (int64_t)(k - 1) * fbytes, u0, step);
    }
}

// picks the alignment class and launches; the arguments have been checked.  k == 1: prev is not read (may be NULL).
void launch_framestack_hwc(char *next, int64_t next_pitch, const char *prev, int64_t prev_pitch, const char *frame,
                           int64_t frame_pitch, int64_t P, int C, int eb, int k, const uint8_t *terminated,
                           const uint8_t *truncated, int rows, hipStream_t stream) {
    const int64_t fbytes = P * C * eb;
    uintptr_t all = (uintptr_t)next | (uintptr_t)next_pitch | (uintptr_t)frame | (uintptr_t)frame_pitch;
    if (k > 1) all |= (uintptr_t)prev | (uintptr_t)prev_pitch;
    const bool dwords = (all & 3) == 0 && (eb == 4 || P % 4 == 0);
    const int copy16 = dwords && (((uintptr_t)next | (uintptr_t)next_pitch | (uintptr_t)prev | (uintptr_t)prev_pitch |
                                   (uintptr_t)fbytes) & 15) == 0;
    // one pass over the transposed frame (two dwords per plane and lane on the register paths), two copy units per lane
    // and pass; at most 64 work-groups along a row
    const int64_t groups = eb == 1 ? P / 4 : P;
    const int64_t items = !dwords ? P * eb : C <= HWC_MAX_CT ? (groups + 1) / 2 : groups;
    const int64_t copied = k > 1 ? (int64_t)(k - 1) * fbytes / (copy16 ? 16 : dwords ? 4 : 1) / 2 : 0;
    const int64_t work = items > copied ? items : copied, bx = (work + FS_BLOCK - 1) / FS_BLOCK;
    const dim3 grid((unsigned)(bx < 1 ? 1 : bx < 64 ? bx : 64), (unsigned)(rows < 65535 ? rows : 65535)), block(FS_BLOCK);
    const int reset = !terminated && !truncated;
#define SF_HWC_LAUNCH(EB, CT)                                                                                              \
    k_framestack_hwc<EB, CT><<<grid, block, 0, stream>>>(next, next_pitch, prev, prev_pitch, frame, frame_pitch, P, C, k,  \
                                                         copy16, terminated, truncated, reset, rows)
#define SF_HWC_LAUNCH_EB(EB)                                                                                               \
    switch (C <= HWC_MAX_CT ? C : 0) {                                                                                     \
        case 1: SF_HWC_LAUNCH(EB, 1); break;                                                                               \
        case 2: SF_HWC_LAUNCH(EB, 2); break;                                                                               \
        case 3: SF_HWC_LAUNCH(EB, 3); break;                                                                               \
        case 4: SF_HWC_LAUNCH(EB, 4); break;                                                                               \
        default: SF_HWC_LAUNCH(EB, 0); break;                                                                              \
    }
    if (!dwords) {
        k_framestack_hwc_bytes<<<grid, block, 0, stream>>>(next, next_pitch, prev, prev_pitch, frame, frame_pitch, P, C, eb,
                                                           k, terminated, truncated, reset, rows);
    } else if (eb == 1) {
        SF_HWC_LAUNCH_EB(1)
    } else {
        SF_HWC_LAUNCH_EB(4)
    }
#undef SF_HWC_LAUNCH_EB
#undef SF_HWC_LAUNCH
}

// the frame geometry both HWC entry points take; P C eb stays far below 2^63 for any k <= FS_MAX_K
#define SF_REQUIRE_HWC_FRAME(name)                                                                                         \
    SF_REQUIRE(H >= 1 && W >= 1 && C >= 1, name ": H=%d W=%d C=%d (each at least 1)", H, W, C);                            \
    SF_REQUIRE(elem_bytes == 1 || elem_bytes == 4, name ": elem_bytes=%d (1 = u8 or 4 = f32)", elem_bytes);                \
    SF_REQUIRE((int64_t)H * W <= ((int64_t)1 << 40) / ((int64_t)C * elem_bytes), name ": frame of %d x %d x %d too large", \
               H, W, C);                                                                                                   \
    SF_REQUIRE(rows >= 0, name ": rows=%d", rows)

}  // namespace

extern "C" int sf_hwc_to_chw(void *dst, int64_t dst_pitch, const void *src, int64_t src_pitch, int H, int W, int C,
                             int elem_bytes, int rows, void *stream) {
    SF_REQUIRE(dst && src, "sf_hwc_to_chw: null dst / src");
    SF_REQUIRE_HWC_FRAME("sf_hwc_to_chw");
    const int64_t P = (int64_t)H * W, row_bytes = P * C * elem_bytes;
    SF_REQUIRE(dst_pitch >= row_bytes && src_pitch >= row_bytes,
               "sf_hwc_to_chw: pitches %lld / %lld smaller than a row of H W C elem_bytes = %lld", (long long)dst_pitch,
               (long long)src_pitch, (long long)row_bytes);
    if (rows == 0) return SF_OK;
    // a frame stack of one slot after a reset: every row takes its transposed frame, nothing is shifted
    launch_framestack_hwc(reinterpret_cast<char *>(dst), dst_pitch, nullptr, 0, reinterpret_cast<const char *>(src),
                          src_pitch, P, C, elem_bytes, 1, nullptr, nullptr, rows, STREAM(stream));
    return sf_launch_status("sf_hwc_to_chw");
}

extern "C" int sf_framestack_step_hwc(void *next, int64_t next_pitch, const void *prev, int64_t prev_pitch,
                                      const void *frame, int64_t frame_pitch, int H, int W, int C, int elem_bytes, int k,
                                      const uint8_t *terminated, const uint8_t *truncated, int rows, void *stream) {
    SF_REQUIRE(next && prev && frame, "sf_framestack_step_hwc: null next / prev / frame");
    SF_REQUIRE(k >= 1 && k <= FS_MAX_K, "sf_framestack_step_hwc: k=%d outside 1..%d", k, FS_MAX_K);
    SF_REQUIRE_HWC_FRAME("sf_framestack_step_hwc");
    const int64_t P = (int64_t)H * W, frame_bytes = P * C * elem_bytes, row_bytes = (int64_t)k * frame_bytes;
    SF_REQUIRE(next_pitch >= row_bytes && prev_pitch >= row_bytes,
               "sf_framestack_step_hwc: pitches %lld / %lld smaller than k * frame_bytes = %lld", (long long)next_pitch,
               (long long)prev_pitch, (long long)row_bytes);
    SF_REQUIRE(frame_pitch >= frame_bytes, "sf_framestack_step_hwc: frame_pitch=%lld < frame_bytes=%lld",
               (long long)frame_pitch, (long long)frame_bytes);
    if (rows == 0) return SF_OK;
    SF_REQUIRE(!rows_overlap((uintptr_t)next, next_pitch, (uintptr_t)prev, prev_pitch, row_bytes, rows),
               "sf_framestack_step_hwc: rows of next and prev overlap");
    launch_framestack_hwc(reinterpret_cast<char *>(next), next_pitch, reinterpret_cast<const char *>(prev), prev_pitch,
                          reinterpret_cast<const char *>(frame), frame_pitch, P, C, elem_bytes, k, terminated, truncated,
                          rows, STREAM(stream));
    return sf_launch_status("sf_framestack_step_hwc");
}

extern "C" int sf_framestack_step(void *next, int64_t next_pitch, const void *prev, int64_t prev_pitch, const void *frame,
                                  int64_t frame_pitch, int64_t frame_bytes, int k, const uint8_t *terminated,
                                  const uint8_t *truncated, int rows, void *stream) {
    SF_REQUIRE(next && prev, "sf_framestack_step: null next / prev");
    SF_REQUIRE(k >= 1 && k <= FS_MAX_K, "sf_framestack_step: k=%d outside 1..%d", k, FS_MAX_K);
    SF_REQUIRE(frame_bytes > 0, "sf_framestack_step: frame_bytes=%lld", (long long)frame_bytes);
    SF_REQUIRE(rows >= 0, "sf_framestack_step: rows=%d", rows);
    const int64_t row_bytes = (int64_t)k * frame_bytes;
    SF_REQUIRE(next_pitch >= row_bytes && prev_pitch >= row_bytes,
               "sf_framestack_step: pitches %lld / %lld smaller than k * frame_bytes = %lld", (long long)next_pitch,
               (long long)prev_pitch, (long long)row_bytes);
    SF_REQUIRE(!frame || frame_pitch >= frame_bytes, "sf_framestack_step: frame_pitch=%lld < frame_bytes=%lld",
               (long long)frame_pitch, (long long)frame_bytes);
    if (rows == 0) return SF_OK;
    SF_REQUIRE(!rows_overlap((uintptr_t)next, next_pitch, (uintptr_t)prev, prev_pitch, row_bytes, rows),
               "sf_framestack_step: rows of next and prev overlap");
    if (k == 1 && !frame) return SF_OK;  // the frame is already where it belongs and there is nothing to shift
    uintptr_t all = (uintptr_t)next | (uintptr_t)prev | (uintptr_t)next_pitch | (uintptr_t)prev_pitch | (uintptr_t)frame_bytes;
    if (frame) all |= (uintptr_t)frame | (uintptr_t)frame_pitch;
    const int unit = (all & 15) == 0 ? 16 : (all & 3) == 0 ? 4 : 1;
    const int64_t fu = frame_bytes / unit, per_row = (int64_t)(frame ? k : k - 1) * fu;
    // two units per lane and pass; at most 64 work-groups along a row, the rest is the row loop's
    const int64_t bx = (per_row + 2 * FS_BLOCK - 1) / (2 * FS_BLOCK);
    const dim3 grid((unsigned)(bx < 64 ? bx : 64), (unsigned)(rows < 65535 ? rows : 65535)), block(FS_BLOCK);
    const int reset = !terminated && !truncated;
    char *n = reinterpret_cast<char *>(next);
    const char *p = reinterpret_cast<const char *>(prev), *f = reinterpret_cast<const char *>(frame);
    if (unit == 16)
        k_framestack_step<uint4><<<grid, block, 0, STREAM(stream)>>>(n, next_pitch, p, prev_pitch, f, frame_pitch, fu, k,
                                                                     terminated, truncated, reset, rows);
    else if (unit == 4)
        k_framestack_step<uint32_t><<<grid, block, 0, STREAM(stream)>>>(n, next_pitch, p, prev_pitch, f, frame_pitch, fu, k,
                                                                        terminated, truncated, reset, rows);
    else
        k_framestack_step<uint8_t><<<grid, block, 0, STREAM(stream)>>>(n, next_pitch, p, prev_pitch, f, frame_pitch, fu, k,
                                                                       terminated, truncated, reset, rows);
    return sf_launch_status("sf_framestack_step");
}
