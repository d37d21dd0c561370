// sf_ingest.hip — observation ingest helpers that run on the device (gfx950): the frame stack of image observations, the
// HWC -> CHW transpose of channel-last frames, and the resize / grey-scale of raw u8 frames.
//
// A host env that delivers ONE new frame per step (--device_framestack=k) has its k-frame observation assembled in the
// trajectory slab: obs[:, t + 1] = the k - 1 newest frames of obs[:, t] followed by the new frame, or k copies of the new
// frame where an episode ended (gym.wrappers.FrameStack over an auto-resetting env).  An env whose frames are [H][W][C]
// (--hwc_observations) has them transposed to C planes on the way: alone (sf_hwc_to_chw) or inside the frame-stack launch
// (sf_framestack_step_hwc).  An env that delivers native frames (--device_resize / --device_grayscale) has them resized,
// grey-scaled and de-interleaved in one launch (sf_frame_resize) into the column or its last slot.  Contract: include/sf_hip.h.
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

// ---- resize and grey-scale of u8 frames ------------------------------------------------------------------------------
// The arithmetic (include/sf_hip.h) is integer only.  On one axis, in units of 1 / (W OW) of it, destination pixel x covers
// [x W, (x + 1) W) and source pixel s covers [s OW, (s + 1) OW): x reads the columns s0 = x W / OW .. s1 = ((x + 1) W - 1) / OW
// with the weights  first = min((s0 + 1) OW, (x + 1) W) - x W,  last = (x + 1) W - s1 OW (s1 > s0),  OW in between.
constexpr int RS_BLOCK = 256;
constexpr int RS_LDS_BYTES = 32 * 1024;  // the staged band of one work-group: several of them fit a CU's 160 KB
constexpr int RS_BAND_ROWS = 32;         // source rows per band at most (an odd line stride keeps 32 of them on 32 banks)
constexpr int RS_TILE_ITEMS = RS_BLOCK;  // lane items (4 output pixels of one plane) a strip aims at
constexpr int64_t RS_MAX_AREA = (int64_t)1 << 23;  // area: 255 H W stays below 2^31, the sums are 32-bit

struct ResizeG {
    int H, W, C, OH, OW, hwc, gray;
    int lines;       // staged lines per source row: 1 (HWC: a whole row; CHW: the row of the work-group's channel), 3 (CHW, grey)
    int line_bytes;  // W C (HWC) or W
    int ls;          // bytes between staged lines: a multiple of 4 with an ODD dword count, >= line_bytes + 3
    int cap;         // source rows a band holds
    int R, strips;   // output rows per strip, strips per plane
    int load4, store4;
    int unit;        // 16 / 4: every line is whole 16-byte / 4-byte units at aligned addresses (staged as such); 0: dword by dword
    FastDiv dOW, dOH, dD, dLd, dUnit;  // p / OW and x W / OW; y H / OH; the final / D; staged dword / unit -> line
};

struct Span {  // the source pixels one output pixel reads along one axis
    int s0, s1, wf, wl;
};
// The area kernel multiplies with the full-rate 24-bit multiplier (m24; v_mul_lo_u32 runs at a quarter of its rate): on
// the LDS path a line fits the band, so W, OW and every column index stay below 2^15, H, OH and every row index are at most
// 2^23 (RS_MAX_AREA), a row sum is at most 255 W < 2^23, and every product is below 2^31.
__device__ __forceinline__ uint32_t m24(uint32_t a, uint32_t b) { return __umul24(a, b); }
__device__ __forceinline__ Span span_of(int x, int n_src, int n_dst, const FastDiv &d) {
    Span a;
    const int beg = (int)m24(x, n_src), end = beg + n_src;
    a.s0 = (int)fdiv((uint32_t)beg, d);
    a.s1 = (int)fdiv((uint32_t)(end - 1), d);
    const int next = (int)m24(a.s0 + 1, n_dst);
    a.wf = (next < end ? next : end) - beg;
    a.wl = end - (int)m24(a.s1, n_dst);
    return a;
}
__device__ __forceinline__ uint32_t gray_of(uint32_t r, uint32_t g, uint32_t b) {
    return (9798u * r + 19235u * g + 3735u * b + 16384u) >> 15;
}

// one staged row's weighted sums for one output pixel: rs[c] = sum over the pixel's columns of wx * in — the first and the
// last column carry their edge weights, the columns between them are added up plainly and weighted once (n_dst each)
template <int NC>
__device__ __forceinline__ void row_sums(const uint8_t *const (&ln)[NC], int cs, const Span &a, uint32_t w_mid, uint32_t (&rs)[NC]) {
    int o = (int)m24(a.s0, cs);
#pragma unroll
    for (int c = 0; c < NC; ++c) rs[c] = m24(a.wf, ln[c][o]);
    if (a.s1 > a.s0) {
        uint32_t mid[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) mid[c] = 0;
        for (int s = a.s0 + 1; s < a.s1; ++s) {
            o += cs;
#pragma unroll
            for (int c = 0; c < NC; ++c) mid[c] += ln[c][o];
        }
        o = (int)m24(a.s1, cs);
#pragma unroll
        for (int c = 0; c < NC; ++c) rs[c] += m24(w_mid, mid[c]) + m24(a.wl, ln[c][o]);
    }
}

// global -> LDS for lines whose bytes are whole units of V (uint4 / uint32_t) at aligned addresses: `total` units, n units
// per line, two per lane in flight before the first LDS store
template <typename V, int HWC>
__device__ __forceinline__ void stage_units(uint32_t *band, const char *frow, const ResizeG &g, int lo, int cg, int total,
                                            const FastDiv &dn, int tid) {
    constexpr int U = (int)sizeof(V), DW = U / 4;
    const int n = (int)dn.d, nd = g.ls >> 2;
    auto where = [&](int i, int &li, int &d) -> const char * {
        li = (int)fdiv((uint32_t)i, dn);
        d = i - li * n;
        const int r = lo + (g.lines == 3 ? li / 3 : li), l = g.lines == 3 ? li - (li / 3) * 3 : cg;
        const uint32_t start = HWC ? (uint32_t)r * g.line_bytes : ((uint32_t)l * g.H + r) * g.W;
        return frow + start + (uint32_t)d * U;
    };
    for (int i = tid; i < total; i += 2 * RS_BLOCK) {
        int li0, d0, li1, d1;
        const int i2 = i + RS_BLOCK < total ? i + RS_BLOCK : i;
        const V a = *reinterpret_cast<const V *>(where(i, li0, d0));
        const V b = *reinterpret_cast<const V *>(where(i2, li1, d1));
        const uint32_t *aw = reinterpret_cast<const uint32_t *>(&a), *bw = reinterpret_cast<const uint32_t *>(&b);
#pragma unroll
        for (int k = 0; k < DW; ++k) band[li0 * nd + d0 * DW + k] = aw[k];
        if (i2 != i) {
#pragma unroll
            for (int k = 0; k < DW; ++k) band[li1 * nd + d1 * DW + k] = bw[k];
        }
    }
}

// The area filter.  blockIdx.x = (channel group, strip of g.R output rows), blockIdx.y = frame (grid-strided).  The
// work-group stages the source rows its strip covers in LDS, every byte loaded from global memory once, contiguous across a
// wave: 16 bytes per lane where base, pitch and line length are multiples of 16 (g.unit), dwords where they are multiples
// of 4; otherwise line by line as the dwords they occupy in global memory (a line keeps its address modulo 4), a dword
// shared with the neighbouring line or with bytes outside the frame gathered bytewise, as is everything when !load4.
// Every lane then owns 4 consecutive pixels of one output plane (GRAY: their three channels): spans and edge weights are
// derived once per pixel, the loops over the staged pixels only multiply and add.  SAME_ROW (OW % 4 == 0: the 4 pixels
// share their output row): one walk over the staged rows serves all four.  A strip covering more rows than a band holds
// (R = 1) walks them band after band with the sums in registers; should it also have more items than lanes, each pass of
// 256 items stages the bands again (frames wider than 1024 output pixels shrunk more than 32-fold: merely correct).
template <int GRAY, int HWC, int SAME_ROW>
__global__ __launch_bounds__(RS_BLOCK) void k_resize_area(char *dst, int64_t dst_pitch, const char *__restrict__ src,
                                                          int64_t src_pitch, ResizeG g, int rows) {
    extern __shared__ uint32_t rs_band[];
    const uint8_t *band8 = reinterpret_cast<const uint8_t *>(rs_band);
    constexpr int NC = GRAY ? 3 : 1;
    const int tid = threadIdx.x;
    const int cg = blockIdx.x / g.strips, strip = blockIdx.x - cg * g.strips;  // cg: the channel of a CHW colour launch
    const int y0 = strip * g.R, y1 = y0 + g.R < g.OH ? y0 + g.R : g.OH;
    const int sy0 = (int)fdiv((uint32_t)(y0 * g.H), g.dOH), sy1 = (int)fdiv((uint32_t)(y1 * g.H - 1), g.dOH) + 1;
    const int groups = ((y1 - y0) * g.OW + 3) >> 2;
    const int planes = HWC && !GRAY ? g.C : 1;  // output planes this work-group writes from one staged band
    const int items = groups * planes, p_end = y1 * g.OW;
    const bool one_band = sy1 - sy0 <= g.cap;
    const int nd = g.ls >> 2;
    const int cs = HWC ? g.C : 1;                // bytes between neighbouring pixels of one channel in a staged line
    const int64_t plane_bytes = (int64_t)g.OH * g.OW;
    for (int b = blockIdx.y; b < rows; b += gridDim.y) {
        const char *frow = src + (int64_t)b * src_pitch;
        char *drow = dst + (int64_t)b * dst_pitch;
        for (int pass = 0; pass < items; pass += RS_BLOCK) {
            const int item = pass + tid;
            const bool live = item < items;
            const int pl = live ? item / groups : 0, gi = item - pl * groups;  // (one division per lane and pass)
            const int ch = GRAY ? 0 : HWC ? pl : cg;                         // the channel a colour lane resizes
            const int p0 = y0 * g.OW + 4 * gi;
            Span sx[4], sy[SAME_ROW ? 1 : 4];
            uint32_t acc[4][NC];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int p = live && p0 + j < p_end ? p0 + j : y0 * g.OW;  // (a dead pixel computes a live one's value)
                const int yy = (int)fdiv((uint32_t)p, g.dOW), xx = p - yy * g.OW;
                if (!SAME_ROW || j == 0) sy[SAME_ROW ? 0 : j] = span_of(yy, g.H, g.OH, g.dOH);
                sx[j] = span_of(xx, g.W, g.OW, g.dOW);
#pragma unroll
                for (int c = 0; c < NC; ++c) acc[j][c] = 0;
            }
            for (int lo = sy0; lo < sy1; lo += g.cap) {
                const int hi = lo + g.cap < sy1 ? lo + g.cap : sy1;
                if (!(one_band && pass > 0)) {
                    __syncthreads();  // the band's readers are done
                    const int nlines = (hi - lo) * g.lines;
                    if (g.unit == 16) {
                        stage_units<uint4, HWC>(rs_band, frow, g, lo, cg, nlines * (int)g.dUnit.d, g.dUnit, tid);
                    } else if (g.unit == 4) {
                        stage_units<uint32_t, HWC>(rs_band, frow, g, lo, cg, nlines * (int)g.dUnit.d, g.dUnit, tid);
                    } else {
                        for (int i = tid; i < nlines * nd; i += RS_BLOCK) {
                            const int li = (int)fdiv((uint32_t)i, g.dLd), d = i - li * nd;
                            const int r = lo + (g.lines == 3 ? li / 3 : li), l = g.lines == 3 ? li - (li / 3) * 3 : cg;
                            const uint32_t start = HWC ? (uint32_t)r * g.line_bytes : ((uint32_t)l * g.H + r) * g.W;
                            const int o = 4 * d - (int)(start & 3);  // the line bytes o .. o + 3 live in this dword
                            const char *gp = frow + start + o;
                            uint32_t v = 0;
                            if (g.load4 && o >= 0 && o + 4 <= g.line_bytes) {
                                v = *reinterpret_cast<const uint32_t *>(gp);
                            } else {
#pragma unroll
                                for (int q = 0; q < 4; ++q)
                                    if (o + q >= 0 && o + q < g.line_bytes) v |= (uint32_t)(uint8_t)gp[q] << (8 * q);
                            }
                            rs_band[i] = v;
                        }
                    }
                    __syncthreads();
                }
                // where pixel 0 of source row r sits in the band, per channel of the lane (a line keeps its phase)
                auto lines_of = [&](int r, const uint8_t *(&ln)[NC]) {
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        const int l = g.lines == 3 ? c : 0;
                        const uint32_t start = HWC ? m24(r, g.line_bytes) : ((uint32_t)(g.lines == 3 ? c : cg) * g.H + r) * g.W;
                        ln[c] = band8 + m24((r - lo) * g.lines + l, g.ls) + (start & 3) + (HWC ? (GRAY ? c : ch) : 0);
                    }
                };
                if constexpr (SAME_ROW) {
                    const int r0 = sy[0].s0 > lo ? sy[0].s0 : lo, r1 = sy[0].s1 < hi - 1 ? sy[0].s1 : hi - 1;
                    for (int r = r0; r <= r1; ++r) {
                        const uint32_t wy = r == sy[0].s0 ? sy[0].wf : r == sy[0].s1 ? sy[0].wl : g.OH;
                        const uint8_t *ln[NC];
                        lines_of(r, ln);
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            uint32_t rs[NC];
                            row_sums<NC>(ln, cs, sx[j], (uint32_t)g.OW, rs);
#pragma unroll
                            for (int c = 0; c < NC; ++c) acc[j][c] += m24(wy, rs[c]);
                        }
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int r0 = sy[j].s0 > lo ? sy[j].s0 : lo, r1 = sy[j].s1 < hi - 1 ? sy[j].s1 : hi - 1;
                        for (int r = r0; r <= r1; ++r) {
                            const uint32_t wy = r == sy[j].s0 ? sy[j].wf : r == sy[j].s1 ? sy[j].wl : g.OH;
                            const uint8_t *ln[NC];
                            lines_of(r, ln);
                            uint32_t rs[NC];
                            row_sums<NC>(ln, cs, sx[j], (uint32_t)g.OW, rs);
#pragma unroll
                            for (int c = 0; c < NC; ++c) acc[j][c] += m24(wy, rs[c]);
                        }
                    }
                }
            }
            if (!live) continue;
            uint32_t out = 0;
            uint8_t px[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint32_t v[NC];
#pragma unroll
                for (int c = 0; c < NC; ++c) v[c] = fdiv(acc[j][c] + (g.dD.d >> 1), g.dD);  // (2 S + D) / (2 D): sf_selftest_host
                if constexpr (GRAY) px[j] = (uint8_t)gray_of(v[0], v[1], v[2]);
                else px[j] = (uint8_t)v[0];
                out |= (uint32_t)px[j] << (8 * j);
            }
            char *d = drow + (int64_t)(GRAY ? 0 : ch) * plane_bytes + p0;
            if (g.store4) {
                *reinterpret_cast<uint32_t *>(d) = out;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (p0 + j < p_end) d[j] = (char)px[j];
            }
        }
    }
}

// Nearest: out[y][x] = in[y H / OH][x W / OW], up or down.  Nothing is shared between output pixels that is worth
// staging: a lane gathers the bytes of its 4 pixels of one output plane straight from global memory (only the bytes the
// output keeps are read; an up-scale re-reads them from the cache) and stores a dword, or bytes where !store4.
template <int GRAY>
__global__ __launch_bounds__(RS_BLOCK) void k_resize_nearest(char *dst, int64_t dst_pitch, const char *__restrict__ src,
                                                             int64_t src_pitch, ResizeG g, int rows) {
    const int P = g.OH * g.OW, groups = (P + 3) >> 2, planes = GRAY ? 1 : g.C;
    const int cs = g.hwc ? 1 : g.H * g.W;  // bytes between the channels of one pixel
    for (int b = blockIdx.y; b < rows; b += gridDim.y) {
        const uint8_t *frow = reinterpret_cast<const uint8_t *>(src) + (int64_t)b * src_pitch;
        char *drow = dst + (int64_t)b * dst_pitch;
        for (int gi = blockIdx.x * RS_BLOCK + threadIdx.x; gi < groups; gi += gridDim.x * RS_BLOCK) {
            uint32_t at[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int p = 4 * gi + j < P ? 4 * gi + j : P - 1;
                const int yy = (int)fdiv((uint32_t)p, g.dOW), xx = p - yy * g.OW;
                const uint32_t s = fdiv((uint32_t)(yy * g.H), g.dOH) * g.W + fdiv((uint32_t)(xx * g.W), g.dOW);
                at[j] = g.hwc ? s * g.C : s;
            }
            for (int c = 0; c < planes; ++c) {
                uint32_t out = 0;
                uint8_t px[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint8_t *q = frow + at[j];
                    if constexpr (GRAY) px[j] = (uint8_t)gray_of(q[0], q[cs], q[2 * (int64_t)cs]);
                    else px[j] = q[(int64_t)c * cs];
                    out |= (uint32_t)px[j] << (8 * j);
                }
                char *d = drow + (int64_t)c * P + 4 * gi;
                if (g.store4) {
                    *reinterpret_cast<uint32_t *>(d) = out;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (4 * gi + j < P) d[j] = (char)px[j];
                }
            }
        }
    }
}

// Any geometry, 64-bit indices, one output pixel per lane, bytes from and to global memory: frames whose rows do not fit
// the LDS band or whose index products leave 31 bits.  Merely correct.
__global__ __launch_bounds__(RS_BLOCK) void k_resize_wide(char *dst, int64_t dst_pitch, const char *__restrict__ src,
                                                          int64_t src_pitch, int64_t H, int64_t W, int C, int hwc, int64_t OH,
                                                          int64_t OW, int interp, int gray, int rows) {
    const int64_t P = OH * OW, ps = hwc ? C : 1, cs = hwc ? 1 : H * W, D = H * W;
    const int planes = gray ? 1 : C, nc = gray ? 3 : 1;
    for (int b = blockIdx.y; b < rows; b += gridDim.y) {
        const uint8_t *frow = reinterpret_cast<const uint8_t *>(src) + (int64_t)b * src_pitch;
        char *drow = dst + (int64_t)b * dst_pitch;
        for (int64_t i = (int64_t)blockIdx.x * RS_BLOCK + threadIdx.x; i < P * planes; i += (int64_t)gridDim.x * RS_BLOCK) {
            const int64_t pl = i / P, p = i - pl * P, yy = p / OW, xx = p - yy * OW;
            const int64_t ya = yy * H / OH, xa = xx * W / OW;
            const int64_t yb = interp ? ((yy + 1) * H - 1) / OH : ya, xb = interp ? ((xx + 1) * W - 1) / OW : xa;
            uint32_t v[3] = {0, 0, 0};
            for (int c = 0; c < nc; ++c) {
                const uint8_t *q = frow + (gray ? c : pl) * cs;
                if (!interp) {
                    v[c] = q[(ya * W + xa) * ps];
                    continue;
                }
                uint64_t S = 0;
                for (int64_t r = ya; r <= yb; ++r) {
                    const int64_t t0 = r * OH > yy * H ? r * OH : yy * H, t1 = (r + 1) * OH < (yy + 1) * H ? (r + 1) * OH : (yy + 1) * H;
                    uint64_t rs = 0;
                    for (int64_t s = xa; s <= xb; ++s) {
                        const int64_t u0 = s * OW > xx * W ? s * OW : xx * W, u1 = (s + 1) * OW < (xx + 1) * W ? (s + 1) * OW : (xx + 1) * W;
                        rs += (uint64_t)(u1 - u0) * q[(r * W + s) * ps];
                    }
                    S += (uint64_t)(t1 - t0) * rs;
                }
                v[c] = (uint32_t)((2 * S + (uint64_t)D) / (2 * (uint64_t)D));
            }
            drow[i] = (char)(gray ? gray_of(v[0], v[1], v[2]) : v[0]);
        }
    }
}

int gcd_int(int a, int b) { return b ? gcd_int(b, a % b) : a; }

}  // namespace

extern "C" int sf_frame_resize(void *dst, int64_t dst_pitch, const void *src, int64_t src_pitch, int H, int W, int C,
                               int src_hwc, int OH, int OW, int interp, int gray, int rows, void *stream) {
    SF_REQUIRE(dst && src, "sf_frame_resize: null dst / src");
    SF_REQUIRE(H >= 1 && W >= 1 && C >= 1 && OH >= 1 && OW >= 1, "sf_frame_resize: H=%d W=%d C=%d OH=%d OW=%d (each at least 1)",
               H, W, C, OH, OW);
    SF_REQUIRE(interp == 0 || interp == 1, "sf_frame_resize: interp=%d (0 = nearest or 1 = area)", interp);
    SF_REQUIRE(!interp || (OH <= H && OW <= W), "sf_frame_resize: the area filter only shrinks, %d x %d -> %d x %d", H, W, OH, OW);
    SF_REQUIRE(!interp || (int64_t)H * W <= RS_MAX_AREA, "sf_frame_resize: area filter on %d x %d pixels, more than 2^23", H, W);
    SF_REQUIRE(!gray || C == 3, "sf_frame_resize: gray needs C == 3 (R, G, B), got C=%d", C);
    SF_REQUIRE((int64_t)H * W <= ((int64_t)1 << 40) / C && (int64_t)OH * OW <= ((int64_t)1 << 40) / C,
               "sf_frame_resize: frame of %d x %d x %d -> %d x %d too large", H, W, C, OH, OW);
    SF_REQUIRE(rows >= 0, "sf_frame_resize: rows=%d", rows);
    const int64_t src_bytes = (int64_t)H * W * C, out_plane = (int64_t)OH * OW, dst_bytes = out_plane * (gray ? 1 : C);
    SF_REQUIRE(src_pitch >= src_bytes, "sf_frame_resize: src_pitch=%lld < H W C = %lld", (long long)src_pitch, (long long)src_bytes);
    SF_REQUIRE(dst_pitch >= dst_bytes, "sf_frame_resize: dst_pitch=%lld < C' OH OW = %lld", (long long)dst_pitch,
               (long long)dst_bytes);
    if (rows == 0) return SF_OK;
    char *d = reinterpret_cast<char *>(dst);
    const char *s = reinterpret_cast<const char *>(src);
    const unsigned gy = (unsigned)(rows < 65535 ? rows : 65535);
    const int64_t lim = (int64_t)1 << 31;
    ResizeG g{};
    g.H = H; g.W = W; g.C = C; g.OH = OH; g.OW = OW; g.hwc = src_hwc != 0; g.gray = gray != 0;
    g.lines = !g.hwc && g.gray ? 3 : 1;
    const int64_t line_bytes = g.hwc ? (int64_t)W * C : W;
    int64_t ls = (line_bytes + 3 + 3) / 4 * 4;
    if ((ls / 4) % 2 == 0) ls += 4;
    // 32-bit index products on the fast paths: y H and x W (fdiv wants them below 2^31), pixel and byte offsets of a frame
    const bool narrow = (int64_t)OH * H < lim && (int64_t)OW * W < lim && out_plane + 4 < lim && src_bytes < lim;
    const bool fits = ls * g.lines <= RS_LDS_BYTES;
    if (!narrow || (interp && !fits)) {
        const int64_t bx = (dst_bytes + RS_BLOCK - 1) / RS_BLOCK;
        k_resize_wide<<<dim3((unsigned)(bx < 4096 ? bx : 4096), gy), dim3(RS_BLOCK), 0, STREAM(stream)>>>(
            d, dst_pitch, s, src_pitch, H, W, C, g.hwc, OH, OW, interp, g.gray, rows);
        return sf_launch_status("sf_frame_resize");
    }
    g.line_bytes = (int)line_bytes;
    g.ls = (int)ls;
    g.load4 = (((uintptr_t)src | (uintptr_t)src_pitch) & 3) == 0;
    const bool dst4 = (((uintptr_t)dst | (uintptr_t)dst_pitch | (uintptr_t)out_plane) & 3) == 0;
    g.dOW = make_fastdiv((uint32_t)OW);
    g.dOH = make_fastdiv((uint32_t)OH);
    g.dD = make_fastdiv((uint32_t)((int64_t)H * W));
    g.dLd = make_fastdiv((uint32_t)(ls / 4));
    // every line starts at a multiple of its length (HWC) or of W (planar): whole aligned units when the base, the pitch
    // and that length are multiples of the unit
    const uintptr_t src_all = (uintptr_t)src | (uintptr_t)src_pitch | (uintptr_t)line_bytes;
    g.unit = (src_all & 15) == 0 ? 16 : (src_all & 3) == 0 ? 4 : 0;
    g.dUnit = make_fastdiv((uint32_t)(g.unit ? line_bytes / g.unit : 1));
    if (!interp) {
        g.store4 = dst4;
        const int64_t bx = ((out_plane + 3) / 4 + RS_BLOCK - 1) / RS_BLOCK;
        const dim3 grid((unsigned)(bx < 1024 ? bx : 1024), gy), block(RS_BLOCK);
        if (g.gray) k_resize_nearest<1><<<grid, block, 0, STREAM(stream)>>>(d, dst_pitch, s, src_pitch, g, rows);
        else k_resize_nearest<0><<<grid, block, 0, STREAM(stream)>>>(d, dst_pitch, s, src_pitch, g, rows);
        return sf_launch_status("sf_frame_resize");
    }
    // the band: as many source rows as 32 KB hold, RS_BAND_ROWS at most; the strip: as many output rows as are sure to
    // cover no more than a band (ceil(R H / OH) + 1 rows), about RS_TILE_ITEMS lane items, and — for dword stores — a
    // whole number of dwords, so that every strip starts on one
    const int64_t by_lds = RS_LDS_BYTES / (ls * g.lines);
    g.cap = (int)(by_lds < RS_BAND_ROWS ? by_lds : RS_BAND_ROWS);
    const int r_fit = (int)((int64_t)(g.cap - 1) * OH / H) > 1 ? (int)((int64_t)(g.cap - 1) * OH / H) : 1;
    const int64_t per_row = (int64_t)(OW + 3) / 4 * (g.hwc && !g.gray ? C : 1);
    const int r_tgt = (int)((RS_TILE_ITEMS + per_row - 1) / per_row);
    int R = r_fit < r_tgt ? r_fit : r_tgt;
    if (R > OH) R = OH;
    g.store4 = dst4;
    if (dst4 && R < OH) {
        const int m = 4 / gcd_int(OW, 4);  // rows per whole number of dwords
        if (R >= m) R -= R % m;
        else if (m <= r_fit && m < OH) R = m;
        else g.store4 = 0;
    }
    g.R = R;
    g.strips = (OH + R - 1) / R;
    int64_t band = ((int64_t)R * H + OH - 1) / OH + 1;  // rows one strip covers at most
    if (band > H) band = H;
    if (band > g.cap) band = g.cap;
    const size_t lds = (size_t)(band * g.lines * ls);
    const int64_t tiles = (int64_t)g.strips * (!g.hwc && !g.gray ? C : 1);
    SF_REQUIRE(tiles < lim, "sf_frame_resize: %lld work-groups per frame", (long long)tiles);
    const dim3 grid((unsigned)tiles, gy), block(RS_BLOCK);
#define SF_RS_LAUNCH(GRAY, HWC, SAME)                                                                                      \
    k_resize_area<GRAY, HWC, SAME><<<grid, block, lds, STREAM(stream)>>>(d, dst_pitch, s, src_pitch, g, rows)
#define SF_RS_LAUNCH_SAME(GRAY, HWC)                                                                                       \
    if (OW % 4 == 0) SF_RS_LAUNCH(GRAY, HWC, 1);                                                                           \
    else SF_RS_LAUNCH(GRAY, HWC, 0)
    if (g.gray && g.hwc) { SF_RS_LAUNCH_SAME(1, 1); }
    else if (g.gray) { SF_RS_LAUNCH_SAME(1, 0); }
    else if (g.hwc) { SF_RS_LAUNCH_SAME(0, 1); }
    else { SF_RS_LAUNCH_SAME(0, 0); }
#undef SF_RS_LAUNCH_SAME
#undef SF_RS_LAUNCH
    return sf_launch_status("sf_frame_resize");
}

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
