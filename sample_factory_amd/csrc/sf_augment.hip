// sf_augment.hip — training-time image augmentation on the device (gfx950): the random shift of RAD / DrQ / DrAC (pad by
// `pad` pixels with edge replication, crop back at a random offset) as ONE gather launch that reads a minibatch's frames
// through the learner's row addressing and writes a dense [n][C][H][W] batch.  pad = 0 is the plain gather.  A byte mover:
// u8 and f32 frames alike, any alignment of src, dst and the pitches.  Contract: include/sf_hip.h; the NumPy model is
// sample_factory_amd/envs/frame_ops.py (random_shift_draws, random_shift_frames).
// sf_augment_gather is the same launch with two more transformations behind the shift — an intensity scale and a cutout
// rectangle (frame_ops.py: intensity_draws, cutout_draws, augment_frames) — applied to every output dword in registers
// before its 16-byte store: the kernels below are templates on their geometry struct, ShiftG (the shift alone, the code of
// sf_random_shift_gather) or AugG<cutout, intensity> (the shift and the per-sample operations that are on).
#include "sf_common.h"

#define STREAM(s) reinterpret_cast<hipStream_t>(s)

namespace {

constexpr int RSG_LDS_BYTES = 64 * 1024;  // the staged source rows of one work-group at most
constexpr int RSG_GRID = 8192;            // work-groups along the samples at most (grid-strided)
constexpr int RSG_WIDE_BLOCK = 256;

constexpr uint32_t AUG_LANE_CUTOUT = 8u;     // lane 2 of the Philox counter: the cutout rectangle of a sample
constexpr uint32_t AUG_LANE_INTENSITY = 9u;  // ... its intensity scale and its fill byte (10: the host's op draw)

struct ShiftG {
    static constexpr bool OPS = false;
    int C, H, W, sh;  // sh = log2(elem_bytes): 0 (u8) or 2 (f32)
    int Wb, S;        // bytes of a frame row and of a sample
    int pad, recurrence, traj_T;
    int U;            // 16-byte output units per strip
    uint32_t seed, draw_id;
    FastDiv dWb, dH;
};

// the operations of sf_augment_gather behind the shift: cut_max = 0 and intensity = 0 switch theirs off
struct AugOps {
    int cut_min, cut_max, cut_fill, intensity;
};
template <bool CUT, bool INT>  // which of the two are compiled in: a launch pays for the operations it applies only
struct AugG : ShiftG {
    static constexpr bool OPS = true, CUTOUT = CUT, INTENSITY = INT;
    AugOps ops;
};

// what a sample's draws come to: the cutout covers rows [cy0, cy1) and columns [cx0, cx1) of every plane (empty when
// off), filled with the four equal bytes of fillw; pixels are scaled by s / 256 (256 = off: the identity)
struct AugS {
    int cy0, cy1, cx0, cx1;
    uint32_t s, fillw;
    float scale;
};

// dataset row d = index[i] | offset + i; its slab row (sf_common.h's sample addressing) and its shift (dy, dx) in
// [0, 2 pad]: ONE Philox block per sample, counter (draw_id, 0, 5, 0), key (seed, d / recurrence).  Every value is the
// same in all lanes of the work-group.
__device__ __forceinline__ int64_t shift_of_sample(const int32_t *__restrict__ index, int64_t offset, int64_t i, int traj_T,
                                                   int recurrence, int pad, uint32_t seed, uint32_t draw_id, int &dy, int &dx) {
    const int64_t d = index ? (int64_t)index[i] : offset + i;
    dy = 0;
    dx = 0;
    if (pad > 0) {
        uint32_t w[4];
        sf_philox4x32_10(draw_id, 0u, 5u, 0u, seed, (uint32_t)(d / recurrence), w);
        const uint32_t m = 2u * (uint32_t)pad + 1u;
        dx = (int)(((uint64_t)w[0] * m) >> 32);
        dy = (int)(((uint64_t)w[1] * m) >> 32);
    }
    return traj_T > 0 ? d + d / traj_T : d;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

__device__ __forceinline__ int mulhi_i(uint32_t a, int m) { return (int)(((uint64_t)a * (uint32_t)m) >> 32); }

// The cutout rectangle and the intensity of dataset row d: one Philox block each and only for the operations that are on,
// counter (draw_id, 0, lane, 0), key (seed, d / recurrence) as for the shift.  The same in all lanes of the work-group.
__device__ __forceinline__ AugS ops_of_sample(const AugOps &p, const int32_t *__restrict__ index, int64_t offset, int64_t i,
                                              int recurrence, uint32_t seed, uint32_t draw_id, int H, int W) {
    const int64_t d = index ? (int64_t)index[i] : offset + i;
    const uint32_t group = (uint32_t)(d / recurrence);
    AugS a{0, 0, 0, 0, 256u, 0u, 1.0f};
    uint32_t w[4];
    if (p.cut_max > 0) {
        sf_philox4x32_10(draw_id, 0u, AUG_LANE_CUTOUT, 0u, seed, group, w);
        const int lo_h = p.cut_min < H ? p.cut_min : H, hi_h = p.cut_max < H ? p.cut_max : H;
        const int lo_w = p.cut_min < W ? p.cut_min : W, hi_w = p.cut_max < W ? p.cut_max : W;
        const int ch = lo_h + mulhi_i(w[0], hi_h - lo_h + 1), cw = lo_w + mulhi_i(w[1], hi_w - lo_w + 1);
        a.cy0 = mulhi_i(w[2], H - ch + 1);
        a.cx0 = mulhi_i(w[3], W - cw + 1);
        a.cy1 = a.cy0 + ch;
        a.cx1 = a.cx0 + cw;
    }
    if (p.intensity > 0 || (p.cut_max > 0 && p.cut_fill)) {
        sf_philox4x32_10(draw_id, 0u, AUG_LANE_INTENSITY, 0u, seed, group, w);
        a.s = 256u - (uint32_t)p.intensity + (uint32_t)mulhi_i(w[0], 2 * p.intensity + 1);
        a.scale = (float)a.s * (1.0f / 256.0f);  // exact: s has 9 bits
        if (p.cut_fill) a.fillw = (w[1] >> 24) * 0x01010101u;
    }
    return a;
}

// a u8 pixel under the scale: min(255, (x s + 128) >> 8); an f32 one: ONE rounded multiply
__device__ __forceinline__ uint32_t scale_u8(uint32_t x, uint32_t s) {
    const uint32_t v = (x * s + 128u) >> 8;
    return v < 255u ? v : 255u;
}
__device__ __forceinline__ uint32_t scale_f32(uint32_t bits, float scale) {
    return __float_as_uint(__fmul_rn(__uint_as_float(bits), scale));
}

// Four u8 pixels under the scale, two at a time in 16-bit halves.  s = 256 hi + lo with hi in {0, 1}: x lo + 128 fits 16
// bits (255 * 255 + 128), and (x s + 128) >> 8 = ((x lo + 128) >> 8) + x hi because x hi 256 is a multiple of 256.
typedef unsigned short aug_u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t scale_u8x2(uint32_t two, uint32_t s) {
    const uint16_t lo = (uint16_t)(s & 255u), hi = (uint16_t)(s >> 8);
    const aug_u16x2 x = __builtin_bit_cast(aug_u16x2, two), l = {lo, lo}, h = {hi, hi}, half = {128, 128}, top = {255, 255};
    const aug_u16x2 r = __builtin_elementwise_min((aug_u16x2)(((x * l + half) >> 8) + x * h), top);
    return __builtin_bit_cast(uint32_t, r);
}
__device__ __forceinline__ uint32_t scale_u8x4(uint32_t v, uint32_t s) {
    return scale_u8x2(v & 0x00FF00FFu, s) | scale_u8x2((v >> 8) & 0x00FF00FFu, s) << 8;
}

// the bytes [lo, hi) of a dword, 0 <= lo <= hi <= 4 (none when hi == lo): one bit-field mask; a field of 32 bits has none
__device__ __forceinline__ uint32_t byte_span(int lo, int hi) {
    const uint32_t m = ((1u << (8 * (hi - lo))) - 1u) << (8 * lo);
    return hi - lo >= 4 ? 0xFFFFFFFFu : m;
}

// A dword that lies in ONE output row (row y of its plane, bytes b .. b + 3 of the row; four u8 pixels or one f32 element
// on the dword grid) after the shift: scaled, then the cutout's fill selected into the bytes whose columns lie in the
// rectangle.  No lane-dependent branch: interior, edge and outside dwords run the same instructions.
template <class G>
__device__ __forceinline__ uint32_t ops_dword(uint32_t v, int y, int b, int sh, const AugS &a) {
    if constexpr (G::INTENSITY) v = sh ? scale_f32(v, a.scale) : scale_u8x4(v, a.s);  // (s = 256 is the identity in both)
    if constexpr (G::CUTOUT) {
        const uint32_t m = byte_span(clampi((a.cx0 << sh) - b, 0, 4), clampi((a.cx1 << sh) - b, 0, 4));
        const uint32_t sel = (y >= a.cy0 && y < a.cy1) ? m : 0u;
        v = (v & ~sel) | (a.fillw & sel);
    }
    return v;
}

// The LDS path.  One work-group per sample (grid-strided).  The sample's output bytes are cut at the 16-byte boundaries of
// their ADDRESSES: a head of h < 16 bytes up to the first boundary, nb whole 16-byte units, a tail of t < 16 bytes.  A
// strip is g.U consecutive units (the head rides with the first strip, the tail with the last); a sample that fits the
// LDS is one strip.  Per strip:
//   1. the frame rows its bytes read — plane-rows s_first .. s_last of the source sample, one contiguous span, because the
//      source plane-row c H + clip(y + dy - pad) never decreases along the output — are staged in LDS as the aligned 16-byte
//      granules that hold them (uint4 loads, contiguous across the wave, two per lane in flight): the LDS image keeps the
//      span's address modulo 16, every source byte is loaded once, nothing is loaded bytewise;
//   2. a lane builds its unit's four dwords from the image.  A u8 dword whose 4 bytes lie in one output row reads the
//      4-byte window of the staged source row that holds its (clamped) columns — at any phase: the two LDS dwords around
//      it, funnel-shifted — and a byte permute repeats the edge pixel where columns clamp; an f32 element on the dword
//      grid is read the same way at its clamped column.  A dword with a row end inside it gathers its bytes one by one.
//      ONE 16-byte store.
//   3. head and tail bytes are gathered the same way and stored bytewise.
// All offsets are below 2^31 (the host checks S): 32-bit arithmetic, divisions by W elem_bytes and H through FastDiv.
//
// G = AugG<..> (sf_augment_gather): the sample's rectangle and scale are drawn once next to its shift; a dword in one row goes
// through ops_dword on its way into the unit, every byte that is gathered singly (head, tail, a dword with a row end
// inside it, f32 off the dword grid) through aug_byte — the same arithmetic on one pixel.
template <class G>
__global__ __launch_bounds__(256) void k_random_shift_gather(char *dst, int64_t dst_pitch, const char *__restrict__ src,
                                                             int64_t src_pitch, const int32_t *__restrict__ index,
                                                             int64_t offset, int64_t n, G g) {
    constexpr bool OPS = G::OPS;
    extern __shared__ uint4 rsg_img16[];
    const uint32_t *img = reinterpret_cast<const uint32_t *>(rsg_img16);
    const uint8_t *img8 = reinterpret_cast<const uint8_t *>(rsg_img16);
    const int tid = threadIdx.x, nt = blockDim.x;
    const int emask = (1 << g.sh) - 1;
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
        int dy, dx;
        const int64_t row = shift_of_sample(index, offset, i, g.traj_T, g.recurrence, g.pad, g.seed, g.draw_id, dy, dx);
        const int shy = dy - g.pad, shx = dx - g.pad;
        AugS au{};
        if constexpr (OPS) au = ops_of_sample(g.ops, index, offset, i, g.recurrence, g.seed, g.draw_id, g.H, g.W);
        const char *srow = src + row * src_pitch;
        char *drow = dst + i * dst_pitch;
        const int to16 = (int)((0 - reinterpret_cast<uintptr_t>(drow)) & 15);
        const int h = to16 < g.S ? to16 : g.S, nb = (g.S - h) >> 4, t = g.S - h - 16 * nb;
        const int nstrips = nb > 0 ? (nb + g.U - 1) / g.U : 1;
        // source plane-row of output plane-row r
        auto src_row = [&](int r) {
            const int c = (int)fdiv((uint32_t)r, g.dH), y = r - c * g.H;
            return c * g.H + clampi(y + shy, 0, g.H - 1);
        };
        for (int k = 0; k < nstrips; ++k) {
            const int u0 = k * g.U, u1 = u0 + g.U < nb ? u0 + g.U : nb;
            const int b0 = k == 0 ? 0 : h + 16 * u0, b1 = k == nstrips - 1 ? g.S : h + 16 * u1;  // the strip's output bytes
            const int q0 = src_row((int)fdiv((uint32_t)b0, g.dWb)) * g.Wb;
            const int q1 = (src_row((int)fdiv((uint32_t)(b1 - 1), g.dWb)) + 1) * g.Wb;            // source bytes [q0, q1)
            const uintptr_t a = reinterpret_cast<uintptr_t>(srow + q0);
            const int ph = (int)(a & 15), n16 = (ph + (q1 - q0) + 15) >> 4;
            const uint4 *g16 = reinterpret_cast<const uint4 *>(a - ph);
            __syncthreads();  // the image's readers are done
            for (int j = tid; j < n16; j += 2 * nt) {
                const int j2 = j + nt < n16 ? j + nt : j;
                const uint4 v0 = g16[j], v1 = g16[j2];
                rsg_img16[j] = v0;
                if (j2 != j) rsg_img16[j2] = v1;
            }
            __syncthreads();
            const int base = ph - q0;  // source byte q of the sample sits at image byte base + q
            // image byte of output byte o
            auto byte_at = [&](int o) {
                const int r = (int)fdiv((uint32_t)o, g.dWb), b = o - r * g.Wb;
                const int x = clampi((b >> g.sh) + shx, 0, g.W - 1);
                return base + src_row(r) * g.Wb + (x << g.sh) + (b & emask);
            };
            // output byte o under the operations (G = AugG): the fill inside the rectangle, else the pixel that holds it,
            // scaled (an f32 pixel is put together from its four bytes first)
            auto aug_byte = [&](int o) -> uint32_t {
                const int r = (int)fdiv((uint32_t)o, g.dWb), b = o - r * g.Wb, xo = b >> g.sh;
                const int y = r - (int)fdiv((uint32_t)r, g.dH) * g.H;
                if (y >= au.cy0 && y < au.cy1 && xo >= au.cx0 && xo < au.cx1) return au.fillw & 255u;
                const int at = base + src_row(r) * g.Wb + (clampi(xo + shx, 0, g.W - 1) << g.sh);
                if (g.sh == 0) return au.s != 256u ? scale_u8(img8[at], au.s) : img8[at];
                uint32_t e = (uint32_t)img8[at] | (uint32_t)img8[at + 1] << 8 | (uint32_t)img8[at + 2] << 16 | (uint32_t)img8[at + 3] << 24;
                if (au.s != 256u) e = scale_f32(e, au.scale);
                return (e >> (8 * (b & 3))) & 255u;
            };
            // the four dwords of a unit, walked along the output: (c, y, b) = the dword's plane, row and byte in the row,
            // rb = the image byte of its source row's first byte; one division pair per unit, a row end only steps them.
            //   u8, in one row: the row's 4-byte window that holds the dword's (clamped) columns — it starts at
            //     clip(x0, 0, W - 4) — from the two LDS dwords around it, funnel-shifted, and ONE byte permute whose selector
            //     repeats the edge pixel (the identity away from the border): no branch between interior and border;
            //   f32 on the dword grid: the element at its clamped column, read the same way;
            //   rows narrower than 4 pixels, f32 off the dword grid: 4 byte reads of the same source row;
            //   a row end inside the dword: byte by byte.
            const bool window4 = g.sh == 0 && g.W >= 4;
            for (int u = u0 + tid; u < u1; u += nt) {
                const int o = h + 16 * u;
                const int r = (int)fdiv((uint32_t)o, g.dWb);
                int b = o - r * g.Wb, c = (int)fdiv((uint32_t)r, g.dH), y = r - c * g.H;
                int rb = base + (c * g.H + clampi(y + shy, 0, g.H - 1)) * g.Wb;
                uint32_t v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (b >= g.Wb) {  // the dword begins a later row
                        if (g.Wb >= 4) {
                            b -= g.Wb;
                            y += 1;
                            if (y == g.H) { y = 0; c += 1; }
                        } else {
                            const int r2 = (int)fdiv((uint32_t)(o + 4 * j), g.dWb);
                            b = o + 4 * j - r2 * g.Wb;
                            c = (int)fdiv((uint32_t)r2, g.dH);
                            y = r2 - c * g.H;
                        }
                        rb = base + (c * g.H + clampi(y + shy, 0, g.H - 1)) * g.Wb;
                    }
                    if (b + 3 < g.Wb && (window4 || (g.sh == 2 && (b & 3) == 0))) {
                        const int x0 = (b >> g.sh) + shx;
                        const int a0 = clampi(x0, 0, window4 ? g.W - 4 : g.W - 1), at = rb + (a0 << g.sh);
                        const uint32_t lo = img[at >> 2], hi = img[(at >> 2) + 1];
                        const uint32_t win = (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (at & 3)));
                        // u8: byte q of the dword is column clip(x0 + q): window byte clip(x0 - a0 + q, 0, 3) — 4 bytes of
                        // the sequence 0 0 0 0 0 1 2 3 3 3 3 3 from position 4 + clip(x0 - a0, -4, 4)
                        const int dl = window4 ? clampi(x0 - a0, -4, 4) : 0;
                        const uint64_t seq = dl <= 0 ? (uint64_t)0x03020100u << 32 : ((uint64_t)0x03030303u << 32) | 0x03020100u;
                        const uint32_t sel = (uint32_t)(seq >> (8 * (dl <= 0 ? 4 + dl : dl)));
                        v[j] = __builtin_amdgcn_perm(0u, win, sel);
                        if constexpr (OPS) v[j] = ops_dword<G>(v[j], y, b, g.sh, au);
                    } else if (!OPS && b + 3 < g.Wb) {
                        v[j] = 0;
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int x = clampi(((b + q) >> g.sh) + shx, 0, g.W - 1);
                            v[j] |= (uint32_t)img8[rb + (x << g.sh) + ((b + q) & emask)] << (8 * q);
                        }
                    } else {
                        v[j] = 0;
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            if constexpr (OPS) v[j] |= aug_byte(o + 4 * j + q) << (8 * q);
                            else v[j] |= (uint32_t)img8[byte_at(o + 4 * j + q)] << (8 * q);
                        }
                    }
                    b += 4;
                }
                *reinterpret_cast<uint4 *>(drow + o) = uint4{v[0], v[1], v[2], v[3]};
            }
            if constexpr (OPS) {
                if (k == 0 && tid < h) drow[tid] = (char)aug_byte(tid);
                if (k == nstrips - 1 && tid < t) drow[h + 16 * nb + tid] = (char)aug_byte(h + 16 * nb + tid);
            } else {
                if (k == 0 && tid < h) drow[tid] = (char)img8[byte_at(tid)];
                if (k == nstrips - 1 && tid < t) drow[h + 16 * nb + tid] = (char)img8[byte_at(h + 16 * nb + tid)];
            }
        }
    }
}

// Samples whose rows do not fit the LDS strips, or of 2^31 bytes and more: 64-bit offsets, no LDS.  A lane owns one
// ALIGNED dword of the output (the first and the last may reach outside the sample: their bytes inside are stored
// one by one), and reads every source byte out of the aligned dword that holds it (the caches serve the re-reads).
// Merely correct.  G = AugG<..>: every byte is its pixel's, scaled (an f32 pixel from its four bytes), or the fill.
template <class G>
__global__ __launch_bounds__(RSG_WIDE_BLOCK) void k_random_shift_gather_wide(char *dst, int64_t dst_pitch,
                                                                             const char *__restrict__ src, int64_t src_pitch,
                                                                             const int32_t *__restrict__ index, int64_t offset,
                                                                             int64_t n, G g) {
    constexpr bool OPS = G::OPS;
    const int64_t Wb = (int64_t)g.W << g.sh, S = Wb * g.H * g.C;
    const int emask = (1 << g.sh) - 1;
    for (int64_t i = blockIdx.y; i < n; i += gridDim.y) {
        int dy, dx;
        const int64_t row = shift_of_sample(index, offset, i, g.traj_T, g.recurrence, g.pad, g.seed, g.draw_id, dy, dx);
        const int shy = dy - g.pad, shx = dx - g.pad;
        AugS au{};
        if constexpr (OPS) au = ops_of_sample(g.ops, index, offset, i, g.recurrence, g.seed, g.draw_id, g.H, g.W);
        const uintptr_t sa = reinterpret_cast<uintptr_t>(src + row * src_pitch);
        char *drow = dst + i * dst_pitch;
        const uintptr_t D = reinterpret_cast<uintptr_t>(drow), D0 = D & ~(uintptr_t)3;
        const int64_t nd = (int64_t)((((D + (uintptr_t)S + 3) & ~(uintptr_t)3) - D0) >> 2);
        for (int64_t wd = (int64_t)blockIdx.x * RSG_WIDE_BLOCK + threadIdx.x; wd < nd; wd += (int64_t)gridDim.x * RSG_WIDE_BLOCK) {
            const int64_t o0 = (int64_t)(D0 - D) + 4 * wd;  // (negative for the bytes in front of the sample)
            uint32_t out = 0;
            uint8_t px[4] = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t o = o0 + j;
                if (o < 0 || o >= S) continue;
                const int64_t r = o / Wb, b = o - r * Wb, c = r / g.H;
                const int y = clampi((int)(r - c * g.H) + shy, 0, g.H - 1);
                const int x = clampi((int)(b >> g.sh) + shx, 0, g.W - 1);
                const uintptr_t at = sa + (uintptr_t)((c * g.H + y) * Wb + ((int64_t)x << g.sh) + (b & emask));
                auto src_byte = [](uintptr_t p) { return (*reinterpret_cast<const uint32_t *>(p & ~(uintptr_t)3) >> (8 * (p & 3))) & 255u; };
                if constexpr (OPS) {
                    const int yo = (int)(r - c * g.H), xo = (int)(b >> g.sh);
                    if (yo >= au.cy0 && yo < au.cy1 && xo >= au.cx0 && xo < au.cx1) {
                        px[j] = (uint8_t)au.fillw;
                    } else if (g.sh == 0) {
                        px[j] = (uint8_t)(au.s != 256u ? scale_u8(src_byte(at), au.s) : src_byte(at));
                    } else {
                        const uintptr_t e0 = at - (uintptr_t)(b & 3);
                        uint32_t e = src_byte(e0) | src_byte(e0 + 1) << 8 | src_byte(e0 + 2) << 16 | src_byte(e0 + 3) << 24;
                        if (au.s != 256u) e = scale_f32(e, au.scale);
                        px[j] = (uint8_t)(e >> (8 * (b & 3)));
                    }
                } else {
                    px[j] = (uint8_t)(*reinterpret_cast<const uint32_t *>(at & ~(uintptr_t)3) >> (8 * (at & 3)));
                }
                out |= (uint32_t)px[j] << (8 * j);
            }
            if (o0 >= 0 && o0 + 4 <= S) {
                *reinterpret_cast<uint32_t *>(drow + o0) = out;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (o0 + j >= 0 && o0 + j < S) drow[o0 + j] = (char)px[j];
            }
        }
    }
}

}  // namespace

template <class G>
static void launch_lds(dim3 grid, dim3 block, size_t lds, void *stream, char *d, int64_t dp, const char *s, int64_t sp,
                       const int32_t *index, int64_t offset, int64_t n, const G &g) {
    k_random_shift_gather<G><<<grid, block, lds, STREAM(stream)>>>(d, dp, s, sp, index, offset, n, g);
}
template <class G>
static void launch_wide(dim3 grid, void *stream, char *d, int64_t dp, const char *s, int64_t sp, const int32_t *index,
                        int64_t offset, int64_t n, const G &g) {
    k_random_shift_gather_wide<G><<<grid, dim3(RSG_WIDE_BLOCK), 0, STREAM(stream)>>>(d, dp, s, sp, index, offset, n, g);
}
// ShiftG widened to the instantiation that compiles in exactly the operations `ops` switches on
template <class F>
static void with_ops_geometry(const ShiftG &g, const AugOps &ops, F &&launch) {
    auto as = [&](auto gg) {
        static_cast<ShiftG &>(gg) = g;
        gg.ops = ops;
        launch(gg);
    };
    if (ops.cut_max > 0 && ops.intensity > 0) as(AugG<true, true>{});
    else if (ops.cut_max > 0) as(AugG<true, false>{});
    else as(AugG<false, true>{});
}

// both entry points: the refusals (under the caller's name), the strip plan and the launch; ops = nullptr or all off runs the
// shift-only kernels
static int gather_launch(const char *who, void *dst, int64_t dst_sample_pitch, const void *src, int64_t src_sample_pitch,
                         const int32_t *index, int64_t offset, int64_t n, int traj_T, int C, int H, int W, int elem_bytes,
                         int pad, const AugOps *ops, int recurrence, uint32_t seed, uint32_t draw_id, void *stream) {
    SF_REQUIRE(dst && src, "%s: null dst / src", who);
    SF_REQUIRE(n >= 0, "%s: n=%lld", who, (long long)n);
    SF_REQUIRE(pad >= 0 && pad <= 255, "%s: pad=%d outside 0..255", who, pad);
    SF_REQUIRE(elem_bytes == 1 || elem_bytes == 4, "%s: elem_bytes=%d (1 = u8 or 4 = f32)", who, elem_bytes);
    SF_REQUIRE(recurrence >= 1, "%s: recurrence=%d (at least 1)", who, recurrence);
    SF_REQUIRE(C >= 1 && H >= 1 && W >= 1, "%s: C=%d H=%d W=%d (each at least 1)", who, C, H, W);
    SF_REQUIRE(traj_T >= 0 && offset >= 0, "%s: traj_T=%d offset=%lld", who, traj_T, (long long)offset);
    SF_REQUIRE((int64_t)H * W <= ((int64_t)1 << 40) / ((int64_t)C * elem_bytes),
               "%s: sample of %d x %d x %d too large", who, C, H, W);
    const int64_t Wb = (int64_t)W * elem_bytes, S = Wb * H * C;
    SF_REQUIRE(dst_sample_pitch >= S && src_sample_pitch >= S,
               "%s: pitches %lld / %lld smaller than a sample of C H W elem_bytes = %lld", who,
               (long long)dst_sample_pitch, (long long)src_sample_pitch, (long long)S);
    if (ops) {
        const bool cut = ops->cut_max != 0;
        SF_REQUIRE(ops->cut_max >= 0 && ops->cut_max <= 65535, "%s: cut_max=%d outside 0..65535 (0 = off)", who, ops->cut_max);
        SF_REQUIRE(!cut || (ops->cut_min >= 1 && ops->cut_min <= ops->cut_max),
                   "%s: cut_min=%d cut_max=%d (1 <= cut_min <= cut_max)", who, ops->cut_min, ops->cut_max);
        SF_REQUIRE(ops->cut_fill == 0 || ops->cut_fill == 1, "%s: cut_fill=%d (0 = zero or 1 = random)", who, ops->cut_fill);
        SF_REQUIRE(ops->intensity >= 0 && ops->intensity <= 255, "%s: intensity=%d outside 0..255", who, ops->intensity);
        SF_REQUIRE(!(ops->cut_fill == 1 && elem_bytes == 4), "%s: cut_fill=1 (a random byte) with elem_bytes=4: u8 frames only", who);
    }
    if (n == 0) return SF_OK;
    const bool with_ops = ops && (ops->cut_max > 0 || ops->intensity > 0);
    ShiftG g{};
    g.C = C; g.H = H; g.W = W; g.sh = elem_bytes == 4 ? 2 : 0;
    g.pad = pad; g.recurrence = recurrence; g.traj_T = traj_T; g.seed = seed; g.draw_id = draw_id;
    char *d = reinterpret_cast<char *>(dst);
    const char *s = reinterpret_cast<const char *>(src);
    // the strip: the whole sample where its rows fit the LDS, else as many 16-byte units as are SURE to: a strip of
    // 16 U + 30 bytes (head and tail included) touches at most R = (16 U + 29) / Wb + 2 output plane-rows; along them the
    // source plane-row advances by one per row and by up to pad + 1 where the next plane begins
    int64_t U = 0, lds = 0;
    if (S < ((int64_t)1 << 31) - 64) {
        auto image_bytes = [&](int64_t rows) { return (rows * Wb + 15 + 15) / 16 * 16 + 16; };  // phase, round-up, the pair's 2nd dword
        if (image_bytes((int64_t)C * H) <= RSG_LDS_BYTES) {
            U = (S >> 4) + 1;
            lds = image_bytes((int64_t)C * H);
        } else {
            for (int64_t u = RSG_LDS_BYTES / 32; u >= 1 && !U; u >>= 1) {
                const int64_t R = (16 * u + 29) / Wb + 2, span = R + ((R - 1) / H + 1) * pad;
                if (image_bytes(span) <= RSG_LDS_BYTES) {
                    U = u;
                    lds = image_bytes(span < (int64_t)C * H ? span : (int64_t)C * H);
                }
            }
        }
    }
    if (U) {
        g.Wb = (int)Wb; g.S = (int)S; g.U = (int)U;
        g.dWb = make_fastdiv((uint32_t)Wb);
        g.dH = make_fastdiv((uint32_t)H);
        const int block = S <= 4096 ? 64 : 256;
        const dim3 grid((unsigned)(n < RSG_GRID ? n : RSG_GRID));
        auto launch = [&](const auto &gg) {
            launch_lds(grid, dim3(block), (size_t)lds, stream, d, dst_sample_pitch, s, src_sample_pitch, index, offset, n, gg);
        };
        if (with_ops) with_ops_geometry(g, *ops, launch);
        else launch(g);
    } else {
        const int64_t bx = (S / 4 + RSG_WIDE_BLOCK) / RSG_WIDE_BLOCK;
        const dim3 grid((unsigned)(bx < 1024 ? bx : 1024), (unsigned)(n < 65535 ? n : 65535));
        auto launch = [&](const auto &gg) { launch_wide(grid, stream, d, dst_sample_pitch, s, src_sample_pitch, index, offset, n, gg); };
        if (with_ops) with_ops_geometry(g, *ops, launch);
        else launch(g);
    }
    return sf_launch_status(who);
}

extern "C" int sf_random_shift_gather(void *dst, int64_t dst_sample_pitch, const void *src, int64_t src_sample_pitch,
                                      const int32_t *index, int64_t offset, int64_t n, int traj_T, int C, int H, int W,
                                      int elem_bytes, int pad, int recurrence, uint32_t seed, uint32_t draw_id, void *stream) {
    return gather_launch("sf_random_shift_gather", dst, dst_sample_pitch, src, src_sample_pitch, index, offset, n, traj_T, C, H, W,
                         elem_bytes, pad, nullptr, recurrence, seed, draw_id, stream);
}

// The shift, then the intensity scale, then the cutout (include/sf_hip.h).  With both off it is sf_random_shift_gather.
extern "C" int sf_augment_gather(void *dst, int64_t dst_sample_pitch, const void *src, int64_t src_sample_pitch,
                                 const int32_t *index, int64_t offset, int64_t n, int traj_T, int C, int H, int W, int elem_bytes,
                                 int pad, int cut_min, int cut_max, int cut_fill, int intensity, int recurrence, uint32_t seed,
                                 uint32_t draw_id, void *stream) {
    const AugOps ops{cut_min, cut_max, cut_fill, intensity};
    return gather_launch("sf_augment_gather", dst, dst_sample_pitch, src, src_sample_pitch, index, offset, n, traj_T, C, H, W,
                         elem_bytes, pad, &ops, recurrence, seed, draw_id, stream);
}
