// sf_augment.hip — training-time image augmentation on the device (gfx950): the random shift of RAD / DrQ / DrAC (pad by
// `pad` pixels with edge replication, crop back at a random offset) as ONE gather launch that reads a minibatch's frames
// through the learner's row addressing and writes a dense [n][C][H][W] batch.  pad = 0 is the plain gather.  A byte mover:
// u8 and f32 frames alike, any alignment of src, dst and the pitches.  Contract: include/sf_hip.h; the NumPy model is
// sample_factory_amd/envs/frame_ops.py (random_shift_draws, random_shift_frames).
#include "sf_common.h"

#define STREAM(s) reinterpret_cast<hipStream_t>(s)

namespace {

constexpr int RSG_LDS_BYTES = 64 * 1024;  // the staged source rows of one work-group at most
constexpr int RSG_GRID = 8192;            // work-groups along the samples at most (grid-strided)
constexpr int RSG_WIDE_BLOCK = 256;

struct ShiftG {
    int C, H, W, sh;  // sh = log2(elem_bytes): 0 (u8) or 2 (f32)
    int Wb, S;        // bytes of a frame row and of a sample
    int pad, recurrence, traj_T;
    int U;            // 16-byte output units per strip
    uint32_t seed, draw_id;
    FastDiv dWb, dH;
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
__global__ __launch_bounds__(256) void k_random_shift_gather(char *dst, int64_t dst_pitch, const char *__restrict__ src,
                                                             int64_t src_pitch, const int32_t *__restrict__ index,
                                                             int64_t offset, int64_t n, ShiftG g) {
    extern __shared__ uint4 rsg_img16[];
    const uint32_t *img = reinterpret_cast<const uint32_t *>(rsg_img16);
    const uint8_t *img8 = reinterpret_cast<const uint8_t *>(rsg_img16);
    const int tid = threadIdx.x, nt = blockDim.x;
    const int emask = (1 << g.sh) - 1;
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
        int dy, dx;
        const int64_t row = shift_of_sample(index, offset, i, g.traj_T, g.recurrence, g.pad, g.seed, g.draw_id, dy, dx);
        const int shy = dy - g.pad, shx = dx - g.pad;
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
                    } else if (b + 3 < g.Wb) {
                        v[j] = 0;
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int x = clampi(((b + q) >> g.sh) + shx, 0, g.W - 1);
                            v[j] |= (uint32_t)img8[rb + (x << g.sh) + ((b + q) & emask)] << (8 * q);
                        }
                    } else {
                        v[j] = 0;
#pragma unroll
                        for (int q = 0; q < 4; ++q) v[j] |= (uint32_t)img8[byte_at(o + 4 * j + q)] << (8 * q);
                    }
                    b += 4;
                }
                *reinterpret_cast<uint4 *>(drow + o) = uint4{v[0], v[1], v[2], v[3]};
            }
            if (k == 0 && tid < h) drow[tid] = (char)img8[byte_at(tid)];
            if (k == nstrips - 1 && tid < t) drow[h + 16 * nb + tid] = (char)img8[byte_at(h + 16 * nb + tid)];
        }
    }
}

// Samples whose rows do not fit the LDS strips, or of 2^31 bytes and more: 64-bit offsets, no LDS.  A lane owns one
// ALIGNED dword of the output (the first and the last may reach outside the sample: their bytes inside are stored
// one by one), and reads every source byte out of the aligned dword that holds it (the caches serve the re-reads).
// Merely correct.
__global__ __launch_bounds__(RSG_WIDE_BLOCK) void k_random_shift_gather_wide(char *dst, int64_t dst_pitch,
                                                                             const char *__restrict__ src, int64_t src_pitch,
                                                                             const int32_t *__restrict__ index, int64_t offset,
                                                                             int64_t n, ShiftG g) {
    const int64_t Wb = (int64_t)g.W << g.sh, S = Wb * g.H * g.C;
    const int emask = (1 << g.sh) - 1;
    for (int64_t i = blockIdx.y; i < n; i += gridDim.y) {
        int dy, dx;
        const int64_t row = shift_of_sample(index, offset, i, g.traj_T, g.recurrence, g.pad, g.seed, g.draw_id, dy, dx);
        const int shy = dy - g.pad, shx = dx - g.pad;
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
                px[j] = (uint8_t)(*reinterpret_cast<const uint32_t *>(at & ~(uintptr_t)3) >> (8 * (at & 3)));
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

extern "C" int sf_random_shift_gather(void *dst, int64_t dst_sample_pitch, const void *src, int64_t src_sample_pitch,
                                      const int32_t *index, int64_t offset, int64_t n, int traj_T, int C, int H, int W,
                                      int elem_bytes, int pad, int recurrence, uint32_t seed, uint32_t draw_id, void *stream) {
    SF_REQUIRE(dst && src, "sf_random_shift_gather: null dst / src");
    SF_REQUIRE(n >= 0, "sf_random_shift_gather: n=%lld", (long long)n);
    SF_REQUIRE(pad >= 0 && pad <= 255, "sf_random_shift_gather: pad=%d outside 0..255", pad);
    SF_REQUIRE(elem_bytes == 1 || elem_bytes == 4, "sf_random_shift_gather: elem_bytes=%d (1 = u8 or 4 = f32)", elem_bytes);
    SF_REQUIRE(recurrence >= 1, "sf_random_shift_gather: recurrence=%d (at least 1)", recurrence);
    SF_REQUIRE(C >= 1 && H >= 1 && W >= 1, "sf_random_shift_gather: C=%d H=%d W=%d (each at least 1)", C, H, W);
    SF_REQUIRE(traj_T >= 0 && offset >= 0, "sf_random_shift_gather: traj_T=%d offset=%lld", traj_T, (long long)offset);
    SF_REQUIRE((int64_t)H * W <= ((int64_t)1 << 40) / ((int64_t)C * elem_bytes),
               "sf_random_shift_gather: sample of %d x %d x %d too large", C, H, W);
    const int64_t Wb = (int64_t)W * elem_bytes, S = Wb * H * C;
    SF_REQUIRE(dst_sample_pitch >= S && src_sample_pitch >= S,
               "sf_random_shift_gather: pitches %lld / %lld smaller than a sample of C H W elem_bytes = %lld",
               (long long)dst_sample_pitch, (long long)src_sample_pitch, (long long)S);
    if (n == 0) return SF_OK;
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
        k_random_shift_gather<<<dim3((unsigned)(n < RSG_GRID ? n : RSG_GRID)), dim3(block), (size_t)lds, STREAM(stream)>>>(
            d, dst_sample_pitch, s, src_sample_pitch, index, offset, n, g);
    } else {
        const int64_t bx = (S / 4 + RSG_WIDE_BLOCK) / RSG_WIDE_BLOCK;
        k_random_shift_gather_wide<<<dim3((unsigned)(bx < 1024 ? bx : 1024), (unsigned)(n < 65535 ? n : 65535)),
                                     dim3(RSG_WIDE_BLOCK), 0, STREAM(stream)>>>(d, dst_sample_pitch, s, src_sample_pitch, index,
                                                                                offset, n, g);
    }
    return sf_launch_status("sf_random_shift_gather");
}
