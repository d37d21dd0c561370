// sf_ingest.hip — observation ingest helpers that run on the device (gfx950): the frame stack of image observations.
//
// A host env that delivers ONE new frame per step (--device_framestack=k) has its k-frame observation assembled in the
// trajectory slab: obs[:, t + 1] = the k - 1 newest frames of obs[:, t] followed by the new frame, or k copies of the new
// frame where an episode ended (gym.wrappers.FrameStack over an auto-resetting env).  Contract: include/sf_hip.h.
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

}  // namespace

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
