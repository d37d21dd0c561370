// sf_pixcatch.hip — PixelCatch, a device-resident pixel game (gfx950): ONE launch advances N games and renders the next
// observation of every game straight into its row of a slab column.  Integer arithmetic only; the NumPy model in
// sample_factory_amd/envs/pixel_catch.py is the contract and this file equals it bit for bit.  Contract: include/sf_hip.h.
//
// Work split: one work-group per env.  Every lane reads the env's old state words, all lanes compute the same new state
// (uniform values), a barrier follows, and only then lane 0 writes the new words, the reward and the flag: no work-group
// ever renders from a state another one has advanced.  The frame is a pure store stream: the k planes are walked one after
// the other (plane geometry uniform), a lane owns one store unit (16 or 4 bytes) at a time, contiguous across the wave.  A
// unit whose rows touch neither the ball's rows nor the paddle's is background and is stored as zeros at once; the others
// build their bytes in registers from the rectangles' coordinates, a row end (or a plane end) inside the unit included.
// The launch is bound by its stores as long as the integer work stays small: building every unit byte by byte took 35.0 us
// at 4096 x 4 x 84 x 84 where the stores alone take 28; with the zero test and pc_unit16 it takes 27.8 us.
//
// Levels (sf_pixcatch_reset_levels / sf_pixcatch_step_levels, template parameter DECOYS): the up to 8 static decoys of the
// episode's level are the same in all k planes, so the work-group keeps ONE plane of them in LDS, as the bytes the frame
// gets (255 in a decoy, else 0).  The level is drawn once, from uniform values (one Philox block on the scalar unit); lane
// d bs + i of the first waves draws decoy d (one block) and writes row i of it, between two barriers, the first of which
// is the barrier the state already needs.  A store unit then ORs the plane's bytes at its first pixel's index over what it
// built from ball and paddle: one aligned 16-byte LDS read where planes are multiples of 16 bytes, aligned dwords shifted
// by bytes elsewhere (bytes HW .. HW + 15 repeat bytes 0 .. 15, for a unit that runs into the next plane).  The background
// test and the unit builders are those of the game without levels: a unit that holds nothing but decoys costs the LDS read
// and four ORs, whatever the number of decoys.  DECOYS = false compiles to the kernel without levels: no LDS, one barrier.
#include "sf_common.h"

#define STREAM(s) reinterpret_cast<hipStream_t>(s)

namespace {

constexpr int PC_BLOCK = 256;
constexpr int PC_MAX_K = 8;
constexpr int PC_HDR = 4;        // state words before the history: draw index, balls left, vx, vy
constexpr int PC_MAX_SIDE = 1024;  // px, bx, by are packed into 10 bits each while a frame is rendered
constexpr int PC_MAX_DECOYS = 8;
constexpr uint32_t PC_LEVEL_KEY = 0x4C564C53u;  // key word 0 of the decoys' Philox stream: no seed, no env in it
// counter lane 2 of the library's Philox streams (sf_hip.h): 4 is the ball's draw below, 5 the random shift's
constexpr uint32_t PC_LANE_LEVEL = 6u;  // the level of an episode
constexpr uint32_t PC_LANE_DECOY = 7u;  // the decoys of a level
constexpr int PC_MAX_MAP_BYTES = 64 * 1024;     // the decoy plane has to fit the LDS of one work-group

// The game's constants: fixed integer functions of the field (pixel_catch.geometry is the same arithmetic).
struct PcGeom {
    int bs;   // ball: bs x bs pixels
    int pw;   // paddle width
    int ph;   // paddle height; the paddle occupies rows [H - ph, H)
    int ps;   // paddle speed, pixels per step
    int vxm;  // |vx| <= vxm
    int vym;  // vy in 1 .. vym
    int D;    // the ball has reached the paddle's rows when by >= D = H - ph - bs + 1
    int ok;
};

PcGeom pc_geom(int H, int W) {
    PcGeom g;
    const int m = H < W ? H : W;
    g.bs = m / 21 > 2 ? m / 21 : 2;
    g.pw = W / 7 > 3 ? W / 7 : 3;
    g.ph = H / 28 > 1 ? H / 28 : 1;
    g.ps = (W + 27) / 28;
    g.vxm = W / 42 > 1 ? W / 42 : 1;
    g.D = H - g.ph - g.bs + 1;
    g.vym = ((g.D + 1) / 2) * g.ps >= W - g.pw ? 2 : 1;
    // a player who knows the landing column gets there even at vy = 1 .. vym from the far edge; one reflection per step
    g.ok = H >= 1 && W >= 1 && H <= PC_MAX_SIDE && W <= PC_MAX_SIDE && g.D >= 2 && W - g.pw >= 1 && W - g.bs >= g.vxm &&
           (int64_t)g.D * g.ps >= W - g.pw;
    return g;
}

struct PcArgs {
    int H, W, HW, k, balls;
    PcGeom g;
    FastDiv dW;
    int decoys, levels;  // DECOYS kernels only
    uint32_t start_level;
};

// dwords of the decoy plane of an H x W field: bytes [0, HW + 16) and the dword behind them that the byte shift reads
__host__ __device__ inline int pc_map_words(int HW) { return (HW + 16 + 3) / 4 + 1; }

__device__ __forceinline__ uint32_t pc_mulhi(uint32_t word, uint32_t range) { return __umulhi(word, range); }

__device__ __forceinline__ uint32_t pc_pack(int px, int bx, int by) {
    return (uint32_t)px | ((uint32_t)bx << 10) | ((uint32_t)by << 20);
}

// The general form: the bytes of one store unit of `NW` dwords, one by one, first byte at (x, y) of the plane with geometry
// g0; the unit may cross any number of row ends and run into the next plane (geometry g1).  No branch per byte: compares and
// selects only.
template <int NW>
__device__ __forceinline__ void pc_unit(uint32_t (&w)[NW], uint32_t x, uint32_t y, uint32_t g0, uint32_t g1, const PcArgs &a) {
    const uint32_t W = (uint32_t)a.W, H = (uint32_t)a.H, bs = (uint32_t)a.g.bs, pw = (uint32_t)a.g.pw, ph = (uint32_t)a.g.ph;
    const uint32_t py = H - ph;
    uint32_t px = g0 & 1023u, bx = (g0 >> 10) & 1023u, by = g0 >> 20;
#pragma unroll
    for (int i = 0; i < NW; ++i) w[i] = 0;
#pragma unroll
    for (int i = 0; i < 4 * NW; ++i) {
        const bool ball = (x - bx < bs) & (y - by < bs);
        const bool pad = (x - px < pw) & (y - py < ph);
        const uint32_t v = ball ? 255u : (pad ? 128u : 0u);
        w[i >> 2] |= v << (8 * (i & 3));
        ++x;
        const bool wrap = x == W;
        x = wrap ? 0u : x;
        y += wrap ? 1u : 0u;
        const bool next = y == H;
        y = next ? 0u : y;
        px = next ? (g1 & 1023u) : px;
        bx = next ? ((g1 >> 10) & 1023u) : bx;
        by = next ? (g1 >> 20) : by;
    }
}

// bits [lo, lo + len) of a 16-bit byte mask, cut to [i0, i1), or nothing when the row is not one of the rectangle's
__device__ __forceinline__ uint32_t pc_bits(int lo, int len, int i0, int i1, bool on) {
    const int a = min(max(lo, i0), i1), b = min(max(lo + len, i0), i1);
    return on ? (1u << b) - (1u << a) : 0u;
}

// The 16 bytes of a unit of a field at least 16 wide, inside one plane: it covers bytes [0, s) of row y and bytes [s, 16) of
// row y + 1 (s = 16: one row).  Each rectangle contributes at most one run of bytes per row: one bit per byte first, then the
// bits are spread to bytes, four at a time, with shifts (ball 255 = 128 | 127, paddle 128).
__device__ __forceinline__ void pc_unit16(uint32_t (&w)[4], uint32_t x, uint32_t y, uint32_t g0, const PcArgs &a) {
    const int W = a.W, bs = a.g.bs, pw = a.g.pw;
    const uint32_t py = (uint32_t)(a.H - a.g.ph), ph = (uint32_t)a.g.ph;
    const int px = (int)(g0 & 1023u), bx = (int)((g0 >> 10) & 1023u);
    const uint32_t by = g0 >> 20;
    const int s = min(W - (int)x, 16);
    const uint32_t ball = pc_bits(bx - (int)x, bs, 0, s, y - by < (uint32_t)bs) | pc_bits(s + bx, bs, s, 16, y + 1 - by < (uint32_t)bs);
    const uint32_t pad = (pc_bits(px - (int)x, pw, 0, s, y - py < ph) | pc_bits(s + px, pw, s, 16, y + 1 - py < ph)) & ~ball;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t nb = (ball >> (4 * i)) & 15u, np = (pad >> (4 * i)) & 15u;
        const uint32_t tb = (nb | (nb << 7) | (nb << 14) | (nb << 21)) & 0x01010101u;  // bit j -> byte j
        const uint32_t tp = (np | (np << 7) | (np << 14) | (np << 21)) & 0x01010101u;
        w[i] = ((tb | tp) << 7) | ((tb << 7) - tb);
    }
}

// GENERIC: bytes one by one (fields narrower than 16, 4-byte units, units that straddle a plane end); else pc_unit16.
// DECOYS: the levels of sf_pixcatch_*_levels; dynamic LDS of pc_map_words(HW) dwords.
template <int U, bool GENERIC, bool DECOYS>
__global__ __launch_bounds__(PC_BLOCK) void k_pixcatch(int32_t *state, const int32_t *actions, uint8_t *obs, int64_t pitch,
                                                       float *rewards, uint8_t *terminated, int N, int env0, uint32_t seed,
                                                       PcArgs a, int reset) {
    constexpr int NW = U / 4;
    const int e = blockIdx.x;
    if (e >= N) return;
    const int k = a.k, W = a.W, words = PC_HDR + 3 * k;
    int32_t *st = state + (int64_t)e * words;

    // ---- the old state, read by every lane before any lane writes (the barrier below)
    int32_t draw = 0, left = a.balls, vx = 0, vy = 1, px = (W - a.g.pw) / 2, bx = 0, by = 0;
    uint32_t hist[PC_MAX_K];  // plane j: packed (px, bx, by); plane k - 1 is the current position
#pragma unroll
    for (int j = 0; j < PC_MAX_K; ++j) hist[j] = 0;
    if (!reset) {
        draw = __builtin_amdgcn_readfirstlane(st[0]);
        left = __builtin_amdgcn_readfirstlane(st[1]);
        vx = __builtin_amdgcn_readfirstlane(st[2]);
        vy = __builtin_amdgcn_readfirstlane(st[3]);
#pragma unroll
        for (int j = 0; j < PC_MAX_K; ++j)
            if (j < k) {
                const int32_t hx = __builtin_amdgcn_readfirstlane(st[PC_HDR + 3 * j]);
                const int32_t hb = __builtin_amdgcn_readfirstlane(st[PC_HDR + 3 * j + 1]);
                const int32_t hy = __builtin_amdgcn_readfirstlane(st[PC_HDR + 3 * j + 2]);
                hist[j] = pc_pack(hx, hb, hy);
                if (j == k - 1) { px = hx; bx = hb; by = hy; }
            }
    }

    // ---- one step of the game (uniform across the work-group)
    float reward = 0.0f;
    int term = 0;
    bool fill = reset != 0, new_ball = reset != 0;
    if (!reset) {
        const int act = __builtin_amdgcn_readfirstlane(actions[e]);
        const int dx = act == 1 ? -a.g.ps : (act == 2 ? a.g.ps : 0);  // any other value: stay
        px = min(max(px + dx, 0), W - a.g.pw);
        const int mx = W - a.g.bs;
        bx += vx;
        if (bx < 0) { bx = -bx; vx = -vx; }
        if (bx > mx) { bx = 2 * mx - bx; vx = -vx; }
        by += vy;
        if (by >= a.g.D) {
            const bool caught = (px < bx + a.g.bs) & (bx < px + a.g.pw);
            reward = caught ? 1.0f : -1.0f;
            new_ball = true;
            if (--left == 0) {
                term = 1;
                left = a.balls;
                px = (W - a.g.pw) / 2;
                fill = true;
            }
        }
    }
    if (new_ball) {
        uint32_t r[4];
        sf_philox4x32_10((uint32_t)draw, 0u, 4u, 0u, seed, (uint32_t)(env0 + e), r);
        bx = (int)pc_mulhi(r[0], (uint32_t)(W - a.g.bs + 1));
        vx = (int)pc_mulhi(r[1], (uint32_t)(2 * a.g.vxm + 1)) - a.g.vxm;
        vy = 1 + (int)pc_mulhi(r[2], (uint32_t)a.g.vym);
        by = 0;
        ++draw;
    }
    const uint32_t cur = pc_pack(px, bx, by);
    uint32_t nh[PC_MAX_K + 1];
#pragma unroll
    for (int j = 0; j < PC_MAX_K; ++j) nh[j] = (fill || j + 1 >= k) ? cur : hist[j + 1 < PC_MAX_K ? j + 1 : j];
    nh[PC_MAX_K] = cur;

    extern __shared__ uint4 pc_plane[];  // DECOYS: the decoys of the episode's level as a plane of bytes, 255 or 0
    uint32_t *pc_map = reinterpret_cast<uint32_t *>(pc_plane);
    uint32_t level = 0u;
    if constexpr (DECOYS) {
        const int nw = pc_map_words(a.HW);
        for (int i = threadIdx.x; i < nw; i += PC_BLOCK) pc_map[i] = 0u;
        const uint32_t ep = (uint32_t)(draw - 1) / (uint32_t)a.balls;  // uniform, as the level is
        uint32_t r[4];
        sf_philox4x32_10(ep, 0u, PC_LANE_LEVEL, 0u, seed, (uint32_t)(env0 + e), r);
        level = a.start_level + (a.levels > 0 ? pc_mulhi(r[0], (uint32_t)a.levels) : r[0]);
    }
    __syncthreads();  // every lane holds the old state: now it may be replaced
    if constexpr (DECOYS) {
        uint8_t *map = reinterpret_cast<uint8_t *>(pc_map);
        const uint32_t ubs = (uint32_t)a.g.bs;
        for (uint32_t t = threadIdx.x; t < (uint32_t)a.decoys * ubs; t += PC_BLOCK) {  // lane d bs + i: row i of decoy d
            const uint32_t d = t / ubs, i = t - d * ubs;
            uint32_t r[4];
            sf_philox4x32_10(d, 0u, PC_LANE_DECOY, 0u, PC_LEVEL_KEY, level, r);
            const uint32_t dx = pc_mulhi(r[0], (uint32_t)(W - a.g.bs + 1)), dy = pc_mulhi(r[1], (uint32_t)a.g.D);
            const uint32_t q0 = (dy + i) * (uint32_t)W + dx;
            for (uint32_t q = q0; q < q0 + ubs; ++q) {
                map[q] = 255;
                if (q < 16u) map[(uint32_t)a.HW + q] = 255;  // the bytes a unit reads past the plane's end: the next plane's first
            }
        }
    }
    if (threadIdx.x == 0) {
        st[0] = draw; st[1] = left; st[2] = vx; st[3] = vy;
#pragma unroll
        for (int j = 0; j < PC_MAX_K; ++j)
            if (j < k) {
                st[PC_HDR + 3 * j] = (int32_t)(nh[j] & 1023u);
                st[PC_HDR + 3 * j + 1] = (int32_t)((nh[j] >> 10) & 1023u);
                st[PC_HDR + 3 * j + 2] = (int32_t)(nh[j] >> 20);
            }
        if (!reset) {
            rewards[e] = reward;
            terminated[e] = (uint8_t)term;
        }
    }

    if constexpr (DECOYS) __syncthreads();  // the decoy plane is complete

    // ---- render: plane after plane, a lane per store unit
    uint8_t *row = obs + (int64_t)e * pitch;
    const uint32_t HW = (uint32_t)a.HW, py = (uint32_t)(a.H - a.g.ph), bs = (uint32_t)a.g.bs;
    for (int j = 0; j < k; ++j) {
        uint32_t g0 = nh[0], g1 = nh[0];
#pragma unroll
        for (int i = 1; i <= PC_MAX_K; ++i) {
            g0 = j == i ? nh[i] : g0;
            g1 = j + 1 == i ? nh[i] : g1;
        }
        const uint32_t gby = g0 >> 20;
        const uint32_t base = (uint32_t)j * HW;                  // first byte of the plane in the env's row
        const uint32_t p_lo = (base + U - 1) / U, p_hi = (base + HW + U - 1) / U;  // units whose first byte is in the plane
        for (uint32_t p = p_lo + threadIdx.x; p < p_hi; p += PC_BLOCK) {
            const uint32_t L = p * U - base;
            const uint32_t y0 = fdiv(L, a.dW), x0 = L - y0 * (uint32_t)W;
            // row of the unit's last byte (GENERIC: any number of rows on; >= H: the unit runs into the next plane)
            const uint32_t y1 = GENERIC ? fdiv(L + U - 1, a.dW) : y0 + (x0 + U > (uint32_t)W ? 1u : 0u);
            uint32_t w[NW];
#pragma unroll
            for (int i = 0; i < NW; ++i) w[i] = 0;
            if (((y1 >= gby) & (y0 < gby + bs)) | (y1 >= py)) {
                if constexpr (GENERIC) pc_unit<NW>(w, x0, y0, g0, g1, a);
                else pc_unit16(w, x0, y0, g0, a);
            }
            if constexpr (DECOYS && GENERIC) {  // the decoy plane's bytes [L, L + U): aligned dwords, shifted by bytes
                const uint32_t *m = pc_map + (L >> 2);
#pragma unroll
                for (int i = 0; i < NW; ++i) w[i] |= __builtin_amdgcn_alignbyte(m[i + 1], m[i], L & 3u);
            } else if constexpr (DECOYS) {       // L is a multiple of 16 here
                const uint4 dv = pc_plane[L >> 4];
                w[0] |= dv.x; w[1] |= dv.y; w[2] |= dv.z; w[3] |= dv.w;
            }
            if constexpr (U == 16)
                *reinterpret_cast<uint4 *>(row + (size_t)p * 16) = make_uint4(w[0], w[1], w[2], w[3]);
            else
                *reinterpret_cast<uint32_t *>(row + (size_t)p * 4) = w[0];
        }
    }
}

int pc_launch(const char *name, int32_t *state, const int32_t *actions, uint8_t *obs, int64_t pitch, float *rewards,
              uint8_t *terminated, int N, int env0, uint32_t seed, int H, int W, int k, int balls, int reset, void *stream,
              int decoys = 0, int levels = 0, uint32_t start_level = 0) {
    SF_REQUIRE(state && obs, "%s: null state / obs_out", name);
    SF_REQUIRE(reset || (actions && rewards && terminated), "%s: null actions / rewards / terminated", name);
    SF_REQUIRE(N > 0, "%s: N = %d must be positive", name, N);
    SF_REQUIRE(k >= 1 && k <= PC_MAX_K, "%s: k = %d outside 1 .. %d", name, k, PC_MAX_K);
    SF_REQUIRE(balls >= 1, "%s: balls = %d must be at least 1", name, balls);
    const PcGeom g = pc_geom(H, W);
    SF_REQUIRE(g.ok, "%s: a %d x %d field is too small (or above %d) for ball and paddle", name, H, W, PC_MAX_SIDE);
    const int64_t bytes = (int64_t)k * H * W;
    SF_REQUIRE(pitch >= bytes, "%s: out_pitch %lld below k H W = %lld", name, (long long)pitch, (long long)bytes);
    const uintptr_t mis = (uintptr_t)obs | (uintptr_t)pitch | (uintptr_t)bytes;
    SF_REQUIRE((mis & 3) == 0, "%s: obs_out, out_pitch and k H W = %lld must all be multiples of 4 (16 for the wide stores)",
               name, (long long)bytes);
    SF_REQUIRE(decoys >= 0 && decoys <= PC_MAX_DECOYS, "%s: decoys = %d outside 0 .. %d", name, decoys, PC_MAX_DECOYS);
    SF_REQUIRE(levels >= 0, "%s: levels = %d must be 0 (unlimited) or positive", name, levels);
    const size_t lds = decoys > 0 ? (size_t)pc_map_words(H * W) * 4 : 0;
    SF_REQUIRE(lds <= (size_t)PC_MAX_MAP_BYTES, "%s: with decoys a %d x %d field needs %zu bytes of LDS, above %d",
               name, H, W, lds, PC_MAX_MAP_BYTES);
    PcArgs a;
    a.H = H; a.W = W; a.HW = H * W; a.k = k; a.balls = balls; a.g = g; a.dW = make_fastdiv((uint32_t)W);
    a.decoys = decoys; a.levels = levels; a.start_level = start_level;
    const bool wide = (mis & 15) == 0, rows16 = W >= 16 && a.HW % 16 == 0;  // 16-byte units of at most two rows of one plane
    const dim3 grid((unsigned)N), block(PC_BLOCK);
#define PC_GO(U, G, D) \
    k_pixcatch<U, G, D><<<grid, block, lds, STREAM(stream)>>>(state, actions, obs, pitch, rewards, terminated, N, env0, seed, a, reset)
#define PC_PICK(D) \
    do { \
        if (wide && rows16) PC_GO(16, false, D); \
        else if (wide) PC_GO(16, true, D); \
        else PC_GO(4, true, D); \
    } while (0)
    if (decoys > 0) PC_PICK(true);
    else PC_PICK(false);
#undef PC_PICK
#undef PC_GO
    return sf_launch_status(name);
}

}  // namespace

extern "C" int sf_pixcatch_state_words(int k) { return k >= 1 && k <= PC_MAX_K ? PC_HDR + 3 * k : SF_ERR_ARG; }

extern "C" int sf_pixcatch_reset(int32_t *state, uint8_t *obs_out, int64_t out_pitch, int N, int env0, uint32_t seed, int H,
                                 int W, int k, int balls, void *stream) {
    return pc_launch("sf_pixcatch_reset", state, nullptr, obs_out, out_pitch, nullptr, nullptr, N, env0, seed, H, W, k, balls,
                     1, stream);
}

extern "C" int sf_pixcatch_step(int32_t *state, const int32_t *actions, uint8_t *obs_out, int64_t out_pitch, float *rewards,
                                uint8_t *terminated, int N, int env0, uint32_t seed, int H, int W, int k, int balls,
                                void *stream) {
    return pc_launch("sf_pixcatch_step", state, actions, obs_out, out_pitch, rewards, terminated, N, env0, seed, H, W, k, balls,
                     0, stream);
}

extern "C" int sf_pixcatch_reset_levels(int32_t *state, uint8_t *obs_out, int64_t out_pitch, int N, int env0, uint32_t seed,
                                        int H, int W, int k, int balls, int decoys, int levels, uint32_t start_level,
                                        void *stream) {
    return pc_launch("sf_pixcatch_reset_levels", state, nullptr, obs_out, out_pitch, nullptr, nullptr, N, env0, seed, H, W, k,
                     balls, 1, stream, decoys, levels, start_level);
}

extern "C" int sf_pixcatch_step_levels(int32_t *state, const int32_t *actions, uint8_t *obs_out, int64_t out_pitch,
                                       float *rewards, uint8_t *terminated, int N, int env0, uint32_t seed, int H, int W, int k,
                                       int balls, int decoys, int levels, uint32_t start_level, void *stream) {
    return pc_launch("sf_pixcatch_step_levels", state, actions, obs_out, out_pitch, rewards, terminated, N, env0, seed, H, W, k,
                     balls, 0, stream, decoys, levels, start_level);
}
