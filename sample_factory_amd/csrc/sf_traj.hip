// Episode statistics an env defines itself (include/sf_hip.h: sf_episode_stats_add).
// The reference takes every per-agent tensor of a vectorised env's infos at the envs that finished and averages it on the
// host (batched_sampling.py:235-251, runner.py:263-278).  Here the sums stay on the device, next to ep_stats.
#include "sf_common.h"

#define STREAM(s) reinterpret_cast<hipStream_t>(s)

// element b of one channel as f64 (the dtype code is uniform over the launch: no divergence)
__device__ __forceinline__ double epstat_load(const void *p, int64_t stride, int dtype, int64_t b) {
    const int64_t i = b * stride;
    switch (dtype) {
        case SF_EPSTAT_F32: return (double)static_cast<const float *>(p)[i];
        case SF_EPSTAT_F64: return static_cast<const double *>(p)[i];
        case SF_EPSTAT_I32: return (double)static_cast<const int32_t *>(p)[i];
        case SF_EPSTAT_I64: return (double)static_cast<const int64_t *>(p)[i];
        default: return (double)static_cast<const uint8_t *>(p)[i];
    }
}

// one lane per env.  A wave without a finished env loads no channel and reduces nothing; the block's count is shared by
// its channels.  lds[w][k]: wave w's sum of channel k, lds[w][MAX]: its number of finished envs.
__global__ __launch_bounds__(256) void k_episode_stats_add(sf_epstat_channels ch, int K,
                                                           const uint8_t *__restrict__ terminated,
                                                           const uint8_t *__restrict__ truncated,
                                                           const uint8_t *__restrict__ active, int64_t B,
                                                           double *__restrict__ acc) {
    __shared__ double lds[4][SF_EPSTAT_MAX_CHANNELS + 1];
    const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool fin = false;
    if (b < B) {
        fin = (terminated[b] | truncated[b]) != 0;
        if (active) fin = fin && active[b] != 0;
    }
    const unsigned long long who = __ballot(fin);  // wave-uniform
    if (lane == 0) lds[wave][SF_EPSTAT_MAX_CHANNELS] = (double)__popcll(who);
    for (int k = 0; k < K; ++k) {
        double v = 0.0;
        if (who) {
            if (fin) v = epstat_load(ch.ptr[k], ch.stride[k], ch.dtype[k], b);
            v = sf_wave_sum(v);
        }
        if (lane == 0) lds[wave][k] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < K) {
        const int k = threadIdx.x, c = SF_EPSTAT_MAX_CHANNELS;
        const double n = lds[0][c] + lds[1][c] + lds[2][c] + lds[3][c];
        if (n > 0.0) {
            atomicAdd(&acc[2 * k], lds[0][k] + lds[1][k] + lds[2][k] + lds[3][k]);
            atomicAdd(&acc[2 * k + 1], n);
        }
    }
}

extern "C" int sf_episode_stats_add(const sf_epstat_channels *h_ch, int K, const uint8_t *terminated,
                                    const uint8_t *truncated, const uint8_t *active, int64_t B, double *acc,
                                    void *stream) {
    SF_REQUIRE(K >= 1 && K <= SF_EPSTAT_MAX_CHANNELS, "sf_episode_stats_add: K = %d outside 1 .. %d", K,
               SF_EPSTAT_MAX_CHANNELS);
    SF_REQUIRE(h_ch && terminated && truncated && acc, "sf_episode_stats_add: null pointer");
    SF_REQUIRE(B >= 0 && B <= (int64_t)0x7fffffff * 256, "sf_episode_stats_add: bad B");
    sf_epstat_channels ch = {};  // (channels beyond K travel as zeros, whatever the caller left there)
    for (int k = 0; k < K; ++k) {
        SF_REQUIRE(h_ch->ptr[k], "sf_episode_stats_add: channel %d: null pointer", k);
        SF_REQUIRE(h_ch->stride[k] >= 1, "sf_episode_stats_add: channel %d: stride < 1", k);
        SF_REQUIRE(h_ch->dtype[k] >= SF_EPSTAT_F32 && h_ch->dtype[k] <= SF_EPSTAT_U8,
                   "sf_episode_stats_add: channel %d: unknown dtype code %d", k, (int)h_ch->dtype[k]);
        ch.ptr[k] = h_ch->ptr[k];
        ch.stride[k] = h_ch->stride[k];
        ch.dtype[k] = h_ch->dtype[k];
    }
    if (B == 0) return SF_OK;
    k_episode_stats_add<<<dim3((unsigned)((B + 255) / 256)), dim3(256), 0, STREAM(stream)>>>(ch, K, terminated, truncated,
                                                                                            active, B, acc);
    return sf_launch_status("sf_episode_stats_add");
}
