// sf_rl.hip — the HBM/latency-bound part of the APPO hot path for gfx950 (MI355X):
// validity mask, GAE/returns scan, running-mean-std, V-trace, fused PPO loss fwd+bwd, minibatch index sets,
// grad-norm + Adam, action sampling, trajectory-step writes and the synthetic vector env.
// Reference op sequences replaced by each kernel are cited in include/sf_hip.h.
//
// Compiled with -ffp-contract=off: these kernels keep the reference's fp32 op order (torch CPU/GPU elementwise ops
// round after every op), so results match the oracle to the last bit wherever libm does.
#include "sf_common.h"

thread_local char sf_err_buf[512] = "";

extern "C" const char *sf_last_error(void) { return sf_err_buf; }
extern "C" int sf_abi_version(void) { return 19; }

#define STREAM(s) reinterpret_cast<hipStream_t>(s)

__device__ __forceinline__ float clampf(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }

// =========================================================================================== K13 validity mask
__global__ __launch_bounds__(256) void k_valid_mask(const int32_t *__restrict__ policy_id,
                                                    const float *__restrict__ policy_version,
                                                    uint8_t *__restrict__ valids, uint8_t *__restrict__ valids_flat,
                                                    float *__restrict__ actions,
                                                    int num_actions, float *__restrict__ logp, int E, int T,
                                                    int my_pid, int train_step, int max_lag,
                                                    int32_t *__restrict__ num_invalid) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t N = (int64_t)E * T;
    const bool in = i < N;
    bool valid = true;
    if (in) {
        const int64_t e = i / T;
        const int t = (int)(i - e * T);
        valid = (policy_id[i] == my_pid) && (((float)train_step - policy_version[i]) < (float)max_lag);
        valids[e * (T + 1) + t] = (uint8_t)valid;
        if (valids_flat) valids_flat[i] = (uint8_t)valid;  // the [E*T] dataset view (learner.py:1009-1012) without a compaction copy
        if (t == T - 1) valids[e * (T + 1) + T] = (uint8_t)valid;  // learner.py:955
        if (!valid) {
            for (int a = 0; a < num_actions; ++a) actions[i * num_actions + a] = 0.0f;
            logp[i] = -1.0f;
        }
    }
    const unsigned long long b = __ballot(in && !valid);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(num_invalid, (int32_t)__popcll(b));
}

extern "C" int sf_valid_mask(const int32_t *policy_id, const float *policy_version, uint8_t *valids,
                             uint8_t *valids_flat, float *actions, int num_actions, float *log_prob_actions, int E, int T,
                             int my_policy_id, int train_step, int max_policy_lag, int32_t *num_invalid, void *stream) {
    SF_REQUIRE(E > 0 && T > 0 && num_actions > 0, "sf_valid_mask: bad shape E=%d T=%d na=%d", E, T, num_actions);
    SF_REQUIRE(policy_id && policy_version && valids && actions && log_prob_actions && num_invalid,
               "sf_valid_mask: null pointer");
    int rc = sf_hip_status(hipMemsetAsync(num_invalid, 0, sizeof(int32_t), STREAM(stream)), "sf_valid_mask memset");
    if (rc) return rc;
    const int64_t N = (int64_t)E * T;
    k_valid_mask<<<dim3((unsigned)((N + 255) / 256)), dim3(256), 0, STREAM(stream)>>>(
        policy_id, policy_version, valids, valids_flat, actions, num_actions, log_prob_actions, E, T, my_policy_id,
        train_step, max_policy_lag, num_invalid);
    return sf_launch_status("sf_valid_mask");
}

// =========================================================================================== K10+K11 GAE / returns
// A 256-thread block owns 64 consecutive envs.  The env-major [E,T] rows are staged through LDS in [64 x 32]-step tiles
// (row stride 33 words -> the per-lane row walk of the scan is bank-conflict-free): all four waves issue the tile's
// loads as coalesced runs of consecutive words — every load of a tile is in flight before the first LDS write (the
// one-wave version waited for each load in turn: 330 serialised round trips, 68 us at (4096, 32)) — wave 0 runs the
// time recursion with one register per lane (= env) in the reference's op order, all four waves store the results.
constexpr int GAE_TC = 32;
constexpr int GAE_LD = GAE_TC + 1;
constexpr int GAE_NT = 256;
constexpr int GAE_IT = (64 * GAE_LD + GAE_NT - 1) / GAE_NT;  // loads per thread and array: 9

struct GaeTile {
    float v[GAE_IT];
};
__device__ __forceinline__ GaeTile gae_fetch_f32(const float *g, int64_t row_stride, int e0, int E, int t0, int ncols,
                                                 int tid) {
    GaeTile r;
#pragma unroll
    for (int i = 0; i < GAE_IT; ++i) {
        const int idx = i * GAE_NT + tid;
        const int row = idx / ncols, col = idx - row * ncols;
        const int e = e0 + row;
        const bool ok = row < 64 && e < E;
        const float x = g[ok ? (int64_t)e * row_stride + t0 + col : 0];  // branch-free: clamped address, late select
        r.v[i] = ok ? x : 0.0f;
    }
    return r;
}
__device__ __forceinline__ GaeTile gae_fetch_u8(const uint8_t *g, int64_t row_stride, int e0, int E, int t0, int ncols,
                                                int tid) {
    GaeTile r;
#pragma unroll
    for (int i = 0; i < GAE_IT; ++i) {
        const int idx = i * GAE_NT + tid;
        const int row = idx / ncols, col = idx - row * ncols;
        const int e = e0 + row;
        const bool ok = row < 64 && e < E;
        const uint8_t x = g[ok ? (int64_t)e * row_stride + t0 + col : 0];
        r.v[i] = (ok && x) ? 1.0f : 0.0f;
    }
    return r;
}
__device__ __forceinline__ void gae_put(float (*s)[GAE_LD], const GaeTile &r, int ncols, int tid) {
#pragma unroll
    for (int i = 0; i < GAE_IT; ++i) {
        const int idx = i * GAE_NT + tid;
        const int row = idx / ncols, col = idx - row * ncols;
        if (row < 64) s[row][col] = r.v[i];
    }
}
__device__ __forceinline__ void gae_tile_store_f32(const float (*s)[GAE_LD], float *g, int64_t row_stride, int e0,
                                                   int E, int t0, int ncols, int tid) {
#pragma unroll
    for (int i = 0; i < GAE_IT; ++i) {
        const int idx = i * GAE_NT + tid;
        const int row = idx / ncols, col = idx - row * ncols;
        const int e = e0 + row;
        if (row < 64 && e < E) g[(int64_t)e * row_stride + t0 + col] = s[row][col];
    }
}

__global__ __launch_bounds__(GAE_NT) void k_gae_returns(float *__restrict__ rewards, const uint8_t *__restrict__ dones,
                                                        const uint8_t *__restrict__ time_outs,
                                                        const float *__restrict__ values,
                                                        const uint8_t *__restrict__ valids,
                                                        const double *__restrict__ rms_stats, int E, int T, float gamma,
                                                        float gl, int value_bootstrap, float *__restrict__ adv_out,
                                                        float *__restrict__ ret_out) {
    __shared__ float s_r[64][GAE_LD], s_v[64][GAE_LD], s_d[64][GAE_LD], s_to[64][GAE_LD], s_va[64][GAE_LD],
        s_adv[64][GAE_LD], s_ret[64][GAE_LD];
    const int tid = threadIdx.x, lane = tid;  // the scan runs on wave 0: lane == tid < 64
    const int e0 = blockIdx.x * 64;
    const bool denorm = rms_stats != nullptr;
    float mu = 0.f, sigma = 1.f;
    if (denorm) {
        mu = (float)rms_stats[0];
        sigma = sqrtf((float)rms_stats[1] + 1e-5f);
    }
    float cum = 0.0f;
    for (int t0 = ((T - 1) / GAE_TC) * GAE_TC; t0 >= 0; t0 -= GAE_TC) {
        const int tc = min(GAE_TC, T - t0);
        // every load of the tile is issued before the first LDS write
        const GaeTile fr = gae_fetch_f32(rewards, T, e0, E, t0, tc, tid);
        const GaeTile fd = gae_fetch_u8(dones, T, e0, E, t0, tc, tid);
        const GaeTile fv = gae_fetch_f32(values, T + 1, e0, E, t0, tc + 1, tid);
        const GaeTile fa = gae_fetch_u8(valids, T + 1, e0, E, t0, tc + 1, tid);
        GaeTile ft;
        if (value_bootstrap) ft = gae_fetch_u8(time_outs, T, e0, E, t0, tc, tid);
        __syncthreads();  // the previous tile's stores have read s_adv / s_ret / s_r
        gae_put(s_r, fr, tc, tid);
        gae_put(s_d, fd, tc, tid);
        gae_put(s_v, fv, tc + 1, tid);
        gae_put(s_va, fa, tc + 1, tid);
        if (value_bootstrap) gae_put(s_to, ft, tc, tid);
        __syncthreads();
        if (tid < 64) {
            // per-lane backward scan over this tile (lane = env)
            for (int c = tc; c >= 0; --c) {  // de-normalise the values of this row first (learner.py:969-979)
                float v = s_v[lane][c];
                if (denorm) v = clampf(v, -5.0f, 5.0f) * sigma + mu;
                s_v[lane][c] = v;
            }
            for (int c = tc - 1; c >= 0; --c) {
                const float v = s_v[lane][c], vn = s_v[lane][c + 1];
                const float valid = s_va[lane][c], valid_n = s_va[lane][c + 1];
                const float done = s_d[lane][c];
                float r = s_r[lane][c];
                if (value_bootstrap) {  // learner.py:990
                    r = r + ((gamma * v) * s_to[lane][c]) * done;
                    s_r[lane][c] = r;
                }
                const float a = (r - v) * valid;
                const float b = (1.0f - done) * ((gamma * vn) * valid_n);
                const float delta = a + b;
                const float disc = gl * valid + (1.0f - valid);
                cum = delta + (disc * cum) * (1.0f - done);
                s_adv[lane][c] = cum;
                s_ret[lane][c] = cum + valid * v;  // learner.py:1003
            }
        }
        __syncthreads();
        gae_tile_store_f32(s_adv, adv_out, T, e0, E, t0, tc, tid);
        gae_tile_store_f32(s_ret, ret_out, T, e0, E, t0, tc, tid);
        if (value_bootstrap) gae_tile_store_f32(s_r, rewards, T, e0, E, t0, tc, tid);
    }
}

extern "C" int sf_gae_returns(float *rewards, const uint8_t *dones, const uint8_t *time_outs, const float *values,
                              const uint8_t *valids, const double *rms_stats, int E, int T, float gamma,
                              float gae_lambda, int value_bootstrap, float *advantages, float *returns,
                              void *stream) {
    SF_REQUIRE(E > 0 && T > 0, "sf_gae_returns: bad shape E=%d T=%d", E, T);
    SF_REQUIRE(rewards && dones && values && valids && advantages && returns, "sf_gae_returns: null pointer");
    SF_REQUIRE(!value_bootstrap || time_outs, "sf_gae_returns: value_bootstrap needs time_outs");
    // the reference multiplies the python doubles gamma*lambda before the cast to f32 (rl_utils.py:90)
    const float gl = (float)((double)gamma * (double)gae_lambda);
    k_gae_returns<<<dim3((unsigned)((E + 63) / 64)), dim3(GAE_NT), 0, STREAM(stream)>>>(
        rewards, dones, time_outs, values, valids, rms_stats, E, T, gamma, gl, value_bootstrap, advantages, returns);
    return sf_launch_status("sf_gae_returns");
}

// =========================================================================================== K12 running mean/std
__global__ __launch_bounds__(256) void k_moments(const float *__restrict__ x, const uint8_t *__restrict__ valids,
                                                 const int32_t *__restrict__ index, int64_t offset, int64_t n,
                                                 int dense_x, double *__restrict__ moments) {
    __shared__ double lds[4 * 3];
    double acc[3] = {0.0, 0.0, 0.0};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = index ? (int64_t)index[i] : offset + i;
        if (!valids || valids[j]) {
            const double v = (double)x[dense_x ? i : j];
            acc[0] += v;
            acc[1] += v * v;
            acc[2] += 1.0;
        }
    }
    sf_block_sum<3>(acc, lds);
    if (threadIdx.x == 0) {
        atomicAdd(&moments[0], acc[0]);
        atomicAdd(&moments[1], acc[1]);
        atomicAdd(&moments[2], acc[2]);
    }
}

extern "C" int sf_moments(const float *x, const uint8_t *valids, const int32_t *index, int64_t offset, int64_t n,
                          int dense_x, double *moments, void *stream) {
    SF_REQUIRE(x && moments && n >= 0 && offset >= 0, "sf_moments: bad args");
    int rc = sf_hip_status(hipMemsetAsync(moments, 0, 3 * sizeof(double), STREAM(stream)), "sf_moments memset");
    if (rc || n == 0) return rc;
    // latency-bound at minibatch sizes (32768 elements = 164 KB): one element per thread and one round trip, not an
    // 8-deep dependent loop on 16 CUs; large inputs grid-stride over 2048 blocks (8 per CU)
    const int64_t blocks = (n + 255) / 256;
    k_moments<<<dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, STREAM(stream)>>>(
        x, valids, index, offset, n, dense_x, moments);
    return sf_launch_status("sf_moments");
}

__global__ void k_rms_update(const double *__restrict__ stats_in, const double *__restrict__ moments,
                             double *__restrict__ stats_out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const double n = moments[2];
    const double mean = stats_in[0], var = stats_in[1], count = stats_in[2];
    if (n <= 0.0) { stats_out[0] = mean; stats_out[1] = var; stats_out[2] = count; return; }
    // batch mean / unbiased variance are fp32 tensors in the reference (x.mean(), x.var()) -> round to f32
    const double bm64 = moments[0] / n;
    const double bv64 = (moments[1] - moments[0] * bm64) / (n - 1.0);
    const double batch_mean = (double)(float)bm64, batch_var = (double)(float)bv64;
    const double delta = batch_mean - mean;
    const double tot = count + n;
    const double new_mean = mean + delta * n / tot;
    const double M2 = var * count + batch_var * n + (delta * delta) * count * n / tot;
    stats_out[0] = new_mean;
    stats_out[1] = M2 / tot;
    stats_out[2] = tot;
}

extern "C" int sf_rms_update(const double *stats_in, const double *moments, double *stats_out, void *stream) {
    SF_REQUIRE(stats_in && moments && stats_out, "sf_rms_update: null pointer");
    k_rms_update<<<dim3(1), dim3(64), 0, STREAM(stream)>>>(stats_in, moments, stats_out);
    return sf_launch_status("sf_rms_update");
}

__global__ __launch_bounds__(256) void k_rms_apply(float *__restrict__ x, int64_t n,
                                                   const double *__restrict__ stats, int denormalize) {
    const float mu = (float)stats[0];
    const float sigma = sqrtf((float)stats[1] + 1e-5f);
    const float inv = 1.0f / sigma;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        // torch.clamp hands a NaN on (a one-sample batch has no unbiased variance: NaN statistics); fminf / fmaxf drop it
        const float u = denormalize ? x[i] : (x[i] - mu) * inv;
        const float c = (u != u) ? u : clampf(u, -5.0f, 5.0f);
        x[i] = denormalize ? c * sigma + mu : c;
    }
}

extern "C" int sf_rms_apply(float *x, int64_t n, const double *stats, int denormalize, void *stream) {
    SF_REQUIRE(x && stats && n >= 0, "sf_rms_apply: bad args");
    if (n == 0) return SF_OK;
    const int64_t blocks = (n + 255) / 256;
    k_rms_apply<<<dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, STREAM(stream)>>>(x, n, stats,
                                                                                                   denormalize);
    return sf_launch_status("sf_rms_apply");
}

// =========================================================================================== action distributions
// The arithmetic of one column of a member, shared by V-trace, the PPO loss and the samplers.  Every
// helper is inlined and keeps one operation order, so all its callers round alike; the column loop stays in the caller:
// a lane-per-row kernel walks k = 0 .. D, a wave-per-row kernel k = lane, lane + 64, .. and sums over the wave after.
struct HeadsDev {
    int num_heads, head_n[SF_MAX_ACTION_HEADS];  // a kernel argument (260 bytes); the launchers check num_heads
};
struct LossDev {
    float clip_lo, clip_hi, clip_value, value_coeff, expl_coeff, kl_coeff;
    int expl_kind, action_kind, dense_adv;
    HeadsDev hd;
    int ov_T;  // > 0: old_values is the slab's [E, ov_T + 1] array read in place (dataset row e*T+t -> e*(T+1)+t)
};
constexpr float HALF_LOG_2PI = 0.91893853320467274178f;

// Box(D) member, parameters [means | log_std]: the standard deviation of a column, the Normal log-density of an action
__device__ __forceinline__ float box_sd(float zlog) { return clampf(expf(zlog), 1e-4f, 1e4f); }
__device__ __forceinline__ float box_logp(float a, float mu, float sd) {
    return -((a - mu) * (a - mu)) / (2.f * (sd * sd)) - logf(sd) - HALF_LOG_2PI;
}
// column k of a Box(D) member in the loss: adds its log-prob, entropy and KL(current || old) to the three sums
__device__ __forceinline__ void box_loss_terms(const float *__restrict__ z, const float *__restrict__ zo,
                                               const float *__restrict__ act, int D, int k, float &lp, float &ent,
                                               float &kl) {
    const float mu = z[k], sd = box_sd(z[D + k]);
    lp += box_logp(act[k], mu, sd);
    ent += 0.5f + HALF_LOG_2PI + logf(sd);
    const float muo = zo[k], sdo = box_sd(zo[D + k]);
    const float vr = (sd / sdo) * (sd / sdo);
    const float t1 = ((mu - muo) / sdo) * ((mu - muo) / sdo);
    kl += 0.5f * (vr + t1 - 1.f - logf(vr));
}
// ... and its gradient: gz[k] (mean) and gz[D + k] (log_std; zero where exp(log_std) is beyond the clamp)
__device__ __forceinline__ void box_grad(const float *__restrict__ z, const float *__restrict__ zo,
                                         const float *__restrict__ act, int D, int k, float dL_dlogp, float inv_n,
                                         const LossDev &h, float *__restrict__ gz) {
    const float mu = z[k], e = expf(z[D + k]);
    const float sd = clampf(e, 1e-4f, 1e4f);
    const float dsd = (e >= 1e-4f && e <= 1e4f) ? e : 0.f;
    const float a = act[k];
    const float var = sd * sd;
    float gmu = dL_dlogp * ((a - mu) / var);
    float gsd = dL_dlogp * (((a - mu) * (a - mu)) / (var * sd) - 1.f / sd);
    if (h.expl_kind == 1) gsd += -h.expl_coeff * inv_n * (1.f / sd);
    if (h.kl_coeff != 0.f) {
        const float muo = zo[k], sdo = box_sd(zo[D + k]);
        gmu += h.kl_coeff * inv_n * ((mu - muo) / (sdo * sdo));
        gsd += h.kl_coeff * inv_n * (sd / (sdo * sdo) - 1.f / sd);
    }
    gz[k] = gmu;
    gz[D + k] = gsd * dsd;
}
// the standard normal a sampler draws for column k of Box member h: Box-Muller on Philox counter (step, k / 2, 3, h),
// two columns per counter
__device__ __forceinline__ float box_eps(uint32_t step, int k, int h, uint32_t seed, uint32_t row) {
    uint32_t w[4];
    sf_philox4x32_10(step, (uint32_t)(k >> 1), 3u, (uint32_t)h, seed, row, w);
    const uint32_t w1 = (k & 1) ? w[2] : w[0], w2 = (k & 1) ? w[3] : w[1];
    const float u1 = ((float)(w1 >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float u2 = (float)(w2 >> 8) * (1.0f / 16777216.0f);
    return sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}
// the uniform in [0, 1) a sampler draws Discrete member h from: Philox counter (step, h, 2, 0)
__device__ __forceinline__ float cat_uniform(uint32_t step, int h, uint32_t seed, uint32_t row) {
    uint32_t w[4];
    sf_philox4x32_10(step, (uint32_t)h, 2u, 0u, seed, row, w);
    return (float)(w[0] >> 8) * (1.0f / 16777216.0f);
}

// Discrete(nh) member read in place, one lane per row: maximum and log-sum-exp of its logits
__device__ __forceinline__ void cat_lse(const float *__restrict__ z, int nh, float &mx, float &lse) {
    mx = -INFINITY;
    for (int k = 0; k < nh; ++k) mx = fmaxf(mx, z[k]);
    float se = 0.f;
    for (int k = 0; k < nh; ++k) se += expf(z[k] - mx);
    lse = logf(se);
}
// Discrete(nh) member in the loss, one lane per row: softmax statistics of the current and the old logits, entropy, KL,
// KL(p || uniform) (klpu), its mirror sum u * (lu - lp) (a2) and the log-prob of `act` (lpa)
struct CatTerms {
    float mx, lse, mxo, lseo, ent, kl, klpu, a2, lpa;
};
__device__ __forceinline__ CatTerms cat_terms(const float *__restrict__ z, const float *__restrict__ zo, int nh, int act) {
    CatTerms t;
    float m1 = -INFINITY, m2 = -INFINITY;
    for (int k = 0; k < nh; ++k) { m1 = fmaxf(m1, z[k]); m2 = fmaxf(m2, zo[k]); }
    float s1 = 0.f, s2 = 0.f;
    for (int k = 0; k < nh; ++k) { s1 += expf(z[k] - m1); s2 += expf(zo[k] - m2); }
    t.mx = m1; t.lse = logf(s1); t.mxo = m2; t.lseo = logf(s2);
    const float u = 1.0f / (float)nh, lu = logf(u);
    float lpa = 0.f, e = 0.f, kk = 0.f, a1 = 0.f, a2 = 0.f;
    for (int k = 0; k < nh; ++k) {
        const float lp = (z[k] - m1) - t.lse, p = expf(lp), q = (zo[k] - m2) - t.lseo;
        if (k == act) lpa = lp;
        e -= p * lp;
        kk += p * (lp - q);
        a1 += p * (lp - lu);
        a2 += u * (lu - lp);
    }
    t.ent = e; t.kl = kk; t.klpu = a1; t.a2 = a2; t.lpa = lpa;
    return t;
}
// gradient of one column of a Discrete(nh) member (zk / zok: its current and old logit, the old one read only when the
// KL term is on; taken: it is the recorded action; u = 1 / nh, lu = log u), from the member's seven statistics
__device__ __forceinline__ float cat_grad(float zk, float zok, bool taken, float mx, float lse, float mxo, float lseo,
                                          float ent, float kl, float klpu, float u, float lu, float dL_dlogp, float inv_n,
                                          float symkl_gate, const LossDev &h) {
    const float lp = (zk - mx) - lse, p = expf(lp), q = (zok - mxo) - lseo;
    float gk = dL_dlogp * ((taken ? 1.f : 0.f) - p);
    if (h.expl_kind == 1) gk += h.expl_coeff * inv_n * (p * (lp + ent));
    if (h.expl_kind == 2) gk += symkl_gate * h.expl_coeff * inv_n * 0.5f * (p * ((lp - lu) - klpu) + p - u);
    if (h.kl_coeff != 0.f) gk += h.kl_coeff * inv_n * (p * ((lp - q) - kl));
    return gk;
}

// Discrete(A), A <= MAXA, held in registers: the row into zz (-inf beyond A), its maximum and log-sum-exp.  MAXA bounds
// the unrolled loops, so no array is indexed dynamically.
template <int MAXA>
__device__ __forceinline__ void reg_softmax(const float *__restrict__ z, int A, float (&zz)[MAXA], float &mx, float &lse) {
    mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < MAXA; ++k) { zz[k] = k < A ? z[k] : -INFINITY; mx = fmaxf(mx, zz[k]); }
    float se = 0.f;
#pragma unroll
    for (int k = 0; k < MAXA; ++k) if (k < A) se += expf(zz[k] - mx);
    lse = logf(se);
}

// Discrete(n) under an action mask (the rule above k_sample_write_masked), one lane per row: softmax statistics of the
// logits with -1e9 on the masked-out columns, the allowed probability mass, 1 / (mass + 1e-13) and the total of the
// weights masked_p gives (multinomial normalises its weights)
struct MaskedStats {
    float mx, lse, psum, inv, tot;
    bool all_zero;
};
__device__ __forceinline__ MaskedStats masked_stats(const float *__restrict__ z, const uint8_t *__restrict__ mk, int n) {
    MaskedStats s;
    s.mx = -INFINITY;
    for (int k = 0; k < n; ++k) s.mx = fmaxf(s.mx, z[k] + (mk[k] ? 0.f : -1e9f));
    float se = 0.f;
    for (int k = 0; k < n; ++k) se += expf((z[k] + (mk[k] ? 0.f : -1e9f)) - s.mx);
    s.lse = logf(se);
    s.psum = 0.f;
    for (int k = 0; k < n; ++k) s.psum += mk[k] ? expf((z[k] - s.mx) - s.lse) : 0.f;
    s.all_zero = s.psum == 0.f;
    s.inv = 1.0f / (s.psum + 1e-13f);
    s.tot = s.all_zero ? (float)n * 1e-6f : s.psum * s.inv;
    return s;
}
// weight of a column before multinomial's normalisation (an all-masked member: n weights of 1e-6), and its log-prob
__device__ __forceinline__ float masked_p(const MaskedStats &s, float zk, uint8_t allowed) {
    return s.all_zero ? 1e-6f : (allowed ? expf((zk - s.mx) - s.lse) * s.inv : 0.f);
}
__device__ __forceinline__ float masked_logp(const MaskedStats &s, float zk, uint8_t allowed) {
    return ((zk + (allowed ? 0.f : -1e9f)) - s.mx) - s.lse;
}
// Training under the mask: the reference's `probs` of a column, softmax * mask / (sum + 1e-13).  The
// 1e-6 weights of masked_p are the sampler's multinomial guard and no part of the loss: an all-zero slice has p = 0.
__device__ __forceinline__ float masked_prob(const MaskedStats &s, float zk, uint8_t allowed) {
    return allowed ? expf((zk - s.mx) - s.lse) * s.inv : 0.f;
}
// a mask row of dataset row d: the slab's [E, mask_T + 1, A] array read in place (mask_T > 0, the mapping of ov_row),
// or the flat [N, ldm] array
__device__ __forceinline__ const uint8_t *mask_row(const uint8_t *__restrict__ mask, int64_t ldm, int mask_T, int64_t d) {
    return mask + (mask_T > 0 ? d + d / mask_T : d) * ldm;
}
// Discrete(nh) member in the masked loss, one lane per row (cat_terms under a mask; no symmetric-KL terms: the masked
// entry points refuse that loss): statistics of the current and of the old logits under the SAME mask slice, entropy
// -sum p lp, KL sum p (lp - lp_old) and the log-prob of `act`
struct MaskedCatTerms {
    MaskedStats s, so;
    float ent, kl, lpa;
};
__device__ __forceinline__ MaskedCatTerms masked_cat_terms(const float *__restrict__ z, const float *__restrict__ zo,
                                                           const uint8_t *__restrict__ mk, int nh, int act) {
    MaskedCatTerms t;
    t.s = masked_stats(z, mk, nh);
    t.so = masked_stats(zo, mk, nh);
    float lpa = 0.f, e = 0.f, kk = 0.f;
    for (int k = 0; k < nh; ++k) {
        const float lp = masked_logp(t.s, z[k], mk[k]), p = masked_prob(t.s, z[k], mk[k]);
        const float q = masked_logp(t.so, zo[k], mk[k]);
        if (k == act) lpa = lp;
        e -= p * lp;
        kk += p * (lp - q);
    }
    t.ent = e; t.kl = kk; t.lpa = lpa;
    return t;
}
// gradient of one column of a masked Discrete member: d logp_a / dz_k = delta_ak - exp(lp_k) on every column (exp(-1e9)
// is 0: exactly zero on a masked-out column of a slice that allows something, delta - 1 / n on an all-zero slice); the
// entropy and KL terms carry p_k and vanish with it
__device__ __forceinline__ float masked_cat_grad(float zk, float zok, uint8_t allowed, bool taken, float mx, float lse,
                                                 float inv, float mxo, float lseo, float ent, float kl, float dL_dlogp,
                                                 float inv_n, const LossDev &h) {
    const float off = allowed ? 0.f : -1e9f;
    const float lp = ((zk + off) - mx) - lse, q = ((zok + off) - mxo) - lseo;
    const float p = allowed ? expf((zk - mx) - lse) * inv : 0.f;
    float gk = dL_dlogp * ((taken ? 1.f : 0.f) - expf(lp));
    if (h.expl_kind == 1) gk += h.expl_coeff * inv_n * (p * (lp + ent));
    if (h.kl_coeff != 0.f) gk += h.kl_coeff * inv_n * (p * ((lp - q) - kl));
    return gk;
}

// log-prob of the taken action under the current policy, for one sample (used by v-trace and the loss head).
template <int MAXA>
__device__ __forceinline__ float action_logp(const float *__restrict__ z, int A, int action_kind,
                                             const float *__restrict__ act_row) {
    if (action_kind == 0) {
        float zz[MAXA], mx, lse;
        reg_softmax<MAXA>(z, A, zz, mx, lse);
        const int a = (int)act_row[0];
        float r = 0.f;
#pragma unroll
        for (int k = 0; k < MAXA; ++k) if (k == a) r = (zz[k] - mx) - lse;
        return r;
    } else {
        const int D = A / 2;
        float r = 0.f;
        for (int k = 0; k < D; ++k) r += box_logp(act_row[k], z[k], box_sd(z[D + k]));
        return r;
    }
}

// =========================================================================================== K17 V-trace
// A head list as the entry points receive it (host array): 1 .. cap members, none empty.  Fills `out`, returns the number
// of parameters the members read, or -1 with the reason in sf_err_buf (`what` names the entry point).  Nothing is
// launched with a list this has not passed: the kernels index head_n with num_heads unchecked.
static int heads_from_host(const char *what, const int32_t *head_n, int num_heads, int cap, int *out_n, bool *any_box) {
    if (!head_n || num_heads < 1 || num_heads > cap) {
        snprintf(sf_err_buf, sizeof(sf_err_buf), "%s: %d action heads, the limit is %d%s", what, num_heads, cap,
                 cap < SF_MAX_ACTION_HEADS ? " members in sf_loss_cfg (sf_ppo_loss_heads takes a longer list)"
                                          : " (SF_MAX_ACTION_HEADS)");
        return -1;
    }
    int tot = 0;
    *any_box = false;
    for (int i = 0; i < num_heads; ++i) {  // head_n > 0: Discrete(n), n logits; < 0: Box(-n), 2 * (-n) parameters
        if (head_n[i] == 0) {
            snprintf(sf_err_buf, sizeof(sf_err_buf), "%s: empty action head (member %d of %d)", what, i, num_heads);
            return -1;
        }
        out_n[i] = head_n[i];
        tot += head_n[i] > 0 ? head_n[i] : -2 * head_n[i];
        *any_box = *any_box || head_n[i] < 0;
    }
    for (int i = num_heads; i < SF_MAX_ACTION_HEADS; ++i) out_n[i] = 0;
    return tot;
}
// action columns of a Tuple space: one per Discrete member (head_n > 0), D per Box(D) member (head_n = -D)
__device__ __host__ __forceinline__ int heads_action_cols(const int *head_n, int num_heads) {
    int c = 0;
    for (int h = 0; h < num_heads; ++h) c += head_n[h] > 0 ? 1 : -head_n[h];
    return c;
}
static bool heads_any_discrete(const HeadsDev &hd) {
    for (int h = 0; h < hd.num_heads; ++h) if (hd.head_n[h] > 0) return true;
    return false;
}
// log-prob of a Tuple action: sum over the members of log_softmax(z_h)[a_h] (Discrete) / Normal log-density (Box, head_n = -D)
// MASKED: a Discrete member's log-prob is the masked log-softmax on its slice of the mask row mk
template <bool MASKED>
__device__ __forceinline__ float tuple_logp(const float *__restrict__ z, const float *__restrict__ act, const HeadsDev &hd,
                                            const uint8_t *__restrict__ mk) {
    float lp = 0.f;
    int off = 0, aoff = 0;
    for (int h = 0; h < hd.num_heads; ++h) {
        const int nh = hd.head_n[h];
        if (nh < 0) {
            const int D = -nh;
            for (int k = 0; k < D; ++k) lp += box_logp(act[aoff + k], z[off + k], box_sd(z[off + D + k]));
            off += 2 * D; aoff += D;
            continue;
        }
        if constexpr (MASKED) {
            const MaskedStats ms = masked_stats(z + off, mk + off, nh);
            const int a = min(max((int)act[aoff], 0), nh - 1);  // (a recorded action is in range; never read past the slice)
            lp += masked_logp(ms, z[off + a], mk[off + a]);
        } else {
            float mx, lse;
            cat_lse(z + off, nh, mx, lse);
            lp += (z[off + (int)act[aoff]] - mx) - lse;
        }
        off += nh; aoff += 1;
    }
    return lp;
}

// ------------------------------------------------------------------------------------------- wide family (A > 128)
// One wave64 per sample row, four rows per 256-thread block; the lanes stride the columns of a head, so one load
// instruction covers 256 contiguous bytes and nothing per-column is kept in a lane.  A row is read from HBM once (the
// statistics pass); the terms and gradient passes read it again from cache.  Rows start at column 1 of the heads
// matrix, so only 4-byte alignment is assumed: every access is a dword.  Reductions are xor butterflies, which leave
// the same bits in every lane (a + b == b + a), so the branches taken on them are wave-uniform.
constexpr int WIDE_MIN_A = 129;   // A <= 128: the lane-per-sample kernels, untouched
constexpr int WIDE_ROWS = 4;      // waves (= rows) per block

__device__ __forceinline__ float wide_allsum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ float wide_allmax(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ int wide_allmin(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    return v;
}
// one step of a lane's running (max, sum of exp(x - max)): one expf per element
__device__ __forceinline__ void wide_push(float &m, float &s, float x) {
    const float e = expf(-fabsf(x - m));  // m = -inf before the first element: e = 0, s = 0 * 0 + 1
    s = x > m ? s * e + 1.f : s + e;
    m = fmaxf(m, x);
}
// the lanes' running pairs -> max and log-sum-exp of the head, in every lane (a lane that saw no column has m = -inf,
// s = 0 and adds 0)
__device__ __forceinline__ void wide_finish(float m, float s, float &mx, float &lse) {
    mx = wide_allmax(m);
    lse = logf(wide_allsum(s * expf(m - mx)));
}
// max and log-sum-exp over nh columns of z (masked-out columns count as z - 1e9, the rule above k_sample_write_masked)
__device__ __forceinline__ void wide_lse(const float *__restrict__ z, int nh, int lane, const uint8_t *__restrict__ mk,
                                         float &mx, float &lse) {
    float m = -INFINITY, s = 0.f;
    // (unroll 4: four independent loads in flight per lane; these loops wait on memory, not on the ALU)
    if (mk) {
#pragma unroll 4
        for (int k = lane; k < nh; k += 64) wide_push(m, s, z[k] + (mk[k] ? 0.f : -1e9f));
    } else {
#pragma unroll 4
        for (int k = lane; k < nh; k += 64) wide_push(m, s, z[k]);
    }
    wide_finish(m, s, mx, lse);
}
// a single Discrete(A) / Box(A / 2) as a one-member head list
static HeadsDev single_head(int A, int action_kind) {
    HeadsDev hd = {};
    hd.num_heads = 1;
    hd.head_n[0] = action_kind == 0 ? A : -(A / 2);
    return hd;
}

// k_vtrace_ratio for A > 128: log-prob of the taken action, one wave per row.  MASKED: a Discrete member's log-sum-exp
// runs under its slice of the row's mask (wide_lse's rule), and so does the taken action's log-prob.
template <bool MASKED>
__device__ __forceinline__ void vtrace_ratio_wide(const float *__restrict__ params, int ldp,
                                                  const float *__restrict__ actions, const float *__restrict__ old_logp,
                                                  const int32_t *__restrict__ index, int64_t offset, int64_t n,
                                                  float *__restrict__ ratio_out, const HeadsDev &hd,
                                                  const uint8_t *__restrict__ mask, int64_t ldm, int mask_T) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t k = (int64_t)blockIdx.x * WIDE_ROWS + wave;
    if (k >= n) return;
    const int nact = heads_action_cols(hd.head_n, hd.num_heads);
    const int64_t d = index ? (int64_t)index[k] : offset + k;
    const float *z = params + k * ldp, *act = actions + d * nact;
    float lp = 0.f;
    int off = 0, aoff = 0;
    for (int h = 0; h < hd.num_heads; ++h) {
        const int nh = hd.head_n[h];
        if (nh < 0) {
            const int D = -nh;
            float r = 0.f;
            for (int j = lane; j < D; j += 64) r += box_logp(act[aoff + j], z[off + j], box_sd(z[off + D + j]));
            lp += wide_allsum(r);
            off += 2 * D; aoff += D;
            continue;
        }
        float mx, lse;
        if constexpr (MASKED) {
            const uint8_t *mk = mask_row(mask, ldm, mask_T, d) + off;
            wide_lse(z + off, nh, lane, mk, mx, lse);
            const int a = min(max((int)act[aoff], 0), nh - 1);
            lp += ((z[off + a] + (mk[a] ? 0.f : -1e9f)) - mx) - lse;
        } else {
            wide_lse(z + off, nh, lane, nullptr, mx, lse);
            const int a = min(max((int)act[aoff], 0), nh - 1);  // (a recorded action is in range; never read past the row)
            lp += (z[off + a] - mx) - lse;
        }
        off += nh; aoff += 1;
    }
    if (lane == 0) ratio_out[k] = clampf(expf(lp - old_logp[d]), 0.05f, 20.0f);
}

__global__ __launch_bounds__(256) void k_vtrace_ratio_wide(const float *__restrict__ params, int ldp,
                                                           const float *__restrict__ actions,
                                                           const float *__restrict__ old_logp,
                                                           const int32_t *__restrict__ index, int64_t offset, int64_t n,
                                                           float *__restrict__ ratio_out, HeadsDev hd) {
    vtrace_ratio_wide<false>(params, ldp, actions, old_logp, index, offset, n, ratio_out, hd, nullptr, 0, 0);
}

__global__ __launch_bounds__(256) void k_masked_vtrace_ratio_wide(const float *__restrict__ params, int ldp,
                                                                  const float *__restrict__ actions,
                                                                  const float *__restrict__ old_logp,
                                                                  const int32_t *__restrict__ index, int64_t offset,
                                                                  int64_t n, float *__restrict__ ratio_out, HeadsDev hd,
                                                                  const uint8_t *__restrict__ mask, int64_t ldm,
                                                                  int mask_T) {
    vtrace_ratio_wide<true>(params, ldp, actions, old_logp, index, offset, n, ratio_out, hd, mask, ldm, mask_T);
}

// phase 1 (parallel over samples): clamped importance ratio pi/pi_old of every step -> ratio_out[k]
template <int MAXA>
__global__ __launch_bounds__(256) void k_vtrace_ratio(const float *__restrict__ params, int ldp,
                                                      const float *__restrict__ actions,
                                                      const float *__restrict__ old_logp,
                                                      const int32_t *__restrict__ index, int64_t offset, int64_t n, int A,
                                                      int action_kind, float *__restrict__ ratio_out, HeadsDev hd) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int nact = hd.num_heads > 1 ? heads_action_cols(hd.head_n, hd.num_heads) : (action_kind == 0 ? 1 : A / 2);
    const int64_t d = index ? (int64_t)index[k] : offset + k;
    const float lp = hd.num_heads > 1 ? tuple_logp<false>(params + k * ldp, actions + d * nact, hd, nullptr)
                                      : action_logp<MAXA>(params + k * ldp, A, action_kind, actions + d * nact);
    ratio_out[k] = clampf(expf(lp - old_logp[d]), 0.05f, 20.0f);  // learner.py:591-594
}

// k_vtrace_ratio under an action mask, A <= 128: any head list, a plain Discrete(A) as a one-member list
__global__ __launch_bounds__(256) void k_masked_vtrace_ratio(const float *__restrict__ params, int ldp,
                                                             const float *__restrict__ actions,
                                                             const float *__restrict__ old_logp,
                                                             const int32_t *__restrict__ index, int64_t offset, int64_t n,
                                                             float *__restrict__ ratio_out, HeadsDev hd,
                                                             const uint8_t *__restrict__ mask, int64_t ldm, int mask_T) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int nact = heads_action_cols(hd.head_n, hd.num_heads);
    const int64_t d = index ? (int64_t)index[k] : offset + k;
    const float lp = tuple_logp<true>(params + k * ldp, actions + d * nact, hd, mask_row(mask, ldm, mask_T, d));
    ratio_out[k] = clampf(expf(lp - old_logp[d]), 0.05f, 20.0f);
}

// phase 2 (one lane per trajectory): the reverse recursion of learner.py:618-635; vs[k] holds the ratio of step k on
// entry (read before it is overwritten with the result)
__global__ __launch_bounds__(64) void k_vtrace(const float *__restrict__ values, int ldv,
                                               const float *__restrict__ rewards, const uint8_t *__restrict__ dones,
                                               const int32_t *__restrict__ index, int64_t offset, int64_t ntraj, int rec,
                                               float gamma, float rho_hat, float c_hat, float *__restrict__ vs,
                                               float *__restrict__ adv) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ntraj) return;
    const int64_t base = j * rec;
    const int64_t last = base + rec - 1;
    const int64_t dl = index ? (int64_t)index[last] : offset + last;
    float next_values = (values[last * ldv] - rewards[dl]) / gamma;
    float next_vs = next_values;
    for (int i = rec - 1; i >= 0; --i) {
        const int64_t k = base + i;
        const int64_t d = index ? (int64_t)index[k] : offset + k;
        const float ratio = vs[k];  // written by k_vtrace_ratio
        const float rho = fminf(rho_hat, ratio), c = fminf(c_hat, ratio);
        const float not_done = 1.0f - (dones[d] ? 1.0f : 0.0f);
        const float ndg = not_done * gamma;
        const float cv = values[k * ldv], r = rewards[d];
        const float delta_s = rho * ((r + ndg * next_values) - cv);
        adv[k] = rho * ((r + ndg * next_vs) - cv);
        next_vs = (cv + delta_s) + (ndg * c) * (next_vs - next_values);
        vs[k] = next_vs;
        next_values = cv;
    }
}

// sf_vtrace (mask = nullptr) and sf_vtrace_masked: `what` names the entry point in the messages
static int vtrace_launch(const char *what, const float *params, int ld_params, const float *values, int ld_values,
                         const float *actions, const float *old_logp, const float *rewards, const uint8_t *dones,
                         const int32_t *index, int64_t offset, int64_t n, int A, int action_kind, int recurrence,
                         float gamma, float rho_hat, float c_hat, float *vs, float *adv, const int32_t *head_n,
                         int num_heads, const uint8_t *mask, int64_t ld_mask, int mask_T, void *stream) {
    SF_REQUIRE(ld_params >= A && ld_values >= 1, "%s: bad strides", what);
    HeadsDev hd = {};
    if (head_n && num_heads > 1) {
        SF_REQUIRE(action_kind == 0, "%s: a head list needs action_kind 0", what);
        bool any_box;
        const int tot = heads_from_host(what, head_n, num_heads, SF_MAX_ACTION_HEADS, hd.head_n, &any_box);
        if (tot < 0) return SF_ERR_ARG;
        hd.num_heads = num_heads;
        SF_REQUIRE(tot == A, "%s: head sizes sum to %d, A = %d", what, tot, A);
    }
    SF_REQUIRE(params && values && actions && old_logp && rewards && dones && vs && adv, "%s: null pointer", what);
    SF_REQUIRE(recurrence > 0 && n % recurrence == 0, "%s: n=%lld not a multiple of recurrence=%d", what,
               (long long)n, recurrence);
    SF_REQUIRE(A > 0 && (action_kind == 0 || (action_kind == 1 && A % 2 == 0)),
               "%s: unsupported action params A=%d kind=%d", what, A, action_kind);
    const int64_t ntraj = n / recurrence;
    if (ntraj == 0) return SF_OK;
    const dim3 grid((unsigned)((ntraj + 63) / 64)), block(64), rgrid((unsigned)((n + 255) / 256));
    if (mask) {  // the masked ratio pass: any head list, in place (a plain Discrete(A) is a one-member list)
        const HeadsDev mh = hd.num_heads > 1 ? hd : single_head(A, action_kind);
        SF_REQUIRE(heads_any_discrete(mh), "%s: a pure Box space has no action mask", what);
        if (A >= WIDE_MIN_A) {
            SF_REQUIRE((n + WIDE_ROWS - 1) / WIDE_ROWS <= 0x7fffffffLL, "%s: n=%lld too large", what, (long long)n);
            k_masked_vtrace_ratio_wide<<<dim3((unsigned)((n + WIDE_ROWS - 1) / WIDE_ROWS)), dim3(256), 0, STREAM(stream)>>>(
                params, ld_params, actions, old_logp, index, offset, n, vs, mh, mask, ld_mask, mask_T);
        } else {
            k_masked_vtrace_ratio<<<rgrid, dim3(256), 0, STREAM(stream)>>>(params, ld_params, actions, old_logp, index,
                                                                          offset, n, vs, mh, mask, ld_mask, mask_T);
        }
        k_vtrace<<<grid, block, 0, STREAM(stream)>>>(values, ld_values, rewards, dones, index, offset, ntraj, recurrence,
                                                     gamma, rho_hat, c_hat, vs, adv);
        return sf_launch_status(what);
    }
#define VT_LAUNCH(M)                                                                                                   \
    k_vtrace_ratio<M><<<rgrid, dim3(256), 0, STREAM(stream)>>>(params, ld_params, actions, old_logp, index, offset, n, A, \
                                                               action_kind, vs, hd)
    if (A >= WIDE_MIN_A) {  // wave-per-row ratio
        SF_REQUIRE((n + WIDE_ROWS - 1) / WIDE_ROWS <= 0x7fffffffLL, "%s: n=%lld too large", what, (long long)n);
        k_vtrace_ratio_wide<<<dim3((unsigned)((n + WIDE_ROWS - 1) / WIDE_ROWS)), dim3(256), 0, STREAM(stream)>>>(
            params, ld_params, actions, old_logp, index, offset, n, vs,
            hd.num_heads > 1 ? hd : single_head(A, action_kind));
    } else if (A <= 8) VT_LAUNCH(8);
    else if (A <= 32) VT_LAUNCH(32);
    else VT_LAUNCH(128);
#undef VT_LAUNCH
    // the recursion reads the ratios only: one kernel whatever the distribution is
    k_vtrace<<<grid, block, 0, STREAM(stream)>>>(values, ld_values, rewards, dones, index, offset, ntraj, recurrence, gamma,
                                                 rho_hat, c_hat, vs, adv);
    return sf_launch_status(what);
}

extern "C" int sf_vtrace(const float *params, int ld_params, const float *values, int ld_values,
                         const float *actions, const float *old_logp, const float *rewards, const uint8_t *dones,
                         const int32_t *index, int64_t offset, int64_t n, int A, int action_kind, int recurrence,
                         float gamma, float rho_hat, float c_hat, float *vs, float *adv, const int32_t *head_n,
                         int num_heads, void *stream) {
    return vtrace_launch("sf_vtrace", params, ld_params, values, ld_values, actions, old_logp, rewards, dones, index, offset,
                         n, A, action_kind, recurrence, gamma, rho_hat, c_hat, vs, adv, head_n, num_heads, nullptr, 0, 0,
                         stream);
}

// the mask arguments of sf_vtrace_masked / sf_ppo_loss_masked, checked before anything else of the call
static int masked_args_ok(const char *what, const uint8_t *mask, int64_t ld_mask, int mask_T, int A) {
    SF_REQUIRE(mask, "%s: null mask", what);
    SF_REQUIRE(ld_mask >= A, "%s: ld_mask=%lld, the mask has one column per distribution parameter (A=%d)", what,
               (long long)ld_mask, A);
    SF_REQUIRE(mask_T >= 0, "%s: mask_T=%d is negative (0: a flat [N, ld_mask] mask; T: the slab's [E, T + 1, A])", what,
               mask_T);
    return SF_OK;
}

// sf_vtrace under the action mask the rows were sampled under
extern "C" int sf_vtrace_masked(const float *params, int ld_params, const float *values, int ld_values,
                                const float *actions, const float *old_logp, const float *rewards, const uint8_t *dones,
                                const int32_t *index, int64_t offset, int64_t n, int A, int action_kind, int recurrence,
                                float gamma, float rho_hat, float c_hat, float *vs, float *adv, const int32_t *head_n,
                                int num_heads, const uint8_t *mask, int64_t ld_mask, int mask_T, void *stream) {
    if (int rc = masked_args_ok("sf_vtrace_masked", mask, ld_mask, mask_T, A)) return rc;
    SF_REQUIRE(action_kind == 0, "sf_vtrace_masked: a pure Box space has no action mask");
    return vtrace_launch("sf_vtrace_masked", params, ld_params, values, ld_values, actions, old_logp, rewards, dones, index,
                         offset, n, A, action_kind, recurrence, gamma, rho_hat, c_hat, vs, adv, head_n, num_heads, mask,
                         ld_mask, mask_T, stream);
}

// =========================================================================================== K16 PPO loss fwd+bwd
// One lane per sample; the per-sample distribution lives in registers (template MAXA bounds the unrolled loops so no
// array is indexed dynamically).  Loss sums use wave shuffles -> LDS -> one double atomic per block per quantity.
// The four loss kernels differ in how a row's distribution terms are laid out over lanes and registers; what comes
// before (loss_prologue), between the forward terms and the gradient (loss_row) and after (loss_epilogue) is one code.
__device__ __forceinline__ int64_t ov_row(const LossDev &h, int64_t d) {
    if (h.ov_T <= 0) return d;
    const int64_t e = d / h.ov_T;
    return d + e;  // e*(T+1) + t = (e*T + t) + e
}

__device__ __forceinline__ void atomic_max_float(double *addr, float v) {
    // sums[4] holds the running max as a double; KL >= 0 up to rounding, compare on the bit pattern of (v+1) > 0
    unsigned long long *a = reinterpret_cast<unsigned long long *>(addr);
    const double dv = (double)v;
    unsigned long long old = *a, assumed;
    do {
        assumed = old;
        if (__longlong_as_double((long long)assumed) >= dv) break;
        old = atomicCAS(a, assumed, (unsigned long long)__double_as_longlong(dv));
    } while (assumed != old);
}

// global (all-reduced) advantage moments {sum, sum of squares, count} -> mean / unbiased variance, learner.py:646-647
__device__ __forceinline__ void adv_mean_var(const double *__restrict__ moments, double &mean64, double &var64) {
    const double mn = moments[2];
    mean64 = moments[0] / mn;
    var64 = (moments[1] - moments[0] * mean64) / (mn - 1.0);
}
struct LossPre {
    float adv_mean, denom, inv_n, symkl_gate;
};
// gated: the symmetric-KL exploration loss is selected and this is not its pre-pass.  Its clamp(max=30) / non-finite
// gate needs the MEAN, which a pre-pass leaves in sums[6] (see ppo_loss_launch); otherwise the gate is open.
__device__ __forceinline__ LossPre loss_prologue(const double *__restrict__ moments, const double *__restrict__ sums,
                                                 bool gated) {
    double mean64, var64;
    adv_mean_var(moments, mean64, var64);
    const double mn = moments[2];
    LossPre p;
    p.adv_mean = (float)mean64;
    const float adv_std = (float)sqrt(var64 > 0.0 ? var64 : (mn > 1.0 ? 0.0 : NAN));
    p.denom = fmaxf(adv_std, 1e-7f);
    p.inv_n = 1.0f / (float)mn;
    p.symkl_gate = gated ? (float)sums[6] : 1.0f;
    return p;
}

// Clipped surrogate and clipped value loss of one row with their derivatives (autograd semantics of min / max ties and
// clamp boundaries).  dlogp = logp - old_logp as the caller formed it (float, or rounded from a double sum).
struct LossRow {
    float ratio, raw_ratio, pl, vl, dL_dlogp, dvl;
};
__device__ __forceinline__ LossRow loss_row(float dlogp, float adv, float v, float vo, float R, const LossPre &p,
                                            const LossDev &h) {
    LossRow r;
    r.raw_ratio = expf(dlogp);
    r.ratio = clampf(r.raw_ratio, 0.05f, 20.0f);
    const float advn = (adv - p.adv_mean) / p.denom;
    const float clipped = clampf(r.ratio, h.clip_lo, h.clip_hi);
    const float lu_ = r.ratio * advn, lc_ = clipped * advn;
    r.pl = fminf(lu_, lc_);
    const float vclip = vo + clampf(v - vo, -h.clip_value, h.clip_value);
    const float l1 = (v - R) * (v - R), l2 = (vclip - R) * (vclip - R);
    r.vl = fmaxf(l1, l2);
    float dpl_dr;
    const bool in_clip = r.ratio >= h.clip_lo && r.ratio <= h.clip_hi;
    if (lu_ < lc_) dpl_dr = advn;
    else if (lu_ > lc_) dpl_dr = in_clip ? advn : 0.f;
    else dpl_dr = 0.5f * advn + (in_clip ? 0.5f * advn : 0.f);
    const bool in_hard = r.raw_ratio >= 0.05f && r.raw_ratio <= 20.0f;
    r.dL_dlogp = in_hard ? (-p.inv_n) * dpl_dr * r.raw_ratio : 0.f;
    const bool in_v = (v - vo) >= -h.clip_value && (v - vo) <= h.clip_value;
    if (l1 > l2) r.dvl = 2.f * (v - R);
    else if (l2 > l1) r.dvl = in_v ? 2.f * (vclip - R) : 0.f;
    else r.dvl = (v - R) + (in_v ? (vclip - R) : 0.f);
    return r;
}

// block reduction of a 256-thread block's sums {policy, exploration, KL, value} and of its largest KL into sums[0..4];
// sym_pass: acc[0] is the symmetric-KL sum of the pre-pass, into sums[7]
__device__ __forceinline__ void loss_epilogue(double (&acc)[4], float kl_max, double *__restrict__ sums, int sym_pass) {
    __shared__ double lds[4 * 4];
    __shared__ float lds_max[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    kl_max = sf_wave_max(kl_max);
    if (lane == 0) lds_max[wave] = kl_max;
    sf_block_sum<4>(acc, lds);  // contains a __syncthreads()
    if (threadIdx.x == 0) {
        if (sym_pass) { atomicAdd(&sums[7], acc[0]); return; }
        atomicAdd(&sums[0], acc[0]);
        atomicAdd(&sums[1], acc[1]);
        atomicAdd(&sums[2], acc[2]);
        atomicAdd(&sums[3], acc[3]);
        const float m = fmaxf(fmaxf(lds_max[0], lds_max[1]), fmaxf(lds_max[2], lds_max[3]));
        if (m > -1.0f) atomic_max_float(&sums[4], m);
    }
}

template <int MAXA>
__global__ __launch_bounds__(256) void k_ppo_loss(const float *__restrict__ params, int ldp,
                                                  const float *__restrict__ values, int ldv,
                                                  const float *__restrict__ actions,
                                                  const float *__restrict__ old_logp,
                                                  const float *__restrict__ old_params,
                                                  const float *__restrict__ old_values, const float *__restrict__ adv,
                                                  const float *__restrict__ targets,
                                                  const uint8_t *__restrict__ valids,
                                                  const int32_t *__restrict__ index, int64_t offset, int64_t n, int A,
                                                  LossDev h, const double *__restrict__ moments,
                                                  double *__restrict__ sums, float *__restrict__ g_params,
                                                  float *__restrict__ g_values, float *__restrict__ ratio_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const LossPre p = loss_prologue(moments, sums, h.expl_kind == 2);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    float kl_max = -1.0f;
    if (i < n) {
        const int64_t d = index ? (int64_t)index[i] : offset + i;
        const bool valid = valids[d] != 0;
        const float *z = params + i * ldp, *zold = old_params + d * A;
        float *gz = g_params + i * ldp;
        float logp_a = 0.f, ent = 0.f, kl = 0.f, symkl = 0.f;
        const int D = A / 2;
        float zz[MAXA], zo[MAXA];
        float mx = -INFINITY, mxo = -INFINITY, lse = 0.f, lseo = 0.f;
        int act = 0;
        if (h.action_kind == 0) {
            // (reg_softmax twice, with the two rows' loops fused: two separate passes at MAXA = 128 go to scratch)
#pragma unroll
            for (int k = 0; k < MAXA; ++k) {
                zz[k] = k < A ? z[k] : -INFINITY;
                zo[k] = k < A ? zold[k] : -INFINITY;
                mx = fmaxf(mx, zz[k]);
                mxo = fmaxf(mxo, zo[k]);
            }
            float se = 0.f, seo = 0.f;
#pragma unroll
            for (int k = 0; k < MAXA; ++k)
                if (k < A) { se += expf(zz[k] - mx); seo += expf(zo[k] - mxo); }
            lse = logf(se);
            lseo = logf(seo);
            act = (int)actions[d];
            const float u = 1.0f / (float)A, lu = logf(u);
            float a1 = 0.f, a2 = 0.f;
#pragma unroll
            for (int k = 0; k < MAXA; ++k)
                if (k < A) {
                    const float lp = (zz[k] - mx) - lse, p_ = expf(lp), q = (zo[k] - mxo) - lseo;
                    if (k == act) logp_a = lp;
                    ent -= p_ * lp;
                    kl += p_ * (lp - q);
                    a1 += p_ * (lp - lu);
                    a2 += u * (lu - lp);
                }
            symkl = 0.5f * (a1 + a2);
        } else {
            for (int k = 0; k < D; ++k) box_loss_terms(z, zold, actions + d * D, D, k, logp_a, ent, kl);
        }
        const int64_t da = h.dense_adv ? i : d;
        const LossRow r = loss_row(logp_a - old_logp[d], adv[da], values[i * ldv], old_values[ov_row(h, d)], targets[da],
                                   p, h);
        if (ratio_out) ratio_out[i] = r.ratio;  // summaries (learner.py:886-903)
        if (valid) {
            acc[0] = r.pl;
            acc[1] = (h.expl_kind == 2) ? symkl : ent;
            acc[2] = kl;
            acc[3] = r.vl;
            kl_max = kl;
            if (h.action_kind == 0) {
                const float u = 1.0f / (float)A, lu = logf(u);
                float klpu = 0.f;
                if (h.expl_kind == 2) {
#pragma unroll
                    for (int k = 0; k < MAXA; ++k)
                        if (k < A) { const float lp = (zz[k] - mx) - lse; klpu += expf(lp) * (lp - lu); }
                }
#pragma unroll
                for (int k = 0; k < MAXA; ++k)
                    if (k < A)
                        gz[k] = cat_grad(zz[k], zo[k], k == act, mx, lse, mxo, lseo, ent, kl, klpu, u, lu, r.dL_dlogp,
                                         p.inv_n, p.symkl_gate, h);
            } else {
                for (int k = 0; k < D; ++k) box_grad(z, zold, actions + d * D, D, k, r.dL_dlogp, p.inv_n, h, gz);
            }
            g_values[i * ldv] = h.value_coeff * p.inv_n * r.dvl;
        } else {
            for (int k = 0; k < A; ++k) gz[k] = 0.f;
            g_values[i * ldv] = 0.f;
        }
    }
    loss_epilogue(acc, kl_max, sums, 0);
}

// Tuple of Discrete / Box heads (TupleActionDistribution, action_distributions.py:197-287), A <= 128: independent
// members whose log-prob / entropy / KL / symmetric-KL add up.  Same loss and backward as k_ppo_loss, per-member softmax
// statistics; members are read from global memory in place (these kernels are ~0.1 % of a step: clarity over register
// blocking).  sym_pass != 0: only accumulate the symmetric-KL sum (pre-pass for its mean gate) into sums[7].
// KEEP (k_ppo_loss_md, up to 8 members): a member's seven statistics stay in the lane between the forward loop and the
// gradient loop, and the row's log-prob is a float sum.  !KEEP (k_ppo_loss_mh, up to SF_MAX_ACTION_HEADS members): seven
// float[64] arrays would be 448 registers, i.e. scratch, so the gradient loop calls cat_terms again (the same expressions,
// hence the same bits, for a second pass of expf over a row that is in cache); the row's log-prob is a sum of up to 64
// members' (|lp| can pass 100 each) and is added up in double, so that the ratio exp(logp - old_logp) does not inherit the
// rounding of a float running sum of that size.
// MASKED (k_masked_ppo_loss_md / k_masked_ppo_loss_mh): a Discrete member's terms and gradient come from
// masked_cat_terms / masked_cat_grad on its slice of the row's mask, the kept slot klpu_h holds 1 / (mass + 1e-13); a Box
// member never reads the mask.  The unmasked instantiations have no mask code at all.
template <bool KEEP, bool MASKED>
__device__ __forceinline__ void ppo_loss_tuple(const float *__restrict__ params, int ldp,
                                               const float *__restrict__ values, int ldv,
                                               const float *__restrict__ actions, const float *__restrict__ old_logp,
                                               const float *__restrict__ old_params,
                                               const float *__restrict__ old_values, const float *__restrict__ adv,
                                               const float *__restrict__ targets, const uint8_t *__restrict__ valids,
                                               const int32_t *__restrict__ index, int64_t offset, int64_t n, int A,
                                               const LossDev &h, const double *__restrict__ moments,
                                               double *__restrict__ sums, float *__restrict__ g_params,
                                               float *__restrict__ g_values, float *__restrict__ ratio_out,
                                               int sym_pass, const uint8_t *__restrict__ mask, int64_t ldm,
                                               int mask_T) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const LossPre p = loss_prologue(moments, sums, h.expl_kind == 2 && !sym_pass);
    const int H = h.hd.num_heads;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    float kl_max = -1.0f;
    if (i < n) {
        const int64_t d = index ? (int64_t)index[i] : offset + i;
        const bool valid = valids[d] != 0;
        const float *z = params + i * ldp, *zo = old_params + d * A;
        const float *arow = actions + d * heads_action_cols(h.hd.head_n, H);
        float *gz = g_params + i * ldp;
        const uint8_t *mk = nullptr;
        if constexpr (MASKED) mk = mask_row(mask, ldm, mask_T, d);
        float logp_a = 0.f;   // KEEP
        double logp_d = 0.0;  // !KEEP
        float ent = 0.f, kl = 0.f, symkl = 0.f;
        constexpr int NK = KEEP ? 8 : 1;
        float mx[NK], lse[NK], mxo[NK], lseo[NK], ent_h[NK], kl_h[NK], klpu_h[NK];
        auto keep = [&](const CatTerms &t, int s) {
            mx[s] = t.mx; lse[s] = t.lse; mxo[s] = t.mxo; lseo[s] = t.lseo;
            ent_h[s] = t.ent; kl_h[s] = t.kl; klpu_h[s] = t.klpu;
        };
        auto keep_masked = [&](const MaskedCatTerms &t, int s) {
            mx[s] = t.s.mx; lse[s] = t.s.lse; mxo[s] = t.so.mx; lseo[s] = t.so.lse;
            ent_h[s] = t.ent; kl_h[s] = t.kl; klpu_h[s] = t.s.inv;
        };
        int off = 0, aoff = 0;
        for (int hd = 0; hd < H; ++hd) {
            const int nh = h.hd.head_n[hd];
            if (nh < 0) {  // Box(D) member
                const int Dh = -nh;
                float lpp = KEEP ? logp_a : 0.f, e = 0.f, kk = 0.f;  // (the float sum runs on through the columns)
                for (int k = 0; k < Dh; ++k) box_loss_terms(z + off, zo + off, arow + aoff, Dh, k, lpp, e, kk);
                if constexpr (KEEP) logp_a = lpp;
                else logp_d += (double)lpp;
                ent += e; kl += kk;
                off += 2 * Dh; aoff += Dh;
                continue;
            }
            if constexpr (MASKED) {
                const MaskedCatTerms t = masked_cat_terms(z + off, zo + off, mk + off, nh, (int)arow[aoff]);
                if constexpr (KEEP) { keep_masked(t, hd); logp_a += t.lpa; }
                else logp_d += (double)t.lpa;
                ent += t.ent; kl += t.kl;
            } else {
                const CatTerms t = cat_terms(z + off, zo + off, nh, (int)arow[aoff]);
                if constexpr (KEEP) { keep(t, hd); logp_a += t.lpa; }
                else logp_d += (double)t.lpa;
                ent += t.ent; kl += t.kl; symkl += 0.5f * (t.klpu + t.a2);
            }
            off += nh; aoff += 1;
        }
        if (sym_pass) {
            if (valid) acc[0] = symkl;
        } else {
            const float dlogp = KEEP ? logp_a - old_logp[d] : (float)(logp_d - (double)old_logp[d]);
            const int64_t da = h.dense_adv ? i : d;
            const LossRow r = loss_row(dlogp, adv[da], values[i * ldv], old_values[ov_row(h, d)], targets[da], p, h);
            if (ratio_out) ratio_out[i] = r.ratio;
            if (valid) {
                acc[0] = r.pl;
                acc[1] = (h.expl_kind == 2) ? symkl : ent;
                acc[2] = kl;
                acc[3] = r.vl;
                kl_max = kl;
                off = 0;
                aoff = 0;
                for (int hd = 0; hd < H; ++hd) {
                    const int nh = h.hd.head_n[hd];
                    if (nh < 0) {  // Box(D) member
                        const int Dh = -nh;
                        for (int k = 0; k < Dh; ++k)
                            box_grad(z + off, zo + off, arow + aoff, Dh, k, r.dL_dlogp, p.inv_n, h, gz + off);
                        off += 2 * Dh; aoff += Dh;
                        continue;
                    }
                    const int act = (int)arow[aoff];
                    aoff += 1;
                    const int s = KEEP ? hd : 0;
                    if constexpr (MASKED) {
                        if constexpr (!KEEP) keep_masked(masked_cat_terms(z + off, zo + off, mk + off, nh, act), 0);
                        for (int k = 0; k < nh; ++k)
                            gz[off + k] = masked_cat_grad(z[off + k], zo[off + k], mk[off + k], k == act, mx[s], lse[s],
                                                          klpu_h[s], mxo[s], lseo[s], ent_h[s], kl_h[s], r.dL_dlogp,
                                                          p.inv_n, h);
                        off += nh;
                        continue;
                    }
                    if constexpr (!KEEP) keep(cat_terms(z + off, zo + off, nh, act), 0);  // the first loop's values, bit for bit
                    const float u = 1.0f / (float)nh, lu = logf(u);
                    for (int k = 0; k < nh; ++k)
                        gz[off + k] = cat_grad(z[off + k], zo[off + k], k == act, mx[s], lse[s], mxo[s], lseo[s], ent_h[s],
                                               kl_h[s], klpu_h[s], u, lu, r.dL_dlogp, p.inv_n, p.symkl_gate, h);
                    off += nh;
                }
                g_values[i * ldv] = h.value_coeff * p.inv_n * r.dvl;
            } else {
                for (int k = 0; k < A; ++k) gz[k] = 0.f;
                g_values[i * ldv] = 0.f;
            }
        }
    }
    loss_epilogue(acc, kl_max, sums, sym_pass);
}

__global__ __launch_bounds__(256) void k_ppo_loss_md(const float *__restrict__ params, int ldp,
                                                     const float *__restrict__ values, int ldv,
                                                     const float *__restrict__ actions,
                                                     const float *__restrict__ old_logp,
                                                     const float *__restrict__ old_params,
                                                     const float *__restrict__ old_values, const float *__restrict__ adv,
                                                     const float *__restrict__ targets,
                                                     const uint8_t *__restrict__ valids,
                                                     const int32_t *__restrict__ index, int64_t offset, int64_t n, int A,
                                                     LossDev h, const double *__restrict__ moments,
                                                     double *__restrict__ sums, float *__restrict__ g_params,
                                                     float *__restrict__ g_values, float *__restrict__ ratio_out,
                                                     int sym_pass) {
    ppo_loss_tuple<true, false>(params, ldp, values, ldv, actions, old_logp, old_params, old_values, adv, targets, valids,
                                index, offset, n, A, h, moments, sums, g_params, g_values, ratio_out, sym_pass, nullptr, 0,
                                0);
}

__global__ __launch_bounds__(256) void k_ppo_loss_mh(const float *__restrict__ params, int ldp,
                                                     const float *__restrict__ values, int ldv,
                                                     const float *__restrict__ actions,
                                                     const float *__restrict__ old_logp,
                                                     const float *__restrict__ old_params,
                                                     const float *__restrict__ old_values, const float *__restrict__ adv,
                                                     const float *__restrict__ targets,
                                                     const uint8_t *__restrict__ valids,
                                                     const int32_t *__restrict__ index, int64_t offset, int64_t n, int A,
                                                     LossDev h, const double *__restrict__ moments,
                                                     double *__restrict__ sums, float *__restrict__ g_params,
                                                     float *__restrict__ g_values, float *__restrict__ ratio_out,
                                                     int sym_pass) {
    ppo_loss_tuple<false, false>(params, ldp, values, ldv, actions, old_logp, old_params, old_values, adv, targets, valids,
                                 index, offset, n, A, h, moments, sums, g_params, g_values, ratio_out, sym_pass, nullptr,
                                 0, 0);
}

// k_ppo_loss_md / k_ppo_loss_mh under an action mask; a plain Discrete(A <= 128) runs k_masked_ppo_loss_md as a one-member
// list (a masked k_ppo_loss<128> would not fit the register file: the unmasked one sits at 256 VGPRs + 53 AGPRs)
#define SF_MASKED_LOSS_KERNEL(NAME, KEEP)                                                                                \
    __global__ __launch_bounds__(256) void NAME(                                                                         \
        const float *__restrict__ params, int ldp, const float *__restrict__ values, int ldv,                            \
        const float *__restrict__ actions, const float *__restrict__ old_logp, const float *__restrict__ old_params,     \
        const float *__restrict__ old_values, const float *__restrict__ adv, const float *__restrict__ targets,          \
        const uint8_t *__restrict__ valids, const int32_t *__restrict__ index, int64_t offset, int64_t n, int A,         \
        LossDev h, const double *__restrict__ moments, double *__restrict__ sums, float *__restrict__ g_params,          \
        float *__restrict__ g_values, float *__restrict__ ratio_out, const uint8_t *__restrict__ mask, int64_t ldm,      \
        int mask_T) {                                                                                                    \
        ppo_loss_tuple<KEEP, true>(params, ldp, values, ldv, actions, old_logp, old_params, old_values, adv, targets,    \
                                   valids, index, offset, n, A, h, moments, sums, g_params, g_values, ratio_out, 0, mask, \
                                   ldm, mask_T);                                                                         \
    }
SF_MASKED_LOSS_KERNEL(k_masked_ppo_loss_md, true)
SF_MASKED_LOSS_KERNEL(k_masked_ppo_loss_mh, false)
#undef SF_MASKED_LOSS_KERNEL

// pre-pass for the symmetric-KL exploration loss: mean over valid samples decides clamp(max=30) / isfinite gate
template <int MAXA>
__global__ __launch_bounds__(256) void k_symkl_sum(const float *__restrict__ params, int ldp,
                                                   const uint8_t *__restrict__ valids,
                                                   const int32_t *__restrict__ index, int64_t offset, int64_t n, int A,
                                                   double *__restrict__ out) {
    __shared__ double lds[4];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double acc[1] = {0.0};
    if (i < n) {
        const int64_t d = index ? (int64_t)index[i] : offset + i;
        if (valids[d]) {
            float zz[MAXA], mx, lse;
            reg_softmax<MAXA>(params + i * ldp, A, zz, mx, lse);
            const float u = 1.0f / (float)A, lu = logf(u);
            float a1 = 0.f, a2 = 0.f;
#pragma unroll
            for (int k = 0; k < MAXA; ++k)
                if (k < A) { const float lp = (zz[k] - mx) - lse; a1 += expf(lp) * (lp - lu); a2 += u * (lu - lp); }
            acc[0] = 0.5f * (a1 + a2);
        }
    }
    sf_block_sum<1>(acc, lds);
    if (threadIdx.x == 0) atomicAdd(out, acc[0]);
}

// k_ppo_loss / k_ppo_loss_md for A > 128 (any head list of up to SF_MAX_ACTION_HEADS members): the same formulas, one wave per row.
// Pass 1 per head: max / log-sum-exp of the current and the old logits in one read; pass 2: the head's log-prob,
// entropy, KL and symmetric-KL terms (kept per head in LDS: the gradient needs them and the row's total log-prob);
// pass 3: the gradient row, written 256 contiguous bytes per store.  The block's waves walk the rows with a grid
// stride and add their sums in double, so a launch issues a few thousand atomics whatever n is.
// sym_pass != 0: only the symmetric-KL sum of the valid rows (pre-pass for its mean gate) into sums[7].
// MASKED (k_masked_ppo_loss_wide): pass 1 pushes z - 1e9 on masked-out columns, for the current and the
// old logits alike; pass 2 sums the allowed columns' softmax mass, -s lp and s (lp - lp_old) and scales the last two by
// 1 / (mass + 1e-13), which slot 6 keeps for the gradient pass (no symmetric-KL there: the launcher refuses it).
template <bool MASKED>
__device__ __forceinline__ void ppo_loss_wide(const float *__restrict__ params, int ldp,
                                              const float *__restrict__ values, int ldv,
                                              const float *__restrict__ actions, const float *__restrict__ old_logp,
                                              const float *__restrict__ old_params, const float *__restrict__ old_values,
                                              const float *__restrict__ adv, const float *__restrict__ targets,
                                              const uint8_t *__restrict__ valids, const int32_t *__restrict__ index,
                                              int64_t offset, int64_t n, int A, const LossDev &h,
                                              const double *__restrict__ moments, double *__restrict__ sums,
                                              float *__restrict__ g_params, float *__restrict__ g_values,
                                              float *__restrict__ ratio_out, int sym_pass,
                                              const uint8_t *__restrict__ mask, int64_t ldm, int mask_T) {
    // per wave and head: mx, lse, mxo, lseo, entropy, KL, KL(p || uniform); 8 KB for the longest list
    __shared__ float hstat[WIDE_ROWS][SF_MAX_ACTION_HEADS][8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const LossPre p = loss_prologue(moments, sums, h.expl_kind == 2 && !sym_pass);
    const int H = h.hd.num_heads;
    const int NA = heads_action_cols(h.hd.head_n, H);
    float (*st)[8] = hstat[wave];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    float kl_max = -1.0f;
    for (int64_t i = (int64_t)blockIdx.x * WIDE_ROWS + wave; i < n; i += (int64_t)gridDim.x * WIDE_ROWS) {
        const int64_t d = index ? (int64_t)index[i] : offset + i;
        const bool valid = valids[d] != 0;
        const float *z = params + i * ldp, *zo = old_params + d * A, *arow = actions + d * NA;
        const uint8_t *mk = nullptr;
        if constexpr (MASKED) mk = mask_row(mask, ldm, mask_T, d);
        if (sym_pass) {
            if (!valid) continue;
            float symkl = 0.f;
            int off = 0;
            for (int hd = 0; hd < H; ++hd) {
                const int nh = h.hd.head_n[hd];  // categorical heads only (the launcher checks)
                float m1, l1;
                wide_lse(z + off, nh, lane, nullptr, m1, l1);
                const float u = 1.0f / (float)nh, lu = logf(u);
                float a1 = 0.f, a2 = 0.f;
#pragma unroll 4
                for (int k = lane; k < nh; k += 64) {
                    const float lp = (z[off + k] - m1) - l1;
                    a1 += expf(lp) * (lp - lu);
                    a2 += u * (lu - lp);
                }
                symkl += 0.5f * (wide_allsum(a1) + wide_allsum(a2));
                off += nh;
            }
            if (lane == 0) acc[0] += symkl;
            continue;
        }
        float *gz = g_params + i * ldp;
        float logp_a = 0.f, ent = 0.f, kl = 0.f, symkl = 0.f;
        double logp_d = 0.0;  // the same sum in double: what a list of more than 8 members takes its ratio from
        int off = 0, aoff = 0;
        for (int hd = 0; hd < H; ++hd) {
            const int nh = h.hd.head_n[hd];
            if (nh < 0) {  // Box(D) member
                const int Dh = -nh;
                float lpp = 0.f, e = 0.f, kk = 0.f;
                for (int k = lane; k < Dh; k += 64) box_loss_terms(z + off, zo + off, arow + aoff, Dh, k, lpp, e, kk);
                lpp = wide_allsum(lpp);
                logp_a += lpp; logp_d += (double)lpp;
                ent += wide_allsum(e);
                kl += wide_allsum(kk);
                off += 2 * Dh; aoff += Dh;
                continue;
            }
            float m1 = -INFINITY, s1 = 0.f, m2 = -INFINITY, s2 = 0.f;
            if constexpr (MASKED) {
#pragma unroll 4
                for (int k = lane; k < nh; k += 64) {
                    const float mo = mk[off + k] ? 0.f : -1e9f;
                    wide_push(m1, s1, z[off + k] + mo);
                    wide_push(m2, s2, zo[off + k] + mo);
                }
            } else {
#pragma unroll 4
                for (int k = lane; k < nh; k += 64) { wide_push(m1, s1, z[off + k]); wide_push(m2, s2, zo[off + k]); }
            }
            float mx, lse, mxo, lseo;
            wide_finish(m1, s1, mx, lse);
            wide_finish(m2, s2, mxo, lseo);
            const int act = (int)arow[aoff];
            if constexpr (MASKED) {
                float lpa = 0.f, e = 0.f, kk = 0.f, ps = 0.f;
#pragma unroll 4
                for (int k = lane; k < nh; k += 64) {
                    const uint8_t ok = mk[off + k];
                    const float mo = ok ? 0.f : -1e9f;
                    const float lp = ((z[off + k] + mo) - mx) - lse, q = ((zo[off + k] + mo) - mxo) - lseo;
                    const float s_ = ok ? expf((z[off + k] - mx) - lse) : 0.f;
                    if (k == act) lpa = lp;
                    ps += s_;
                    e -= s_ * lp;
                    kk += s_ * (lp - q);
                }
                lpa = wide_allsum(lpa);
                const float inv = 1.0f / (wide_allsum(ps) + 1e-13f);
                e = wide_allsum(e) * inv; kk = wide_allsum(kk) * inv;
                st[hd][0] = mx; st[hd][1] = lse; st[hd][2] = mxo; st[hd][3] = lseo;
                st[hd][4] = e; st[hd][5] = kk; st[hd][6] = inv;
                logp_a += lpa; logp_d += (double)lpa; ent += e; kl += kk;
                off += nh; aoff += 1;
                continue;
            }
            const float u = 1.0f / (float)nh, lu = logf(u);
            float lpa = 0.f, e = 0.f, kk = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll 4
            for (int k = lane; k < nh; k += 64) {
                const float lp = (z[off + k] - mx) - lse, p_ = expf(lp), q = (zo[off + k] - mxo) - lseo;
                if (k == act) lpa = lp;
                e -= p_ * lp;
                kk += p_ * (lp - q);
                a1 += p_ * (lp - lu);
                a2 += u * (lu - lp);
            }
            lpa = wide_allsum(lpa); e = wide_allsum(e); kk = wide_allsum(kk);
            a1 = wide_allsum(a1); a2 = wide_allsum(a2);
            // every lane stores the same bits and reads back its own store: no barrier
            st[hd][0] = mx; st[hd][1] = lse; st[hd][2] = mxo; st[hd][3] = lseo;
            st[hd][4] = e; st[hd][5] = kk; st[hd][6] = a1;
            logp_a += lpa; logp_d += (double)lpa; ent += e; kl += kk; symkl += 0.5f * (a1 + a2);
            off += nh; aoff += 1;
        }
        // up to 8 members: the float sum, as ever; more (|logp| can reach several hundred): the double one, see ppo_loss_tuple
        const float dlogp = H > 8 ? (float)(logp_d - (double)old_logp[d]) : logp_a - old_logp[d];
        const int64_t da = h.dense_adv ? i : d;
        const LossRow r = loss_row(dlogp, adv[da], values[i * ldv], old_values[ov_row(h, d)], targets[da], p, h);
        if (ratio_out && lane == 0) ratio_out[i] = r.ratio;
        if (!valid) {  // no loss, zero gradient
            for (int k = lane; k < A; k += 64) gz[k] = 0.f;
            if (lane == 0) g_values[i * ldv] = 0.f;
            continue;
        }
        if (lane == 0) {
            acc[0] += r.pl;
            acc[1] += (h.expl_kind == 2) ? symkl : ent;
            acc[2] += kl;
            acc[3] += r.vl;
            kl_max = fmaxf(kl_max, kl);
        }
        off = 0;
        aoff = 0;
        for (int hd = 0; hd < H; ++hd) {
            const int nh = h.hd.head_n[hd];
            if (nh < 0) {  // Box(D) member
                const int Dh = -nh;
                for (int k = lane; k < Dh; k += 64)
                    box_grad(z + off, zo + off, arow + aoff, Dh, k, r.dL_dlogp, p.inv_n, h, gz + off);
                off += 2 * Dh; aoff += Dh;
                continue;
            }
            const int act = (int)arow[aoff];
            aoff += 1;
            const float mx = st[hd][0], lse = st[hd][1], mxo = st[hd][2], lseo = st[hd][3];
            const float ent_h = st[hd][4], kl_h = st[hd][5], klpu_h = st[hd][6];
            if constexpr (MASKED) {
#pragma unroll 4
                for (int k = lane; k < nh; k += 64)
                    gz[off + k] = masked_cat_grad(z[off + k], h.kl_coeff != 0.f ? zo[off + k] : 0.f, mk[off + k], k == act,
                                                  mx, lse, klpu_h, mxo, lseo, ent_h, kl_h, r.dL_dlogp, p.inv_n, h);
                off += nh;
                continue;
            }
            const float u = 1.0f / (float)nh, lu = logf(u);
#pragma unroll 4
            for (int k = lane; k < nh; k += 64)
                gz[off + k] = cat_grad(z[off + k], h.kl_coeff != 0.f ? zo[off + k] : 0.f, k == act, mx, lse, mxo, lseo,
                                       ent_h, kl_h, klpu_h, u, lu, r.dL_dlogp, p.inv_n, p.symkl_gate, h);
            off += nh;
        }
        if (lane == 0) g_values[i * ldv] = h.value_coeff * p.inv_n * r.dvl;
    }
    loss_epilogue(acc, kl_max, sums, sym_pass);
}

__global__ __launch_bounds__(256) void k_ppo_loss_wide(const float *__restrict__ params, int ldp,
                                                       const float *__restrict__ values, int ldv,
                                                       const float *__restrict__ actions,
                                                       const float *__restrict__ old_logp,
                                                       const float *__restrict__ old_params,
                                                       const float *__restrict__ old_values,
                                                       const float *__restrict__ adv, const float *__restrict__ targets,
                                                       const uint8_t *__restrict__ valids,
                                                       const int32_t *__restrict__ index, int64_t offset, int64_t n, int A,
                                                       LossDev h, const double *__restrict__ moments,
                                                       double *__restrict__ sums, float *__restrict__ g_params,
                                                       float *__restrict__ g_values, float *__restrict__ ratio_out,
                                                       int sym_pass) {
    ppo_loss_wide<false>(params, ldp, values, ldv, actions, old_logp, old_params, old_values, adv, targets, valids, index,
                         offset, n, A, h, moments, sums, g_params, g_values, ratio_out, sym_pass, nullptr, 0, 0);
}

__global__ __launch_bounds__(256) void k_masked_ppo_loss_wide(const float *__restrict__ params, int ldp,
                                                              const float *__restrict__ values, int ldv,
                                                              const float *__restrict__ actions,
                                                              const float *__restrict__ old_logp,
                                                              const float *__restrict__ old_params,
                                                              const float *__restrict__ old_values,
                                                              const float *__restrict__ adv,
                                                              const float *__restrict__ targets,
                                                              const uint8_t *__restrict__ valids,
                                                              const int32_t *__restrict__ index, int64_t offset, int64_t n,
                                                              int A, LossDev h, const double *__restrict__ moments,
                                                              double *__restrict__ sums, float *__restrict__ g_params,
                                                              float *__restrict__ g_values, float *__restrict__ ratio_out,
                                                              const uint8_t *__restrict__ mask, int64_t ldm, int mask_T) {
    ppo_loss_wide<true>(params, ldp, values, ldv, actions, old_logp, old_params, old_values, adv, targets, valids, index,
                        offset, n, A, h, moments, sums, g_params, g_values, ratio_out, 0, mask, ldm, mask_T);
}

__global__ void k_symkl_gate(double *__restrict__ sums, const double *__restrict__ moments) {
    if (threadIdx.x || blockIdx.x) return;
    const float m = (float)(sums[7] / moments[2]);
    sums[6] = (isfinite(m) && m <= 30.0f) ? 1.0 : 0.0;
}

// hd: the checked member list (one member: Discrete(A) / Box(A / 2))
static LossDev make_loss_dev(const sf_loss_cfg *c, const HeadsDev &hd) {
    LossDev h;
    h.clip_hi = (float)(1.0 + (double)c->clip_ratio);
    h.clip_lo = (float)(1.0 / (1.0 + (double)c->clip_ratio));
    h.clip_value = c->clip_value;
    h.value_coeff = c->value_loss_coeff;
    h.expl_coeff = c->exploration_coeff;
    h.kl_coeff = c->kl_coeff;
    h.expl_kind = c->exploration_coeff == 0.f ? 0 : c->exploration_kind;
    h.action_kind = c->action_kind;
    h.dense_adv = c->dense_adv;
    h.hd = hd;
    h.ov_T = c->old_values_T > 0 ? c->old_values_T : 0;
    return h;
}

static int ppo_loss_wide_launch(const float *params, int ld_params, const float *values, int ld_values,
                                const float *actions, const float *old_logp, const float *old_params,
                                const float *old_values, const float *adv, const float *targets, const uint8_t *valids,
                                const int32_t *index, int64_t offset, int64_t n, int A, const LossDev &h,
                                const double *moments, double *sums, float *g_params, float *g_values, float *ratio_out,
                                const uint8_t *mask, int64_t ld_mask, int mask_T, void *stream) {
    const int64_t want = (n + WIDE_ROWS - 1) / WIDE_ROWS;
    const dim3 grid((unsigned)(want < 2048 ? want : 2048)), block(256);  // 256 CUs x 8 blocks; the rows are grid-strided
    if (mask) {
        k_masked_ppo_loss_wide<<<grid, block, 0, STREAM(stream)>>>(params, ld_params, values, ld_values, actions, old_logp,
                                                                   old_params, old_values, adv, targets, valids, index,
                                                                   offset, n, A, h, moments, sums, g_params, g_values,
                                                                   ratio_out, mask, ld_mask, mask_T);
        return sf_launch_status("sf_ppo_loss_masked");
    }
    if (h.expl_kind == 2) {
        k_ppo_loss_wide<<<grid, block, 0, STREAM(stream)>>>(params, ld_params, values, ld_values, actions, old_logp,
                                                            old_params, old_values, adv, targets, valids, index, offset,
                                                            n, A, h, moments, sums, g_params, g_values, nullptr, 1);
        k_symkl_gate<<<dim3(1), dim3(64), 0, STREAM(stream)>>>(sums, moments);
    }
    k_ppo_loss_wide<<<grid, block, 0, STREAM(stream)>>>(params, ld_params, values, ld_values, actions, old_logp, old_params,
                                                        old_values, adv, targets, valids, index, offset, n, A, h, moments,
                                                        sums, g_params, g_values, ratio_out, 0);
    return sf_launch_status("sf_ppo_loss");
}

// sf_ppo_loss and sf_ppo_loss_heads: `what` names the entry point in the messages; head_n / num_heads is the struct's list
// (cap 8) or the argument's (cap SF_MAX_ACTION_HEADS).  num_heads <= 1: one Discrete(A) / Box(A / 2).
static int ppo_loss_launch(const char *what, const float *params, int ld_params, const float *values, int ld_values,
                           const float *actions, const float *old_logp, const float *old_params,
                           const float *old_values, const float *adv, const float *targets, const uint8_t *valids,
                           const int32_t *index, int64_t offset, int64_t n, int A, const sf_loss_cfg *h_cfg,
                           const int32_t *head_n, int num_heads, int cap, const double *moments, double *sums,
                           float *g_params, float *g_values, float *ratio_out, const uint8_t *mask, int64_t ld_mask,
                           int mask_T, void *stream) {
    SF_REQUIRE(ld_params >= A && ld_values >= 1, "%s: bad strides", what);
    SF_REQUIRE(params && values && actions && old_logp && old_params && old_values && adv && targets && valids &&
                   h_cfg && moments && sums && g_params && g_values,
               "%s: null pointer", what);
    SF_REQUIRE(n > 0 && A > 0, "%s: bad shape n=%lld A=%d", what, (long long)n, A);
    SF_REQUIRE(h_cfg->action_kind == 0 || (h_cfg->action_kind == 1 && A % 2 == 0), "%s: bad action_kind", what);
    SF_REQUIRE(!(h_cfg->exploration_kind == 2 && h_cfg->action_kind != 0 && h_cfg->exploration_coeff != 0.f),
               "%s: symmetric_kl exploration loss needs a categorical distribution", what);
    const bool tuple = h_cfg->action_kind == 0 && num_heads > 1;
    HeadsDev hd = single_head(A, h_cfg->action_kind);
    if (tuple) {  // every check of the list comes before the first launch (the memset included)
        bool any_box;
        const int tot = heads_from_host(what, head_n, num_heads, cap, hd.head_n, &any_box);
        if (tot < 0) return SF_ERR_ARG;
        hd.num_heads = num_heads;
        SF_REQUIRE(tot == A, "%s: head sizes sum to %d, A = %d", what, tot, A);
        SF_REQUIRE(!(any_box && h_cfg->exploration_kind == 2 && h_cfg->exploration_coeff != 0.f),
                   "%s: symmetric_kl exploration loss needs categorical heads only (the reference's "
                   "ContinuousActionDistribution has no symmetric_kl_with_uniform_prior)", what);
    }
    if (mask) {  // sf_ppo_loss_masked: the rule is defined per Discrete member, without the uniform-prior term
        SF_REQUIRE(h_cfg->action_kind == 0 && heads_any_discrete(hd), "%s: a pure Box space has no action mask", what);
        SF_REQUIRE(!(h_cfg->exploration_kind == 2 && h_cfg->exploration_coeff != 0.f),
                   "%s: exploration_loss=symmetric_kl has no meaning under an action mask (log-probs of masked-out "
                   "actions are about -1e9); use exploration_loss=entropy", what);
    }
    const LossDev h = make_loss_dev(h_cfg, hd);
    int rc = sf_hip_status(hipMemsetAsync(sums, 0, 8 * sizeof(double), STREAM(stream)), "sf_ppo_loss memset");
    if (rc) return rc;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
#define PL_DISPATCH(KERNEL, ...)                                                        \
    do {                                                                                \
        if (A <= 8) KERNEL<8><<<grid, block, 0, STREAM(stream)>>>(__VA_ARGS__);         \
        else if (A <= 32) KERNEL<32><<<grid, block, 0, STREAM(stream)>>>(__VA_ARGS__);  \
        else KERNEL<128><<<grid, block, 0, STREAM(stream)>>>(__VA_ARGS__);              \
    } while (0)
    if (mask) {  // one wave per row from WIDE_MIN_A parameters on, else one lane per row over the member list
        if (A >= WIDE_MIN_A) return ppo_loss_wide_launch(params, ld_params, values, ld_values, actions, old_logp,
                                                         old_params, old_values, adv, targets, valids, index, offset, n,
                                                         A, h, moments, sums, g_params, g_values, ratio_out, mask,
                                                         ld_mask, mask_T, stream);
        auto kern = h.hd.num_heads <= 8 ? k_masked_ppo_loss_md : k_masked_ppo_loss_mh;
        kern<<<grid, block, 0, STREAM(stream)>>>(params, ld_params, values, ld_values, actions, old_logp, old_params,
                                                 old_values, adv, targets, valids, index, offset, n, A, h, moments, sums,
                                                 g_params, g_values, ratio_out, mask, ld_mask, mask_T);
        return sf_launch_status(what);
    }
    if (tuple) {
        if (A >= WIDE_MIN_A) return ppo_loss_wide_launch(params, ld_params, values, ld_values, actions, old_logp,
                                                         old_params, old_values, adv, targets, valids, index, offset, n,
                                                         A, h, moments, sums, g_params, g_values, ratio_out, nullptr, 0,
                                                         0, stream);
        // up to 8 members: their statistics stay in the lane (k_ppo_loss_md); more: recomputed (k_ppo_loss_mh)
        auto kern = h.hd.num_heads <= 8 ? k_ppo_loss_md : k_ppo_loss_mh;
        if (h.expl_kind == 2) {
            kern<<<grid, block, 0, STREAM(stream)>>>(params, ld_params, values, ld_values, actions, old_logp, old_params,
                                                     old_values, adv, targets, valids, index, offset, n, A, h, moments,
                                                     sums, g_params, g_values, nullptr, 1);
            k_symkl_gate<<<dim3(1), dim3(64), 0, STREAM(stream)>>>(sums, moments);
        }
        kern<<<grid, block, 0, STREAM(stream)>>>(params, ld_params, values, ld_values, actions, old_logp, old_params,
                                                 old_values, adv, targets, valids, index, offset, n, A, h, moments, sums,
                                                 g_params, g_values, ratio_out, 0);
        return sf_launch_status(what);
    }
    if (A >= WIDE_MIN_A)  // a single Discrete(A) / Box(A / 2) as a one-member head list
        return ppo_loss_wide_launch(params, ld_params, values, ld_values, actions, old_logp, old_params, old_values, adv,
                                    targets, valids, index, offset, n, A, h, moments, sums, g_params, g_values,
                                    ratio_out, nullptr, 0, 0, stream);
    if (h.expl_kind == 2) {
        PL_DISPATCH(k_symkl_sum, params, ld_params, valids, index, offset, n, A, sums + 7);
        k_symkl_gate<<<dim3(1), dim3(64), 0, STREAM(stream)>>>(sums, moments);
    }
    PL_DISPATCH(k_ppo_loss, params, ld_params, values, ld_values, actions, old_logp, old_params, old_values, adv, targets, valids, index,
                offset, n, A, h, moments, sums, g_params, g_values, ratio_out);
#undef PL_DISPATCH
    return sf_launch_status(what);
}

extern "C" int sf_ppo_loss(const float *params, int ld_params, const float *values, int ld_values,
                           const float *actions, const float *old_logp, const float *old_params,
                           const float *old_values, const float *adv, const float *targets, const uint8_t *valids,
                           const int32_t *index, int64_t offset, int64_t n, int A, const sf_loss_cfg *h_cfg,
                           const double *moments, double *sums, float *g_params, float *g_values, float *ratio_out,
                           void *stream) {
    return ppo_loss_launch("sf_ppo_loss", params, ld_params, values, ld_values, actions, old_logp, old_params, old_values,
                           adv, targets, valids, index, offset, n, A, h_cfg, h_cfg ? h_cfg->head_n : nullptr,
                           h_cfg ? h_cfg->num_heads : 0, 8, moments, sums, g_params, g_values, ratio_out, nullptr, 0, 0,
                           stream);
}

extern "C" int sf_ppo_loss_heads(const float *params, int ld_params, const float *values, int ld_values,
                                 const float *actions, const float *old_logp, const float *old_params,
                                 const float *old_values, const float *adv, const float *targets, const uint8_t *valids,
                                 const int32_t *index, int64_t offset, int64_t n, int A, const sf_loss_cfg *h_cfg,
                                 const double *moments, double *sums, float *g_params, float *g_values, float *ratio_out,
                                 const int32_t *head_n, int num_heads, void *stream) {
    // the list is the argument's, whatever the struct says; one member is that member alone, as num_heads <= 1 there
    SF_REQUIRE(head_n && num_heads >= 1 && num_heads <= SF_MAX_ACTION_HEADS,
               "sf_ppo_loss_heads: %d action heads, the limit is %d (SF_MAX_ACTION_HEADS)", num_heads,
               SF_MAX_ACTION_HEADS);
    if (num_heads == 1)
        SF_REQUIRE(h_cfg && head_n[0] == (h_cfg->action_kind == 0 ? A : -(A / 2)),
                   "sf_ppo_loss_heads: a one-member list must be Discrete(A) with action_kind 0 or Box(A / 2) with 1");
    else
        SF_REQUIRE(h_cfg && h_cfg->action_kind == 0, "sf_ppo_loss_heads: a head list needs action_kind 0");
    return ppo_loss_launch("sf_ppo_loss_heads", params, ld_params, values, ld_values, actions, old_logp, old_params,
                           old_values, adv, targets, valids, index, offset, n, A, h_cfg, head_n, num_heads,
                           SF_MAX_ACTION_HEADS, moments, sums, g_params, g_values, ratio_out, nullptr, 0, 0, stream);
}

// sf_ppo_loss_heads under the action mask the rows were sampled under
extern "C" int sf_ppo_loss_masked(const float *params, int ld_params, const float *values, int ld_values,
                                  const float *actions, const float *old_logp, const float *old_params,
                                  const float *old_values, const float *adv, const float *targets, const uint8_t *valids,
                                  const int32_t *index, int64_t offset, int64_t n, int A, const sf_loss_cfg *h_cfg,
                                  const double *moments, double *sums, float *g_params, float *g_values, float *ratio_out,
                                  const int32_t *head_n, int num_heads, const uint8_t *mask, int64_t ld_mask, int mask_T,
                                  void *stream) {
    if (int rc = masked_args_ok("sf_ppo_loss_masked", mask, ld_mask, mask_T, A)) return rc;
    SF_REQUIRE(head_n && num_heads >= 1 && num_heads <= SF_MAX_ACTION_HEADS,
               "sf_ppo_loss_masked: %d action heads, the limit is %d (SF_MAX_ACTION_HEADS)", num_heads,
               SF_MAX_ACTION_HEADS);
    SF_REQUIRE(h_cfg && h_cfg->action_kind == 0, "sf_ppo_loss_masked: a pure Box space has no action mask");
    if (num_heads == 1)
        SF_REQUIRE(head_n[0] == A, "sf_ppo_loss_masked: a one-member list must be Discrete(A)");
    return ppo_loss_launch("sf_ppo_loss_masked", params, ld_params, values, ld_values, actions, old_logp, old_params,
                           old_values, adv, targets, valids, index, offset, n, A, h_cfg, head_n, num_heads,
                           SF_MAX_ACTION_HEADS, moments, sums, g_params, g_values, ratio_out, mask, ld_mask, mask_T, stream);
}

// =========================================================================================== consistency loss (DrAC)
// --augment_consistency_coeff: KL(target || student) of the action distributions plus the squared value
// difference between two rows of one heads matrix — row i on the clean frames (the target, a constant) and its twin on the
// shifted ones (the student) — with the gradient for the student row only.  The arithmetic is the PPO loss's: cat_lse /
// wide_push for a Discrete member's statistics, box_sd for a Box column, so both round as sf_ppo_loss does; rows with the
// same bits give exactly 0 (lp_t - lp_s, p_s - p_t, vr - 1, log 1 and mu_s - mu_t are all exact zeros).
// column k of a Box(D) member: its KL(N_t || N_s), and the student's gradient scaled by `scale` into gz[k] / gz[D + k]
__device__ __forceinline__ float box_consistency(const float *__restrict__ zt, const float *__restrict__ zs, int D, int k,
                                                 float scale, float *__restrict__ gz) {
    const float mut = zt[k], sdt = box_sd(zt[D + k]);
    const float mus = zs[k], es = expf(zs[D + k]);
    const float sds = clampf(es, 1e-4f, 1e4f);
    const bool inside = es >= 1e-4f && es <= 1e4f;  // (beyond the clamp the standard deviation does not move: box_grad)
    const float vr = (sdt / sds) * (sdt / sds);
    const float dl = (mut - mus) / sds;
    gz[k] = scale * ((mus - mut) / (sds * sds));
    gz[D + k] = inside ? scale * (1.f - vr - dl * dl) : 0.f;
    return 0.5f * (vr + dl * dl - 1.f - logf(vr));
}
// column k of a Discrete member from the two rows' statistics: its KL term, the student's gradient into *g
__device__ __forceinline__ float cat_consistency(float ztk, float zsk, float mxt, float lset, float mxs, float lses,
                                                 float scale, float *__restrict__ g) {
    const float lpt = (ztk - mxt) - lset, pt = expf(lpt), lps = (zsk - mxs) - lses;
    *g = scale * (expf(lps) - pt);
    return pt * (lpt - lps);
}
// block reduction of {sum KL, sum (dv)^2, n_valid} and the largest KL into sums[0], [1], [3] and [2]
__device__ __forceinline__ void consistency_epilogue(double (&acc)[3], float kl_max, double *__restrict__ sums) {
    __shared__ double lds[4 * 3];
    __shared__ float lds_max[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    kl_max = sf_wave_max(kl_max);
    if (lane == 0) lds_max[wave] = kl_max;
    sf_block_sum<3>(acc, lds);  // contains a __syncthreads()
    if (threadIdx.x == 0) {
        atomicAdd(&sums[0], acc[0]);
        atomicAdd(&sums[1], acc[1]);
        atomicAdd(&sums[3], acc[2]);
        const float m = fmaxf(fmaxf(lds_max[0], lds_max[1]), fmaxf(lds_max[2], lds_max[3]));
        if (m > -1.0f) atomic_max_float(&sums[2], m);
    }
}

// A <= 128: one lane per row over the member list, both rows read in place (as k_ppo_loss_mh reads them)
__global__ __launch_bounds__(256) void k_consistency_loss(const float *__restrict__ params_t,
                                                          const float *__restrict__ params_s, int ldp,
                                                          const float *__restrict__ values_t,
                                                          const float *__restrict__ values_s, int ldv,
                                                          const uint8_t *__restrict__ valids,
                                                          const int32_t *__restrict__ index, int64_t offset, int64_t n,
                                                          int A, HeadsDev hd, float coeff_policy, float coeff_value,
                                                          const double *__restrict__ moments, double *__restrict__ sums,
                                                          float *__restrict__ g_params_s, float *__restrict__ g_values_s) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const float inv_n = 1.0f / (float)moments[2];
    double acc[3] = {0.0, 0.0, 0.0};
    float kl_max = -1.0f;
    if (i < n) {
        const int64_t d = index ? (int64_t)index[i] : offset + i;
        const float *zt = params_t + i * ldp, *zs = params_s + i * ldp;
        float *gz = g_params_s + i * ldp;
        if (valids[d] != 0) {
            const float sp = coeff_policy * inv_n;
            float kl = 0.f;
            int off = 0;
            for (int h = 0; h < hd.num_heads; ++h) {
                const int nh = hd.head_n[h];
                if (nh < 0) {  // Box(D) member
                    const int D = -nh;
                    for (int k = 0; k < D; ++k) kl += box_consistency(zt + off, zs + off, D, k, sp, gz + off);
                    off += 2 * D;
                    continue;
                }
                float mxt, lset, mxs, lses, kk = 0.f;
                cat_lse(zt + off, nh, mxt, lset);
                cat_lse(zs + off, nh, mxs, lses);
                for (int k = 0; k < nh; ++k)
                    kk += cat_consistency(zt[off + k], zs[off + k], mxt, lset, mxs, lses, sp, gz + off + k);
                kl += kk;
                off += nh;
            }
            const float dv = values_s[i * ldv] - values_t[i * ldv];
            g_values_s[i * ldv] = coeff_value * inv_n * (2.f * dv);
            acc[0] = kl;
            acc[1] = dv * dv;
            acc[2] = 1.0;
            kl_max = kl;
        } else {  // not counted, zero gradient row
            for (int k = 0; k < A; ++k) gz[k] = 0.f;
            g_values_s[i * ldv] = 0.f;
        }
    }
    consistency_epilogue(acc, kl_max, sums);
}

// A > 128: one wave64 per row, four rows per block, lanes striding the columns of a member (the wide family's layout)
__global__ __launch_bounds__(256) void k_consistency_loss_wide(const float *__restrict__ params_t,
                                                               const float *__restrict__ params_s, int ldp,
                                                               const float *__restrict__ values_t,
                                                               const float *__restrict__ values_s, int ldv,
                                                               const uint8_t *__restrict__ valids,
                                                               const int32_t *__restrict__ index, int64_t offset,
                                                               int64_t n, int A, HeadsDev hd, float coeff_policy,
                                                               float coeff_value, const double *__restrict__ moments,
                                                               double *__restrict__ sums, float *__restrict__ g_params_s,
                                                               float *__restrict__ g_values_s) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float inv_n = 1.0f / (float)moments[2];
    const float sp = coeff_policy * inv_n;
    double acc[3] = {0.0, 0.0, 0.0};
    float kl_max = -1.0f;
    for (int64_t i = (int64_t)blockIdx.x * WIDE_ROWS + wave; i < n; i += (int64_t)gridDim.x * WIDE_ROWS) {
        const int64_t d = index ? (int64_t)index[i] : offset + i;
        const float *zt = params_t + i * ldp, *zs = params_s + i * ldp;
        float *gz = g_params_s + i * ldp;
        if (valids[d] == 0) {  // wave-uniform: not counted, zero gradient row
            for (int k = lane; k < A; k += 64) gz[k] = 0.f;
            if (lane == 0) g_values_s[i * ldv] = 0.f;
            continue;
        }
        float kl = 0.f;
        int off = 0;
        for (int h = 0; h < hd.num_heads; ++h) {
            const int nh = hd.head_n[h];
            float kk = 0.f;
            if (nh < 0) {  // Box(D) member
                const int D = -nh;
                for (int k = lane; k < D; k += 64) kk += box_consistency(zt + off, zs + off, D, k, sp, gz + off);
                kl += wide_allsum(kk);
                off += 2 * D;
                continue;
            }
            float m1 = -INFINITY, s1 = 0.f, m2 = -INFINITY, s2 = 0.f;
#pragma unroll 4
            for (int k = lane; k < nh; k += 64) { wide_push(m1, s1, zt[off + k]); wide_push(m2, s2, zs[off + k]); }
            float mxt, lset, mxs, lses;
            wide_finish(m1, s1, mxt, lset);
            wide_finish(m2, s2, mxs, lses);
#pragma unroll 4
            for (int k = lane; k < nh; k += 64)
                kk += cat_consistency(zt[off + k], zs[off + k], mxt, lset, mxs, lses, sp, gz + off + k);
            kl += wide_allsum(kk);
            off += nh;
        }
        if (lane == 0) {
            const float dv = values_s[i * ldv] - values_t[i * ldv];
            g_values_s[i * ldv] = coeff_value * inv_n * (2.f * dv);
            acc[0] += kl;
            acc[1] += dv * dv;
            acc[2] += 1.0;
            kl_max = fmaxf(kl_max, kl);
        }
    }
    consistency_epilogue(acc, kl_max, sums);
}

extern "C" int sf_consistency_loss(const float *params_t, const float *params_s, int ld_params, const float *values_t,
                                   const float *values_s, int ld_values, const uint8_t *valids, const int32_t *index,
                                   int64_t offset, int64_t n, int A, int action_kind, const int32_t *head_n,
                                   int num_heads, float coeff_policy, float coeff_value, const double *moments,
                                   double *sums, float *g_params_s, float *g_values_s, void *stream) {
    const char *what = "sf_consistency_loss";
    SF_REQUIRE(params_t && params_s && values_t && values_s && valids && moments && sums && g_params_s && g_values_s,
               "%s: null pointer", what);
    SF_REQUIRE(n >= 0 && A > 0 && offset >= 0, "%s: bad shape n=%lld A=%d offset=%lld", what, (long long)n, A,
               (long long)offset);
    SF_REQUIRE(ld_params >= A && ld_values >= 1, "%s: bad strides", what);
    SF_REQUIRE(action_kind == 0 || (action_kind == 1 && A % 2 == 0), "%s: bad action_kind %d for A=%d", what,
               action_kind, A);
    // (comparisons, so that NaN fails too)
    SF_REQUIRE(coeff_policy >= 0.f && coeff_policy <= 3.402823466e38f && coeff_value >= 0.f && coeff_value <= 3.402823466e38f,
               "%s: the coefficients must be finite and not negative", what);
    HeadsDev hd = single_head(A, action_kind);
    if (head_n || num_heads > 1) {  // the member list, as sf_ppo_loss_heads takes it; every check comes before the memset
        bool any_box;
        const int tot = heads_from_host(what, head_n, num_heads, SF_MAX_ACTION_HEADS, hd.head_n, &any_box);
        if (tot < 0) return SF_ERR_ARG;
        hd.num_heads = num_heads;
        if (num_heads == 1)
            SF_REQUIRE(head_n[0] == (action_kind == 0 ? A : -(A / 2)),
                       "%s: a one-member list must be Discrete(A) with action_kind 0 or Box(A / 2) with 1", what);
        else
            SF_REQUIRE(action_kind == 0, "%s: a head list needs action_kind 0", what);
        SF_REQUIRE(tot == A, "%s: head sizes sum to %d, A = %d", what, tot, A);
    }
    if (n == 0) return SF_OK;
    const bool wide = A >= WIDE_MIN_A;
    const int64_t want = wide ? (n + WIDE_ROWS - 1) / WIDE_ROWS : (n + 255) / 256;
    SF_REQUIRE(want <= 0x7fffffffLL, "%s: n=%lld too large", what, (long long)n);
    int rc = sf_hip_status(hipMemsetAsync(sums, 0, 4 * sizeof(double), STREAM(stream)), "sf_consistency_loss memset");
    if (rc) return rc;
    if (wide)  // 256 CUs x 8 blocks; the rows are grid-strided
        k_consistency_loss_wide<<<dim3((unsigned)(want < 2048 ? want : 2048)), dim3(256), 0, STREAM(stream)>>>(
            params_t, params_s, ld_params, values_t, values_s, ld_values, valids, index, offset, n, A, hd, coeff_policy,
            coeff_value, moments, sums, g_params_s, g_values_s);
    else
        k_consistency_loss<<<dim3((unsigned)want), dim3(256), 0, STREAM(stream)>>>(
            params_t, params_s, ld_params, values_t, values_s, ld_values, valids, index, offset, n, A, hd, coeff_policy,
            coeff_value, moments, sums, g_params_s, g_values_s);
    return sf_launch_status(what);
}

__global__ void k_loss_scalars(const double *__restrict__ sums, const double *__restrict__ moments, LossDev h,
                               float *__restrict__ out) {
    if (threadIdx.x || blockIdx.x) return;
    const double n = moments[2];
    double mean64, var64;
    adv_mean_var(moments, mean64, var64);
    out[0] = (float)(-(sums[0] / n));
    if (h.expl_kind == 1) out[1] = (float)(-(double)h.expl_coeff * (sums[1] / n));
    else if (h.expl_kind == 2) {
        float m = (float)(sums[1] / n);
        if (!isfinite(m)) m = 0.f;
        out[1] = h.expl_coeff * fminf(m, 30.0f);
    } else out[1] = 0.f;
    out[2] = (float)((double)h.kl_coeff * (sums[2] / n));
    out[3] = (float)((double)h.value_coeff * (sums[3] / n));
    out[4] = (float)(sums[2] / n);
    out[5] = (float)sums[4];
    out[6] = (float)mean64;
    out[7] = (float)sqrt(var64 > 0.0 ? var64 : 0.0);
    out[8] = (float)n;
    out[9] = (float)(sums[1] / n);
}

extern "C" int sf_loss_scalars(const double *sums, const double *moments, const sf_loss_cfg *h_cfg, float *out,
                               void *stream) {
    SF_REQUIRE(sums && moments && h_cfg && out, "sf_loss_scalars: null pointer");
    k_loss_scalars<<<dim3(1), dim3(64), 0, STREAM(stream)>>>(sums, moments, make_loss_dev(h_cfg, HeadsDev{}), out);
    return sf_launch_status("sf_loss_scalars");
}

// =========================================================================================== train summaries
// learner.py:843-923 (_record_summaries) for the last minibatch of a training call: the reference evaluates ~25 small
// torch reductions with one .item() each; here ONE pass over the minibatch's rows accumulates every statistic
// (block reduction -> one atomic per block and quantity), a second small launch takes the maximum of Adam's second
// moments, and the caller reads 24 doubles back.  out layout (device double[24], initialised by the call):
//   [0] n rows  [1] n valid  [2] n same-policy  [3] sum value  [4] sum |1 - ratio| (valid)  [5] n clipped (valid)
//   [6] sum |v - v_old|  [7] sum version_diff (same policy)
//   [8] ratio min (valid)  [9] ratio max (valid)  [10] max |v - v_old|  [11] act min  [12] act max  [13] adv min
//   [14] adv max  [15] max |old action parameter|  [16] version_diff min  [17] version_diff max  [18] max exp_avg_sq
constexpr int SUMM_NS = 8, SUMM_NM = 11, SUMM_OUT = 24;
struct SummArgs {
    const uint8_t *valids;
    const float *ratio, *values, *old_values, *actions, *adv, *policy_version, *action_logits;
    const int32_t *policy_id, *index;
    int64_t offset, n;
    int ld_values, old_values_T, num_actions, A, dense_adv, my_pid;
    float train_step, clip_lo, clip_hi;
};
__device__ __forceinline__ void atomic_minmax_d(double *addr, double v, bool is_max) {
    unsigned long long *a = reinterpret_cast<unsigned long long *>(addr);
    unsigned long long old = *a, assumed;
    do {
        assumed = old;
        const double cur = __longlong_as_double((long long)assumed);
        if (is_max ? cur >= v : cur <= v) break;
        old = atomicCAS(a, assumed, (unsigned long long)__double_as_longlong(v));
    } while (assumed != old);
}
__global__ void k_summ_init(double *out) {
    const int i = threadIdx.x;
    if (i >= SUMM_OUT) return;
    // sums 0; minima +inf; maxima -inf
    const bool is_min = i == 8 || i == 11 || i == 13 || i == 16;
    const bool is_max = i == 9 || i == 10 || i == 12 || i == 14 || i == 15 || i == 17 || i == 18;
    out[i] = is_min ? (double)INFINITY : is_max ? -(double)INFINITY : 0.0;
}
__global__ __launch_bounds__(256) void k_train_summaries(SummArgs p, double *__restrict__ out) {
    __shared__ double lds[4 * SUMM_NS];
    __shared__ float ldm[4 * SUMM_NM];
    double s[SUMM_NS] = {0, 0, 0, 0, 0, 0, 0, 0};
    // minima: r_min, act_min, adv_min, vd_min;  maxima: r_max, dv_max, act_max, adv_max, logit_absmax, vd_max (+1 spare)
    float mn[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
    float mx[7] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < p.n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t d = p.index ? (int64_t)p.index[i] : p.offset + i;
        const bool valid = p.valids[d] != 0, same = p.policy_id[d] == p.my_pid;
        const float v = p.values[i * p.ld_values];
        const int64_t dv_row = p.old_values_T > 0 ? d + d / p.old_values_T : d;
        const float dv = fabsf(v - p.old_values[dv_row]);
        s[0] += 1.0;
        s[1] += valid ? 1.0 : 0.0;
        s[2] += same ? 1.0 : 0.0;
        s[3] += (double)v;
        s[6] += (double)dv;
        mx[1] = fmaxf(mx[1], dv);
        if (valid) {
            const float r = p.ratio[i];
            s[4] += (double)fabsf(1.0f - r);
            s[5] += (r < p.clip_lo ? 1.0 : 0.0) + (r > p.clip_hi ? 1.0 : 0.0);
            mn[0] = fminf(mn[0], r);
            mx[0] = fmaxf(mx[0], r);
        }
        for (int a = 0; a < p.num_actions; ++a) {
            const float x = p.actions[d * p.num_actions + a];
            mn[1] = fminf(mn[1], x);
            mx[2] = fmaxf(mx[2], x);
        }
        const float ad = p.adv[p.dense_adv ? i : d];
        mn[2] = fminf(mn[2], ad);
        mx[3] = fmaxf(mx[3], ad);
        for (int a = 0; a < p.A; ++a) mx[4] = fmaxf(mx[4], fabsf(p.action_logits[d * p.A + a]));
        if (same) {
            const float vd = p.train_step - p.policy_version[d];
            s[7] += (double)vd;
            mn[3] = fminf(mn[3], vd);
            mx[5] = fmaxf(mx[5], vd);
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < SUMM_NS; ++k) s[k] = sf_wave_sum(s[k]);
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) mn[k] = fminf(mn[k], __shfl_down(mn[k], off, 64));
#pragma unroll
    for (int k = 0; k < 7; ++k) mx[k] = sf_wave_max(mx[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < SUMM_NS; ++k) lds[wave * SUMM_NS + k] = s[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) ldm[wave * SUMM_NM + k] = mn[k];
#pragma unroll
        for (int k = 0; k < 7; ++k) ldm[wave * SUMM_NM + 4 + k] = mx[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int nw = (blockDim.x + 63) >> 6;
        for (int k = 0; k < SUMM_NS; ++k) {
            double t = 0.0;
            for (int w = 0; w < nw; ++w) t += lds[w * SUMM_NS + k];
            if (t != 0.0) atomicAdd(&out[k], t);
        }
        float m4[4] = {INFINITY, INFINITY, INFINITY, INFINITY}, x7[7];
        for (int k = 0; k < 7; ++k) x7[k] = -INFINITY;
        for (int w = 0; w < nw; ++w) {
            for (int k = 0; k < 4; ++k) m4[k] = fminf(m4[k], ldm[w * SUMM_NM + k]);
            for (int k = 0; k < 7; ++k) x7[k] = fmaxf(x7[k], ldm[w * SUMM_NM + 4 + k]);
        }
        // out slots: 8 r_min, 9 r_max, 10 dv_max, 11 act_min, 12 act_max, 13 adv_min, 14 adv_max, 15 logit, 16 vd_min, 17 vd_max
        atomic_minmax_d(&out[8], (double)m4[0], false);
        atomic_minmax_d(&out[9], (double)x7[0], true);
        atomic_minmax_d(&out[10], (double)x7[1], true);
        atomic_minmax_d(&out[11], (double)m4[1], false);
        atomic_minmax_d(&out[12], (double)x7[2], true);
        atomic_minmax_d(&out[13], (double)m4[2], false);
        atomic_minmax_d(&out[14], (double)x7[3], true);
        atomic_minmax_d(&out[15], (double)x7[4], true);
        atomic_minmax_d(&out[16], (double)m4[3], false);
        atomic_minmax_d(&out[17], (double)x7[5], true);
    }
}
__global__ __launch_bounds__(256) void k_max_f32(const float *__restrict__ x, int64_t n, double *__restrict__ out) {
    __shared__ float ldm[4];
    float m = -INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        m = fmaxf(m, x[i]);
    m = sf_wave_max(m);
    if ((threadIdx.x & 63) == 0) ldm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int)((blockDim.x + 63) >> 6); ++w) m = fmaxf(m, ldm[w]);
        atomic_minmax_d(out, (double)m, true);
    }
}

extern "C" int sf_train_summaries(const uint8_t *valids, const float *ratio, const float *values, int ld_values,
                                  const float *old_values, int old_values_T, const float *actions, int num_actions,
                                  const float *adv, int dense_adv, const int32_t *policy_id, const float *policy_version,
                                  const float *action_logits, int A, const int32_t *index, int64_t offset, int64_t n,
                                  int my_policy_id, int train_step, float clip_ratio, const float *exp_avg_sq, int64_t P,
                                  double *out, void *stream) {
    SF_REQUIRE(valids && ratio && values && old_values && actions && adv && policy_id && policy_version && action_logits &&
                   out && n > 0 && num_actions > 0 && A > 0 && ld_values >= 1,
               "sf_train_summaries: bad args");
    SummArgs p{valids, ratio, values, old_values, actions, adv, policy_version, action_logits, policy_id, index, offset, n,
               ld_values, old_values_T, num_actions, A, dense_adv, my_policy_id, (float)train_step,
               (float)(1.0 / (1.0 + (double)clip_ratio)), (float)(1.0 + (double)clip_ratio)};
    k_summ_init<<<dim3(1), dim3(64), 0, STREAM(stream)>>>(out);
    const int64_t blocks = (n + 255) / 256;
    k_train_summaries<<<dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, STREAM(stream)>>>(p, out);
    if (exp_avg_sq && P > 0) {
        const int64_t b2 = (P + 1023) / 1024;
        k_max_f32<<<dim3((unsigned)(b2 < 1024 ? b2 : 1024)), dim3(256), 0, STREAM(stream)>>>(exp_avg_sq, P, out + 18);
    }
    return sf_launch_status("sf_train_summaries");
}

// =========================================================================================== device row copies
// dst[r][0..row_bytes) = src[r][0..row_bytes) for r < rows, rows `pitch` bytes apart on either side: the slab's column
// copies (next rollout's obs[:, 0] <- obs[:, T], rnn_states likewise, bootstrap value -> values[:, T]).  16-byte units
// when every address allows it, 4-byte units otherwise, bytes as the last resort.
template <typename V>
__global__ __launch_bounds__(256) void k_copy_rows(char *__restrict__ dst, int64_t dst_pitch, const char *__restrict__ src,
                                                   int64_t src_pitch, int64_t units_per_row, int64_t rows) {
    const int64_t total = units_per_row * rows;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / units_per_row, u = i - r * units_per_row;
        *reinterpret_cast<V *>(dst + r * dst_pitch + u * (int64_t)sizeof(V)) =
            *reinterpret_cast<const V *>(src + r * src_pitch + u * (int64_t)sizeof(V));
    }
}
extern "C" int sf_copy_rows(void *dst, int64_t dst_pitch, const void *src, int64_t src_pitch, int64_t row_bytes,
                            int64_t rows, void *stream) {
    SF_REQUIRE(dst && src && row_bytes > 0 && rows > 0 && (rows == 1 || (llabs(dst_pitch) >= row_bytes && llabs(src_pitch) >= row_bytes)),
               "sf_copy_rows: bad args (row_bytes=%lld rows=%lld)", (long long)row_bytes, (long long)rows);
    const uintptr_t all = (uintptr_t)dst | (uintptr_t)src | (uintptr_t)dst_pitch | (uintptr_t)src_pitch | (uintptr_t)row_bytes;
    const int unit = (all & 15) == 0 ? 16 : (all & 3) == 0 ? 4 : 1;
    const int64_t upr = row_bytes / unit, total = upr * rows;
    const dim3 grid((unsigned)((total + 255) / 256 < 65536 ? (total + 255) / 256 : 65536)), block(256);
    char *d = reinterpret_cast<char *>(dst);
    const char *s = reinterpret_cast<const char *>(src);
    if (unit == 16) k_copy_rows<uint4><<<grid, block, 0, STREAM(stream)>>>(d, dst_pitch, s, src_pitch, upr, rows);
    else if (unit == 4) k_copy_rows<uint32_t><<<grid, block, 0, STREAM(stream)>>>(d, dst_pitch, s, src_pitch, upr, rows);
    else k_copy_rows<uint8_t><<<grid, block, 0, STREAM(stream)>>>(d, dst_pitch, s, src_pitch, upr, rows);
    return sf_launch_status("sf_copy_rows");
}

// =========================================================================================== host-env ingest
extern "C" int sf_h2d_rows(void *dst, int64_t dst_pitch, const void *src, int64_t src_pitch, int64_t row_bytes,
                           int64_t rows, void *stream) {
    SF_REQUIRE(dst && src && row_bytes > 0 && rows > 0 && dst_pitch >= row_bytes && src_pitch >= row_bytes,
               "sf_h2d_rows: row_bytes=%lld rows=%lld pitches %lld/%lld", (long long)row_bytes, (long long)rows,
               (long long)dst_pitch, (long long)src_pitch);
    const hipError_t e = hipMemcpy2DAsync(dst, (size_t)dst_pitch, src, (size_t)src_pitch, (size_t)row_bytes,
                                          (size_t)rows, hipMemcpyHostToDevice, STREAM(stream));
    SF_REQUIRE(e == hipSuccess, "sf_h2d_rows: hipMemcpy2DAsync: %s", hipGetErrorString(e));
    return 0;
}

// =========================================================================================== K14 minibatch indices
__device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;
    return x;
}
// bijection on [0, 2^(2*half)) : 4-round balanced Feistel
__device__ __forceinline__ uint32_t feistel(uint32_t x, int half, uint32_t key) {
    const uint32_t mask = (1u << half) - 1u;
    uint32_t l = x >> half, r = x & mask;
#pragma unroll
    for (int round = 0; round < 4; ++round) {
        const uint32_t f = mix32(r ^ (key + 0x9E3779B9u * (uint32_t)(round + 1))) & mask;
        const uint32_t nl = r, nr = l ^ f;
        l = nl; r = nr;
    }
    return (l << half) | r;
}

// chunk_starts != NULL: the permutation comes from the host (the reference's seeded np.random.permutation of the
// recurrence-aligned chunk starts, learner.py:507-510), given as dataset indices; only the expansion runs here.
__global__ __launch_bounds__(256) void k_minibatch_indices(int32_t *__restrict__ out, int64_t n_chunks, int rec,
                                                           int shuffle, int half, uint32_t key,
                                                           const int32_t *__restrict__ chunk_starts) {
    const int64_t wave_first = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) & ~(int64_t)63;  // first chunk of wave
    const int lane = threadIdx.x & 63;
    const int64_t j = wave_first + lane;
    uint32_t start = 0;
    if (j < n_chunks) {
        uint32_t x = (uint32_t)j;
        if (chunk_starts) {
            x = (uint32_t)chunk_starts[j] / (uint32_t)rec;
        } else if (shuffle) {
            do { x = feistel(x, half, key); } while ((int64_t)x >= n_chunks);  // cycle walking keeps it a bijection
        }
        start = x;
    }
    // expansion: the wave's 64 chunk starts are exchanged with wave shuffles so that the 64*rec output words are
    // written as fully coalesced runs (lane l writes word q*64+l of the wave's output span).
    const int64_t out_base = wave_first * rec;
    for (int q = 0; q < rec; ++q) {
        const int w = q * 64 + lane;
        const int src_lane = w / rec, r = w - src_lane * rec;
        const uint32_t s = __shfl(start, src_lane, 64);
        if (wave_first + src_lane < n_chunks) out[out_base + w] = (int32_t)(s * (uint32_t)rec + (uint32_t)r);
    }
}

extern "C" int sf_minibatch_indices(int32_t *out, int64_t experience_size, int recurrence, int shuffle, uint32_t seed,
                                    uint32_t epoch, void *stream) {
    SF_REQUIRE(out && experience_size > 0 && recurrence > 0 && experience_size % recurrence == 0,
               "sf_minibatch_indices: experience_size=%lld recurrence=%d", (long long)experience_size, recurrence);
    SF_REQUIRE(experience_size < (1LL << 31), "sf_minibatch_indices: experience too large for int32 indices");
    const int64_t n_chunks = experience_size / recurrence;
    int bits = 1;
    while ((1LL << bits) < n_chunks) ++bits;
    const int half = (bits + 1) / 2;
    const uint32_t key = seed * 0x9E3779B1u + epoch * 0x85EBCA77u + 0x165667B1u;
    k_minibatch_indices<<<dim3((unsigned)((n_chunks + 255) / 256)), dim3(256), 0, STREAM(stream)>>>(
        out, n_chunks, recurrence, shuffle, half, key, nullptr);
    return sf_launch_status("sf_minibatch_indices");
}

extern "C" int sf_minibatch_expand(const int32_t *chunk_starts, int32_t *out, int64_t experience_size, int recurrence,
                                   void *stream) {
    SF_REQUIRE(chunk_starts && out && experience_size > 0 && recurrence > 0 && experience_size % recurrence == 0,
               "sf_minibatch_expand: experience_size=%lld recurrence=%d", (long long)experience_size, recurrence);
    SF_REQUIRE(experience_size < (1LL << 31), "sf_minibatch_expand: experience too large for int32 indices");
    const int64_t n_chunks = experience_size / recurrence;
    k_minibatch_indices<<<dim3((unsigned)((n_chunks + 255) / 256)), dim3(256), 0, STREAM(stream)>>>(
        out, n_chunks, recurrence, 0, 0, 0u, chunk_starts);
    return sf_launch_status("sf_minibatch_expand");
}

// =========================================================================================== K18/K19 clip + Adam
__global__ __launch_bounds__(256) void k_grad_sumsq(const float *__restrict__ g, int64_t P,
                                                    double *__restrict__ sumsq) {
    __shared__ double lds[4];
    double acc[1] = {0.0};
    const int64_t nvec = P / 4;
    const float4 *g4 = reinterpret_cast<const float4 *>(g);
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = tid; i < nvec; i += nt) {
        const float4 v = g4[i];
        acc[0] += (double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w;
    }
    for (int64_t i = nvec * 4 + tid; i < P; i += nt) acc[0] += (double)g[i] * g[i];
    sf_block_sum<1>(acc, lds);
    if (threadIdx.x == 0) atomicAdd(sumsq, acc[0]);
}

extern "C" int sf_grad_sumsq(const float *g, int64_t P, double *sumsq, void *stream) {
    SF_REQUIRE(g && sumsq && P > 0, "sf_grad_sumsq: bad args");
    SF_REQUIRE(((uintptr_t)g & 15) == 0, "sf_grad_sumsq: gradient buffer must be 16-byte aligned");
    int rc = sf_hip_status(hipMemsetAsync(sumsq, 0, sizeof(double), STREAM(stream)), "sf_grad_sumsq memset");
    if (rc) return rc;
    const int64_t blocks = (P / 4 + 255) / 256;
    k_grad_sumsq<<<dim3((unsigned)(blocks < 1024 ? (blocks ? blocks : 1) : 1024)), dim3(256), 0, STREAM(stream)>>>(
        g, P, sumsq);
    return sf_launch_status("sf_grad_sumsq");
}

struct AdamC {
    float lr_step, bc2_sqrt, w1, b2, w2, eps, max_norm, grad_scale;
};

__device__ __forceinline__ void adam1(float &p, float g, float &m, float &v, const AdamC &c, float coef) {
    g = g * coef;
    m = m + (g - m) * c.w1;
    v = v * c.b2 + (g * g) * c.w2;
    const float denom = sqrtf(v) / c.bc2_sqrt + c.eps;
    p = p - c.lr_step * (m / denom);
}

__global__ __launch_bounds__(256) void k_adam(float *__restrict__ p, const float *__restrict__ g,
                                              float *__restrict__ m, float *__restrict__ v, int64_t P, AdamC c,
                                              const double *__restrict__ sumsq, const uint32_t *__restrict__ skip,
                                              const float *__restrict__ lr_dev) {
    if (skip && *skip) return;  // an aborted fused recurrent pass produced this gradient: leave weights and moments alone
    if (lr_dev) c.lr_step *= *lr_dev;  // sf_adam_step_dlr: the learning rate lives on the device (KL-adaptive schedule)
    float coef = c.grad_scale;
    if (sumsq && c.max_norm > 0.f) {
        // clip_grad_norm_: total_norm of the (already grad_scale'd) gradient
        const float total = (float)sqrt(*sumsq) * fabsf(c.grad_scale);
        const float cc = c.max_norm / (total + 1e-6f);
        coef = c.grad_scale * fminf(cc, 1.0f);
    }
    const int64_t nvec = P / 4;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
    float4 *p4 = reinterpret_cast<float4 *>(p), *m4 = reinterpret_cast<float4 *>(m), *v4 = reinterpret_cast<float4 *>(v);
    const float4 *g4 = reinterpret_cast<const float4 *>(g);
    for (int64_t i = tid; i < nvec; i += nt) {
        float4 pp = p4[i], mm = m4[i], vv = v4[i];
        const float4 gg = g4[i];
        adam1(pp.x, gg.x, mm.x, vv.x, c, coef);
        adam1(pp.y, gg.y, mm.y, vv.y, c, coef);
        adam1(pp.z, gg.z, mm.z, vv.z, c, coef);
        adam1(pp.w, gg.w, mm.w, vv.w, c, coef);
        p4[i] = pp; m4[i] = mm; v4[i] = vv;
    }
    for (int64_t i = nvec * 4 + tid; i < P; i += nt) adam1(p[i], g[i], m[i], v[i], c, coef);
}

static int adam_step_impl(float *p, const float *g, float *m, float *v, int64_t P, int step, float lr, float beta1,
                          float beta2, float eps, float max_grad_norm, const double *sumsq, float grad_scale,
                          const uint32_t *skip_flag, const float *lr_dev, void *stream, const char *who) {
    SF_REQUIRE(p && g && m && v && P > 0 && step >= 1, "%s: bad args", who);
    SF_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0,
               "%s: buffers must be 16-byte aligned", who);
    AdamC c;
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    c.lr_step = (float)((double)lr / bc1);
    c.bc2_sqrt = (float)sqrt(bc2);
    c.w1 = (float)(1.0 - (double)beta1);
    c.b2 = beta2;
    c.w2 = (float)(1.0 - (double)beta2);
    c.eps = eps;
    c.max_norm = max_grad_norm;
    c.grad_scale = grad_scale;
    const int64_t blocks = (P / 4 + 255) / 256;
    k_adam<<<dim3((unsigned)(blocks < 2048 ? (blocks ? blocks : 1) : 2048)), dim3(256), 0, STREAM(stream)>>>(
        p, g, m, v, P, c, sumsq, skip_flag, lr_dev);
    return sf_launch_status(who);
}

extern "C" int sf_adam_step(float *p, const float *g, float *m, float *v, int64_t P, int step, float lr, float beta1,
                            float beta2, float eps, float max_grad_norm, const double *sumsq, float grad_scale,
                            const uint32_t *skip_flag, void *stream) {
    return adam_step_impl(p, g, m, v, P, step, lr, beta1, beta2, eps, max_grad_norm, sumsq, grad_scale, skip_flag, nullptr,
                          stream, "sf_adam_step");
}
// the same step with the learning rate read from DEVICE memory: lr = *lr_dev * lr_scale (lr_scale: the valid-sample
// fraction of learner.py:788-794).  With sf_lr_kl_adaptive this keeps the per-minibatch KL-adaptive schedule
// (learner.py:46-85, lr_schedule=kl_adaptive_minibatch) off the host: no read-back between SGD steps.
extern "C" int sf_adam_step_dlr(float *p, const float *g, float *m, float *v, int64_t P, int step, const float *lr_dev,
                                float lr_scale, float beta1, float beta2, float eps, float max_grad_norm,
                                const double *sumsq, float grad_scale, const uint32_t *skip_flag, void *stream) {
    SF_REQUIRE(lr_dev, "sf_adam_step_dlr: null lr_dev");
    return adam_step_impl(p, g, m, v, P, step, lr_scale, beta1, beta2, eps, max_grad_norm, sumsq, grad_scale, skip_flag,
                          lr_dev, stream, "sf_adam_step_dlr");
}

// Measurement helper (bench.py's roofline.clock_ghz): ONE wave spins for `spin_cycles` shader cycles and reports how many
// ticks of the constant 100 MHz wall clock (s_memrealtime) went by meanwhile: shader clock [GHz] = 0.1 * out[0] / out[1].
// Launched on a side stream during the timed region it reads the clock the chip actually runs at under that load (the
// DVFS-governed clock is what the 2.4 GHz peak has to be scaled by; sysfs / smi values proved unreliable on the boxes).
__global__ void k_clock_probe(unsigned long long *__restrict__ out, int spin_cycles) {
    if (threadIdx.x || blockIdx.x) return;
    const unsigned long long w0 = wall_clock64(), c0 = clock64();
    unsigned long long c1 = c0;
    while ((long long)(c1 - c0) < (long long)spin_cycles) c1 = clock64();
    const unsigned long long w1 = wall_clock64();
    out[0] = c1 - c0;
    out[1] = w1 - w0;
}
extern "C" int sf_clock_probe(unsigned long long *out, int spin_cycles, void *stream) {
    SF_REQUIRE(out && spin_cycles > 0, "sf_clock_probe: bad args");
    k_clock_probe<<<dim3(1), dim3(64), 0, STREAM(stream)>>>(out, spin_cycles);
    return sf_launch_status("sf_clock_probe");
}

// learner.py:46-85 (KlAdaptiveScheduler.update): lr /= 1.5 (floor lr_min) when the KL of the step exceeds 2 x threshold,
// lr *= 1.5 (cap lr_max) when it is below threshold / 2.  kl: device float (the minibatch's mean KL, sf_loss_scalars[4]);
// lr_dev: device float, updated in place; lr_out (may be NULL): a copy of the new value for the epoch's read-back.
__global__ void k_lr_kl_adaptive(const float *__restrict__ kl, float *__restrict__ lr_dev, float threshold, float lr_min,
                                 float lr_max, float *__restrict__ lr_out) {
    if (threadIdx.x || blockIdx.x) return;
    const double k = (double)*kl;
    double lr = (double)*lr_dev;
    if (k > 2.0 * (double)threshold) lr = fmax(lr / 1.5, (double)lr_min);
    if (k < 0.5 * (double)threshold) lr = fmin(lr * 1.5, (double)lr_max);
    *lr_dev = (float)lr;
    if (lr_out) *lr_out = (float)lr;
}
extern "C" int sf_lr_kl_adaptive(const float *kl, float *lr_dev, float threshold, float lr_min, float lr_max,
                                 float *lr_out, void *stream) {
    SF_REQUIRE(kl && lr_dev, "sf_lr_kl_adaptive: null pointer");
    k_lr_kl_adaptive<<<dim3(1), dim3(64), 0, STREAM(stream)>>>(kl, lr_dev, threshold, lr_min, lr_max, lr_out);
    return sf_launch_status("sf_lr_kl_adaptive");
}

// =========================================================================================== Lamb (cfg.optimizer=lamb)
// sample_factory/algo/utils/optimizers.py:14-189 as the Learner configures it (learner.py:228-243: lr, betas, eps;
// weight_decay 1e-4, min_trust 0.01, bias correction, no look-ahead), list-params path: Adam direction + weight decay,
// then a per-TENSOR trust ratio min(||w||, 10) / ||step|| clamped to [min_trust, 1/min_trust].  The flat buffer carries
// a segment id per element (one id per reference tensor; 255 = padding), so two streaming passes suffice:
//   pass 1: moments, direction u -> scratch, per-segment sum w^2 / sum u^2 (LDS bins -> one atomic per bin and block)
//   pass 2: w -= lr * trust[seg] * u
struct LambC {
    float inv_bc1, inv_bc2_sqrt, w1, b1, b2, w2, eps, wd, max_norm, grad_scale, lr, min_trust;
};
constexpr int LAMB_MAX_SEG = 64;

__global__ __launch_bounds__(256) void k_lamb_dir(const float *__restrict__ p, const float *__restrict__ g,
                                                  float *__restrict__ m, float *__restrict__ v,
                                                  float *__restrict__ upd, const uint8_t *__restrict__ seg, int64_t P,
                                                  LambC c, const double *__restrict__ sumsq,
                                                  double *__restrict__ seg_sums, const uint32_t *__restrict__ skip) {
    if (skip && *skip) return;
    __shared__ double bins[2 * LAMB_MAX_SEG];
    for (int i = threadIdx.x; i < 2 * LAMB_MAX_SEG; i += blockDim.x) bins[i] = 0.0;
    __syncthreads();
    float coef = c.grad_scale;
    if (sumsq && c.max_norm > 0.f) {
        const float total = (float)sqrt(*sumsq) * fabsf(c.grad_scale);
        coef = c.grad_scale * fminf(c.max_norm / (total + 1e-6f), 1.0f);
    }
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = tid; i < P; i += nt) {
        const int sg = seg[i];
        if (sg >= LAMB_MAX_SEG) continue;  // padding
        const float gg = g[i] * coef, w = p[i];
        const float mm = m[i] * c.b1 + c.w1 * gg;          // exp_avg.mul_(b1).add_(grad, alpha=1-b1)
        const float vv = v[i] * c.b2 + c.w2 * (gg * gg);   // exp_avg_sq.mul_(b2).addcmul_(grad, grad, value=1-b2)
        m[i] = mm; v[i] = vv;
        const float mh = mm * c.inv_bc1, vh = sqrtf(vv) * c.inv_bc2_sqrt;
        float u = mh / (vh + c.eps);
        if (c.wd > 0.f) u = u + c.wd * w;
        upd[i] = u;
        atomicAdd(&bins[2 * sg], (double)w * (double)w);
        atomicAdd(&bins[2 * sg + 1], (double)u * (double)u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * LAMB_MAX_SEG; i += blockDim.x)
        if (bins[i] != 0.0) atomicAdd(&seg_sums[i], bins[i]);
}

__global__ __launch_bounds__(256) void k_lamb_apply(float *__restrict__ p, const float *__restrict__ upd,
                                                    const uint8_t *__restrict__ seg, int64_t P, LambC c,
                                                    const double *__restrict__ seg_sums,
                                                    const uint32_t *__restrict__ skip) {
    if (skip && *skip) return;
    __shared__ float trust[LAMB_MAX_SEG];
    for (int i = threadIdx.x; i < LAMB_MAX_SEG; i += blockDim.x) {
        const float wn = (float)sqrt(seg_sums[2 * i]), sn = (float)sqrt(seg_sums[2 * i + 1]);
        float tr = 1.0f;
        if (c.min_trust != 1.0f && wn != 0.f && sn != 0.f) {
            tr = fminf(wn, 10.0f) / sn;
            tr = fminf(fmaxf(tr, c.min_trust), 1.0f / c.min_trust);
        }
        trust[i] = tr;
    }
    __syncthreads();
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = tid; i < P; i += nt) {
        const int sg = seg[i];
        if (sg < LAMB_MAX_SEG) p[i] = p[i] + (-c.lr * trust[sg]) * upd[i];  // p.add_(adam_step, alpha=-lr*trust)
    }
}

extern "C" int sf_lamb_step(float *p, const float *g, float *m, float *v, float *scratch, const uint8_t *seg_id,
                            double *seg_sums, int64_t P, int num_segments, int step, float lr, float beta1, float beta2,
                            float eps, float weight_decay, float min_trust, float max_grad_norm, const double *sumsq,
                            float grad_scale, const uint32_t *skip_flag, void *stream) {
    SF_REQUIRE(p && g && m && v && scratch && seg_id && seg_sums && P > 0 && step >= 1, "sf_lamb_step: bad args");
    SF_REQUIRE(num_segments >= 1 && num_segments <= LAMB_MAX_SEG, "sf_lamb_step: 1..%d segments", LAMB_MAX_SEG);
    LambC c;
    c.inv_bc1 = (float)(1.0 / (1.0 - pow((double)beta1, (double)step)));
    c.inv_bc2_sqrt = (float)(1.0 / sqrt(1.0 - pow((double)beta2, (double)step)));
    c.b1 = beta1; c.w1 = (float)(1.0 - (double)beta1);
    c.b2 = beta2; c.w2 = (float)(1.0 - (double)beta2);
    c.eps = eps; c.wd = weight_decay; c.max_norm = max_grad_norm; c.grad_scale = grad_scale; c.lr = lr;
    c.min_trust = min_trust;
    int rc = sf_hip_status(hipMemsetAsync(seg_sums, 0, 2 * LAMB_MAX_SEG * sizeof(double), STREAM(stream)), "sf_lamb_step");
    if (rc) return rc;
    const int64_t blocks = (P + 255) / 256;
    const dim3 grid((unsigned)(blocks < 1024 ? blocks : 1024));
    k_lamb_dir<<<grid, dim3(256), 0, STREAM(stream)>>>(p, g, m, v, scratch, seg_id, P, c, sumsq, seg_sums, skip_flag);
    k_lamb_apply<<<grid, dim3(256), 0, STREAM(stream)>>>(p, scratch, seg_id, P, c, seg_sums, skip_flag);
    return sf_launch_status("sf_lamb_step");
}

// =========================================================================================== K4/K5 sample + write
template <int MAXA>
__global__ __launch_bounds__(256) void k_sample_write(const float *__restrict__ logits, int ldl,
                                                      const float *__restrict__ values, int ldv, int B, int A, int T, int t,
                                                      uint32_t seed, uint32_t step, uint32_t row0, float version,
                                                      int deterministic, int action_kind,
                                                      float *__restrict__ t_actions,
                                                      float *__restrict__ t_logits, float *__restrict__ t_logp,
                                                      float *__restrict__ t_values, float *__restrict__ t_version,
                                                      int32_t *__restrict__ env_actions) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float *z = logits + (int64_t)b * ldl;
    if (action_kind == 1) {  // Box(D): params = [means | log_std]; a = mu + sd*eps, eps from Box-Muller on Philox
        const int D = A / 2;
        const int64_t it = (int64_t)b * T + t;
        float lp = 0.f;
        for (int k = 0; k < D; ++k) {
            const float eps = box_eps(step, k, 0, seed, row0 + (uint32_t)b);
            const float mu = z[k], sd = box_sd(z[D + k]);
            const float a = deterministic ? mu : mu + sd * eps;  // argmax_actions: the mean (action_distributions.py:78-79)
            t_actions[it * D + k] = a;
            lp += box_logp(a, mu, sd);
        }
        for (int k = 0; k < A; ++k) t_logits[it * A + k] = z[k];
        t_logp[it] = lp;
        t_version[it] = version;
        t_values[(int64_t)b * (T + 1) + t] = values[(int64_t)b * ldv];
        return;
    }
    float zz[MAXA], mx, lse;
    reg_softmax<MAXA>(z, A, zz, mx, lse);
    int a = A - 1;
    if (deterministic) {
        bool found = false;
#pragma unroll
        for (int k = 0; k < MAXA; ++k) if (k < A && !found && zz[k] == mx) { a = k; found = true; }
    } else {
        const float u = cat_uniform(step, 0, seed, row0 + (uint32_t)b);
        float acc = 0.f;
        bool found = false;
        int last_pos = A - 1;  // last action whose probability did not underflow
#pragma unroll
        for (int k = 0; k < MAXA; ++k)
            if (k < A && !found) {
                const float p = expf((zz[k] - mx) - lse);
                acc += p;
                if (p > 0.f) last_pos = k;
                if (u < acc) { a = k; found = true; }
            }
        // the f32 CDF can end a few ulps below 1 and u can reach 1 - 2^-24: take the last action that has any
        // probability, never a zero-probability tail action (torch.multinomial never draws a zero weight)
        if (!found) a = last_pos;
    }
    float lp = 0.f;
#pragma unroll
    for (int k = 0; k < MAXA; ++k) if (k == a) lp = (zz[k] - mx) - lse;
    const int64_t it = (int64_t)b * T + t;
    t_actions[it] = (float)a;
    t_logp[it] = lp;
    t_version[it] = version;
    t_values[(int64_t)b * (T + 1) + t] = values[(int64_t)b * ldv];
#pragma unroll
    for (int k = 0; k < MAXA; ++k) if (k < A) t_logits[it * A + k] = zz[k];
    if (env_actions) env_actions[b] = a;
}

// The four samplers for A > 128, one wave per env row: any head list of up to SF_MAX_ACTION_HEADS members, with or without
// an action mask (mask != nullptr: the rule above k_sample_write_masked per Discrete member, on the member's own mask
// columns).  Same Philox counters, uniforms and draw rule as the lane-per-row samplers.  The CDF is walked 64 columns at a time: an inclusive wave scan of the chunk's
// probabilities plus the carry of the chunks before it, a ballot for the first lane with u < cdf.
__global__ __launch_bounds__(256) void k_sample_write_wide(const float *__restrict__ logits, int ldl,
                                                           const float *__restrict__ values, int ldv,
                                                           const uint8_t *__restrict__ mask, int64_t ldm, int B, int A,
                                                           int T, int t, uint32_t seed, uint32_t step, uint32_t row0,
                                                           float version, int deterministic, HeadsDev hd,
                                                           float *__restrict__ t_actions, float *__restrict__ t_logits,
                                                           float *__restrict__ t_logp, float *__restrict__ t_values,
                                                           float *__restrict__ t_version,
                                                           int32_t *__restrict__ env_actions) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x * WIDE_ROWS + wave;
    if (b >= B) return;
    const float *z = logits + (int64_t)b * ldl;
    const uint8_t *mk = mask ? mask + (int64_t)b * ldm : nullptr;
    const int64_t it = (int64_t)b * T + t;
    const int H = hd.num_heads;
    const int NA = heads_action_cols(hd.head_n, H);
    float lp_sum = 0.f;
    int off = 0, aoff = 0;
    for (int h = 0; h < H; ++h) {
        const int nh = hd.head_n[h];
        if (nh < 0) {  // Box(D) member: a = mu + sd * eps, eps from Box-Muller on Philox counter (step, k / 2, 3, h)
            const int D = -nh;
            float lpp = 0.f;
            for (int k = lane; k < D; k += 64) {
                const float eps = box_eps(step, k, h, seed, row0 + (uint32_t)b);
                const float mu = z[off + k], sd = box_sd(z[off + D + k]);
                const float a = deterministic ? mu : mu + sd * eps;
                t_actions[it * NA + aoff + k] = a;
                lpp += box_logp(a, mu, sd);
            }
            lp_sum += wide_allsum(lpp);
            off += 2 * D; aoff += D;
            continue;
        }
        const float *zh = z + off;
        // the member's slice of the row's mask: mask column c belongs to logits column c (one head: off = 0)
        const uint8_t *mh = mk ? mk + off : nullptr;
        // masked: probs = softmax * mask / (sum + 1e-13), an all-masked member draws from nh weights of 1e-6; the
        // statistics of masked_stats, reduced over the wave
        MaskedStats ms = {0.f, 0.f, 1.f, 1.f, 1.f, false};
        wide_lse(zh, nh, lane, mh, ms.mx, ms.lse);
        const float mx = ms.mx, lse = ms.lse;
        if (mh) {
            float ps = 0.f;
            for (int k = lane; k < nh; k += 64) ps += mh[k] ? expf((zh[k] - mx) - lse) : 0.f;
            ms.psum = wide_allsum(ps);
            ms.all_zero = ms.psum == 0.f;
            ms.inv = 1.0f / (ms.psum + 1e-13f);
            ms.tot = ms.all_zero ? (float)nh * 1e-6f : ms.psum * ms.inv;
        }
        int a;
        if (deterministic) {
            int first = 0x7fffffff;
            if (!mh) {  // first maximum, as torch.argmax
                for (int k = lane; k < nh; k += 64) if (zh[k] == mx) first = min(first, k);
            } else if (ms.all_zero) {
                first = 0;
            } else {  // first maximum of the masked probabilities
                float best = -1.f;
                for (int k = lane; k < nh; k += 64) best = fmaxf(best, masked_p(ms, zh[k], mh[k]));
                best = wide_allmax(best);
                for (int k = lane; k < nh; k += 64) if (masked_p(ms, zh[k], mh[k]) == best) first = min(first, k);
            }
            a = min(wide_allmin(first), nh - 1);  // (no maximum found: NaN logits, out of scope; stay inside the row)
        } else {
            const float u = cat_uniform(step, h, seed, row0 + (uint32_t)b);
            float carry = 0.f;
            int last_pos = -1;  // last action whose probability did not underflow
            a = -1;
            for (int base = 0; base < nh; base += 64) {
                const int k = base + lane;
                float p = 0.f;
                if (k < nh) {
                    if (!mh) p = expf((zh[k] - mx) - lse);
                    else p = masked_p(ms, zh[k], mh[k]) / ms.tot;
                }
                float c = p;
#pragma unroll
                for (int s = 1; s < 64; s <<= 1) {
                    const float up = __shfl_up(c, s, 64);
                    if (lane >= s) c += up;
                }
                c += carry;
                // (the scan adds in a different order per lane: behind a zero p the f32 cdf may sit an ulp ABOVE its
                // neighbour's, so a crossing only counts where there is probability)
                const unsigned long long hit = __ballot(p > 0.f && u < c);
                const unsigned long long pos = __ballot(p > 0.f);
                if (pos) last_pos = base + 63 - __clzll((long long)pos);
                if (hit) { a = base + __ffsll((long long)hit) - 1; break; }
                carry = __shfl(c, 63, 64);
            }
            // the f32 CDF can end a few ulps below 1 and u can reach 1 - 2^-24: take the last action that has any
            // probability, never a zero-probability (underflowed or masked-out) one
            if (a < 0) a = last_pos >= 0 ? last_pos : nh - 1;
        }
        lp_sum += mh ? masked_logp(ms, zh[a], mh[a]) : (zh[a] - mx) - lse;
        if (lane == 0) {
            t_actions[it * NA + aoff] = (float)a;
            if (env_actions) env_actions[(int64_t)b * H + h] = a;  // all-Discrete head lists only (the launchers check)
        }
        off += nh; aoff += 1;
    }
#pragma unroll 4
    for (int k = lane; k < A; k += 64) t_logits[it * A + k] = z[k];
    if (lane == 0) {
        t_logp[it] = lp_sum;
        t_version[it] = version;
        t_values[(int64_t)b * (T + 1) + t] = values[(int64_t)b * ldv];
    }
}

static int sample_write_wide_launch(const char *what, const float *logits, int ld_logits, const float *values,
                                    int ld_values, const uint8_t *mask, int64_t ld_mask, int B, int A, int T, int t,
                                    uint32_t seed, uint32_t step, uint32_t row0, float policy_version, int deterministic,
                                    const HeadsDev &hd, float *traj_actions, float *traj_logits, float *traj_logp,
                                    float *traj_values, float *traj_policy_version, int32_t *env_actions, void *stream) {
    SF_REQUIRE(ld_logits >= A && ld_values >= 1 && (!mask || ld_mask >= A), "%s: bad strides", what);
    k_sample_write_wide<<<dim3((unsigned)((B + WIDE_ROWS - 1) / WIDE_ROWS)), dim3(256), 0, STREAM(stream)>>>(
        logits, ld_logits, values, ld_values, mask, ld_mask, B, A, T, t, seed, step, row0, policy_version, deterministic,
        hd, traj_actions, traj_logits, traj_logp, traj_values, traj_policy_version, env_actions);
    return sf_launch_status(what);
}

extern "C" int sf_sample_write_step(const float *logits, int ld_logits, const float *values, int ld_values, int B,
                                    int A, int T, int t, uint32_t seed, uint32_t step, uint32_t row0, float policy_version,
                                    int deterministic, int action_kind, float *traj_actions, float *traj_logits, float *traj_logp,
                                    float *traj_values, float *traj_policy_version, int32_t *env_actions,
                                    void *stream) {
    SF_REQUIRE(logits && values && traj_actions && traj_logits && traj_logp && traj_values && traj_policy_version,
               "sf_sample_write_step: null pointer");
    SF_REQUIRE(action_kind == 1 || env_actions, "sf_sample_write_step: discrete actions need the int32 env_actions");
    SF_REQUIRE(action_kind == 0 || (action_kind == 1 && A % 2 == 0), "sf_sample_write_step: bad action_kind");
    SF_REQUIRE(B > 0 && A > 0 && T > 0 && t >= 0 && t < T, "sf_sample_write_step: bad shape B=%d A=%d T=%d t=%d",
               B, A, T, t);
    if (A >= WIDE_MIN_A)
        return sample_write_wide_launch("sf_sample_write_step", logits, ld_logits, values, ld_values, nullptr, 0, B, A, T,
                                        t, seed, step, row0, policy_version, deterministic,
                                        single_head(A, action_kind), traj_actions, traj_logits, traj_logp,
                                        traj_values, traj_policy_version, env_actions, stream);
    const dim3 grid((unsigned)((B + 255) / 256)), block(256);
#define SW_LAUNCH(M)                                                                                               \
    k_sample_write<M><<<grid, block, 0, STREAM(stream)>>>(logits, ld_logits, values, ld_values, B, A, T, t, seed, step, row0,            \
                                                          policy_version, deterministic, action_kind, traj_actions, traj_logits, \
                                                          traj_logp, traj_values, traj_policy_version, env_actions)
    if (A <= 8) SW_LAUNCH(8);
    else if (A <= 32) SW_LAUNCH(32);
    else SW_LAUNCH(128);
#undef SW_LAUNCH
    return sf_launch_status("sf_sample_write_step");
}


// Discrete(A) with an action mask (obs["action_mask"], inference_worker.py:324-331; action_distributions.py:84-96,
// 110-142): logits of masked-out actions get -1e9, probs = softmax * mask / (sum + 1e-13), an all-zero row falls back to
// uniform (the reference substitutes 1e-6 everywhere before torch.multinomial), log-prob from the masked log-softmax.
// The RAW logits go to the trajectory (the learner re-evaluates the unmasked distribution, as the reference does).
__global__ __launch_bounds__(256) void k_sample_write_masked(const float *__restrict__ logits, int ldl,
                                                             const float *__restrict__ values, int ldv,
                                                             const uint8_t *__restrict__ mask, int64_t ldm, int B, int A,
                                                             int T, int t, uint32_t seed, uint32_t step, uint32_t row0,
                                                             float version, int deterministic,
                                                             float *__restrict__ t_actions, float *__restrict__ t_logits,
                                                             float *__restrict__ t_logp, float *__restrict__ t_values,
                                                             float *__restrict__ t_version,
                                                             int32_t *__restrict__ env_actions) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float *z = logits + (int64_t)b * ldl;
    const uint8_t *mk = mask + (int64_t)b * ldm;
    const MaskedStats ms = masked_stats(z, mk, A);
    int a = A - 1;
    if (deterministic) {
        float best = -1.f;
        for (int k = 0; k < A; ++k) {
            const float p = masked_p(ms, z[k], mk[k]);
            if (p > best) { best = p; a = k; }
        }
    } else {
        const float u = cat_uniform(step, 0, seed, row0 + (uint32_t)b);
        float acc = 0.f;
        for (int k = 0; k < A; ++k) {
            acc += masked_p(ms, z[k], mk[k]) / ms.tot;
            if (u < acc) { a = k; break; }
        }
        if (!ms.all_zero && !mk[a]) {  // rounding left u beyond the last allowed action: take the last allowed one
            for (int k = A - 1; k >= 0; --k) if (mk[k]) { a = k; break; }
        }
    }
    const int64_t it = (int64_t)b * T + t;
    t_actions[it] = (float)a;
    t_logp[it] = masked_logp(ms, z[a], mk[a]);
    t_version[it] = version;
    t_values[(int64_t)b * (T + 1) + t] = values[(int64_t)b * ldv];
    for (int k = 0; k < A; ++k) t_logits[it * A + k] = z[k];
    if (env_actions) env_actions[b] = a;
}

extern "C" int sf_sample_write_step_masked(const float *logits, int ld_logits, const float *values, int ld_values,
                                           const uint8_t *action_mask, int64_t ld_mask, int B, int A, int T, int t,
                                           uint32_t seed, uint32_t step, uint32_t row0, float policy_version,
                                           int deterministic, float *traj_actions, float *traj_logits, float *traj_logp,
                                           float *traj_values, float *traj_policy_version, int32_t *env_actions,
                                           void *stream) {
    SF_REQUIRE(logits && values && action_mask && traj_actions && traj_logits && traj_logp && traj_values &&
                   traj_policy_version, "sf_sample_write_step_masked: null pointer");
    SF_REQUIRE(B > 0 && A > 0 && T > 0 && t >= 0 && t < T && ld_logits >= A && ld_values >= 1 && ld_mask >= A,
               "sf_sample_write_step_masked: bad shape B=%d A=%d T=%d t=%d", B, A, T, t);
    if (A >= WIDE_MIN_A)
        return sample_write_wide_launch("sf_sample_write_step_masked", logits, ld_logits, values, ld_values, action_mask,
                                        ld_mask, B, A, T, t, seed, step, row0, policy_version, deterministic,
                                        single_head(A, 0), traj_actions, traj_logits, traj_logp, traj_values,
                                        traj_policy_version, env_actions, stream);
    k_sample_write_masked<<<dim3((unsigned)((B + 255) / 256)), dim3(256), 0, STREAM(stream)>>>(
        logits, ld_logits, values, ld_values, action_mask, ld_mask, B, A, T, t, seed, step, row0, policy_version,
        deterministic, traj_actions, traj_logits, traj_logp, traj_values, traj_policy_version, env_actions);
    return sf_launch_status("sf_sample_write_step_masked");
}

// Tuple of Discrete / Box heads, one lane per row: every head is sampled from its own Philox uniform (counter lane 1 =
// head index).  MASKED: the rule above k_sample_write_masked per Discrete member, on the member's slice of the row's
// mask (mask column c belongs to logits column c; the 2 * D columns under a Box(D) member are never read).  The mask
// changes the probabilities, never the uniforms.  The unmasked instantiation has no mask code at all.
template <bool MASKED>
__device__ __forceinline__ void sample_write_tuple_row(const float *__restrict__ z, const uint8_t *__restrict__ mk,
                                                       const float *__restrict__ values, int ldv, int b, int A, int T,
                                                       int t, uint32_t seed, uint32_t step, uint32_t row0, float version,
                                                       int deterministic, const HeadsDev &hd,
                                                       float *__restrict__ t_actions, float *__restrict__ t_logits,
                                                       float *__restrict__ t_logp, float *__restrict__ t_values,
                                                       float *__restrict__ t_version,
                                                       int32_t *__restrict__ env_actions) {
    const int64_t it = (int64_t)b * T + t;
    const int H = hd.num_heads;
    const int NA = heads_action_cols(hd.head_n, H);
    float lp_sum = 0.f;
    int off = 0, aoff = 0;
    for (int h = 0; h < H; ++h) {
        const int nh = hd.head_n[h];
        if (nh < 0) {  // Box(D) member: a = mu + sd * eps
            const int D = -nh;
            for (int k = 0; k < D; ++k) {
                const float eps = box_eps(step, k, h, seed, row0 + (uint32_t)b);
                const float mu = z[off + k], sd = box_sd(z[off + D + k]);
                const float a = deterministic ? mu : mu + sd * eps;
                t_actions[it * NA + aoff + k] = a;
                lp_sum += box_logp(a, mu, sd);
            }
            off += 2 * D; aoff += D;
            continue;
        }
        const float *zh = z + off;
        int a = nh - 1;
        if constexpr (MASKED) {
            const uint8_t *mh = mk + off;
            const MaskedStats ms = masked_stats(zh, mh, nh);
            if (deterministic) {  // first maximum of the masked probabilities (an all-zero slice: nh equal weights, action 0)
                float best = -1.f;
                for (int k = 0; k < nh; ++k) {
                    const float p = masked_p(ms, zh[k], mh[k]);
                    if (p > best) { best = p; a = k; }
                }
            } else {
                const float u = cat_uniform(step, h, seed, row0 + (uint32_t)b);
                float acc = 0.f;
                int last_pos = -1;  // last action with any probability (allowed, not underflowed)
                bool found = false;
                for (int k = 0; k < nh; ++k) {
                    const float p = masked_p(ms, zh[k], mh[k]) / ms.tot;
                    acc += p;
                    if (p > 0.f) last_pos = k;
                    if (u < acc) { a = k; found = true; break; }  // (acc only moves where p > 0: never a masked-out k)
                }
                // rounding left u beyond the last allowed action: take the last allowed one
                if (!found && last_pos >= 0) a = last_pos;
            }
            lp_sum += masked_logp(ms, zh[a], mh[a]);
        } else {
            float mx, lse;
            cat_lse(zh, nh, mx, lse);
            if (deterministic) {
                for (int k = nh - 1; k >= 0; --k) if (zh[k] == mx) a = k;  // first maximum, as torch.argmax
            } else {
                const float u = cat_uniform(step, h, seed, row0 + (uint32_t)b);
                float acc = 0.f;
                int last_pos = nh - 1;
                bool found = false;
                for (int k = 0; k < nh; ++k) {
                    const float p = expf((zh[k] - mx) - lse);
                    acc += p;
                    if (p > 0.f) last_pos = k;
                    if (u < acc) { a = k; found = true; break; }
                }
                if (!found) a = last_pos;  // rounding left u beyond the CDF: the last action with non-zero probability
            }
            lp_sum += (zh[a] - mx) - lse;
        }
        t_actions[it * NA + aoff] = (float)a;
        if (env_actions) env_actions[(int64_t)b * H + h] = a;  // all-Discrete tuples only (the launcher checks)
        off += nh; aoff += 1;
    }
    for (int k = 0; k < A; ++k) t_logits[it * A + k] = z[k];
    t_logp[it] = lp_sum;
    t_version[it] = version;
    t_values[(int64_t)b * (T + 1) + t] = values[(int64_t)b * ldv];
}

__global__ __launch_bounds__(256) void k_sample_write_tuple(const float *__restrict__ logits, int ldl,
                                                            const float *__restrict__ values, int ldv, int B, int A, int T,
                                                            int t, uint32_t seed, uint32_t step, uint32_t row0,
                                                            float version, int deterministic, HeadsDev hd,
                                                            float *__restrict__ t_actions, float *__restrict__ t_logits,
                                                            float *__restrict__ t_logp, float *__restrict__ t_values,
                                                            float *__restrict__ t_version,
                                                            int32_t *__restrict__ env_actions) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    sample_write_tuple_row<false>(logits + (int64_t)b * ldl, nullptr, values, ldv, b, A, T, t, seed, step, row0, version,
                                  deterministic, hd, t_actions, t_logits, t_logp, t_values, t_version, env_actions);
}

__global__ __launch_bounds__(256) void k_sample_write_masked_tuple(const float *__restrict__ logits, int ldl,
                                                                   const float *__restrict__ values, int ldv,
                                                                   const uint8_t *__restrict__ mask, int64_t ldm, int B,
                                                                   int A, int T, int t, uint32_t seed, uint32_t step,
                                                                   uint32_t row0, float version, int deterministic,
                                                                   HeadsDev hd, float *__restrict__ t_actions,
                                                                   float *__restrict__ t_logits, float *__restrict__ t_logp,
                                                                   float *__restrict__ t_values,
                                                                   float *__restrict__ t_version,
                                                                   int32_t *__restrict__ env_actions) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    sample_write_tuple_row<true>(logits + (int64_t)b * ldl, mask + (int64_t)b * ldm, values, ldv, b, A, T, t, seed, step,
                                 row0, version, deterministic, hd, t_actions, t_logits, t_logp, t_values, t_version,
                                 env_actions);
}

// sf_sample_write_step_tuple (action_mask = nullptr) and sf_sample_write_step_tuple_masked: `what` names the entry point
// in the messages.  Every check comes before the launch.
static int sample_write_tuple_launch(const char *what, const float *logits, int ld_logits, const float *values,
                                     int ld_values, const uint8_t *action_mask, int64_t ld_mask, int B, int num_heads,
                                     const int32_t *head_n, int T, int t, uint32_t seed, uint32_t step, uint32_t row0,
                                     float policy_version, int deterministic, float *traj_actions, float *traj_logits,
                                     float *traj_logp, float *traj_values, float *traj_policy_version,
                                     int32_t *env_actions, void *stream) {
    SF_REQUIRE(logits && values && head_n && traj_actions && traj_logits && traj_logp && traj_values &&
                   traj_policy_version, "%s: null pointer", what);
    SF_REQUIRE(B > 0 && T > 0 && t >= 0 && t < T, "%s: bad shape heads=%d B=%d T=%d t=%d", what, num_heads, B, T, t);
    HeadsDev hd = {};
    bool any_box;
    const int A = heads_from_host(what, head_n, num_heads, SF_MAX_ACTION_HEADS, hd.head_n, &any_box);
    if (A < 0) return SF_ERR_ARG;
    hd.num_heads = num_heads;
    SF_REQUIRE(!any_box || !env_actions,
               "%s: a tuple with a Box member has no int32 env_actions (the env reads the trajectory's f32 action row)",
               what);
    SF_REQUIRE(!action_mask || ld_mask >= A,
               "%s: ld_mask=%lld, the mask has one column per distribution parameter (A=%d)", what, (long long)ld_mask, A);
    SF_REQUIRE(ld_logits >= A && ld_values >= 1, "%s: bad strides", what);
    if (A >= WIDE_MIN_A)
        return sample_write_wide_launch(what, logits, ld_logits, values, ld_values, action_mask, ld_mask, B, A, T, t, seed,
                                        step, row0, policy_version, deterministic, hd, traj_actions, traj_logits,
                                        traj_logp, traj_values, traj_policy_version, env_actions, stream);
    const dim3 grid((unsigned)((B + 255) / 256)), block(256);
    if (action_mask)
        k_sample_write_masked_tuple<<<grid, block, 0, STREAM(stream)>>>(
            logits, ld_logits, values, ld_values, action_mask, ld_mask, B, A, T, t, seed, step, row0, policy_version,
            deterministic, hd, traj_actions, traj_logits, traj_logp, traj_values, traj_policy_version, env_actions);
    else
        k_sample_write_tuple<<<grid, block, 0, STREAM(stream)>>>(
            logits, ld_logits, values, ld_values, B, A, T, t, seed, step, row0, policy_version, deterministic, hd,
            traj_actions, traj_logits, traj_logp, traj_values, traj_policy_version, env_actions);
    return sf_launch_status(what);
}

extern "C" int sf_sample_write_step_tuple(const float *logits, int ld_logits, const float *values, int ld_values, int B,
                                          int num_heads, const int32_t *head_n, int T, int t, uint32_t seed,
                                          uint32_t step, uint32_t row0, float policy_version, int deterministic,
                                          float *traj_actions, float *traj_logits, float *traj_logp, float *traj_values,
                                          float *traj_policy_version, int32_t *env_actions, void *stream) {
    return sample_write_tuple_launch("sf_sample_write_step_tuple", logits, ld_logits, values, ld_values, nullptr, 0, B,
                                     num_heads, head_n, T, t, seed, step, row0, policy_version, deterministic, traj_actions,
                                     traj_logits, traj_logp, traj_values, traj_policy_version, env_actions, stream);
}

// sf_sample_write_step_tuple under obs["action_mask"]: u8 [B, A], one column per distribution parameter
extern "C" int sf_sample_write_step_tuple_masked(const float *logits, int ld_logits, const float *values, int ld_values,
                                                 const uint8_t *action_mask, int64_t ld_mask, int B, int num_heads,
                                                 const int32_t *head_n, int T, int t, uint32_t seed, uint32_t step,
                                                 uint32_t row0, float policy_version, int deterministic,
                                                 float *traj_actions, float *traj_logits, float *traj_logp,
                                                 float *traj_values, float *traj_policy_version, int32_t *env_actions,
                                                 void *stream) {
    SF_REQUIRE(action_mask, "sf_sample_write_step_tuple_masked: null action_mask");
    return sample_write_tuple_launch("sf_sample_write_step_tuple_masked", logits, ld_logits, values, ld_values, action_mask,
                                     ld_mask, B, num_heads, head_n, T, t, seed, step, row0, policy_version, deterministic,
                                     traj_actions, traj_logits, traj_logp, traj_values, traj_policy_version, env_actions,
                                     stream);
}

// =========================================================================================== K1/K6 env step -> traj
// one thread per agent row b; pid: the policy id THIS row records (the is_active kernel below passes -1 for some rows)
__device__ __forceinline__ void traj_write_env_row(const float *__restrict__ rewards,
                                                   const uint8_t *__restrict__ terminated,
                                                   const uint8_t *__restrict__ truncated, int B, int T, int t,
                                                   float scale, float clip, int pid, float *__restrict__ t_rewards,
                                                   uint8_t *__restrict__ t_dones, uint8_t *__restrict__ t_timeouts,
                                                   int32_t *__restrict__ t_pid, float *__restrict__ ep_ret,
                                                   int32_t *__restrict__ ep_len, double *__restrict__ ep_stats,
                                                   double *lds) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    double acc[3] = {0.0, 0.0, 0.0};
    if (b < B) {
        const float raw = rewards[b];
        const bool term = terminated[b] != 0, trunc = truncated ? truncated[b] != 0 : false;
        const bool done = term || trunc;
        const int64_t it = (int64_t)b * T + t;
        t_rewards[it] = clampf(raw * scale, -clip, clip);  // batched_sampling.py:208-213
        t_dones[it] = (uint8_t)done;
        t_timeouts[it] = (uint8_t)trunc;
        t_pid[it] = pid;
        if (ep_ret) {
            const float r = ep_ret[b] + raw;  // episode stats use the raw reward (batched_sampling.py:216-219)
            const int l = ep_len[b] + 1;
            if (done) { acc[0] = r; acc[1] = (double)l; acc[2] = 1.0; ep_ret[b] = 0.f; ep_len[b] = 0; }
            else { ep_ret[b] = r; ep_len[b] = l; }
        }
    }
    if (ep_stats) {
        sf_block_sum<3>(acc, lds);
        if (threadIdx.x == 0 && acc[2] > 0.0) {
            atomicAdd(&ep_stats[0], acc[0]);
            atomicAdd(&ep_stats[1], acc[1]);
            atomicAdd(&ep_stats[2], acc[2]);
        }
    }
}

__global__ __launch_bounds__(256) void k_traj_write_env(const float *__restrict__ rewards,
                                                        const uint8_t *__restrict__ terminated,
                                                        const uint8_t *__restrict__ truncated, int B, int T, int t,
                                                        float scale, float clip, int pid,
                                                        float *__restrict__ t_rewards, uint8_t *__restrict__ t_dones,
                                                        uint8_t *__restrict__ t_timeouts, int32_t *__restrict__ t_pid,
                                                        float *__restrict__ ep_ret, int32_t *__restrict__ ep_len,
                                                        double *__restrict__ ep_stats) {
    __shared__ double lds[4 * 3];
    traj_write_env_row(rewards, terminated, truncated, B, T, t, scale, clip, pid, t_rewards, t_dones, t_timeouts, t_pid,
                       ep_ret, ep_len, ep_stats, lds);
}

// the same step for envs that report info["is_active"]: a row the env declared inactive at its PREVIOUS step records
// policy_id -1 (the learner's validity mask drops it), then the row's byte takes what the env reported with this step
// (non_batched_sampling.py:82-84, 197-203).  The thread that owns row b is the only one that touches active[b].
__global__ __launch_bounds__(256) void k_traj_write_env_active(
    const float *__restrict__ rewards, const uint8_t *__restrict__ terminated, const uint8_t *__restrict__ truncated, int B,
    int T, int t, float scale, float clip, int pid, float *__restrict__ t_rewards, uint8_t *__restrict__ t_dones,
    uint8_t *__restrict__ t_timeouts, int32_t *__restrict__ t_pid, float *__restrict__ ep_ret,
    int32_t *__restrict__ ep_len, double *__restrict__ ep_stats, const uint8_t *__restrict__ active_in,
    uint8_t *__restrict__ active) {
    __shared__ double lds[4 * 3];
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) {
        if (!active[b]) pid = -1;
        active[b] = (uint8_t)(active_in[b] != 0);
    }
    traj_write_env_row(rewards, terminated, truncated, B, T, t, scale, clip, pid, t_rewards, t_dones, t_timeouts, t_pid,
                       ep_ret, ep_len, ep_stats, lds);
}

extern "C" int sf_traj_write_env_step(const float *rewards, const uint8_t *terminated, const uint8_t *truncated, int B,
                                      int T, int t, float reward_scale, float reward_clip, int policy_id,
                                      float *traj_rewards, uint8_t *traj_dones, uint8_t *traj_time_outs,
                                      int32_t *traj_policy_id, float *ep_return, int32_t *ep_len, double *ep_stats,
                                      void *stream) {
    SF_REQUIRE(rewards && terminated && traj_rewards && traj_dones && traj_time_outs && traj_policy_id,
               "sf_traj_write_env_step: null pointer");
    SF_REQUIRE(B > 0 && T > 0 && t >= 0 && t < T, "sf_traj_write_env_step: bad shape");
    SF_REQUIRE((ep_return == nullptr) == (ep_len == nullptr), "sf_traj_write_env_step: ep_return/ep_len mismatch");
    k_traj_write_env<<<dim3((unsigned)((B + 255) / 256)), dim3(256), 0, STREAM(stream)>>>(
        rewards, terminated, truncated, B, T, t, reward_scale, reward_clip, policy_id, traj_rewards, traj_dones,
        traj_time_outs, traj_policy_id, ep_return, ep_len, ep_stats);
    return sf_launch_status("sf_traj_write_env_step");
}

extern "C" int sf_traj_write_env_step_active(const float *rewards, const uint8_t *terminated, const uint8_t *truncated,
                                             int B, int T, int t, float reward_scale, float reward_clip, int policy_id,
                                             float *traj_rewards, uint8_t *traj_dones, uint8_t *traj_time_outs,
                                             int32_t *traj_policy_id, float *ep_return, int32_t *ep_len,
                                             double *ep_stats, const uint8_t *active_in, uint8_t *active_state,
                                             void *stream) {
    SF_REQUIRE(rewards && terminated && traj_rewards && traj_dones && traj_time_outs && traj_policy_id,
               "sf_traj_write_env_step_active: null pointer");
    SF_REQUIRE(active_in && active_state, "sf_traj_write_env_step_active: null active_in / active_state");
    SF_REQUIRE(B > 0 && T > 0 && t >= 0 && t < T, "sf_traj_write_env_step_active: bad shape");
    SF_REQUIRE(active_in + B <= active_state || active_state + B <= active_in,
               "sf_traj_write_env_step_active: active_in aliases active_state");
    SF_REQUIRE((ep_return == nullptr) == (ep_len == nullptr), "sf_traj_write_env_step_active: ep_return/ep_len mismatch");
    k_traj_write_env_active<<<dim3((unsigned)((B + 255) / 256)), dim3(256), 0, STREAM(stream)>>>(
        rewards, terminated, truncated, B, T, t, reward_scale, reward_clip, policy_id, traj_rewards, traj_dones,
        traj_time_outs, traj_policy_id, ep_return, ep_len, ep_stats, active_in, active_state);
    return sf_launch_status("sf_traj_write_env_step_active");
}

// =========================================================================================== synthetic env
__global__ __launch_bounds__(256) void k_synth_obs(uint8_t *__restrict__ obs, int64_t env_stride, int B, int env0,
                                                   int64_t blocks_per_env, uint32_t seed, uint32_t step) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (int64_t)B * blocks_per_env) return;
    const int64_t e = gid / blocks_per_env, blk = gid - e * blocks_per_env;
    uint32_t w[4];
    sf_philox4x32_10(step, (uint32_t)blk, 0u, 0u, seed, (uint32_t)(env0 + e), w);
    *reinterpret_cast<uint4 *>(obs + e * env_stride + blk * 16) = make_uint4(w[0], w[1], w[2], w[3]);
}

extern "C" int sf_synth_obs(uint8_t *obs, int64_t env_stride, int B, int env0, int64_t obs_bytes, uint32_t seed,
                            uint32_t step, void *stream) {
    SF_REQUIRE(obs && B > 0 && obs_bytes > 0 && obs_bytes % 16 == 0 && env_stride % 16 == 0 &&
                   ((uintptr_t)obs & 15) == 0,
               "sf_synth_obs: obs_bytes/env_stride/base must be multiples of 16");
    const int64_t total = (int64_t)B * (obs_bytes / 16);
    k_synth_obs<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, STREAM(stream)>>>(obs, env_stride, B, env0,
                                                                                         obs_bytes / 16, seed, step);
    return sf_launch_status("sf_synth_obs");
}

__global__ __launch_bounds__(256) void k_synth_step(const int32_t *__restrict__ actions, int B, int env0,
                                                    int num_actions, uint32_t seed, uint32_t step,
                                                    float *__restrict__ rewards, uint8_t *__restrict__ terminated) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const uint32_t env = (uint32_t)(env0 + b);
    rewards[b] = (actions[b] == (int32_t)((step + env) % (uint32_t)num_actions)) ? 1.0f : 0.0f;
    uint32_t w[4];
    sf_philox4x32_10(step, 0u, 1u, 0u, seed, env, w);
    terminated[b] = (uint8_t)(w[0] < (1u << 22));
}

extern "C" int sf_synth_step(const int32_t *actions, int B, int env0, int num_actions, uint32_t seed, uint32_t step,
                             float *rewards, uint8_t *terminated, void *stream) {
    SF_REQUIRE(actions && rewards && terminated && B > 0 && num_actions > 0, "sf_synth_step: bad args");
    k_synth_step<<<dim3((unsigned)((B + 255) / 256)), dim3(256), 0, STREAM(stream)>>>(actions, B, env0, num_actions,
                                                                                      seed, step, rewards, terminated);
    return sf_launch_status("sf_synth_step");
}

// ---- Ant-shaped continuous synthetic env (SURVEY.md §8d C5 stand-in), one lane per env:
// obs' = terminated ? noise : 0.9 * obs + 0.1 * noise, reward = -mean(a^2) + 0.1 * obs[0], terminated ~ Bernoulli(1/256);
// noise ~ N(0, 1) from Philox4x32-10 keyed by (seed, env), counter (step, block) via Box-Muller.  `state` is the env's
// own copy of the observation; `obs_out` (row stride out_stride floats) is slot t+1 of the trajectory slab.
__device__ __forceinline__ void synth_normals(uint32_t seed, uint32_t env, uint32_t step, uint32_t blk, float (&z)[4]) {
    uint32_t w[4];
    sf_philox4x32_10(step, blk, 2u, 0u, seed, env, w);
    const float u0 = ((float)(w[0] >> 8) + 0.5f) * (1.0f / 16777216.0f), u1 = (float)(w[1] >> 8) * (1.0f / 16777216.0f);
    const float u2 = ((float)(w[2] >> 8) + 0.5f) * (1.0f / 16777216.0f), u3 = (float)(w[3] >> 8) * (1.0f / 16777216.0f);
    const float r0 = sqrtf(-2.0f * logf(u0)), r1 = sqrtf(-2.0f * logf(u2));
    z[0] = r0 * cosf(6.2831853f * u1); z[1] = r0 * sinf(6.2831853f * u1);
    z[2] = r1 * cosf(6.2831853f * u3); z[3] = r1 * sinf(6.2831853f * u3);
}

// one lane per (env, block of 4 observation dims): 7 lanes per env at D = 27
__global__ __launch_bounds__(256) void k_synth_vec_step(float *__restrict__ state, const float *__restrict__ actions,
                                                        int64_t act_stride, float *__restrict__ obs_out, int64_t out_stride,
                                                        int B, int D, int A, int env0, uint32_t seed, uint32_t step,
                                                        int reset, float *__restrict__ rewards,
                                                        uint8_t *__restrict__ terminated) {
    const int nblk = (D + 3) >> 2;
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= B * nblk) return;
    const int b = gid / nblk, blk = gid - b * nblk, d0 = blk * 4;
    const uint32_t env = (uint32_t)(env0 + b);
    float *st = state + (int64_t)b * D, *out = obs_out + (int64_t)b * out_stride;
    bool term = reset != 0;
    if (!reset) {
        uint32_t w[4];
        sf_philox4x32_10(step, 0u, 1u, 0u, seed, env, w);  // (every lane of the env draws the same word)
        term = w[0] < (1u << 24);  // 1/256
        if (blk == 0) {
            float sq = 0.0f;
            for (int a = 0; a < A; ++a) {
                const float v = actions[(int64_t)b * act_stride + a];
                sq += v * v;
            }
            rewards[b] = -(sq / (float)A) + 0.1f * st[0];
            terminated[b] = (uint8_t)term;
        }
    }
    float z[4];
    synth_normals(seed, env, step, (uint32_t)blk, z);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (d0 + k < D) {
            const float v = term ? z[k] : 0.9f * st[d0 + k] + 0.1f * z[k];
            st[d0 + k] = v;
            out[d0 + k] = v;
        }
    }
}

extern "C" int sf_synth_vec_step(float *state, const float *actions, int64_t act_stride, float *obs_out, int64_t out_stride,
                                 int B, int D, int A, int env0, uint32_t seed, uint32_t step, int reset, float *rewards,
                                 uint8_t *terminated, void *stream) {
    SF_REQUIRE(state && obs_out && B > 0 && D > 0 && (reset || (actions && rewards && terminated && A > 0)),
               "sf_synth_vec_step: bad args");
    const int64_t lanes = (int64_t)B * ((D + 3) / 4);
    k_synth_vec_step<<<dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, STREAM(stream)>>>(
        state, actions, act_stride, obs_out, out_stride, B, D, A, env0, seed, step, reset, rewards, terminated);
    return sf_launch_status("sf_synth_vec_step");
}

// =========================================================================================== observation normaliser
// utils/normalize.py:24-70 (ObservationNormalizer) + running_mean_std.py:22-136 (RunningMeanStd(Dict)InPlace with
// full-shape statistics): x' = (float(x) - obs_subtract_mean) * (1/obs_scale); per-element running mean/var/count
// (f64, Chan merge); normalised = clamp((x' - mu) * (1/sqrt(var + 1e-5)), +-5).
// Sample addressing is the same as the network kernels': logical sample i -> row (index ? index[i] : offset + i),
// optionally mapped dataset->slab (e*T+t -> e*(T+1)+t), times `stride` elements.
__device__ __forceinline__ int64_t on_row(const int32_t *__restrict__ index, int64_t offset, int traj_T, int64_t i) {
    int64_t d = index ? (int64_t)index[i] : offset + i;
    if (traj_T > 0) d += d / traj_T;
    return d;
}

template <bool U8>
__global__ __launch_bounds__(256) void k_obsnorm_moments(const void *__restrict__ in, int64_t stride,
                                                         const int32_t *__restrict__ index, int64_t offset, int traj_T,
                                                         int64_t n, int D, float sub_mean, float inv_scale,
                                                         double *__restrict__ sum, double *__restrict__ sumsq) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= D) return;
    const int64_t per = (n + gridDim.y - 1) / gridDim.y;
    const int64_t beg = (int64_t)blockIdx.y * per, end = (beg + per < n) ? beg + per : n;
    double s = 0.0, ss = 0.0;
    for (int64_t i = beg; i < end; ++i) {
        const int64_t row = on_row(index, offset, traj_T, i);
        const float raw = U8 ? (float)reinterpret_cast<const uint8_t *>(in)[row * stride + d]
                             : reinterpret_cast<const float *>(in)[row * stride + d];
        const double x = (double)((raw - sub_mean) * inv_scale);
        s += x;
        ss += x * x;
    }
    atomicAdd(&sum[d], s);
    atomicAdd(&sumsq[d], ss);
}

extern "C" int sf_obsnorm_moments(const void *in, int in_u8, int64_t stride, const int32_t *index, int64_t offset,
                                  int traj_T, int64_t n, int D, float sub_mean, float inv_scale, double *sum,
                                  double *sumsq, void *stream) {
    SF_REQUIRE(in && sum && sumsq && n > 0 && D > 0, "sf_obsnorm_moments: bad args");
    int rc = sf_hip_status(hipMemsetAsync(sum, 0, sizeof(double) * D, STREAM(stream)), "sf_obsnorm_moments memset");
    if (!rc) rc = sf_hip_status(hipMemsetAsync(sumsq, 0, sizeof(double) * D, STREAM(stream)), "sf_obsnorm_moments memset");
    if (rc) return rc;
    const unsigned bx = (unsigned)((D + 255) / 256);
    unsigned by = (unsigned)(4096 / bx);
    if (by < 1) by = 1;
    if ((int64_t)by > n) by = (unsigned)n;
    if (in_u8) k_obsnorm_moments<true><<<dim3(bx, by), dim3(256), 0, STREAM(stream)>>>(in, stride, index, offset, traj_T, n, D, sub_mean, inv_scale, sum, sumsq);
    else k_obsnorm_moments<false><<<dim3(bx, by), dim3(256), 0, STREAM(stream)>>>(in, stride, index, offset, traj_T, n, D, sub_mean, inv_scale, sum, sumsq);
    return sf_launch_status("sf_obsnorm_moments");
}

// stats: mean[D], var[D] (f64), count[1] (f64); batch moments {sum, sumsq}[D] over n samples -> merged stats (in
// place; count advanced by the launch with blockIdx 0) and the derived f32 tables mu[D], rstd[D] the apply kernel uses.
__global__ __launch_bounds__(256) void k_obsnorm_update(double *__restrict__ mean, double *__restrict__ var,
                                                        const double *__restrict__ count_in,
                                                        double *__restrict__ count_out, const double *__restrict__ sum,
                                                        const double *__restrict__ sumsq, double n, int D,
                                                        float *__restrict__ mu_tab, float *__restrict__ rstd_tab) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    const double count = count_in[0];
    if (d < D) {
        double m = mean[d], v = var[d];
        if (n > 0.0) {
            const double bm64 = sum[d] / n;
            const double bv64 = (sumsq[d] - sum[d] * bm64) / (n - 1.0);
            const double bm = (double)(float)bm64, bv = (double)(float)bv64;  // x.mean(0), x.var(0) are f32 tensors
            const double delta = bm - m, tot = count + n;
            const double M2 = v * count + bv * n + (delta * delta) * count * n / tot;
            m = m + delta * n / tot;
            v = M2 / tot;
            mean[d] = m;
            var[d] = v;
        }
        mu_tab[d] = (float)m;
        rstd_tab[d] = 1.0f / sqrtf((float)v + 1e-5f);
    }
    if (d == 0) count_out[0] = count + n;
}

extern "C" int sf_obsnorm_update(double *mean, double *var, const double *count_in, double *count_out,
                                 const double *sum, const double *sumsq, int64_t n, int D, float *mu_tab,
                                 float *rstd_tab, void *stream) {
    SF_REQUIRE(mean && var && count_in && count_out && mu_tab && rstd_tab && D > 0 && n >= 0 && (n == 0 || (sum && sumsq)),
               "sf_obsnorm_update: bad args");
    SF_REQUIRE(count_in != count_out, "sf_obsnorm_update: count_in and count_out must be different buffers");
    k_obsnorm_update<<<dim3((unsigned)((D + 255) / 256)), dim3(256), 0, STREAM(stream)>>>(
        mean, var, count_in, count_out, sum, sumsq, (double)n, D, mu_tab, rstd_tab);
    return sf_launch_status("sf_obsnorm_update");
}

// out[i][pos] = clamp(((x - sub_mean)*inv_scale - mu[d]) * rstd[d], +-5); images (C,H,W given, C>0): d = c*HW + p is
// written channels-last at pos = p*C + c (the layout the conv kernels read); vectors (C == 0): pos = d.
template <bool U8>
__global__ __launch_bounds__(256) void k_obsnorm_apply(const void *__restrict__ in, int64_t stride,
                                                       const int32_t *__restrict__ index, int64_t offset, int traj_T,
                                                       int64_t n, int D, int C, int HW, float sub_mean,
                                                       float inv_scale, const float *__restrict__ mu,
                                                       const float *__restrict__ rstd, float *__restrict__ out) {
    const int64_t total = n * D;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = g / D;
        const int pos = (int)(g - i * D);
        int d = pos;
        if (C > 0) { const int p = pos / C, c = pos - p * C; d = c * HW + p; }
        const int64_t row = on_row(index, offset, traj_T, i);
        const float raw = U8 ? (float)reinterpret_cast<const uint8_t *>(in)[row * stride + d]
                             : reinterpret_cast<const float *>(in)[row * stride + d];
        const float x = (raw - sub_mean) * inv_scale;
        out[g] = clampf((x - mu[d]) * rstd[d], -5.0f, 5.0f);
    }
}

extern "C" int sf_obsnorm_apply(const void *in, int in_u8, int64_t stride, const int32_t *index, int64_t offset,
                                int traj_T, int64_t n, int D, int C, int HW, float sub_mean, float inv_scale,
                                const float *mu, const float *rstd, float *out, void *stream) {
    SF_REQUIRE(in && mu && rstd && out && n > 0 && D > 0, "sf_obsnorm_apply: bad args");
    SF_REQUIRE(C == 0 || C * HW == D, "sf_obsnorm_apply: C*HW != D");
    const int64_t blocks = (n * D + 255) / 256;
    const unsigned grid = (unsigned)(blocks < 65536 ? blocks : 65536);
    if (in_u8) k_obsnorm_apply<true><<<dim3(grid), dim3(256), 0, STREAM(stream)>>>(in, stride, index, offset, traj_T, n, D, C, HW, sub_mean, inv_scale, mu, rstd, out);
    else k_obsnorm_apply<false><<<dim3(grid), dim3(256), 0, STREAM(stream)>>>(in, stride, index, offset, traj_T, n, D, C, HW, sub_mean, inv_scale, mu, rstd, out);
    return sf_launch_status("sf_obsnorm_apply");
}

// =========================================================================================== fused small MLP encoder
// Inference on VECTOR observations (model/encoder.py:72-87 MlpEncoder behind utils/normalize.py:24-70): input
// normalisation -> Linear(D, H1) + act -> Linear(H1, H2) + act in ONE launch.  At rollout sizes (2048 envs x 27 floats)
// each of these layers is a 13 us MFMA-kernel launch doing 7 MFLOP; here a 256-thread block takes 16 samples, keeps both
// weight matrices in LDS and each thread produces 4 columns of one row with fmaf chains in ascending k — the same
// arithmetic (bit for bit) as the exact-f32 MFMA kernels, which the training pass keeps using (it needs the
// intermediate activations).
__device__ __forceinline__ float mlp_act(float x, int kind) {
    if (kind == 1) return fmaxf(x, 0.f);
    if (kind == 2) return tanhf(x);
    if (kind == 3) return x > 0.f ? x : expm1f(x);
    return x;
}

constexpr int MLP2_ROWS = 16;  // samples per block (2048 envs: 128 blocks); a thread owns 1 row x 4 columns

__global__ __launch_bounds__(256) void k_mlp2_fwd(const float *__restrict__ x, int64_t x_stride, int64_t n, int D,
                                                  float sub_mean, float inv_scale, const float *__restrict__ mu,
                                                  const float *__restrict__ rstd, const float *__restrict__ w1,
                                                  const float *__restrict__ b1, int H1, const float *__restrict__ w2,
                                                  const float *__restrict__ b2, int H2, int act,
                                                  float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *sw1 = sm, *sw2 = sw1 + D * H1, *sx = sw2 + H1 * H2, *sh = sx + MLP2_ROWS * D;  // sh: [ROWS][H1]
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * MLP2_ROWS;
    // every global load of the prologue is issued before the first LDS store (a load -> store loop waits for each load
    // in turn: 30 serialised round trips were 14 of the first version's 18 us)
    {
        constexpr int NV = 8;  // float4s per thread and matrix: up to 8192 weights each (checked by the launcher)
        float4 v1[NV], v2[NV];
        const int n1 = D * H1 / 4, n2 = H1 * H2 / 4;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int q1 = tid + 256 * i, q2 = tid + 256 * i;
            v1[i] = reinterpret_cast<const float4 *>(w1)[q1 < n1 ? q1 : 0];
            v2[i] = reinterpret_cast<const float4 *>(w2)[q2 < n2 ? q2 : 0];
        }
        constexpr int NX = 4;  // observation words per thread: up to 16 rows x 64 values
        float xv[NX];
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            const int q = tid + 256 * i;
            const int qq = q < MLP2_ROWS * D ? q : 0;
            const int r = qq / D, d = qq - r * D;
            const int64_t row = r0 + r < n ? r0 + r : n - 1;
            float v = (x[row * x_stride + d] - sub_mean) * inv_scale;
            if (mu) v = fminf(fmaxf((v - mu[d]) * rstd[d], -5.0f), 5.0f);
            xv[i] = v;
        }
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int q = tid + 256 * i;
            if (q < n1) reinterpret_cast<float4 *>(sw1)[q] = v1[i];
            if (q < n2) reinterpret_cast<float4 *>(sw2)[q] = v2[i];
        }
#pragma unroll
        for (int i = 0; i < NX; ++i) {
            const int q = tid + 256 * i;
            if (q < MLP2_ROWS * D) sx[q] = xv[i];
        }
    }
    __syncthreads();
    const int ra = tid >> 4, cg = tid & 15;
    auto layer = [&](const float *in, int K, const float *w, const float *bias, int N, float *dst, int64_t dst_ld,
                     bool to_global) {
        for (int c0 = cg * 4; c0 < N; c0 += 64) {  // 4 consecutive columns per pass
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
            for (int k = 0; k < K; ++k) {  // ascending k, one fmaf chain per output element (= the MFMA kernels' sums)
                const float a = in[ra * K + k];
                const float4 wv = *reinterpret_cast<const float4 *>(w + k * N + c0);
                acc[0] = fmaf(a, wv.x, acc[0]);
                acc[1] = fmaf(a, wv.y, acc[1]);
                acc[2] = fmaf(a, wv.z, acc[2]);
                acc[3] = fmaf(a, wv.w, acc[3]);
            }
            if (!to_global || r0 + ra < n) {
                float4 o;
                o.x = mlp_act(acc[0] + bias[c0], act);
                o.y = mlp_act(acc[1] + bias[c0 + 1], act);
                o.z = mlp_act(acc[2] + bias[c0 + 2], act);
                o.w = mlp_act(acc[3] + bias[c0 + 3], act);
                *reinterpret_cast<float4 *>(dst + (to_global ? r0 + ra : ra) * dst_ld + c0) = o;
            }
        }
    };
    layer(sx, D, sw1, b1, H1, sh, H1, false);
    __syncthreads();
    layer(sh, H1, sw2, b2, H2, out, H2, true);
}

extern "C" int sf_mlp2_fwd(const float *x, int64_t x_stride, int64_t n, int D, float sub_mean, float inv_scale,
                           const float *mu, const float *rstd, const float *w1, const float *b1, int H1, const float *w2,
                           const float *b2, int H2, int act, float *out, void *stream) {
    SF_REQUIRE(x && w1 && b1 && w2 && b2 && out && n > 0 && D > 0, "sf_mlp2_fwd: bad args");
    SF_REQUIRE(H1 > 0 && H2 > 0 && H1 % 8 == 0 && H2 % 8 == 0 && (mu == nullptr) == (rstd == nullptr),
               "sf_mlp2_fwd: layer widths must be multiples of 8 (H1=%d H2=%d)", H1, H2);
    const size_t lds = sizeof(float) * ((size_t)D * H1 + (size_t)H1 * H2 + MLP2_ROWS * (size_t)(D + H1));
    SF_REQUIRE(lds <= 64 * 1024 && D <= 64 && D * H1 <= 8192 && H1 * H2 <= 8192 && ((uintptr_t)w1 & 15) == 0 && ((uintptr_t)w2 & 15) == 0 &&
                   ((uintptr_t)out & 15) == 0,
               "sf_mlp2_fwd: D=%d H1=%d H2=%d exceed the fused kernel (use the layer kernels)", D, H1, H2);
    k_mlp2_fwd<<<dim3((unsigned)((n + MLP2_ROWS - 1) / MLP2_ROWS)), dim3(256), lds, STREAM(stream)>>>(x, x_stride, n, D, sub_mean, inv_scale, mu,
                                                                                   rstd, w1, b1, H1, w2, b2, H2, act, out);
    return sf_launch_status("sf_mlp2_fwd");
}

// =========================================================================================== recurrent core cells
// model/core.py:19-64 (ModelCoreRNN = torch.nn.GRU / nn.LSTM, one layer) as explicit cell kernels; the projections
// (x W_ih^T + b_ih, h W_hh^T + b_hh) are the MFMA linear kernels, these are the elementwise halves.  BPTT runs as a
// time loop over recurrence-length chunks with the state zeroed after a done/invalid step — the loop form that the
// reference's own test (tests/algo/test_rnn.py) proves equal to its PackedSequence path (rnn_utils.py:114-158).
// kind 0 = GRU (gates r,z,n), 1 = LSTM (gates i,f,g,o).  All matrices row-major; h_prev/c_prev may be strided rows.
// The cell expressions themselves live in sf_rnn_cell.h, shared with the row-owned sequence passes of sf_rnn.hip.
#include "sf_rnn_cell.h"

// gates_out [C, 4H]: GRU stores {r, z, n, hn = (W_hn h + b_hn)}; LSTM stores {i, f, g, o}.
// h_out/c_out: the new state (core output); h_next/c_next = state * keep[c] (keep = 1 - done_or_invalid; NULL = 1).
__global__ __launch_bounds__(256) void k_rnn_cell_fwd(int kind, const float *__restrict__ gx,
                                                      const float *__restrict__ gh, const float *__restrict__ h_prev,
                                                      int64_t ld_h, const float *__restrict__ c_prev, int64_t ld_c,
                                                      const float *__restrict__ keep, int C, int H,
                                                      float *__restrict__ gates_out, float *__restrict__ h_out,
                                                      float *__restrict__ c_out, float *__restrict__ h_next,
                                                      float *__restrict__ c_next) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)C * H) return;
    const int64_t c = i / H;
    const int j = (int)(i - c * H);
    const float k = keep ? keep[c] : 1.0f;
    if (kind == 0) {
        const float hp = h_prev[c * ld_h + j];
        float r_pre, z_pre, hn, xn;
        if (gh) {
            const float *x = gx + c * 3 * H, *g = gh + c * 3 * H;
            r_pre = x[j] + g[j];
            z_pre = x[H + j] + g[H + j];
            hn = g[2 * H + j];
            xn = x[2 * H + j];
        } else {  // gx [C, 4H] = {r_pre, z_pre (x and h parts summed), x W_in^T + b_in, h W_hn^T + b_hn} (sf_linear_fwd_dual)
            const float *x = gx + c * 4 * H;
            r_pre = x[j];
            z_pre = x[H + j];
            xn = x[2 * H + j];
            hn = x[3 * H + j];
        }
        float r, z, n, h;
        sf_gru_cell_fwd(r_pre, z_pre, xn, hn, hp, r, z, n, h);
        if (gates_out) {
            float *go = gates_out + c * 4 * H;
            go[j] = r; go[H + j] = z; go[2 * H + j] = n; go[3 * H + j] = hn;
        }
        h_out[i] = h;
        if (h_next) h_next[i] = h * k;
    } else {
        const float *x = gx + c * 4 * H;
        const float cp = c_prev[c * ld_c + j];
        float pre[4];
        if (gh) {
            const float *g = gh + c * 4 * H;
#pragma unroll
            for (int q = 0; q < 4; ++q) pre[q] = x[q * H + j] + g[q * H + j];
        } else {  // gx already holds x W_ih^T + b_ih + h W_hh^T + b_hh (sf_linear_fwd_dual)
#pragma unroll
            for (int q = 0; q < 4; ++q) pre[q] = x[q * H + j];
        }
        float ig, fg, gg, og, cn, h;
        sf_lstm_cell_fwd(pre[0], pre[1], pre[2], pre[3], cp, ig, fg, gg, og, cn, h);
        if (gates_out) {
            float *go = gates_out + c * 4 * H;
            go[j] = ig; go[H + j] = fg; go[2 * H + j] = gg; go[3 * H + j] = og;
        }
        h_out[i] = h;
        c_out[i] = cn;
        if (h_next) h_next[i] = h * k;
        if (c_next) c_next[i] = cn * k;
    }
}

extern "C" int sf_rnn_cell_fwd(int kind, const float *gx, const float *gh, const float *h_prev, int64_t ld_h,
                               const float *c_prev, int64_t ld_c, const float *keep, int C, int H, float *gates_out,
                               float *h_out, float *c_out, float *h_next, float *c_next, void *stream) {
    SF_REQUIRE((kind == 0 || kind == 1) && gx && h_prev && h_out && C > 0 && H > 0, "sf_rnn_cell_fwd: bad args");
    SF_REQUIRE(kind == 0 || (c_prev && c_out), "sf_rnn_cell_fwd: LSTM needs c_prev and c_out");
    const int64_t n = (int64_t)C * H;
    k_rnn_cell_fwd<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, STREAM(stream)>>>(
        kind, gx, gh, h_prev, ld_h, c_prev, ld_c, keep, C, H, gates_out, h_out, c_out, h_next, c_next);
    return sf_launch_status("sf_rnn_cell_fwd");
}

// backward of one step.  dh [C,H] = gradient wrt this step's h_out (output gradient + carry from t+1, already
// masked); dc_in = carry into c_out (LSTM; NULL = 0).  Outputs: dgx [C,G*H] (gradient wrt x W_ih^T + b_ih),
// dgh [C,G*H] (wrt h W_hh^T + b_hh; LSTM: may alias dgx or be NULL since both are equal), dh_direct [C,H] (the part
// of dL/dh_prev that does not go through W_hh; GRU: dh*z, LSTM: 0 -> not written), dc_prev [C,H] (LSTM: dc*f).
__global__ __launch_bounds__(256) void k_rnn_cell_bwd(int kind, const float *__restrict__ dh,
                                                      const float *__restrict__ dc_in,
                                                      const float *__restrict__ gates, const float *__restrict__ h_prev,
                                                      int64_t ld_h, const float *__restrict__ c_prev, int64_t ld_c,
                                                      const float *__restrict__ c_out, int C, int H,
                                                      float *__restrict__ dgx, float *__restrict__ dgh,
                                                      float *__restrict__ dh_direct, float *__restrict__ dc_prev) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)C * H) return;
    const int64_t c = i / H;
    const int j = (int)(i - c * H);
    const float *go = gates + c * 4 * H;
    const float d = dh[i];
    if (kind == 0) {
        const float r = go[j], z = go[H + j], n = go[2 * H + j], hn = go[3 * H + j];
        const float hp = h_prev[c * ld_h + j];
        float dr_pre, dz_pre, dn_pre, dnr, dhd;
        sf_gru_cell_bwd(d, r, z, n, hn, hp, dr_pre, dz_pre, dn_pre, dnr, dhd);
        float *x = dgx + c * 3 * H, *g = dgh + c * 3 * H;
        x[j] = dr_pre; x[H + j] = dz_pre; x[2 * H + j] = dn_pre;
        g[j] = dr_pre; g[H + j] = dz_pre; g[2 * H + j] = dnr;
        dh_direct[i] = dhd;
    } else {
        const float ig = go[j], fg = go[H + j], gg = go[2 * H + j], og = go[3 * H + j];
        float *x = dgx + c * 4 * H;
        float di, df, dg, dob, dcp;
        sf_lstm_cell_bwd(d, dc_in ? dc_in[i] : 0.0f, ig, fg, gg, og, c_out[i], c_prev[c * ld_c + j], di, df, dg, dob, dcp);
        x[j] = di; x[H + j] = df; x[2 * H + j] = dg; x[3 * H + j] = dob;
        if (dgh && dgh != dgx) {
            float *g = dgh + c * 4 * H;
            g[j] = di; g[H + j] = df; g[2 * H + j] = dg; g[3 * H + j] = dob;
        }
        dc_prev[i] = dcp;
    }
}

extern "C" int sf_rnn_cell_bwd(int kind, const float *dh, const float *dc_in, const float *gates, const float *h_prev,
                               int64_t ld_h, const float *c_prev, int64_t ld_c, const float *c_out, int C, int H,
                               float *dgx, float *dgh, float *dh_direct, float *dc_prev, void *stream) {
    SF_REQUIRE((kind == 0 || kind == 1) && dh && gates && dgx && C > 0 && H > 0, "sf_rnn_cell_bwd: bad args");
    SF_REQUIRE(kind == 1 || (h_prev && dgh && dh_direct), "sf_rnn_cell_bwd: GRU needs h_prev, dgh, dh_direct");
    SF_REQUIRE(kind == 0 || (c_prev && c_out && dc_prev), "sf_rnn_cell_bwd: LSTM needs c_prev, c_out, dc_prev");
    const int64_t n = (int64_t)C * H;
    k_rnn_cell_bwd<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, STREAM(stream)>>>(
        kind, dh, dc_in, gates, h_prev, ld_h, c_prev, ld_c, c_out, C, H, dgx, dgh, dh_direct, dc_prev);
    return sf_launch_status("sf_rnn_cell_bwd");
}

// rollout: state input of step t+1 = new state * (1 - done) (batched_sampling.py:332-335); out row b = [h | c] (c: LSTM)
__global__ __launch_bounds__(256) void k_rnn_store_state(const float *__restrict__ h, const float *__restrict__ c,
                                                         const uint8_t *__restrict__ dones, int64_t done_stride,
                                                         float *__restrict__ out, int64_t out_stride, int64_t B, int H) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int W = c ? 2 * H : H;
    if (i >= B * W) return;
    const int64_t b = i / W;
    const int j = (int)(i - b * W);
    const float v = j < H ? h[b * H + j] : c[b * H + j - H];
    out[b * out_stride + j] = dones[b * done_stride] ? 0.0f : v;
}

extern "C" int sf_rnn_store_state(const float *h, const float *c, const uint8_t *dones, int64_t done_stride, float *out,
                                  int64_t out_stride, int64_t B, int H, void *stream) {
    SF_REQUIRE(h && dones && out && B > 0 && H > 0, "sf_rnn_store_state: bad args");
    const int64_t n = B * (c ? 2 * H : H);
    k_rnn_store_state<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, STREAM(stream)>>>(h, c, dones, done_stride, out,
                                                                                             out_stride, B, H);
    return sf_launch_status("sf_rnn_store_state");
}

// training pass of a recurrent model over a minibatch of Cn chunks of R consecutive dataset rows (learner.py:557-569,
// rnn_utils.py:59-105): chunk c starts at dataset row r0 = index ? index[c*R] : offset + c*R.  One launch instead of the
// torch op sequence {arange, gathers, ~, |, transpose, float, index_select}:
//   keep_tm[t][c] = !(dones[r0 + t] | !valids[r0 + t])      (state is zeroed AFTER a done / invalid step)
//   h0[c][:]      = rnn_states[r0][:]                       (the state the chunk's first step was collected with)
__global__ __launch_bounds__(256) void k_rnn_chunk_setup(const uint8_t *__restrict__ dones,
                                                         const uint8_t *__restrict__ valids,
                                                         const float *__restrict__ rnn_states,
                                                         const int32_t *__restrict__ index, int64_t offset, int Cn,
                                                         int R, int S, int traj_T, float *__restrict__ keep_tm,
                                                         float *__restrict__ h0) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nk = (int64_t)Cn * R;
    if (i < nk) {  // i = t * Cn + c
        const int t = (int)(i / Cn), c = (int)(i - (int64_t)t * Cn);
        const int64_t row = index ? (int64_t)index[(int64_t)c * R + t] : offset + (int64_t)c * R + t;
        keep_tm[i] = (dones[row] || !valids[row]) ? 0.0f : 1.0f;
    } else if (i < nk + (int64_t)Cn * S) {
        const int64_t j = i - nk;
        const int c = (int)(j / S), e = (int)(j - (int64_t)c * S);
        int64_t row = index ? (int64_t)index[(int64_t)c * R] : offset + (int64_t)c * R;
        if (traj_T > 0) row = (row / traj_T) * (traj_T + 1) + row % traj_T;  // dataset row e*T+t -> slab row e*(T+1)+t
        h0[j] = rnn_states[row * S + e];
    }
}

extern "C" int sf_rnn_chunk_setup(const uint8_t *dones, const uint8_t *valids, const float *rnn_states,
                                  const int32_t *index, int64_t offset, int Cn, int R, int S, int traj_T, float *keep_tm,
                                  float *h0, void *stream) {
    SF_REQUIRE(dones && valids && rnn_states && keep_tm && h0 && Cn > 0 && R > 0 && S > 0, "sf_rnn_chunk_setup: bad args");
    const int64_t tot = (int64_t)Cn * R + (int64_t)Cn * S;
    k_rnn_chunk_setup<<<dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, STREAM(stream)>>>(
        dones, valids, rnn_states, index, offset, Cn, R, S, traj_T, keep_tm, h0);
    return sf_launch_status("sf_rnn_chunk_setup");
}

// y[c, :] = (a[c, :] + b[c, :]) * keep[c]    (carry of dL/dh across a step boundary; b or keep may be NULL)
__global__ __launch_bounds__(256) void k_rows_add_scale(const float *__restrict__ a, const float *__restrict__ b,
                                                        const float *__restrict__ keep, int64_t C, int H,
                                                        float *__restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= C * H) return;
    const float v = a[i] + (b ? b[i] : 0.0f);
    y[i] = keep ? v * keep[i / H] : v;
}

extern "C" int sf_rows_add_scale(const float *a, const float *b, const float *keep, int64_t C, int H, float *y,
                                 void *stream) {
    SF_REQUIRE(a && y && C > 0 && H > 0, "sf_rows_add_scale: bad args");
    k_rows_add_scale<<<dim3((unsigned)((C * H + 255) / 256)), dim3(256), 0, STREAM(stream)>>>(a, b, keep, C, H, y);
    return sf_launch_status("sf_rows_add_scale");
}


// ---- ActionParameterizationContinuousNonAdaptiveStddev with continuous_tanh_scale > 0 (model/action_parameterization.py
// :62-66): action means y = tanh(x / s) * s, in place on `ncols` columns of the heads matrix; backward g *= 1 - (y/s)^2.
__global__ __launch_bounds__(256) void k_tanh_scale(float *__restrict__ x, float *__restrict__ gy, const float *__restrict__ y,
                                                    int ld, int64_t n, int col0, int ncols, float s, float inv_s) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n * ncols; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / ncols;
        const int64_t o = r * ld + col0 + (i - r * ncols);
        if (x) x[o] = tanhf(x[o] * inv_s) * s;
        else { const float t = y[o] * inv_s; gy[o] *= 1.f - t * t; }
    }
}
extern "C" int sf_tanh_scale_fwd(float *x, int ld, int64_t n, int col0, int ncols, float scale, void *stream) {
    SF_REQUIRE(x && n > 0 && ncols > 0 && col0 >= 0 && col0 + ncols <= ld && scale > 0.f, "sf_tanh_scale_fwd: bad args");
    const int64_t tot = n * ncols;
    k_tanh_scale<<<dim3((unsigned)((tot + 255) / 256 < 4096 ? (tot + 255) / 256 : 4096)), dim3(256), 0, STREAM(stream)>>>(
        x, nullptr, nullptr, ld, n, col0, ncols, scale, 1.f / scale);
    return sf_launch_status("sf_tanh_scale_fwd");
}
extern "C" int sf_tanh_scale_bwd(float *g, const float *y, int ld, int64_t n, int col0, int ncols, float scale,
                                 void *stream) {
    SF_REQUIRE(g && y && n > 0 && ncols > 0 && col0 >= 0 && col0 + ncols <= ld && scale > 0.f, "sf_tanh_scale_bwd: bad args");
    const int64_t tot = n * ncols;
    k_tanh_scale<<<dim3((unsigned)((tot + 255) / 256 < 4096 ? (tot + 255) / 256 : 4096)), dim3(256), 0, STREAM(stream)>>>(
        nullptr, g, y, ld, n, col0, ncols, scale, 1.f / scale);
    return sf_launch_status("sf_tanh_scale_bwd");
}
