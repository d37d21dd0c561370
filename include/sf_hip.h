/*
 * sf_hip.h — C ABI of libsf_hip.so: the MI355X (gfx950) APPO hot path behind Sample Factory's plugin surface.
 *
 * The reference (Sample Factory v2.1.3) has NO native boundary: its hot path is Python calling stock PyTorch ops
 * (SURVEY.md §2.3).  This header therefore declares one entry point per reference *op sequence* on the path; each
 * comment cites the reference lines (paths relative to sample_factory/) that the call replaces.  INTEGRATION.md
 * shows the ctypes stub a Sample Factory maintainer would add at each of those call sites.
 *
 * Conventions
 *  - plain C types only; every pointer is a DEVICE pointer (HBM) unless its name starts with `h_`;
 *  - `stream` is a hipStream_t passed as void* (0 = the null stream); calls only enqueue work, they never
 *    synchronise the device, never allocate, never throw;
 *  - return 0 on success, a negative code on failure; sf_last_error() returns the message of the last failure
 *    on the calling thread;
 *  - boundary layout is the reference's: env-major [E, T(+1), ...] trajectory tensors, flat index e*T + t
 *    (learner.py:1009-1012); policy outputs stored as f32 (shared_buffers.py:100-103); bool tensors are 1 byte.
 */
#ifndef SF_HIP_H
#define SF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SF_OK 0
#define SF_ERR_ARG (-1)
#define SF_ERR_LAUNCH (-2)
#define SF_ERR_UNSUPPORTED (-3)
/* members of a Tuple action space (action_distributions.py:197-287 composes any number; Humanoid discretised is 17,
 * ShadowHand 20 to 24).  Every entry point that takes a head list refuses a longer one before it launches anything. */
#define SF_MAX_ACTION_HEADS 64

const char *sf_last_error(void);
int sf_abi_version(void);

/* ---- K13: validity mask ---------------------------------------------------------------------------------
 * learner.py:949-955 (valids = policy_id==pid & train_step-policy_version < max_policy_lag; last column copies
 * the previous one) and :1021-1032 (count invalids; actions=0, log_prob_actions=-1 at invalid rows).
 * valids [E,T+1] u8 out; valids_flat (may be NULL): the same mask as the flat [E*T] dataset array the minibatch consumers
 * index (the reference's `valids[:, :-1]` flatten, learner.py:1009-1012, without its copy); num_invalid: device int32
 * (overwritten). actions [E*T*num_actions], logp [E*T] in/out. */
int sf_valid_mask(const int32_t *policy_id, const float *policy_version, uint8_t *valids, uint8_t *valids_flat,
                  float *actions, int num_actions, float *log_prob_actions, int E, int T, int my_policy_id,
                  int train_step, int max_policy_lag, int32_t *num_invalid, void *stream);

/* ---- K10+K11: value de-normalisation, value bootstrap, GAE, returns ---------------------------------------
 * learner.py:969-1003 + rl_utils.py:52-94 (gae_advantages / calculate_discounted_sum_torch).
 * values [E,T+1] (column T = bootstrap value, learner.py:964-967), valids [E,T+1] u8, dones/time_outs [E,T] u8.
 * rms_stats: device double[3] {mean,var,count} of the returns normaliser, or NULL when normalize_returns=False.
 * rewards is updated in place when value_bootstrap != 0 (learner.py:990).  advantages, returns: [E,T] out;
 * returns are NOT yet normalised (that is sf_rms_*).  One wavefront scans 64 envs; tiles are staged through LDS. */
int sf_gae_returns(float *rewards, const uint8_t *dones, const uint8_t *time_outs, const float *values,
                   const uint8_t *valids, const double *rms_stats, int E, int T, float gamma, float gae_lambda,
                   int value_bootstrap, float *advantages, float *returns, void *stream);

/* ---- K12: RunningMeanStdInPlace (scalar statistics) -------------------------------------------------------
 * running_mean_std.py:51-110.  sf_moments accumulates {sum, sumsq, count} (double[3], zeroed by the call) over x[n]
 * restricted to valid entries: element i of the minibatch is dataset row j = index[i] (index != NULL) or offset + i;
 * valids NULL = all rows count, else valids[j]; the value is x[j], or x[i] when dense_x != 0 (x holds the minibatch's own
 * n values, e.g. the V-trace advantages, while valids is still the dataset's array).
 * Between the two calls a data-parallel learner all-reduces the 3 doubles.
 * sf_rms_update merges the batch moments into stats (Chan merge, :51-62, unbiased batch variance) -> stats_out.
 * sf_rms_apply normalises ((x-mean)/sqrt(var+1e-5) clamp +-5) or de-normalises (clamp, *sigma, +mean) in place. */
int sf_moments(const float *x, const uint8_t *valids, const int32_t *index, int64_t offset, int64_t n, int dense_x,
               double *moments, void *stream);
int sf_rms_update(const double *stats_in, const double *moments, double *stats_out, void *stream);
int sf_rms_apply(float *x, int64_t n, const double *stats, int denormalize, void *stream);

/* ---- K2/K8 (normalize_input=True): observation running mean/std ------------------------------------------------
 * utils/normalize.py:24-70 (ObservationNormalizer), running_mean_std.py:22-136 (RunningMeanStdDictInPlace, full-shape
 * statistics).  x' = (float(x) - obs_subtract_mean) * (1/obs_scale).  Sample addressing as in the network kernels
 * (index | offset, traj_T slab mapping, `stride` elements between rows).  D = elements per observation.
 * sf_obsnorm_moments: per-element {sum, sumsq}[D] of x' over n samples (f64, zeroed by the call).
 * sf_obsnorm_update:  Chan merge into mean/var[D] (in place) and count (count_in -> count_out), refreshes the f32
 *                     tables mu[D], rstd[D] = 1/sqrt(var+1e-5) (n == 0: tables only, e.g. after loading a checkpoint).
 * sf_obsnorm_apply:   out f32 [n, D] = clamp((x' - mu) * rstd, +-5); for images (C > 0) written channels-last
 *                     ([n, H*W, C]) for the NHWC conv kernels.  The north-star preset (normalize_input=False) never
 *                     runs these: there the u8 frames are consumed in place by sf_conv_fwd. */
int sf_obsnorm_moments(const void *in, int in_u8, int64_t stride, const int32_t *index, int64_t offset, int traj_T,
                       int64_t n, int D, float sub_mean, float inv_scale, double *sum, double *sumsq, void *stream);
int sf_obsnorm_update(double *mean, double *var, const double *count_in, double *count_out, const double *sum,
                      const double *sumsq, int64_t n, int D, float *mu_tab, float *rstd_tab, void *stream);
int sf_obsnorm_apply(const void *in, int in_u8, int64_t stride, const int32_t *index, int64_t offset, int traj_T,
                     int64_t n, int D, int C, int HW, float sub_mean, float inv_scale, const float *mu,
                     const float *rstd, float *out, void *stream);

/* ---- K3/K15 recurrent core: GRU / LSTM cells -------------------------------------------------------------------
 * model/core.py:19-64 (ModelCoreRNN over torch.nn.GRU / nn.LSTM, one layer); learner.py:557-581 +
 * rnn_utils.py:114-158 (BPTT over recurrence-length chunks; PackedSequence there, a masked time loop here — the
 * equivalence is the reference's own tests/algo/test_rnn.py).  kind 0 = GRU (gate order r,z,n), 1 = LSTM (i,f,g,o),
 * torch's parameter layout.  gx = x W_ih^T + b_ih, gh = h W_hh^T + b_hh come from sf_conv_fwd (1x1) launches; gh == NULL:
 * gx is the output of ONE sf_linear_fwd_dual launch — LSTM: the complete pre-activation gx + gh [C,4H]; GRU (gru_H = H):
 * [C,4H] = {r and z pre-activations with both parts summed, x W_in^T + b_in, h W_hn^T + b_hn}.
 * fwd: gates_out [C,4H] (GRU {r,z,n,W_hn h + b_hn}; LSTM {i,f,g,o}; NULL at inference), h_out/c_out = new state,
 *      h_next/c_next = new state * keep[c] (keep = 1 - done_or_invalid, learner.py:561; NULL = keep everything).
 * bwd: dh = dL/dh_out of this step (output gradient + masked carry), dc_in = carry into c_out (LSTM); writes dgx, dgh
 *      [C,G*H] (LSTM: dgh may be NULL/alias dgx), dh_direct (GRU: the path of dL/dh_prev that bypasses W_hh),
 *      dc_prev (LSTM).  The W_hh path of dL/dh_prev is sf_conv_dgrad(dgh, W_hh). */
int sf_rnn_cell_fwd(int kind, const float *gx, const float *gh, const float *h_prev, int64_t ld_h, const float *c_prev,
                    int64_t ld_c, const float *keep, int C, int H, float *gates_out, float *h_out, float *c_out,
                    float *h_next, float *c_next, void *stream);
int sf_rnn_cell_bwd(int kind, const float *dh, const float *dc_in, const float *gates, const float *h_prev,
                    int64_t ld_h, const float *c_prev, int64_t ld_c, const float *c_out, int C, int H, float *dgx,
                    float *dgh, float *dh_direct, float *dc_prev, void *stream);
/* y[c,:] = (a[c,:] + b[c,:]) * keep[c] — gradient carry across a step boundary (b, keep optional). */
int sf_rows_add_scale(const float *a, const float *b, const float *keep, int64_t C, int H, float *y, void *stream);

/* ---- K17: V-trace -----------------------------------------------------------------------------------------
 * learner.py:601-640 (the reference runs this loop on the CPU).  Flat minibatch of n samples made of
 * n/recurrence trajectories; sample i of the minibatch is dataset row (index ? index[i] : offset+i).
 * params [n,A] (row stride ld_params) / values [n] (stride ld_values): CURRENT policy outputs (minibatch order; the
 * strides let both be columns of the fused heads GEMM output [n, 1+A]); actions/old_logp/rewards/dones: dataset
 * arrays; dones u8.  Outputs vs, adv [n] in minibatch order.  action_kind as in sf_ppo_loss.  Any A > 0: up to 128
 * parameters the ratio pass keeps a row in one lane's registers, above that one wave walks a row (k_vtrace_ratio_wide). */
int sf_vtrace(const float *params, int ld_params, const float *values, int ld_values, const float *actions,
              const float *old_logp, const float *rewards, const uint8_t *dones, const int32_t *index, int64_t offset,
              int64_t n, int A, int action_kind, int recurrence, float gamma, float rho_hat, float c_hat, float *vs,
              float *adv, const int32_t *head_n /* host; Tuple members as in sf_loss_cfg.head_n, or NULL */,
              int num_heads /* <= SF_MAX_ACTION_HEADS */, void *stream);

/* ---- K16: PPO loss head, forward + backward ----------------------------------------------------------------
 * learner.py:586-669 (ratio, clamp [0.05,20], per-minibatch advantage normalisation, clipped surrogate, entropy /
 * symmetric-KL exploration loss, KL(new||old), clipped value loss; all means over valid samples) and the autograd
 * backward of their sum wrt the action-distribution parameters and the value.
 * action_kind 0 = Discrete(A) (action_distributions.py:99-194), 1 = Box(A/2) (:290-323).
 * exploration_kind 0 none, 1 entropy, 2 symmetric_kl.
 * moments: device double[3] {sum, sumsq, n_valid} of the UN-normalised advantage over the (global) minibatch,
 * produced by sf_moments (+ all-reduce).  adv/targets: dataset arrays unless dense_adv != 0 (v-trace: minibatch
 * order).  sums: device double[8], zeroed by the call, receives {policy, entropy-or-symkl, kl, value} sums over
 * valid samples, [4] = max KL, [5] = n_valid; sf_loss_scalars turns them into the reference's loss scalars.
 * params/values are read with row strides ld_params/ld_values (elements); g_params [n,A], g_values [n] are written
 * with the SAME strides (so they can be columns of one [n, 1+A] heads-gradient matrix), minibatch order. */
typedef struct {
    float clip_ratio;        /* cfg.ppo_clip_ratio  (clip_high = 1+c, clip_low = 1/(1+c), learner.py:544-546) */
    float clip_value;        /* cfg.ppo_clip_value */
    float value_loss_coeff;  /* cfg.value_loss_coeff */
    float exploration_coeff; /* cfg.exploration_loss_coeff */
    float kl_coeff;          /* cfg.kl_loss_coeff */
    int32_t exploration_kind;
    int32_t action_kind;
    int32_t dense_adv;
    /* Tuple spaces (action_distributions.py:197-287: independent members built by get_action_distribution, :222-225;
     * log-prob, entropy, KL and symmetric-KL are sums over the members): num_heads > 1 and, per member h,
     * head_n[h] = n > 0 for Discrete(n) (n logits, one action column) or head_n[h] = -D < 0 for Box(D) (2 D parameters
     * [means | log_std], D action columns; symmetric-KL exploration is refused for it, as the reference's
     * ContinuousActionDistribution has no symmetric_kl_with_uniform_prior).  Parameters sum to A; `actions` holds the
     * members' columns side by side per sample.  num_heads <= 1: one Discrete(A).  The struct holds 8 members and its
     * size is part of the ABI; a longer list (up to SF_MAX_ACTION_HEADS) goes to sf_ppo_loss_heads as an argument. */
    int32_t num_heads;
    int32_t head_n[8];
    /* > 0: `old_values` is the trajectory slab's values array [E, old_values_T + 1] read IN PLACE — dataset row
     * e*T + t lives at e*(T+1) + t (the reference drops the last column by `[:, :-1]` + flatten, learner.py:1009-1012:
     * a copy); 0: old_values is the flat [N] array. */
    int32_t old_values_T;
} sf_loss_cfg;

/* Any A > 0.  A <= 128: one lane per sample, the distribution in registers.  A > 128 (one wide Discrete / Box, or a
 * head list whose parameters add up to more): k_ppo_loss_wide, one wave64 per sample row, lanes striding the columns,
 * same formulas, same sums[0..7]; rows only need 4-byte alignment (they start at column 1 of the heads matrix). */
int sf_ppo_loss(const float *params, int ld_params, const float *values, int ld_values, const float *actions,
                const float *old_logp, const float *old_params, const float *old_values, const float *adv,
                const float *targets, const uint8_t *valids, const int32_t *index, int64_t offset, int64_t n, int A,
                const sf_loss_cfg *h_cfg, const double *moments, double *sums, float *g_params, float *g_values,
                float *ratio_out /* [n] clamped pi/pi_old per sample for the summaries (learner.py:886-903), or NULL */,
                void *stream);
/* sf_ppo_loss for a Tuple of 1 .. SF_MAX_ACTION_HEADS members (TupleActionDistribution, action_distributions.py:197-287:
 * log_prob :258, entropy :265, kl_divergence :271 and symmetric_kl_with_uniform_prior :278 are sums over the
 * members): head_n (host array of num_heads entries, as sf_loss_cfg.head_n) replaces the struct's num_heads / head_n,
 * which are not read; everything else as sf_ppo_loss, same launcher.  Up to 8 members run the kernels sf_ppo_loss runs,
 * with the same results; more run k_ppo_loss_mh (A <= 128: one lane per sample, the members' statistics recomputed in the
 * gradient loop, not kept) or k_ppo_loss_wide (A > 128), and add the row's log-prob — up to 64 terms — up in double.
 * A bad list (num_heads outside 1 .. SF_MAX_ACTION_HEADS, an empty member, sizes that do not sum to A, a Box member with
 * symmetric-KL exploration) returns SF_ERR_ARG before any launch. */
int sf_ppo_loss_heads(const float *params, int ld_params, const float *values, int ld_values, const float *actions,
                      const float *old_logp, const float *old_params, const float *old_values, const float *adv,
                      const float *targets, const uint8_t *valids, const int32_t *index, int64_t offset, int64_t n, int A,
                      const sf_loss_cfg *h_cfg, const double *moments, double *sums, float *g_params, float *g_values,
                      float *ratio_out, const int32_t *head_n /* host */, int num_heads, void *stream);
/* Training under the action mask the rows were SAMPLED under (the reference's
 * CategoricalActionDistribution(raw_logits, action_mask), action_distributions.py:84-180, which its learner never hands
 * the mask).  Per Discrete member with logits slice z and mask slice m, the rule of sf_sample_write_step_masked:
 *   logp_k = ((z_k + (m_k ? 0 : -1e9f)) - mx) - lse;   p_k = m_k ? exp((z_k - mx) - lse) / (sum of those + 1e-13) : 0
 * (the sampler's 1e-6 multinomial weights are no part of the loss); member log-prob logp_a, entropy -sum p_k logp_k,
 * KL(new || old) = sum p_k (logp_k - logp_old_k) with the OLD distribution built from old_params under the SAME mask row;
 * row quantities are sums over the members; a Box(D) member never reads the 2 D mask columns under it.  The gradient is
 * the analytic derivative: d logp_a / dz_k = delta_ak - exp(logp_k), exactly 0 on a masked-out column of a slice that
 * allows something; an all-zero slice behaves as n equal logits (|z| < 32 is absorbed by z - 1e9 in f32) with p = 0,
 * entropy 0, KL 0 and gradient delta_ak - 1 / n.
 * mask: u8, row stride ld_mask >= A, column c belonging to parameter column c.  mask_T > 0: the trajectory slab's
 * [E, mask_T + 1, A] array read in place, dataset row e * T + t at mask row e * (T + 1) + t (as old_values_T);
 * mask_T == 0: a flat [N, ld_mask] array.  Rows go through index / offset like every dataset array.
 * sf_ppo_loss_masked takes the member list as sf_ppo_loss_heads does (one member: Discrete(A)); both refuse, before any
 * launch or memset (SF_ERR_ARG): a null mask, ld_mask < A, mask_T < 0, a pure Box space, every head list the unmasked
 * entry refuses, and (the loss) symmetric-KL exploration with a non-zero coefficient, whose uniform-prior term
 * u (log u - logp_k) has no meaning where logp_k is about -1e9. */
int sf_ppo_loss_masked(const float *params, int ld_params, const float *values, int ld_values, const float *actions,
                       const float *old_logp, const float *old_params, const float *old_values, const float *adv,
                       const float *targets, const uint8_t *valids, const int32_t *index, int64_t offset, int64_t n, int A,
                       const sf_loss_cfg *h_cfg, const double *moments, double *sums, float *g_params, float *g_values,
                       float *ratio_out, const int32_t *head_n /* host */, int num_heads, const uint8_t *mask,
                       int64_t ld_mask, int mask_T, void *stream);
/* sf_vtrace with the importance ratios taken under the mask (rule and mask addressing above); k_vtrace is unchanged. */
int sf_vtrace_masked(const float *params, int ld_params, const float *values, int ld_values, const float *actions,
                     const float *old_logp, const float *rewards, const uint8_t *dones, const int32_t *index,
                     int64_t offset, int64_t n, int A, int action_kind, int recurrence, float gamma, float rho_hat,
                     float c_hat, float *vs, float *adv, const int32_t *head_n /* host, or NULL */, int num_heads,
                     const uint8_t *mask, int64_t ld_mask, int mask_T, void *stream);
/* ---- consistency loss between two rows of a heads matrix (--augment_consistency_coeff) -------------
 * DrAC (Raileanu et al.): the PPO loss stays on the clean frames, and a regulariser pulls policy and value on the
 * augmented frames towards their values on the clean ones.  The reference has no augmentation.  Row i of the launch is
 * dataset row d = index ? index[i] : offset + i (read for valids[d] only); its target is row i of params_t / values_t
 * (a constant: nothing is written for it), its student row i of params_s / values_s; both pairs are strided column views
 * (ld_params, ld_values in elements, rows 4-byte aligned), in the learner rows [0, n) and [n, 2n) of ONE heads matrix.
 * Per valid row, summed over the members of the head list (action_kind / head_n / num_heads as sf_vtrace takes them;
 * head_n NULL: one Discrete(A) or Box(A / 2)):
 *   Discrete member, logits z, lp = log_softmax(z), p = exp(lp):
 *     KL = sum_k p_t,k (lp_t,k - lp_s,k)                        d KL / d z_s,k = p_s,k - p_t,k
 *   Box(D) member, column k, sd = clamp(exp(log_std), 1e-4, 1e4) (the loss's clamp):
 *     vr = (sd_t / sd_s)^2,  dl = (mu_t - mu_s) / sd_s,  KL = (vr + dl^2 - 1 - ln vr) / 2
 *     d KL / d mu_s = (mu_s - mu_t) / sd_s^2       d KL / d log_std_s = 1 - vr - dl^2, 0 where exp(log_std_s) is beyond the clamp
 *   value: (v_s - v_t)^2
 * With inv_n = 1 / moments[2] (the global valid count sf_ppo_loss divides by) the call writes, for every valid row,
 *   g_params_s[i][:A] = coeff_policy inv_n dKL/dz_s      g_values_s[i] = coeff_value inv_n 2 (v_s - v_t)
 * and an all-zero gradient row for an invalid one (valids[d] == 0), which is not counted; columns beyond A and other rows
 * are not touched.  sums: device double[4], zeroed by the call: {sum KL, sum (v_s - v_t)^2, max KL, n_valid} over the
 * valid rows; the loss is coeff_policy sums[0] inv_n + coeff_value sums[1] inv_n.  Rows with the same bits give exactly 0.
 * A <= 128: one lane per row; A > 128: one wave64 per row (the wide family of sf_ppo_loss, same helpers, same rounding).
 * Refused before any launch or memset (SF_ERR_ARG): a null pointer (index and head_n may be null), n < 0, A <= 0,
 * offset < 0, ld_params < A, ld_values < 1, action_kind not 0 / 1 or 1 with an odd A, a head list sf_ppo_loss_heads
 * refuses (num_heads outside 1 .. SF_MAX_ACTION_HEADS, an empty member, sizes that do not sum to A, a one-member list
 * that is not the single space, several members with action_kind 1), a negative or non-finite coefficient.  n == 0:
 * SF_OK, nothing is launched. */
int sf_consistency_loss(const float *params_t, const float *params_s, int ld_params, const float *values_t,
                        const float *values_s, int ld_values, const uint8_t *valids, const int32_t *index, int64_t offset,
                        int64_t n, int A, int action_kind, const int32_t *head_n /* host, or NULL */, int num_heads,
                        float coeff_policy, float coeff_value, const double *moments, double *sums, float *g_params_s,
                        float *g_values_s, void *stream);
/* out[0..3] = policy, exploration, kl, value losses; [4] kl mean; [5] kl max; [6] adv mean; [7] adv std;
 * [8] n_valid; [9] entropy (or symkl) mean — device float[16]. */
int sf_loss_scalars(const double *sums, const double *moments, const sf_loss_cfg *h_cfg, float *out, void *stream);
/* learner.py:843-923 (`_record_summaries`: ~25 torch reductions with an `.item()` each) for one minibatch in ONE pass:
 * rows i < n are dataset rows index[i] | offset + i; ratio [n] (sf_ppo_loss's ratio_out), values (new, stride ld_values),
 * old_values (flat [N], or the slab's [E, old_values_T + 1]), actions [N, num_actions], adv ([n] if dense_adv else [N]),
 * policy_id / policy_version / valids [N], action_logits [N, A]; exp_avg_sq [P] (may be NULL).  out: device double[24]:
 * [0] rows [1] valid [2] same-policy [3] sum value [4] sum |1 - ratio| over valid [5] clipped ratios (valid, outside
 * [1/(1+clip_ratio), 1+clip_ratio]) [6] sum |v - v_old| [7] sum (train_step - policy_version) over same-policy rows;
 * [8]/[9] ratio min / max (valid) [10] max |v - v_old| [11]/[12] action min / max [13]/[14] adv min / max
 * [15] max |old action parameter| [16]/[17] version_diff min / max [18] max exp_avg_sq (minima +inf / maxima -inf when
 * no row qualified). */
int sf_train_summaries(const uint8_t *valids, const float *ratio, const float *values, int ld_values,
                       const float *old_values, int old_values_T, const float *actions, int num_actions, const float *adv,
                       int dense_adv, const int32_t *policy_id, const float *policy_version, const float *action_logits,
                       int A, const int32_t *index, int64_t offset, int64_t n, int my_policy_id, int train_step,
                       float clip_ratio, const float *exp_avg_sq, int64_t P, double *out, void *stream);

/* ---- K14: minibatch index sets ------------------------------------------------------------------------------
 * learner.py:498-526.  Writes experience_size int32 indices: a pseudo-random permutation (stateless 4-round
 * Feistel network with cycle walking, keyed by seed/epoch) of the recurrence-aligned chunk starts, each expanded to
 * `recurrence` consecutive indices; minibatch k is out[k*batch .. (k+1)*batch).  shuffle==0 writes the identity
 * (contiguous slices, the reference default). */
int sf_minibatch_indices(int32_t *out, int64_t experience_size, int recurrence, int shuffle, uint32_t seed,
                         uint32_t epoch, void *stream);
/* learner.py:507-519 with the REFERENCE's permutation: chunk_starts (device int32[experience_size / recurrence]) is the
 * host's seeded np.random.permutation(np.arange(0, experience_size, recurrence)), uploaded as is; out receives the
 * expanded index runs [s, s+1, .., s+recurrence-1] per chunk, i.e. exactly np.concatenate(...) of :512-515. */
int sf_minibatch_expand(const int32_t *chunk_starts, int32_t *out, int64_t experience_size, int recurrence,
                        void *stream);

/* ---- K18/K19: global-norm clip + Adam ------------------------------------------------------------------------
 * learner.py:782-797: torch.nn.utils.clip_grad_norm_(max_grad_norm) then torch.optim.Adam.step (eps=cfg.adam_eps,
 * no weight decay/amsgrad; learner.py:228-243).  All parameters live in one flat fp32 buffer of P elements.
 * sf_grad_sumsq: sumsq (device double[1], zeroed by the call) = sum g^2.  sf_adam_step reads it: coef =
 * min(1, max_norm/(sqrt(sumsq)+1e-6)) (skipped when max_grad_norm <= 0 or sumsq == NULL), g scaled by
 * grad_scale*coef, then the Adam update in torch's op order.  `step` is the 1-based Adam step count.
 * skip_flag (device uint32, may be NULL): when the word is non-zero as the kernel starts, the launch is a no-op —
 * weights and moments stay untouched (the sticky abort word of the fused recurrent passes, see sf_lstm_seq_fwd). */
int sf_grad_sumsq(const float *g, int64_t P, double *sumsq, void *stream);
int sf_adam_step(float *p, const float *g, float *m, float *v, int64_t P, int step, float lr, float beta1,
                 float beta2, float eps, float max_grad_norm, const double *sumsq, float grad_scale,
                 const uint32_t *skip_flag, void *stream);
/* sf_adam_step with the learning rate in DEVICE memory (lr = *lr_dev * lr_scale; lr_scale = the valid-sample fraction of
 * learner.py:788-794), and the per-minibatch KL-adaptive schedule of learner.py:46-85 (lr_schedule=kl_adaptive_minibatch:
 * lr /= 1.5 above 2 x threshold, *= 1.5 below threshold / 2, within [lr_min, lr_max]) as a one-thread launch on the
 * minibatch's mean KL (sf_loss_scalars out[4]): the schedule no longer costs a host read-back per SGD step.
 * lr_out (may be NULL) receives a copy of the new rate (read back once per epoch with the loss scalars). */
int sf_adam_step_dlr(float *p, const float *g, float *m, float *v, int64_t P, int step, const float *lr_dev,
                     float lr_scale, float beta1, float beta2, float eps, float max_grad_norm, const double *sumsq,
                     float grad_scale, const uint32_t *skip_flag, void *stream);
int sf_lr_kl_adaptive(const float *kl, float *lr_dev, float threshold, float lr_min, float lr_max, float *lr_out,
                      void *stream);
/* measurement helper: one wave spins for spin_cycles shader cycles; out[0] = shader cycles, out[1] = ticks of the constant
 * 100 MHz wall clock elapsed meanwhile (device uint64[2]) -> shader clock [GHz] = 0.1 * out[0] / out[1].  bench.py launches
 * it on a side stream during the timed region (roofline.clock_ghz). */
int sf_clock_probe(unsigned long long *out, int spin_cycles, void *stream);

/* Lamb (cfg.optimizer = "lamb"; algo/utils/optimizers.py:14-189 as configured by learner.py:228-243: Adam direction
 * with bias correction + weight_decay * w, then per-TENSOR trust ratio min(||w||, 10)/||step|| clamped to
 * [min_trust, 1/min_trust]; the reference's `step` starts at 1).  seg_id[P] (u8): index of the reference tensor each
 * flat element belongs to, 255 = padding (skipped); scratch[P] f32; seg_sums: device double[128] (zeroed by the call).
 * Gradient clipping and skip_flag as in sf_adam_step. */
int sf_lamb_step(float *p, const float *g, float *m, float *v, float *scratch, const uint8_t *seg_id, double *seg_sums,
                 int64_t P, int num_segments, int step, float lr, float beta1, float beta2, float eps,
                 float weight_decay, float min_trust, float max_grad_norm, const double *sumsq, float grad_scale,
                 const uint32_t *skip_flag, void *stream);

/* ---- K4/K5: action sampling + policy outputs -> trajectory step ------------------------------------------------
 * action_distributions.py:110-148 (softmax, multinomial, log_softmax, gather), actor_critic.py:112-117,
 * inference_worker.py:235-269,330-339 and batched_sampling.py:308-311 (policy outputs copied into traj[:, t]).
 * logits [B,A] (row stride ld_logits), values [B] (stride ld_values): network outputs.  Samples by inverse CDF from a Philox4x32-10 uniform
 * (key = (seed, row0+b), counter = (step, 0, 2, 0)) and writes, for env b, element (b*stride + t) of the
 * trajectory tensors: actions (f32), log_prob_actions, values (row stride T+1), policy_version, action_logits
 * (A floats) and the int32 action for the env.  `deterministic` != 0 takes argmax (enjoy.py:177-182).
 * action_kind 1 = Box(A/2): params are [means | log_std] (action_distributions.py:290-310); the action
 * mu + clamp(exp(log_std),1e-4,1e4)*eps (eps: Box-Muller on Philox stream 3) is written as A/2 floats into
 * traj_actions[b*T+t] (the env reads it from there; env_actions may be NULL); deterministic takes the mean.
 * Any A > 0.  The three samplers hand rows of more than 128 parameters to k_sample_write_wide (one wave64 per env row;
 * the CDF is walked 64 columns at a time: wave scan + carry, a ballot finds the first crossing) — same Philox counters,
 * uniforms and draw rule: first index with u < cdf, else the last action of non-zero probability; arg-max = first maximum. */
int sf_sample_write_step(const float *logits, int ld_logits, const float *values, int ld_values, int B, int A, int T,
                         int t, uint32_t seed, uint32_t step, uint32_t row0, float policy_version, int deterministic,
                         int action_kind, float *traj_actions,
                         float *traj_logits, float *traj_logp, float *traj_values, float *traj_policy_version,
                         int32_t *env_actions, void *stream);

/* Discrete(A) with obs["action_mask"] (u8 [B, A], row stride ld_mask; inference_worker.py:324-331): sampling and
 * log-prob follow masked_softmax / masked_log_softmax (action_distributions.py:84-96); raw logits are recorded. */
int sf_sample_write_step_masked(const float *logits, int ld_logits, const float *values, int ld_values,
                                const uint8_t *action_mask, int64_t ld_mask, int B, int A, int T, int t, uint32_t seed,
                                uint32_t step, uint32_t row0, float policy_version, int deterministic,
                                float *traj_actions, float *traj_logits, float *traj_logp, float *traj_values,
                                float *traj_policy_version, int32_t *env_actions, void *stream);

/* Tuple variant of sf_sample_write_step (TupleActionDistribution.sample_actions_log_probs,
 * action_distributions.py:241-245): member h (head_n[h] as in sf_loss_cfg, host array of num_heads <= SF_MAX_ACTION_HEADS entries) is
 * sampled by inverse CDF from its own Philox uniform (counter (step, h, 2, 0)) if Discrete, as mu + sd * eps with
 * Box-Muller normals from counter (step, dim / 2, 3, h) if Box(D) (deterministic: arg-max / the mean); traj_actions
 * gets the members' columns side by side, traj_logp the SUM of the members' log-probs.  env_actions [B, num_heads]
 * int32 for an all-Discrete tuple; NULL (required) when a member is a Box — the env then reads traj_actions[:, t]. */
int sf_sample_write_step_tuple(const float *logits, int ld_logits, const float *values, int ld_values, int B,
                               int num_heads, const int32_t *head_n, int T, int t, uint32_t seed, uint32_t step,
                               uint32_t row0, float policy_version, int deterministic, float *traj_actions,
                               float *traj_logits, float *traj_logp, float *traj_values, float *traj_policy_version,
                               int32_t *env_actions, void *stream);

/* sf_sample_write_step_tuple under obs["action_mask"]: u8 [B, A], A = the members' parameter counts added up, row b at
 * action_mask + b * ld_mask (ld_mask >= A), mask column c belonging to logits column c.  A Discrete member reads the
 * slice at its own logits offset and follows the rule of sf_sample_write_step_masked on it: masked-out logits count as
 * z - 1e9 in the log-sum-exp, p = softmax * mask / (sum + 1e-13), an all-zero slice draws uniformly (arg-max: action 0),
 * the member's log-prob is the masked log-softmax at the drawn action; the 2 * D columns under a Box(D) member are never
 * read and the member is sampled as without a mask.  (The reference's Tuple path indexes the mask by member along the
 * BATCH dimension, action_distributions.py:224; this is the per-parameter layout its Discrete path uses.)  Philox
 * counters as in sf_sample_write_step_tuple: the mask changes probabilities, never uniforms.  Raw logits are recorded.
 * Refused before any launch (-1): a null mask, ld_mask < A, and what sf_sample_write_step_tuple refuses. */
int sf_sample_write_step_tuple_masked(const float *logits, int ld_logits, const float *values, int ld_values,
                                      const uint8_t *action_mask, int64_t ld_mask, int B, int num_heads,
                                      const int32_t *head_n, int T, int t, uint32_t seed, uint32_t step, uint32_t row0,
                                      float policy_version, int deterministic, float *traj_actions, float *traj_logits,
                                      float *traj_logp, float *traj_values, float *traj_policy_version,
                                      int32_t *env_actions, void *stream);

/* ---- K1/K6: env outputs -> trajectory step ---------------------------------------------------------------------
 * batched_sampling.py:208-213 (reward*scale, clamp +-clip), :319-335 (rewards/dones/time_outs/policy_id into
 * traj[:, t]) and :215-287 (episode statistics, kept on device: ep_return/ep_len per env, and on `done` the
 * finished episode is added to ep_stats {sum_return, sum_len, count} (device double[3])). */
int sf_traj_write_env_step(const float *rewards, const uint8_t *terminated, const uint8_t *truncated, int B, int T,
                           int t, float reward_scale, float reward_clip, int policy_id, float *traj_rewards,
                           uint8_t *traj_dones, uint8_t *traj_time_outs, int32_t *traj_policy_id, float *ep_return,
                           int32_t *ep_len, double *ep_stats, void *stream);

/* sf_traj_write_env_step for envs that report info["is_active"] (non_batched_sampling.py:82-84, 197-203; DESIGN.md
 * 3.13), one launch in its place.  active_state: one persistent u8 per agent row, 1 = the agent acted at this step.
 * traj_policy_id[b, t] = active_state[b] ? policy_id : -1, and only then active_state[b] = active_in[b] != 0 (what the
 * env reported WITH this step: it rules the next one).  The thread that owns row b reads and rewrites its byte.  Every
 * other output holds the bits sf_traj_write_env_step writes.  Refused before any launch (-1): a null active_in or
 * active_state, an active_in that aliases active_state, and what sf_traj_write_env_step refuses. */
int sf_traj_write_env_step_active(const float *rewards, const uint8_t *terminated, const uint8_t *truncated, int B, int T,
                                  int t, float reward_scale, float reward_clip, int policy_id, float *traj_rewards,
                                  uint8_t *traj_dones, uint8_t *traj_time_outs, int32_t *traj_policy_id, float *ep_return,
                                  int32_t *ep_len, double *ep_stats, const uint8_t *active_in, uint8_t *active_state,
                                  void *stream);

/* ---- statistics an env defines itself (csrc/sf_traj.hip) ------------------------------------
 * batched_sampling.py:235-251: every per-agent tensor of a vectorised env's `infos` is a statistic, taken at the envs
 * that finished (`value[finished]`); runner.py:263-278 averages them.  Here the values stay on the device: one launch
 * per env step adds them to per-channel accumulators that the runner reads back with ep_stats, once per report.
 * A channel is one such tensor: element b of channel k is ptr[k][b * stride[k]] (stride in ELEMENTS of its dtype). */
#define SF_EPSTAT_MAX_CHANNELS 16
#define SF_EPSTAT_F32 0
#define SF_EPSTAT_F64 1
#define SF_EPSTAT_I32 2
#define SF_EPSTAT_I64 3
#define SF_EPSTAT_U8 4 /* u8 and 1-byte bool */
typedef struct {
    const void *ptr[SF_EPSTAT_MAX_CHANNELS]; /* device pointers */
    int64_t stride[SF_EPSTAT_MAX_CHANNELS];  /* >= 1, in elements */
    int32_t dtype[SF_EPSTAT_MAX_CHANNELS];   /* SF_EPSTAT_* */
} sf_epstat_channels;
/* For every b < B with terminated[b] | truncated[b] (and active[b] != 0 where active is given) and every channel k < K:
 * acc[k][0] += (double)value_k[b], acc[k][1] += 1.  acc: device double [K][2]; the call adds to it and never zeroes it.
 * h_ch is read on the host and travels by value in the launch: it may be reused as soon as the call returns.
 * One launch, one lane per env: the values are converted to f64 on load and summed over the wave and the block in f64,
 * then one atomicAdd pair per channel and block (blocks without a finished env add nothing).
 * Refused before any launch (SF_ERR_ARG): K outside 1 .. SF_EPSTAT_MAX_CHANNELS; a null h_ch, terminated, truncated, acc
 * or channel pointer; B < 0; a stride < 1; an unknown dtype code.  B == 0: SF_OK, nothing is launched. */
int sf_episode_stats_add(const sf_epstat_channels *h_ch, int K, const uint8_t *terminated, const uint8_t *truncated,
                         const uint8_t *active /* or NULL */, int64_t B, double *acc, void *stream);

/* Ant-shaped continuous stand-in env (config 5): f32 observations [B, D], Box actions [B, A] (row stride act_stride
 * floats, e.g. traj.actions[:, t]).  One launch per env step writes the next observation into `state` (the env's own
 * [B, D] copy) AND into obs_out (row stride out_stride floats = slot t+1 of the slab); reset != 0: fresh observations
 * only.  obs' = terminated ? noise : 0.9*obs + 0.1*noise, reward = -mean(a^2) + 0.1*obs[0], terminated ~ Bernoulli(1/256). */
int sf_synth_vec_step(float *state, const float *actions, int64_t act_stride, float *obs_out, int64_t out_stride, int B,
                      int D, int A, int env0, uint32_t seed, uint32_t step, int reset, float *rewards,
                      uint8_t *terminated, void *stream);

/* ---- host-env ingest ---------------------------------------------------------------------
 * batched_sampling.py:62-82 / rl_utils.py:38: observations of a CPU vector env (envpool: one [B, ...] host array per
 * step) go into slot t of the device slab.  Rows of `row_bytes` bytes, `rows` of them, from (pinned) host memory with
 * pitch src_pitch to device memory with pitch dst_pitch (= (T+1) * row_bytes for slab[:, t]): ONE pitched DMA
 * (hipMemcpy2DAsync) on `stream` — no contiguous device staging copy, no kernel.  Returns without synchronising. */
int sf_h2d_rows(void *dst, int64_t dst_pitch, const void *src, int64_t src_pitch, int64_t row_bytes, int64_t rows,
                void *stream);
/* device -> device row copy with pitches (one launch): the column copies of the slab protocol — the next rollout's
 * obs[:, 0] / rnn_states[:, 0] <- this rollout's [:, T] (batched_sampling.py:289-296, TensorDict `copy_` per leaf in the
 * reference), the bootstrap value -> values[:, T] (learner.py:962-969). */
int sf_copy_rows(void *dst, int64_t dst_pitch, const void *src, int64_t src_pitch, int64_t row_bytes, int64_t rows,
                 void *stream);
/* ---- frame stack on the device (csrc/sf_ingest.hip) ----------------------------------------------------------
 * The reference stacks frames inside the env (sf_examples/atari/atari_utils.py:112, gym.wrappers.FrameStack(env,
 * cfg.env_framestack)), so a host env ships the whole [k C, H, W] observation every step although (k - 1) / k of it
 * already sits in the slab column before.  With --device_framestack=k the env delivers ONE frame and the stack is kept
 * in the slab.  Byte granular (u8 and f32 frames alike): row b of `next` / `prev` is k slots of frame_bytes, oldest
 * first, rows next_pitch / prev_pitch bytes apart (obs[:, t + 1] / obs[:, t]).  With done = terminated[b] | truncated[b]
 * (either pointer may be NULL = all zero):
 *   not done:                          next[b][j] = prev[b][j + 1] for j < k - 1, next[b][k - 1] = frame[b]
 *   done, or BOTH flag pointers NULL:  next[b][j] = frame[b] for every j   (the auto-reset observation refills the
 *                                      stack; both NULL is an env reset, prev is then not read)
 * frame == NULL: the new frame has already been written to next[b][k - 1] (sf_h2d_rows straight into the last slot:
 * the rows are contiguous, the pitch is the column's); that slot is then read for done rows and never written.
 * One launch; 16-byte accesses when every address, pitch and frame_bytes allow it, else 4-byte, else single bytes.
 * Refused before any launch (SF_ERR_ARG): null next / prev, k outside 1 .. 16, frame_bytes <= 0, a pitch below
 * k * frame_bytes, frame_pitch < frame_bytes, rows < 0, rows of next and prev that share bytes.  rows == 0: SF_OK,
 * nothing is launched. */
int sf_framestack_step(void *next, int64_t next_pitch, const void *prev, int64_t prev_pitch, const void *frame,
                       int64_t frame_pitch, int64_t frame_bytes, int k, const uint8_t *terminated,
                       const uint8_t *truncated, int rows, void *stream);
/* ---- channel-last frames (csrc/sf_ingest.hip, --hwc_observations) ---------------------------------------------
 * Most pixel envs deliver [H][W][C] frames (the reference transposes them on the host, in the env's wrapper stack:
 * PixelFormatChwWrapper); the encoders read [C][H][W].  elem_bytes: 1 (u8) or 4 (f32).
 * sf_hwc_to_chw: row b of `src` is one frame [H][W][C], rows src_pitch bytes apart; row b of `dst` is C planes of H W
 * elements, rows dst_pitch bytes apart (a slab column obs[:, t], or the last C planes of a stacked column):
 *   dst[b][c][p] = src[b][p][c]  for p < H W, bit for bit.
 * One launch.  Alignment classes: when dst, src and both pitches are multiples of 4 — and, for u8, H W is too — every
 * global access is a dword that is contiguous across the lanes of a wave (u8: a lane owns 4 pixels, loads its C
 * interleaved dwords and de-interleaves them in registers with byte permutes for C <= 4; wider C gathers with byte loads
 * and still stores dwords; f32: a lane owns a pixel).  Anything else takes a byte-wise path.  Any C >= 1; C == 1 is a
 * row copy.  dst and src must not share bytes (not checked).
 * Refused before any launch (SF_ERR_ARG): null dst / src, H, W or C < 1, elem_bytes not 1 or 4, a pitch below
 * H W C elem_bytes, rows < 0.  rows == 0: SF_OK, nothing is launched. */
int sf_hwc_to_chw(void *dst, int64_t dst_pitch, const void *src, int64_t src_pitch, int H, int W, int C, int elem_bytes,
                  int rows, void *stream);
/* sf_framestack_step with a mandatory separate `frame` buffer whose rows are [H][W][C] (frame_bytes = H W C elem_bytes):
 * the same launch count, the transpose rides in it.  With done as above:
 *   not done:                          next[b][j] = prev[b][j + 1] for j < k - 1 (ONE shifted contiguous copy, 16-byte
 *                                      accesses where next, prev, their pitches and frame_bytes allow), next[b][k - 1] =
 *                                      chw(frame[b])
 *   done, or BOTH flag pointers NULL:  next[b][j] = chw(frame[b]) for every j; each source element is loaded once
 * Alignment classes of the transpose as for sf_hwc_to_chw, over next, prev (k > 1), frame and the three pitches.
 * Refused before any launch (SF_ERR_ARG): null next / prev / frame, k outside 1 .. 16, H, W or C < 1, elem_bytes not 1
 * or 4, a pitch below k * frame_bytes, frame_pitch < frame_bytes, rows < 0, rows of next and prev that share bytes.
 * rows == 0: SF_OK, nothing is launched. */
int sf_framestack_step_hwc(void *next, int64_t next_pitch, const void *prev, int64_t prev_pitch, const void *frame,
                           int64_t frame_pitch, int H, int W, int C, int elem_bytes, int k, const uint8_t *terminated,
                           const uint8_t *truncated, int rows, void *stream);
/* ---- resize and grey-scale of u8 frames (csrc/sf_ingest.hip, --device_resize / --device_grayscale) ---------------
 * The arithmetic a raw-pixel env's image wrappers do on the host (the reference's ResizeWrapper: cv2.resize, then
 * COLOR_RGB2GRAY; the area resize + grey-scale of the usual Atari preprocessing), as ONE launch that also reads
 * channel-last frames.  u8 in, u8 out, integer arithmetic only; sample_factory_amd/envs/frame_ops.py is the same
 * arithmetic in NumPy, bit for bit.
 * Row b of `src` is one frame, [H][W][C] when src_hwc, else [C][H][W], rows src_pitch bytes apart; row b of `dst` is C'
 * planes of OH OW bytes (C' = gray ? 1 : C), rows dst_pitch bytes apart (a slab column obs[:, t] or the last slot of a
 * stacked column).  Per channel:
 *   interp 0, nearest:  out[y][x] = in[y H / OH][x W / OW]  (floor divisions); any OH, OW >= 1, up-scaling included.
 *   interp 1, area:     the exact box average over fractional pixel coverage.  Along an axis, in units of 1 / (W OW) of
 *                       it, destination pixel x covers [x W, (x + 1) W) and source pixel s covers [s OW, (s + 1) OW);
 *                       wx(x, s) is the length of their overlap (the weights of one x sum to W), wy likewise.  With
 *                       S = sum wy wx in and D = H W:  out = (2 S + D) / (2 D), floored: ties round half up.  Needs
 *                       OH <= H and OW <= W.  S is a 32-bit sum: H W > 2^23 is REFUSED (255 H W must stay below 2^31).
 *   gray (C == 3, channel order R, G, B):  (9798 R + 19235 G + 3735 B + 16384) >> 15 of the resized AND ROUNDED channels
 *                       (resize first, then grey, the reference wrapper's order; ITU-R 601 luma in 15-bit fixed point).
 *   Without gray every channel is resized on its own.  OH == H and OW == W is legal (grey-scale or de-interleave alone).
 * This is the exact value of what OpenCV's INTER_AREA approximates in float: a result may differ from OpenCV's by 1 in
 * the last bit on ties.
 * Area launches stage the source rows a strip of output rows covers in LDS (at most 32 KB and 32 rows per work-group,
 * lines padded to an odd dword stride), each source byte read from global memory once, contiguous across a wave: 16 bytes
 * per lane when src, src_pitch and the line length (W C, planar: W) are multiples of 16, dwords when src and src_pitch are
 * multiples of 4, bytewise otherwise; a lane then computes 4 consecutive output pixels from LDS.  A strip of one output row
 * that covers more rows than a band walks them band after band.  Nearest launches gather from global memory (only the bytes kept are read).  Stores
 * are dwords (4 output pixels per lane) when dst, dst_pitch and OH OW are multiples of 4, bytes otherwise: any alignment
 * gives the same bytes.  Frames whose rows exceed the LDS band (W C, or 3 (W + 8) for planar grey, above 32 KB) or whose
 * index products OH H, OW W, H W C leave 31 bits take a bytewise 64-bit path.  dst and src must not share bytes (not
 * checked).
 * Refused before any launch (SF_ERR_ARG): null dst / src; H, W, C, OH or OW < 1; interp not 0 or 1; area with OH > H or
 * OW > W, or with H W > 2^23; gray with C != 3; src_pitch < H W C; dst_pitch < C' OH OW; rows < 0.
 * rows == 0: SF_OK, nothing is launched. */
int sf_frame_resize(void *dst, int64_t dst_pitch, const void *src, int64_t src_pitch, int H, int W, int C, int src_hwc,
                    int OH, int OW, int interp, int gray, int rows, void *stream);

/* ---- synthetic vector env (SURVEY.md §8d "C2 synthetic inputs") ------------------------------------------------
 * Device-resident stand-in for a GPU env (the reference's pattern: sf_examples/brax/train_brax.py:160-204).
 * sf_synth_obs writes frame `step` of envs [env0, env0+B) as u8 [obs_bytes] each, env b at obs + b*env_stride —
 * i.e. straight into slot t of the trajectory slab (zero-copy K1).  sf_synth_step: reward = (action ==
 * (step+env)%num_actions), terminated ~ Bernoulli(1/1024) from the Philox stream.  Bit-reproducible on CPU. */
int sf_synth_obs(uint8_t *obs, int64_t env_stride, int B, int env0, int64_t obs_bytes, uint32_t seed, uint32_t step,
                 void *stream);
int sf_synth_step(const int32_t *actions, int B, int env0, int num_actions, uint32_t seed, uint32_t step,
                  float *rewards, uint8_t *terminated, void *stream);

/* ---- PixelCatch: a learnable pixel game on the device (csrc/sf_pixcatch.hip, envs/pixel_catch.py) ------------------
 * A ball falls down an H x W field and reflects off the side walls; the player moves a paddle along the bottom rows
 * (action 0 stay, 1 left, 2 right; any other value is read as 0).  When the ball reaches the paddle's rows the reward is
 * +1 if their column ranges overlap, else -1, and a new ball is drawn at the top; after `balls` balls terminated = 1 and
 * the env resets itself in the same step (paddle centred, new ball, every plane shows the new first frame).  All
 * arithmetic is integer; sample_factory_amd/envs/pixel_catch.py is the same game in NumPy, bit for bit (observations,
 * rewards, flags, state words), and documents the constants (ball, paddle, speeds: fixed functions of H and W).
 * Randomness: sf_philox4x32_10, counter (draw index, 0, 4, 0), key (seed, env0 + e); words 0, 1, 2 give column, vx and vy
 * by multiply-high.  The draw index lives in the state: no argument changes from step to step.
 * state: int32 [N][sf_pixcatch_state_words(k) = 4 + 3 k], contiguous: {draw index, balls left, vx, vy}, then per plane j
 * {paddle x, ball x, ball y}; plane k - 1 is the current position, plane j the one k - 1 - j steps ago.
 * obs_out: row e is k planes of H W bytes, oldest first, rows out_pitch bytes apart (a slab column obs[:, t + 1]):
 * background 0, paddle 128, ball 255 (the maximum where they overlap).
 * sf_pixcatch_reset writes the first state and observation of envs [env0, env0 + N); sf_pixcatch_step reads actions
 * int32 [N], advances every env by one step and writes observation, rewards f32 [N] and terminated u8 [N].
 * One launch, one work-group per env; the old state is read by every lane before a barrier, written by one lane after
 * it.  The frame is stored in 16-byte units when obs_out, out_pitch and k H W are multiples of 16, in 4-byte units when
 * they are multiples of 4; a unit may straddle a row end or a plane end.  Units away from ball and paddle store zeros; the
 * others are built in registers (16-byte units of a field at least 16 wide whose planes are multiples of 16 bytes: one bit
 * per byte from the rectangles' runs in the unit's two rows, spread to bytes with shifts; any other unit byte by byte with
 * compares and selects).  No sub-dword store touches the frame.
 * Refused before any launch (SF_ERR_ARG): a null pointer; N <= 0; k outside 1 .. 8; balls < 1; a field too small for
 * ball and paddle (or a side above 1024); out_pitch < k H W; obs_out, out_pitch or k H W not a multiple of 4.
 * sf_pixcatch_state_words returns SF_ERR_ARG for k outside 1 .. 8. */
int sf_pixcatch_state_words(int k);
int sf_pixcatch_reset(int32_t *state, uint8_t *obs_out, int64_t out_pitch, int N, int env0, uint32_t seed, int H, int W,
                      int k, int balls, void *stream);
int sf_pixcatch_step(int32_t *state, const int32_t *actions, uint8_t *obs_out, int64_t out_pitch, float *rewards,
                     uint8_t *terminated, int N, int env0, uint32_t seed, int H, int W, int k, int balls, void *stream);
/* Levels: sf_pixcatch_reset_levels / sf_pixcatch_step_levels are the two entry points above plus `decoys` (nd, 0 .. 8),
 * `levels` (L >= 0) and `start_level` (S).  A level places nd static decoys in the field: bs x bs squares of 255 that never
 * move.  Levels change the rendered frame only: state words, rewards and flags are those of the game without decoys, and
 * with decoys = 0 the two entry points ARE sf_pixcatch_reset / sf_pixcatch_step (the same kernel; levels have no effect).
 *   episode   ep = (state[0] - 1) / balls, from the state the launch writes (the draw index counts the balls drawn)
 *   level     w = sf_philox4x32_10(counter (ep, 0, 6, 0), key (seed, env0 + e)); level = S + mulhi(w[0], L) for L > 0 (a
 *             finite set of L levels), S + w[0] for L = 0 (unlimited levels), both mod 2^32
 *   decoy d   w = sf_philox4x32_10(counter (d, 0, 7, 0), key (0x4C564C53, level)): the square at x = mulhi(w[0], W - bs + 1),
 *             y = mulhi(w[1], D); its rows end at H - ph - 1 at the latest, above the paddle's.  Neither the seed nor the
 *             env enters the key: a level looks the same in every run.
 * Counter lane 2 of the library's Philox streams: 6 is the level of an episode, 7 the decoys of a level (0 .. 5: below).
 * A pixel is 255 if it lies in the ball or in a decoy of the episode's level, else 128 if it lies in the paddle, else 0;
 * all k planes show the current episode's decoys.  pixel_catch.py (episode_level, level_decoys, render) is the contract.
 * The work-group keeps ONE plane of the level's decoys in LDS, as the bytes the frame gets (H W + 16 bytes, rounded up to
 * dwords, and a dword): the level is drawn once from uniform values, lane d bs + i draws decoy d and writes row i of it
 * between two barriers, and a store unit ORs the plane's 16 or 4 bytes at its first pixel's index over what it built from
 * ball and paddle (or over zeros).  A unit that holds nothing but decoys costs one LDS read, whatever their number.
 * Refused before any launch (SF_ERR_ARG), on top of the refusals above: decoys outside 0 .. 8; levels < 0; decoys > 0 on a
 * field whose plane exceeds 64 KB of LDS (H W above 65 516 pixels: 255 x 255 runs, 256 x 256 does not). */
int sf_pixcatch_reset_levels(int32_t *state, uint8_t *obs_out, int64_t out_pitch, int N, int env0, uint32_t seed, int H,
                             int W, int k, int balls, int decoys, int levels, uint32_t start_level, void *stream);
int sf_pixcatch_step_levels(int32_t *state, const int32_t *actions, uint8_t *obs_out, int64_t out_pitch, float *rewards,
                            uint8_t *terminated, int N, int env0, uint32_t seed, int H, int W, int k, int balls, int decoys,
                            int levels, uint32_t start_level, void *stream);

/* ---- random-shift augmentation of a minibatch's frames (csrc/sf_augment.hip, --augment_random_shift) ---------------
 * The random shift of RAD / DrQ / DrAC — pad every frame by `pad` pixels with edge replication, crop back to H x W at a
 * random offset — as ONE gather launch.  The reference has no augmentation.  Sample i of the launch is dataset row
 * d = index ? index[i] : offset + i, read at src + (traj_T > 0 ? d + d / traj_T : d) * src_sample_pitch (the learner's
 * row addressing of a [E, T + 1, ...] slab leaf) and written densely at dst + i * dst_sample_pitch (pitches in bytes):
 *   dst[i][c][y][x] = src[row][c][clip(y + dy - pad, 0, H - 1)][clip(x + dx - pad, 0, W - 1)]
 * for elements of elem_bytes = 1 (u8) or 4 (f32) bytes, bit for bit; all C planes of a sample (a frame stack, RGB) move
 * together.  The draw: w = sf_philox4x32_10(counter (draw_id, 0, 5, 0), key (seed, d / recurrence)), m = 2 pad + 1,
 * dx = (w[0] * m) >> 32, dy = (w[1] * m) >> 32 as 64-bit products: both in [0, 2 pad], one draw per recurrence-long
 * chunk of dataset rows, so that a recurrent state never sees the picture jump inside a BPTT chunk.  Counter lane 2 of the
 * library's Philox streams: 0 .. 3 the samplers and synthetic envs of sf_rl.hip, 4 PixelCatch's balls, 5 this draw, 6 and 7
 * PixelCatch's levels and their decoys, 8 .. 10 the cutout, the intensity and the op draw of sf_augment_gather (below).
 * sample_factory_amd/envs/frame_ops.py (random_shift_draws, random_shift_frames) is the same arithmetic in NumPy.
 * pad == 0 is the plain indexed gather (no Philox block is computed); with C = H = 1, W = F it makes the dense copy of a
 * vector key.
 * One work-group per sample: the frame rows a strip of the output reads are staged in LDS as the aligned 16-byte granules
 * that hold them (every source byte is loaded once, nothing bytewise; the clamped border rows and columns come from the
 * staged image), a lane assembles 16 output bytes — a u8 dword inside one row from the 4-byte window of the staged row
 * that holds its clamped columns (the two LDS dwords around it, funnel-shifted) and one byte permute that repeats the edge
 * pixel, an f32 element at its clamped column, a dword with a row end inside it byte by byte from LDS — and stores them
 * as one 16-byte unit; only the bytes in front of a sample's first and behind its last 16-byte boundary are stored singly.  Any alignment of src, dst,
 * the pitches and the sample size gives the same bytes.  Samples whose rows do not fit 64 KB of LDS take a dword-wise path
 * without LDS.  dst and src must not share bytes (not checked); index entries are trusted as the other consumers trust
 * them.
 * Refused before any launch (SF_ERR_ARG): null dst / src; n < 0; pad outside 0 .. 255; elem_bytes not 1 or 4;
 * recurrence < 1; C, H or W < 1; traj_T < 0 or offset < 0; a pitch below C H W elem_bytes.  n == 0: SF_OK, nothing is
 * launched. */
int sf_random_shift_gather(void *dst, int64_t dst_sample_pitch, const void *src, int64_t src_sample_pitch,
                           const int32_t *index, int64_t offset, int64_t n, int traj_T, int C, int H, int W, int elem_bytes,
                           int pad, int recurrence, uint32_t seed, uint32_t draw_id, void *stream);

/* ---- cutout and intensity behind the shift, in the same launch (--augment_cutout, --augment_intensity) -------------
 * sf_augment_gather is sf_random_shift_gather — the same addressing, draws, alignment rules and launch shape — with two
 * more per-sample transformations applied to every output dword in registers before it is stored, in ONE fixed order:
 * shift, then intensity, then cutout.  All planes of a sample are transformed alike.  With mulhi(a, m) = (a * m) >> 32 as
 * a 64-bit product and w = sf_philox4x32_10(counter (draw_id, 0, LANE, 0), key (seed, d / recurrence)):
 *   cutout     LANE = 8 (AUG_LANE_CUTOUT), on when cut_max > 0: ch = lo_h + mulhi(w[0], hi_h - lo_h + 1) with
 *              lo_h = min(cut_min, H), hi_h = min(cut_max, H); cw the same from w[1] and W; y0 = mulhi(w[2], H - ch + 1),
 *              x0 = mulhi(w[3], W - cw + 1).  out[c][y0 .. y0 + ch)[x0 .. x0 + cw) = fill in OUTPUT coordinates: the
 *              rectangle always lies inside the frame and may be all of it.  fill = 0 (0.0f) with cut_fill = 0, the
 *              sample's byte w'[1] >> 24 of the LANE = 9 block with cut_fill = 1 (u8 only).  The fill is not scaled.
 *   intensity  LANE = 9 (AUG_LANE_INTENSITY), on when intensity = A > 0: s = 256 - A + mulhi(w[0], 2 A + 1), in
 *              [256 - A, 256 + A].  u8: min(255, (x * s + 128) >> 8); f32: x * (float)(s / 256), ONE rounded multiply.
 *   LANE = 10  (AUGMENT_LANE_SELECT) is drawn on the host only: which op an SGD step applies under --augment_mix one.
 * sample_factory_amd/envs/frame_ops.py (cutout_draws, intensity_draws, augment_frames, augment_op_of_step) is the same
 * arithmetic in NumPy, bit for bit.  A Philox block is computed per sample only for the ops that are on; with cut_max = 0
 * and intensity = 0 the launch IS sf_random_shift_gather's.  A dword inside one row takes the scale and a byte select
 * between itself and the fill (the selector from its row and its columns against the rectangle: interior, edge and outside
 * dwords run the same instructions); bytes gathered singly take the same arithmetic per pixel.
 * Refused before any launch (SF_ERR_ARG): everything sf_random_shift_gather refuses; cut_max outside 0 .. 65535; with
 * cut_max > 0, cut_min < 1 or cut_min > cut_max; cut_fill not 0 or 1; cut_fill = 1 with elem_bytes = 4; intensity outside
 * 0 .. 255.  n == 0: SF_OK, nothing is launched. */
int sf_augment_gather(void *dst, int64_t dst_sample_pitch, const void *src, int64_t src_sample_pitch, const int32_t *index,
                      int64_t offset, int64_t n, int traj_T, int C, int H, int W, int elem_bytes, int pad, int cut_min,
                      int cut_max, int cut_fill, int intensity, int recurrence, uint32_t seed, uint32_t draw_id, void *stream);

/* ---- K2/K3/K8/K9/K15/K18: actor-critic network (fp32 MFMA) -------------------------------------------------------
 * model/encoder.py:90-150 (conv head + MLP), model/actor_critic.py:160-195 (critic_linear + distribution_linear),
 * utils/normalize.py:51-70 + rl_utils.py:36-42 (u8 -> f32, -mean, *1/scale fused into the first layer's loader;
 * the f32 copy of the observations is never materialised).
 *
 * One implicit-GEMM kernel family, out[M,N] = act(gather(in)[M,K] * W[K,N] + bias), for conv fwd, linear fwd,
 * data-gradient and weight-gradient; see DESIGN.md.  Activations are NHWC ([sample, oh, ow, c]); weights are
 * stored K-major [KH*KW*Cin, Cout] (k = (kh*KW + kw)*Cin + c) — conversion to/from the reference's OIHW layout
 * happens in state_dict()/load_state_dict() on the host side. */
typedef struct {
    int32_t Cin, H, W;        /* input  feature map (per sample) */
    int32_t Cout, KH, KW, stride;
    int32_t OH, OW;           /* output feature map */
    int32_t in_u8;            /* input format: 0 = f32 NHWC activations; 1 = raw u8 NCHW observation frames; 2 = f32
                                 NCHW observation frames (e.g. Box(0, 1, (C, H, W), float32)).  Frames (1, 2): the
                                 loader applies (x - sub_mean) * inv_scale, weights use k = (c*KH + kh)*KW + kw, there
                                 is no data gradient.  Format 2 runs on the f32 matrix instructions only (16-byte loads
                                 when KW, stride and W are multiples of 4 and the frames 16-byte aligned, scalar loads
                                 otherwise); no other kernel family and no *_supported query but sf_conv_norm_supported
                                 takes it.  (Format 2 was added without an ABI version change: the struct layout and
                                 the meaning of 0 / 1 are unchanged, and a value outside 0..2 is now refused.) */
    int32_t relu;             /* activation kind: 0 none, 1 ReLU, 2 tanh, 3 ELU(alpha=1) (model/model_utils.py:27-35).
                                 forward: fused in the epilogue; sf_conv_dgrad: the kind that PRODUCED in_act, whose
                                 derivative (through the stored output) is fused into the dgrad epilogue */
    int32_t traj_T;           /* >0: input rows live in a trajectory slab [E, T+1, ...]; logical sample d (flat dataset
                                 index e*T+t, learner.py:1009-1012) is slab row e*(T+1)+t — read in place, no batcher
                                 copy (batcher.py:192-212) and no [:, :-1] reshape copy (learner.py:1005-1012) */
    float sub_mean, inv_scale;
} sf_conv_desc;

/* forward: in = u8 NCHW [n, Cin,H,W] (in_u8 = 1), f32 NCHW [n, Cin,H,W] (in_u8 = 2) or f32 NHWC [n,H,W,Cin]; sample i of
 * the batch is input row
 * (index ? index[i] : offset+i) * in_sample_stride (elements).  out f32 NHWC [n,OH,OW,Cout].
 * workspace (optional, >= sf_conv_fwd_workspace bytes, 16-byte aligned): lets small launches (e.g. the 3136->512
 * layer at inference batch 4096: 256 tiles for 256 CUs) split the reduction over gridDim.z and finish with a
 * deterministic ordered sum (+bias, ReLU); NULL = never split.
 * Arithmetic: f32 operands, f32 accumulation on the f32 matrix instructions.  One dispatch differs: the Nature-CNN
 * first layer on raw u8 frames (in_u8, 4x84x84, 8x8 stride 4, Cout <= 32, n >= 256, integer sub_mean in [0, 255]) runs
 * sf_conv_fwd / sf_conv_wgrad on the bf16 matrix instruction with operands that are EXACT in bf16 (pixel - mean; the f32
 * weights / output gradients split exactly into three bf16 terms): every product is exact, accumulation is f32, and
 * inv_scale multiplies the accumulated sum (csrc/sf_nn_u8.h; SF_CONV1_BF16=0 selects the f32 kernels). */
int64_t sf_conv_fwd_workspace(int64_t n, const sf_conv_desc *h_desc);
int sf_conv_fwd(const void *in, int64_t in_sample_stride, const int32_t *index, int64_t offset, const float *w,
                const float *bias, float *out, int64_t n, const sf_conv_desc *h_desc, void *workspace,
                int64_t workspace_bytes, void *stream);
/* weight/bias gradient: dw[K,Cout] (+)= gather(in)^T * dout, db[Cout] = sum dout; dout already has the ReLU mask
 * applied (sf_conv_fwd's consumer does it).  Deterministic two-stage split reduction; workspace >=
 * sf_conv_wgrad_workspace(...) bytes. */
int64_t sf_conv_wgrad_workspace(int64_t n, const sf_conv_desc *h_desc);
int sf_conv_wgrad(const void *in, int64_t in_sample_stride, const int32_t *index, int64_t offset, const float *dout,
                  float *dw, float *db, int64_t n, const sf_conv_desc *h_desc, void *workspace, void *stream);
/* data gradient: din[n,H,W,Cin] = conv_transpose(dout, w) * act'(in_act) (in_act = this layer's input activation,
 * i.e. the previous layer's post-activation output, kind = h_desc->relu; NULL = no activation derivative). */
int sf_conv_dgrad(const float *dout, const float *w, const float *in_act, float *din, int64_t n,
                  const sf_conv_desc *h_desc, void *stream);
/* ReLU SIGN-BIT MASKS between a layer's forward and its weight gradient (model/encoder.py:90-119 under autograd keeps
 * the whole activation for ReLU's backward; here 1 bit per element).  sf_conv_fwd_relu_mask = sf_conv_fwd that also
 * records relu_mask[n*OH*OW] (u32 per output pixel, bit c = channel c of that pixel is > 0; Cout = 32);
 * sf_conv_wgrad_relu_mask = sf_conv_wgrad whose `dout` is the gradient wrt the layer's ReLU OUTPUT, NOT yet masked: the
 * kernel applies the recorded bits on the way in (weight AND bias gradient).  The data-gradient launch that produced
 * `dout` is then called with in_act = NULL and never re-reads this layer's activation (1.68 GB per C2 minibatch).
 * sf_conv_relu_mask_supported: 1 for the launches both kernels take (first layer on raw u8 frames on the exact-product
 * bf16 kernels, Cout == 32, ReLU); otherwise use the plain entry points with in_act. */
int sf_conv_relu_mask_supported(int64_t n, const sf_conv_desc *h_desc);
int sf_conv_fwd_relu_mask(const void *in, int64_t in_sample_stride, const int32_t *index, int64_t offset, const float *w,
                          const float *bias, float *out, uint32_t *relu_mask, int64_t n, const sf_conv_desc *h_desc,
                          void *stream);
int sf_conv_wgrad_relu_mask(const void *in, int64_t in_sample_stride, const int32_t *index, int64_t offset,
                            const float *dout, const uint32_t *relu_mask, float *dw, float *db, int64_t n,
                            const sf_conv_desc *h_desc, void *workspace, void *stream);

/* First conv layer on raw u8 frames WITH the observation normaliser applied in the loader — cfg.normalize_input=True on
 * image observations (cfg/cfg.py:337-341: the default; sf_examples/atari/atari_params.py:39).  Replaces, for the launches
 * it takes, the reference's f32 materialisation of every frame (utils/normalize.py:40-70: obs.float() clone, sub_, mul_;
 * running_mean_std.py:79-110: x.sub_(mu).mul_(1/sigma).clamp_(-5, 5)) followed by conv1 (model/encoder.py:90-119):
 * x' = clamp(((float(u8) - sub_mean) * inv_scale - mu[d]) * rstd[d], +-5) is formed where the byte enters LDS, d = the
 * byte's offset inside the NCHW frame; mu / rstd = the f32 tables [Cin*H*W] sf_obsnorm_update maintains (16-byte
 * aligned).  No normalised copy of the frames exists in HBM (28 KB instead of 28 + 2 x 113 KB per
 * frame and pass).  sf_conv_wgrad_norm = the weight / bias gradient against the same normalised input (dout already
 * masked by the activation derivative; workspace >= sf_conv_wgrad_workspace bytes).  sf_conv_norm_supported: 1 for the
 * launches these take: every valid descriptor of u8 frames (in_u8 = 1) or f32 frames (in_u8 = 2), any geometry, any n.
 * They run on the f32 matrix instructions with x' formed in the loader of the register-staged kernels: vector loads
 * (4 u8 pixels per 4-byte word / 4 f32 pixels per 16 bytes, and 16 bytes of each table) when KW, stride, W and Cout are
 * multiples of 4, the frames and their sample stride 4-byte (u8) / 16-byte (f32) aligned and the tables 16-byte aligned;
 * the scalar loader otherwise (tables and f32 frames 4-byte aligned).  The Nature-CNN conv1 on u8 frames (4x84x84 -> 32,
 * 8x8 stride 4, aligned operands) runs on the strip-image kernels instead.  It answers 0 for f32 NHWC activations
 * (in_u8 = 0) and under SF_CONV1_NORM=0: then sf_obsnorm_apply + sf_conv_fwd on the f32 batch.  Sample addressing
 * (index | offset, traj_T) as sf_conv_fwd. */
int sf_conv_norm_supported(int64_t n, const sf_conv_desc *h_desc);
int sf_conv_fwd_norm(const void *in, int64_t in_sample_stride, const int32_t *index, int64_t offset, const float *mu,
                     const float *rstd, const float *w, const float *bias, float *out, int64_t n,
                     const sf_conv_desc *h_desc, void *stream);
int sf_conv_wgrad_norm(const void *in, int64_t in_sample_stride, const int32_t *index, int64_t offset, const float *mu,
                       const float *rstd, const float *dout, float *dw, float *db, int64_t n, const sf_conv_desc *h_desc,
                       void *workspace, void *stream);

/* Inference on vector observations in one launch: [(x - sub_mean) * inv_scale -> (optional) running mean/std
 * normalisation with clamp +-5] -> act(x W1 + b1) -> act(. W2 + b2); utils/normalize.py:24-70 + model/encoder.py:72-87
 * (MlpEncoder with two layers).  x: f32 rows of D values, x_stride floats apart (e.g. slab obs[:, t]); w1 [D, H1], w2
 * [H1, H2] K-major; mu / rstd: [D] tables of the observation normaliser or both NULL; act: 0 none, 1 relu, 2 tanh, 3 elu;
 * out [n, H2].  Same arithmetic (fmaf chain, ascending k) as sf_conv_fwd on the two layers; needs H1, H2 % 8 == 0 and
 * (D*H1 + H1*H2 + 64*(D+H1)) * 4 <= 64 KiB, else returns an error (use the layer kernels). */
int sf_mlp2_fwd(const float *x, int64_t x_stride, int64_t n, int D, float sub_mean, float inv_scale, const float *mu,
                const float *rstd, const float *w1, const float *b1, int H1, const float *w2, const float *b2, int H2,
                int act, float *out, void *stream);

/* rollout: rnn_states[:, t+1] = new_state * (1 - done) (batched_sampling.py:332-335) in one launch; h (and c for an
 * LSTM) are the cell's [B, H] outputs, dones the u8 [B] column traj.dones[:, t] (element stride done_stride), out the
 * [B, H or 2H] view traj.rnn_states[:, t+1] (row stride out_stride floats). */
int sf_rnn_store_state(const float *h, const float *c, const uint8_t *dones, int64_t done_stride, float *out,
                       int64_t out_stride, int64_t B, int H, void *stream);

/* sf_rnn_store_state for a rollout that tracks inactive agents (non_batched_sampling.py:605-612): a row
 * whose step was recorded with policy_id < 0 keeps the state it had,
 *   out[b] = (policy_id[b] < 0 ? prev[b] : [h[b] | c[b]]) * (1 - done[b]).
 * prev: the [B, H or 2H] view traj.rnn_states[:, t] (this layer's columns, row stride prev_stride floats); policy_id: the
 * i32 [B] column traj.policy_id[:, t] (element stride pid_stride).  With no negative policy_id the bits of
 * sf_rnn_store_state.  Refused before any launch (-1): what sf_rnn_store_state refuses, a null prev or policy_id, a
 * row stride below the row width, an out whose extent overlaps prev's. */
int sf_rnn_store_state_held(const float *h, const float *c, const uint8_t *dones, int64_t done_stride, const float *prev,
                            int64_t prev_stride, const int32_t *policy_id, int64_t pid_stride, float *out,
                            int64_t out_stride, int64_t B, int H, void *stream);

/* training pass of a recurrent model (learner.py:557-569, rnn_utils.py:59-105): minibatch = Cn chunks of R consecutive
 * dataset rows, chunk c starting at row index[c*R] (index != NULL: a permuted minibatch, every chunk's R rows consecutive
 * in it) or offset + c*R.  keep_tm [R][Cn] f32 = 0 where the step is done or invalid (the state is zeroed after it), else
 * 1; h0 [Cn][S] = rnn_states[chunk start] (dones / valids: u8 per dataset row; rnn_states [rows][S] f32, or — traj_T > 0 —
 * the slab itself, [E][traj_T + 1][S] read in place: dataset row e*T+t is slab row e*(T+1)+t, no compaction copy). */
int sf_rnn_chunk_setup(const uint8_t *dones, const uint8_t *valids, const float *rnn_states, const int32_t *index,
                       int64_t offset, int Cn, int R, int S, int traj_T, float *keep_tm, float *h0, void *stream);

/* ---- fused LSTM sequence passes (config 5: LSTM-512 core, BPTT over recurrence-length chunks) -------------------
 * model/core.py:19-64 + algo/learning/rnn_utils.py:114-158 as ONE persistent launch per pass instead of
 * {recurrent GEMM, cell, carries} x R launches: every work-group keeps its slice of W_hh in LDS for all R steps and
 * exchanges h_t (forward) / gate gradients (backward) with the other work-groups of its row group through L2.
 * Layouts (all f32, row-major, time-major over the R steps of Cn chunks): gx [R][Cn][4H] = x W_ih^T + b_ih;
 * whh [H][4H] (K-major, torch gate order i,f,g,o); keep [R][Cn] = 1 - done_or_invalid; gates [R][Cn][4H] (post-
 * activation); hprev / cprev [R+1][Cn][H] with slot 0 = the chunk-start state on entry, slot t+1 = state_t * keep[t];
 * hout / cout [R][Cn][H] the unmasked new state.  sync: >= 129 device uint32; words 0..127 are the hand-off counters
 * (zeroed by the call), word 128 is the STICKY abort word: set by a pass that gave up waiting for a work-group, never
 * cleared by the library (the caller zeroes it once, e.g. at the start of Learner.train, and hands the same word to
 * sf_adam_step / sf_lamb_step as `skip_flag`, so that the garbage gradients of an aborted pass never reach the weights).  sf_lstm_seq_supported: 1 when (Cn, H) can
 * take this path on the current device AND is offered it (H in {256, 512}, Cn up to the rows of one launch: 16 hidden units
 * per work-group with their W_hh slice resident in LDS; grid <= #CUs.  The passes run more chunks as row slabs, below, but
 * there the per-step launches measured 9 - 55 % faster, DESIGN.md 3.4, so the query answers 0 and only a direct call takes
 * them), else use the row-owned passes below (H <= 128), the wide passes (H = 1024) or
 * sf_rnn_cell_fwd/bwd per step.
 * sf_lstm_seq_bwd: dout [R][Cn][H] = dL/d hout; writes dgx [R][Cn][4H] = dL/d(gate pre-activations) (= the gradient of
 * both gx and h W_hh^T + b_hh); the carries of dL/dh and dL/dc live in registers.
 * Row slabs: one launch serves at most 8 * 256 rows (fewer row groups on a device with fewer CUs:
 * sf_rnn_seq_slab_rows).  A call with more chunks runs as consecutive launches on `stream`, each over a slab of rows
 * [r0, r1) of the same dense buffers (Cn stays the row pitch); the counters are zeroed before every launch, the abort
 * word never; once it is set the remaining slabs are still enqueued and return at their first wait.  Every slab is launched
 * with the plan a stand-alone call on r1 - r0 rows gets, so its rows are bit-identical to that call's, and a call that fits
 * one launch is exactly that launch.  Whatever the slabs, a hand-off tensor is addressed as a whole through 32-bit offsets:
 * (R+1) Cn H 4 and R Cn G H 4 bytes must stay below 2 GiB, and the FORWARD pass refuses a shape whose backward pass would be
 * refused, so a pass pair fails before anything runs. */
int sf_lstm_seq_supported(int Cn, int H);
int sf_lstm_seq_fwd(const float *gx, const float *whh, const float *bhh, const float *keep, float *gates, float *hprev,
                    float *hout, float *cprev, float *cout, uint32_t *sync, int R, int Cn, int H, int env_major,
                    void *stream);
int sf_lstm_seq_bwd(const float *dout, const float *gates, const float *cprev, const float *cout, const float *keep,
                    const float *whh, float *dgx, uint32_t *sync, int R, int Cn, int H, int env_major, void *stream);
/* env_major (all four passes): hout / dout are [Cn][R][H] — the row order of the minibatch (chunk c, step t = row c*R + t
 * of the core's output and of its gradient) — instead of time-major [R][Cn][H]: the caller needs no transpose copies
 * around the pass.  Everything else stays time-major. */

/* the same two passes for a GRU-512 core (the reference's DEFAULT: cfg rnn_type=gru, rnn_size=512; model/core.py:19-64).
 * gx [R][Cn][3H], whh [H][3H], bhh [3H] (torch gate order r,z,n); gates [R][Cn][4H] = {r, z, n, hn} with
 * hn = h W_hn^T + b_hn (the recurrent part of the candidate gate, needed by the backward pass); hprev / hout as above.
 * Backward: hprev = the forward pass's buffer; writes dgx [R][Cn][3H] = {dr, dz, dn} (gradient of gx: W_ih, encoder)
 * and dgh [R][Cn][3H] = {dr, dz, dn * r} (gradient of h W_hh^T + b_hh: W_hh / b_hh, and the hand-off payload of the
 * pass); the direct path dL/dh_prev += dh * z and the carry stay in registers.  Supported shapes: sf_lstm_seq_supported. */
int sf_gru_seq_fwd(const float *gx, const float *whh, const float *bhh, const float *keep, float *gates, float *hprev,
                   float *hout, uint32_t *sync, int R, int Cn, int H, int env_major, void *stream);
int sf_gru_seq_bwd(const float *dout, const float *gates, const float *hprev, const float *keep, const float *whh,
                   float *dgx, float *dgh, uint32_t *sync, int R, int Cn, int H, int env_major, void *stream);

/* Forward sequence passes WITH the input projection (model/core.py:37-64: nn.LSTM / nn.GRU compute x W_ih^T + b_ih
 * themselves): instead of gx [R][Cn][G*H] — written by a GEMM launch and read back by the pass — the pass takes
 * x [R][Cn][Kx] (time-major core input), wih_t [G*H][Kx] (W_ih in torch's own [gate column][input] layout) and
 * bih [G*H]; every work-group multiplies its own gate columns, the products of step t+1 run while it waits for the
 * other work-groups' h_t.  gx_t = x_t W_ih^T + b_ih is formed in f32 exactly as the GEMM's epilogue does (MFMA sum, then
 * + b_ih), then used as in sf_lstm_seq_fwd / sf_gru_seq_fwd.  sf_seq_fwd_x_supported: Kx == 64 and row groups of at
 * most 128 rows (Cn <= 1024 on 256 CUs; one launch, never slabs), else project with sf_conv_fwd_t and call the gx form. */
int sf_seq_fwd_x_supported(int Cn, int H, int Kx);
int sf_lstm_seq_fwd_x(const float *x, const float *wih_t, const float *bih, int Kx, const float *whh, const float *bhh,
                      const float *keep, float *gates, float *hprev, float *hout, float *cprev, float *cout,
                      uint32_t *sync, int R, int Cn, int H, int env_major, void *stream);
int sf_gru_seq_fwd_x(const float *x, const float *wih_t, const float *bih, int Kx, const float *whh, const float *bhh,
                     const float *keep, float *gates, float *hprev, float *hout, uint32_t *sync, int R, int Cn, int H,
                     int env_major, void *stream);

/* ---- row-owned sequence passes for narrow cores (H in {32, 64, 128}; kind 0 = GRU, 1 = LSTM) ------------------------
 * The same two BPTT passes as above for the widths at which the whole W_hh fits one work-group (GRU-64: 48 KB): instead
 * of splitting the hidden units across work-groups that hand h_t to each other through L2, ONE work-group owns a tile of
 * chunk rows (16; 32 at H = 32) and walks all R steps of them alone, grid = ceil(Cn / tile).  No `sync` argument: no
 * counters, no polling, no abort word; any Cn > 0.  W_hh stays in LDS for the whole pass (H <= 64; streamed from L2 at
 * H = 128), h / c and the dL/dh, dL/dc carries stay in registers, the recurrent products run on v_mfma_f32_16x16x4_f32
 * in one fixed order over k, so a row's results are bit-identical whatever Cn and whatever else is in the batch; the
 * cell arithmetic is the device code of sf_rnn_cell_fwd / sf_rnn_cell_bwd.
 * Buffers and layouts are exactly those of sf_lstm_seq_* / sf_gru_seq_*: gx [R][Cn][G*H], whh [H][G*H], bhh [G*H],
 * keep [R][Cn], gates [R][Cn][4H] (GRU {r, z, n, hn}), hprev / cprev [R+1][Cn][H] (slot 0 given on entry, slot t+1 =
 * state_t * keep[t]; written, never read back), hout / cout [R][Cn][H] (hout / dout [Cn][R][H] when env_major); cprev /
 * cout are NULL for a GRU.  Backward: writes dgx [R][Cn][G*H] and, GRU only, dgh [R][Cn][3H] = {dr, dz, dn * r} (LSTM:
 * dgh may be NULL, both gradients are dgx; hprev may be NULL); the W_hh / b_hh gradient is sf_conv_wgrad over
 * (hprev[0..R), dgh) as for the other passes.  whh must be 16-byte aligned.
 * sf_rnn_rowseq_supported: 1 for the (kind, Cn, H) these passes take; they are offered where they measured faster than
 * the per-step launches (tools/rowseq_bench.py).  An unsupported shape or a bad operand returns an
 * error before anything is launched. */
int sf_rnn_rowseq_supported(int kind, int Cn, int H);
int sf_rnn_rowseq_fwd(int kind, const float *gx, const float *whh, const float *bhh, const float *keep, float *gates,
                      float *hprev, float *hout, float *cprev, float *cout, int R, int Cn, int H, int env_major, void *stream);
int sf_rnn_rowseq_bwd(int kind, const float *dout, const float *gates, const float *hprev, const float *cprev,
                      const float *cout, const float *keep, const float *whh, float *dgx, float *dgh,
                      int R, int Cn, int H, int env_major, void *stream);

/* ---- persistent sequence passes at H = 1024 (kind 0 = GRU, 1 = LSTM) ---------------------------------------------------
 * The scheme of sf_lstm_seq_* / sf_gru_seq_* with 8 hidden units per work-group, at which both W_hh slices fit LDS
 * (forward 32 gate columns x 1028 floats, backward 8 rows x (G*H + 4) floats); 128 work-groups form a row group, a launch
 * serves min(8, #CUs / 128) row groups of at most 256 rows (512 rows on 256 CUs) and more rows run as slabs, exactly as
 * above.  Operands, layouts, `sync` (counters + sticky abort word) and env_major are those of sf_lstm_seq_* /
 * sf_gru_seq_*; cprev / cout are NULL for a GRU; backward: hprev and dgh may be NULL for an LSTM (both gradients are dgx).
 * Exact-f32 MFMA products in one k-order per output element (it depends on the hidden unit only), so a row's results are
 * bit-identical whatever Cn, slab or row group it lands in; the cell arithmetic is the device code of sf_rnn_cell_fwd /
 * sf_rnn_cell_bwd.  hprev, whh and the gate-gradient payload (dgx for an LSTM, dgh for a GRU) must be 16-byte aligned.
 * sf_rnn_wideseq_supported: 1 for H == 1024, kind 0 / 1, 0 < Cn <= 64 (GRU) / 512 (LSTM) on a device with at least 128
 * CUs: the chunk range in which Learner.train was shown faster than on the per-step launches by more than the spread
 * (the GRU is level with them at 512 chunks, and at 2048 the per-step GEMMs win by 1.8 - 1.9 x).  The two passes themselves run any Cn > 0 at this width; any other kind or
 * width, or a bad operand, returns an error before anything is launched.
 * sf_rnn_seq_slab_rows(kind, H, pass): the largest number of rows ONE launch of the forward (pass 0) / backward (pass 1)
 * pass serves on the current device, for every width with a persistent pass (256, 512, 1024); 0 for any other width. */
int sf_rnn_wideseq_supported(int kind, int Cn, int H);
int sf_rnn_seq_slab_rows(int kind, int H, int pass);
int sf_rnn_wideseq_fwd(int kind, const float *gx, const float *whh, const float *bhh, const float *keep, float *gates,
                       float *hprev, float *hout, float *cprev, float *cout, uint32_t *sync, int R, int Cn, int H,
                       int env_major, void *stream);
int sf_rnn_wideseq_bwd(int kind, const float *dout, const float *gates, const float *hprev, const float *cprev,
                       const float *cout, const float *keep, const float *whh, float *dgx, float *dgh, uint32_t *sync,
                       int R, int Cn, int H, int env_major, void *stream);

/* The name of the kernel instantiation a fused pass runs, as rocprofv3 prints it (`k_lstm_seq_fwd<512, 16, 2, 0>`,
 * `k_gru_seq_bwd_r<256, 4>`, `k_rowseq_fwd<1, 64>`, `k_wideseq_bwd<0, 2>`): answered from the launch plan and the dispatch
 * table the entry points themselves use.  family: 0 = sf_lstm_seq_* / sf_gru_seq_* (H 256 / 512), 1 = sf_rnn_rowseq_*,
 * 2 = sf_rnn_wideseq_*; kind 0 = GRU, 1 = LSTM; pass 0 = forward, 1 = backward; Kx != 0: the forward pass with the input
 * projection fused in (sf_*_seq_fwd_x), 0: the gx form.  A call of more than sf_rnn_seq_slab_rows rows is named by its
 * first, full slab (the shorter last slab may run another instantiation).  out: at least 48 bytes.  Fails, with a message,
 * for a (family, kind, Cn, H, Kx) the entry point refuses; the limits that depend on R (2 GiB) are not its business. */
int sf_rnn_seq_kernel_name(int family, int kind, int pass, int Cn, int H, int Kx, char *out, int cap);

/* ---- data-parallel learner replicas (SURVEY.md §8(b) "DP -> sf_allreduce_grads", §8(e)) ----------------------------
 * New capability: the reference runs ONE learner per policy (algo/utils/shared_buffers.py:26-32), so these replace no
 * reference function; a host without torch.distributed binds them for the exchange algo/learning/learner.py performs
 * per SGD step.  One RCCL communicator per rank, created once on the rank's current device: rank 0 calls
 * sf_dp_unique_id and ships the SF_DP_UNIQUE_ID_BYTES bytes to the other ranks by any host channel; every rank then
 * calls sf_dp_comm_create (a collective: returns when all nranks ranks joined).  sf_allreduce_grads: in-place SUM of n
 * fp32 values over the ranks (each replica's gradient already carries the GLOBAL 1/n_valid), enqueued on `stream`;
 * calls on one communicator must be issued in the same order on every rank.  sf_dp_allreduce_f64: the 3-double
 * moment / loss-scalar exchanges (op 0 = sum, 1 = max).  sf_dp_broadcast: root's bytes to everyone (initial weights).
 * librccl.so.1 is loaded on first use (dlopen), never at library load. */
#define SF_DP_UNIQUE_ID_BYTES 128
int sf_dp_unique_id(void *out_id);
int sf_dp_comm_create(const void *id_bytes, int nranks, int rank, void **comm_out);
int sf_dp_comm_destroy(void *comm);
int sf_dp_comm_info(void *comm, int *nranks, int *rank);
int sf_allreduce_grads(void *comm, float *grads, int64_t n, void *stream);
int sf_dp_allreduce_f64(void *comm, double *buf, int64_t n, int op, void *stream);
int sf_dp_broadcast(void *comm, void *buf, int64_t nbytes, int root, void *stream);

/* ---- one-shot ("direct") exchange for small buckets (<= 8 MB never goes round a ring) -----------------
 * Every rank owns a mailbox in its HBM which every peer maps (hipIpc) and reads over xGMI: ONE kernel per rank and call
 * publishes the bucket, waits for the peers' flags and adds the peers' copies in rank order (bit-identical results on all
 * ranks; one hop instead of 2 (W-1)).  Meant for the 0.31 MB conv bucket of the gradient, which completes last in the
 * backward pass, and the 24 ... 400-byte moment / loss-scalar buckets; larger buckets stay on sf_allreduce_grads.
 * sf_dp_oneshot_create: allocates the mailbox for buckets of up to max_bytes and writes its SF_DP_IPC_HANDLE_BYTES handle
 * to handle_out; the host ships every rank's handle to every rank (rank order, any channel) and calls
 * sf_dp_oneshot_connect.  The all-reduce calls are collective, in place, enqueued on `stream`, and must be issued in the
 * same order on every rank (they carry a sequence number).  A peer that does not arrive within 5 s sets the context's error
 * word (sf_dp_oneshot_status) instead of hanging the queue.  No reference counterpart (one learner per policy:
 * sample_factory/algo/utils/shared_buffers.py:26-32). */
#define SF_DP_IPC_HANDLE_BYTES 64
int sf_dp_oneshot_create(int nranks, int rank, int64_t max_bytes, void **ctx_out, void *handle_out);
int sf_dp_oneshot_connect(void *ctx, const void *all_handles /* nranks x SF_DP_IPC_HANDLE_BYTES, rank order */);
int sf_dp_oneshot_allreduce_f32(void *ctx, float *buf, int64_t n, void *stream);            /* SUM */
int sf_dp_oneshot_allreduce_f64(void *ctx, double *buf, int64_t n, int op, void *stream);   /* op 0 = SUM, 1 = MAX */
int sf_dp_oneshot_status(void *ctx);
int sf_dp_oneshot_destroy(void *ctx);

/* action means squashed to [-scale, scale] (continuous_tanh_scale > 0, model/action_parameterization.py:62-66), in
 * place on columns [col0, col0+ncols) of a row-major [n, ld] matrix: y = tanh(x/scale)*scale; backward: g *= 1-(y/scale)^2
 * with y the squashed output. */
int sf_tanh_scale_fwd(float *x, int ld, int64_t n, int col0, int ncols, float scale, void *stream);
int sf_tanh_scale_bwd(float *g, const float *y, int ld, int64_t n, int col0, int ncols, float scale, void *stream);

/* Two linear layers into ONE accumulator: out [n][N] = a1 w1t^T + a2 w2t^T + bias1 + bias2 (a_i: [n][K_i] rows lda_i
 * floats apart; w_it: [N][K_i], i.e. torch's own Linear / LSTM weight layout; biases may be NULL).  One inference step
 * of model/core.py:37-64's nn.LSTM is this launch on (x, weight_ih_l0, bias_ih_l0) and (h, weight_hh_l0, bias_hh_l0)
 * followed by sf_rnn_cell_fwd(gh = NULL): the short first product (K1 = 64) rides in the pipeline of the long one instead
 * of being a launch of its own.  gru_H > 0 (nn.GRU, N = 4 * gru_H, w_it = weight_{ih,hh}_l0 [3H][K_i]): the candidate
 * gate's two parts stay apart — columns [0,2H) both products + both biases, [2H,3H) the first layer's rows 2H.. only,
 * [3H,4H) the second layer's rows 2H.. only — which is what sf_rnn_cell_fwd(kind 0, gh = NULL) reads.  K1, K2 multiples of
 * 32; sf_linear_fwd_dual_supported: the launch fills the chip (else use two sf_conv_fwd launches). */
int sf_linear_fwd_dual_supported(int64_t n, int N, int K1, int K2);
int sf_linear_fwd_dual(const float *a1, int64_t lda1, const float *w1t, const float *bias1, int K1, const float *a2,
                       int64_t lda2, const float *w2t, const float *bias2, int K2, float *out, int64_t n, int N,
                       int gru_H, void *stream);

/* Forward for the dense hot layers through the gfx950 LDS-DMA path: same result contract as sf_conv_fwd, but the
 * weights are given Cout-major, wt[Cout, K] (sf_transpose of the canonical [K, Cout] array), the input must be f32
 * NHWC with Cin % 32 == 0, dense samples (no index gather), 16-byte aligned.  sf_conv_fwd_t_supported says whether a
 * launch qualifies (and is large enough to be worth it); everything else goes through sf_conv_fwd.  A wide layer with
 * a long reduction and few rows (the fc layer of one rollout step) is split along K: sf_conv_fwd_t_workspace gives the
 * scratch bytes such a launch needs (0 = none; 16-byte aligned; the call fails loudly if it is missing). */
int sf_conv_fwd_t_supported(int64_t n, const sf_conv_desc *desc);
int64_t sf_conv_fwd_t_workspace(int64_t n, const sf_conv_desc *desc);
int sf_conv_fwd_t(const float *in, int64_t in_sample_stride, const float *wt, const float *bias, float *out,
                  int64_t n, const sf_conv_desc *desc, void *workspace, int64_t workspace_bytes, void *stream);
int sf_transpose(const float *w, float *wt, int K, int N, void *stream); /* wt[N,K] = w[K,N]^T */

/* The same forwards with an OUTPUT sample stride (floats; sign-bit words: mask_sample_stride u32 words): sample s, pixel p
 * is written to out + s * out_sample_stride + p * Cout, with the arithmetic and the stores of the dense entry point.  One
 * rollout step can so write slot t of an activation buffer laid out [E, T, OH*OW, Cout]; the next layer reads that slot
 * through its input stride, and the learner reads rows [e*T + t] of the buffer as the dense activation of its dataset
 * rows.  Only the launches whose dense kernel has a strided twin are taken: sf_conv_fwd_os_supported(op, ...) with op = 0
 * for sf_conv_fwd_relu_mask_os (k_conv1_u8_bf16_w_os) and op = 3 for sf_conv_fwd_t_os (k_fwd_glds_zt_os, k_fwd_img_os; never
 * split along K, so no workspace).  The strides must be multiples of 4 floats and at least one sample long, out 16-byte
 * aligned. */
int sf_conv_fwd_os_supported(int op, int64_t n, const sf_conv_desc *desc, int64_t in_sample_stride,
                             int64_t out_sample_stride);
int sf_conv_fwd_relu_mask_os(const void *in, int64_t in_sample_stride, const int32_t *index, int64_t offset,
                             const float *w, const float *bias, float *out, int64_t out_sample_stride,
                             uint32_t *relu_mask, int64_t mask_sample_stride, int64_t n, const sf_conv_desc *h_desc,
                             void *stream);
int sf_conv_fwd_t_os(const float *in, int64_t in_sample_stride, const float *wt, const float *bias, float *out,
                     int64_t out_sample_stride, int64_t n, const sf_conv_desc *desc, void *stream);
/* ... in TWO SEGMENTS of samples: a rollout launch of n trajectories of which only the first keep_n belong to the learner's
 * first minibatch (0 <= keep_n <= n).  Samples s < keep_n are read and written exactly as above (in / in_sample_stride, out /
 * out_sample_stride, relu_mask / mask_sample_stride).  Samples s >= keep_n are read from in2 + (s - keep_n) * H*W*Cin and written
 * to out2 + (s - keep_n) * OH*OW*Cout, both dense (the ordinary activation buffer), and their sign-bit words are not stored.
 * in2 / out2 16-byte aligned; the pointers of an empty segment are not looked at.  Same kernels (the entry points above are
 * their keep_n = n case), same bytes as the dense entry point in both segments: k_conv1_u8_bf16_w_os and k_fwd_img_os select
 * the bases per sample, k_fwd_glds_zt_os cuts its row tiles per segment and runs the dense segment's tiles through the body
 * of k_fwd_glds_zt.  The frames of sf_conv_fwd_relu_mask_os2 have one segment.  sf_conv_fwd_t_os2 also takes a linear layer
 * (H = W = 1: the fc layer behind conv3, whose input then has the two segments): k_fwd_glds_z_os<64, 64, 2, 2>, the unsplit
 * 64 x 64 form of k_fwd_glds_z with the same tile cut, at any n; out_sample_stride is then the row pitch of the first segment
 * (Cout for one dense output, with out2 = out + keep_n * Cout).  sf_conv_kernel_name op 7 names it. */
int sf_conv_fwd_os2_supported(int op, int64_t n, int64_t keep_n, const sf_conv_desc *desc, int64_t in_sample_stride,
                              int64_t out_sample_stride);
int sf_conv_fwd_relu_mask_os2(const void *in, int64_t in_sample_stride, const int32_t *index, int64_t offset,
                              const float *w, const float *bias, float *out, int64_t out_sample_stride,
                              uint32_t *relu_mask, int64_t mask_sample_stride, float *out2, int64_t keep_n, int64_t n,
                              const sf_conv_desc *h_desc, void *stream);
int sf_conv_fwd_t_os2(const float *in, int64_t in_sample_stride, const float *in2, const float *wt, const float *bias,
                      float *out, int64_t out_sample_stride, float *out2, int64_t keep_n, int64_t n,
                      const sf_conv_desc *desc, void *stream);

/* Profiling aid (no reference counterpart): the kernel instantiation a conv/linear launch resolves to, spelled as
 * rocprofv3 prints it ("k_conv_fwd<128, 64, 2, 2, 0>").  op: 0 forward, 1 wgrad, 2 dgrad, 3 sf_conv_fwd_t,
 * 4 sf_conv_fwd_norm, 5 sf_conv_wgrad_norm, 6 sf_conv_fwd_relu_mask_os, 7 sf_conv_fwd_t_os
 * (also the names of the two-segment entry points _os2; for a linear layer op 7 names k_fwd_glds_z_os). */
int sf_conv_kernel_name(int op, int64_t n, const sf_conv_desc *desc, int split_k_allowed, char *out, int cap);
/* dense layer: out[M,N] = act(in[M,K] * w[K,N] + bias); wgrad: dw[K,N] = in^T dout, db = colsum(dout);
 * dgrad: din[M,K] = (dout[M,N] * w^T) * relu_mask(in_act). */
int sf_linear_fwd(const float *in, const float *w, const float *bias, float *out, int64_t M, int K, int N, int relu,
                  void *stream);
int64_t sf_linear_wgrad_workspace(int64_t M, int K, int N);
int sf_linear_wgrad(const float *in, const float *dout, float *dw, float *db, int64_t M, int K, int N,
                    void *workspace, void *stream);
int sf_linear_dgrad(const float *dout, const float *w, const float *in_act, float *din, int64_t M, int K, int N,
                    void *stream);
/* elementwise helper for the backward chain: g[i] = (act[i] > 0) ? g[i] : 0 */
int sf_relu_mask(float *g, const float *act, int64_t n, void *stream);

/* ---- resnet_impala encoder (model/encoder.py:153-221: ResnetEncoder, three stages of conv3x3 -> MaxPool2d(3, 2, 1) ->
 * two ResBlocks x + conv3x3(act(conv3x3(act(x)))), then act, flatten and encoder_conv_mlp_layers; encoder.py:186-213 is the
 * residual block, whose activations are NOT in place: the skip carries the un-activated x).  3x3 convs with stride 1 and
 * padding 1, NHWC activations, weights K-major [9*Cin, Cout], k = (kh*3 + kw)*Cin + c.  The fully connected layers after
 * the last stage are sf_conv_fwd / sf_conv_wgrad / sf_conv_dgrad as 1x1 layers. */
typedef struct {
    int32_t Cin, H, W, Cout; /* input = output feature map (same padding); Cout 16 or 32, Cin <= 32 (16 or 32 for dgrad) */
    int32_t in_u8;           /* 1: the raw u8 NCHW frames, (x - sub_mean) * inv_scale on load (utils/normalize.py:51-70);
                                0: f32 NHWC [n, H, W, Cin], dense */
    int32_t act_in;          /* activation applied to the input on load, 0 none 1 ReLU 2 tanh 3 ELU (model_utils.py:27-35);
                                sf_res_conv_dgrad: the activation whose derivative at `pre` multiplies the data gradient */
    int32_t traj_T;          /* u8 frames only: slab addressing as sf_conv_desc.traj_T */
    float sub_mean, inv_scale;
} sf_res_desc;

/* Conv2d(Cin, Cout, 3, stride=1, padding=1) forward (encoder.py:162-164 and the two convs of encoder.py:193-197):
 * out[n,H,W,Cout] = [residual +] (conv(act_in(in)) + bias); out_act (optional) = act_out(out), the activated copy the
 * next consumer reads (encoder.py:170: the activation after the last stage).  The zero padding is in the normalised,
 * activated domain, as torch pads the normalised f32 tensor.  Sample i is input row index[i] | offset + i (u8 frames:
 * slab row through traj_T) times in_sample_stride elements.  w, out, out_act, residual 16-byte aligned. */
int sf_res_conv_fwd(const void *in, int64_t in_sample_stride, const int32_t *index, int64_t offset, const float *w,
                    const float *bias, const float *residual, float *out, float *out_act, int act_out, int64_t n,
                    const sf_res_desc *h_desc, void *stream);
/* The raw-frame first layer (in_u8 = 1) WITH the observation normaliser applied in the loader (cfg.normalize_input=True):
 * every in-image pixel becomes clamp(((float(u8) - sub_mean) * inv_scale - mu[d]) * rstd[d], +-5), d = its offset inside
 * the NCHW frame, mu / rstd = the f32 tables [Cin*H*W] sf_obsnorm_update maintains (4-byte aligned); the zero padding
 * stays zero, as torch pads the normalised tensor.  No residual, no activated copy; everything else as
 * sf_res_conv_fwd.  Replaces sf_obsnorm_apply + sf_res_conv_fwd on the f32 NHWC batch. */
int sf_res_conv_fwd_norm(const void *in, int64_t in_sample_stride, const int32_t *index, int64_t offset, const float *mu,
                         const float *rstd, const float *w, const float *bias, float *out, int64_t n,
                         const sf_res_desc *h_desc, void *stream);
/* MaxPool2d(3, stride=2, padding=1) (encoder.py:165) on f32 NHWC [n,H,W,C] -> [n,(H-1)/2+1,(W-1)/2+1,C] plus the window
 * position kh*3 + kw of every maximum (u8); -inf padding, torch's tie rule (first maximum in scan order, NaN wins). */
int sf_res_pool_fwd(const float *in, float *out, uint8_t *argmax, int64_t n, int H, int W, int C, void *stream);
/* its backward: every input element gathers dout from the windows whose recorded maximum it is (deterministic). */
int sf_res_pool_bwd(const float *dout, const uint8_t *argmax, float *din, int64_t n, int H, int W, int C, void *stream);
/* data gradient of the 3x3 conv: din = [g_add +] conv_transpose(dout, w) * act_in'(pre) (pre: the layer's stored
 * PRE-activation input, NULL when act_in = 0); g_add lets a residual block finish g_x = g_y + dgrad * act'(x) in one
 * pass.  f32 layers, Cin and Cout 16 or 32. */
int sf_res_conv_dgrad(const float *dout, const float *w, const float *pre, const float *g_add, float *din, int64_t n,
                      const sf_res_desc *h_desc, void *stream);
/* weight / bias gradient of the 3x3 conv: dw[9*Cin, Cout] = patches(act_in(in))^T dout, db = sum dout (overwritten);
 * same input addressing as sf_res_conv_fwd; deterministic two-stage reduction (no float atomics) through a workspace of
 * sf_res_conv_wgrad_workspace(...) bytes. */
int64_t sf_res_conv_wgrad_workspace(int64_t n, const sf_res_desc *h_desc);
int sf_res_conv_wgrad(const void *in, int64_t in_sample_stride, const int32_t *index, int64_t offset, const float *dout,
                      float *dw, float *db, int64_t n, const sf_res_desc *h_desc, void *workspace,
                      int64_t workspace_bytes, void *stream);
/* ... of the raw-frame first layer against the input sf_res_conv_fwd_norm forms (same tables, same workspace size). */
int sf_res_conv_wgrad_norm(const void *in, int64_t in_sample_stride, const int32_t *index, int64_t offset, const float *mu,
                           const float *rstd, const float *dout, float *dw, float *db, int64_t n,
                           const sf_res_desc *h_desc, void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SF_HIP_H */
