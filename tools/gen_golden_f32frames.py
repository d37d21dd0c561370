"""Generate the float32-frame fixtures by RUNNING THE REFERENCE (ConvEncoder, sample_factory/model/encoder.py:90-150, inside
ActorCriticSharedWeights) on seeded weights and float32 CHW observations (the frames a user env emits after scaling its
pixels itself, e.g. Box(0, 1, (C, H, W), np.float32)):

 * tests/golden/model_fwd_f32frames.npz: forwards of convnet_simple / convnet_impala / convnet_atari on C in {1, 3, 4},
   one odd H x W (the scalar loader) and non-trivial obs_subtract_mean / obs_scale;
 * tests/golden/train_f32frames{,_norm,_gru}.npz: Learner.train replays (16 x 8 on 3x36x36 f32 frames, 2 minibatches,
   invalid rows, float64 first-step anchors), plain / normalize_input=True / GRU core.

The replay frames take 16 levels in [0, 1] so that the compressed fixtures stay small.  Build machine only (the reference
is not present where the GPU tests run); the fixtures are committed.  Uses the helpers of oracle.gen_golden without
changing them.  Usage:  python tools/gen_golden_f32frames.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle.gen_golden as gg  # noqa: E402
from oracle.gen_golden import gen_train, gym, load_seeded, make_cfg, make_learner, save  # noqa: E402

CASES = (  # (tag, obs shape, architecture, nonlinearity, samples, obs_subtract_mean, obs_scale)
    ("simple4", (4, 84, 84), "convnet_simple", "relu", 3, 0.0, 1.0),
    ("impala3", (3, 64, 64), "convnet_impala", "elu", 4, 0.5, 2.0),
    ("atari1", (1, 84, 84), "convnet_atari", "tanh", 3, 0.0, 1.0),
    ("odd3", (3, 45, 53), "convnet_atari", "relu", 5, 0.25, 0.5),  # odd H and W: the scalar loader
)
TRAIN_OBS = (3, 36, 36)
TRAIN_ARGS = ["--encoder_conv_architecture=convnet_simple", "--nonlinearity=elu", "--encoder_conv_mlp_layers", "64"]


def _quantised_fill(fill):
    """oracle.gen_golden.fill_batch, with f32 image observations drawn from 16 levels in [0, 1]"""
    def f(b, g, *a, **k):
        fill(b, g, *a, **k)
        for v in b["obs"].values():
            if v.dtype == torch.float32 and v.dim() == 5:
                v.copy_(torch.randint(0, 16, v.shape, generator=g).float() / 15.0)
    return f


def main():
    out = {}
    for ci, (tag, shape, arch, act, n, mean, scale) in enumerate(CASES):
        obs_space = gym.spaces.Dict({"obs": gym.spaces.Box(0, 1, shape, np.float32)})
        cfg = make_cfg([f"--encoder_conv_architecture={arch}", f"--nonlinearity={act}", f"--obs_scale={scale}",
                        f"--obs_subtract_mean={mean}", "--normalize_input=False", "--rollout=4", "--batch_size=8",
                        "--num_batches_per_epoch=1"])
        learner, _ = make_learner(cfg, obs_space, gym.spaces.Discrete(6), 2)
        seed = 41 + ci
        shapes = load_seeded(learner.actor_critic, seed=seed)
        g = torch.Generator().manual_seed(140 + ci)
        obs = torch.randint(0, 16, (n,) + shape, generator=g).float() / 15.0  # 16 levels: a small fixture
        ac = learner.actor_critic
        ac.eval()
        with torch.no_grad():
            nobs = ac.normalize_obs({"obs": obs})
            head = ac.forward_head(nobs)
            res = ac.forward_tail(head, values_only=False, sample_actions=False)
            conv0 = ac.encoder.encoders["obs"].enc.conv_head[0](nobs["obs"])
        out.update({f"{tag}_obs": obs.numpy(), f"{tag}_param_seed": seed, f"{tag}_nonlinearity": act, f"{tag}_arch": arch,
                    f"{tag}_sub_mean": mean, f"{tag}_scale": scale, f"{tag}_head_sample": head[:, ::7].numpy(),
                    f"{tag}_action_logits": res["action_logits"].numpy(), f"{tag}_values": res["values"].numpy(),
                    f"{tag}_conv0_preact_sample": conv0[:, :, ::2, ::2].numpy(),
                    f"{tag}_param_names": np.array([k for k, _ in shapes]),
                    f"{tag}_param_shapes": np.array([str(s) for _, s in shapes]),
                    f"{tag}_num_params": sum(int(np.prod(s)) for _, s in shapes)})
    save("model_fwd_f32frames", ref="model/encoder.py:90-150 ConvEncoder inside ActorCriticSharedWeights on float32 frames",
         cases=np.array([c[0] for c in CASES]), **out)
    gg.fill_batch = _quantised_fill(gg.fill_batch)
    obs = gym.spaces.Dict({"obs": gym.spaces.Box(0, 1, TRAIN_OBS, np.float32)})
    common = dict(E=16, T=8, A=6, nb=2, epochs=1, subsample=37, p_other_policy=0.1, fp64_first_step=True,
                  extra=["--exploration_loss_coeff=0.01"])
    gen_train("f32frames", obs, TRAIN_ARGS + ["--normalize_input=False"], **common)
    gen_train("f32frames_norm", obs, TRAIN_ARGS + ["--normalize_input=True"], **common)
    gen_train("f32frames_gru", obs, TRAIN_ARGS + ["--normalize_input=False", "--use_rnn=True", "--rnn_type=gru",
                                                 "--rnn_size=32", "--recurrence=8"], use_rnn=True, **common)


if __name__ == "__main__":
    main()
