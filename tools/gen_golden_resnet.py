"""Generate the resnet_impala fixtures by RUNNING THE REFERENCE (ResnetEncoder, sample_factory/model/encoder.py:153-221,
inside ActorCriticSharedWeights) on seeded weights and frames:

 * tests/golden/model_fwd_resnet.npz: forwards on u8 and f32 observations, with samples of the first conv's
   pre-activation and of the first pool's output;
 * tests/golden/train_resnet{,_norm,_gru}.npz: Learner.train replays (16 x 8 on 4x36x36, 2 minibatches, invalid rows,
   float64 first-step anchors), plain / normalize_input=True / GRU core.

Build machine only (the reference is not present where the GPU tests run); the fixture is committed.  Uses the helpers of
oracle.gen_golden without changing them.  Usage:  python tools/gen_golden_resnet.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.gen_golden import gen_train, gym, load_seeded, make_cfg, make_learner, save  # noqa: E402

CASES = (  # (tag, obs shape, nonlinearity, samples, f32 observations)
    ("elu84", (4, 84, 84), "elu", 3, False),
    ("relu84", (4, 84, 84), "relu", 3, False),
    ("odd", (3, 13, 17), "tanh", 5, False),  # odd H and W: padding and pool edges on both parities
    ("f32", (3, 13, 17), "elu", 4, True),    # f32 frames (the torch path; the native tower takes u8 frames)
)
TRAIN_ARGS = ["--encoder_conv_architecture=resnet_impala", "--nonlinearity=elu", "--obs_scale=255.0",
              "--encoder_conv_mlp_layers", "64"]


def main():
    out = {}
    for ci, (tag, shape, act, n, f32) in enumerate(CASES):
        obs_space = gym.spaces.Dict({"obs": gym.spaces.Box(0, 255, shape, np.float32 if f32 else np.uint8)})
        cfg = make_cfg(["--encoder_conv_architecture=resnet_impala", f"--nonlinearity={act}", "--obs_scale=255.0",
                        "--obs_subtract_mean=0.0", "--normalize_input=False", "--rollout=4", "--batch_size=8",
                        "--num_batches_per_epoch=1"])
        learner, _ = make_learner(cfg, obs_space, gym.spaces.Discrete(6), 2)
        seed = 21 + ci
        shapes = load_seeded(learner.actor_critic, seed=seed)
        g = torch.Generator().manual_seed(90 + ci)
        obs = torch.randint(0, 256, (n,) + shape, generator=g, dtype=torch.uint8)
        if f32:
            obs = obs.float() + torch.rand(obs.shape, generator=g)
        ac = learner.actor_critic
        ac.eval()
        with torch.no_grad():
            nobs = ac.normalize_obs({"obs": obs})
            head = ac.forward_head(nobs)
            res = ac.forward_tail(head, values_only=False, sample_actions=False)
            conv_head = ac.encoder.encoders["obs"].conv_head
            conv0 = conv_head[0](nobs["obs"])
            pool0 = conv_head[1](conv0)
        out.update({f"{tag}_obs": obs.numpy(), f"{tag}_param_seed": seed, f"{tag}_nonlinearity": act,
                    f"{tag}_head_sample": head[:, ::7].numpy(), f"{tag}_action_logits": res["action_logits"].numpy(),
                    f"{tag}_values": res["values"].numpy(), f"{tag}_conv0_preact_sample": conv0[:, :, ::3, ::3].numpy(),
                    f"{tag}_pool0_sample": pool0[:, :, ::2, ::2].numpy(),
                    f"{tag}_param_names": np.array([k for k, _ in shapes]),
                    f"{tag}_param_shapes": np.array([str(s) for _, s in shapes]),
                    f"{tag}_f32": f32, f"{tag}_num_params": sum(int(np.prod(s)) for _, s in shapes)})
    save("model_fwd_resnet", ref="model/encoder.py:153-221 ResnetEncoder inside ActorCriticSharedWeights (obs_scale=255)",
         cases=np.array([c[0] for c in CASES]), **out)
    obs = gym.spaces.Dict({"obs": gym.spaces.Box(0, 255, (4, 36, 36), np.uint8)})
    common = dict(E=16, T=8, A=6, nb=2, epochs=1, subsample=37, p_other_policy=0.1, fp64_first_step=True,
                  extra=["--exploration_loss_coeff=0.01"])
    gen_train("resnet", obs, TRAIN_ARGS + ["--normalize_input=False"], obs_seed=3601, **common)
    gen_train("resnet_norm", obs, TRAIN_ARGS + ["--normalize_input=True"], obs_seed=3602, **common)
    gen_train("resnet_gru", obs, TRAIN_ARGS + ["--normalize_input=False", "--use_rnn=True", "--rnn_type=gru",
                                              "--rnn_size=32", "--recurrence=8"], obs_seed=3603, use_rnn=True, **common)


if __name__ == "__main__":
    main()
