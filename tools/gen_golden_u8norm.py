"""Generate the u8-frame normalize_input fixture by RUNNING THE REFERENCE (ConvEncoder, sample_factory/model/encoder.py:90-150,
inside ActorCriticSharedWeights, with the observation normaliser of utils/normalize.py:24-70 in front of it):

 * tests/golden/train_u8norm.npz: a Learner.train replay, 16 x 8 on 3x36x52 u8 frames (three channels, not square),
   convnet_simple, normalize_input=True, 2 minibatches, invalid rows, float64 first-step anchors.

The replay frames take 8 levels in [0, 255] so that the compressed fixture stays small.  Build machine only (the reference
is not present where the GPU tests run); the fixture is committed.  Uses the helpers of oracle.gen_golden without changing
them.  Usage:  python tools/gen_golden_u8norm.py
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle.gen_golden as gg  # noqa: E402
from oracle.gen_golden import gen_train, gym  # noqa: E402

TRAIN_OBS = (3, 36, 52)
TRAIN_ARGS = ["--encoder_conv_architecture=convnet_simple", "--nonlinearity=elu", "--obs_scale=255.0",
              "--encoder_conv_mlp_layers", "64", "--normalize_input=True"]
LEVELS = 8


def _quantised_fill(fill):
    """oracle.gen_golden.fill_batch, with u8 image observations drawn from LEVELS values in [0, 255]"""
    def f(b, g, *a, **k):
        fill(b, g, *a, **k)
        for v in b["obs"].values():
            if v.dtype == torch.uint8 and v.dim() == 5:
                v.copy_((torch.randint(0, LEVELS, v.shape, generator=g) * (255 // (LEVELS - 1))).to(torch.uint8))
    return f


def main():
    gg.fill_batch = _quantised_fill(gg.fill_batch)
    obs = gym.spaces.Dict({"obs": gym.spaces.Box(0, 255, TRAIN_OBS, np.uint8)})
    gen_train("u8norm", obs, TRAIN_ARGS, E=16, T=8, A=6, nb=2, epochs=1, subsample=37, p_other_policy=0.1,
              fp64_first_step=True, extra=["--exploration_loss_coeff=0.01"])


if __name__ == "__main__":
    main()
