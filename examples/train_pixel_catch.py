"""PixelCatch: a learnable pixel task that needs no emulator — the game runs and renders on the MI355X, the policy is the
conv encoder, and the catch rate rises within seconds.  Touches only the `sample_factory.*` surface a user programs against
(env registration, argument parsing, run_rl), like examples/train_gym_env.py.

  python examples/train_pixel_catch.py --env=pixel_catch --experiment=pixel_catch --train_for_env_steps=2000000

`pixel_catch` is the device env (sample_factory_amd/envs/pixel_catch.py: one HIP launch per step renders the next observation
into the trajectory slab); `pixel_catch_host` is the same game in NumPy on the host, bit for bit — with
`--pixel_catch_frames=1 --device_framestack=4` it sends one frame per step and the stack is kept on the device.  A reward of
+1 is a catch, -1 a miss: an episode of `--pixel_catch_balls` balls returns between -balls and +balls.

  python -m sample_factory_amd.enjoy  does not know the env: evaluate with
  python examples/train_pixel_catch.py --enjoy --env=pixel_catch --experiment=pixel_catch --max_num_episodes=256

Levels: `--pixel_catch_decoys=6 --pixel_catch_levels=8` trains on the 8 levels [0, 8), each with 6 static decoy balls; the
flags are saved with the experiment, and `--enjoy ... --pixel_catch_start_level=1000000 --pixel_catch_levels=100000` plays the
checkpoint on levels it has never seen.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from sample_factory.cfg.arguments import parse_full_cfg, parse_sf_args  # noqa: E402
from sample_factory.envs.env_utils import register_env  # noqa: E402
from sample_factory.envs.pixel_catch import (add_pixel_catch_args, make_pixel_catch_env,  # noqa: E402
                                             make_pixel_catch_host_env)
from sample_factory.train import run_rl  # noqa: E402

# what tests/test_gpu_pixel_catch_e2e.py trains with (36 x 36 there); any of it can be overridden on the command line
DEFAULTS = dict(use_rnn=False, nonlinearity="relu", normalize_input=False, obs_scale=255.0,
                encoder_conv_architecture="convnet_simple", encoder_conv_mlp_layers=[64], rollout=8, batch_size=2048,
                num_batches_per_epoch=4, num_epochs=1, learning_rate=5e-4, num_workers=1, num_envs_per_worker=1,
                worker_num_splits=1, async_rl=False, serial_mode=True, env_gpu_observations=False, env_gpu_actions=False)


def register_custom_components() -> None:
    register_env("pixel_catch", make_pixel_catch_env)
    register_env("pixel_catch_host", make_pixel_catch_host_env)


def parse_custom_args(argv=None, evaluation: bool = False):
    parser, _partial = parse_sf_args(argv=argv, evaluation=evaluation)
    add_pixel_catch_args(parser)
    parser.set_defaults(**DEFAULTS)
    return parse_full_cfg(parser, argv)


if __name__ == "__main__":
    register_custom_components()
    argv = [a for a in sys.argv[1:] if a != "--enjoy"]
    if "--enjoy" in sys.argv[1:]:
        from sample_factory.enjoy import enjoy
        status, avg = enjoy(parse_custom_args(argv, evaluation=True))
        print(f"Avg episode reward: {avg:.3f}")
        sys.exit(status)
    sys.exit(run_rl(parse_custom_args(argv)))
