"""--encoder_conv_bf16: parsing and default, the architectures it takes and the ones it refuses."""
import numpy as np
import pytest

from sample_factory_amd.cfg.arguments import default_cfg, parse_full_cfg, parse_sf_args, verify_cfg


def _info(shape, dtype):
    from sample_factory_amd.algo.utils.env_info import EnvInfo
    from sample_factory_amd.envs import spaces
    return EnvInfo(spaces.Dict({"obs": spaces.Box(0, 255, shape, dtype)}), spaces.Discrete(3), 1)


def test_flag_parses_and_defaults_to_false():
    argv = ["--env=x"]
    parser, _ = parse_sf_args(argv)
    assert parse_full_cfg(parser, argv).encoder_conv_bf16 is False
    assert parse_full_cfg(parser, argv + ["--encoder_conv_bf16=True"]).encoder_conv_bf16 is True


@pytest.mark.parametrize("arch", ["convnet_simple", "convnet_atari"])
def test_verify_cfg_accepts_the_flag(arch):
    cfg = default_cfg(env="x", use_rnn=False, encoder_conv_architecture=arch, encoder_conv_bf16=True)
    assert verify_cfg(cfg, _info((4, 84, 84), np.uint8))


@pytest.mark.parametrize("arch,shape,named", [("convnet_impala", (4, 84, 84), "convnet_impala"),
                                              ("resnet_impala", (4, 84, 84), "resnet_impala"), ("convnet_simple", (24,), "MLP")])
def test_verify_cfg_refuses_the_flag(arch, shape, named):
    cfg = default_cfg(env="x", encoder_conv_architecture=arch, encoder_conv_bf16=True)
    with pytest.raises(ValueError, match="encoder_conv_bf16.*" + named):
        verify_cfg(cfg, _info(shape, np.uint8 if len(shape) == 3 else np.float32))
