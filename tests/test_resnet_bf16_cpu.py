"""--encoder_resnet_bf16: parsing and default, and the refusal with another architecture."""
import numpy as np
import pytest

from sample_factory_amd.cfg.arguments import default_cfg, parse_full_cfg, parse_sf_args, verify_cfg


def test_flag_parses_and_defaults_to_false():
    argv = ["--env=x", "--encoder_conv_architecture=resnet_impala"]
    parser, _ = parse_sf_args(argv)
    assert parse_full_cfg(parser, argv).encoder_resnet_bf16 is False
    assert parse_full_cfg(parser, argv + ["--encoder_resnet_bf16=True"]).encoder_resnet_bf16 is True


def test_verify_cfg_refuses_the_flag_with_another_architecture():
    from sample_factory_amd.algo.utils.env_info import EnvInfo
    from sample_factory_amd.cfg.arguments import resnet_bf16
    from sample_factory_amd.envs import spaces
    info = EnvInfo(spaces.Dict({"obs": spaces.Box(0, 255, (3, 16, 16), np.uint8)}), spaces.Discrete(3), 1)
    assert resnet_bf16(default_cfg(env="x", encoder_conv_architecture="resnet_impala", encoder_resnet_bf16=True))
    with pytest.raises(ValueError, match="encoder_resnet_bf16.*encoder_conv_architecture"):
        verify_cfg(default_cfg(env="x", encoder_conv_architecture="convnet_simple", encoder_resnet_bf16=True), info)
