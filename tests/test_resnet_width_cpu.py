"""--encoder_resnet_width: parsing, config.json round trip, refusals, and the torch twin's parameter shapes."""
import json
import os

import numpy as np
import pytest

from sample_factory_amd.cfg.arguments import (cfg_dict, default_cfg, load_from_checkpoint, parse_full_cfg, parse_sf_args,
                                              verify_cfg)


def test_flag_parses_defaults_to_one_and_survives_config_json(tmp_path):
    argv = ["--env=x", f"--train_dir={tmp_path}", "--experiment=w", "--encoder_conv_architecture=resnet_impala"]
    parser, _ = parse_sf_args(argv)
    assert parse_full_cfg(parser, argv).encoder_resnet_width == 1
    cfg = parse_full_cfg(parser, argv + ["--encoder_resnet_width=4"])
    assert cfg.encoder_resnet_width == 4
    os.makedirs(tmp_path / "w")
    with open(tmp_path / "w" / "config.json", "w") as f:  # what Runner._save_cfg writes: the JSON-able flags
        json.dump({k: v for k, v in cfg_dict(cfg).items() if isinstance(v, (int, float, str, bool, list, type(None)))}, f)
    argv = ["--env=x", f"--train_dir={tmp_path}", "--experiment=w"]  # enjoy: the flag is not given again
    parser, _ = parse_sf_args(argv, evaluation=True)
    assert load_from_checkpoint(parse_full_cfg(parser, argv)).encoder_resnet_width == 4


@pytest.mark.parametrize("kw,match", [
    (dict(encoder_conv_architecture="resnet_impala", encoder_resnet_width=3), "encoder_resnet_width"),
    (dict(encoder_conv_architecture="resnet_impala", encoder_resnet_width=0), "encoder_resnet_width"),
    (dict(encoder_conv_architecture="convnet_simple", encoder_resnet_width=2),
     "encoder_resnet_width.*encoder_conv_architecture"),
])
def test_verify_cfg_refuses(kw, match):
    from sample_factory_amd.algo.utils.env_info import EnvInfo
    from sample_factory_amd.envs import spaces
    info = EnvInfo(spaces.Dict({"obs": spaces.Box(0, 255, (3, 16, 16), np.uint8)}), spaces.Discrete(3), 1)
    with pytest.raises(ValueError, match=match):
        verify_cfg(default_cfg(env="x", **kw), info)


@pytest.mark.parametrize("k", [1, 2, 4])
def test_torch_twin_parameter_shapes_scale_with_the_width(k):
    from sample_factory_amd.envs import spaces
    from sample_factory_amd.model.encoder import ResnetEncoder
    cfg = default_cfg(env="x", encoder_conv_architecture="resnet_impala", encoder_resnet_width=k,
                      encoder_conv_mlp_layers=[64])
    enc = ResnetEncoder(cfg, spaces.Box(0, 255, (3, 16, 16), np.uint8))
    shapes = {n: tuple(p.shape) for n, p in enc.named_parameters()}
    cin, i = 3, 0
    for c in (16 * k, 32 * k, 32 * k):
        assert shapes[f"conv_head.{i}.weight"] == (c, cin, 3, 3) and shapes[f"conv_head.{i}.bias"] == (c,)
        for b in (i + 2, i + 3):
            for j in (1, 3):
                assert shapes[f"conv_head.{b}.res_block_core.{j}.weight"] == (c, c, 3, 3)
        cin, i = c, i + 4
    assert shapes["mlp_layers.0.weight"] == (64, 32 * k * 2 * 2) and len(shapes) == 2 * 15 + 2
