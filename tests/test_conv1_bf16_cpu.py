"""--encoder_conv1_bf16 without a GPU: the flag, the four names, and the host-side refusals of the entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from sample_factory_amd import lib
from sample_factory_amd.cfg.arguments import default_cfg, parse_full_cfg, parse_sf_args, verify_cfg
from tests.test_conv_bf16_cpu import _info

NAMES = ["sf_conv1_bf16_supported", "sf_conv1_fwd_bf16", "sf_conv1_wgrad_bf16_workspace", "sf_conv1_wgrad_bf16"]


def test_flag_parses_and_defaults_to_false():
    argv = ["--env=x"]
    parser, _ = parse_sf_args(argv)
    assert parse_full_cfg(parser, argv).encoder_conv1_bf16 is False
    assert parse_full_cfg(parser, argv + ["--encoder_conv1_bf16=True"]).encoder_conv1_bf16 is True


def test_verify_cfg_accepts_convnet_impala_and_refuses_resnet_and_vectors():
    cfg = default_cfg(env="x", use_rnn=False, encoder_conv_architecture="convnet_impala", encoder_conv1_bf16=True)
    assert verify_cfg(cfg, _info((4, 84, 84), np.uint8))
    with pytest.raises(ValueError, match="encoder_conv1_bf16.*resnet_impala"):
        verify_cfg(default_cfg(env="x", encoder_conv_architecture="resnet_impala", encoder_conv1_bf16=True),
                   _info((4, 84, 84), np.uint8))
    with pytest.raises(ValueError, match="encoder_conv1_bf16.*MLP"):
        verify_cfg(default_cfg(env="x", encoder_conv1_bf16=True), _info((24,), np.float32))


def test_names_are_declared_and_listed():
    header = open(os.path.join(os.path.dirname(lib.__file__), "..", "include", "sf_hip.h")).read()
    for name in NAMES:
        assert name in lib.SYMBOLS and re.search(r"\b%s\(" % name, header), name


@pytest.mark.parametrize("over", [dict(in_u8=0), dict(KH=4, KW=4, stride=2, OH=17, OW=17), dict(Cout=64), dict(Cin=17),
                                  dict(OH=9), dict(W=70000, OW=17499)])
def test_entry_points_refuse_unserved_descriptors_before_looking_at_a_pointer(over):
    f = dict(Cin=4, H=36, W=36, Cout=32, KH=8, KW=8, stride=4, OH=8, OW=8, in_u8=1, relu=1, traj_T=0, sub_mean=0.0, inv_scale=1.0)
    f.update(over)
    d = lib.sf_conv_desc(**f)
    L, null, n = lib.load(), C.c_void_p(0), C.c_int64(2)
    assert L.sf_conv1_bf16_supported(0, n, C.byref(d)) == 0 and L.sf_conv1_bf16_supported(1, n, C.byref(d)) == 0
    assert L.sf_conv1_wgrad_bf16_workspace(n, C.byref(d)) == 0
    assert L.sf_conv1_fwd_bf16(null, n, null, n, null, null, null, null, null, n, C.byref(d), null) == -3
    assert L.sf_conv1_wgrad_bf16(null, n, null, n, null, null, null, null, null, n, C.byref(d), null, C.c_int64(0), null) == -3
    assert (b"image too wide" if "W" in over else b"raw-frame bf16 family") in L.sf_last_error()
