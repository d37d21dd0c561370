"""--mlp_bf16 without a GPU: the flag, the five names, and the host-side refusals of the entry points."""
import ctypes as C
import os
import re

import pytest

from sample_factory_amd import lib
from sample_factory_amd.cfg.arguments import default_cfg, parse_full_cfg, parse_sf_args, verify_cfg

NAMES = ["sf_linear_bf16_supported", "sf_linear_fwd_bf16", "sf_linear_dgrad_bf16", "sf_linear_wgrad_bf16_workspace",
         "sf_linear_wgrad_bf16"]


def test_flag_parses_and_defaults_to_false():
    argv = ["--env=x"]
    parser, _ = parse_sf_args(argv)
    assert parse_full_cfg(parser, argv).mlp_bf16 is False
    assert parse_full_cfg(parser, argv + ["--mlp_bf16=True"]).mlp_bf16 is True


def test_verify_cfg_refuses_the_flag_with_resnet_impala():
    from tests.test_conv_bf16_cpu import _info
    import numpy as np
    assert verify_cfg(default_cfg(env="x", use_rnn=False, mlp_bf16=True), _info((24,), np.float32))
    with pytest.raises(ValueError, match="mlp_bf16.*resnet_impala"):
        verify_cfg(default_cfg(env="x", encoder_conv_architecture="resnet_impala", mlp_bf16=True), _info((4, 84, 84), np.uint8))


def test_names_are_declared_and_listed():
    header = open(os.path.join(os.path.dirname(lib.__file__), "..", "include", "sf_hip.h")).read()
    for name in NAMES:
        assert name in lib.SYMBOLS and re.search(r"\b%s\(" % name, header), name


@pytest.mark.parametrize("n,K,N", [(2, 12, 64), (2, 64, 12), (2, 4, 8), (0, 64, 64)])
def test_entry_points_refuse_unserved_shapes_before_looking_at_a_pointer(n, K, N):
    L, null, n = lib.load(), C.c_void_p(0), C.c_int64(n)
    assert all(L.sf_linear_bf16_supported(op, n, K, N) == 0 for op in (0, 1, 2))
    assert L.sf_linear_wgrad_bf16_workspace(n, K, N) == 0
    assert L.sf_linear_fwd_bf16(null, null, null, null, n, K, N, 1, null) == -3
    assert L.sf_linear_dgrad_bf16(null, null, null, null, n, K, N, 1, null) == -3
    assert L.sf_linear_wgrad_bf16(null, null, null, null, n, K, N, null, C.c_int64(0), null) == -3
    assert b"K % 8" in L.sf_last_error()
