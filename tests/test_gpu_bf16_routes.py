"""Which lib wrappers a convnet_atari tower calls, in order, under each combination of the bf16 flags: one rollout forward, one
training forward and one backward on u8 (4, 36, 36) frames with one fully connected encoder layer, the smallest geometry all
three families serve.  The lists in CALLS were recorded with _passes() below on the commit BEFORE _Layer.route existed (the
flags were then dispatched on L.kind at every call site), on an MI355X; they are not derived from the routing code.  The raw
recording is tests/golden/bf16_routes_parent_calls.json; the lists written out here must equal it name for name."""
import inspect
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from sample_factory_amd import lib  # noqa: E402
from tests.test_gpu_resnet import _cfg, _space  # noqa: E402

N, A, SHAPE = 6, 5, (4, 36, 36)
CONV1, CONV, MLP = "encoder_conv1_bf16", "encoder_conv_bf16", "mlp_bf16"
SETTINGS = {"none": (), "conv1": (CONV1,), "conv": (CONV,), "mlp": (MLP,), "all": (CONV1, CONV, MLP)}
# the runs of names that recur in the recorded lists: one layer's forward on the fp32 dispatch (layer 0 has no transposed
# weights to ask conv_fwd_t about; the heads take conv_fwd_t), one layer's backward per family (layer 0 has no data gradient)
F32_0 = ["conv_fwd_workspace", "conv_fwd_raw"]
F32 = ["conv_fwd_t_supported"] + F32_0
HEADS = ["conv_fwd_t_supported", "conv_fwd_t_workspace", "conv_fwd_t"]
MASK = ["conv_relu_mask_supported"]  # asked by the training forward of an fp32 layer 0 (declined at this geometry)
BWD = ["conv_wgrad_workspace", "conv_wgrad_raw", "conv_dgrad"]
BWD_CONV1 = ["conv1_wgrad_bf16_workspace", "conv1_wgrad_bf16"]
BWD_CONV = ["conv_wgrad_bf16_workspace", "conv_wgrad_bf16", "conv_dgrad_bf16"]
BWD_MLP = ["linear_wgrad_bf16_workspace", "linear_wgrad_bf16", "linear_dgrad_bf16"]
# setting -> ("inf" forward, "train" forward, backward): layers conv1, conv2, conv3, fc, heads forward; heads .. conv1 backward
CALLS = {
    "none": (F32_0 + 3 * F32 + HEADS, MASK + F32_0 + 3 * F32 + HEADS, 4 * BWD + BWD[:2]),
    "conv1": (["conv1_fwd_bf16"] + 3 * F32 + HEADS, ["conv1_fwd_bf16"] + 3 * F32 + HEADS, 4 * BWD + BWD_CONV1),
    "conv": (F32_0 + 2 * ["conv_fwd_bf16"] + F32 + HEADS, MASK + F32_0 + 2 * ["conv_fwd_bf16"] + F32 + HEADS,
             2 * BWD + 2 * BWD_CONV + BWD[:2]),
    "mlp": (F32_0 + 2 * F32 + ["linear_fwd_bf16"] + HEADS, MASK + F32_0 + 2 * F32 + ["linear_fwd_bf16"] + HEADS,
            BWD + BWD_MLP + 2 * BWD + BWD[:2]),
    "all": (["conv1_fwd_bf16", "conv_fwd_bf16", "conv_fwd_bf16", "linear_fwd_bf16"] + HEADS,
            ["conv1_fwd_bf16", "conv_fwd_bf16", "conv_fwd_bf16", "linear_fwd_bf16"] + HEADS,
            BWD + BWD_MLP + 2 * BWD_CONV + BWD_CONV1),
}


def _passes(flags, setattr_):
    """build the tower, wrap every public function of lib named after a conv or linear op with a recorder (through setattr_),
    run the three passes; returns (model, recorded names, heads of the "inf" forward, heads of the "train" forward)"""
    from sample_factory_amd.envs import spaces
    from sample_factory_amd.model.model_factory import create_actor_critic
    cfg = _cfg("relu", encoder_conv_architecture="convnet_atari", encoder_conv_mlp_layers=[64], **{f: True for f in flags})
    torch.manual_seed(3)
    ac = create_actor_critic(cfg, _space(SHAPE), spaces.Discrete(A), torch.device("cuda"))
    g = torch.Generator().manual_seed(11)
    obs = torch.randint(0, 256, (N,) + SHAPE, generator=g, dtype=torch.uint8).cuda()
    gh = torch.randn(N, ac.heads_ld, generator=g).cuda()
    gh[:, 1 + A:] = 0
    calls = []

    def recorder(name, fn):
        def wrapped(*a, **k):
            calls.append(name)
            return fn(*a, **k)
        return wrapped
    for name, fn in inspect.getmembers(lib, inspect.isfunction):
        if not name.startswith("_") and any(s in name for s in ("conv_", "conv1_", "linear_")):
            setattr_(lib, name, recorder(name, fn))
    inf = ac.forward_heads(obs, N, sample_stride=ac.obs_elems, tag="inf")[-1].clone()
    acts = ac.forward_heads(obs, N, sample_stride=ac.obs_elems, tag="train")
    ac.backward(acts, gh, obs, N, sample_stride=ac.obs_elems)
    torch.cuda.synchronize()
    return ac, calls, inf, acts[-1]


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_wrappers_called_in_the_recorded_order(monkeypatch, setting):
    flags = SETTINGS[setting]
    ac, calls, inf, train = _passes(flags, monkeypatch.setattr)
    with open(os.path.join(os.path.dirname(__file__), "golden", "bf16_routes_parent_calls.json")) as f:
        assert sum(CALLS[setting], []) == json.load(f)["calls"][setting]
    assert calls == sum(CALLS[setting], [])
    assert [L.bf16 for L in ac.layers] == [L.route is not None for L in ac.layers]
    assert [L.bf16 for L in ac.layers] == [CONV1 in flags, CONV in flags, CONV in flags, MLP in flags, False]
    assert torch.equal(inf, train)
