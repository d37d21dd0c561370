"""Which model `create_actor_critic` builds for every configuration and SF_NATIVE_* switch: the dispatch table, pinned on
stubs of the model classes (the factory imports them inside the function, so a monkeypatched module attribute is what it
builds).  CPU only: `device="cuda"` is just a torch.device here."""
import numpy as np
import pytest

from sample_factory_amd.cfg.arguments import default_cfg
from sample_factory_amd.envs import spaces
from sample_factory_amd.model import actor_critic, actor_critic_multikey, actor_critic_separate, torch_policy
from sample_factory_amd.model.model_factory import create_actor_critic, global_model_factory

AC, SEP, MK, TORCH = "ActorCritic", "SeparateActorCritic", "MultiKeyActorCritic", "TorchPolicyAdapter"

IMG_U8 = spaces.Box(0, 255, (3, 64, 64), np.uint8)
IMG_F32 = spaces.Box(0, 1, (3, 64, 64), np.float32)
IMG_F64 = spaces.Box(0, 1, (3, 64, 64), np.float64)
VEC = spaces.Box(-1, 1, (8,), np.float32)
OBS = {
    "vec": {"obs": VEC},
    "u8": {"obs": IMG_U8},
    "f32": {"obs": IMG_F32},
    "f64": {"obs": IMG_F64},
    "multi": {"obs": IMG_U8, "vec": VEC},
    "multi_f32": {"obs": IMG_F32, "vec": VEC},
}


def _stub(name, raises):
    class Stub:
        def __init__(self, *args, **kwargs):
            if raises:
                raise NotImplementedError(f"{name} stub refuses")
            self.built = name
    return Stub


# (row id, configuration, expected class); configuration keys: obs, sep (separate actor / critic weights), arch, layers
# (rnn_num_layers), device, user ("encoder" | "actor_critic": a registered factory part), env (switches), raises (the stub
# of that class raises NotImplementedError)
ROWS = [
    ("vec_cpu", dict(obs="vec", device="cpu"), AC),  # the single-key candidate is tried regardless of device
    ("vec", dict(obs="vec"), AC),
    ("u8", dict(obs="u8"), AC),
    ("u8_stacked_rnn", dict(obs="u8", layers=2), AC),
    ("f32", dict(obs="f32"), AC),
    ("f32_cpu", dict(obs="f32", device="cpu"), TORCH),
    ("f32_switch_off", dict(obs="f32", env={"SF_NATIVE_F32FRAMES": "0"}), TORCH),
    ("f64", dict(obs="f64"), AC),
    ("multi", dict(obs="multi"), MK),
    ("multi_stacked_rnn", dict(obs="multi", layers=2), MK),
    ("multi_cpu", dict(obs="multi", device="cpu"), TORCH),
    ("multi_switch_off", dict(obs="multi", env={"SF_NATIVE_MULTIKEY": "0"}), TORCH),
    ("multi_f32", dict(obs="multi_f32"), MK),
    ("multi_f32_switch_off", dict(obs="multi_f32", env={"SF_NATIVE_F32FRAMES": "0"}), TORCH),
    ("resnet", dict(obs="u8", arch="resnet_impala"), MK),
    ("resnet_cpu", dict(obs="u8", arch="resnet_impala", device="cpu"), MK),  # tried regardless of device
    ("resnet_stacked_rnn", dict(obs="u8", arch="resnet_impala", layers=2), MK),
    ("resnet_switch_off", dict(obs="u8", arch="resnet_impala", env={"SF_NATIVE_RESNET": "0"}), TORCH),
    ("resnet_f32", dict(obs="f32", arch="resnet_impala"), MK),
    ("resnet_f32_switch_off", dict(obs="f32", arch="resnet_impala", env={"SF_NATIVE_F32FRAMES": "0"}), MK),  # ignored
    ("resnet_f32_cpu", dict(obs="f32", arch="resnet_impala", device="cpu"), MK),
    ("resnet_multi", dict(obs="multi", arch="resnet_impala"), MK),
    ("resnet_multi_switch_off", dict(obs="multi", arch="resnet_impala", env={"SF_NATIVE_MULTIKEY": "0"}), TORCH),
    ("resnet_separate", dict(obs="u8", arch="resnet_impala", sep=True), TORCH),
    ("resnet_vec_only", dict(obs="vec", arch="resnet_impala"), AC),  # no image key: not a resnet model
    ("sep", dict(obs="vec", sep=True), SEP),
    ("sep_u8", dict(obs="u8", sep=True), SEP),
    ("sep_stacked_rnn", dict(obs="u8", sep=True, layers=2), SEP),
    ("sep_cpu", dict(obs="vec", sep=True, device="cpu"), TORCH),
    ("sep_switch_off", dict(obs="vec", sep=True, env={"SF_NATIVE_SEPARATE_WEIGHTS": "0"}), TORCH),
    ("sep_f32", dict(obs="f32", sep=True), SEP),
    ("sep_f32_switch_off", dict(obs="f32", sep=True, env={"SF_NATIVE_F32FRAMES": "0"}), TORCH),
    ("sep_f64", dict(obs="f64", sep=True), SEP),
    ("sep_multi", dict(obs="multi", sep=True), SEP),
    ("sep_multi_switch_off", dict(obs="multi", sep=True, env={"SF_NATIVE_MULTIKEY": "0"}), TORCH),
    ("user_encoder", dict(obs="vec", user="encoder"), TORCH),
    ("user_encoder_multi", dict(obs="multi", user="encoder"), TORCH),
    ("user_actor_critic", dict(obs="u8", user="actor_critic"), TORCH),
    ("user_actor_critic_sep", dict(obs="vec", sep=True, user="actor_critic"), TORCH),
    ("refused_single", dict(obs="f64", raises=AC), TORCH),
    ("refused_multi", dict(obs="multi", raises=MK), TORCH),
    ("refused_resnet", dict(obs="u8", arch="resnet_impala", raises=MK), TORCH),
    ("refused_sep", dict(obs="vec", sep=True, raises=SEP), TORCH),
]


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_create_actor_critic_dispatch(row, monkeypatch):
    _, c, expected = row
    for mod, name in ((actor_critic, AC), (actor_critic_separate, SEP), (actor_critic_multikey, MK)):
        monkeypatch.setattr(mod, name, _stub(name, c.get("raises") == name))

    class Adapter:
        def __init__(self, cfg, obs_space, action_space, device, module, all_reduce=None):
            self.built, self.module = TORCH, module

    monkeypatch.setattr(torch_policy, "TorchPolicyAdapter", Adapter)
    monkeypatch.setattr(torch_policy, "build_torch_actor_critic", lambda *a: "default_torch_module")
    for k in ("SF_NATIVE_RESNET", "SF_NATIVE_MULTIKEY", "SF_NATIVE_SEPARATE_WEIGHTS", "SF_NATIVE_F32FRAMES"):
        monkeypatch.delenv(k, raising=False)
    for k, v in c.get("env", {}).items():
        monkeypatch.setenv(k, v)
    cfg = default_cfg(actor_critic_share_weights=not c.get("sep", False),
                      encoder_conv_architecture=c.get("arch", "convnet_simple"), use_rnn=True, rnn_type="gru",
                      rnn_num_layers=c.get("layers", 1))
    f = global_model_factory()
    if c.get("user") == "encoder":
        f.register_encoder_factory(lambda cfg_, obs_space_: None)
    elif c.get("user") == "actor_critic":
        f.register_actor_critic_factory(lambda cfg_, obs_space_, action_space_: "user_module")
    try:
        ac = create_actor_critic(cfg, spaces.Dict(OBS[c["obs"]]), spaces.Discrete(5), c.get("device", "cuda"))
    finally:
        f.reset()
    assert ac.built == expected
    if expected == TORCH:
        assert ac.module == ("user_module" if c.get("user") == "actor_critic" else "default_torch_module")
