"""resnet_impala (model/encoder.py:153-221 of the reference) without a GPU: the model factory builds it (the torch path on a
CPU device) with the reference's parameter names, shapes and count, and its forward equals the reference's on seeded weights
(tests/golden/model_fwd_resnet.npz, written by tools/gen_golden_resnet.py)."""
import ast
import os

import numpy as np
import pytest
import torch

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "model_fwd_resnet.npz"), allow_pickle=True)


def _model(tag, device):
    from sample_factory_amd.cfg.arguments import default_cfg
    from sample_factory_amd.envs import spaces
    from sample_factory_amd.model.model_factory import create_actor_critic
    obs = G[f"{tag}_obs"]
    cfg = default_cfg(encoder_conv_architecture="resnet_impala", nonlinearity=str(G[f"{tag}_nonlinearity"]),
                      obs_scale=255.0, obs_subtract_mean=0.0, normalize_input=False, use_rnn=False,
                      normalize_returns=False)
    cfg.dp_world = 1
    space = spaces.Dict({"obs": spaces.Box(0, 255, tuple(obs.shape[1:]), np.uint8)})
    return create_actor_critic(cfg, space, spaces.Discrete(6), torch.device(device))


def _seeded(tag):
    from oracle.weights import seeded_state
    shapes = [(str(n), ast.literal_eval(str(s))) for n, s in zip(G[f"{tag}_param_names"], G[f"{tag}_param_shapes"])]
    return shapes, {k: torch.from_numpy(v) for k, v in seeded_state(shapes, int(G[f"{tag}_param_seed"])).items()}


@pytest.mark.parametrize("tag", ["elu84", "relu84", "odd"])
def test_resnet_impala_cpu_torch_path_matches_reference(tag):
    from sample_factory_amd.model.torch_policy import TorchPolicyAdapter
    ac = _model(tag, "cpu")
    assert isinstance(ac, TorchPolicyAdapter)
    shapes, sd = _seeded(tag)
    assert [(n, tuple(s)) for n, s in ac.ref_param_shapes()] == [(n, tuple(s)) for n, s in shapes]
    assert ac.num_params() == int(G[f"{tag}_num_params"])
    if tag == "elu84":
        assert ac.num_params() == 2084311 and len(shapes) == 36
    ac.load_state_dict(sd, strict=True)
    ac.eval()
    res = ac.forward({"obs": torch.from_numpy(G[f"{tag}_obs"])}, None)
    np.testing.assert_allclose(res["action_logits"].detach().numpy(), G[f"{tag}_action_logits"], atol=2e-5, rtol=1e-4)
    np.testing.assert_allclose(res["values"].detach().numpy(), G[f"{tag}_values"], atol=2e-5, rtol=1e-4)
