"""Only the trajectories of the first minibatch are kept: the rollout launches are split at keep_n, the kept
buffers have keep_rows = batch_size // rollout rows, an env instance beyond them runs the plain forward.  As in
tests/test_gpu_rollout_reuse.py, cfg.reuse_rollout_activations=auto and =off must give the same bytes — parameters, Adam
moments, the loss scalars of every SGD step, the slab — over two iterations.
  * 256 agents, rollout 4, four minibatches of 256: 64 of 256 trajectories are kept, every launch is split at sample 64;
  * 1280 agents, four minibatches of 1280: all three conv layers are kept (320 of 1280 rows), the fc layer reads the two
    segments;
  * 4096 agents, four minibatches of 4096: the fc layer runs its unsplit 64 x 64 kernel, reads the two segments through its
    twin, and its output is reused as well (fc_reused);
  * two env instances of 256 agents, four minibatches of 512: instance 0 is split at 128, instance 1 keeps nothing and
    launches no strided kernel (counted through lib.PROFILE).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_gpu_rollout_reuse import _cfg, _prefix_expected, _same  # noqa: E402

ITERS = 2


def _run(knob, profile=False, **over):
    from sample_factory_amd import lib
    from sample_factory_amd.train import make_runner
    cfg, runner = make_runner(_cfg(reuse_rollout_activations=knob, **over))
    assert runner.init() == 0
    lr, ac = runner.learner, runner.learner.actor_critic
    scalars = []
    lib.PROFILE = {} if profile else None
    try:
        for _ in range(ITERS):
            runner.iteration()
            scalars.append(lr._scalars[:, :10].clone())
        torch.cuda.synchronize()
        launches = {k[-1]: len(v) for k, v in (lib.PROFILE or {}).items() if isinstance(k, tuple) and "_os<" in str(k[-1])}
    finally:
        lib.PROFILE = None
    out = dict(flat_params=ac.flat_params, exp_avg=lr.exp_avg, exp_avg_sq=lr.exp_avg_sq)
    out.update({f"scalars{i}": s for i, s in enumerate(scalars)})
    tr = runner.traj
    for k in ("actions", "action_logits", "log_prob_actions", "values", "rewards", "dones", "policy_version", "valids"):
        out["traj." + k] = tr[k]
    out["traj.obs"] = tr["obs"]["obs"]
    out = {k: v.detach().cpu().clone() for k, v in out.items()}
    kp = getattr(ac, "_keep", None)
    info = dict(stats=dict(lr.reuse_stats), prefix=kp["prefix"] if kp else 0, junction=kp["junction"] if kp else None,
                keep_rows=kp["rows"] if kp else 0, launches=launches,
                shapes={k: tuple(t.shape) for k, t in ac._bufs.items() if isinstance(k, tuple) and k and k[0] == "keep"})
    runner.close_envs()
    return out, info


def _pair(**over):
    on, info = _run("auto", **over)
    off, info_off = _run("off", **{k: v for k, v in over.items() if k != "profile"})
    _same(on, off)
    assert info_off["prefix"] == 0 and not info_off["shapes"] and info_off["stats"]["reused"] == 0
    assert info["stats"]["reused"] == ITERS and info["stats"]["plain"] == 0, info
    return info


def test_a_quarter_of_the_rows_is_kept():
    info = _pair()
    want = _prefix_expected(256, 256)
    assert want >= 1 and info["prefix"] == want and info["stats"]["last_prefix"] == want, info
    assert info["keep_rows"] == 64 and info["junction"] in ("twin", "copy")
    assert info["shapes"] and all(s[0] == 64 and s[1] == 4 for s in info["shapes"].values()), info["shapes"]


def test_three_layers_and_the_fc_junction():
    over = dict(synthetic_num_agents=1280, batch_size=1280)
    info = _pair(**over)
    want = _prefix_expected(1280, 1280)
    assert info["prefix"] == want and info["stats"]["last_prefix"] == want and info["keep_rows"] == 320, info
    assert all(s[0] == 320 for s in info["shapes"].values()), info["shapes"]
    from tests.test_gpu_kernel_ledger import DEFAULT_SWITCHES
    assert want == 3 or not DEFAULT_SWITCHES
    if DEFAULT_SWITCHES:  # the fc launch of 1280 samples is split along K: its output is never reused
        assert info["stats"]["fc_reused"] == 0 and ("keep", "fc") not in info["shapes"]


def test_fc_is_reused_where_it_runs_unsplit():
    over = dict(synthetic_num_agents=4096, batch_size=4096)
    info = _pair(**over)
    want = _prefix_expected(4096, 4096)
    assert info["prefix"] == want and info["keep_rows"] == 1024 and info["stats"]["last_prefix"] == want, info
    from tests.test_gpu_kernel_ledger import DEFAULT_SWITCHES
    if DEFAULT_SWITCHES:
        assert want == 3 and info["junction"] == "twin" and info["stats"]["fc_reused"] == ITERS, info
        assert info["shapes"][("keep", "fc")] == (1024, 4, 512)


def test_an_instance_beyond_the_first_minibatch_keeps_nothing():
    over = dict(num_envs_per_worker=2, worker_num_splits=2, batch_size=512, num_batches_per_epoch=4)
    info = _pair(profile=True, **over)
    want = _prefix_expected(256, 512)
    assert want >= 1 and info["prefix"] == want and info["keep_rows"] == 128, info
    assert all(s[0] == 128 for s in info["shapes"].values()), info["shapes"]
    # instance 0 launches `prefix` strided kernels per rollout step (and the junction's twin, if it has one); instance 1 none
    per_step = want + (1 if info["junction"] == "twin" else 0)
    assert sum(info["launches"].values()) == per_step * 4 * ITERS, info["launches"]
