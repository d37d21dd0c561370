"""Action spaces with more than 128 distribution parameters through the whole engine: env -> policy forward (the fused
[F, 1 + A] heads GEMM) -> wave-per-row sampler -> slab -> Learner.train (V-trace, PPO loss, heads gradients) -> Adam."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from sample_factory_amd import lib as L
    L.load()
    return L


def test_wide_masked_bandit_end_to_end(lib):
    """Discrete(300) with obs["action_mask"]: no masked-out action is ever recorded, the recorded log-prob is the masked
    log-softmax of the recorded raw logits, the parameters stay finite and change, and the policy improves: the mean
    reward of the last 10 iterations is above that of the first 10 (a uniform policy over the ~150 allowed actions earns
    ~0.007 per step; nothing absolute is asserted)"""
    from sample_factory_amd.cfg.arguments import default_cfg
    from sample_factory_amd.envs.env_utils import register_env
    from sample_factory_amd.envs.synthetic import make_masked_bandit_env
    from sample_factory_amd.train import make_runner
    register_env("masked_bandit", make_masked_bandit_env)
    A, n_agents, iters = 300, 256, 60
    cfg = default_cfg(env="masked_bandit", use_rnn=False, nonlinearity="tanh", normalize_input=False,
                      encoder_mlp_layers=[64], rollout=8, batch_size=1024, num_batches_per_epoch=2, num_epochs=2,
                      num_workers=1, num_envs_per_worker=1, async_rl=False, seed=4, serial_mode=True,
                      synthetic_num_agents=n_agents, synthetic_num_actions=A, learning_rate=1e-2, gamma=0.0,
                      normalize_returns=False)
    cfg, runner = make_runner(cfg)
    runner.init()
    ac = runner.learner.actor_critic
    assert ac.num_action_params == A and runner.traj["obs"]["action_mask"].shape == (n_agents, 9, A)
    p0 = ac.flat_params.clone()
    rewards = []
    for it in range(iters):
        runner.iteration()
        tr = runner.traj
        # (column 0 of the slab already holds the NEXT rollout's first observation/mask: carry_over)
        a = tr["actions"][:, 1:, 0].long()
        mk = tr["obs"]["action_mask"][:, 1:-1]
        assert ((a >= 0) & (a < A)).all()
        assert mk.gather(-1, a.unsqueeze(-1)).all()                     # the sampler never picks a masked-out action
        lg = tr["action_logits"][:, 1:] + (mk == 0) * -1e9
        lp = torch.log_softmax(lg, -1).gather(-1, a.unsqueeze(-1)).squeeze(-1)
        assert (lp - tr["log_prob_actions"][:, 1:]).abs().max() < 1e-5
        rewards.append(float(tr["rewards"].mean()))
    assert torch.isfinite(ac.flat_params).all() and not torch.equal(p0, ac.flat_params)
    first, last = float(np.mean(rewards[:10])), float(np.mean(rewards[-10:]))
    print(f"masked bandit, {A} actions: mean reward of the first 10 iterations {first:.4f}, of the last 10 {last:.4f}")
    assert last > first, (first, last)


@pytest.mark.parametrize("async_rl", [False, True], ids=["sync", "async"])
def test_eight_head_tuple_with_vtrace_end_to_end(lib, async_rl):
    """Tuple of eight Discrete(21) members — 168 logits, every member narrow, the total wide — sampled, V-traced and trained
    on the wide kernels; the model round-trips through state_dict"""
    from sample_factory_amd.cfg.arguments import default_cfg
    from sample_factory_amd.envs.env_utils import register_env
    from sample_factory_amd.envs.synthetic import make_synthetic_tuple_env
    from sample_factory_amd.train import make_runner
    register_env("synthetic_tuple", make_synthetic_tuple_env)
    cfg = default_cfg(env="synthetic_tuple", use_rnn=False, nonlinearity="relu", normalize_input=False, obs_scale=255.0,
                      encoder_conv_architecture="convnet_atari", rollout=8, recurrence=8, batch_size=256,
                      num_batches_per_epoch=2, num_epochs=1, num_workers=1, num_envs_per_worker=1, async_rl=async_rl,
                      seed=2, serial_mode=not async_rl, synthetic_num_agents=64, kl_loss_coeff=0.05,
                      synthetic_head_sizes=(21,) * 8, with_vtrace=True, normalize_returns=False,
                      shuffle_minibatches=False)
    cfg, runner = make_runner(cfg)
    runner.init()
    ac = runner.learner.actor_critic
    # (async_rl: the slab holds the rollout being collected next to the one being trained on)
    assert ac.num_action_params == 168 and runner.traj["actions"].shape[1:] == (8, 8)
    p0 = ac.flat_params.clone()
    stats, trained = None, 0
    for _ in range(5):  # (async_rl: the first round only samples)
        out = runner.iteration()
        stats, trained = (out, trained + 1) if out is not None else (stats, trained)
    if async_rl:
        runner.stop_sampler_thread()
    torch.cuda.synchronize()
    assert trained >= 3
    tr = runner.traj
    a = tr["actions"]
    assert ((a >= 0) & (a < 21) & (a == a.round())).all()
    assert torch.isfinite(tr["log_prob_actions"]).all() and torch.isfinite(tr["action_logits"]).all()
    assert torch.isfinite(tr["values"]).all()
    assert np.isfinite(stats["train"]["loss"]) and stats["train"]["kl_divergence"] >= -1e-6
    assert torch.isfinite(ac.flat_params).all() and not torch.equal(p0, ac.flat_params)
    # recorded log-prob = sum of the eight members' log-softmax at the recorded actions
    lg = tr["action_logits"].view(a.shape[0], 8, 8, 21)
    lp = torch.log_softmax(lg, -1).gather(-1, a.long().unsqueeze(-1)).squeeze(-1).sum(-1)
    assert (lp - tr["log_prob_actions"]).abs().max() < 2e-5
    sd = {k: v.clone() for k, v in ac.state_dict().items()}
    flat = ac.flat_params.clone()
    ac.flat_params.zero_()
    ac.load_state_dict(sd)
    assert torch.equal(flat, ac.flat_params)
    sd2 = ac.state_dict()
    assert sd.keys() == sd2.keys() and all(torch.equal(sd[k], sd2[k]) for k in sd)


def test_deterministic_rollout_on_discrete_300(lib):
    """an evaluation-style rollout (rollout(deterministic=True)) on Discrete(300): the recorded action is the arg-max of
    the recorded logits"""
    from sample_factory_amd.cfg.arguments import default_cfg
    from sample_factory_amd.envs.env_utils import register_env
    from sample_factory_amd.envs.synthetic import SyntheticVecEnv
    from sample_factory_amd.train import make_runner

    def make_env(full_env_name, cfg=None, env_config=None, render_mode=None):
        return SyntheticVecEnv(num_agents=cfg.synthetic_num_agents, num_actions=300, seed=cfg.seed or 0)

    register_env("synthetic_discrete_300", make_env)
    cfg = default_cfg(env="synthetic_discrete_300", use_rnn=False, nonlinearity="relu", normalize_input=False,
                      obs_scale=255.0, encoder_conv_architecture="convnet_atari", rollout=8, batch_size=256,
                      num_batches_per_epoch=2, num_epochs=1, num_workers=1, num_envs_per_worker=1, async_rl=False, seed=3,
                      serial_mode=True, synthetic_num_agents=64)
    cfg, runner = make_runner(cfg)
    runner.init()
    runner.iteration()  # one training step: logits that are no longer the initial near-ties
    runner.sampler.rollout(deterministic=True)
    torch.cuda.synchronize()
    tr = runner.traj
    assert tr["action_logits"].shape == (64, 8, 300)
    assert torch.equal(tr["actions"][..., 0].long(), tr["action_logits"].argmax(-1))
    lp = torch.log_softmax(tr["action_logits"], -1).max(-1).values
    assert (lp - tr["log_prob_actions"]).abs().max() < 1e-5


@pytest.mark.parametrize("n,F,A", [(256, 64, 129), (1000, 512, 1000), (2048, 512, 4096)])
def test_heads_gemm_and_its_gradients_at_wide_cout(lib, n, F, A):
    """the fused heads layer [F, 1 + A (+ pad to 4)] as the model launches it (sf_conv_fwd / sf_conv_fwd_t on the layer's
    descriptor, sf_conv_wgrad, sf_conv_dgrad) and the plain linear entry points at the odd width 1 + A itself
    (130, 1001, 4097), against float64"""
    g = torch.Generator().manual_seed(n + A)
    for N in ((1 + A + 3) // 4 * 4, 1 + A):
        x = torch.randn((n, F), generator=g)
        w = torch.randn((F, N), generator=g) / np.sqrt(F)
        b = torch.randn(N, generator=g) * 0.1
        dy = torch.randn((n, N), generator=g)
        xd, wd, bd, dyd = x.cuda(), w.cuda(), b.cuda(), dy.cuda()
        ref = x.double() @ w.double() + b.double()
        rw, rb = x.double().t() @ dy.double(), dy.double().sum(0)
        rd = dy.double() @ w.double().t()
        tol = lambda r: 3e-5 * max(1.0, r.abs().max().item())
        if N % 4 == 0:
            d = lib.sf_conv_desc(Cin=F, H=1, W=1, Cout=N, KH=1, KW=1, stride=1, OH=1, OW=1, in_u8=0, relu=0, traj_T=0,
                                 sub_mean=0.0, inv_scale=1.0)
            out = torch.full((n, N), 7.0, device="cuda")
            lib.conv_fwd(xd, F, None, 0, wd, bd, out, n, d)
            assert (out.cpu().double() - ref).abs().max().item() < tol(ref), "heads forward"
            if lib.conv_fwd_t_supported(n, d):
                nb = lib.conv_fwd_t_workspace(n, d)
                ws = torch.empty(nb, dtype=torch.uint8, device="cuda") if nb else None
                out2 = torch.full((n, N), 7.0, device="cuda")
                lib.conv_fwd_t(xd, F, wd.t().contiguous(), bd, out2, n, d, ws)
                assert (out2.cpu().double() - ref).abs().max().item() < tol(ref), "heads forward (Cout-major weights)"
            dw, db = torch.zeros_like(wd), torch.zeros_like(bd)
            ws = torch.empty(lib.conv_wgrad_workspace(n, d), dtype=torch.uint8, device="cuda")
            lib.conv_wgrad(xd, F, None, 0, dyd, dw, db, n, d, ws)
            assert (dw.cpu().double() - rw).abs().max().item() < tol(rw), "heads weight gradient"
            assert (db.cpu().double() - rb).abs().max().item() < tol(rb), "heads bias gradient"
            din = torch.full((n, F), 7.0, device="cuda")
            lib.conv_dgrad(dyd, wd, None, din, n, d)
            assert (din.cpu().double() - rd).abs().max().item() < tol(rd), "heads data gradient"
        else:
            out = torch.full((n, N), 7.0, device="cuda")
            lib.linear_fwd(xd, wd, bd, out, n, F, N, False)
            assert (out.cpu().double() - ref).abs().max().item() < tol(ref), "linear forward"
            dw, db = torch.zeros_like(wd), torch.zeros_like(bd)
            ws = torch.empty(lib.linear_wgrad_workspace(n, F, N), dtype=torch.uint8, device="cuda")
            lib.linear_wgrad(xd, dyd, dw, db, n, F, N, ws)
            assert (dw.cpu().double() - rw).abs().max().item() < tol(rw), "linear weight gradient"
            assert (db.cpu().double() - rb).abs().max().item() < tol(rb), "linear bias gradient"
            din = torch.full((n, F), 7.0, device="cuda")
            lib.linear_dgrad(dyd, wd, torch.ones((n, F), device="cuda"), din, n, F, N)
            assert (din.cpu().double() - rd).abs().max().item() < tol(rd), "linear data gradient"
