"""What the env-defined episode statistics cost:

 * sf_episode_stats_add at B = 4096 with K = 1, 4 and 16 f32 channels, against sf_copy_rows on the same bytes (the
   library's smallest launch that moves them), replayed from launch programs, the two alternating window by window;
 * a synchronous rollout step of the c2 shape (synthetic_atari frames, convnet_atari, 4096 agents, rollout 32) with the
   env stepped through step(): reporting 4 per-agent device tensors in a dict, against the same env reporting nothing —
   the difference is the added cost per rollout step with infos on;
 * the same rollout on the zero-copy env (no infos: the flagship path), and — with --parent_root, the root of a built
   checkout of the parent commit — that rollout on the parent's code, each window in a fresh process, alternating.

  python tools/episode_stats_bench.py [--windows 7] [--parent_root DIR] [--out profiles/episode_stats_bench.json]"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T, PROG = 4096, 32, 32


def _stats(v):
    v = sorted(v)
    return dict(median=round(v[len(v) // 2], 3), min=round(v[0], 3), max=round(v[-1], 3))


class StepOnlyEnv:
    """the synthetic frame env behind step() alone (no zero-copy hook), reporting `channels` per-agent f32 tensors"""

    def __init__(self, inner, channels):
        import torch
        self.inner, self.num_agents = inner, inner.num_agents
        self.observation_space, self.action_space = inner.observation_space, inner.action_space
        self.vals = [torch.full((self.num_agents,), float(k), device="cuda") for k in range(channels)]

    def reset(self, **kw):
        return self.inner.reset(**kw)

    def step(self, actions):
        o, r, te, tr, _ = self.inner.step(actions)
        return o, r, te, tr, ({f"stat_{k}": v for k, v in enumerate(self.vals)} if self.vals else {})

    def close(self):
        pass


def _make_step_only(name, cfg=None, env_config=None, render_mode=None):
    from sample_factory_amd.envs.synthetic import make_synthetic_env
    return StepOnlyEnv(make_synthetic_env(name, cfg, env_config, render_mode), int(getattr(cfg, "bench_info_channels", 0)))


def rollout_us_per_step(env_name: str, channels: int, rollouts: int) -> float:
    """one window: `rollouts` synchronous rollouts of T steps, HIP-event timed, after two warm-up rollouts"""
    import torch
    from sample_factory_amd.cfg.arguments import default_cfg
    from sample_factory_amd.envs.env_utils import register_env
    from sample_factory_amd.envs.synthetic import make_synthetic_env
    from sample_factory_amd.train import make_runner
    register_env("synthetic_atari", make_synthetic_env)
    register_env("synthetic_atari_step", _make_step_only)
    cfg = default_cfg(env=env_name, use_rnn=False, recurrence=1, encoder_conv_architecture="convnet_atari",
                      nonlinearity="relu", encoder_conv_mlp_layers=[512], obs_scale=255.0, normalize_input=False, rollout=T,
                      batch_size=B * T // 8, num_batches_per_epoch=8, num_epochs=1, num_workers=1, num_envs_per_worker=1,
                      async_rl=False, serial_mode=True, seed=0, synthetic_num_agents=B, bench_info_channels=channels,
                      train_dir=tempfile.mkdtemp(prefix="episode_stats_bench_"), experiment="b")
    cfg, runner = make_runner(cfg)
    assert runner.init() == 0
    sm = runner.sampler
    for _ in range(3):  # plain run, recording, first replay
        sm.rollout(0.0)
        sm.carry_over()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(rollouts):
        sm.rollout(0.0)
        sm.carry_over()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / (rollouts * T)
    runner.close_envs()
    return us


def child(root: str, env_name: str, channels: int, rollouts: int) -> float:
    """the same window in a fresh process that imports the package under `root`"""
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", env_name, str(channels), str(rollouts), root],
                         capture_output=True, text=True, check=True, timeout=300).stdout
    return float(out.strip().splitlines()[-1])


def kernel_part(windows: int, reps: int) -> dict:
    import torch
    from sample_factory_amd import lib
    g = torch.Generator(device="cuda")
    g.manual_seed(0)
    term = torch.rand(B, device="cuda", generator=g) < 0.02
    trunc = torch.rand(B, device="cuda", generator=g) < 0.01
    out = {}
    for K in (1, 4, 16):
        vals = torch.randn(K, B, device="cuda", generator=g)
        dst = torch.empty_like(vals)
        acc = torch.zeros((K, 2), dtype=torch.float64, device="cuda")
        progs = {}
        for name, fn in (("episode_stats_add", lambda: lib.episode_stats_add(list(vals), term, trunc, None, acc)),
                         ("copy_rows", lambda: lib.copy_rows(dst, vals))):
            with lib.record_launches() as prog:
                for _ in range(PROG):
                    fn()
            assert prog.unsafe is None and len(prog.calls) == PROG
            progs[name] = prog

        def window(prog):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                prog.replay()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / (reps * PROG)
        ms = {name: [] for name in progs}
        for prog in progs.values():
            window(prog)
        for _ in range(windows):
            for name, prog in progs.items():
                ms[name].append(window(prog))
        out[f"K{K}"] = dict(bytes_read=K * B * 4 + 2 * B, us_per_launch={n: _stats(v) for n, v in ms.items()})
    return out


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        env_name, channels, rollouts, root = sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
        sys.path.insert(0, root)
        print(rollout_us_per_step(env_name, channels, rollouts))
        return
    p = argparse.ArgumentParser()
    p.add_argument("--windows", type=int, default=7)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--rollouts", type=int, default=6)
    p.add_argument("--parent_root", default=None)
    p.add_argument("--commit", default=None, help="what to record as the commit (default: git's HEAD of this checkout)")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "episode_stats_bench.json"))
    args = p.parse_args()
    sys.path.insert(0, ROOT)
    from sample_factory_amd import build
    commit = args.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                           text=True).stdout.strip()
    out = dict(commit=commit or None, source_sha16=build.source_sha16(), agents=B, rollout=T,
               windows=args.windows, kernel=kernel_part(args.windows, args.reps))
    legs = dict(step_env_4_channels=(ROOT, "synthetic_atari_step", 4), step_env_no_infos=(ROOT, "synthetic_atari_step", 0),
                zero_copy_no_infos=(ROOT, "synthetic_atari", 0))
    if args.parent_root:
        legs["zero_copy_no_infos_parent"] = (os.path.abspath(args.parent_root), "synthetic_atari", 0)
    us = {name: [] for name in legs}
    for _ in range(args.windows):  # alternating windows, every one a fresh process: all legs see the same machine
        for name, (root, env_name, channels) in legs.items():
            us[name].append(child(root, env_name, channels, args.rollouts))
    roll = {name: dict(us_per_rollout_step=_stats(v), windows=[round(x, 2) for x in v]) for name, v in us.items()}
    med = lambda n: roll[n]["us_per_rollout_step"]["median"]  # noqa: E731
    roll["added_us_per_step_with_4_channels"] = round(med("step_env_4_channels") - med("step_env_no_infos"), 2)
    if args.parent_root:
        roll["no_infos_over_parent"] = round(med("zero_copy_no_infos") / med("zero_copy_no_infos_parent"), 4)
        pv = us["zero_copy_no_infos_parent"]
        roll["parent_window_spread"] = round((max(pv) - min(pv)) / med("zero_copy_no_infos_parent"), 4)
    out["rollout"] = roll
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
