"""Feed a checkpoint written by THIS engine (tests/golden/ours_checkpoint_mlp.pth) to the REFERENCE's Learner
(TEST INFRASTRUCTURE; the reference is imported as oracle/ref_import.py resolves it, SF_REFERENCE_ROOT first).
python -m oracle.check_our_checkpoint"""
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

from oracle import ref_import  # noqa: F401
import gymnasium as gym  # the stub
from oracle.gen_golden import MLP_OBS, make_learner
import sample_factory.cfg.arguments as ref_arguments
from sample_factory.cfg.arguments import parse_full_cfg, parse_sf_args

# parse_full_cfg tags the config with the git revision of the working directory, found by listing every directory above
# it (utils.git_root): that fails where an ancestor may not be listed and has nothing to do with loading a checkpoint,
# so the check answers it the way the reference does outside a git checkout
ref_arguments.get_git_commit_hash = lambda: ("unknown", "not a git repository")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    g = np.load(os.path.join(ROOT, "tests", "golden", "ours_checkpoint_mlp.npz"))
    train_dir = tempfile.mkdtemp(prefix="sf_ours_ckpt_")
    d = os.path.join(train_dir, "ours_ckpt", "checkpoint_p0")
    os.makedirs(d)
    shutil.copy(os.path.join(ROOT, "tests", "golden", "ours_checkpoint_mlp.pth"), os.path.join(d, str(g["file_name"])))
    argv = ["--algo=APPO", "--env=synthetic", "--experiment=ours_ckpt", f"--train_dir={train_dir}", "--device=cpu",
            "--serial_mode=True", "--seed=0", "--use_rnn=False", "--recurrence=1", "--rollout=8", "--batch_size=64",
            "--num_batches_per_epoch=2", "--num_epochs=2"] + str(g["argv"]).split()
    parser, _ = parse_sf_args(argv)
    cfg = parse_full_cfg(parser, argv)
    learner, _ = make_learner(cfg, MLP_OBS, gym.spaces.Discrete(6), 16)   # Learner.init() -> load_from_checkpoint
    assert learner.train_step == int(g["train_step"]) and learner.env_steps == int(g["env_steps"]), \
        (learner.train_step, learner.env_steps)
    st = learner.optimizer.state_dict()["state"]
    assert len(st) == len(list(learner.actor_critic.parameters())) and float(st[0]["step"]) == int(g["train_step"])
    ac = learner.actor_critic
    ac.eval()
    with torch.no_grad():
        res = ac.forward_tail(ac.forward_head(ac.normalize_obs({"obs": torch.from_numpy(g["probe"]).clone()})),
                              values_only=False, sample_actions=False)
    np.testing.assert_allclose(res["action_logits"].numpy(), g["logits"], atol=2e-5, rtol=1e-4)
    np.testing.assert_allclose(res["values"].numpy(), g["values"], atol=2e-5, rtol=1e-4)
    print("INTEROP OK", learner.train_step, learner.env_steps)
    shutil.rmtree(train_dir, ignore_errors=True)


if __name__ == "__main__":
    main()
