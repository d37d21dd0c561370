"""The two kernels of --track_inactive_agents against numpy oracles written here and against the plain
kernels they stand in for: sf_traj_write_env_step_active and sf_rnn_store_state_held."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T = 5
SLAB = ("rewards", "dones", "time_outs", "policy_id")


@pytest.fixture(scope="module")
def lib():
    from sample_factory_amd import lib as L
    L.load()
    return L


def dev(x, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(x))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda().contiguous()


def _buffers(B):
    tr = dict(rewards=torch.full((B, T), 7.0, device="cuda"), dones=torch.zeros((B, T), dtype=torch.bool, device="cuda"),
              time_outs=torch.zeros((B, T), dtype=torch.bool, device="cuda"),
              policy_id=torch.full((B, T), 9, dtype=torch.int32, device="cuda"))
    ep = dict(ep_return=dev(np.linspace(-1, 1, B).astype(np.float32)), ep_len=dev(np.arange(B, dtype=np.int32) % 4),
              ep_stats=torch.zeros(3, dtype=torch.float64, device="cuda"))
    return tr, ep


def _bits(bufs):
    return {k: v.cpu().numpy().tobytes() for d in bufs for k, v in d.items()}


@pytest.mark.parametrize("B", [1, 64, 70])
def test_write_env_step_active_against_the_oracle_and_the_plain_kernel(lib, B):
    """all T steps in sequence: policy_id = -1 where the PREVIOUS report said inactive (the state starts at 1), the state
    after every step is this step's report; everything else is what sf_traj_write_env_step writes on the same inputs"""
    rng = np.random.default_rng(B)
    PID, scale, clip = 3, 0.5, 2.0
    tr, ep = _buffers(B)          # written by the new kernel
    tr0, ep0 = _buffers(B)        # copies, written by the plain kernel
    state = torch.ones(B, dtype=torch.uint8, device="cuda")
    want_state = np.ones(B, bool)
    for t in range(T):
        rew = (rng.standard_normal(B) * 6).astype(np.float32)   # well beyond clip / scale = 4
        term, trunc = rng.random(B) < 0.3, rng.random(B) < 0.2
        flags = rng.random(B) < 0.5
        # the report as the runner hands it over: bool bytes; any non-zero byte counts as active
        active_in = dev(np.where(flags, rng.integers(1, 256, B), 0).astype(np.uint8))
        args = (dev(rew), dev(term, torch.bool), dev(trunc, torch.bool), T, t, scale, clip, PID)
        lib.traj_write_env_step_active(*args, tr["rewards"], tr["dones"], tr["time_outs"], tr["policy_id"], ep["ep_return"],
                                       ep["ep_len"], ep["ep_stats"], active_in, state)
        lib.traj_write_env_step(*args, tr0["rewards"], tr0["dones"], tr0["time_outs"], tr0["policy_id"], ep0["ep_return"],
                                ep0["ep_len"], ep0["ep_stats"])
        np.testing.assert_array_equal(tr["policy_id"][:, t].cpu().numpy(), np.where(want_state, PID, -1), err_msg=f"step {t}")
        want_state = flags
        np.testing.assert_array_equal(state.cpu().numpy(), want_state.astype(np.uint8), err_msg=f"state after step {t}")
        np.testing.assert_array_equal(tr["dones"][:, t].cpu().numpy(), term | trunc)
        np.testing.assert_array_equal(tr["time_outs"][:, t].cpu().numpy(), trunc)
        assert np.abs(rew * scale).max() > clip or B == 1
        a, b = _bits([tr, ep]), _bits([tr0, ep0])
        for k in a:
            if k != "policy_id":
                assert a[k] == b[k], f"step {t}: {k} differs from sf_traj_write_env_step"
        assert (tr["policy_id"][:, t + 1:] == 9).all() and (tr["rewards"][:, t + 1:] == 7.0).all()
    assert (tr0["policy_id"] == PID).all()
    assert ep["ep_stats"][2].item() > 0 or B == 1


@pytest.mark.parametrize("B", [1, 64, 70])
def test_write_env_step_active_with_all_flags_set_is_the_plain_kernel(lib, B):
    """an env that never reports is_active: the whole slab, policy_id included, holds the plain kernel's bits (also
    without episode statistics and without a truncated array, which both kernels take as NULL)"""
    rng = np.random.default_rng(100 + B)
    tr, ep = _buffers(B)
    tr0, ep0 = _buffers(B)
    state, ones = torch.ones(B, dtype=torch.uint8, device="cuda"), torch.ones(B, dtype=torch.bool, device="cuda")
    for t in range(T):
        rew = dev((rng.standard_normal(B) * 6).astype(np.float32))
        term = dev(rng.random(B) < 0.3, torch.bool)
        trunc = dev(rng.random(B) < 0.2, torch.bool) if t % 2 == 0 else None
        stats = t < 3
        e, e0 = (ep, ep0) if stats else (dict.fromkeys(ep), dict.fromkeys(ep0))
        lib.traj_write_env_step_active(rew, term, trunc, T, t, 0.5, 2.0, 0, tr["rewards"], tr["dones"], tr["time_outs"],
                                       tr["policy_id"], e["ep_return"], e["ep_len"], e["ep_stats"], ones, state)
        lib.traj_write_env_step(rew, term, trunc, T, t, 0.5, 2.0, 0, tr0["rewards"], tr0["dones"], tr0["time_outs"],
                                tr0["policy_id"], e0["ep_return"], e0["ep_len"], e0["ep_stats"])
    assert _bits([tr, ep]) == _bits([tr0, ep0])
    assert (state == 1).all() and (ones == 1).all()


def test_write_env_step_active_refuses_through_the_wrapper(lib):
    tr, ep = _buffers(4)
    z, zb = torch.zeros(4, device="cuda"), torch.zeros(4, dtype=torch.bool, device="cuda")
    state = torch.ones(4, dtype=torch.uint8, device="cuda")
    call = lambda a_in, st: lib.traj_write_env_step_active(  # noqa: E731
        z, zb, zb, T, 0, 1.0, 1.0, 0, tr["rewards"], tr["dones"], tr["time_outs"], tr["policy_id"], ep["ep_return"],
        ep["ep_len"], ep["ep_stats"], a_in, st)
    for a_in, st in ((None, state), (zb, None), (state, state), (torch.ones(5, dtype=torch.bool, device="cuda"), state)):
        with pytest.raises(lib.SfHipError):
            call(a_in, st)
    assert (tr["policy_id"] == 9).all() and (state == 1).all()  # nothing ran


def _held_oracle(h, c, done, prev, pid):
    new = h if c is None else np.concatenate([h, c], 1)
    return np.where(done[:, None], np.float32(0.0), np.where((pid < 0)[:, None], prev, new))


@pytest.mark.parametrize("lstm", [False, True], ids=["gru", "lstm"])
@pytest.mark.parametrize("H", [32, 33])
@pytest.mark.parametrize("B", [1, 70])
def test_store_state_held_against_the_formula_and_the_plain_kernel(lib, B, H, lstm):
    """two stacked layers = two column slices of the strided view rnn_states[:, t] -> [:, t + 1]; exact equality (a select
    and a mask: no arithmetic).  The policy_id / dones columns are strided slab columns as well."""
    rng = np.random.default_rng(1000 * B + 2 * H + lstm)
    SL = 2 * H if lstm else H
    t = 2
    slab_np = rng.standard_normal((B, T + 1, 2 * SL)).astype(np.float32)
    slab = dev(slab_np)
    pid_np = np.where(rng.random((B, T)) < 0.5, -1, 2).astype(np.int32)
    if B > 1:
        pid_np[0, t], pid_np[1, t] = -1, 2   # both kinds of row are there
    done_np = rng.random((B, T)) < 0.3
    pid, dones = dev(pid_np), dev(done_np, torch.bool)
    want = slab_np.copy()
    parts = []
    for l in range(2):
        h = rng.standard_normal((B, H)).astype(np.float32)
        c = rng.standard_normal((B, H)).astype(np.float32) if lstm else None
        parts.append((dev(h), dev(c) if lstm else None))
        cols = slice(l * SL, (l + 1) * SL)
        want[:, t + 1, cols] = _held_oracle(h, c, done_np[:, t], slab_np[:, t, cols], pid_np[:, t])
    for l, (h, c) in enumerate(parts):
        cols = slice(l * SL, (l + 1) * SL)
        lib.rnn_store_state_held(h, c, dones[:, t], slab[:, t, cols], pid[:, t], slab[:, t + 1, cols])
    got = slab.cpu().numpy()
    assert got.tobytes() == want.tobytes()  # column t + 1 is the formula, every other column is untouched
    # no negative policy_id: the bits of sf_rnn_store_state
    a, b = dev(slab_np), dev(slab_np)
    valid = torch.full((B, T), 2, dtype=torch.int32, device="cuda")
    for l, (h, c) in enumerate(parts):
        cols = slice(l * SL, (l + 1) * SL)
        lib.rnn_store_state_held(h, c, dones[:, t], a[:, t, cols], valid[:, t], a[:, t + 1, cols])
        lib.rnn_store_state(h, c, dones[:, t], b[:, t + 1, cols])
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


@pytest.mark.parametrize("col0,width", [(1, 40), (0, 41), (4, 40)], ids=["base+1", "odd_stride", "base+4"])
def test_store_state_held_on_views_the_16_byte_path_cannot_take(lib, col0, width):
    """H = 32 allows 16-byte accesses, a view that starts one float into the row or whose rows are an odd number of floats
    apart does not (base+4 does): the same result either way, nothing written outside the view"""
    B, H, t = 70, 32, 1
    rng = np.random.default_rng(col0 + width)
    slab_np = rng.standard_normal((B, 3, width)).astype(np.float32)
    h, done = rng.standard_normal((B, H)).astype(np.float32), rng.random(B) < 0.3
    pid = np.where(rng.random(B) < 0.5, -1, 0).astype(np.int32)
    slab, cols = dev(slab_np), slice(col0, col0 + H)
    lib.rnn_store_state_held(dev(h), None, dev(done, torch.bool), slab[:, t, cols], dev(pid), slab[:, t + 1, cols])
    want = slab_np.copy()
    want[:, t + 1, cols] = _held_oracle(h, None, done, slab_np[:, t, cols], pid)
    assert slab.cpu().numpy().tobytes() == want.tobytes()


def test_store_state_held_refuses_overlap_through_the_wrapper(lib):
    B, H = 4, 32
    slab = torch.zeros((B, 3, 2 * H), device="cuda")
    h, dones = torch.ones((B, H), device="cuda"), torch.zeros((B, 3), dtype=torch.bool, device="cuda")
    pid = torch.zeros((B, 3), dtype=torch.int32, device="cuda")
    with pytest.raises(lib.SfHipError, match="overlaps"):
        lib.rnn_store_state_held(h, None, dones[:, 0], slab[:, 0, :H], pid[:, 0], slab[:, 0, :H])
    with pytest.raises(lib.SfHipError, match="overlaps"):
        lib.rnn_store_state_held(h, None, dones[:, 0], slab[:, 0, :H], pid[:, 0], slab[:, 0, 1:H + 1])
    with pytest.raises(lib.SfHipError):
        lib.rnn_store_state_held(h, None, dones[:, 0], slab[:, 0, :H], pid[:, 0].long(), slab[:, 1, :H])
    assert (slab == 0).all()
    lib.rnn_store_state_held(h, None, dones[:, 0], slab[:, 0, :H], pid[:, 0], slab[:, 0, H:])  # neighbours: fine
    assert (slab[:, 0, H:] == 1).all() and (slab[:, 0, :H] == 0).all() and (slab[:, 1:] == 0).all()
