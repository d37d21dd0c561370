"""The observation ingest plan (algo/sampling/obs_ingest.py) without a GPU: what ObsIngestPlan.from_cfg derives and refuses,
and — with the library wrappers replaced by recorders and tensors on the CPU — the exact calls a KeyRoute makes for every
combination of the three stages: which function, on which views of the slab leaf, with which scalars."""
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from sample_factory_amd.envs import spaces  # noqa: E402

B, T, K = 3, 2, 4
H, W, C = 6, 8, 3
OH, OW = 3, 4


def _space(hwc: bool, dtype=np.uint8, shape=None):
    return spaces.Dict({"obs": spaces.Box(0, 255, shape or ((H, W, C) if hwc else (C, H, W)), dtype),
                        "vec": spaces.Box(-1.0, 1.0, (5,), np.float32), "action_mask": spaces.Box(0, 1, (4,), np.uint8)})


def _cfg(hwc=False, rs=False, k=1, **kw):
    from sample_factory_amd.cfg.arguments import default_cfg
    flags = dict(hwc_observations=hwc, device_resize=[OH, OW] if rs else [], device_grayscale=rs, device_framestack=k)
    return default_cfg(env="x", **dict(flags, **kw))


def _plan(hwc=False, rs=False, k=1, zero_copy=False, space=None, **kw):
    from sample_factory_amd.algo.sampling.obs_ingest import ObsIngestPlan
    return ObsIngestPlan.from_cfg(space or _space(hwc), _cfg(hwc, rs, k, **kw), zero_copy)


class Calls:
    """recorders in place of the library wrappers and of the runner's _to_device: a tensor argument is written down as
    "stage" (the route's staging buffer), as (shape, strides, offset relative to the leaf) for a view of the slab leaf, or
    kept as the object it is"""

    def __init__(self, monkeypatch):
        from sample_factory_amd import lib
        self.log, self.x, self.route = [], None, None
        for fn in ("framestack_step", "framestack_step_hwc", "hwc_to_chw", "frame_resize"):
            monkeypatch.setattr(lib, fn, lambda *a, _fn=fn: self.log.append((_fn,) + tuple(self.seen(v) for v in a)))

    def seen(self, v):
        if not isinstance(v, torch.Tensor):
            return v
        if self.route.stage is not None and v is self.route.stage:
            return "stage"
        if v.untyped_storage().data_ptr() == self.x.untyped_storage().data_ptr():
            return tuple(v.shape), v.stride(), v.storage_offset() - self.x.storage_offset()
        return v

    def to_device(self, name, src, dst):
        self.log.append(("to_device", name, src, self.seen(dst)))

    def take(self):
        out, self.log = self.log, []
        return out


def _leaf(slab_shape, dtype=torch.uint8):
    """a slab leaf [B, T + 1, *slab_shape] that is a view at an offset into a larger allocation, as traj[rows] is"""
    return torch.zeros((B + 1, T + 1) + tuple(slab_shape), dtype=dtype)[1:]


@pytest.mark.parametrize("k", [1, K])
@pytest.mark.parametrize("rs", [False, True], ids=["native", "resize_grey"])
@pytest.mark.parametrize("hwc", [False, True], ids=["chw", "hwc"])
def test_a_route_makes_exactly_the_calls_of_its_configuration(monkeypatch, hwc, rs, k):
    from sample_factory_amd.algo.sampling.obs_ingest import KeyRoute
    key = _plan(hwc, rs, k).keys["obs"]
    c1, h1, w1 = (1, OH, OW) if rs else (C, H, W)
    assert key.image and key.hwc == hwc and key.k == k and key.dtype == np.uint8
    assert key.native_shape == ((H, W, C) if hwc else (C, H, W))
    assert key.resize == ((OH, OW) if rs else None) and key.gray == rs and key.interp == "area"
    assert key.frame_shape == (c1, h1, w1) and key.slab_shape == (k * c1, h1, w1)

    x = _leaf(key.slab_shape)
    calls = Calls(monkeypatch)
    calls.x = x
    route = calls.route = KeyRoute(key, x)
    if hwc or rs:
        assert route.stage.shape == (B,) + key.native_shape and route.stage.dtype == torch.uint8
    else:
        assert route.stage is None

    frame_elems = c1 * h1 * w1
    col_elems = k * frame_elems
    pitch = (T + 1) * col_elems

    def view(t, slot=False):  # x[:, t], or the last frame slot of it, relative to the leaf
        return ((B, c1 if slot else k * c1, h1, w1), (pitch, h1 * w1, w1, 1),
                t * col_elems + ((k - 1) * frame_elems if slot else 0))

    term, trunc = torch.zeros(B, dtype=torch.bool), torch.ones(B, dtype=torch.bool)
    for t in range(T + 1):
        src = np.zeros((B,) + key.native_shape, np.uint8)
        flags = (None, None) if t == 0 else (term, trunc)
        assert route.slot(x, t).data_ptr() == x[:, t, (k - 1) * c1:].data_ptr() and route.slot(x, t).shape == (B, c1, h1, w1)
        route.store(x, "obs", src, t, calls.to_device)
        if rs:
            want = [("to_device", "obs", src, "stage"), ("frame_resize", view(t, slot=k > 1), "stage", hwc, "area", True)]
        elif hwc:
            want = [("to_device", "obs", src, "stage")] + ([("hwc_to_chw", view(t), "stage")] if k == 1 else [])
        else:
            want = [("to_device", "obs", src, view(t, slot=k > 1))]
        got = calls.take()
        assert len(got) == len(want) and all(len(g) == len(w_) and all(a is b or a == b for a, b in zip(g, w_))
                                             for g, w_ in zip(got, want)), (got, want)
        assert route.frame is (route.stage if (hwc or rs) else None)

        route.complete(x, t, *flags)
        prev = view(t - 1 if t > 0 else 1)
        if k == 1:
            want = []
        elif hwc and not rs:
            want = [("framestack_step_hwc", view(t), prev, K, "stage") + flags]
        else:
            want = [("framestack_step", view(t), prev, K, None) + flags]
        got = calls.take()
        assert len(got) == len(want) and all(len(g) == len(w_) and all(a is b or a == b for a, b in zip(g, w_))
                                             for g, w_ in zip(got, want)), (got, want)


@pytest.mark.parametrize("k", [1, K])
@pytest.mark.parametrize("rs", [False, True], ids=["native", "resize_grey"])
@pytest.mark.parametrize("hwc", [False, True], ids=["chw", "hwc"])
def test_vector_and_mask_keys_come_out_untouched(monkeypatch, hwc, rs, k):
    from sample_factory_amd.algo.sampling.obs_ingest import KeyRoute
    space = _space(hwc)
    plan = _plan(hwc, rs, k, space=space)
    assert list(plan.keys) == ["obs", "vec", "action_mask"] and plan.identity == (not hwc and not rs and k == 1)
    slab = plan.slab_obs_space()
    assert slab["obs"].shape == plan.keys["obs"].slab_shape
    for name, dtype in (("vec", torch.float32), ("action_mask", torch.uint8)):
        key = plan.keys[name]
        assert slab[name] is space[name]
        assert (key.image, key.hwc, key.resize, key.k) == (False, False, None, 1)
        assert key.native_shape == key.frame_shape == key.slab_shape == space[name].shape and key.dtype == space[name].dtype
        x = _leaf(key.slab_shape, dtype)
        calls = Calls(monkeypatch)
        calls.x, calls.route = x, KeyRoute(key, x)
        assert calls.route.stage is None
        for t in range(T + 1):
            src = np.zeros((B,) + key.native_shape)
            calls.route.store(x, "obs." + name, src, t, calls.to_device)
            calls.route.complete(x, t, None, None)
            n = key.slab_shape[0]
            (got,) = calls.take()   # exactly one transfer, straight into the column, and no launch
            assert got[:2] == ("to_device", "obs." + name) and got[2] is src and got[3] == ((B, n), ((T + 1) * n, 1), t * n)


class _OnDevice(torch.Tensor):
    """a CPU tensor that says it lives on the device: what the in-place test looks at"""
    is_cuda = True


@pytest.mark.parametrize("rs", [False, True], ids=["transposed", "preprocessed"])
def test_a_device_tensor_with_contiguous_rows_is_read_in_place(monkeypatch, rs):
    from sample_factory_amd.algo.sampling.obs_ingest import KeyRoute
    key = _plan(True, rs, 1).keys["obs"]
    x = _leaf(key.slab_shape)
    calls = Calls(monkeypatch)
    calls.x = x
    route = calls.route = KeyRoute(key, x)
    kernel = "frame_resize" if rs else "hwc_to_chw"
    tight = torch.zeros((B, H, W, C), dtype=torch.uint8)
    pitched = torch.zeros((B, 2, H, W, C), dtype=torch.uint8)[:, 0]               # contiguous rows, further apart
    for src in (tight, pitched):
        src = src.as_subclass(_OnDevice)
        route.store(x, "obs", src, 1, calls.to_device)
        (got,) = calls.take()                                                      # no transfer: the launch alone
        assert got[0] == kernel and got[2] is src and route.frame is src
    strided = torch.zeros((B, H, W, 2 * C), dtype=torch.uint8)[..., ::2]          # rows that are no contiguous blocks
    other_dtype = torch.zeros((B, H, W, C), dtype=torch.float32)
    other_shape = torch.zeros((B, C, H, W), dtype=torch.uint8)
    for src in (strided.as_subclass(_OnDevice), other_dtype.as_subclass(_OnDevice), other_shape.as_subclass(_OnDevice), tight):
        route.store(x, "obs", src, 1, calls.to_device)
        first, second = calls.take()                                               # staged, then the launch on the buffer
        assert first[0] == "to_device" and first[2] is src and first[3] == "stage"
        assert second[0] == kernel and second[2] == "stage" and route.frame is route.stage


def test_every_refusal_is_raised_by_the_plan():
    with pytest.raises(ValueError, match="device_resize"):
        _plan(device_resize=[84])
    with pytest.raises(ValueError, match="device_resize"):
        _plan(device_resize=[84, 84, 3])
    with pytest.raises(ValueError, match="at least 1"):
        _plan(device_resize=[0, 8])
    with pytest.raises(ValueError, match="device_resize_interpolation"):
        _plan(device_resize=[3, 4], device_resize_interpolation="cubic")
    with pytest.raises(ValueError, match="only shrinks"):
        _plan(device_resize=[H + 1, W])
    assert _plan(device_resize=[H + 1, W], device_resize_interpolation="nearest").keys["obs"].slab_shape == (C, H + 1, W)
    two_sizes = spaces.Dict({"obs": spaces.Box(0, 255, (3, 6, 8), np.uint8), "aux": spaces.Box(0, 255, (3, 4, 8), np.uint8)})
    with pytest.raises(ValueError, match="differ in size"):
        _plan(space=two_sizes, device_grayscale=True)
    alone = _plan(device_grayscale=True).keys["obs"]                               # grey-scale alone keeps the size
    assert alone.resize == (H, W) and alone.frame_shape == (1, H, W)
    with pytest.raises(ValueError, match="'obs'"):
        _plan(rs=True, space=_space(False, np.float32))
    with pytest.raises(ValueError, match="3 \\(R, G, B\\)"):
        _plan(rs=True, space=_space(False, shape=(4, H, W)))
    vectors = spaces.Dict({"obs": spaces.Box(-1, 1, (5,), np.float32)})
    with pytest.raises(ValueError, match="three dimensions"):
        _plan(hwc=True, space=vectors)
    with pytest.raises(ValueError, match="three dimensions"):
        _plan(k=2, space=vectors)
    with pytest.raises(ValueError, match="three"):
        _plan(rs=True, space=vectors)
    with pytest.raises(ValueError, match="device_framestack=0"):
        _plan(k=0)
    for flags, advice in ((dict(hwc=True), "hwc_observations with a zero-copy env.*step_into.*write CHW there"),
                          (dict(rs=True), "device_resize / device_grayscale with a zero-copy env.*step_into.*preprocess inside"),
                          (dict(device_grayscale=True), "device_resize / device_grayscale with a zero-copy env.*step_into"),
                          (dict(k=2), "device_framestack=2 with a zero-copy env.*step_into.*stack inside the env")):
        with pytest.raises(NotImplementedError, match=advice):
            _plan(zero_copy=True, **flags)


def test_the_identity_plan_leaves_the_env_info_as_it_is():
    from sample_factory_amd.algo.utils.env_info import EnvInfo, with_device_ingest
    space = _space(False)
    plan = _plan(zero_copy=True, space=space)
    assert plan.identity and plan.slab_obs_space() is space
    assert all(key.slab_shape == key.native_shape == space[name].shape for name, key in plan.keys.items())
    info = EnvInfo(space, spaces.Discrete(3), B)
    assert with_device_ingest(info, types.SimpleNamespace(step_into=lambda *a: None), _cfg()) is info
    assert with_device_ingest(info, types.SimpleNamespace(), _cfg()) is info
    bare = _plan(space=spaces.Box(0, 255, (C, H, W), np.uint8), k=K)               # a bare Box is the key "obs"
    assert list(bare.keys) == ["obs"] and bare.keys["obs"].slab_shape == (K * C, H, W) and not bare.identity


def test_double_stacking_is_warned_about_once(monkeypatch):
    from sample_factory_amd.algo.sampling import obs_ingest
    from sample_factory_amd.utils import utils
    seen = []
    monkeypatch.setattr(obs_ingest, "_framestack_warned", False)
    monkeypatch.setattr(utils.log, "warning", lambda *a, **kw: seen.append(a))
    _plan(k=1, env_framestack=4)
    assert not seen
    _plan(k=K, env_framestack=4)
    _plan(k=K, env_framestack=4)
    assert len(seen) == 1 and "env_framestack" in seen[0][0]


def test_importing_the_plan_does_not_load_the_library():
    import subprocess
    code = ("import sample_factory_amd.algo.sampling.obs_ingest as m, sample_factory_amd.lib as lib; "
            "assert lib._lib is None; print('ok')")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_pitch():
    from sample_factory_amd.lib import _pitch
    one = torch.zeros(8, dtype=torch.float32)
    assert _pitch(one.expand(1, 8), 1, 32) == 32                               # one row, stride 0: its row
    assert _pitch(torch.zeros(32).as_strided((1, 8), (4, 1)), 1, 32) == 32    # one row, a stride shorter than the row
    assert _pitch(torch.zeros(32).as_strided((1, 8), (20, 1)), 1, 32) == 80   # one row, a longer stride is kept
    rows = torch.zeros(3, 2, 8, dtype=torch.float32)[:, 0]
    assert _pitch(rows, 3, 32) == 64 and _pitch(rows, 3, 1000) == 64       # several rows: the stride, whatever the row
    assert _pitch(torch.zeros(3, 5, dtype=torch.uint8), 3, 5) == 5            # in bytes of the tensor's own dtype
