"""sf_episode_stats_add (include/sf_hip.h) against NumPy float64.

Every value is a multiple of 1/8 in [-64, 64] (integers and bytes: integers in that range), the accumulators start at a
sentinel that is a multiple of 1/8 too, and no sum here exceeds 2^15: every float64 partial sum is exact in any order, so
sums and counts are compared with ==.  That is not a tolerance.

Shapes: B = 259 is one full 256-lane block plus a partial wave of a second one, B = 64 one wave, B = 1 one lane.  K = 17
goes through the wrapper as two launches (16 + 1).  Every dtype code and a channel with element stride 3 are in every
case with K >= 6."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = 1000.125, -77.5
DTYPES = [torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8, torch.bool]


def _channel(rng, B, k):
    """(the tensor that owns the memory, the 1-d device view handed over, its float64 host values); channels 5 and 12 of a
    case are the middle column of a [B, 3] matrix: element stride 3"""
    dt = DTYPES[k % len(DTYPES)]
    strided = k == 5 or k == 12
    shape = (B, 3) if strided else (B,)
    if dt in (torch.float32, torch.float64):
        host = rng.integers(-512, 513, shape) / 8.0
    elif dt == torch.bool:
        host = rng.integers(0, 2, shape)
    elif dt == torch.uint8:
        host = rng.integers(0, 65, shape)
    else:
        host = rng.integers(-64, 65, shape)
    full = torch.from_numpy(np.asarray(host)).to(dt).cuda()
    if strided:  # (channel 5 is bool, channel 12 f32)
        view = full[:, 1]
        assert view.stride(0) == 3
        return full, view, np.asarray(host)[:, 1].astype(np.float64)
    return full, full, np.asarray(host).astype(np.float64)


def _masks(rng, B, kind):
    if kind == "none":
        term, trunc = np.zeros(B, bool), np.zeros(B, bool)
    elif kind == "all":
        term, trunc = np.ones(B, bool), rng.random(B) < 0.5
    else:  # random, overlapping: some rows carry both flags, some one, some none
        term, trunc = rng.random(B) < 0.4, rng.random(B) < 0.4
        if B >= 64:
            assert (term & trunc).any() and (term & ~trunc).any() and (~term & trunc).any() and (~term & ~trunc).any()
    return term, trunc


def _run_case(B, K, kind, with_active, seed, trunc_dtype=torch.bool):
    from sample_factory_amd import lib
    rng = np.random.default_rng(seed)
    chans = [_channel(rng, B, k) for k in range(K)]
    term, trunc = _masks(rng, B, kind)
    active = (rng.random(B) < 0.6) if with_active else None
    d_term = torch.from_numpy(term).cuda()
    d_trunc = torch.from_numpy(trunc).to(trunc_dtype).cuda()
    d_active = torch.from_numpy(active).cuda() if with_active else None
    buf = torch.full((2 * K + 8,), GUARD, dtype=torch.float64, device="cuda")
    acc = buf[:2 * K].view(K, 2)
    acc.fill_(SENTINEL)
    before = [c[0].clone() for c in chans]
    lib.episode_stats_add([c[1] for c in chans], d_term, d_trunc, d_active, acc)
    torch.cuda.synchronize()
    fin = term | trunc
    if with_active:
        fin = fin & active
    want = np.empty((K, 2))
    for k, (_, _, host) in enumerate(chans):
        want[k] = SENTINEL + host[fin].sum(dtype=np.float64), SENTINEL + fin.sum()
    got = acc.cpu().numpy()
    assert np.array_equal(got, want), (B, K, kind, with_active, np.argwhere(got != want)[:4], got[got != want][:4],
                                       want[got != want][:4])
    assert (buf[2 * K:] == GUARD).all(), "the call wrote behind acc"
    for (full, _, _), b4 in zip(chans, before):
        assert torch.equal(full, b4)
    assert np.array_equal(d_term.cpu().numpy(), term) and np.array_equal(d_trunc.cpu().numpy().astype(bool), trunc)
    if with_active:
        assert np.array_equal(d_active.cpu().numpy(), active)
    return int(fin.sum())


@pytest.mark.parametrize("with_active", [False, True], ids=["no_active", "active"])
@pytest.mark.parametrize("kind", ["none", "all", "random"])
@pytest.mark.parametrize("B", [1, 64, 259])
def test_every_dtype_and_a_strided_channel_k17(B, kind, with_active):
    n = _run_case(B, 17, kind, with_active, seed=B * 7 + len(kind))
    if kind == "none":
        assert n == 0
    if kind == "all" and not with_active:
        assert n == B


@pytest.mark.parametrize("K", [1, 3, 16])
def test_channel_counts_one_launch(K, monkeypatch):
    from sample_factory_amd import lib
    calls = []
    real = lib.load().sf_episode_stats_add

    class Spy:
        def __getattr__(self, name):
            fn = getattr(lib._lib, name)
            if name != "sf_episode_stats_add":
                return fn
            return lambda *a: (calls.append(a[1]), fn(*a))[1]
    assert real is not None
    monkeypatch.setattr(lib, "load", lambda: Spy())
    _run_case(259, K, "random", False, seed=K)
    _run_case(259, K, "random", True, seed=K + 100, trunc_dtype=torch.uint8)
    assert calls == [K, K]


def test_seventeen_channels_are_two_launches(monkeypatch):
    from sample_factory_amd import lib
    calls = []
    lib.load()

    class Spy:
        def __getattr__(self, name):
            fn = getattr(lib._lib, name)
            if name != "sf_episode_stats_add":
                return fn
            return lambda *a: (calls.append(a[1]), fn(*a))[1]
    monkeypatch.setattr(lib, "load", lambda: Spy())
    _run_case(259, 17, "random", True, seed=5)
    assert calls == [16, 1]


def test_the_call_adds_twice_and_replays_from_a_launch_program():
    """two calls add twice (nothing is zeroed); recorded in a lib.LaunchProgram it replays on the same addresses"""
    from sample_factory_amd import lib
    B = 259
    rng = np.random.default_rng(3)
    vals = rng.integers(-512, 513, B) / 8.0
    term = rng.random(B) < 0.5
    x = torch.from_numpy(vals).float().cuda()
    d_term, d_trunc = torch.from_numpy(term).cuda(), torch.zeros(B, dtype=torch.bool, device="cuda")
    acc = torch.zeros((1, 2), dtype=torch.float64, device="cuda")
    lib.episode_stats_add([x], d_term, d_trunc, None, acc)
    with lib.record_launches() as prog:
        lib.episode_stats_add([x], d_term, d_trunc, None, acc)
    assert prog.unsafe is None and [c[2] for c in prog.calls] == ["sf_episode_stats_add"]
    prog.replay()
    # a replay reads the CURRENT contents of the recorded addresses
    term2 = ~term
    d_term.copy_(torch.from_numpy(term2).cuda())
    prog.replay()
    torch.cuda.synchronize()
    want = [3 * vals[term].sum() + vals[term2].sum(), 3 * term.sum() + term2.sum()]
    assert acc.cpu().numpy().tolist() == [want]


def test_refusals_launch_nothing():
    from sample_factory_amd import lib
    L = lib.load()
    B = 64
    x = torch.ones(B, dtype=torch.float32, device="cuda")
    ones = torch.ones(B, dtype=torch.bool, device="cuda")
    acc = torch.full((4,), SENTINEL, dtype=torch.float64, device="cuda")

    def chans(n=1, stride=1, dtype=lib.EPSTAT_F32, ptr=None):
        ch = lib.sf_epstat_channels()
        for k in range(n):
            ch.ptr[k], ch.stride[k], ch.dtype[k] = (x.data_ptr() if ptr is None else ptr), stride, dtype
        return ch

    def call(ch, K, term=ones, trunc=ones, B_=B, acc_=acc):
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        return L.sf_episode_stats_add(C.byref(ch) if ch is not None else None, K, p(term), p(trunc), None, C.c_int64(B_),
                                      p(acc_), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    bad = [call(chans(), 0), call(chans(16), 17), call(chans(), -1), call(None, 1), call(chans(), 1, term=None),
           call(chans(), 1, trunc=None), call(chans(), 1, acc_=None), call(chans(), 1, B_=-1), call(chans(1), 2),
           call(chans(ptr=0), 1), call(chans(stride=0), 1), call(chans(stride=-3), 1), call(chans(dtype=5), 1),
           call(chans(dtype=-1), 1), call(chans(dtype=99), 1, B_=0)]
    assert bad == [-1] * len(bad), bad
    assert b"sf_episode_stats_add" in L.sf_last_error()
    assert call(chans(), 1, B_=0) == 0  # SF_OK, nothing launched
    torch.cuda.synchronize()
    assert (acc == SENTINEL).all(), "a refused call (or B == 0) touched acc"
    assert call(chans(2), 2) == 0      # the same arguments, valid: both channels add
    torch.cuda.synchronize()
    assert acc.cpu().numpy().tolist() == [SENTINEL + B] * 4
    # the wrapper refuses what it can see
    for args in (([], ones, ones, None, acc.view(2, 2)), ([x], ones, ones, None, acc.view(2, 2)),
                 ([x.cpu()], ones, ones, None, acc[:2].view(1, 2)), ([x[:8]], ones, ones, None, acc[:2].view(1, 2)),
                 ([x.half()], ones, ones, None, acc[:2].view(1, 2)), ([x], ones, ones[:8], None, acc[:2].view(1, 2))):
        with pytest.raises(lib.SfHipError):
            lib.episode_stats_add(*args)
