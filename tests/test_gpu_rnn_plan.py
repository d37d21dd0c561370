"""The launch plan of the fused recurrent passes and its name query (sf_rnn_seq_kernel_name, csrc/sf_rnn.hip).

Every instantiation the plan can select is pinned by name at the smallest chunk count that selects it, run through the
public wrappers under lib.PROFILE (whose keys must carry the name the query gave) and checked against the float64 loop of
tests/test_gpu_rnn_wideseq.py with that file's bound.  The key tuples are compared with literal ones; the query refuses what
the entry points refuse; lib.rnn_seq_family agrees with the three *_supported queries, and the model files the family it
names.  The literal names hold for 256 CUs and the default switches; elsewhere only they are suspended."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests.test_gpu_rnn_wideseq import (_model_runs, case, check_against_float64, make_inputs, run_fused,  # noqa: E402
                                        run_per_step, slab_rows, truth_fp64)

GRU, LSTM = 0, 1
KIND = ("gru", "lstm")
PERSISTENT, ROW_OWNED, WIDE = 0, 1, 2  # `family` of sf_rnn_seq_kernel_name
R = 2
# switches that do not touch the dispatch; any other SF_* variable in the environment suspends the name asserts
NOT_DISPATCH = {"SF_HIP_LIB", "SF_FUZZ_SEED", "SF_FUZZ_CASES", "SF_LAUNCH_PROGRAMS"}
DEFAULT_SWITCHES = not any(k.startswith("SF_") and k not in NOT_DISPATCH for k in os.environ)


@pytest.fixture(scope="module")
def lib():
    from sample_factory_amd import lib as L
    L.load()
    return L


def names_pinned():
    return DEFAULT_SWITCHES and torch.cuda.get_device_properties(0).multi_processor_count == 256


def profiled(lib, fn):
    """fn() under lib.PROFILE = {}: (its result, the profile's keys in launch order)"""
    lib.PROFILE = {}
    try:
        res = fn()
        torch.cuda.synchronize()
        return res, list(lib.PROFILE)
    finally:
        lib.PROFILE = None


def check_names(lib, family, kind, Cn, H, want_fwd, want_bwd, keys, ops, Kx=0):
    """the query's names are the literals (where pinned) and the names in the profile keys of the two launches"""
    fwd = lib.rnn_seq_kernel_name(family, kind, 0, Cn, H, Kx)
    bwd = lib.rnn_seq_kernel_name(family, kind, 1, Cn, H)
    print(f"family={family} kind={kind} Cn={Cn} H={H} Kx={Kx}: {fwd} | {bwd}")
    if names_pinned():
        assert (fwd, bwd) == (want_fwd, want_bwd)
    if keys is not None:
        assert [(k[0], k[-1]) for k in keys] == [(ops[0], fwd), (ops[1], bwd)], keys


# Cn -> (forward instantiation, backward kernel and instantiation): the smallest chunk counts at which the plan changes
PERSISTENT_ROWS = {16: ("16, 1, 0", "_r<{H}, 2>"), 513: ("16, 2, 0", "_r<{H}, 4>"), 1025: ("16, 4, 0", "<{H}, 16, 4>")}


@pytest.mark.parametrize("Cn", sorted(PERSISTENT_ROWS))
@pytest.mark.parametrize("H", [256, 512])
@pytest.mark.parametrize("kind", [GRU, LSTM])
def test_roster_persistent(lib, kind, H, Cn):
    """1, 2 and 3 sub-tiles (3 runs the 4-sub-tile instantiation); the register-resident backward up to 1024 rows, the LDS one
    beyond"""
    fwd, bwd = PERSISTENT_ROWS[Cn]
    x, truth, step, _ = case(lib, kind, H, Cn, R)
    (new, _), keys = profiled(lib, lambda: run_fused(lib, kind, H, Cn, x))
    check_names(lib, PERSISTENT, kind, Cn, H, f"k_{KIND[kind]}_seq_fwd<{H}, {fwd}>", f"k_{KIND[kind]}_seq_bwd" + bwd.format(H=H),
                keys, (f"{KIND[kind]}_fwd", f"{KIND[kind]}_bwd"))
    check_against_float64(f"kind={kind} H={H} Cn={Cn}", truth, step, new)


@pytest.mark.parametrize("H", [256, 512])
@pytest.mark.parametrize("kind", [GRU, LSTM])
def test_roster_first_slab_names_a_call_of_two_slabs(lib, kind, H):
    """name only (test_slabs_at_256_and_512_equal_stand_alone_calls has the numbers): a call of slab + 37 rows is named as a call
    of `slab` rows"""
    slab = max(slab_rows(lib, kind, H))
    names = [lib.rnn_seq_kernel_name(PERSISTENT, kind, p, slab + 37, H) for p in (0, 1)]
    assert names == [lib.rnn_seq_kernel_name(PERSISTENT, kind, p, slab, H) for p in (0, 1)]
    if names_pinned():
        assert names == [f"k_{KIND[kind]}_seq_fwd<{H}, 16, 4, 0>", f"k_{KIND[kind]}_seq_bwd<{H}, 16, 4>"]


@pytest.mark.parametrize("Cn,nsub", [(16, 1), (513, 2)])
@pytest.mark.parametrize("H", [256, 512])
@pytest.mark.parametrize("kind", [GRU, LSTM])
def test_roster_persistent_with_input_projection(lib, kind, H, Cn, nsub):
    """Kx = 64: the pass forms gx = x W_ih^T + b_ih itself.  The gx form, fed with the float64 projection rounded to f32, meets
    the float64 bound; the x form equals it within the bound of test_fused_sequence_forward_with_input_projection"""
    G, Kx = (4 if kind else 3), 64
    assert lib.seq_fwd_x_supported(Cn, H, Kx)
    x = make_inputs(kind, H, Cn, R, seed=7000 + 1000 * kind + 10 * H + Cn)
    g = torch.Generator().manual_seed(Cn + H + G)
    xin = torch.randn((R, Cn, Kx), generator=g)
    wih = torch.randn((G * H, Kx), generator=g) / np.sqrt(Kx)
    bih = torch.randn((G * H,), generator=g) * 0.1
    x["gx"] = (xin.double() @ wih.double().t() + bih.double()).float()
    gxf, _ = run_fused(lib, kind, H, Cn, x)
    check_against_float64(f"kind={kind} H={H} Cn={Cn} gx form", truth_fp64(kind, H, x), run_per_step(lib, kind, H, Cn, x), gxf)
    d = lambda t: t.cuda().contiguous()
    z = lambda *s: torch.zeros(s, device="cuda")
    sync = torch.zeros(192, dtype=torch.int32, device="cuda")
    got = dict(gates=z(R, Cn, 4 * H), hprev=z(R + 1, Cn, H), hout=z(R, Cn, H))
    got["hprev"][0] = d(x["h0"])
    if kind:
        got.update(cprev=z(R + 1, Cn, H), cout=z(R, Cn, H))
        got["cprev"][0] = d(x["c0"])

    def fwd_x():
        lib.rnn_seq_fwd("persistent", kind, None, d(x["whh"]), d(x["bhh"]), d(x["keep"]), got["gates"], got["hprev"], got["hout"],
                        got.get("cprev"), got.get("cout"), sync, R, Cn, H, x=d(xin), wih_t=d(wih), bih=d(bih))
    _, keys = profiled(lib, fwd_x)
    assert int(sync[128]) == 0, "the forward pass aborted"
    name = lib.rnn_seq_kernel_name(PERSISTENT, kind, 0, Cn, H, Kx)
    if names_pinned():
        assert name == f"k_{KIND[kind]}_seq_fwd<{H}, 16, {nsub}, 4>"
    assert keys == [(f"{KIND[kind]}_fwd", R * Cn, H + Kx, 1, 1, G * H, 1, 1, 1, 1, name)]
    for k, v in got.items():
        np.testing.assert_allclose(v.cpu().numpy(), gxf[k].cpu().numpy(), atol=4e-6, rtol=2e-5, err_msg=k)
    if names_pinned():  # three sub-tiles: no instantiation with the projection, the query fails as the entry point does
        assert not lib.seq_fwd_x_supported(1025, H, Kx)
        with pytest.raises(lib.SfHipError, match="unsupported"):
            lib.rnn_seq_kernel_name(PERSISTENT, kind, 0, 1025, H, Kx)


def run_row_owned(lib, kind, H, Cn, x):
    """the two row-owned launches through the routers, time-major"""
    G = 4 if kind else 3
    d = lambda t: t.cuda().contiguous()
    z = lambda *s: torch.zeros(s, device="cuda")
    gates, hprev, hout = z(R, Cn, 4 * H), z(R + 1, Cn, H), z(R, Cn, H)
    cprev, cout = (z(R + 1, Cn, H), z(R, Cn, H)) if kind else (None, None)
    hprev[0] = d(x["h0"])
    if kind:
        cprev[0] = d(x["c0"])
    whh, keep = d(x["whh"]), d(x["keep"])
    lib.rnn_seq_fwd("row_owned", kind, d(x["gx"]), whh, d(x["bhh"]), keep, gates, hprev, hout, cprev, cout, None, R, Cn, H)
    dgx = z(R, Cn, G * H)
    dgh = z(R, Cn, G * H) if kind == GRU else None
    lib.rnn_seq_bwd("row_owned", kind, d(x["dout"]), gates, hprev, cprev, cout, keep, whh, dgx, dgh, None, R, Cn, H)
    res = dict(gates=gates, hout=hout, hprev=hprev, dgx=dgx, dgh=dgh if kind == GRU else dgx)
    if kind:
        res.update(cout=cout, cprev=cprev)
    return res


@pytest.mark.parametrize("H", [32, 64, 128])
@pytest.mark.parametrize("kind", [GRU, LSTM])
def test_roster_row_owned(lib, kind, H):
    Cn = 37
    x = make_inputs(kind, H, Cn, R, seed=1000 * kind + 10 * H + Cn)
    new, keys = profiled(lib, lambda: run_row_owned(lib, kind, H, Cn, x))
    check_names(lib, ROW_OWNED, kind, Cn, H, f"k_rowseq_fwd<{kind}, {H}>", f"k_rowseq_bwd<{kind}, {H}>", keys, ("rowseq_fwd", "rowseq_bwd"))
    check_against_float64(f"kind={kind} H={H} Cn={Cn}", truth_fp64(kind, H, x), run_per_step(lib, kind, H, Cn, x), new)


@pytest.mark.parametrize("Cn,nsub", [(16, 1), (129, 2), (257, 4)])
@pytest.mark.parametrize("kind", [GRU, LSTM])
def test_roster_wide(lib, kind, Cn, nsub):
    """two row groups of 128 work-groups on 256 CUs: 1, 2 and 3 sub-tiles"""
    x, truth, step, _ = case(lib, kind, 1024, Cn, R)
    (new, _), keys = profiled(lib, lambda: run_fused(lib, kind, 1024, Cn, x))
    check_names(lib, WIDE, kind, Cn, 1024, f"k_wideseq_fwd<{kind}, {nsub}>", f"k_wideseq_bwd<{kind}, {nsub}>", keys,
                ("wideseq_fwd", "wideseq_bwd"))
    check_against_float64(f"kind={kind} H=1024 Cn={Cn}", truth, step, new)


# (op, family, kind, pass, Cn, H, steps, x_cols) -> the key: rows = steps * Cn (forward R steps, backward R - 1), K = H + x_cols,
# N = G * H
KEYS = [
    (("lstm_fwd", PERSISTENT, LSTM, 0, 513, 512, R, 0), ("lstm_fwd", 1026, 512, 1, 1, 2048, 1, 1, 1, 1, "k_lstm_seq_fwd<512, 16, 2, 0>")),
    (("gru_bwd", PERSISTENT, GRU, 1, 16, 256, R - 1, 0), ("gru_bwd", 16, 256, 1, 1, 768, 1, 1, 1, 1, "k_gru_seq_bwd_r<256, 2>")),
    (("lstm_bwd", PERSISTENT, LSTM, 1, 1025, 512, R - 1, 0), ("lstm_bwd", 1025, 512, 1, 1, 2048, 1, 1, 1, 1, "k_lstm_seq_bwd<512, 16, 4>")),
    (("gru_fwd", PERSISTENT, GRU, 0, 16, 512, R, 64), ("gru_fwd", 32, 576, 1, 1, 1536, 1, 1, 1, 1, "k_gru_seq_fwd<512, 16, 1, 4>")),
    (("gru_fwd", PERSISTENT, GRU, 0, 2085, 256, R, 0), ("gru_fwd", 4170, 256, 1, 1, 768, 1, 1, 1, 1, "k_gru_seq_fwd<256, 16, 4, 0>")),
    (("rowseq_fwd", ROW_OWNED, GRU, 0, 37, 64, R, 0), ("rowseq_fwd", 74, 64, 1, 1, 192, 1, 1, 1, 1, "k_rowseq_fwd<0, 64>")),
    (("rowseq_bwd", ROW_OWNED, LSTM, 1, 37, 128, R - 1, 0), ("rowseq_bwd", 37, 128, 1, 1, 512, 1, 1, 1, 1, "k_rowseq_bwd<1, 128>")),
    (("wideseq_fwd", WIDE, GRU, 0, 257, 1024, R, 0), ("wideseq_fwd", 514, 1024, 1, 1, 3072, 1, 1, 1, 1, "k_wideseq_fwd<0, 4>")),
    (("wideseq_bwd", WIDE, LSTM, 1, 129, 1024, R - 1, 0), ("wideseq_bwd", 129, 1024, 1, 1, 4096, 1, 1, 1, 1, "k_wideseq_bwd<1, 2>")),
]


@pytest.mark.parametrize("args,want", KEYS, ids=[f"{a[0]}-{a[4]}-{a[5]}-{a[7]}" for a, _ in KEYS])
def test_key_layout_is_unchanged(lib, args, want):
    """the tuples bench.py's profile and the kernel-stats tables are keyed by; no key (and no library call) unless one is wanted"""
    assert lib.PROFILE is None and lib._rnn_key(*args) is None
    key, _ = profiled(lib, lambda: lib._rnn_key(*args))
    assert key[:-1] == want[:-1]
    if names_pinned():
        assert key == want


def test_the_query_refuses_what_the_entry_points_refuse(lib):
    L = lib.load()
    import ctypes as C
    buf = C.create_string_buffer(96)
    bad = [(f, k, p, 64, 96, 0) for f in (PERSISTENT, ROW_OWNED, WIDE) for k in (GRU, LSTM) for p in (0, 1)]  # H = 96
    bad += [(PERSISTENT, 2, 0, 64, 512, 0), (ROW_OWNED, 2, 1, 64, 64, 0), (WIDE, 2, 0, 64, 1024, 0)]           # kind = 2
    bad += [(PERSISTENT, LSTM, 0, 0, 512, 0), (ROW_OWNED, GRU, 0, 0, 64, 0), (WIDE, GRU, 1, 0, 1024, 0)]       # Cn = 0
    bad += [(PERSISTENT, LSTM, 0, 64, 512, 32), (PERSISTENT, GRU, 0, 64, 256, 32)]                             # Kx = 32
    bad += [(3, GRU, 0, 64, 512, 0), (3, LSTM, 1, 64, 64, 0), (-1, GRU, 0, 64, 1024, 0)]                       # family = 3
    bad += [(PERSISTENT, LSTM, 1, 64, 512, 64), (ROW_OWNED, GRU, 0, 64, 64, 64), (WIDE, GRU, 0, 64, 1024, 64),  # no x form there
            (PERSISTENT, LSTM, 0, 64, 1024, 0), (WIDE, LSTM, 0, 64, 512, 0), (ROW_OWNED, LSTM, 0, 64, 256, 0)]  # another family's width
    for a in bad:
        buf.value = b""
        assert L.sf_rnn_seq_kernel_name(*a, buf, 96) != 0, a
        msg = L.sf_last_error().decode()
        assert msg.startswith("sf_rnn_seq_kernel_name:") and buf.value == b"", (a, msg)
        with pytest.raises(lib.SfHipError, match="sf_rnn_seq_kernel_name"):
            lib.rnn_seq_kernel_name(*a)
    assert L.sf_rnn_seq_kernel_name(PERSISTENT, GRU, 0, 64, 512, 0, buf, 8) != 0  # no room for a name
    assert L.sf_rnn_seq_kernel_name(PERSISTENT, GRU, 0, 64, 512, 0, buf, 96) == 0 and buf.value.startswith(b"k_gru_seq_fwd<512, 16, ")


def test_family_agrees_with_the_supported_queries(lib):
    for kind in (GRU, LSTM):
        for H in (32, 64, 96, 128, 256, 512, 1000, 1024, 2048):
            for Cn in (-1, 0, 1, 64, 65, 512, 513, 2048, 2049, 100000):
                want = ("persistent" if lib.lstm_seq_supported(Cn, H) else "row_owned" if lib.rnn_rowseq_supported(kind, Cn, H) else
                        "persistent_wide" if lib.rnn_wideseq_supported(kind, Cn, H) else None)
                assert lib.rnn_seq_family(kind, Cn, H) == want, (kind, Cn, H)
                if want is not None:  # an offered shape has a plan and a name
                    fam = lib.RNN_FAMILIES.index(want)
                    assert all(lib.rnn_seq_kernel_name(fam, kind, p, Cn, H).startswith("k_") for p in (0, 1))
    assert lib.rnn_seq_family(GRU, 24, 64) == "row_owned" and lib.rnn_seq_family(LSTM, 24, 256) == "persistent"
    assert lib.rnn_seq_family(GRU, 24, 1024) == "persistent_wide" and lib.rnn_seq_family(GRU, 24, 96) is None


@pytest.mark.parametrize("H", [64, 256, 1024])
def test_model_files_the_family_the_library_names(lib, H, monkeypatch):
    """ActorCritic on Box(24,) observations, GRU, recurrence 4, 24 chunks: _rnn_saved names lib.rnn_seq_family's family with the
    fused passes on and "per_step" with them off (asserted inside _model_runs, which also runs the backward pass)"""
    family = lib.rnn_seq_family(GRU, 24, H)
    assert family == {64: "row_owned", 256: "persistent", 1024: "persistent_wide"}[H]
    runs = _model_runs(lib, monkeypatch, "gru", H, 1, 4, 24, family)
    assert set(runs) == {True, False}
