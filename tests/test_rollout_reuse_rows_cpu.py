"""Which trajectories the rollout keeps for the first SGD step, and where a rollout launch is split (algo/learning/
rollout_reuse.py: keep_rows, keep_n), as pure functions; and the guard refusing a minibatch that reaches beyond them."""
from sample_factory_amd.algo.learning.rollout_reuse import SlotRecord, fc_reusable, keep_n, keep_rows, reuse_prefix

T, GEN, PTR, ROW_B, STEP_B = 4, 9, 4096, 5 * 28224, 28224


def test_keep_rows():
    assert keep_rows(32768, 32, 4096) == 1024   # the headline workload: a quarter of the trajectories
    assert keep_rows(1024, 4, 256) == 256       # one minibatch is the whole dataset
    assert keep_rows(4096, 4, 256) == 256       # never more than there are
    assert keep_rows(256, 4, 256) == 64
    assert keep_rows(130, 4, 256) == 32         # whole trajectories only
    assert keep_rows(2, 4, 256) == 0 and keep_rows(256, 0, 256) == 0 and keep_rows(0, 4, 256) == 0


def test_keep_n():
    assert keep_n(1024, 0, 4096) == 1024                              # straddling: the launch is split
    assert keep_n(64, 0, 256) == 64
    assert keep_n(512, 0, 256) == 256 and keep_n(512, 256, 256) == 256  # entirely inside minibatch 0
    assert keep_n(256, 256, 256) == 0 and keep_n(256, 512, 256) == 0  # entirely outside: the plain forward
    assert keep_n(300, 256, 256) == 44                                # the second instance straddles
    assert keep_n(0, 0, 256) == 0
    for kept in range(0, 700, 37):  # the instances' kept parts tile [0, kept) exactly
        assert sum(keep_n(kept, r0, 256) for r0 in (0, 256, 512)) == min(kept, 768)


def _decide(keep, n, blocks):
    recs = {(r0, t): SlotRecord(r0, r1, t, GEN, PTR + r0 * ROW_B + t * STEP_B) for r0, r1 in blocks for t in range(T)}
    return reuse_prefix(epoch=0, batch_num=0, indexed=False, offset=0, n=n, T=T, keep_T=T, keep_rows=keep, records=recs,
                        generation=GEN, obs_ptr=PTR, obs_row_bytes=ROW_B, obs_step_bytes=STEP_B, has_normalizer=False,
                        has_rnn=False, async_rl=False, snapshot_reads=False, layer_ok=[True, True, True])


def test_minibatch_beyond_the_kept_rows_is_refused():
    kept = keep_rows(256, T, 256)  # 64 trajectories; the launch over rows [0, 256) records its kept part only
    blocks = [(0, keep_n(kept, 0, 256))]
    assert _decide(kept, 256, blocks) == (3, "ok")
    assert _decide(kept, 260, blocks) == (0, "rows beyond the kept buffer")
    assert _decide(kept, 1024, blocks) == (0, "rows beyond the kept buffer")
    # two instances, the second one straddling: [0, 256) + [256, 300)
    kept = 300
    blocks = [(r0, r0 + keep_n(kept, r0, 256)) for r0 in (0, 256)]
    assert blocks == [(0, 256), (256, 300)]
    assert _decide(kept, 300 * T, blocks)[0] == 3
    assert _decide(kept, 301 * T, blocks)[0] == 0
    assert _decide(kept, 300 * T, blocks[:1])[0] == 0  # the straddling instance's kept part was never written


def test_fc_guard():
    """the fc output is reused only between unsplit launches of the two tile forms whose bytes were compared"""
    small, big = "k_fwd_glds_z<64, 64, 2, 2>", "k_fwd_glds_z<128, 128, 2, 2>"
    assert fc_reusable(small, big, 0, 0) and fc_reusable(small, small, 0, 0) and fc_reusable(big, big, 0, 0)
    assert not fc_reusable(small, big, 4096, 0) and not fc_reusable(small, big, 0, 256)  # a launch split along K
    assert not fc_reusable(small, "k_fwd_glds<128, 128, 2, 2, 2>", 0, 0)                 # another kernel
    assert not fc_reusable("k_conv_fwd<128, 64, 2, 2, 0>", big, 0, 0)
    assert not fc_reusable("k_fwd_glds_z<128, 64, 2, 2>", big, 0, 0)                     # a form nobody compared
