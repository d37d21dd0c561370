"""The decision to reuse the rollout's conv activations (algo/learning/rollout_reuse.py) as a pure function of its inputs."""
from sample_factory_amd.algo.learning.rollout_reuse import SlotRecord, reuse_prefix, twin_name

T, ROWS, GEN, PTR, ROW_B, STEP_B = 4, 512, 9, 4096, 5 * 28224, 28224


def _records(row_blocks=((0, 512),), gen=GEN, ptr=PTR, steps=range(T), slot_shift=0):
    return {(r0, t): SlotRecord(r0, r1, t + slot_shift, gen, ptr + r0 * ROW_B + t * STEP_B) for r0, r1 in row_blocks for t in steps}


def _decide(**over):
    kw = dict(epoch=0, batch_num=0, indexed=False, offset=0, n=1024, T=T, keep_T=T, keep_rows=ROWS, records=_records(),
              generation=GEN, obs_ptr=PTR, obs_row_bytes=ROW_B, obs_step_bytes=STEP_B, has_normalizer=False, has_rnn=False,
              async_rl=False, snapshot_reads=False, layer_ok=[True, True, True])
    kw.update(over)
    return reuse_prefix(**kw)[0]


def test_reuses_the_first_minibatch():
    assert _decide() == 3
    assert _decide(offset=1024, n=1024) == 3  # (any whole-trajectory range of the first minibatch that the slots cover)
    assert _decide(records=_records(((0, 256), (256, 512))), n=2048) == 3  # two env instances: row offsets


def test_layers_are_a_prefix():
    assert _decide(layer_ok=[True, True, False]) == 2
    assert _decide(layer_ok=[True, False, True]) == 1
    assert _decide(layer_ok=[False, True, True]) == 0
    assert _decide(layer_ok=[]) == 0


def test_every_condition_is_needed():
    assert _decide(epoch=1) == 0 and _decide(batch_num=1) == 0
    assert _decide(indexed=True) == 0
    assert _decide(async_rl=True) == 0 and _decide(snapshot_reads=True) == 0
    assert _decide(has_normalizer=True) == 0 and _decide(has_rnn=True) == 0
    assert _decide(T=8) == 0 and _decide(keep_T=0) == 0
    assert _decide(offset=2) == 0 and _decide(n=1022) == 0 and _decide(n=0) == 0
    assert _decide(offset=1024, n=2048) == 0                       # rows beyond the kept buffer
    assert _decide(generation=GEN + 1) == 0                        # the weights changed since the rollout
    assert _decide(records=_records(gen=GEN - 1)) == 0
    assert _decide(obs_ptr=PTR + 512 * ROW_B) == 0                 # kept from another sampling round's slab rows
    assert _decide(records=_records(steps=range(T - 1))) == 0      # a step that was never kept
    assert _decide(records=_records(((0, 256),)), n=2048) == 0     # rows that were never kept
    assert _decide(records=_records(((0, 256), (300, 512))), n=2048) == 0  # a hole between two instances
    assert _decide(records=_records(slot_shift=1)) == 0            # written into another slot than its step's
    assert _decide(records={}) == 0


def test_a_stale_block_outside_the_minibatch_does_not_matter():
    recs = _records(((0, 256),))
    recs.update(_records(((256, 512),), gen=GEN - 3))
    assert _decide(records=recs, n=1024) == 3 and _decide(records=recs, n=2048) == 0


def test_twin_name():
    assert twin_name("k_fwd_img<64, 9, 9, 3, 1, 2, 1, 7>") == "k_fwd_img_os<64, 9, 9, 3, 1, 2, 1, 7>"
    assert twin_name("k_conv1_u8_bf16_w<false>") == "k_conv1_u8_bf16_w_os<false>"
