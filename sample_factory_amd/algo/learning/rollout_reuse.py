"""Reuse of the rollout's conv activations by the first SGD step: the decision, as a pure function.

In synchronous mode the rollout runs conv1 -> conv2 -> conv3 on obs[:, t] with the learner's own weights, and the first
minibatch of the first epoch — dataset rows [0, batch_size) when minibatches are not shuffled — runs the same layers on the
same frames with the same weights before the first optimiser step.  The rollout therefore writes those activations into
kept buffers laid out [keep_rows, T, pixels, channels] (row e * T + t = dataset row e * T + t; keep_rows = the trajectories
of minibatch 0, the others are written densely as without reuse) and the training forward resumes behind them.  Everything here is host bookkeeping; nothing in this module touches the device.
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Sequence, Tuple


class SlotRecord(NamedTuple):
    """what one rollout step left in slot t of kept rows [row0, row1)"""
    row0: int
    row1: int
    t: int
    generation: int   # the model's weights generation the step ran with
    obs_ptr: int      # address of the frame of kept row `row0` at step t (the slab row the step read)


def keep_rows(batch_size: int, T: int, rows: int) -> int:
    """trajectories whose activations are kept: the whole trajectories of minibatch 0 = dataset rows [0, batch_size), at most
    the `rows` trajectories there are.  Nothing beyond them is ever read back, so nothing beyond them is kept."""
    if T <= 0 or batch_size <= 0 or rows <= 0:
        return 0
    return min(int(batch_size) // int(T), int(rows))


def keep_n(kept_rows: int, row0: int, n: int) -> int:
    """of a rollout launch over trajectories [row0, row0 + n): how many of its leading samples belong to the kept rows
    [0, kept_rows) — the split point of the two-segment forward (0: the launch keeps nothing and runs the plain forward)"""
    return max(0, min(int(n), int(kept_rows) - int(row0)))


def twin_name(dense: str) -> str:
    """name of the strided-output twin of a dense kernel instantiation: k_x<...> -> k_x_os<...>"""
    return dense.replace("<", "_os<", 1)


# tile forms of fwd_glds_body whose unsplit launches were shown to give the same bytes (tests/test_gpu_fwd_two_segment.py::
# test_fc_tile_shapes_give_the_same_bytes): one accumulator chain per output element, k in ascending 32-deep chunks
FC_SAME_BYTES_FORMS = ("k_fwd_glds_z<64, 64, 2, 2>", "k_fwd_glds_z<128, 128, 2, 2>")


def fc_reusable(name_roll: str, name_train: str, workspace_roll: int, workspace_train: int) -> bool:
    """may the fc output the rollout computed stand in for the training launch's?  The conv layers ask for the SAME kernel;
    the fc layer runs 64 x 64 tiles at the rollout size and 128 x 128 tiles at the training size, so for it the rule is: both
    launches are k_fwd_glds_z instantiations whose bytes were shown to agree, and neither is split along K (a split launch
    adds partial sums in another order; it is the launch that asks for a workspace)."""
    if workspace_roll or workspace_train:
        return False
    return name_roll in FC_SAME_BYTES_FORMS and name_train in FC_SAME_BYTES_FORMS


def reuse_prefix(*, epoch: int, batch_num: int, indexed: bool, offset: int, n: int, T: int, keep_T: int, keep_rows: int,
                 records: Dict[Tuple[int, int], SlotRecord], generation: int, obs_ptr: int, obs_row_bytes: int,
                 obs_step_bytes: int, has_normalizer: bool, has_rnn: bool, async_rl: bool, snapshot_reads: bool,
                 layer_ok: Sequence[bool]) -> Tuple[int, str]:
    """(number of leading conv layers whose kept activations the training forward of this minibatch may use, reason).

    0 unless this is epoch 0 / minibatch 0, the minibatch is the contiguous dataset rows [offset, offset + n) of whole
    trajectories of length T == keep_T, every (row, step) of them was written by a rollout step that ran with the CURRENT
    weights generation on exactly the frame the dataset holds there (obs_ptr + row * obs_row_bytes + t * obs_step_bytes), and
    the model and mode have nothing between the frames and conv1 (normaliser), no recurrence, no second set of weights.
    layer_ok[i]: layer i's rollout launch and training launch run the same kernel with no split reduction; the layers are
    reused as a prefix, the first False ends it."""
    if epoch != 0 or batch_num != 0:
        return 0, "not the first minibatch"
    if indexed:
        return 0, "minibatch gathered through an index"
    if async_rl or snapshot_reads:
        return 0, "the rollout does not read the learner's weights"
    if has_normalizer or has_rnn:
        return 0, "normaliser or recurrent core"
    if keep_T <= 0 or T != keep_T:
        return 0, "trajectory length differs from the kept one"
    if n <= 0 or offset % T or n % T:
        return 0, "minibatch does not consist of whole trajectories"
    e0, e1 = offset // T, (offset + n) // T
    if e1 > keep_rows:
        return 0, "rows beyond the kept buffer"
    for t in range(T):
        covered = e0
        for (row0, tt), r in sorted(records.items()):
            if tt != t or r.row1 <= e0 or r.row0 >= e1:
                continue
            if r.row0 > covered:
                return 0, f"rows {covered}..{r.row0} of step {t} were never kept"
            if r.generation != generation:
                return 0, "the weights changed since the rollout"
            if r.t != t or r.obs_ptr != obs_ptr + r.row0 * obs_row_bytes + t * obs_step_bytes:
                return 0, "kept from other slab rows than this dataset's"
            covered = max(covered, r.row1)
        if covered < e1:
            return 0, f"rows {covered}..{e1} of step {t} were never kept"
    prefix = 0
    for ok in layer_ok:
        if not ok:
            break
        prefix += 1
    return prefix, "ok" if prefix else "first layer's launches differ"
