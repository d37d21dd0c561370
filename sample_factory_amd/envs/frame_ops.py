"""Resize and grey-scale of u8 frames in NumPy: the arithmetic of sf_frame_resize (include/sf_hip.h), bit for bit.

--device_resize / --device_grayscale run it on the device; this module runs the identical preprocessing on the host (an
evaluation harness of one's own, a comparison run) and is what the tests hold the kernel against.  Integer arithmetic
only, u8 in, u8 out, vectorised over any leading batch axes:

  nearest:  out[y][x] = in[(y * H) // OH][(x * W) // OW]; any OH, OW >= 1.
  area:     the exact box average over fractional pixel coverage.  Along an axis, in units of 1 / (W * OW) of it,
            destination pixel x covers [x * W, (x + 1) * W) and source pixel s covers [s * OW, (s + 1) * OW); the weight
            wx(x, s) is the length of the overlap (the weights of one x sum to W).  S = sum wy * wx * in, D = H * W,
            out = (2 * S + D) // (2 * D): ties round half up.  Only shrinks: OH <= H and OW <= W.
  grey:     (9798 * R + 19235 * G + 3735 * B + 16384) >> 15 — ITU-R 601 luma in 15-bit fixed point — of the resized and
            rounded channels (resize first, then grey: the order of the reference's ResizeWrapper).

The area result is the exact value of what OpenCV's INTER_AREA approximates in float; it may differ from OpenCV by 1 in
the last bit on ties.

The module also holds the NumPy model of the training-time random shift (--augment_random_shift, sf_random_shift_gather;
DESIGN.md 3.17): `random_shift_draws`, `random_shift_frames` and the learner's `random_shift_seed`; and of the cutout and
intensity augmentations that ride in the same launch (--augment_cutout, --augment_intensity, sf_augment_gather; DESIGN.md
3.20): `cutout_draws`, `intensity_draws`, `intensity_frames`, `cutout_frames`, their composition `augment_frames`, and
the host's per-step op draw `augment_op_of_step` (--augment_mix one)."""
from __future__ import annotations

import numpy as np

from sample_factory_amd.envs.pixel_catch import philox

INTERPOLATIONS = ("area", "nearest")
GRAY_R, GRAY_G, GRAY_B, GRAY_SHIFT = 9798, 19235, 3735, 15


def _u8(frames) -> np.ndarray:
    a = np.asarray(frames)
    if a.dtype != np.uint8:
        raise ValueError(f"u8 frames expected, got dtype {a.dtype}")
    if a.ndim < 2:
        raise ValueError(f"frames need at least the two image axes [..., H, W], got shape {a.shape}")
    return a


def _sizes(OH, OW):
    OH, OW = int(OH), int(OW)
    if OH < 1 or OW < 1:
        raise ValueError(f"output size {OH} x {OW}: each at least 1")
    return OH, OW


def area_weights(n_src: int, n_dst: int) -> np.ndarray:
    """[n_dst, n_src] int64: the overlap of destination pixel x = [x * n_src, (x + 1) * n_src) with source pixel
    s = [s * n_dst, (s + 1) * n_dst); every row sums to n_src"""
    x, s = np.arange(n_dst, dtype=np.int64)[:, None], np.arange(n_src, dtype=np.int64)[None, :]
    return np.maximum(0, np.minimum((x + 1) * n_src, (s + 1) * n_dst) - np.maximum(x * n_src, s * n_dst))


def resize_nearest_u8(frames, OH: int, OW: int) -> np.ndarray:
    """[..., H, W] u8 -> [..., OH, OW] u8: out[y][x] = in[(y * H) // OH][(x * W) // OW]"""
    a = _u8(frames)
    OH, OW = _sizes(OH, OW)
    H, W = a.shape[-2:]
    ys, xs = (np.arange(OH, dtype=np.int64) * H) // OH, (np.arange(OW, dtype=np.int64) * W) // OW
    return np.ascontiguousarray(a[..., ys[:, None], xs[None, :]])


def resize_area_u8(frames, OH: int, OW: int) -> np.ndarray:
    """[..., H, W] u8 -> [..., OH, OW] u8: the exact box average, ties rounded half up; OH <= H and OW <= W"""
    a = _u8(frames)
    OH, OW = _sizes(OH, OW)
    H, W = a.shape[-2:]
    if OH > H or OW > W:
        raise ValueError(f"the area filter only shrinks: {H} x {W} -> {OH} x {OW}")
    S = area_weights(H, OH) @ a.astype(np.int64) @ area_weights(W, OW).T
    D = H * W
    return ((2 * S + D) // (2 * D)).astype(np.uint8)


def rgb_to_gray_u8(frames, channel_axis: int = -3) -> np.ndarray:
    """u8 frames with 3 channels (R, G, B) along `channel_axis` -> the same shape with ONE channel there"""
    a = _u8(frames)
    if a.shape[channel_axis] != 3:
        raise ValueError(f"grey-scale needs 3 channels (R, G, B) along axis {channel_axis}, got shape {a.shape}")
    r, g, b = (np.take(a, [c], axis=channel_axis).astype(np.int64) for c in range(3))
    return ((GRAY_R * r + GRAY_G * g + GRAY_B * b + (1 << (GRAY_SHIFT - 1))) >> GRAY_SHIFT).astype(np.uint8)


def preprocess_frames(frames, layout: str, OH: int, OW: int, interpolation: str = "area", grayscale: bool = False) -> np.ndarray:
    """what the device does to one batch of frames under --device_resize OH OW / --device_grayscale: frames
    [N, H, W, C] (layout "hwc") or [N, C, H, W] ("chw") u8 -> [N, C', OH, OW] u8, C' = 1 with grayscale else C"""
    a = _u8(frames)
    if a.ndim != 4 or layout not in ("hwc", "chw"):
        raise ValueError(f"frames [N, H, W, C] with layout 'hwc' or [N, C, H, W] with 'chw' expected, got {a.shape}, {layout!r}")
    if interpolation not in INTERPOLATIONS:
        raise ValueError(f"interpolation must be one of {INTERPOLATIONS}, got {interpolation!r}")
    chw = a.transpose(0, 3, 1, 2) if layout == "hwc" else a
    if grayscale and chw.shape[1] != 3:
        raise ValueError(f"grayscale needs 3 channels (R, G, B), got {chw.shape[1]}")
    out = (resize_area_u8 if interpolation == "area" else resize_nearest_u8)(chw, OH, OW)
    return np.ascontiguousarray(rgb_to_gray_u8(out, 1) if grayscale else out)


# ---- random shift (sf_random_shift_gather) ---------------------------------------------------------------------------
RANDOM_SHIFT_MAX_PAD = 255
RANDOM_SHIFT_LANE = 5  # lane 2 of the Philox counter: 0 .. 3 are taken by sf_rl.hip, 4 by sf_pixcatch.hip


def random_shift_seed(seed, policy_id: int, rank: int = 0) -> int:
    """the Philox key word the learner of `policy_id` (data-parallel replica `rank`) draws its shifts under: distinct per
    run seed, policy and replica, 32 bits"""
    return (((int(seed or 0) * 7919 + int(policy_id)) * 1000003 + int(rank)) * 2654435761 + 1) & 0xFFFFFFFF


def random_shift_draws(seed: int, draw_id: int, groups, pad: int):
    """(dy, dx) int32 arrays, one pair per entry of `groups`, each in [0, 2 * pad]: w = philox4x32_10(counter
    (draw_id, 0, 5, 0), key (seed, group)), dx = (w[0] * m) >> 32, dy = (w[1] * m) >> 32 with m = 2 * pad + 1"""
    pad = int(pad)
    if not 0 <= pad <= RANDOM_SHIFT_MAX_PAD:
        raise ValueError(f"random shift: pad = {pad} outside 0 .. {RANDOM_SHIFT_MAX_PAD}")
    groups = np.asarray(groups)
    w = philox(int(draw_id) & 0xFFFFFFFF, 0, RANDOM_SHIFT_LANE, 0, int(seed) & 0xFFFFFFFF, groups.astype(np.int64))
    m = np.uint64(2 * pad + 1)
    dx = ((w[0].astype(np.uint64) * m) >> np.uint64(32)).astype(np.int32)
    dy = ((w[1].astype(np.uint64) * m) >> np.uint64(32)).astype(np.int32)
    return dy.reshape(groups.shape), dx.reshape(groups.shape)


def random_shift_frames(frames, dy, dx, pad: int) -> np.ndarray:
    """frames [N, C, H, W] (u8 or f32), dy / dx int [N] in [0, 2 * pad]: pad by `pad` pixels with edge replication and crop
    back at (dy, dx): out[i, c, y, x] = frames[i, c, clip(y + dy[i] - pad, 0, H - 1), clip(x + dx[i] - pad, 0, W - 1)]"""
    a = np.asarray(frames)
    if a.ndim != 4:
        raise ValueError(f"frames [N, C, H, W] expected, got shape {a.shape}")
    N, _, H, W = a.shape
    dy, dx = np.asarray(dy, dtype=np.int64).reshape(N), np.asarray(dx, dtype=np.int64).reshape(N)
    ys = np.clip(np.arange(H, dtype=np.int64)[None, :] + dy[:, None] - int(pad), 0, H - 1)  # [N, H]
    xs = np.clip(np.arange(W, dtype=np.int64)[None, :] + dx[:, None] - int(pad), 0, W - 1)  # [N, W]
    return np.ascontiguousarray(a[np.arange(N)[:, None, None, None], np.arange(a.shape[1])[None, :, None, None],
                                  ys[:, None, :, None], xs[:, None, None, :]])


# ---- cutout and intensity (sf_augment_gather) ------------------------------------------------------------------------
AUGMENT_LANE_CUTOUT = 8      # lane 2 of the Philox counter (6 and 7: PixelCatch's levels): the cutout rectangle
AUGMENT_LANE_INTENSITY = 9   # ... the intensity scale and the fill byte
AUGMENT_LANE_SELECT = 10     # ... which op an SGD step applies under --augment_mix one (drawn on the host only)
CUTOUT_MAX_SIDE = 65535
INTENSITY_MAX = 255
CUTOUT_FILLS = ("zero", "random")
AUGMENT_OPS = ("shift", "cutout", "intensity")  # the order of `enabled` in augment_op_of_step


def _mulhi(w, m: int) -> np.ndarray:
    """(w * m) >> 32 as a 64-bit product, w uint32 words, 0 <= m < 2^32"""
    return ((np.asarray(w).astype(np.uint64) * np.uint64(m)) >> np.uint64(32)).astype(np.int64)


def _lane_words(seed: int, draw_id: int, groups, lane: int):
    groups = np.asarray(groups)
    w = philox(int(draw_id) & 0xFFFFFFFF, 0, lane, 0, int(seed) & 0xFFFFFFFF, groups.astype(np.int64))
    return w, groups.shape


def cutout_draws(seed: int, draw_id: int, groups, H: int, W: int, cut_min: int, cut_max: int):
    """(y0, x0, ch, cw) int32 arrays, one rectangle per entry of `groups`: w = philox4x32_10(counter (draw_id, 0, 8, 0),
    key (seed, group)); ch = lo_h + mulhi(w[0], hi_h - lo_h + 1) with lo_h = min(cut_min, H), hi_h = min(cut_max, H); cw the
    same from w[1] and W; y0 = mulhi(w[2], H - ch + 1), x0 = mulhi(w[3], W - cw + 1): always inside the frame"""
    H, W, cut_min, cut_max = int(H), int(W), int(cut_min), int(cut_max)
    if H < 1 or W < 1:
        raise ValueError(f"cutout: frame of {H} x {W}")
    if not 1 <= cut_min <= cut_max <= CUTOUT_MAX_SIDE:
        raise ValueError(f"cutout: side lengths [{cut_min}, {cut_max}] need 1 <= MIN <= MAX <= {CUTOUT_MAX_SIDE}")
    w, shape = _lane_words(seed, draw_id, groups, AUGMENT_LANE_CUTOUT)
    lo_h, hi_h, lo_w, hi_w = min(cut_min, H), min(cut_max, H), min(cut_min, W), min(cut_max, W)
    ch = lo_h + _mulhi(w[0], hi_h - lo_h + 1)
    cw = lo_w + _mulhi(w[1], hi_w - lo_w + 1)
    y0 = (w[2].astype(np.uint64) * (H - ch + 1).astype(np.uint64)) >> np.uint64(32)
    x0 = (w[3].astype(np.uint64) * (W - cw + 1).astype(np.uint64)) >> np.uint64(32)
    return tuple(np.asarray(v).astype(np.int32).reshape(shape) for v in (y0, x0, ch, cw))


def intensity_draws(seed: int, draw_id: int, groups, amp: int):
    """(s, fill) int32 arrays, one pair per entry of `groups`: w = philox4x32_10(counter (draw_id, 0, 9, 0), key (seed,
    group)); s = 256 - amp + mulhi(w[0], 2 amp + 1) in [256 - amp, 256 + amp] (the scale is s / 256), fill = w[1] >> 24"""
    amp = int(amp)
    if not 0 <= amp <= INTENSITY_MAX:
        raise ValueError(f"intensity: amplitude {amp} outside 0 .. {INTENSITY_MAX}")
    w, shape = _lane_words(seed, draw_id, groups, AUGMENT_LANE_INTENSITY)
    s = 256 - amp + _mulhi(w[0], 2 * amp + 1)
    fill = w[1].astype(np.int64) >> 24
    return s.astype(np.int32).reshape(shape), fill.astype(np.int32).reshape(shape)


def intensity_frames(frames, s) -> np.ndarray:
    """frames [N, C, H, W], s int [N]: u8 -> min(255, (x * s + 128) >> 8); f32 -> x * float32(s / 256), ONE float32
    multiply (s / 256 is exact in float32)"""
    a = np.asarray(frames)
    if a.ndim != 4:
        raise ValueError(f"frames [N, C, H, W] expected, got shape {a.shape}")
    s = np.asarray(s, dtype=np.int64).reshape(a.shape[0], 1, 1, 1)
    if a.dtype == np.uint8:
        return np.minimum(255, (a.astype(np.int64) * s + 128) >> 8).astype(np.uint8)
    if a.dtype == np.float32:
        return a * (s.astype(np.float32) / np.float32(256.0))
    raise ValueError(f"u8 or f32 frames expected, got dtype {a.dtype}")


def cutout_frames(frames, y0, x0, ch, cw, fill=None) -> np.ndarray:
    """frames [N, C, H, W]: out[i, :, y0[i]:y0[i] + ch[i], x0[i]:x0[i] + cw[i]] = fill[i] (None: 0), every plane alike"""
    a = np.asarray(frames)
    if a.ndim != 4:
        raise ValueError(f"frames [N, C, H, W] expected, got shape {a.shape}")
    N = a.shape[0]
    y0, x0, ch, cw = (np.asarray(v, dtype=np.int64).reshape(N) for v in (y0, x0, ch, cw))
    if fill is not None and a.dtype != np.uint8:
        raise ValueError(f"a fill byte is for u8 frames, got dtype {a.dtype}")
    fill = np.zeros(N, np.int64) if fill is None else np.asarray(fill, dtype=np.int64).reshape(N)
    out = a.copy()
    for i in range(N):
        out[i, :, y0[i]:y0[i] + ch[i], x0[i]:x0[i] + cw[i]] = fill[i]
    return out


def augment_frames(frames, seed: int, draw_id: int, groups, *, pad: int = 0, cutout=(), cutout_fill: str = "zero",
                   intensity: int = 0) -> np.ndarray:
    """what sf_augment_gather does to frames [N, C, H, W] (u8 or f32) whose sample i draws under groups[i]: the shift, then
    the intensity, then the cutout (in output coordinates, its fill not scaled); a stage whose parameter is 0 / () is
    skipped.  With only `pad` it is random_shift_frames under random_shift_draws"""
    a = np.asarray(frames)
    if a.ndim != 4:
        raise ValueError(f"frames [N, C, H, W] expected, got shape {a.shape}")
    if cutout_fill not in CUTOUT_FILLS:
        raise ValueError(f"cutout_fill must be one of {CUTOUT_FILLS}, got {cutout_fill!r}")
    cut = tuple(int(v) for v in (cutout or ()))
    if len(cut) not in (0, 2):
        raise ValueError(f"cutout must be () or (MIN, MAX), got {cutout!r}")
    if cut and cutout_fill == "random" and a.dtype != np.uint8:
        raise ValueError(f"cutout_fill=random is one byte per sample: u8 frames only, got dtype {a.dtype}")
    groups = np.asarray(groups).reshape(a.shape[0])
    out = a
    if int(pad) > 0:
        dy, dx = random_shift_draws(seed, draw_id, groups, pad)
        out = random_shift_frames(out, dy, dx, pad)
    s, fill = intensity_draws(seed, draw_id, groups, intensity)  # (amp = 0: s = 256, and the fill byte is still drawn)
    if int(intensity) > 0:
        out = intensity_frames(out, s)
    if cut:
        y0, x0, ch, cw = cutout_draws(seed, draw_id, groups, a.shape[2], a.shape[3], *cut)
        out = cutout_frames(out, y0, x0, ch, cw, fill if cutout_fill == "random" else None)
    return np.ascontiguousarray(out)


def augment_op_of_step(seed: int, draw_id: int, enabled):
    """--augment_mix one: the op SGD step `draw_id` applies, out of `enabled` (the switched-on ops in the order shift,
    cutout, intensity): enabled[mulhi(w[0], len(enabled))], w = philox4x32_10(counter (draw_id, 0, 10, 0), key (seed, 0)).
    Stateless: a resumed run draws what the uninterrupted one would have"""
    enabled = list(enabled)
    if not enabled:
        raise ValueError("augment_op_of_step: no op is enabled")
    w, _ = _lane_words(seed, draw_id, np.zeros((), np.int64), AUGMENT_LANE_SELECT)
    return enabled[int(_mulhi(w[0], len(enabled)))]
