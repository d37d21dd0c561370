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
DESIGN.md 3.17): `random_shift_draws`, `random_shift_frames` and the learner's `random_shift_seed`."""
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
