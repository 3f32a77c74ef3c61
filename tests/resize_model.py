"""The map of resized pictures (include/jpeg_compression.h, "Resized pictures") in numpy integers: every target sample is
(S + (D >> 1)) // D, with S the source samples weighted by the exact share of each inside the target sample's footprint and D = W H.
Built from each target sample's at most ceil(W / ow) + 1 taps per axis, one tap at a time: no [ow, W] matrix is ever made."""
from __future__ import annotations

import numpy as np

MAX_RESIZE_RATIO = 64


def check(w: int, h: int, ow: int, oh: int) -> bool:
    """jpegamd_resize_check's rule."""
    return (1 <= w <= 65535 and 1 <= h <= 65535 and 1 <= ow <= w <= MAX_RESIZE_RATIO * ow and 1 <= oh <= h <= MAX_RESIZE_RATIO * oh)


def taps(n: int, on: int) -> tuple:
    """One axis of n source and on target samples -> (index [on, T], weight [on, T]) with T = ceil(n / on) + 1: tap t of target X is
    source sample floor(X n / on) + t (held at n - 1 past the end, where its weight is 0) with weight
    max(0, min((X + 1) n, (x + 1) on) - max(X n, x on))."""
    t = -(-n // on) + 1
    big = np.arange(on, dtype=np.int64)[:, None]
    x = big * n // on + np.arange(t, dtype=np.int64)[None, :]
    w = np.maximum(0, np.minimum((big + 1) * n, (x + 1) * on) - np.maximum(big * n, x * on))
    return np.minimum(x, n - 1), w


def resize_plane(a: np.ndarray, ow: int, oh: int) -> np.ndarray:
    """[H, W] bytes -> [oh, ow] bytes."""
    h, w = a.shape
    assert check(w, h, ow, oh), (w, h, ow, oh)
    src = a.astype(np.int64)
    ix, wx = taps(w, ow)
    iy, wy = taps(h, oh)
    rows = np.zeros((h, ow), np.int64)
    for t in range(ix.shape[1]):
        rows += src[:, ix[:, t]] * wx[None, :, t]
    s = np.zeros((oh, ow), np.int64)
    for t in range(iy.shape[1]):
        s += rows[iy[:, t], :] * wy[:, t, None]
    d = w * h
    v = (s + (d >> 1)) // d
    assert v.min() >= 0 and v.max() <= 255
    return v.astype(np.uint8)


def resize_picture(pic: np.ndarray, ow: int, oh: int) -> np.ndarray:
    """[H, W, C] bytes -> [oh, ow, C] bytes, channel by channel."""
    return np.stack([resize_plane(pic[:, :, c], ow, oh) for c in range(pic.shape[2])], axis=2)


def fit_size(w: int, h: int, max_w: int, max_h: int) -> tuple:
    """jpegamd.fit_size's rule."""
    if w <= max_w and h <= max_h:
        return w, h
    if w * max_h >= h * max_w:
        return max_w, max(1, (h * max_w + w // 2) // w)
    return max(1, (w * max_h + h // 2) // h), max_h
