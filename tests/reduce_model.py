"""The map of reduced pictures (include/jpeg_compression.h, "Reduced pictures") in numpy integers: every reduced sample is the rounded
mean (S + (n >> 1)) // n of the n source samples of its factor x factor box that lie inside the picture."""
from __future__ import annotations

import numpy as np

MAX_REDUCE = 8
SHIFT = 22                                                        # the kernel divides by n with ceil(2^22 / n) and this shift


def reduced_size(w: int, h: int, f: int) -> tuple:
    return -(-w // f), -(-h // f)


def box_counts(w: int, h: int, f: int) -> np.ndarray:
    """n of every box, [oh, ow]."""
    ow, oh = reduced_size(w, h, f)
    nx = np.minimum(f, w - f * np.arange(ow))
    ny = np.minimum(f, h - f * np.arange(oh))
    return ny[:, None] * nx[None, :]


def reduce_plane(a: np.ndarray, f: int) -> np.ndarray:
    """[H, W] bytes -> [oh, ow] bytes."""
    h, w = a.shape
    ow, oh = reduced_size(w, h, f)
    padded = np.zeros((oh * f, ow * f), np.int64)
    padded[:h, :w] = a                                            # zeros outside add nothing to S; n counts the inside alone
    s = padded.reshape(oh, f, ow, f).sum(axis=(1, 3))
    n = box_counts(w, h, f)
    return ((s + (n >> 1)) // n).astype(np.uint8)


def reduce_picture(pic: np.ndarray, f: int) -> np.ndarray:
    """[H, W, C] bytes -> [oh, ow, C] bytes, channel by channel."""
    return np.stack([reduce_plane(pic[:, :, c], f) for c in range(pic.shape[2])], axis=2)


def reciprocal(n: int) -> int:
    """ceil(2^SHIFT / n): the constant rule of the kernel's table."""
    return -(-(1 << SHIFT) // n)
