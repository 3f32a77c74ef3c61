"""The limited-range -> full-range map of JPEGAMD_RANGE_LIMITED (include/jpeg_compression.h), from its definition: every sample is
clamped to its nominal range, then rescaled with round-half-up, in integers.  Two 256-entry tables, and the fixed-point forms that
reproduce them (the 24-bit products of the design notes, and the split into 16-bit terms that the tile kernel evaluates)."""
from __future__ import annotations

import numpy as np


def luma_table() -> np.ndarray:
    """Y' = (255 (clamp(Y, 16, 235) - 16) + 109) // 219 for Y = 0 .. 255."""
    return np.array([(255 * (min(max(v, 16), 235) - 16) + 109) // 219 for v in range(256)], np.uint8)


def chroma_table() -> np.ndarray:
    """C' = (255 (clamp(C, 16, 240) - 16) + 112) // 224 for C = 0 .. 255 (Cb and Cr alike)."""
    return np.array([(255 * (min(max(v, 16), 240) - 16) + 112) // 224 for v in range(256)], np.uint8)


def luma_mad24(t: int) -> int:
    """The Y map of t = clamp(Y, 16, 235) - 16 as one 24-bit multiply-add and a shift."""
    return (2385 * t + 986) >> 11


def chroma_mad24(t: int) -> int:
    return (4663 * t + 2032) >> 12


def luma_split16(t: int) -> int:
    """The same with the multiplier split at bit 8 (2385 = 9 * 256 + 81): every term fits 16 bits."""
    return (9 * t + ((81 * t + 986) >> 8)) >> 3


def chroma_split16(t: int) -> int:
    """4663 = 18 * 256 + 55."""
    return (18 * t + ((55 * t + 2032) >> 8)) >> 4


def expand(planes):
    """(y, cb, cr) limited range -> the full-range planes the encoder codes."""
    y, cb, cr = planes
    ymap, cmap = luma_table(), chroma_table()
    return ymap[y], cmap[cb], cmap[cr]
