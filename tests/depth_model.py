"""The 10-bit -> 8-bit maps of JPEGAMD_SAMPLES_10_MSB / _LSB (include/jpeg_compression.h), from their definition: a sample is a 16-bit
word w, its 10-bit value v follows from the alignment, and the coded 8-bit sample from v and the sample range, in integers with
floor division.  1024-entry tables for the four (range, component) maps, 65 536-entry tables for the two alignments, the fixed-point
forms the tile kernel evaluates, and narrow(): 16-bit planes -> the uint8 planes the encoder codes."""
from __future__ import annotations

import numpy as np

FULL, LIMITED = "full", "limited"
MSB, LSB = "msb", "lsb"


def value_table(align: str) -> np.ndarray:
    """v for every 16-bit word w: w >> 6 (MSB-aligned, the low six bits ignored) or min(w, 1023) (LSB-aligned)."""
    w = np.arange(65536, dtype=np.int64)
    if align == MSB:
        return (w >> 6).astype(np.uint16)
    if align == LSB:
        return np.minimum(w, 1023).astype(np.uint16)
    raise ValueError(align)


def full_table() -> np.ndarray:
    """s = min(255, (v + 2) >> 2) for v = 0 .. 1023: Y, Cb and Cr alike."""
    return np.array([min(255, (v + 2) >> 2) for v in range(1024)], np.uint8)


def luma_table() -> np.ndarray:
    """Y' = (255 (clamp(v, 64, 940) - 64) + 438) // 876 for v = 0 .. 1023."""
    return np.array([(255 * (min(max(v, 64), 940) - 64) + 438) // 876 for v in range(1024)], np.uint8)


def chroma_table() -> np.ndarray:
    """C' = (255 (clamp(v, 64, 960) - 64) + 448) // 896 for v = 0 .. 1023 (Cb and Cr alike)."""
    return np.array([(255 * (min(max(v, 64), 960) - 64) + 448) // 896 for v in range(1024)], np.uint8)


def table(sample_range: str, chroma: bool) -> np.ndarray:
    """The 1024-entry map of one (range, component)."""
    if sample_range == FULL:
        return full_table()
    if sample_range == LIMITED:
        return chroma_table() if chroma else luma_table()
    raise ValueError(sample_range)


# ---- the forms the kernel evaluates: each returns (result, every intermediate term) ---------------------------------------------------
def kernel_value(w: int, shift: int) -> int:
    """A 16-bit shift; the clamp to 1023 belongs to the map behind it (full: explicit; limited: implied by the upper clamp)."""
    return w >> shift


def kernel_full(v: int):
    """v is any 16-bit value (an LSB-aligned word is not clamped yet): min, add, shift, min -- 16-bit terms."""
    a = min(v, 1023)
    b = a + 2
    return min(b >> 2, 255), (a, b)


def kernel_luma(v: int):
    """t = min(v -sat 64, 876); one 24-bit multiply-add; byte 2 of the product (bits 16 .. 23)."""
    t = min(max(v - 64, 0), 876)
    p = 19077 * t + 33000
    return (p >> 16) & 0xFF, (t, p)


def kernel_chroma(v: int):
    """t = min(v -sat 64, 896); 4663 = 18 * 256 + 55 as in the 8-bit map, two bits further down; 16-bit terms."""
    t = min(max(v - 64, 0), 896)
    a = 55 * t + 8136
    b = 18 * t + (a >> 8)
    return b >> 6, (t, a, 18 * t, b)


def kernel_msb_full(w: int):
    """The MSB-aligned full-range map in one saturating add and a shift: (w +sat 128) >> 8."""
    a = min(w + 128, 65535)
    return a >> 8, (a,)


def narrow(planes16, sample_range: str, align: str):
    """(y, cb, cr) of 16-bit words (uint16 or int16: the bit pattern counts) -> the uint8 planes the encoder codes."""
    val = value_table(align)
    y, cb, cr = (val[np.ascontiguousarray(p).view(np.uint16)] for p in planes16)
    ymap, cmap = table(sample_range, False), table(sample_range, True)
    return ymap[y], cmap[cb], cmap[cr]


def narrow_truncating(planes16, align: str):
    """What a narrowing pass that drops bits would give (w >> 8 of the MSB-aligned word, v >> 2): NOT the definition."""
    val = value_table(align)
    return tuple((val[np.ascontiguousarray(p).view(np.uint16)] >> 2).astype(np.uint8) for p in planes16)
