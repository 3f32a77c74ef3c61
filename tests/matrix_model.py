"""The BT.709 -> BT.601 map of JPEGAMD_MATRIX_BT709 (include/jpeg_compression.h), from its definition: the real matrix composes two
exact-rational steps -- BT.709 YCbCr -> R'G'B' (Kr = 0.2126, Kb = 0.0722), then R'G'B' -> BT.601 YCbCr (Kr = 0.299, Kb = 0.114) -- on
full-range 8-bit samples; the six integers are its chroma columns scaled by 2^14 and rounded.  convert() is the map in numpy:
(y, cb, cr) uint8 planes at a subsampling -> the planes the encoder codes.  Luma (x, y) takes the chroma sample at the same indices as
the file's subsampling; no interpolation."""
from __future__ import annotations

from fractions import Fraction as F

import numpy as np

SHIFT = 14
KR709, KB709 = F(2126, 10000), F(722, 10000)
KR601, KB601 = F(299, 1000), F(114, 1000)
SUB_444, SUB_420, SUB_422 = 1, 2, 4                       # JPEGAMD_SUBSAMPLE_*


def real_matrix():
    """[[dY/dcb, dY/dcr], [dCb'/dcb, dCb'/dcr], [dCr'/dcb, dCr'/dcr]] as exact fractions (the luma column is (1, 0, 0))."""
    kg709 = 1 - KR709 - KB709
    # R = Y + 2 (1 - Kr) cr,  B = Y + 2 (1 - Kb) cb,  G = (Y - Kr R - Kb B) / Kg   -- per unit of (cb, cr), at Y = 0
    r = (F(0), 2 * (1 - KR709))
    b = (2 * (1 - KB709), F(0))
    g = tuple(-(KR709 * r[k] + KB709 * b[k]) / kg709 for k in range(2))
    kg601 = 1 - KR601 - KB601
    y = tuple(KR601 * r[k] + kg601 * g[k] + KB601 * b[k] for k in range(2))
    cb = tuple((b[k] - y[k]) / (2 * (1 - KB601)) for k in range(2))
    cr = tuple((r[k] - y[k]) / (2 * (1 - KR601)) for k in range(2))
    return [list(y), list(cb), list(cr)]


def _round(q: F) -> int:
    """Round to nearest, halves away from zero (no coefficient is a half: the choice never shows)."""
    n = abs(q)
    v = int(n + F(1, 2))
    return v if q >= 0 else -v


def coeffs():
    """The six integers round(c * 2^14), row by row: Y' (cb, cr), Cb' (cb, cr), Cr' (cb, cr)."""
    return [_round(c * (1 << SHIFT)) for row in real_matrix() for c in row]


def terms(cb, cr):
    """The three integer terms ((c0 cb + c1 cr + 8192) >> 14) for cb, cr = Cb - 128, Cr - 128 (ints or int64 arrays)."""
    c = coeffs()
    half = 1 << (SHIFT - 1)
    return tuple((c[2 * k] * cb + c[2 * k + 1] * cr + half) >> SHIFT for k in range(3))


def chroma_at_luma(plane, shape, sub):
    """A chroma plane -> one sample per luma site: (x, y), (x >> 1, y) or (x >> 1, y >> 1)."""
    h, w = shape
    ys = np.arange(h) >> (1 if sub == SUB_420 else 0)
    xs = np.arange(w) >> (0 if sub == SUB_444 else 1)
    return plane[np.ix_(ys, xs)]


def convert(planes, sub):
    """(y, cb, cr) uint8, 8-bit full-range BT.709 -> the 8-bit full-range BT.601 planes, by the definition."""
    y, cb, cr = planes
    b, r = cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    ty, tb, tr = terms(b, r)
    ny = np.clip(y.astype(np.int64) + chroma_at_luma(ty, y.shape, sub), 0, 255).astype(np.uint8)
    return ny, np.clip(128 + tb, 0, 255).astype(np.uint8), np.clip(128 + tr, 0, 255).astype(np.uint8)


def convert_real(y, cb, cr):
    """One colour through the real-valued matrix, rounded half-up and clamped (what the integers approximate)."""
    m = real_matrix()
    b, r = cb - 128, cr - 128
    vals = (y + m[0][0] * b + m[0][1] * r, 128 + m[1][0] * b + m[1][1] * r, 128 + m[2][0] * b + m[2][1] * r)
    return tuple(min(max(int((v + F(1, 2)) // 1), 0), 255) for v in vals)


def bt709_ycbcr(r, g, b):
    """An R'G'B' colour (0..255) -> its full-range 8-bit BT.709 (Y, Cb, Cr), rounded half-up."""
    kg = 1 - KR709 - KB709
    y = KR709 * r + kg * g + KB709 * b
    cb = 128 + (b - y) / (2 * (1 - KB709))
    cr = 128 + (r - y) / (2 * (1 - KR709))
    return tuple(min(max(int((v + F(1, 2)) // 1), 0), 255) for v in (y, cb, cr))
