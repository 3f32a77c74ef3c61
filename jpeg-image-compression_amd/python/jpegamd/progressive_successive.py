"""Progressive colour files (SOF2) with successive approximation: the five functions of
`jpegamd.progressive_optimized`, taking the same arguments.

The file holds the coefficients of the one-scan file in the ten scans of libjpeg's default progressive script -- what `cjpeg
-progressive` and PIL's `progressive=True` write -- and decodes to the same pixels: the whole picture coarsely after the first scans,
then refined bit by bit.  Every scan carries a table made of its own symbol counts, and the AC scans code runs of empty blocks with one
symbol.  It is about the size of `jpegamd.progressive_optimized`'s file (a few per cent larger at low qualities, smaller at high ones);
its value is the order in which a viewer sees it.

Planar R, G, B pictures (layout="chw") are not taken.  The per-device context's Huffman mode is neither read nor changed."""
from __future__ import annotations

import jpegamd as _j

_OWN = _j.PROGRESSIVE_SUCCESSIVE


def encode_ycbcr_batch(y, cb, cr=None, quality: int = 0, subsampling: int = _j.SUBSAMPLE_420, order: str = "cbcr",
                       sample_range: str = "full", matrix: str = "bt601") -> list:
    """jpegamd.encode_ycbcr_batch's pictures (planes, or pairs with cr=None) -> N files, for either sample_range and matrix, through
    jpegamd_encode_ycbcr_progressive_successive_batch_async."""
    rng, mat = _j._sample_range(sample_range), _j._matrix(matrix)
    return _j._encode_ycbcr_planes("encode_ycbcr_batch", _j._ycbcr_layout, y, cb, cr, quality, subsampling, order, None, rng, matrix=mat,
                                   interleaved=True, any_kind=True, progressive=_OWN)


def encode_ycbcr16_batch(y, cb, cr=None, quality: int = 0, subsampling: int = _j.SUBSAMPLE_420, order: str = "cbcr",
                         sample_range: str = "full", align: str = "msb", matrix: str = "bt601") -> list:
    """jpegamd.encode_ycbcr16_batch's pictures (10-bit samples in 16-bit words: P010 / I010 families) -> N files."""
    rng, mat = _j._sample_range(sample_range), _j._matrix(matrix)
    if not isinstance(align, str) or align not in ("msb", "lsb"):
        raise ValueError(f'align must be "msb" or "lsb", not {align!r}')
    return _j._encode_ycbcr_planes("encode_ycbcr16_batch", _j._ycbcr16_layout, y, cb, cr, quality, subsampling, order, None, rng,
                                   _j.SAMPLES_10_MSB if align == "msb" else _j.SAMPLES_10_LSB, mat, interleaved=True, any_kind=True,
                                   progressive=_OWN)


def encode_yuyv_batch(frames, quality: int = 0, order: str = "yuyv", sample_range: str = "full", matrix: str = "bt601") -> list:
    """jpegamd.encode_yuyv_batch's packed 4:2:2 frames (YUY2 / UYVY) -> N files at SUBSAMPLE_422."""
    rng, mat = _j._sample_range(sample_range), _j._matrix(matrix)
    return _j._encode_yuyv_frames(frames, quality, order, None, rng, mat, interleaved=True, any_kind=True, progressive=_OWN)


def encode_tensor_batch(t, quality: int = 0, subsampling: int = _j.SUBSAMPLE_420, layout=None) -> list:
    """jpegamd.encode_tensor_batch's packed colour pictures -> N files: [N, H, W, 3], or layout= "rgba" / "bgra" [N, H, W, 4], "hwc".
    [N, H, W] grayscale pictures, subsampling 0 and layout="chw" are ValueErrors."""
    return _j.encode_tensor_batch(t, quality, subsampling, layout, scan="interleaved", _any_layout=True, _progressive=_OWN)


def encode_tensor(t, quality: int = 0, subsampling: int = _j.SUBSAMPLE_420, layout=None) -> bytes:
    """One colour picture -> its file: [H, W, 3], or layout= "rgba" / "bgra" [H, W, 4], "hwc"."""
    return _j.encode_tensor_batch(t, quality, subsampling, "hwc" if layout is None else layout, _single=True, scan="interleaved",
                                  _any_layout=True, _progressive=_OWN)[0]
