"""Progressive colour files (SOF2) -- what web delivery, image CDNs and thumbnail services ask an encoder for -- from every packed or
YCbCr source the one-scan functions of `jpegamd.mjpeg` read.

Each function is its twin in `jpegamd.mjpeg` without `restart_interval=` and `huffman=`: the same tensors, the same layout=, order=,
sample_range=, matrix= and align=.  The file holds the coefficients of the twin's one-scan file in seven scans by spectral selection
(the DC of all three components, then the bands 1..5 and 6..63 of Y, Cb and Cr) and decodes to the same pixels.  It is a little larger
than the one-scan file: it codes no end-of-band runs with the Annex K tables (`jpegamd.progressive_optimized` does, with tables of its
own, and is about the size of the optimised one-scan file).

Planar R, G, B pictures (layout="chw") are not taken.  The Annex K tables are set on the per-device context for the call."""
from __future__ import annotations

import jpegamd as _j


def encode_ycbcr_batch(y, cb, cr=None, quality: int = 0, subsampling: int = _j.SUBSAMPLE_420, order: str = "cbcr",
                       sample_range: str = "full", matrix: str = "bt601") -> list:
    """jpegamd.encode_ycbcr_batch's pictures (planes, or pairs with cr=None) -> N progressive files, for either sample_range and
    matrix, through jpegamd_encode_ycbcr_progressive_batch_async."""
    rng, mat = _j._sample_range(sample_range), _j._matrix(matrix)
    return _j._encode_ycbcr_planes("encode_ycbcr_batch", _j._ycbcr_layout, y, cb, cr, quality, subsampling, order, None, rng, matrix=mat,
                                   interleaved=True, any_kind=True, progressive=True)


def encode_ycbcr16_batch(y, cb, cr=None, quality: int = 0, subsampling: int = _j.SUBSAMPLE_420, order: str = "cbcr",
                         sample_range: str = "full", align: str = "msb", matrix: str = "bt601") -> list:
    """jpegamd.encode_ycbcr16_batch's pictures (10-bit samples in 16-bit words: P010 / I010 families) -> N progressive files."""
    rng, mat = _j._sample_range(sample_range), _j._matrix(matrix)
    if not isinstance(align, str) or align not in ("msb", "lsb"):
        raise ValueError(f'align must be "msb" or "lsb", not {align!r}')
    return _j._encode_ycbcr_planes("encode_ycbcr16_batch", _j._ycbcr16_layout, y, cb, cr, quality, subsampling, order, None, rng,
                                   _j.SAMPLES_10_MSB if align == "msb" else _j.SAMPLES_10_LSB, mat, interleaved=True, any_kind=True,
                                   progressive=True)


def encode_yuyv_batch(frames, quality: int = 0, order: str = "yuyv", sample_range: str = "full", matrix: str = "bt601") -> list:
    """jpegamd.encode_yuyv_batch's packed 4:2:2 frames (YUY2 / UYVY) -> N progressive files at SUBSAMPLE_422."""
    rng, mat = _j._sample_range(sample_range), _j._matrix(matrix)
    return _j._encode_yuyv_frames(frames, quality, order, None, rng, mat, interleaved=True, any_kind=True, progressive=True)


def encode_tensor_batch(t, quality: int = 0, subsampling: int = _j.SUBSAMPLE_420, layout=None) -> list:
    """jpegamd.encode_tensor_batch's packed colour pictures -> N progressive files: [N, H, W, 3], or layout= "rgba" / "bgra"
    [N, H, W, 4], "hwc".  [N, H, W] grayscale pictures, subsampling 0 and layout="chw" are ValueErrors."""
    return _j.encode_tensor_batch(t, quality, subsampling, layout, scan="interleaved", _any_layout=True, _progressive=True)


def encode_tensor(t, quality: int = 0, subsampling: int = _j.SUBSAMPLE_420, layout=None) -> bytes:
    """One colour picture -> its progressive file: [H, W, 3], or layout= "rgba" / "bgra" [H, W, 4], "hwc"."""
    return _j.encode_tensor_batch(t, quality, subsampling, "hwc" if layout is None else layout, _single=True, scan="interleaved",
                                  _any_layout=True, _progressive=True)[0]
