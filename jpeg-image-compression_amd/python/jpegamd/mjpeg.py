"""Colour files with ONE scan of interleaved MCUs -- what Motion-JPEG containers, RTP/JPEG senders, hardware and embedded decoders
take -- from every source the three-scan functions of `jpegamd` read.

Each function is its twin in `jpegamd` without `scan=` and with `restart_interval=` (None / 0: none; 1 .. 65535 MCUs; "row": one MCU
row): the same tensors, the same layout=, order=, sample_range=, matrix= and align=.  The file holds the samples the twin's three-scan
file holds -- after the depth, range and matrix maps of include/jpeg_compression.h, in that order -- and decodes to the same pixels.
Nothing is repacked or converted by a pass of its own: the tile kernel reads every source where it lies (BT.709: behind the one
matrix pass of the three-scan path).

huffman= "standard" (the Annex K tables, default) or "optimized": four tables made for each picture from its own symbol counts, as
libjpeg -optimize makes them -- the same pixels in a smaller file.  The mode is set on the per-device context for the
call and STANDARD is put back behind it.

encode_gray_batch / encode_gray: GRAYSCALE pictures with the same two options -- the grayscale file written as a scan of one component
(DESIGN.md 4.6.11), two tables per picture in "optimized"."""
from __future__ import annotations

import jpegamd as _j


def encode_ycbcr_batch(y, cb, cr=None, quality: int = 0, subsampling: int = _j.SUBSAMPLE_420, order: str = "cbcr",
                       sample_range: str = "full", matrix: str = "bt601", restart_interval=None, huffman: str = "standard") -> list:
    """jpegamd.encode_ycbcr_batch's pictures (planes, or pairs with cr=None) -> N one-scan files, for either sample_range and matrix,
    through jpegamd_encode_ycbcr_interleaved_matrix_batch_async."""
    huff = _j._huffman(huffman)
    rng, mat = _j._sample_range(sample_range), _j._matrix(matrix)
    return _j._encode_ycbcr_planes("encode_ycbcr_batch", _j._ycbcr_layout, y, cb, cr, quality, subsampling, order, restart_interval,
                                   rng, matrix=mat, interleaved=True, any_kind=True, huffman=huff)


def encode_ycbcr16_batch(y, cb, cr=None, quality: int = 0, subsampling: int = _j.SUBSAMPLE_420, order: str = "cbcr",
                         sample_range: str = "full", align: str = "msb", matrix: str = "bt601", restart_interval=None,
                         huffman: str = "standard") -> list:
    """jpegamd.encode_ycbcr16_batch's pictures (10-bit samples in 16-bit words: P010 / I010 families) -> N one-scan files."""
    huff = _j._huffman(huffman)
    rng, mat = _j._sample_range(sample_range), _j._matrix(matrix)
    if not isinstance(align, str) or align not in ("msb", "lsb"):
        raise ValueError(f'align must be "msb" or "lsb", not {align!r}')
    return _j._encode_ycbcr_planes("encode_ycbcr16_batch", _j._ycbcr16_layout, y, cb, cr, quality, subsampling, order, restart_interval,
                                   rng, _j.SAMPLES_10_MSB if align == "msb" else _j.SAMPLES_10_LSB, mat, interleaved=True, any_kind=True,
                                   huffman=huff)


def encode_yuyv_batch(frames, quality: int = 0, order: str = "yuyv", sample_range: str = "full", matrix: str = "bt601",
                      restart_interval=None, huffman: str = "standard") -> list:
    """jpegamd.encode_yuyv_batch's packed 4:2:2 frames (YUY2 / UYVY) -> N one-scan files at SUBSAMPLE_422."""
    huff = _j._huffman(huffman)
    rng, mat = _j._sample_range(sample_range), _j._matrix(matrix)
    return _j._encode_yuyv_frames(frames, quality, order, restart_interval, rng, mat, interleaved=True, any_kind=True, huffman=huff)


def encode_tensor_batch(t, quality: int = 0, subsampling: int = _j.SUBSAMPLE_420, layout=None, restart_interval=None,
                        huffman: str = "standard") -> list:
    """jpegamd.encode_tensor_batch's colour pictures -> N one-scan files: [N, H, W, 3], or layout= "chw" ([N, 3, H, W] or three plane
    tensors), "rgba" / "bgra" [N, H, W, 4], "hwc".  The files are those of the same R, G, B values as [N, H, W, 3].  A one-scan file is
    a colour file: [N, H, W] grayscale pictures and subsampling 0 are ValueErrors."""
    return _j.encode_tensor_batch(t, quality, subsampling, layout, scan="interleaved", restart_interval=restart_interval, _any_layout=True,
                                  _huffman=_j._huffman(huffman))


def encode_tensor(t, quality: int = 0, subsampling: int = _j.SUBSAMPLE_420, layout=None, restart_interval=None,
                  huffman: str = "standard") -> bytes:
    """One colour picture -> its one-scan file: [H, W, 3], or layout= "chw" [3, H, W], "rgba" / "bgra" [H, W, 4], "hwc"."""
    return _j.encode_tensor_batch(t, quality, subsampling, "hwc" if layout is None else layout, _single=True, scan="interleaved",
                                  restart_interval=restart_interval, _any_layout=True, _huffman=_j._huffman(huffman))[0]


def encode_gray_batch(t, quality: int = 0, restart_interval=None, huffman: str = "standard") -> list:
    """Grayscale pictures, a uint8 device tensor [N, H, W] (row-strided, packed within a row) -> N grayscale files with restart
    intervals and the chosen tables (jpegamd_encode_gray_scan_batch_async).  restart_interval: None / 0, an int
    1 .. 65535 (blocks: the MCU of a grayscale scan is one block), or "row" = ceil(W / 8).  Without intervals and with the standard
    tables the files are jpegamd.encode_tensor_batch's.  Bad values are ValueErrors, raised before any device work."""
    return _j._encode_gray_scan_batch(t, quality, restart_interval, huffman, "encode_gray_batch")


def encode_gray(t, quality: int = 0, restart_interval=None, huffman: str = "standard") -> bytes:
    """One grayscale picture [H, W] -> its file, as encode_gray_batch."""
    import torch
    if not isinstance(t, torch.Tensor) or t.dim() != 2:
        raise ValueError("encode_gray needs a uint8 tensor [H, W]")
    return _j._encode_gray_scan_batch(t.unsqueeze(0), quality, restart_interval, huffman, "encode_gray")[0]


def encode_float_batch(t, quality: int = 0, subsampling: int = _j.SUBSAMPLE_420, layout="chw", value_range=(0.0, 1.0),
                       restart_interval=None, huffman: str = "standard") -> list:
    """jpegamd.encode_float_batch's float32 / float16 / bfloat16 pictures -> N one-scan files through
    jpegamd_encode_float_interleaved_batch_async: byte for byte encode_tensor_batch's files of the bytes of the samples.  One channel
    (layout="gray") or subsampling 0: the grayscale file of encode_gray_batch."""
    return _j._encode_float("encode_float_batch", t, quality, subsampling, layout, value_range, False, interleaved=True,
                            restart_interval=restart_interval, huffman=huffman)


def encode_float(t, quality: int = 0, subsampling: int = _j.SUBSAMPLE_420, layout="chw", value_range=(0.0, 1.0), restart_interval=None,
                 huffman: str = "standard") -> bytes:
    """One float picture -> its one-scan file, as encode_float_batch."""
    return _j._encode_float("encode_float", t, quality, subsampling, layout, value_range, True, interleaved=True,
                            restart_interval=restart_interval, huffman=huffman)[0]


def encode_reduced_batch(t, quality: int = 0, subsampling: int = _j.SUBSAMPLE_420, factor: int = 2, layout="chw", restart_interval=None,
                         huffman: str = "standard") -> list:
    """jpegamd.encode_reduced_batch's uint8 pictures, each reduced by `factor` both ways -> N one-scan files through
    jpegamd_encode_reduced_interleaved_batch_async: byte for byte encode_tensor_batch's files of the reduced bytes.  restart_interval
    counts MCUs of the REDUCED picture ("row": one of its MCU rows).  One channel (layout="gray") or subsampling 0: the grayscale file
    of encode_gray_batch."""
    return _j._encode_reduced("encode_reduced_batch", t, quality, subsampling, factor, layout, False, interleaved=True,
                              restart_interval=restart_interval, huffman=huffman)


def encode_reduced(t, quality: int = 0, subsampling: int = _j.SUBSAMPLE_420, factor: int = 2, layout="chw", restart_interval=None,
                   huffman: str = "standard") -> bytes:
    """One picture of bytes -> its reduced one-scan file, as encode_reduced_batch."""
    return _j._encode_reduced("encode_reduced", t, quality, subsampling, factor, layout, True, interleaved=True,
                              restart_interval=restart_interval, huffman=huffman)[0]


def encode_resized_batch(t, quality: int = 0, subsampling: int = _j.SUBSAMPLE_420, size=None, layout="chw", restart_interval=None,
                         huffman: str = "standard") -> list:
    """jpegamd.encode_resized_batch's uint8 pictures, each resized to size = (out_width, out_height) -> N one-scan files through
    jpegamd_encode_resized_interleaved_batch_async: byte for byte encode_tensor_batch's files of the resized bytes.  restart_interval
    counts MCUs of the RESIZED picture ("row": one of its MCU rows).  One channel (layout="gray") or subsampling 0: the grayscale file
    of encode_gray_batch."""
    return _j._encode_resized("encode_resized_batch", t, quality, subsampling, size, layout, False, interleaved=True,
                              restart_interval=restart_interval, huffman=huffman)


def encode_resized(t, quality: int = 0, subsampling: int = _j.SUBSAMPLE_420, size=None, layout="chw", restart_interval=None,
                   huffman: str = "standard") -> bytes:
    """One picture of bytes -> its resized one-scan file, as encode_resized_batch."""
    return _j._encode_resized("encode_resized", t, quality, subsampling, size, layout, True, interleaved=True,
                              restart_interval=restart_interval, huffman=huffman)[0]
