"""Progressive files (SOF2) with a scan script of the caller's, and grayscale progressive files: the five functions
of `jpegamd.progressive_successive` with a `scans=` argument, plus `encode_gray_batch` and `encode_gray`.

`scans` is a list of `(components, ss, se, ah, al)` with `components` a tuple of component indices (0 Y, 1 Cb, 2 Cr), or None for
libjpeg's default script (`SUCCESSIVE` for colour files, `GRAY_SUCCESSIVE` for grayscale ones).  `parse_scan_script` reads the text of
a libjpeg `-scans` file into such a list.  The rules a script has to keep are those of T.81 G.1.1.1 (`jpegamd.validate_scan_script`):
a luma-first preview, a split DC scan, a DC-only thumbnail file and more or fewer refinement passes are all valid scripts.  Every scan
carries a table made of its own symbol counts.

Planar R, G, B pictures (layout="chw") are not taken.  The per-device context's Huffman mode is neither read nor changed."""
from __future__ import annotations

import re

import jpegamd as _j

_Y, _CB, _CR, _ALL = (0,), (1,), (2,), (0, 1, 2)
# the built-in scripts: seven scans by spectral selection, libjpeg's jpeg_simple_progression for three components
# (4.6.14) and for one
SPECTRAL = [(_ALL, 0, 0, 0, 0), (_Y, 1, 5, 0, 0), (_CB, 1, 5, 0, 0), (_CR, 1, 5, 0, 0), (_Y, 6, 63, 0, 0), (_CB, 6, 63, 0, 0), (_CR, 6, 63, 0, 0)]
SUCCESSIVE = [(_ALL, 0, 0, 0, 1), (_Y, 1, 5, 0, 2), (_CR, 1, 63, 0, 1), (_CB, 1, 63, 0, 1), (_Y, 6, 63, 0, 2), (_Y, 1, 63, 2, 1),
              (_ALL, 0, 0, 1, 0), (_CR, 1, 63, 1, 0), (_CB, 1, 63, 1, 0), (_Y, 1, 63, 1, 0)]
GRAY_SUCCESSIVE = [(_Y, 0, 0, 0, 1), (_Y, 1, 5, 0, 2), (_Y, 6, 63, 0, 2), (_Y, 1, 63, 2, 1), (_Y, 0, 0, 1, 0), (_Y, 1, 63, 1, 0)]


def parse_scan_script(text: str) -> list:
    """The text of a libjpeg `-scans` file -> [(components, ss, se, ah, al)].  A scan is `0,1,2: 0-0, 0, 1 ;` -- component indices
    separated by spaces or commas, a colon, `Ss-Se, Ah, Al` (commas or spaces), a semicolon; `#` starts a comment.  The colon-less form
    (a sequential scan: components alone) and anything else is a ValueError.  Whether the scans form a valid script is
    jpegamd.validate_scan_script's to say."""
    if not isinstance(text, str):
        raise ValueError("a scan script is text")
    body = "\n".join(line.split("#", 1)[0] for line in text.splitlines())
    parts = body.split(";")
    if parts[-1].strip():
        raise ValueError(f"scan {len(parts) - 1}: no ';' behind {parts[-1].strip()!r}")
    scans = []
    for k, part in enumerate(parts[:-1]):
        if ":" not in part:
            raise ValueError(f"scan {k}: {part.strip()!r} has no ':' -- a sequential scan has no place in a progressive script")
        left, right = part.split(":", 1)
        m = re.fullmatch(r"\s*(\d+)\s*-\s*(\d+)\s*[,\s]\s*(\d+)\s*[,\s]\s*(\d+)\s*", right)
        comps = re.fullmatch(r"\s*\d+(?:\s*[,\s]\s*\d+)*\s*", left)
        if not m or not comps:
            raise ValueError(f"scan {k}: cannot read {part.strip()!r}")
        scans.append((tuple(int(c) for c in re.findall(r"\d+", left)),) + tuple(int(v) for v in m.groups()))
    if not scans:
        raise ValueError("the script has no scan")
    return scans


def _own(scans):
    return _j.ProgressiveScript(scans)


def encode_ycbcr_batch(y, cb, cr=None, quality: int = 0, subsampling: int = _j.SUBSAMPLE_420, order: str = "cbcr",
                       sample_range: str = "full", matrix: str = "bt601", scans=None) -> list:
    """jpegamd.encode_ycbcr_batch's pictures (planes, or pairs with cr=None) -> N files, for either sample_range and matrix, through
    jpegamd_encode_ycbcr_progressive_script_batch_async."""
    rng, mat = _j._sample_range(sample_range), _j._matrix(matrix)
    return _j._encode_ycbcr_planes("encode_ycbcr_batch", _j._ycbcr_layout, y, cb, cr, quality, subsampling, order, None, rng, matrix=mat,
                                   interleaved=True, any_kind=True, progressive=_own(scans))


def encode_ycbcr16_batch(y, cb, cr=None, quality: int = 0, subsampling: int = _j.SUBSAMPLE_420, order: str = "cbcr",
                         sample_range: str = "full", align: str = "msb", matrix: str = "bt601", scans=None) -> list:
    """jpegamd.encode_ycbcr16_batch's pictures (10-bit samples in 16-bit words: P010 / I010 families) -> N files."""
    rng, mat = _j._sample_range(sample_range), _j._matrix(matrix)
    if not isinstance(align, str) or align not in ("msb", "lsb"):
        raise ValueError(f'align must be "msb" or "lsb", not {align!r}')
    return _j._encode_ycbcr_planes("encode_ycbcr16_batch", _j._ycbcr16_layout, y, cb, cr, quality, subsampling, order, None, rng,
                                   _j.SAMPLES_10_MSB if align == "msb" else _j.SAMPLES_10_LSB, mat, interleaved=True, any_kind=True,
                                   progressive=_own(scans))


def encode_yuyv_batch(frames, quality: int = 0, order: str = "yuyv", sample_range: str = "full", matrix: str = "bt601", scans=None) -> list:
    """jpegamd.encode_yuyv_batch's packed 4:2:2 frames (YUY2 / UYVY) -> N files at SUBSAMPLE_422."""
    rng, mat = _j._sample_range(sample_range), _j._matrix(matrix)
    return _j._encode_yuyv_frames(frames, quality, order, None, rng, mat, interleaved=True, any_kind=True, progressive=_own(scans))


def encode_tensor_batch(t, quality: int = 0, subsampling: int = _j.SUBSAMPLE_420, layout=None, scans=None) -> list:
    """jpegamd.encode_tensor_batch's packed colour pictures -> N files: [N, H, W, 3], or layout= "rgba" / "bgra" [N, H, W, 4], "hwc".
    [N, H, W] grayscale pictures (encode_gray_batch takes them), subsampling 0 and layout="chw" are ValueErrors."""
    return _j.encode_tensor_batch(t, quality, subsampling, layout, scan="interleaved", _any_layout=True, _progressive=_own(scans))


def encode_tensor(t, quality: int = 0, subsampling: int = _j.SUBSAMPLE_420, layout=None, scans=None) -> bytes:
    """One colour picture -> its file: [H, W, 3], or layout= "rgba" / "bgra" [H, W, 4], "hwc"."""
    return _j.encode_tensor_batch(t, quality, subsampling, "hwc" if layout is None else layout, _single=True, scan="interleaved",
                                  _any_layout=True, _progressive=_own(scans))[0]


def encode_gray_batch(t, quality: int = 0, scans=None) -> list:
    """A uint8 DEVICE tensor [N, H, W] of luma planes -> N grayscale progressive files through
    jpegamd_encode_gray_progressive_script_batch_async.  Pictures and rows may be strided, pixels within a row must be packed."""
    if t.dim() != 3:
        raise ValueError("encode_gray_batch takes [N, H, W]")
    n, h, w, stride, order = _j._batch_tensor_layout(t)
    if not t.is_cuda:
        raise ValueError("encode_gray_batch needs a device tensor")
    cap = _j.max_jfif_bytes_progressive_script(w, h, 0, scans)
    if not cap:
        _j.validate_scan_script(scans if scans is not None else GRAY_SUCCESSIVE, 1)
        raise ValueError("bad dimensions")

    def queue(enc, b0, k, outs, cap, size_ptrs, stream):
        imgs = [_j.Encoder.image(t[b0 + i].data_ptr(), w, h, stride, bottom_up=False, channel_order=order, quality=quality) for i in range(k)]
        enc.encode_gray_progressive_script_batch_async(imgs, scans, outs, cap, size_ptrs, stream)

    return _j._encode_pictures(t.device, n, h, w, cap, queue, None)


def encode_gray(t, quality: int = 0, scans=None) -> bytes:
    """One luma plane [H, W] -> its grayscale progressive file."""
    if t.dim() != 2:
        raise ValueError("encode_gray takes [H, W]")
    return encode_gray_batch(t[None], quality, scans)[0]


def encode_float_batch(t, quality: int = 0, subsampling: int = _j.SUBSAMPLE_420, layout="chw", value_range=(0.0, 1.0), scans=None) -> list:
    """jpegamd.encode_float_batch's float32 / float16 / bfloat16 pictures -> N progressive files through
    jpegamd_encode_float_progressive_script_batch_async: byte for byte encode_tensor_batch's files of the bytes of the samples.  One
    channel (layout="gray") or subsampling 0: the grayscale progressive file of encode_gray_batch."""
    return _j._encode_float("encode_float_batch", t, quality, subsampling, layout, value_range, False, progressive=True, scans=scans)


def encode_float(t, quality: int = 0, subsampling: int = _j.SUBSAMPLE_420, layout="chw", value_range=(0.0, 1.0), scans=None) -> bytes:
    """One float picture -> its progressive file, as encode_float_batch."""
    return _j._encode_float("encode_float", t, quality, subsampling, layout, value_range, True, progressive=True, scans=scans)[0]


def encode_reduced_batch(t, quality: int = 0, subsampling: int = _j.SUBSAMPLE_420, factor: int = 2, layout="chw", scans=None) -> list:
    """jpegamd.encode_reduced_batch's uint8 pictures, each reduced by `factor` both ways -> N progressive files through
    jpegamd_encode_reduced_progressive_script_batch_async: byte for byte encode_tensor_batch's files of the reduced bytes.  One channel
    (layout="gray") or subsampling 0: the grayscale progressive file of encode_gray_batch."""
    return _j._encode_reduced("encode_reduced_batch", t, quality, subsampling, factor, layout, False, progressive=True, scans=scans)


def encode_reduced(t, quality: int = 0, subsampling: int = _j.SUBSAMPLE_420, factor: int = 2, layout="chw", scans=None) -> bytes:
    """One picture of bytes -> its reduced progressive file, as encode_reduced_batch."""
    return _j._encode_reduced("encode_reduced", t, quality, subsampling, factor, layout, True, progressive=True, scans=scans)[0]


def encode_resized_batch(t, quality: int = 0, subsampling: int = _j.SUBSAMPLE_420, size=None, layout="chw", scans=None) -> list:
    """jpegamd.encode_resized_batch's uint8 pictures, each resized to size = (out_width, out_height) -> N progressive files through
    jpegamd_encode_resized_progressive_script_batch_async: byte for byte encode_tensor_batch's files of the resized bytes.  One channel
    (layout="gray") or subsampling 0: the grayscale progressive file of encode_gray_batch."""
    return _j._encode_resized("encode_resized_batch", t, quality, subsampling, size, layout, False, progressive=True, scans=scans)


def encode_resized(t, quality: int = 0, subsampling: int = _j.SUBSAMPLE_420, size=None, layout="chw", scans=None) -> bytes:
    """One picture of bytes -> its resized progressive file, as encode_resized_batch."""
    return _j._encode_resized("encode_resized", t, quality, subsampling, size, layout, True, progressive=True, scans=scans)[0]
