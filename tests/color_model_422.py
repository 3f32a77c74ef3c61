"""CPU model of the 4:2:2 colour file (include/jpeg_compression.h) -- TEST INFRASTRUCTURE ONLY.

The file is color_model's with one byte changed and other planes: component 1 of SOF0 carries the sampling factors 0x21, and the
chroma planes are ceil(W / 2) x H (scan_model.chroma_planes at SUB_422).  Everything else is built from color_model's pieces."""
from __future__ import annotations

import numpy as np

import color_model as cm
import scan_model as sm
from scan_model import SUB_422                                  # noqa: F401  (JPEGAMD_SUBSAMPLE_422)

YUYV, UYVY = 4, 5                                               # JPEGAMD_CHROMA_YUYV / _UYVY


def prefix_422(w: int, h: int, quality: int) -> bytes:
    """The 4:4:4 colour prefix with the Y sampling byte of SOF0 set to 0x21."""
    p = bytearray(cm.color_prefix(w, h, quality, cm.SUB_444))
    sof = p.index(b"\xff\xc0")
    at = sof + 2 + 2 + 1 + 2 + 2 + 1 + 1                        # marker, length, precision, height, width, count, component id
    assert p[at - 1] == 1 and p[at] == 0x11
    p[at] = 0x21
    return bytes(p)


def color_file_422(oracle, bmp: bytes, quality: int = 0) -> bytes:
    """The whole 4:2:2 colour file the library must write for this BMP."""
    rgb = cm.read_bmp_rgb(bmp)
    h, w, _ = rgb.shape
    return sm.three_scans(oracle, prefix_422(w, h, quality), cm.gray_scan(oracle, bmp, quality), *sm.chroma_planes(rgb, SUB_422), quality)


def ycbcr_file_422(oracle, y: np.ndarray, cb: np.ndarray, cr: np.ndarray, quality: int = 0) -> bytes:
    """The 4:2:2 file of samples that already are Y, Cb and Cr: coded as given."""
    h, w = y.shape
    assert cb.shape == cr.shape == (h, (w + 1) // 2), (y.shape, cb.shape, cr.shape)
    y_scan = cm.gray_scan(oracle, cm.write_bmp(np.stack([y, y, y], axis=2)), quality)
    return sm.three_scans(oracle, prefix_422(w, h, quality), y_scan, cb, cr, quality)


def pack_yuyv(y: np.ndarray, cb: np.ndarray, cr: np.ndarray, order: str = "yuyv", poison: int = 0x5A) -> np.ndarray:
    """The packed rows of one picture: uint8 [H, 4 ceil(W / 2)], groups Y0 Cb Y1 Cr ("yuyv") or Cb Y0 Cr Y1 ("uyvy").  For odd W the
    last group's second Y byte is `poison`: a value the encoder must never read."""
    h, w = y.shape
    cw = (w + 1) // 2
    ys = np.full((h, 2 * cw), poison, np.uint8)
    ys[:, :w] = y
    out = np.zeros((h, cw, 4), np.uint8)
    iy, icb, icr = ((0, 2), 1, 3) if order == "yuyv" else ((1, 3), 0, 2)
    out[:, :, iy[0]], out[:, :, iy[1]] = ys[:, 0::2], ys[:, 1::2]
    out[:, :, icb], out[:, :, icr] = cb, cr
    return out.reshape(h, 4 * cw)
