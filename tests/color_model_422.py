"""CPU model of the 4:2:2 colour file (include/jpeg_compression.h) -- TEST INFRASTRUCTURE ONLY.

The file is color_model's with one byte changed and other planes: component 1 of SOF0 carries the sampling factors 0x21, and the
chroma planes are ceil(W / 2) x H -- (a + b + 1) >> 1 over the two pixels 2x, 2x + 1 of one row, the last column replicated, no
vertical filter.  Everything else is built from color_model's pieces."""
from __future__ import annotations

import numpy as np

import color_model as cm

SUB_422 = 4                                                     # JPEGAMD_SUBSAMPLE_422
YUYV, UYVY = 4, 5                                               # JPEGAMD_CHROMA_YUYV / _UYVY


def chroma_dims_422(w: int, h: int):
    return (w + 1) // 2, h


def chroma_planes_422(rgb: np.ndarray):
    """The spec's integer Cb / Cr planes at 4:2:2: uint8 [H, ceil(W / 2)] each."""
    cb, cr = (p.astype(np.int64) for p in cm.chroma_planes(rgb, cm.SUB_444))       # cbcr() per pixel
    w = cb.shape[1]
    xs = np.arange(0, w, 2)
    x1 = np.minimum(xs + 1, w - 1)
    return tuple(((p[:, xs] + p[:, x1] + 1) >> 1).astype(np.uint8) for p in (cb, cr))


def luma_plane(rgb: np.ndarray) -> np.ndarray:
    r, g, b = (rgb[:, :, i].astype(np.int64) for i in range(3))
    return ((77 * r + 150 * g + 29 * b) >> 8).astype(np.uint8)


def prefix_422(w: int, h: int, quality: int) -> bytes:
    """The 4:4:4 colour prefix with the Y sampling byte of SOF0 set to 0x21."""
    p = bytearray(cm.color_prefix(w, h, quality, cm.SUB_444))
    sof = p.index(b"\xff\xc0")
    at = sof + 2 + 2 + 1 + 2 + 2 + 1 + 1                        # marker, length, precision, height, width, count, component id
    assert p[at - 1] == 1 and p[at] == 0x11
    p[at] = 0x21
    return bytes(p)


def _file(oracle, w, h, quality, y_scan: bytes, cb: np.ndarray, cr: np.ndarray) -> bytes:
    cq = cm.scaled_table(cm.CHROMA_Q, quality)
    parts = [prefix_422(w, h, quality), y_scan]
    for comp, plane in ((2, cb), (3, cr)):
        parts += [cm.sos(comp), cm.pack_scan(oracle, cm.plane_zigzag(oracle, plane, cq), True)]
    return b"".join(parts) + b"\xff\xd9"


def color_file_422(oracle, bmp: bytes, quality: int = 0) -> bytes:
    """The whole 4:2:2 colour file the library must write for this BMP."""
    rgb = cm.read_bmp_rgb(bmp)
    h, w, _ = rgb.shape
    cb, cr = chroma_planes_422(rgb)
    return _file(oracle, w, h, quality, cm.gray_scan(oracle, bmp, quality), cb, cr)


def ycbcr_file_422(oracle, y: np.ndarray, cb: np.ndarray, cr: np.ndarray, quality: int = 0) -> bytes:
    """The 4:2:2 file of samples that already are Y, Cb and Cr: coded as given."""
    h, w = y.shape
    assert cb.shape == cr.shape == (h, (w + 1) // 2), (y.shape, cb.shape, cr.shape)
    y_scan = cm.gray_scan(oracle, cm.write_bmp(np.stack([y, y, y], axis=2)), quality)
    return _file(oracle, w, h, quality, y_scan, cb, cr)


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
