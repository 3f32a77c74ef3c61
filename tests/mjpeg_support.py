"""What the suites of the one-scan files from every source share (test_mjpeg_host.py, test_gpu_mjpeg.py) -- TEST INFRASTRUCTURE ONLY:
the kinds of YCbCr input, stored samples for each, the planes the header's maps make of them (depth_model, range_model, matrix_model, in
that order), the expected files (interleaved_model / restart_model over those planes), and the calls of the three new C entries queued
on a context."""
from __future__ import annotations

import ctypes as C
import io
from dataclasses import dataclass

import numpy as np
import pytest

import color_model as cm
import color_model_422 as m422
import depth_model as dm
import gpu_support as gs
import interleaved_model as im
from interleaved_model import row_interval                      # noqa: F401  (the suites take it from here)
import matrix_model as mm
import range_model as rgm
import restart_model as rsm
import scan_model as sm
from color_model import synth_rgb
from gpu_support import CBCR, CRCB, PLANES, S420, S422, S444, UYVY, YUYV  # noqa: F401

SUBS = (S444, S420, S422)
# TileSource::layout (jpegamd_internal.h)
SRC_RGB, SRC_PLANE, SRC_PX4, SRC_PLANAR, SRC_PAIR, SRC_QUAD, SRC_PLANE16, SRC_PAIR16 = range(8)
# (layout, chroma tables, expand) of the stage-tap instantiations: what the one-scan path had, and what every other source needs
OLD_TAPS = {(SRC_RGB, 0, 0), (SRC_PLANE, 0, 0), (SRC_PLANE, 1, 0), (SRC_PAIR, 1, 0)}
NEW_TAPS = {(SRC_PX4, 0, 0), (SRC_PLANAR, 0, 0), (SRC_PAIR, 0, 0), (SRC_PAIR, 0, 1), (SRC_PLANE, 0, 1), (SRC_PLANE16, 0, 0), (SRC_PLANE16, 0, 1),
            (SRC_PLANE, 1, 1), (SRC_PAIR, 1, 1), (SRC_QUAD, 1, 0), (SRC_QUAD, 1, 1), (SRC_PLANE16, 1, 0), (SRC_PLANE16, 1, 1),
            (SRC_PAIR16, 1, 0), (SRC_PAIR16, 1, 1)}


@dataclass(frozen=True)
class Kind:
    """One kind of YCbCr samples: 8-bit (align None) or 10-bit words ("msb" / "lsb"), either range, either matrix."""
    name: str
    align: str | None = None
    limited: bool = False
    bt709: bool = False

    def args(self, j):
        """-> (sample_range, sample_format, matrix) of the C entries."""
        fmt = j.SAMPLES_8 if self.align is None else (j.SAMPLES_10_MSB if self.align == "msb" else j.SAMPLES_10_LSB)
        return (j.RANGE_LIMITED if self.limited else j.RANGE_FULL), fmt, (j.MATRIX_BT709 if self.bt709 else j.MATRIX_BT601)

    def binding(self):
        """-> the keywords of the jpegamd / jpegamd.mjpeg functions."""
        kw = dict(sample_range="limited" if self.limited else "full", matrix="bt709" if self.bt709 else "bt601")
        if self.align:
            kw["align"] = self.align
        return kw


FULL8 = Kind("full8")
LIMITED8 = Kind("limited8", limited=True)
MSB10 = Kind("msb10", "msb")
LSB10 = Kind("lsb10", "lsb")
LIMITED10 = Kind("limited10", "msb", True)
KINDS = (LIMITED8, MSB10, LSB10, LIMITED10)
FULL8_709 = Kind("full8-709", bt709=True)
LIMITED8_709 = Kind("limited8-709", limited=True, bt709=True)
LIMITED10_709 = Kind("limited10-709", "msb", True, True)


def derived_planes(rgb, sub):
    """(y, cb, cr) as the RGB entries derive them at `sub`."""
    return tuple(np.ascontiguousarray(p) for p in sm.planes_of(rgb, sub))


def stored_planes(kind: Kind, w, h, sub, seed, smooth=None):
    """(y, cb, cr) as a source of `kind` stores them: uint8, or uint16 words.  Noise over the whole range of the storage -- below and above
    the nominal range, words above 1023, non-zero low bits -- or (smooth: 200 x 120 pictures, small files) photo-like content of which
    every fifth sample is such noise.  BT.709 kinds get chroma far from grey, so that the matrix moves every plane."""
    rng = np.random.default_rng(seed)
    smooth = (w * h > 4096) if smooth is None else smooth
    base = derived_planes(synth_rgb(w, h, seed % 997 + 1), sub) if smooth else None
    out = []
    for k, shape in enumerate(((h, w),) + (gs.chroma_dims(w, h, sub)[::-1],) * 2):
        if kind.align is None:
            p = rng.integers(0, 256, shape, np.uint8)
            if smooth:
                p = np.where(rng.integers(0, 5, shape) == 0, p, base[k])
        else:
            v = rng.integers(0, 1024, shape, np.uint16)
            if smooth:
                v = np.where(rng.integers(0, 5, shape) == 0, v, (base[k].astype(np.uint16) << 2) | rng.integers(0, 4, shape, np.uint16))
            if kind.align == "msb":
                p = (v << 6) | rng.integers(0, 64, shape, np.uint16)
            else:
                p = np.where(rng.integers(0, 7, shape) == 0, rng.integers(1024, 65536, shape, np.uint16), v)     # larger words clamp to 1023
        out.append(np.ascontiguousarray(p.astype(np.uint8 if kind.align is None else np.uint16)))
    return tuple(out)


def mapped_planes(kind: Kind, planes, sub):
    """The 8-bit full-range BT.601 planes the file is built from: the depth map, the range map, the matrix map, in that order."""
    if kind.align is not None:
        p = dm.narrow(planes, dm.LIMITED if kind.limited else dm.FULL, kind.align)
    else:
        p = rgm.expand(planes) if kind.limited else planes
    if kind.bt709:
        p = mm.convert(p, sub)
    return tuple(np.ascontiguousarray(x) for x in p)


def ycc_model(oracle, planes8, q, sub, ri=0):
    """The one-scan file of 8-bit full-range BT.601 planes: interleaved_model's, or restart_model's for ri > 0."""
    if ri:
        return cm.memo(rsm.restart_ycbcr_file, oracle, *planes8, q, sub, ri)
    return cm.memo(im.interleaved_ycbcr_file, oracle, *planes8, q, sub)


def rgb_model(oracle, rgb, q, sub, ri=0):
    if ri:
        return cm.memo(rsm.restart_file, oracle, rgb, q, sub, ri)
    return cm.memo(im.interleaved_file, oracle, rgb, q, sub)


def three_scan_model(oracle, planes8, q, sub):
    return gs.ycc_file(oracle, planes8, q, sub)


def decode(data: bytes) -> np.ndarray:
    image = pytest.importorskip("PIL.Image")
    with image.open(io.BytesIO(data)) as f:
        return np.asarray(f.convert("RGB"))


# ---- calls queued on a context --------------------------------------------------------------------------------------------------------
class OneScan:
    """An Encoder as gpu_support.YccBatch sees it: every YCbCr call goes to jpegamd_encode_ycbcr_interleaved_matrix_batch_async with this
    matrix and restart interval."""

    def __init__(self, jpegamd, enc, matrix, ri):
        self.jpegamd, self.enc, self.matrix, self.ri = jpegamd, enc, matrix, ri

    def encode_ycbcr_batch_async(self, imgs, subsampling, out_ptrs, out_cap, size_ptrs, stream=0, sample_range=0, sample_format=0):
        self.enc.encode_ycbcr_interleaved_matrix_batch_async(imgs, subsampling, sample_range, sample_format, self.matrix, self.ri, out_ptrs,
                                                             out_cap, size_ptrs, stream)


def ycc_call(jpegamd, enc, kind: Kind, planes, dev, sub, layout, ri=0, q=0, cap=None, **kw):
    """One batch of stored planes of `kind` through the new YCbCr entry, queued (gpu_support.YccBatch's storage options in kw)."""
    h, w = planes[0][0].shape
    rng, fmt, matrix = kind.args(jpegamd)
    cap = cap if cap is not None else jpegamd.max_jfif_bytes_interleaved_restart(w, h, sub, ri)
    return gs.YccBatch(jpegamd, OneScan(jpegamd, enc, matrix, ri), planes, dev, sub, layout, quality=q, cap=cap, sample_range=rng,
                       sample_format=fmt, **kw)


def ycc_files(jpegamd, enc, kind, planes, dev, sub, layout, ri=0, q=0, **kw):
    return gs.finish_files(enc, ycc_call(jpegamd, enc, kind, planes, dev, sub, layout, ri, q, **kw))


_fourth = np.random.default_rng(77)


def px4_rows(rgb, bottom_up, bgra):
    """[H, 4 W]: R, G, B, x (or B, G, R, x), a random fourth byte in every pixel."""
    s = rgb[::-1] if bottom_up else rgb
    if bgra:
        s = s[:, :, ::-1]
    return np.concatenate([s, _fourth.integers(0, 256, s.shape[:2] + (1,), np.uint8)], axis=2).reshape(s.shape[0], -1)


class PixelsCall(gs.Outputs):
    """One batch through jpegamd_encode_color_interleaved_pixels_batch_async: order "rgb" / "bgr" / "rgba" / "bgra"."""

    def __init__(self, jpegamd, enc, rgbs, dev, sub, order="rgba", ri=0, q=0, bottom_up=False, stride=None, shift=0, cap=None):
        h, w, _ = rgbs[0].shape
        px4 = order in ("rgba", "bgra")
        blue = order in ("bgr", "bgra")
        stride = stride or (4 if px4 else 3) * w
        rows = [px4_rows(r, bottom_up, blue) if px4 else gs.stored_rows(r, bottom_up, blue) for r in rgbs]
        self.px = [gs.upload(r, dev, stride, shift) for r in rows]
        super().__init__(dev, len(rgbs), cap if cap is not None else jpegamd.max_jfif_bytes_interleaved_restart(w, h, sub, ri))
        code = {"rgb": jpegamd.ORDER_RGB, "bgr": jpegamd.ORDER_BGR, "rgba": jpegamd.ORDER_RGBA, "bgra": jpegamd.ORDER_BGRA}[order]
        imgs = [jpegamd.Encoder.image(ptr, w, h, stride, bottom_up, code, q) for _, ptr in self.px]
        enc.encode_color_interleaved_pixels_batch_async(imgs, sub, ri, self.out_ptrs, self.cap, self.size_ptrs, gs.stream())


class PlanarCall(gs.Outputs):
    """One batch through jpegamd_encode_planar_interleaved_batch_async: three allocations per picture, plane k `shifts[k]` bytes in."""

    def __init__(self, jpegamd, enc, rgbs, dev, sub, ri=0, q=0, bottom_up=False, stride=None, shifts=(0, 0, 0)):
        h, w, _ = rgbs[0].shape
        stride = stride or w
        self.px, imgs = [], []
        for rgb in rgbs:
            s = rgb[::-1] if bottom_up else rgb
            ups = [gs.upload(np.ascontiguousarray(s[:, :, k]), dev, stride, shifts[k]) for k in range(3)]
            self.px.append(ups)
            imgs.append(jpegamd.Encoder.planar_image(tuple(p for _, p in ups), w, h, stride, bottom_up, q))
        super().__init__(dev, len(rgbs), jpegamd.max_jfif_bytes_interleaved_restart(w, h, sub, ri))
        enc.encode_planar_interleaved_batch_async(imgs, sub, ri, self.out_ptrs, self.cap, self.size_ptrs, gs.stream())


class OldYccCall(gs.Outputs):
    """8-bit full-range BT.601 planes through the EXISTING one-scan entry (jpegamd_encode_ycbcr_interleaved_restart_batch_async)."""

    def __init__(self, jpegamd, enc, planes, dev, sub, layout, ri=0, q=0):
        h, w = planes[0][0].shape
        cw, _ = gs.chroma_dims(w, h, sub)
        c_stride = cw if layout == PLANES else 2 * cw
        self.keep, imgs = [], []
        for y, cb, cr in planes:
            ty, py = gs.upload(y, dev, w)
            ups = [gs.upload(rows, dev, c_stride) for rows in cm.chroma_rows(cb, cr, layout)]
            self.keep.append((ty, ups))
            imgs.append(jpegamd.Encoder.ycbcr_image(py, ups[0][1], ups[1][1] if layout == PLANES else 0, w, h, w, c_stride, layout, q))
        super().__init__(dev, len(planes), jpegamd.max_jfif_bytes_interleaved_restart(w, h, sub, ri))
        enc.encode_ycbcr_interleaved_restart_batch_async(imgs, sub, ri, self.out_ptrs, self.cap, self.size_ptrs, gs.stream())


class OldRgbCall(gs.Outputs):
    """Packed RGB pictures through the EXISTING one-scan entry (jpegamd_encode_color_interleaved_restart_batch_async)."""

    def __init__(self, jpegamd, enc, rgbs, dev, sub, ri=0, q=0):
        h, w, _ = rgbs[0].shape
        self.px = [gs.upload(gs.stored_rows(r, False), dev, 3 * w) for r in rgbs]
        super().__init__(dev, len(rgbs), jpegamd.max_jfif_bytes_interleaved_restart(w, h, sub, ri))
        imgs = [jpegamd.Encoder.image(ptr, w, h, 3 * w, False, jpegamd.ORDER_RGB, q) for _, ptr in self.px]
        enc.encode_color_interleaved_restart_batch_async(imgs, sub, ri, self.out_ptrs, self.cap, self.size_ptrs, gs.stream())


# ---- host-only calls: a context that is never read ------------------------------------------------------------------------------------
def fake_context():
    """A block of zeros where the context would be: a check that came too late would read it."""
    fake = (C.c_uint8 * (1 << 16))()
    return fake, C.cast(fake, C.c_void_p)


def out_arrays(n=4):
    return (C.c_void_p * n)(*([C.c_void_p(0x1000)] * n)), (C.c_void_p * n)(*([C.c_void_p(0x2000)] * n))


def call_ycc(jpegamd, ctx, imgs, sub, rng=0, fmt=0, matrix=0, ri=0, count=None, outs=True):
    arr = (jpegamd.YCbCrImage * max(len(imgs), 1))(*imgs) if imgs is not None else None
    out_arr, size_arr = out_arrays() if outs else (None, None)
    return jpegamd.lib.jpegamd_encode_ycbcr_interleaved_matrix_batch_async(ctx, arr, len(imgs) if count is None else count, sub, rng, fmt, matrix,
                                                                           ri, out_arr, 1 << 20, size_arr, None)


def call_pixels(jpegamd, ctx, imgs, sub, ri=0, count=None, outs=True):
    arr = (jpegamd.Image * max(len(imgs), 1))(*imgs) if imgs is not None else None
    out_arr, size_arr = out_arrays() if outs else (None, None)
    return jpegamd.lib.jpegamd_encode_color_interleaved_pixels_batch_async(ctx, arr, len(imgs) if count is None else count, sub, ri, out_arr,
                                                                           1 << 20, size_arr, None)


def call_planar(jpegamd, ctx, imgs, sub, ri=0, count=None, outs=True):
    arr = (jpegamd.PlanarImage * max(len(imgs), 1))(*imgs) if imgs is not None else None
    out_arr, size_arr = out_arrays() if outs else (None, None)
    return jpegamd.lib.jpegamd_encode_planar_interleaved_batch_async(ctx, arr, len(imgs) if count is None else count, sub, ri, out_arr, 1 << 20,
                                                                     size_arr, None)
