"""The one-scan files from every source, on the CPU: that every kind of input has its stage-tap instantiation of the tile kernel
(jpegamd_debug_tile_variant over jpegamd_debug_ycbcr_sources), the argument checks of the three new C entries in front of a context that
is never read, the checks of jpegamd.mjpeg on host tensors, that the inputs of the GPU suite (tests/test_gpu_mjpeg.py) exercise what
they claim to, and an independent decoder over the model's files.  Nothing here needs a device."""
from __future__ import annotations

import ctypes as C
import itertools

import numpy as np
import pytest

import interleaved_model as im
import mjpeg_support as ms
from mjpeg_support import CBCR, CRCB, PLANES, S420, S422, S444, SUBS, UYVY, YUYV

ERR_ARG = -1
NAMES = ("jpegamd_encode_ycbcr_interleaved_matrix_batch_async", "jpegamd_encode_color_interleaved_pixels_batch_async",
         "jpegamd_encode_planar_interleaved_batch_async")


def variant(jpegamd, taps, src):
    return jpegamd.lib.jpegamd_debug_tile_variant(taps, *src)


# ---- the instantiations -----------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_documented(jpegamd):
    header = jpegamd.HEADER_PATH.read_text()
    lib = C.CDLL(str(jpegamd.LIB_PATH))
    for name in NAMES:
        assert name in jpegamd.EXPORTED and hasattr(lib, name) and name in header, name
        assert hasattr(jpegamd.Encoder, name[len("jpegamd_"):])
    assert hasattr(lib, "jpegamd_debug_tile_variant")
    assert "jpegamd_debug_tile_variant" not in header and "jpegamd_debug_tile_variant" not in jpegamd.EXPORTED


def test_every_kind_of_input_has_its_tap_instantiation(jpegamd):
    seen = set()
    kinds = 0
    for layout, fmt, rng, first in itertools.product((PLANES, CBCR, CRCB, YUYV, UYVY), (0, 1, 2), (0, 1), (0, 1)):
        out = (C.c_uint32 * 8)()
        rc = jpegamd.lib.jpegamd_debug_ycbcr_sources(layout, fmt, rng, first, out)
        if layout in (YUYV, UYVY) and fmt != 0:                     # Y210: refused by the encode entries
            assert rc == ERR_ARG
            continue
        assert rc == 0
        kinds += 1
        for src in (tuple(out[:3]), tuple(out[4:7])):
            assert variant(jpegamd, 1, src) == 1, (layout, fmt, rng, first, src)
            seen.add(src)
    assert kinds == (3 * 3 + 2) * 2 * 2
    for src in ((ms.SRC_RGB, 0, 0), (ms.SRC_PX4, 0, 0), (ms.SRC_PLANAR, 0, 0)):      # the Y launches of the RGB entries
        assert variant(jpegamd, 1, src) == 1, src
        seen.add(src)
    assert len(ms.NEW_TAPS) == 15 and len(ms.OLD_TAPS) == 4 and not (ms.NEW_TAPS & ms.OLD_TAPS)
    assert seen == ms.NEW_TAPS | ms.OLD_TAPS                        # (a BT.709 or an RGB batch reads scratch planes: kSrcPlane, full range)
    every = {(l, c, x) for l in range(-1, 10) for c in (0, 1) for x in (0, 1) if variant(jpegamd, 1, (l, c, x))}
    assert every == ms.NEW_TAPS | ms.OLD_TAPS                       # ... and no others
    # the build without taps is what it was: 19 instantiations
    plain = {(l, c, x) for l in range(-1, 10) for c in (0, 1) for x in (0, 1) if variant(jpegamd, 0, (l, c, x))}
    assert len(plain) == 19 and plain >= {(ms.SRC_RGB, 0, 0), (ms.SRC_PLANE, 0, 0), (ms.SRC_PLANE, 1, 0)}


# ---- argument checks of the three entries -------------------------------------------------------------------------------------------------
W, H = 65, 33


def _ycc(jpegamd, layout=PLANES, w=W, h=H, y_stride=None, c_stride=None, sub=S420, bps=1, y=0x100000, cb=0x800000, cr=0x900000, q=0):
    cw = w if sub == S444 else (w + 1) // 2
    packed = layout in (YUYV, UYVY)
    ys = y_stride if y_stride is not None else (4 * cw if packed else bps * w)
    cs = c_stride if c_stride is not None else bps * (cw if layout == PLANES else 2 * cw)
    return jpegamd.Encoder.ycbcr_image(y, cb, cr, w, h, ys, cs, layout, q)


def test_ycbcr_entry_refuses_before_the_context(jpegamd):
    keep, ctx = ms.fake_context()
    j = jpegamd
    good = [_ycc(j), _ycc(j, y=0x200000)]
    call = lambda imgs, sub=S420, **kw: ms.call_ycc(j, ctx, imgs, sub, **kw)    # noqa: E731
    # null and count
    assert ms.call_ycc(j, None, good, S420) == ERR_ARG
    assert call(None, count=1) == ERR_ARG and call(good, outs=False) == ERR_ARG
    assert call(good, count=0) == ERR_ARG and call(good, count=-1) == ERR_ARG and call(good, count=j.MAX_BATCH + 1) == ERR_ARG
    assert call([_ycc(j, y=0)]) == ERR_ARG and call([_ycc(j, cb=0)]) == ERR_ARG and call([_ycc(j, cr=0)]) == ERR_ARG
    assert call([_ycc(j, w=0)]) == ERR_ARG and call([_ycc(j, h=65536)]) == ERR_ARG
    # a later picture that differs from the first
    for other in (_ycc(j, w=W - 1, y_stride=W), _ycc(j, h=H + 1), _ycc(j, y_stride=W + 4), _ycc(j, c_stride=40), _ycc(j, layout=CBCR, c_stride=33),
                  _ycc(j, q=90), _ycc(j, y=0)):
        assert call([good[0], other]) == ERR_ARG
    # range, format, matrix, subsampling, restart interval
    for kw in (dict(rng=2), dict(rng=-1), dict(fmt=3), dict(fmt=-1), dict(matrix=2), dict(matrix=-1), dict(ri=-1), dict(ri=65536), dict(ri=1 << 30)):
        assert call(good, **kw) == ERR_ARG, kw
    for sub in (0, 3, -1, 8):
        assert call(good, sub) == ERR_ARG
    for ri in (0, 1, 65535):                                         # an interval in range does not rescue another bad argument
        assert call(good, ri=ri, rng=2) == ERR_ARG and ms.call_ycc(j, None, good, S420, ri=ri) == ERR_ARG
    # packed layouts: 4:2:2 alone, one byte per sample alone
    for layout in (YUYV, UYVY):
        for sub in (S420, S444):
            assert call([_ycc(j, layout, sub=S422)], sub) == ERR_ARG
        for fmt in (j.SAMPLES_10_MSB, j.SAMPLES_10_LSB):
            assert call([_ycc(j, layout, sub=S422, y_stride=8 * W)], S422, fmt=fmt) == ERR_ARG
        assert call([_ycc(j, layout, sub=S422, y_stride=4 * 33 - 1)], S422) == ERR_ARG      # 4 ceil(W / 2)
    # strides too short: W and the chroma row in bytes, 2 W for 16-bit samples
    for sub in SUBS:
        cw = W if sub == S444 else (W + 1) // 2
        assert call([_ycc(j, sub=sub, y_stride=W - 1)], sub) == ERR_ARG
        assert call([_ycc(j, sub=sub, c_stride=cw - 1)], sub) == ERR_ARG
        assert call([_ycc(j, CBCR, sub=sub, c_stride=2 * cw - 1)], sub) == ERR_ARG
        for fmt in (j.SAMPLES_10_MSB, j.SAMPLES_10_LSB):
            assert call([_ycc(j, sub=sub, bps=2, y_stride=2 * W - 1)], sub, fmt=fmt) == ERR_ARG
            assert call([_ycc(j, sub=sub, bps=2, c_stride=2 * cw - 1)], sub, fmt=fmt) == ERR_ARG
            assert call([_ycc(j, CRCB, sub=sub, bps=2, c_stride=4 * cw - 1)], sub, fmt=fmt) == ERR_ARG
            assert call([_ycc(j, sub=sub)], sub, fmt=fmt) == ERR_ARG             # the strides of bytes under 16-bit samples


def test_pixels_entry_refuses_before_the_context(jpegamd):
    keep, ctx = ms.fake_context()
    j = jpegamd
    for order, bpp in ((j.ORDER_RGB, 3), (j.ORDER_BGR, 3), (j.ORDER_RGBA, 4), (j.ORDER_BGRA, 4)):
        good = [j.Encoder.image(0x100000 * (i + 1), W, H, bpp * W, False, order, 0) for i in range(2)]
        assert ms.call_pixels(j, None, good, S420) == ERR_ARG
        assert ms.call_pixels(j, ctx, None, S420, count=1) == ERR_ARG and ms.call_pixels(j, ctx, good, S420, outs=False) == ERR_ARG
        for count in (0, -1, j.MAX_BATCH + 1):
            assert ms.call_pixels(j, ctx, good, S420, count=count) == ERR_ARG
        for ri in (-1, 65536):
            assert ms.call_pixels(j, ctx, good, S420, ri) == ERR_ARG
        for sub in (0, 3, -1):
            assert ms.call_pixels(j, ctx, good, sub) == ERR_ARG
        assert ms.call_pixels(j, ctx, [j.Encoder.image(0x100000, W, H, bpp * W - 1, False, order, 0)], S420) == ERR_ARG
        assert ms.call_pixels(j, ctx, [j.Encoder.image(0, W, H, bpp * W, False, order, 0)], S420) == ERR_ARG
        for other in (j.Encoder.image(0x300000, W - 1, H, bpp * W, False, order, 0), j.Encoder.image(0x300000, W, H, bpp * W, True, order, 0),
                      j.Encoder.image(0x300000, W, H, bpp * W, False, order, 75), j.Encoder.image(0, W, H, bpp * W, False, order, 0),
                      j.Encoder.image(0x300000, W, H, 4 * W, False, j.ORDER_RGBA if bpp == 3 else j.ORDER_BGR, 0)):
            assert ms.call_pixels(j, ctx, [good[0], other], S420) == ERR_ARG
    for order in (j.ORDER_GRAY, 5, -1, 0x100):                        # GRAY, unknown orders, the internal planar order
        assert ms.call_pixels(j, ctx, [j.Encoder.image(0x100000, W, H, 4 * W, False, order, 0)], S420) == ERR_ARG


def test_planar_entry_refuses_before_the_context(jpegamd):
    keep, ctx = ms.fake_context()
    j = jpegamd
    planes = (0x100000, 0x200000, 0x300000)
    good = [j.Encoder.planar_image(planes, W, H, W), j.Encoder.planar_image(tuple(p + 0x10000 for p in planes), W, H, W)]
    assert ms.call_planar(j, None, good, S420) == ERR_ARG
    assert ms.call_planar(j, ctx, None, S420, count=1) == ERR_ARG and ms.call_planar(j, ctx, good, S420, outs=False) == ERR_ARG
    for count in (0, -1, j.MAX_BATCH + 1):
        assert ms.call_planar(j, ctx, good, S420, count=count) == ERR_ARG
    for sub in (0, 3, -1):                                           # 0: the grayscale file of the three-scan entry has no one-scan twin
        assert ms.call_planar(j, ctx, good, sub) == ERR_ARG
    for ri in (-1, 65536):
        assert ms.call_planar(j, ctx, good, S420, ri) == ERR_ARG
    assert ms.call_planar(j, ctx, [j.Encoder.planar_image(planes, W, H, W - 1)], S420) == ERR_ARG
    for k in range(3):
        bad = tuple(0 if i == k else p for i, p in enumerate(planes))
        assert ms.call_planar(j, ctx, [j.Encoder.planar_image(bad, W, H, W)], S420) == ERR_ARG
        assert ms.call_planar(j, ctx, [good[0], j.Encoder.planar_image(bad, W, H, W)], S420) == ERR_ARG
    for other in (j.Encoder.planar_image(planes, W + 1, H, W + 1), j.Encoder.planar_image(planes, W, H, W + 4),
                  j.Encoder.planar_image(planes, W, H, W, True), j.Encoder.planar_image(planes, W, H, W, False, 80)):
        assert ms.call_planar(j, ctx, [good[0], other], S420) == ERR_ARG


def test_the_old_entries_still_refuse_what_they_refused(jpegamd):
    keep, ctx = ms.fake_context()
    j = jpegamd
    outs, sizes = (C.c_void_p * 1)(C.c_void_p(0x1000)), (C.c_void_p * 1)(C.c_void_p(0x2000))
    for order in (j.ORDER_GRAY, j.ORDER_RGBA, j.ORDER_BGRA):
        arr = (j.Image * 1)(j.Encoder.image(0x100000, W, H, 4 * W, False, order, 0))
        assert j.lib.jpegamd_encode_color_interleaved_batch_async(ctx, arr, 1, S420, outs, 1 << 20, sizes, None) == ERR_ARG
        assert j.lib.jpegamd_encode_color_interleaved_restart_batch_async(ctx, arr, 1, S420, 2, outs, 1 << 20, sizes, None) == ERR_ARG
    for layout in (YUYV, UYVY):
        arr = (j.YCbCrImage * 1)(_ycc(j, layout, sub=S422))
        assert j.lib.jpegamd_encode_ycbcr_interleaved_batch_async(ctx, arr, 1, S422, outs, 1 << 20, sizes, None) == ERR_ARG
        assert j.lib.jpegamd_encode_ycbcr_interleaved_restart_batch_async(ctx, arr, 1, S422, 2, outs, 1 << 20, sizes, None) == ERR_ARG


# ---- the binding ------------------------------------------------------------------------------------------------------------------------
def _raises(call, device: bool):
    with pytest.raises(ValueError) as err:
        call()
    assert ("device tensor" in str(err.value)) == device, str(err.value)


def test_binding_checks_on_host_tensors(jpegamd):
    torch = pytest.importorskip("torch")
    from jpegamd import mjpeg
    u8, i16 = torch.uint8, torch.int16
    y, cb, cr, pairs = torch.zeros(2, 8, 8, dtype=u8), torch.zeros(2, 4, 4, dtype=u8), torch.zeros(2, 4, 4, dtype=u8), torch.zeros(2, 4, 4, 2, dtype=u8)
    y16, cb16, cr16 = (t.to(i16) for t in (y, cb, cr))
    frames = torch.zeros(2, 8, 8, 2, dtype=u8)
    hwc, chw, rgba, gray = (torch.zeros(2, 8, 8, 3, dtype=u8), torch.zeros(2, 3, 8, 8, dtype=u8), torch.zeros(2, 8, 8, 4, dtype=u8),
                            torch.zeros(2, 8, 8, dtype=u8))
    restarts_bad = (-1, 65536, "column", 1.5, True)
    restarts_good = (None, 0, 1, 65535, "row")
    calls = {
        "ycbcr": lambda **kw: mjpeg.encode_ycbcr_batch(y, cb, cr, **kw),
        "nv12": lambda **kw: mjpeg.encode_ycbcr_batch(y, pairs, **kw),
        "ycbcr16": lambda **kw: mjpeg.encode_ycbcr16_batch(y16, cb16, cr16, **kw),
        "yuyv": lambda **kw: mjpeg.encode_yuyv_batch(frames, **kw),
        "batch": lambda **kw: mjpeg.encode_tensor_batch(hwc, **kw),
        "chw": lambda **kw: mjpeg.encode_tensor_batch(chw, layout="chw", **kw),
        "rgba": lambda **kw: mjpeg.encode_tensor_batch(rgba, layout="rgba", **kw),
        "one": lambda **kw: mjpeg.encode_tensor(hwc[0], **kw),
        "one-bgra": lambda **kw: mjpeg.encode_tensor(rgba[0], layout="bgra", **kw),
    }
    for name, call in calls.items():
        for ri in restarts_bad:
            _raises(lambda: call(restart_interval=ri), False)
        for ri in restarts_good:
            _raises(lambda: call(restart_interval=ri), True)
        with pytest.raises(TypeError):
            call(scan="interleaved")                                 # the module has one kind of file
    for name in ("ycbcr", "nv12", "ycbcr16", "yuyv"):
        for kw in (dict(sample_range="video"), dict(matrix="bt2020"), dict(order="vu")):
            _raises(lambda: calls[name](**kw), False)
        for kw in (dict(sample_range="limited"), dict(matrix="bt709"), dict(sample_range="limited", matrix="bt709", restart_interval="row")):
            _raises(lambda: calls[name](**kw), True)
    _raises(lambda: calls["ycbcr16"](align="middle"), False)
    _raises(lambda: calls["ycbcr16"](align="lsb", sample_range="limited"), True)
    _raises(lambda: calls["nv12"](order="crcb"), True)
    _raises(lambda: calls["yuyv"](order="uyvy"), True)
    _raises(lambda: mjpeg.encode_ycbcr_batch(y, cb16, cr16), False)
    _raises(lambda: mjpeg.encode_ycbcr16_batch(y, cb, cr), False)
    _raises(lambda: mjpeg.encode_ycbcr_batch(y, cb[:, :3], cr[:, :3]), False)
    _raises(lambda: mjpeg.encode_ycbcr_batch(y, cb, cr, subsampling=0), False)
    _raises(lambda: mjpeg.encode_yuyv_batch(torch.zeros(2, 8, 7, 2, dtype=u8)), False)
    # tensors: a one-scan file is a colour file
    _raises(lambda: mjpeg.encode_tensor_batch(gray), False)
    _raises(lambda: mjpeg.encode_tensor(gray[0]), False)
    _raises(lambda: mjpeg.encode_tensor_batch(chw, layout="chw", subsampling=0), False)
    _raises(lambda: mjpeg.encode_tensor_batch(hwc, subsampling=3), False)
    _raises(lambda: mjpeg.encode_tensor_batch(hwc, layout="nhwc"), False)
    _raises(lambda: mjpeg.encode_tensor_batch(hwc, layout="rgba"), False)
    _raises(lambda: mjpeg.encode_tensor_batch(hwc.to(torch.float32)), False)
    for layout, t in (("hwc", hwc), ("chw", chw), ("rgba", rgba), ("bgra", rgba)):
        for sub in SUBS:
            _raises(lambda: mjpeg.encode_tensor_batch(t, subsampling=sub, layout=layout), True)
            _raises(lambda: mjpeg.encode_tensor(t[0], subsampling=sub, layout=layout, restart_interval="row"), True)
    _raises(lambda: mjpeg.encode_tensor_batch([chw[:, k] for k in range(3)], layout="chw"), True)
    # scan="interleaved" on the older functions keeps its refusals
    _raises(lambda: jpegamd.encode_tensor_batch(rgba, layout="rgba", scan="interleaved"), False)
    _raises(lambda: jpegamd.encode_tensor_batch(gray, scan="interleaved"), False)
    _raises(lambda: jpegamd.encode_ycbcr_batch(y, cb, cr, sample_range="limited", scan="interleaved"), False)
    _raises(lambda: jpegamd.encode_ycbcr_batch(y, cb, cr, matrix="bt709", scan="interleaved"), False)


# ---- the inputs of the GPU suite ----------------------------------------------------------------------------------------------------------
SIZES = [(17, 9), (200, 120)]


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("sub", SUBS)
def test_inputs_exercise_what_they_claim(jpegamd, oracle, w, h, sub):
    for kind in ms.KINDS + (ms.LIMITED8_709, ms.FULL8_709, ms.LIMITED10_709):
        stored = ms.stored_planes(kind, w, h, sub, 100 + w)
        y, cb, cr = (p.astype(np.int64) for p in stored)
        if kind.align is None and kind.limited:
            assert y.min() < 16 and y.max() > 235 and min(cb.min(), cr.min()) < 16 and max(cb.max(), cr.max()) > 240
        if kind.align == "lsb":
            assert y.max() > 1023 and max(cb.max(), cr.max()) > 1023
        if kind.align == "msb":
            assert (y & 63).any() and (cb & 63).any() and (cr & 63).any()
        if kind.align is not None and kind.limited:
            v = y >> 6
            assert v.min() < 64 and v.max() > 940
        mapped = ms.mapped_planes(kind, stored, sub)
        assert all(p.dtype == np.uint8 and p.shape == s.shape for p, s in zip(mapped, stored))
        if kind.bt709:
            unmatrixed = ms.mapped_planes(ms.Kind("x", kind.align, kind.limited), stored, sub)
            assert (np.abs(unmatrixed[1].astype(np.int64) - 128) > 16).any() and (np.abs(unmatrixed[2].astype(np.int64) - 128) > 16).any()   # not grey
            assert all(not np.array_equal(a, b) for a, b in zip(mapped, unmatrixed))
        if kind.align is None:
            assert all(not np.array_equal(a, b) for a, b in zip(mapped, stored))
        else:
            truncated = tuple((p >> 8).astype(np.uint8) for p in stored) if kind.align == "msb" else tuple((np.minimum(p, 1023) >> 2).astype(np.uint8) for p in stored)
            assert all(not np.array_equal(a, b) for a, b in zip(mapped, truncated))           # one rounding from ten bits, not a shift
        if (w, h) == (17, 9):
            assert ms.ycc_model(oracle, mapped, 50, sub).pad_blocks == (0 if sub == S444 else 2)
        else:
            assert im.segment_count(w, h, sub) > 1


def test_rgb_inputs(jpegamd, oracle):
    for sub in SUBS:
        assert ms.rgb_model(oracle, ms.synth_rgb(17, 9, 3), 50, sub).pad_blocks == (0 if sub == S444 else 2)
        assert im.segment_count(200, 120, sub) > 1
        hs, vs, bw, bh, mx, my = im.geometry(200, 120, sub)
        assert ms.rsm.seg_mcus(sub) % mx != 0                        # the second segment starts in the middle of an MCU row


# ---- an independent decoder ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ms.KINDS + (ms.FULL8, ms.LIMITED8_709, ms.LIMITED10_709), ids=lambda k: k.name)
def test_decoder_sees_the_pixels_of_the_three_scan_file(jpegamd, oracle, kind):
    for sub, (w, h) in ((S420, (40, 24)), (S422, (18, 9)), (S444, (17, 9))):
        stored = ms.stored_planes(kind, w, h, sub, 7, smooth=True)
        mapped = ms.mapped_planes(kind, stored, sub)
        want = ms.decode(ms.three_scan_model(oracle, mapped, 75, sub))
        assert want.shape == (h, w, 3)
        assert np.array_equal(ms.decode(ms.ycc_model(oracle, mapped, 75, sub).file), want)
        assert np.array_equal(ms.decode(ms.ycc_model(oracle, mapped, 75, sub, ms.row_interval(w, sub)).file), want)
