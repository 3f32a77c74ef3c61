"""Restart intervals in the one-scan colour files on the CPU: the model of the file (tests/restart_model.py) against the model without
restart intervals (rule 5), against an independent decoder and against a structural walk of its scan that does not use the model's
writer; the exported symbols, the size bound, the refusals of the two C entries that return before the context is touched, and the
binding's restart_interval= checks.  Nothing here needs a device."""
from __future__ import annotations

import ctypes as C
import io

import numpy as np
import pytest

import color_model as cm
import color_model_422 as m422
import interleaved_model as im
import restart_model as rm
import scan_model as sm

ERR_ARG = -1
CAP = 1 << 20
SIZES = [(16, 16), (17, 9), (24, 40), (200, 120)]
SUBS = (cm.SUB_444, cm.SUB_420, m422.SUB_422)
NAMES = ("jpegamd_encode_color_interleaved_restart_batch_async", "jpegamd_encode_ycbcr_interleaved_restart_batch_async",
         "jpegamd_max_jfif_bytes_interleaved_restart")
Q = 75


def _picture(jpegamd, w, h, seed=11):
    return cm.read_bmp_rgb(jpegamd.synth_bmp(w, h, seed + w + 3 * h, 0, 0))


def _decode(data: bytes) -> np.ndarray:
    image = pytest.importorskip("PIL.Image")
    with image.open(io.BytesIO(data)) as f:
        return np.asarray(f.convert("RGB"))


def intervals_for(w, h, sub):
    """The issue's intervals: 1, a row, a row and one MCU, a coder segment, a segment and one MCU, the scan, beyond the scan, the largest."""
    _, _, _, _, mx, my = im.geometry(w, h, sub)
    s = rm.seg_mcus(sub)
    return sorted({1, mx, mx + 1, s, s + 1, mx * my, mx * my + 5, 65535})


def _model(oracle, rgb, sub, ri):
    return cm.memo(rm.restart_file, oracle, rgb, Q, sub, ri)


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("w,h", SIZES)
def test_one_interval_is_the_plain_file_with_dri(jpegamd, oracle, w, h, sub):
    """Rule 5, byte for byte, for every Ri >= M."""
    rgb = _picture(jpegamd, w, h)
    plain = cm.memo(im.interleaved_file, oracle, rgb, Q, sub)
    _, _, _, _, mx, my = im.geometry(w, h, sub)
    for ri in (mx * my, mx * my + 5, 65535):
        m = _model(oracle, rgb, sub, ri)
        assert m.file == rm.with_dri(plain.file, ri), ri
        assert (m.intervals, m.markers, m.pad_ff, m.aligned) == (1, 0, 0, 0)
        assert m.stuffed == plain.stuffed and m.scan_bits == plain.scan_bits


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("w,h", SIZES)
def test_model_file_decodes_to_the_pixels_of_the_plain_file(jpegamd, oracle, w, h, sub):
    rgb = _picture(jpegamd, w, h)
    want = _decode(cm.memo(im.interleaved_file, oracle, rgb, Q, sub).file)
    assert want.shape == (h, w, 3)
    for ri in intervals_for(w, h, sub):
        assert np.array_equal(_decode(_model(oracle, rgb, sub, ri).file), want), ri


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("w,h", SIZES)
def test_scan_structure(jpegamd, oracle, w, h, sub):
    """Every 0xFF of the scan is followed by 00, by the expected RSTn in order, or by EOI at the end; n - 1 markers; one DRI in front
    of the one SOS, behind the last DHT."""
    rgb = _picture(jpegamd, w, h)
    _, _, _, _, mx, my = im.geometry(w, h, sub)
    for ri in intervals_for(w, h, sub):
        m = _model(oracle, rgb, sub, ri)
        n = -(-(mx * my) // ri)
        markers, stuffed = sm.walk_scan(m.file, im.SOS3)
        assert markers == [i % 8 for i in range(n - 1)], ri
        assert len(markers) == m.markers == n - 1 == m.intervals - 1
        assert stuffed == m.stuffed
        f = m.file
        at = f.index(im.SOS3)
        assert f.count(b"\xff\xdd") == 1 and f[at - 6:at] == bytes([0xFF, 0xDD, 0, 4, ri >> 8, ri & 0xFF])
        assert f[:at - 6] + f[at:at + 14] == im.prefix(w, h, Q, sub)     # 6 bytes longer, nothing else changed
        last_dht = f.rindex(b"\xff\xc4", 0, at)
        assert last_dht + 2 + int.from_bytes(f[last_dht + 2:last_dht + 4], "big") == at - 6
        assert len(f) <= jpegamd.max_jfif_bytes_interleaved_restart(w, h, sub, ri)


def test_marker_counter_wraps(jpegamd, oracle):
    rgb = _picture(jpegamd, 200, 120)
    m = _model(oracle, rgb, cm.SUB_420, 1)
    markers, _ = sm.walk_scan(m.file, im.SOS3)
    assert len(markers) == 103 >= 9 and markers[:10] == [0, 1, 2, 3, 4, 5, 6, 7, 0, 1] and markers[-1] == 102 % 8


def test_predictors_restart(jpegamd, oracle):
    """A flat picture: with Ri = 1 every MCU codes its first Y block's DC in full and both chroma DCs against 0; the plain scan codes
    them once."""
    flat = np.full((16, 24, 3), 200, np.uint8)
    plain = cm.memo(im.interleaved_file, oracle, flat, 50, cm.SUB_444)
    m = cm.memo(rm.restart_file, oracle, flat, 50, cm.SUB_444, 1)
    assert m.intervals == 6 and m.scan_bits > plain.scan_bits
    first = cm.memo(rm.restart_file, oracle, flat[:8, :8], 50, cm.SUB_444, 1)
    assert m.scan_bits == 6 * first.scan_bits                       # every interval is the one-MCU picture's scan


def test_symbols_are_exported_and_documented(jpegamd):
    header = jpegamd.HEADER_PATH.read_text()
    lib = C.CDLL(str(jpegamd.LIB_PATH))
    for name in NAMES:
        assert name in jpegamd.EXPORTED and hasattr(lib, name) and name in header, name
    assert hasattr(jpegamd.Encoder, "encode_color_interleaved_restart_batch_async")
    assert hasattr(jpegamd.Encoder, "encode_ycbcr_interleaved_restart_batch_async")
    assert callable(jpegamd.max_jfif_bytes_interleaved_restart)
    assert "FF DD 00 04" in header and "JPEGAMD_ERR_TOO_LARGE before anything is allocated or launched" in header


def test_size_bound_matches_its_formula(jpegamd):
    for w, h in SIZES + [(8192, 8192), (65535, 65535), (4000, 17), (1, 1)]:
        for sub in SUBS:
            _, _, _, _, mx, my = im.geometry(w, h, sub)
            plain = jpegamd.max_jfif_bytes_interleaved(w, h, sub)
            assert jpegamd.max_jfif_bytes_interleaved_restart(w, h, sub, 0) == plain > 0
            for ri in (1, 2, mx, mx + 1, mx * my, 65535):
                if ri > 65535:
                    continue
                n = -(-(mx * my) // ri)
                assert jpegamd.max_jfif_bytes_interleaved_restart(w, h, sub, ri) == plain + 6 + 4 * (n - 1), (w, h, sub, ri)
    for ri in (-1, 65536, 1 << 20, -65535):
        assert jpegamd.max_jfif_bytes_interleaved_restart(64, 64, cm.SUB_420, ri) == 0
    for w, h, sub in ((0, 8, 1), (8, 0, 2), (8, 8, 0), (8, 8, 3), (65536, 8, 1)):
        assert jpegamd.max_jfif_bytes_interleaved_restart(w, h, sub, 4) == 0


def test_dense_model_files_fit_the_bound(jpegamd, oracle):
    rgb = np.random.default_rng(7).integers(0, 256, (17, 33, 3), np.uint8)
    for sub in SUBS:
        for ri in (1, 2, 3):
            m = cm.memo(rm.restart_file, oracle, rgb, 100, sub, ri)
            assert len(m.file) <= jpegamd.max_jfif_bytes_interleaved_restart(33, 17, sub, ri)


# ---- refusals that need no device -----------------------------------------------------------------------------------------------------
def _fake_context():
    """A block of zeros where the context would be: a check that came too late would read it."""
    fake = (C.c_uint8 * (1 << 16))()
    return fake, C.cast(fake, C.c_void_p)


def _arrays():
    return (C.c_void_p * 4)(*([C.c_void_p(0x1000)] * 4)), (C.c_void_p * 4)(*([C.c_void_p(0x2000)] * 4))


def _call_rgb(jpegamd, ctx, imgs, sub, ri):
    arr = (jpegamd.Image * len(imgs))(*imgs)
    out_arr, size_arr = _arrays()
    return jpegamd.lib.jpegamd_encode_color_interleaved_restart_batch_async(ctx, arr, len(imgs), sub, ri, out_arr, CAP, size_arr, None)


def _call_ycc(jpegamd, ctx, imgs, sub, ri):
    arr = (jpegamd.YCbCrImage * len(imgs))(*imgs)
    out_arr, size_arr = _arrays()
    return jpegamd.lib.jpegamd_encode_ycbcr_interleaved_restart_batch_async(ctx, arr, len(imgs), sub, ri, out_arr, CAP, size_arr, None)


def test_entries_refuse_before_the_context(jpegamd):
    keep, ctx = _fake_context()
    w, h = 65, 33
    rgb = [jpegamd.Encoder.image(0x100000 * (i + 1), w, h, 3 * w, False, jpegamd.ORDER_RGB, 0) for i in range(2)]
    for sub in SUBS:
        cw = w if sub == cm.SUB_444 else (w + 1) // 2
        ycc = [jpegamd.Encoder.ycbcr_image(0x100000 * (i + 1), 0x800000, 0x900000, w, h, w, cw, jpegamd.CHROMA_PLANES, 0) for i in range(2)]
        for ri in (-1, 65536, -65536, 1 << 30):                      # an interval out of range, with everything else in order
            assert _call_rgb(jpegamd, ctx, rgb, sub, ri) == ERR_ARG, (sub, ri)
            assert _call_ycc(jpegamd, ctx, ycc, sub, ri) == ERR_ARG, (sub, ri)
        for ri in (0, 1, 7, 65535):                                  # an interval in range does not rescue any other bad argument
            assert _call_rgb(jpegamd, None, rgb, sub, ri) == ERR_ARG
            assert _call_ycc(jpegamd, None, ycc, sub, ri) == ERR_ARG
            for order in (jpegamd.ORDER_GRAY, jpegamd.ORDER_RGBA, jpegamd.ORDER_BGRA):
                bad = jpegamd.Encoder.image(0x100000, w, h, 4 * w, False, order, 0)
                assert _call_rgb(jpegamd, ctx, [bad], sub, ri) == ERR_ARG, (order, ri)
            for layout in (jpegamd.CHROMA_YUYV, jpegamd.CHROMA_UYVY):  # packed 4:2:2 in one scan stays a follow-up
                bad = jpegamd.Encoder.ycbcr_image(0x100000, 0x800000, 0x900000, w, h, 4 * w, 4 * w, layout, 0)
                assert _call_ycc(jpegamd, ctx, [bad], sub, ri) == ERR_ARG, (layout, ri)
                assert _call_ycc(jpegamd, ctx, [ycc[0], bad], sub, ri) == ERR_ARG, (layout, ri)
            assert _call_rgb(jpegamd, ctx, [rgb[0], jpegamd.Encoder.image(0x300000, w - 1, h, 3 * w, False, jpegamd.ORDER_RGB, 0)], sub, ri) == ERR_ARG
    for sub in (0, 3, -1):
        assert _call_rgb(jpegamd, ctx, rgb, sub, 4) == ERR_ARG


def test_binding_restart_interval_checks_on_the_cpu(jpegamd):
    torch = pytest.importorskip("torch")
    u8 = torch.uint8
    hwc, gray = torch.zeros(2, 8, 8, 3, dtype=u8), torch.zeros(2, 8, 8, dtype=u8)
    y, cb, cr = torch.zeros(2, 8, 8, dtype=u8), torch.zeros(2, 4, 4, dtype=u8), torch.zeros(2, 4, 4, dtype=u8)
    bad = [dict(scan="separate", restart_interval=1), dict(restart_interval=4), dict(scan="separate", restart_interval="row"),
           dict(scan="interleaved", restart_interval=-1), dict(scan="interleaved", restart_interval=65536),
           dict(scan="interleaved", restart_interval="column"), dict(scan="interleaved", restart_interval=1.5),
           dict(scan="interleaved", restart_interval=True)]
    for i, kw in enumerate(bad):
        for call in (lambda: jpegamd.encode_tensor_batch(hwc, **kw), lambda: jpegamd.encode_tensor(hwc[0], **kw),
                     lambda: jpegamd.encode_ycbcr_batch(y, cb, cr, **kw)):
            with pytest.raises(ValueError) as err:
                call()
            assert "device tensor" not in str(err.value), (i, str(err.value))
    with pytest.raises(ValueError) as err:
        jpegamd.encode_tensor_batch(gray, restart_interval=2)
    assert "device tensor" not in str(err.value)
    # well-formed calls only lack a device; 0 and None are "no restart intervals" with either scan
    good = [dict(scan="interleaved", restart_interval=1), dict(scan="interleaved", restart_interval="row"), dict(scan="interleaved", restart_interval=65535),
            dict(scan="interleaved", restart_interval=0), dict(scan="separate", restart_interval=0), dict(restart_interval=None)]
    for kw in good:
        for call in (lambda: jpegamd.encode_tensor_batch(hwc, **kw), lambda: jpegamd.encode_tensor(hwc[0], **kw),
                     lambda: jpegamd.encode_ycbcr_batch(y, cb, cr, **kw)):
            with pytest.raises(ValueError, match="device tensor"):
                call()
    assert jpegamd._restart("row", True, 200, cm.SUB_420) == 13 and jpegamd._restart("row", True, 200, cm.SUB_444) == 25
    assert jpegamd._restart("row", True, 17, m422.SUB_422) == 2
