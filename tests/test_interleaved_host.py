"""Interleaved-MCU colour files on the CPU: the model of the file (tests/interleaved_model.py) against an independent decoder and
against the three-scan model, the file's structure, the pad-block count, the exported symbols, the argument checks of the two C
entries that return before the context is touched, the size bound, and the binding's scan= checks.  Nothing here needs a device."""
from __future__ import annotations

import ctypes as C
import io

import numpy as np
import pytest

import color_model as cm
import color_model_422 as m422
import interleaved_model as im
import scan_model as sm

ERR_ARG = -1
CAP = 1 << 20
SIZES = [(1, 1), (8, 8), (9, 9), (17, 9), (24, 40), (33, 17), (72, 24), (200, 120), (257, 31)]
SUBS = (cm.SUB_444, cm.SUB_420, m422.SUB_422)
NAMES = ("jpegamd_encode_color_interleaved_batch_async", "jpegamd_encode_ycbcr_interleaved_batch_async", "jpegamd_max_jfif_bytes_interleaved")


def _picture(jpegamd, w, h, seed=11):
    return cm.read_bmp_rgb(jpegamd.synth_bmp(w, h, seed + w + 3 * h, 0, 0))


def _decode(data: bytes) -> np.ndarray:
    image = pytest.importorskip("PIL.Image")
    with image.open(io.BytesIO(data)) as f:
        return np.asarray(f.convert("RGB"))


def _scan_of(data: bytes, w: int, h: int, q: int, sub: int) -> bytes:
    n = len(im.prefix(w, h, q, sub))
    assert data[:n] == im.prefix(w, h, q, sub) and data[-2:] == b"\xff\xd9"
    return data[n:-2]


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("quality", (50, 90))
def test_model_file_decodes_to_the_three_scan_pixels(jpegamd, oracle, sub, quality):
    pads = 0
    for w, h in SIZES:
        rgb = _picture(jpegamd, w, h)
        m = cm.memo(im.interleaved_file, oracle, rgb, quality, sub)
        got, want = _decode(m.file), _decode(im.three_scan_file(oracle, rgb, quality, sub))
        assert got.shape == (h, w, 3)
        assert np.array_equal(got, want), (w, h)
        pads += m.pad_blocks
    assert (pads > 0) == (sub != cm.SUB_444)                       # the sizes do bring pad blocks where MCUs are larger than a block


@pytest.mark.parametrize("sub", SUBS)
def test_model_file_structure_and_pad_blocks(jpegamd, oracle, sub):
    for w, h in SIZES:
        rgb = _picture(jpegamd, w, h)
        m = cm.memo(im.interleaved_file, oracle, rgb, 50, sub)
        f = m.file
        assert f.count(b"\xff\xda") == 1                           # exactly one SOS ...
        at = f.index(b"\xff\xda")
        assert f[at:at + 14] == im.SOS3 and f[at + 4] == 3         # ... with Ns = 3
        scan = _scan_of(f, w, h, 50, sub)
        ff = [i for i, b in enumerate(scan) if b == 0xFF]
        assert all(i + 1 < len(scan) and scan[i + 1] == 0x00 for i in ff)            # no marker inside the scan, no restart markers
        assert len(ff) == m.stuffed
        hs, vs, bw, bh, mx, my = im.geometry(w, h, sub)
        assert m.pad_blocks == mx * my * hs * vs - bw * bh
        # the three-scan file's headers, unchanged up to the DHTs
        three = im.three_scan_file(oracle, rgb, 50, sub)
        assert f[:at] == three[:three.index(b"\xff\xda")]


def test_model_luma_scan_is_the_oracles(jpegamd, oracle):
    """The model's Y coefficients and symbols are the ones the three-scan file's Y scan is made of."""
    for w, h, kind in ((33, 17, 1), (72, 24, 0)):
        rgb = cm.read_bmp_rgb(jpegamd.synth_bmp(w, h, 3, kind, 0))
        zz = cm.plane_zigzag(oracle, sm.luma_plane(rgb), cm.scaled_table(cm.LUMA_Q, 90))
        assert sm.pack_scan(oracle, zz, False) == cm.gray_scan(oracle, cm.write_bmp(rgb), 90)


def test_symbols_are_exported_and_documented(jpegamd):
    header = jpegamd.HEADER_PATH.read_text()
    lib = C.CDLL(str(jpegamd.LIB_PATH))
    for name in NAMES:
        assert name in jpegamd.EXPORTED and hasattr(lib, name) and name in header, name
    assert hasattr(jpegamd.Encoder, "encode_color_interleaved_batch_async") and hasattr(jpegamd.Encoder, "encode_ycbcr_interleaved_batch_async")
    assert "FF DA 00 0C 03 01 00 02 11 03 11 00 3F 00" in header
    assert "follow-ups" in header and "jpegamd_encoder_set_pipeline has no effect" in header


def _fake_context():
    """A block of zeros where the context would be: a check that came too late would read it."""
    fake = (C.c_uint8 * (1 << 16))()
    return fake, C.cast(fake, C.c_void_p)


def _arrays(outs=True, sizes=True, null_out=None, null_size=None):
    out_arr = (C.c_void_p * 40)(*([C.c_void_p(0x1000)] * 40)) if outs else None
    size_arr = (C.c_void_p * 40)(*([C.c_void_p(0x2000)] * 40)) if sizes else None
    if null_out is not None:
        out_arr[null_out] = None
    if null_size is not None:
        size_arr[null_size] = None
    return out_arr, size_arr


def _call_rgb(jpegamd, ctx, imgs, count, sub, **kw):
    arr = (jpegamd.Image * max(len(imgs), 1))(*imgs) if imgs else None
    out_arr, size_arr = _arrays(**kw)
    return jpegamd.lib.jpegamd_encode_color_interleaved_batch_async(ctx, arr, count, sub, out_arr, CAP, size_arr, None)


def _call_ycc(jpegamd, ctx, imgs, count, sub, **kw):
    arr = (jpegamd.YCbCrImage * max(len(imgs), 1))(*imgs) if imgs else None
    out_arr, size_arr = _arrays(**kw)
    return jpegamd.lib.jpegamd_encode_ycbcr_interleaved_batch_async(ctx, arr, count, sub, out_arr, CAP, size_arr, None)


def test_rgb_entry_refuses_before_the_context(jpegamd):
    keep, ctx = _fake_context()
    w, h = 65, 33

    def img(base=0x100000, w=w, h=h, stride=None, order=jpegamd.ORDER_RGB, bottom_up=False, q=0):
        return jpegamd.Encoder.image(base, w, h, 3 * w if stride is None else stride, bottom_up, order, q)

    good = [img(0x100000 * (i + 1)) for i in range(40)]
    for sub in (jpegamd.SUBSAMPLE_444, jpegamd.SUBSAMPLE_420, jpegamd.SUBSAMPLE_422):
        assert _call_rgb(jpegamd, None, good[:2], 2, sub) == ERR_ARG                       # null context
        assert _call_rgb(jpegamd, ctx, [], 1, sub) == ERR_ARG                              # null array
        for count in (0, -1, 33):
            assert _call_rgb(jpegamd, ctx, good[:33], count, sub) == ERR_ARG
        assert _call_rgb(jpegamd, ctx, good[:2], 2, sub, outs=False) == ERR_ARG
        assert _call_rgb(jpegamd, ctx, good[:2], 2, sub, sizes=False) == ERR_ARG
        for k in (0, 2):
            assert _call_rgb(jpegamd, ctx, good[:3], 3, sub, null_out=k) == ERR_ARG
            assert _call_rgb(jpegamd, ctx, good[:3], 3, sub, null_size=k) == ERR_ARG
        for order in (jpegamd.ORDER_GRAY, jpegamd.ORDER_RGBA, jpegamd.ORDER_BGRA, 7):       # one scan takes RGB / BGR alone
            assert _call_rgb(jpegamd, ctx, [img(order=order, stride=4 * w)], 1, sub) == ERR_ARG, order
            assert _call_rgb(jpegamd, ctx, [img(order=order, stride=4 * w)] * 2, 2, sub) == ERR_ARG, order
        for bad in (img(base=0), img(w=0), img(w=-2), img(h=0), img(h=65536), img(w=65536, stride=3 * 65536), img(stride=3 * w - 1)):
            assert _call_rgb(jpegamd, ctx, [bad], 1, sub) == ERR_ARG
        for odd in (img(w=w - 1), img(h=h - 1), img(stride=3 * w + 4), img(order=jpegamd.ORDER_BGR), img(bottom_up=True), img(q=90),
                    img(base=0)):
            assert _call_rgb(jpegamd, ctx, [good[0], odd, good[2]], 3, sub) == ERR_ARG      # a later picture of another geometry
    for sub in (0, 3, -1, 5):
        assert _call_rgb(jpegamd, ctx, good[:2], 2, sub) == ERR_ARG, sub


def test_ycbcr_entry_refuses_before_the_context(jpegamd):
    keep, ctx = _fake_context()
    w, h = 65, 33
    planes, cbcr, crcb = jpegamd.CHROMA_PLANES, jpegamd.CHROMA_CBCR, jpegamd.CHROMA_CRCB
    for sub in (jpegamd.SUBSAMPLE_444, jpegamd.SUBSAMPLE_420, jpegamd.SUBSAMPLE_422):
        cw = w if sub == jpegamd.SUBSAMPLE_444 else (w + 1) // 2
        for layout in (planes, cbcr, crcb):
            c_row = cw if layout == planes else 2 * cw

            def img(base=0x100000, w=w, h=h, ys=None, cs=None, layout=layout, q=0, ptrs=None):
                y, cb, cr = ptrs or (base, base + 0x10000, base + 0x20000)
                return jpegamd.Encoder.ycbcr_image(y, cb, cr, w, h, w if ys is None else ys, c_row if cs is None else cs, layout, q)

            good = [img(0x100000 * (i + 1)) for i in range(40)]
            case = (sub, layout)
            assert _call_ycc(jpegamd, None, good[:2], 2, sub) == ERR_ARG, case
            assert _call_ycc(jpegamd, ctx, [], 1, sub) == ERR_ARG, case
            for count in (0, -1, 33):
                assert _call_ycc(jpegamd, ctx, good[:33], count, sub) == ERR_ARG, case
            assert _call_ycc(jpegamd, ctx, good[:2], 2, sub, outs=False) == ERR_ARG, case
            assert _call_ycc(jpegamd, ctx, good[:2], 2, sub, sizes=False) == ERR_ARG, case
            for k in (0, 2):
                assert _call_ycc(jpegamd, ctx, good[:3], 3, sub, null_out=k) == ERR_ARG, case
                assert _call_ycc(jpegamd, ctx, good[:3], 3, sub, null_size=k) == ERR_ARG, case
            nulls = [(0, 0x6000, 0x7000), (0x5000, 0, 0x7000)] + ([(0x5000, 0x6000, 0)] if layout == planes else [])
            for ptrs in nulls:
                assert _call_ycc(jpegamd, ctx, [img(ptrs=ptrs)], 1, sub) == ERR_ARG, (case, ptrs)
                assert _call_ycc(jpegamd, ctx, [good[0], img(ptrs=ptrs), good[2]], 3, sub) == ERR_ARG, (case, ptrs)
            for kw in (dict(ys=w - 1), dict(cs=c_row - 1), dict(ys=0), dict(cs=0), dict(w=0, ys=8, cs=8), dict(h=0), dict(h=65536)):
                assert _call_ycc(jpegamd, ctx, [img(**kw)], 1, sub) == ERR_ARG, (case, kw)
            for odd in (img(w=w - 1), img(h=h - 1), img(ys=w + 4), img(cs=c_row + 4), img(q=90)):
                assert _call_ycc(jpegamd, ctx, [good[0], odd, good[2]], 3, sub) == ERR_ARG, case
            # packed 4:2:2 in one scan is a follow-up: refused as the only picture, the first or a later one; unknown layouts too
            for bad_layout in (jpegamd.CHROMA_YUYV, jpegamd.CHROMA_UYVY, 3, -1, 7):
                bad = img(layout=bad_layout, ys=4 * w, cs=4 * w)
                for imgs, n in (([bad], 1), ([bad, good[1], good[2]], 3), ([good[0], good[1], bad], 3)):
                    assert _call_ycc(jpegamd, ctx, imgs, n, sub) == ERR_ARG, (case, bad_layout, n)
    good = [jpegamd.Encoder.ycbcr_image(0x1000 * (i + 1), 0x100000, 0x200000, 64, 32, 64, 64, planes, 0) for i in range(2)]
    for sub in (0, 3, -1):
        assert _call_ycc(jpegamd, ctx, good, 2, sub) == ERR_ARG, sub


def test_size_bound_matches_its_formula(jpegamd):
    for w, h in SIZES + [(8192, 8192), (65535, 65535), (4000, 17)]:
        for sub in SUBS:
            hs, vs, bw, bh, mx, my = im.geometry(w, h, sub)
            nb = mx * my * (hs * vs + 2)
            want = 640 + 2 * ((nb * 1723 + 7) // 8 + 1) + 2 + 16
            assert jpegamd.max_jfif_bytes_interleaved(w, h, sub) == want, (w, h, sub)
            assert nb >= bw * bh + 2 * mx * my                       # pad blocks are counted
    # the three-scan bound does not hold a picture's pad blocks: 17 x 9 at 4:2:0 has 6 real and 2 pad Y blocks
    assert jpegamd.max_jfif_bytes_interleaved(17, 9, cm.SUB_420) > jpegamd.max_jfif_bytes_color(17, 9, cm.SUB_420)
    for w, h, sub in ((0, 8, 1), (8, 0, 2), (-1, 8, 4), (8, 8, 0), (8, 8, 3), (65536, 8, 1), (8, 65536, 2)):
        assert jpegamd.max_jfif_bytes_interleaved(w, h, sub) == 0, (w, h, sub)


def test_model_files_fit_the_bound(jpegamd, oracle):
    rng = np.random.default_rng(7)
    for w, h in ((17, 9), (33, 17)):
        rgb = rng.integers(0, 256, (h, w, 3), np.uint8)
        for sub in SUBS:
            assert len(cm.memo(im.interleaved_file, oracle, rgb, 100, sub).file) <= jpegamd.max_jfif_bytes_interleaved(w, h, sub)


def test_binding_refuses_unsupported_scan_combinations_on_the_cpu(jpegamd):
    torch = pytest.importorskip("torch")
    u8 = torch.uint8
    s420 = jpegamd.SUBSAMPLE_420
    hwc, chw, px4, gray = torch.zeros(2, 8, 8, 3, dtype=u8), torch.zeros(2, 3, 8, 8, dtype=u8), torch.zeros(2, 8, 8, 4, dtype=u8), torch.zeros(2, 8, 8, dtype=u8)
    bad_batch = [
        dict(t=hwc, scan="both"), dict(t=hwc, scan=None), dict(t=hwc, scan="Interleaved"), dict(t=hwc, scan=1),      # an unknown scan
        dict(t=chw, layout="chw", scan="interleaved"), dict(t=px4, layout="rgba", scan="interleaved"),
        dict(t=px4, layout="bgra", scan="interleaved"), dict(t=gray, scan="interleaved"),                            # grayscale files have one component
        dict(t=hwc, subsampling=0, scan="interleaved"), dict(t=hwc, subsampling=3, scan="interleaved"),
        dict(t=hwc, layout="hwc", subsampling=0, scan="interleaved"),
    ]
    for i, kw in enumerate(bad_batch):
        t = kw.pop("t")
        with pytest.raises(ValueError) as err:
            jpegamd.encode_tensor_batch(t, **kw)
        assert "device tensor" not in str(err.value), (i, str(err.value))
    for i, kw in enumerate([dict(t=gray[0], scan="interleaved"), dict(t=chw[0], layout="chw", scan="interleaved"),
                            dict(t=px4[0], layout="rgba", scan="interleaved"), dict(t=hwc[0], scan="progressive"),
                            dict(t=hwc[0], subsampling=0, scan="interleaved")]):
        t = kw.pop("t")
        with pytest.raises(ValueError) as err:
            jpegamd.encode_tensor(t, **kw)
        assert "device tensor" not in str(err.value), (i, str(err.value))
    y, cb, cr, pairs = torch.zeros(2, 8, 8, dtype=u8), torch.zeros(2, 4, 4, dtype=u8), torch.zeros(2, 4, 4, dtype=u8), torch.zeros(2, 4, 4, 2, dtype=u8)
    for i, kw in enumerate([dict(cb=cb, cr=cr, sample_range="limited", scan="interleaved"), dict(cb=cb, cr=cr, matrix="bt709", scan="interleaved"),
                            dict(cb=pairs, sample_range="limited", matrix="bt709", scan="interleaved"), dict(cb=pairs, scan="mcu"),
                            dict(cb=cb, cr=cr, scan="")]):
        with pytest.raises(ValueError) as err:
            jpegamd.encode_ycbcr_batch(y, subsampling=s420, **kw)
        assert "device tensor" not in str(err.value), (i, str(err.value))
    # well-formed host tensors only lack a device: the scan= checks let them through, and "separate" is the default's own path
    for call in (lambda: jpegamd.encode_tensor_batch(hwc, scan="interleaved"), lambda: jpegamd.encode_tensor_batch(hwc, layout="hwc", scan="interleaved"),
                 lambda: jpegamd.encode_tensor_batch(hwc, scan="separate"), lambda: jpegamd.encode_ycbcr_batch(y, cb, cr, scan="interleaved"),
                 lambda: jpegamd.encode_ycbcr_batch(y, pairs, order="crcb", scan="interleaved"), lambda: jpegamd.encode_tensor(hwc[0], scan="interleaved")):
        with pytest.raises(ValueError, match="device tensor"):
            call()
