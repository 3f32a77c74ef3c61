"""Progressive colour files on the CPU: the model of the file (tests/progressive_model.py) against an independent decoder and the
one-scan model, the file's marker sequence, the size bound, the argument checks of the two C entries that return before the context
is touched, and the checks of jpegamd.progressive.  Nothing here needs a device."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import color_model as cm
import color_model_422 as m422
import interleaved_model as im
import mjpeg_support as ms
import progressive_model as pm
import test_binding_host as tb
from test_binding_host import enc, rec  # noqa: F401  (the recording stand-in for jpegamd.lib, and a context on it)

torch = pytest.importorskip("torch")

ERR_ARG = -1
SIZES = [(1, 1), (8, 8), (17, 9), (24, 40), (257, 31), (200, 120)]
SUBS = (cm.SUB_444, cm.SUB_420, m422.SUB_422)
NAMES = ("jpegamd_encode_color_progressive_batch_async", "jpegamd_encode_ycbcr_progressive_batch_async", "jpegamd_max_jfif_bytes_progressive")


def _picture(jpegamd, w, h, seed=11):
    return cm.read_bmp_rgb(jpegamd.synth_bmp(w, h, seed + w + 3 * h, 0, 0))


def _decode(data: bytes):
    import io
    image = pytest.importorskip("PIL.Image")
    with image.open(io.BytesIO(data)) as f:
        return f.info.get("progressive"), np.asarray(f.convert("RGB"))


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("quality", (50, 90))
def test_model_file_decodes_to_the_one_scan_pixels(jpegamd, oracle, sub, quality):
    for w, h in SIZES:
        rgb = _picture(jpegamd, w, h)
        p = cm.memo(pm.progressive_file, oracle, rgb, quality, sub)
        one = cm.memo(im.interleaved_file, oracle, rgb, quality, sub)
        progressive, got = _decode(p.file)
        _, want = _decode(one.file)
        assert progressive == 1
        assert got.shape == (h, w, 3) and np.array_equal(got, want), (w, h)
        assert p.pad_blocks == one.pad_blocks


def _segments(data: bytes):
    """The file as [(marker, segment bytes with the marker, entropy-coded bytes behind it)]."""
    out, at = [], 2
    assert data[:2] == b"\xff\xd8"
    while at < len(data):
        assert data[at] == 0xFF
        marker = data[at + 1]
        if marker == 0xD9:
            out.append((marker, data[at:at + 2], b""))
            at += 2
            break
        n = 2 + int.from_bytes(data[at + 2:at + 4], "big")
        seg, at = data[at:at + n], at + n
        ecs = b""
        if marker == 0xDA:
            end = at
            while not (data[end] == 0xFF and data[end + 1] != 0x00):
                end += 1
            ecs, at = data[at:end], end
        out.append((marker, seg, ecs))
    assert at == len(data)
    return out


@pytest.mark.parametrize("sub", SUBS)
def test_marker_sequence_and_scan_headers(jpegamd, oracle, sub):
    for w, h in SIZES:
        rgb = _picture(jpegamd, w, h)
        p = cm.memo(pm.progressive_file, oracle, rgb, 50, sub)
        one = cm.memo(im.interleaved_file, oracle, rgb, 50, sub)
        segs = _segments(p.file)
        assert [m for m, _, _ in segs] == [0xE0, 0xDB, 0xC2] + [0xC4] * 4 + [0xDA] * 7 + [0xD9]
        table = [bytes.fromhex("FFDA000C03010002110311000000")]
        table += [bytes([0xFF, 0xDA, 0x00, 0x08, 0x01, c, 0x00 if c == 1 else 0x11, ss, se, 0x00]) for ss, se in ((1, 5), (6, 0x3F)) for c in (1, 2, 3)]
        assert [s for m, s, _ in segs if m == 0xDA] == table
        # the one-scan file's headers with SOF2 for SOF0: same length, same contents, same sampling factors
        at = one.file.index(b"\xff\xda")
        assert p.file[:at] == one.file[:at].replace(b"\xff\xc0\x00\x11", b"\xff\xc2\x00\x11", 1)
        sof = segs[2][1]
        assert sof[11] == {cm.SUB_444: 0x11, cm.SUB_420: 0x22, m422.SUB_422: 0x21}[sub]
        # every scan byte-aligned, stuffed, and as long as its bits say
        for k, (_, _, ecs) in enumerate(s for s in segs if s[0] == 0xDA):
            assert len(ecs) == (p.scan_bits[k] + 7) // 8 + p.stuffed[k]
            assert sum(p.seg_bits[k]) == p.scan_bits[k]


def test_bound_holds_for_noise_at_quality_100(jpegamd, oracle):
    rng = np.random.default_rng(5)
    for w, h in SIZES:
        for sub in SUBS:
            rgb = rng.integers(0, 256, (h, w, 3), np.uint8)
            p = cm.memo(pm.progressive_file, oracle, rgb, 100, sub)
            assert jpegamd.max_jfif_bytes_progressive(w, h, sub) >= len(p.file)
            assert jpegamd.max_jfif_bytes_progressive(w, h, sub) == jpegamd.max_jfif_bytes_interleaved(w, h, sub) + 6 * 12
    for bad in ((0, 8, cm.SUB_444), (8, 0, cm.SUB_444), (65536, 8, cm.SUB_420), (8, 65536, cm.SUB_420), (8, 8, 0), (8, 8, 3), (-1, 8, cm.SUB_444)):
        assert jpegamd.max_jfif_bytes_progressive(*bad) == 0


def test_symbols_are_exported_and_documented(jpegamd):
    header = jpegamd.HEADER_PATH.read_text()
    lib = C.CDLL(str(jpegamd.LIB_PATH))
    for name in NAMES:
        assert name in jpegamd.EXPORTED and hasattr(lib, name) and name in header, name
    assert hasattr(jpegamd.Encoder, "encode_color_progressive_batch_async") and hasattr(jpegamd.Encoder, "encode_ycbcr_progressive_batch_async")
    assert "FF DA 00 0C 03 01 00 02 11 03 11 00 00 00" in header and "FF DA 00 08 01 cc tt 06 3F 00" in header


def test_encoder_methods_reach_their_entries(jpegamd, rec, enc):
    """test_binding_host's check of a batch method, for the two new ones: the entry, its arguments and their order."""
    cases = [("encode_color_progressive_batch_async", (tb.SUB,), "jpegamd_encode_color_progressive_batch_async", jpegamd.Image, [tb.SUB]),
             ("encode_ycbcr_progressive_batch_async", (tb.SUB, tb.RANGE, tb.FORMAT, tb.MATRIX), "jpegamd_encode_ycbcr_progressive_batch_async",
              jpegamd.YCbCrImage, [tb.SUB, tb.RANGE, tb.FORMAT, tb.MATRIX])]
    for method, args, entry, struct, before in cases:
        imgs = tb.pictures(jpegamd, struct)
        assert getattr(enc, method)(imgs, *args, tb.OUTS, tb.CAP, tb.SIZES, tb.STREAM) is None
        (call,) = rec.calls
        tb.check_batch_call(call, entry, struct, imgs, before, [])
        del rec.calls[:]
    rec.code = -1
    with pytest.raises(jpegamd.JpegAmdError) as err:
        enc.encode_color_progressive_batch_async(tb.pictures(jpegamd, jpegamd.Image), tb.SUB, tb.OUTS, tb.CAP, tb.SIZES, tb.STREAM)
    assert err.value.code == -1 and "jpegamd_encode_color_progressive_batch_async" in str(err.value)


def _arrays(n=4):
    return (C.c_void_p * n)(*([C.c_void_p(0x1000)] * n)), (C.c_void_p * n)(*([C.c_void_p(0x2000)] * n))


def _call_pixels(jpegamd, ctx, imgs, sub, count=None, outs=True):
    arr = (jpegamd.Image * max(len(imgs), 1))(*imgs) if imgs is not None else None
    out_arr, size_arr = _arrays() if outs else (None, None)
    return jpegamd.lib.jpegamd_encode_color_progressive_batch_async(ctx, arr, len(imgs) if count is None else count, sub, out_arr, 1 << 20,
                                                                    size_arr, None)


def _call_ycc(jpegamd, ctx, imgs, sub, rng=0, fmt=0, matrix=0, count=None, outs=True):
    arr = (jpegamd.YCbCrImage * max(len(imgs), 1))(*imgs) if imgs is not None else None
    out_arr, size_arr = _arrays() if outs else (None, None)
    return jpegamd.lib.jpegamd_encode_ycbcr_progressive_batch_async(ctx, arr, len(imgs) if count is None else count, sub, rng, fmt, matrix,
                                                                    out_arr, 1 << 20, size_arr, None)


def test_color_entry_refuses_before_the_context_is_read(jpegamd):
    keep, ctx = ms.fake_context()
    j = jpegamd
    good = j.Encoder.image(0x4000, 16, 16, 48, False, j.ORDER_RGB, 50)
    for order in (j.ORDER_RGB, j.ORDER_BGR, j.ORDER_RGBA, j.ORDER_BGRA):          # (nothing but the arguments decides: a null context is refused too)
        img = j.Encoder.image(0x4000, 16, 16, 64, False, order, 50)
        assert _call_pixels(j, None, [img], cm.SUB_420) == ERR_ARG
    assert _call_pixels(j, ctx, [j.Encoder.image(0x4000, 16, 16, 16, False, j.ORDER_GRAY, 50)], cm.SUB_420) == ERR_ARG
    for sub in (0, 3, 5, -1):
        assert _call_pixels(j, ctx, [good], sub) == ERR_ARG
    assert _call_pixels(j, ctx, [good], cm.SUB_420, count=0) == ERR_ARG
    assert _call_pixels(j, ctx, [good], cm.SUB_420, count=j.MAX_BATCH + 1) == ERR_ARG
    assert _call_pixels(j, ctx, None, cm.SUB_420, count=1) == ERR_ARG
    assert _call_pixels(j, ctx, [good], cm.SUB_420, outs=False) == ERR_ARG
    assert _call_pixels(j, ctx, [j.Encoder.image(0x4000, 16, 16, 47, False, j.ORDER_RGB, 50)], cm.SUB_420) == ERR_ARG      # rows overlap
    assert _call_pixels(j, ctx, [j.Encoder.image(0x4000, 0, 16, 48, False, j.ORDER_RGB, 50)], cm.SUB_420) == ERR_ARG
    assert _call_pixels(j, ctx, [j.Encoder.image(0, 16, 16, 48, False, j.ORDER_RGB, 50)], cm.SUB_420) == ERR_ARG
    other = j.Encoder.image(0x8000, 24, 16, 72, False, j.ORDER_RGB, 50)                                                   # two geometries
    assert _call_pixels(j, ctx, [good, other], cm.SUB_420) == ERR_ARG
    assert not any(keep)


def test_ycbcr_entry_refuses_what_its_one_scan_twin_refuses(jpegamd):
    keep, ctx = ms.fake_context()
    j = jpegamd
    good = j.Encoder.ycbcr_image(0x4000, 0x5000, 0x6000, 16, 16, 16, 8, j.CHROMA_PLANES, 50)
    cases = [
        dict(imgs=[good], sub=0), dict(imgs=[good], sub=3),
        dict(imgs=[good], sub=cm.SUB_420, rng=2), dict(imgs=[good], sub=cm.SUB_420, fmt=3), dict(imgs=[good], sub=cm.SUB_420, matrix=2),
        dict(imgs=[good], sub=cm.SUB_420, count=0), dict(imgs=[good], sub=cm.SUB_420, count=j.MAX_BATCH + 1),
        dict(imgs=None, sub=cm.SUB_420, count=1), dict(imgs=[good], sub=cm.SUB_420, outs=False),
        dict(imgs=[j.Encoder.ycbcr_image(0x4000, 0x5000, 0x6000, 16, 16, 15, 8, j.CHROMA_PLANES, 50)], sub=cm.SUB_420),
        dict(imgs=[j.Encoder.ycbcr_image(0x4000, 0x5000, 0, 16, 16, 16, 8, j.CHROMA_PLANES, 50)], sub=cm.SUB_420),
        dict(imgs=[j.Encoder.ycbcr_image(0x4000, 0x5000, 0x6000, 16, 16, 16, 8, 3, 50)], sub=cm.SUB_420),
        dict(imgs=[j.Encoder.ycbcr_image(0x4000, 0, 0, 16, 16, 32, 0, j.CHROMA_YUYV, 50)], sub=cm.SUB_420),      # packed 4:2:2 is 4:2:2
    ]
    for kw in cases:
        assert _call_ycc(j, ctx, **kw) == ms.call_ycc(j, ctx, **kw) == ERR_ARG, kw
    assert _call_ycc(j, None, [good], cm.SUB_420) == ERR_ARG
    assert not any(keep)


def test_binding_functions_raise_before_any_device_work(jpegamd):
    import jpegamd.progressive as prog
    import jpegamd.mjpeg as mj
    t = torch.zeros((2, 16, 16, 3), dtype=torch.uint8)
    bad_tensor = [
        dict(t=t, subsampling=0), dict(t=t, subsampling=3), dict(t=t, layout="nope"), dict(t=t.to(torch.int16)),
        dict(t=torch.zeros((2, 16, 16), dtype=torch.uint8)), dict(t=torch.zeros((2, 16, 16, 4), dtype=torch.uint8), layout="hwc"),
        dict(t=t[:, :, :, :2]), dict(t=t),                                                                           # (the last: a host tensor)
    ]
    for kw in bad_tensor:
        with pytest.raises(ValueError):
            mj.encode_tensor_batch(**kw)
        with pytest.raises(ValueError):
            prog.encode_tensor_batch(**kw)
    with pytest.raises(ValueError):
        prog.encode_tensor_batch(torch.zeros((2, 3, 16, 16), dtype=torch.uint8), layout="chw")      # the planar entry is not part of this file
    with pytest.raises(ValueError):
        prog.encode_tensor(torch.zeros((16, 16), dtype=torch.uint8))
    with pytest.raises(TypeError):
        prog.encode_tensor_batch(t, restart_interval=4)
    with pytest.raises(TypeError):
        prog.encode_tensor_batch(t, huffman="optimized")
    y, c = torch.zeros((1, 16, 16), dtype=torch.uint8), torch.zeros((1, 8, 8), dtype=torch.uint8)
    bad_ycc = [
        dict(y=y, cb=c, cr=c, subsampling=3), dict(y=y, cb=c, cr=c, order="nope"), dict(y=y, cb=c, cr=c, sample_range="video"),
        dict(y=y, cb=c, cr=c, matrix="bt2020"), dict(y=y, cb=c[:, :4], cr=c), dict(y=y, cb=c, cr=None), dict(y=y, cb=c, cr=c),
    ]
    for kw in bad_ycc:
        with pytest.raises(ValueError):
            mj.encode_ycbcr_batch(**kw)
        with pytest.raises(ValueError):
            prog.encode_ycbcr_batch(**kw)
    y16, c16 = y.to(torch.int16), c.to(torch.int16)
    for kw in (dict(y=y16, cb=c16, cr=c16, align="middle"), dict(y=y, cb=c, cr=c), dict(y=y16, cb=c16, cr=c16)):
        with pytest.raises(ValueError):
            mj.encode_ycbcr16_batch(**kw)
        with pytest.raises(ValueError):
            prog.encode_ycbcr16_batch(**kw)
    f = torch.zeros((1, 16, 16, 2), dtype=torch.uint8)
    for kw in (dict(frames=f, order="vyuy"), dict(frames=f[:, :, :15]), dict(frames=f, sample_range=1), dict(frames=f)):
        with pytest.raises(ValueError):
            mj.encode_yuyv_batch(**kw)
        with pytest.raises(ValueError):
            prog.encode_yuyv_batch(**kw)
