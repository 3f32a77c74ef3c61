"""4:2:2 colour files and packed YUY2 / UYVY input on the CPU: the new constants, the size bound, the chroma launch plan, the shape
and stride checks of encode_ycbcr_batch / encode_yuyv_batch, the argument checks of jpegamd_encode_ycbcr_batch_async that return
before the context is touched, and the CPU model of tests/color_model_422.py against an independent decoder.  Nothing here needs a
device."""
from __future__ import annotations

import ctypes as C
import io
import re

import numpy as np
import pytest

import color_model as cm
import color_model_422 as m422

ERR_ARG, ERR_TOO_LARGE = -1, -5
CAP = 1 << 20


# ---- constants ---------------------------------------------------------------------------------------------------------------------
def test_constants_in_python_and_in_the_header(jpegamd):
    header = jpegamd.HEADER_PATH.read_text()
    for name, value in (("SUBSAMPLE_422", 4), ("CHROMA_YUYV", 4), ("CHROMA_UYVY", 5)):
        assert re.search(rf"#define\s+JPEGAMD_{name}\s+{value}\b", header), name
        assert getattr(jpegamd, name) == value
    assert (m422.SUB_422, m422.YUYV, m422.UYVY) == (jpegamd.SUBSAMPLE_422, jpegamd.CHROMA_YUYV, jpegamd.CHROMA_UYVY)
    assert not re.search(r"#define\s+JPEGAMD_(SUBSAMPLE|CHROMA)_\w+\s+3\b", header)       # 3 stays a known-bad value, and the header says why
    assert "3 is skipped" in header
    assert callable(jpegamd.encode_yuyv_batch)


# ---- the size bound ----------------------------------------------------------------------------------------------------------------
def _bounds(jpegamd, w, h):
    return [jpegamd.max_jfif_bytes_color(w, h, s) for s in (jpegamd.SUBSAMPLE_420, jpegamd.SUBSAMPLE_422, jpegamd.SUBSAMPLE_444)]


def test_the_bound_lies_between_its_neighbours(jpegamd):
    b420, b422, b444 = _bounds(jpegamd, 64, 64)                   # chroma blocks 4 x 4, 4 x 8, 8 x 8
    assert 0 < b420 < b422 < b444
    assert b444 - b422 == 2 * (b422 - b420)                       # 16, 32 and 64 blocks per plane
    for w, h in ((8, 8), (5, 3), (1, 1)):                         # one chroma block at every subsampling
        b420, b422, b444 = _bounds(jpegamd, w, h)
        assert 0 < b420 == b422 == b444, (w, h)
    b420, b422, b444 = _bounds(jpegamd, 16, 8)                    # cw x ch = 8 x 4, 8 x 8, 16 x 8: 4:2:2 rounds up to 4:2:0's blocks
    assert b420 == b422 < b444
    b420, b422, b444 = _bounds(jpegamd, 8, 16)                    # 4 x 8, 4 x 16, 8 x 16: ... and here to 4:4:4's
    assert b420 < b422 == b444
    for w, h in ((0, 8), (8, 0), (-1, 8)):
        assert jpegamd.max_jfif_bytes_color(w, h, jpegamd.SUBSAMPLE_422) == 0


@pytest.mark.parametrize("w,h", [(7, 9), (64, 64), (513, 17)])
def test_the_bound_holds_the_model_file_of_noise_at_quality_100(jpegamd, oracle, w, h):
    rgb = np.random.default_rng(w + h).integers(0, 256, (h, w, 3), np.uint8)
    f = m422.color_file_422(oracle, cm.write_bmp(rgb), 100)
    assert len(f) <= jpegamd.max_jfif_bytes_color(w, h, jpegamd.SUBSAMPLE_422), (w, h, len(f))


# ---- the chroma launch plan --------------------------------------------------------------------------------------------------------
def _rows(count, h):
    return count * ((h + 7) // 8 * 8)


def test_chroma_groups_at_422(jpegamd):
    """A 4:2:2 plane is half as wide and as high as its picture, so a batch's 2 x count planes have the block rows of 2 x count
    pictures.  A context of count x H rows holds them in ONE launch where half the width also takes half the tiles and half the
    segments of a block row -- W a multiple of 4096 (16 tiles, two 8-tile segments per block row).  Narrower pictures do not halve
    (a 256-wide picture and its 128-wide plane are one tile per block row each): the planes then go as two launches of `count`.
    A plane never needs more of anything than its picture, so it is never more than two."""
    s422 = jpegamd.SUBSAMPLE_422
    for w, h, count in ((4096, 16, 1), (4096, 16, 5), (4096, 32, 16), (8192, 48, 16), (8192, 16, 3)):
        group, launches, seg_tiles, stitch = jpegamd._chroma_groups(w, _rows(count, h), w, h, count, s422)
        assert (group, launches) == (2 * count, 1), (w, h, count, group, launches)
    for w, h, count in ((16, 16, 3), (256, 48, 16), (640, 16, 5), (2048, 32, 7)):
        group, launches, seg_tiles, stitch = jpegamd._chroma_groups(w, _rows(count, h), w, h, count, s422)
        assert (group, launches) == (count, 2), (w, h, count, group, launches)
    for w, h, count in ((16, 16, 32), (4096, 16, 32), (17, 33, 20), (513, 17, 32), (7, 9, 1), (2049, 3, 17), (640, 480, 9)):
        for pipeline in (jpegamd.PIPELINE_AUTO, jpegamd.PIPELINE_PAIR, jpegamd.PIPELINE_STITCH):
            group, launches, seg_tiles, stitch = jpegamd._chroma_groups(w, _rows(count, h), w, h, count, s422, pipeline)
            assert 1 <= group <= 32 and launches <= 2 and group * launches >= 2 * count, (w, h, count, pipeline, group, launches)
            assert (launches - 1) * group < 2 * count                # no empty launch
    # a larger context takes more planes per launch, up to 32
    assert jpegamd._chroma_groups(640, _rows(32, 64), 640, 64, 20, s422)[:2] == (20, 2)
    assert jpegamd._chroma_groups(640, _rows(64, 64), 640, 64, 16, s422)[:2] == (32, 1)


# ---- shape and stride checks -------------------------------------------------------------------------------------------------------
def test_ycbcr_layout_at_422(jpegamd):
    torch = pytest.importorskip("torch")
    s422, s420 = jpegamd.SUBSAMPLE_422, jpegamd.SUBSAMPLE_420

    def z(*shape):
        return torch.zeros(*shape, dtype=torch.uint8)

    assert jpegamd._ycbcr_layout(z(2, 9, 7), z(2, 9, 4), z(2, 9, 4), s422, "cbcr") == (2, 9, 7, 7, 4, jpegamd.CHROMA_PLANES)
    assert jpegamd._ycbcr_layout(z(2, 9, 7), z(2, 9, 4, 2), None, s422, "cbcr") == (2, 9, 7, 7, 8, jpegamd.CHROMA_CBCR)
    assert jpegamd._ycbcr_layout(z(3, 8, 8), z(3, 8, 4, 2), None, s422, "crcb") == (3, 8, 8, 8, 8, jpegamd.CHROMA_CRCB)
    big = z(4, 20, 40)
    assert jpegamd._ycbcr_layout(big[::2, :16, :32], big[1::2, :16, :16], big[1::2, :16, 16:32], s422, "cbcr") == \
        (2, 16, 32, 40, 40, jpegamd.CHROMA_PLANES)
    bad = [
        (z(2, 8, 8), z(2, 4, 4), z(2, 4, 4)),                     # 4:2:0-shaped chroma
        (z(2, 8, 8), z(2, 4, 4, 2), None),
        (z(2, 8, 8), z(2, 8, 8), z(2, 8, 8)),                     # 4:4:4-shaped chroma
        (z(2, 9, 7), z(2, 9, 3), z(2, 9, 3)),                     # odd W: ceil, not floor
        (z(2, 9, 7), z(2, 5, 4), z(2, 5, 4)),                     # odd H: every row
        (z(2, 8, 8), z(2, 8, 8, 2)[:, :, ::2], None),             # a strided pair
        (z(2, 8, 8), z(2, 8, 4), z(2, 8, 6)[:, :, :4]),           # cb and cr rows 4 and 6 bytes apart
    ]
    for i, (y, cb, cr) in enumerate(bad):
        with pytest.raises(ValueError):
            jpegamd._ycbcr_layout(y, cb, cr, s422, "cbcr")
    with pytest.raises(ValueError):
        jpegamd._ycbcr_layout(z(2, 8, 8), z(2, 8, 4), z(2, 8, 4), s420, "cbcr")        # 4:2:2-shaped chroma at 4:2:0
    with pytest.raises(ValueError):
        jpegamd._ycbcr_layout(z(2, 8, 8), z(2, 8, 4), z(2, 8, 4), 3, "cbcr")           # 3 stays unknown
    with pytest.raises(ValueError, match="device tensor"):
        jpegamd.encode_ycbcr_batch(z(2, 8, 8), z(2, 8, 4), z(2, 8, 4), subsampling=s422)


def test_yuyv_layout(jpegamd):
    torch = pytest.importorskip("torch")

    def z(*shape, dtype=torch.uint8):
        return torch.zeros(*shape, dtype=dtype)

    assert jpegamd._yuyv_layout(z(3, 9, 8, 2), "yuyv") == (3, 9, 8, 16, jpegamd.CHROMA_YUYV)
    assert jpegamd._yuyv_layout(z(3, 9, 8, 2), "uyvy") == (3, 9, 8, 16, jpegamd.CHROMA_UYVY)
    assert jpegamd._yuyv_layout(z(1, 1, 2, 2), "yuyv") == (1, 1, 2, 4, jpegamd.CHROMA_YUYV)
    big = z(6, 20, 40, 2)
    assert jpegamd._yuyv_layout(big[::2], "yuyv") == (3, 20, 40, 80, jpegamd.CHROMA_YUYV)           # strided pictures
    assert jpegamd._yuyv_layout(big[1::2, 2:18, 4:36], "uyvy") == (3, 16, 32, 80, jpegamd.CHROMA_UYVY)   # a crop: strided rows
    assert jpegamd._yuyv_layout(big[:, ::2], "yuyv") == (6, 10, 40, 160, jpegamd.CHROMA_YUYV)       # every second row
    bad = [
        (z(2, 8, 7, 2), "yuyv"),                                  # odd W
        (z(2, 8, 1, 2), "yuyv"),
        (z(2, 8, 8, 2, dtype=torch.int16), "yuyv"),               # dtype
        (z(2, 8, 8, 2, dtype=torch.float32), "uyvy"),
        (z(8, 8, 2), "yuyv"),                                     # one picture, not a batch
        (z(2, 8, 8), "yuyv"),
        (z(2, 8, 8, 4), "yuyv"),                                  # four bytes per pixel
        (z(2, 8, 16, 2)[:, :, ::2], "yuyv"),                      # an unpacked pixel stride
        (z(2, 8, 8, 4)[:, :, :, ::2], "yuyv"),                    # ... an unpacked byte stride
        (z(2, 1, 8, 2).expand(2, 8, 8, 2), "yuyv"),               # overlapping rows (row stride 0)
        (z(2, 16, 8, 2).transpose(1, 2), "yuyv"),                 # columns as rows
        (z(0, 8, 8, 2), "yuyv"),                                  # no picture
        (z(2, 8, 8, 2), "yuy2"),                                  # an unknown order
        (z(2, 8, 8, 2), "cbcr"),
        (z(2, 8, 8, 2), None),
    ]
    for i, (t, order) in enumerate(bad):
        with pytest.raises(ValueError) as err:
            jpegamd.encode_yuyv_batch(t, order=order)
        assert "device tensor" not in str(err.value), (i, str(err.value))
    for t in (z(2, 8, 8, 2), big[1::2, 2:18, 4:36]):              # well formed: only the device is missing
        with pytest.raises(ValueError, match="device tensor"):
            jpegamd.encode_yuyv_batch(t)


# ---- C-ABI argument checks: fake pointers, no launch ---------------------------------------------------------------------------------
def _fake_context():
    """A block of zeros where the context would be: a check that came too late would read it."""
    fake = (C.c_uint8 * (1 << 16))()
    return fake, C.cast(fake, C.c_void_p)


def _call(jpegamd, ctx, imgs, count, sub):
    arr = (jpegamd.YCbCrImage * len(imgs))(*imgs)
    out_arr = (C.c_void_p * 40)(*([C.c_void_p(0x1000)] * 40))
    size_arr = (C.c_void_p * 40)(*([C.c_void_p(0x2000)] * 40))
    return jpegamd.lib.jpegamd_encode_ycbcr_batch_async(ctx, arr, count, sub, out_arr, CAP, size_arr, None)


def test_packed_argument_checks_come_before_the_context(jpegamd):
    """Bad arguments are refused with ERR_ARG before the context is read.  Good ones go on to the context -- here a block of zeros,
    a context that holds no picture at all, so the call ends with ERR_TOO_LARGE before anything touches a device: that answer is how
    a call that PASSED the argument checks shows."""
    keep, ctx = _fake_context()
    s422, s420, s444 = jpegamd.SUBSAMPLE_422, jpegamd.SUBSAMPLE_420, jpegamd.SUBSAMPLE_444
    for layout in (jpegamd.CHROMA_YUYV, jpegamd.CHROMA_UYVY):
        for w in (65, 64, 1):
            row = 4 * ((w + 1) // 2)

            def img(base=0x100000, w=w, h=33, ys=row, layout=layout, q=0, cb=0, cr=0, cs=0):
                return jpegamd.Encoder.ycbcr_image(base, cb, cr, w, h, ys, cs, layout, q)

            good = [img(0x100000 * (i + 1)) for i in range(3)]
            case = (layout, w)
            # null cb / cr, c_stride 0, a stride of exactly 4 ceil(W / 2), odd W: all fine at 4:2:2
            assert good[0].cb is None and good[0].cr is None
            assert _call(jpegamd, ctx, good, 3, s422) == ERR_TOO_LARGE, case
            assert _call(jpegamd, ctx, good[:1], 1, s422) == ERR_TOO_LARGE, case
            assert _call(jpegamd, ctx, [img(ys=row + 3)], 1, s422) == ERR_TOO_LARGE, case         # any stride from there on
            assert _call(jpegamd, ctx, [img(cb=0x5001, cr=0x7003, cs=-5)], 1, s422) == ERR_TOO_LARGE, case   # cb, cr, c_stride are not looked at
            assert _call(jpegamd, None, good, 3, s422) == ERR_ARG, case
            # a packed layout at 4:2:0 or 4:4:4, or an unknown subsampling
            for sub in (s420, s444, 0, 3, -1):
                assert _call(jpegamd, ctx, good, 3, sub) == ERR_ARG, (case, sub)
                assert _call(jpegamd, ctx, good[:1], 1, sub) == ERR_ARG, (case, sub)
            # a stride below 4 ceil(W / 2): also where it would hold the Y samples alone, or W pixels of two bytes
            for ys in {row - 1, w, 2 * w - 1, 0, -row}:
                if ys < row:
                    assert _call(jpegamd, ctx, [img(ys=ys)], 1, s422) == ERR_ARG, (case, ys)
                    assert _call(jpegamd, ctx, [img(0x100000 * (i + 1), ys=ys) for i in range(3)], 3, s422) == ERR_ARG, (case, ys)
            # pictures of one batch differing in layout, geometry, stride or quality -- the odd one first or later
            other = jpegamd.CHROMA_UYVY if layout == jpegamd.CHROMA_YUYV else jpegamd.CHROMA_YUYV
            odd_ones = [img(layout=other), img(layout=jpegamd.CHROMA_PLANES, cb=0x5000, cr=0x6000, cs=row),
                        img(layout=jpegamd.CHROMA_CBCR, cb=0x5000, cs=row), img(w=w + 2, ys=row + 4), img(h=32), img(ys=row + 4), img(q=90)]
            for k, odd in enumerate(odd_ones):
                for imgs in ([good[0], odd, good[2]], [good[0], good[1], odd], [odd, good[1], good[2]]):
                    assert _call(jpegamd, ctx, imgs, 3, s422) == ERR_ARG, (case, k)
            # a null y, a bad size
            assert _call(jpegamd, ctx, [img(base=0)], 1, s422) == ERR_ARG, case
            assert _call(jpegamd, ctx, [good[0], img(base=0), good[2]], 3, s422) == ERR_ARG, case
            for bad in (img(w=0), img(w=-2), img(h=0), img(w=65536, ys=4 * 32768), img(h=65536)):
                assert _call(jpegamd, ctx, [bad], 1, s422) == ERR_ARG, case


def test_planes_and_pairs_at_422_are_sized_by_ceil_w_half_by_h(jpegamd):
    keep, ctx = _fake_context()
    s422 = jpegamd.SUBSAMPLE_422
    w, h = 65, 33
    cw = (w + 1) // 2
    for layout, c_row in ((jpegamd.CHROMA_PLANES, cw), (jpegamd.CHROMA_CBCR, 2 * cw), (jpegamd.CHROMA_CRCB, 2 * cw)):
        def img(cs, base=0x100000):
            return jpegamd.Encoder.ycbcr_image(base, base + 0x10000, base + 0x20000, w, h, w, cs, layout, 0)
        assert _call(jpegamd, ctx, [img(c_row - 1)], 1, s422) == ERR_ARG, layout          # one byte short of a 4:2:2 chroma row
        assert _call(jpegamd, ctx, [img(c_row)], 1, s422) == ERR_TOO_LARGE, layout        # the row itself passes the argument checks
        assert _call(jpegamd, ctx, [img(c_row), img(c_row, 0x400000)], 2, s422) == ERR_TOO_LARGE, layout


# ---- the model, against an independent decoder ---------------------------------------------------------------------------------------
def _psnr(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    return 10 * np.log10(255.0 ** 2 / max(np.mean(d * d), 1e-12))


def test_the_model_file_is_a_422_jpeg_and_keeps_vertical_chroma_detail(jpegamd, oracle):
    """Pins the model (passes without the feature in the library)."""
    PIL = pytest.importorskip("PIL.Image")
    from PIL import JpegImagePlugin
    w, h = 64, 48
    rgb = cm.read_bmp_rgb(jpegamd.synth_bmp(w, h, 4, 0, 0))
    im = PIL.open(io.BytesIO(m422.color_file_422(oracle, cm.write_bmp(rgb), 90)))
    assert im.size == (w, h) and im.mode == "RGB"
    assert JpegImagePlugin.get_sampling(im) == 1                  # PIL's code for 4:2:2
    im.load()
    assert _psnr(np.asarray(im), rgb) > 25
    # rows alternate between two colours of equal luma (77 R + 150 G + 29 B) >> 8 = 119: Cr differs by ~100, Cb by ~50
    a, b = (200, 90, 60), (60, 149, 125)
    luma = [(77 * r + 150 * g + 29 * bb) >> 8 for r, g, bb in (a, b)]
    assert luma[0] == luma[1]
    stripes = np.zeros((h, w, 3), np.uint8)
    stripes[0::2], stripes[1::2] = a, b
    bmp = cm.write_bmp(stripes)
    q = 95                                                        # chroma table entry (7, 0) is 99 -> 10 at quality 95: the top frequency survives
    f422 = m422.color_file_422(oracle, bmp, q)
    f420 = cm.color_file(oracle, bmp, q, cm.SUB_420)
    d422 = np.asarray(PIL.open(io.BytesIO(f422)).convert("RGB"))
    d420 = np.asarray(PIL.open(io.BytesIO(f420)).convert("RGB"))
    p422, p420 = _psnr(d422, stripes), _psnr(d420, stripes)
    print(f"PSNR of the row-striped picture at quality {q}: 4:2:2 {p422:.2f} dB, 4:2:0 {p420:.2f} dB")
    # seen with amplitude (200, 90, 60) / (60, 149, 125) at quality 95: 4:2:2 45.21 dB, 4:2:0 14.56 dB (its chroma is the flat average)
    assert p422 > p420 + 6.0, (p422, p420)
