"""YCbCr input on the CPU: the exported symbol and the ctypes mirror of the header, the argument checks of
jpegamd_encode_ycbcr_batch_async that return before the context is touched, and the shape / dtype / stride checks of
encode_ycbcr_batch.  Nothing here needs a device."""
from __future__ import annotations

import ctypes as C
import re

import pytest

ERR_ARG = -1
CAP = 1 << 20
NAME = "jpegamd_encode_ycbcr_batch_async"


def test_ycbcr_symbol_and_struct(jpegamd):
    header = jpegamd.HEADER_PATH.read_text()
    assert NAME in jpegamd.EXPORTED
    assert hasattr(C.CDLL(str(jpegamd.LIB_PATH)), NAME)
    assert NAME in header
    for name, value in (("PLANES", 0), ("CBCR", 1), ("CRCB", 2)):
        assert re.search(rf"#define\s+JPEGAMD_CHROMA_{name}\s+{value}\b", header), name
        assert getattr(jpegamd, f"CHROMA_{name}") == value
    assert "no range or matrix conversion" in header.lower()                            # the header says what is NOT done
    assert hasattr(jpegamd.Encoder, "ycbcr_image") and hasattr(jpegamd.Encoder, "encode_ycbcr_batch_async")
    # JpegAmdYCbCrImage as the header declares it: three pointers, then six int32 in this order
    body = re.search(r"typedef struct JpegAmdYCbCrImage \{(.*?)\} JpegAmdYCbCrImage;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *") for decl in body.split(";") if decl.strip()
             for n in re.sub(r"^\s*(const\s+)?\w+\s+", "", decl).split(",")]                  # the declarators behind the type
    assert names == ["y", "cb", "cr", "width", "height", "y_stride", "c_stride", "chroma_layout", "quality"]
    assert [f[0] for f in jpegamd.YCbCrImage._fields_] == names
    assert C.sizeof(jpegamd.YCbCrImage) == 3 * 8 + 6 * 4
    offsets = {n: getattr(jpegamd.YCbCrImage, n).offset for n in names}
    assert offsets == dict(y=0, cb=8, cr=16, width=24, height=28, y_stride=32, c_stride=36, chroma_layout=40, quality=44)
    img = jpegamd.Encoder.ycbcr_image(0x100, 0x200, 0, 5, 4, 8, 6, jpegamd.CHROMA_CBCR, 90)
    assert (img.y, img.cb, img.cr) == (0x100, 0x200, None)
    assert (img.width, img.height, img.y_stride, img.c_stride, img.chroma_layout, img.quality) == (5, 4, 8, 6, 1, 90)


def _fake_context():
    """A block of zeros where the context would be: a check that came too late would read it."""
    fake = (C.c_uint8 * (1 << 16))()
    return fake, C.cast(fake, C.c_void_p)


def _call(jpegamd, ctx, imgs, count, sub, outs=True, sizes=True, null_out=None, null_size=None):
    n = max(len(imgs), 1)
    arr = (jpegamd.YCbCrImage * n)(*imgs) if imgs else None
    out_arr = (C.c_void_p * 40)(*([C.c_void_p(0x1000)] * 40)) if outs else None
    size_arr = (C.c_void_p * 40)(*([C.c_void_p(0x2000)] * 40)) if sizes else None
    if null_out is not None:
        out_arr[null_out] = None
    if null_size is not None:
        size_arr[null_size] = None
    return jpegamd.lib.jpegamd_encode_ycbcr_batch_async(ctx, arr, count, sub, out_arr, CAP, size_arr, None)


def test_ycbcr_argument_checks_come_before_the_context(jpegamd):
    keep, ctx = _fake_context()
    s420, s444 = jpegamd.SUBSAMPLE_420, jpegamd.SUBSAMPLE_444
    planes, cbcr, crcb = jpegamd.CHROMA_PLANES, jpegamd.CHROMA_CBCR, jpegamd.CHROMA_CRCB

    for sub in (s444, s420):
        for layout in (planes, cbcr, crcb):
            w, h = 65, 33                                                                   # odd both ways: cw = 33 at 4:2:0
            cw = (w + 1) // 2 if sub == s420 else w
            c_row = cw if layout == planes else 2 * cw

            def img(base=0x100000, w=w, h=h, ys=None, cs=None, layout=layout, q=0, ptrs=None):
                y, cb, cr = ptrs or (base, base + 0x10000, base + 0x20000)
                return jpegamd.Encoder.ycbcr_image(y, cb, cr, w, h, w if ys is None else ys, c_row if cs is None else cs, layout, q)

            def first_and_later(bad):
                """`bad` as the only picture, as the first of three and as a later one."""
                return [([bad], 1), ([bad, good[1], good[2]], 3), ([good[0], bad, good[2]], 3), ([good[0], good[1], bad], 3)]

            good = [img(0x100000 * (i + 1)) for i in range(40)]
            case = (sub, layout)
            assert _call(jpegamd, None, good[:2], 2, sub) == ERR_ARG, case                 # null context
            assert _call(jpegamd, ctx, [], 1, sub) == ERR_ARG, case                        # null array
            assert _call(jpegamd, ctx, good[:1], 0, sub) == ERR_ARG, case                  # count out of range
            assert _call(jpegamd, ctx, good[:1], -1, sub) == ERR_ARG, case
            assert _call(jpegamd, ctx, good[:33], 33, sub) == ERR_ARG, case
            assert _call(jpegamd, ctx, good[:2], 2, sub, outs=False) == ERR_ARG, case
            assert _call(jpegamd, ctx, good[:2], 2, sub, sizes=False) == ERR_ARG, case
            for k in (0, 2):                                                                # a null element, first or later
                assert _call(jpegamd, ctx, good[:3], 3, sub, null_out=k) == ERR_ARG, case
                assert _call(jpegamd, ctx, good[:3], 3, sub, null_size=k) == ERR_ARG, case
            # null y, null cb, and null cr where two planes are meant
            nulls = [(0, 0x6000, 0x7000), (0x5000, 0, 0x7000)] + ([(0x5000, 0x6000, 0)] if layout == planes else [])
            for ptrs in nulls:
                for imgs, n in first_and_later(img(ptrs=ptrs)):
                    assert _call(jpegamd, ctx, imgs, n, sub) == ERR_ARG, (case, ptrs, n)
            # a stride too short: every picture carries it (one geometry), so the first picture decides
            for kw in (dict(ys=w - 1), dict(cs=c_row - 1), dict(ys=0), dict(cs=0), dict(cs=-c_row)):
                assert _call(jpegamd, ctx, [img(**kw)], 1, sub) == ERR_ARG, (case, kw)
                assert _call(jpegamd, ctx, [img(0x100000 * (i + 1), **kw) for i in range(3)], 3, sub) == ERR_ARG, (case, kw)
            if layout != planes:                                                            # a pair row is 2 cw bytes
                assert _call(jpegamd, ctx, [img(cs=2 * cw - 1)], 1, sub) == ERR_ARG, case
                assert _call(jpegamd, ctx, [img(cs=cw)], 1, sub) == ERR_ARG, case
            for bad in (img(w=0, ys=8, cs=8), img(w=-3, ys=8, cs=8), img(h=0), img(h=-1), img(w=65536, ys=65536, cs=2 * 65536),
                        img(h=65536)):
                assert _call(jpegamd, ctx, [bad], 1, sub) == ERR_ARG, case
            for bad_layout in (3, -1, 7):                                                   # an unknown layout
                for imgs, n in first_and_later(img(layout=bad_layout, cs=2 * w)):
                    assert _call(jpegamd, ctx, imgs, n, sub) == ERR_ARG, (case, bad_layout, n)
            # mixed geometry: width, height, either stride, layout, quality -- in the first picture or a later one
            other = cbcr if layout == planes else planes
            for odd in (img(w=w - 1), img(h=h - 1), img(ys=w + 4), img(cs=c_row + 4), img(layout=other, cs=2 * w), img(q=90)):
                for imgs, n in first_and_later(odd)[1:]:
                    assert _call(jpegamd, ctx, imgs, n, sub) == ERR_ARG, (case, n)
    good = [jpegamd.Encoder.ycbcr_image(0x1000 * (i + 1), 0x100000, 0x200000, 64, 32, 64, 64, planes, 0) for i in range(2)]
    for sub in (0, 3, -1):                                                                  # an unknown subsampling
        assert _call(jpegamd, ctx, good, 2, sub) == ERR_ARG, sub
        assert _call(jpegamd, ctx, good[:1], 1, sub) == ERR_ARG, sub


def test_encode_ycbcr_batch_rejects_bad_tensors(jpegamd):
    torch = pytest.importorskip("torch")
    u8 = torch.uint8
    s420, s444 = jpegamd.SUBSAMPLE_420, jpegamd.SUBSAMPLE_444

    def z(*shape, dtype=u8):
        return torch.zeros(*shape, dtype=dtype)

    bad = [
        (dict(y=z(2, 8, 8, dtype=torch.float32), cb=z(2, 4, 4), cr=z(2, 4, 4)), s420),     # dtype
        (dict(y=z(2, 8, 8), cb=z(2, 4, 4, dtype=torch.int16), cr=z(2, 4, 4)), s420),
        (dict(y=z(2, 8, 8), cb=z(2, 4, 4), cr=z(2, 4, 4, dtype=torch.int8)), s420),
        (dict(y=z(2, 8, 8), cb=z(2, 4, 4, 2, dtype=torch.int16)), s420),
        (dict(y=z(2, 8, 8), cb=z(2, 8, 8), cr=z(2, 8, 8)), s420),                          # chroma shape for the subsampling
        (dict(y=z(2, 8, 8), cb=z(2, 4, 4), cr=z(2, 4, 4)), s444),
        (dict(y=z(2, 8, 8), cb=z(2, 4, 4), cr=z(2, 4, 5)), s420),
        (dict(y=z(2, 8, 8), cb=z(3, 4, 4), cr=z(3, 4, 4)), s420),
        (dict(y=z(2, 9, 7), cb=z(2, 4, 3), cr=z(2, 4, 3)), s420),                          # odd W and H: ceil, not floor
        (dict(y=z(2, 9, 7), cb=z(2, 5, 3), cr=z(2, 5, 3)), s420),
        (dict(y=z(2, 9, 7), cb=z(2, 4, 4), cr=z(2, 4, 4)), s420),
        (dict(y=z(2, 9, 7), cb=z(2, 4, 3, 2)), s420),
        (dict(y=z(2, 9, 7), cb=z(2, 5, 4, 2)), s444),
        (dict(y=z(2, 8, 8), cb=z(2, 4, 4, 3)), s420),                                      # pairs are two bytes
        (dict(y=z(8, 8), cb=z(4, 4), cr=z(4, 4)), s420),                                   # one picture, not a batch
        (dict(y=z(2, 8, 16)[:, :, ::2], cb=z(2, 4, 4), cr=z(2, 4, 4)), s420),              # a strided sample
        (dict(y=z(2, 8, 8), cb=z(2, 4, 8)[:, :, ::2], cr=z(2, 4, 4)), s420),
        (dict(y=z(2, 8, 8), cb=z(2, 4, 4), cr=z(2, 4, 8)[:, :, ::2]), s420),
        (dict(y=z(2, 8, 8), cb=z(2, 4, 8, 2)[:, :, ::2]), s420),
        (dict(y=z(2, 8, 8), cb=z(2, 4, 4, 4)[:, :, :, ::2]), s420),
        (dict(y=z(2, 8, 8), cb=z(2, 4, 4), cr=z(2, 4, 6)[:, :, :4]), s420),                # cb and cr rows 4 and 6 bytes apart
        (dict(y=z(2, 8, 8), cb=z(2, 4, 4)), s420),                                         # cr=None with a 3-D cb
        (dict(y=z(2, 8, 8), cb=z(2, 4, 8)), s420),
        (dict(y=z(2, 8, 8), cb=z(2, 4, 4, 2), order="nv12"), s420),                        # an unknown order
        (dict(y=z(2, 8, 8), cb=z(2, 4, 4, 2), order="CBCR"), s420),
        (dict(y=z(2, 8, 8), cb=z(2, 4, 4), cr=z(2, 4, 4), order="yv12"), s420),
        (dict(y=z(2, 8, 8), cb=z(2, 4, 4, 2), order=None), s420),
        (dict(y=z(2, 8, 8), cb=z(2, 4, 4, 2)), 0),                                         # an unknown subsampling
        (dict(y=z(0, 8, 8), cb=z(0, 4, 4, 2)), s420),                                      # no picture
    ]
    for i, (kw, sub) in enumerate(bad):
        with pytest.raises(ValueError) as err:
            jpegamd.encode_ycbcr_batch(subsampling=sub, **kw)
        assert "device tensor" not in str(err.value), (i, str(err.value))


def test_well_formed_host_ycbcr_tensors_only_lack_a_device(jpegamd):
    torch = pytest.importorskip("torch")
    u8 = torch.uint8
    s420, s444 = jpegamd.SUBSAMPLE_420, jpegamd.SUBSAMPLE_444
    h, w = 16, 24
    frames = torch.zeros(4, 3 * h // 2, w, dtype=u8)                                       # NV12 frames, sliced as the docstring shows
    frame = frames[0]
    big = torch.zeros(6, 40, 48, dtype=u8)
    good = [
        (dict(y=torch.zeros(2, 8, 8, dtype=u8), cb=torch.zeros(2, 4, 4, dtype=u8), cr=torch.zeros(2, 4, 4, dtype=u8)), s420),
        (dict(y=torch.zeros(2, 9, 7, dtype=u8), cb=torch.zeros(2, 5, 4, dtype=u8), cr=torch.zeros(2, 5, 4, dtype=u8)), s420),
        (dict(y=torch.zeros(2, 9, 7, dtype=u8), cb=torch.zeros(2, 5, 4, 2, dtype=u8)), s420),
        (dict(y=torch.zeros(2, 9, 7, dtype=u8), cb=torch.zeros(2, 9, 7, 2, dtype=u8), order="crcb"), s444),
        (dict(y=torch.zeros(1, 1, 1, dtype=u8), cb=torch.zeros(1, 1, 1, 2, dtype=u8)), s420),
        (dict(y=frame[:h].unsqueeze(0), cb=frame[h:].view(h // 2, w // 2, 2).unsqueeze(0)), s420),
        (dict(y=frames[:, :h], cb=frames[:, h:].unflatten(2, (w // 2, 2))), s420),
        (dict(y=frames[::2, :h], cb=frames[::2, h:].unflatten(2, (w // 2, 2)), order="crcb"), s420),
        (dict(y=big[::2, 2:34, 4:36], cb=big[1::2, :16, :16], cr=big[1::2, 16:32, 16:32]), s420),   # crops: strided rows and pictures
        (dict(y=big[:3, :20, :30], cb=big[3:, :20, :30], cr=big[3:, 20:, :30]), s444),
    ]
    for i, (kw, sub) in enumerate(good):
        with pytest.raises(ValueError, match="device tensor"):
            jpegamd.encode_ycbcr_batch(subsampling=sub, **kw)
