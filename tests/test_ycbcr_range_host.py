"""Limited-range YCbCr input on the CPU: the exported symbol and the two range constants, the map itself (from its definition, and
the fixed-point forms that must equal it), the argument checks of jpegamd_encode_ycbcr_range_batch_async that return before the
context is touched, and the sample_range argument of the tensor entries.  Nothing here needs a device."""
from __future__ import annotations

import ctypes as C
import re

import numpy as np
import pytest

import range_model as rm

ERR_ARG = -1
CAP = 1 << 20
NAME = "jpegamd_encode_ycbcr_range_batch_async"


def test_range_symbol_and_constants(jpegamd):
    header = jpegamd.HEADER_PATH.read_text()
    assert NAME in jpegamd.EXPORTED
    assert hasattr(C.CDLL(str(jpegamd.LIB_PATH)), NAME)
    assert re.search(rf"int32_t\s+{NAME}\s*\(", header)
    for name, value in (("FULL", 0), ("LIMITED", 1)):
        assert re.search(rf"#define\s+JPEGAMD_RANGE_{name}\s+{value}\b", header), name
        assert getattr(jpegamd, f"RANGE_{name}") == value
    assert "no range or matrix conversion" in header.lower()        # the full-range entry still says what it does NOT do
    assert "jpegamd_encode_ycbcr_batch_async" in jpegamd.EXPORTED   # ... and is still there
    # the prototype: the range sits between the subsampling and the outputs
    proto = re.search(rf"{NAME}\s*\((.*?)\)\s*;", header, re.S).group(1)
    names = [re.sub(r".*[\s*]", "", p.strip()) for p in proto.split(",")]
    assert names == ["enc", "imgs", "count", "subsampling", "sample_range", "outs_dev", "out_capacity", "out_sizes_dev", "stream"]
    assert len(jpegamd.lib.jpegamd_encode_ycbcr_range_batch_async.argtypes) == len(names)


def test_the_map():
    ymap, cmap = rm.luma_table(), rm.chroma_table()
    assert ymap.shape == cmap.shape == (256,) and ymap.dtype == cmap.dtype == np.uint8
    #            0  15  16  17  128  234  235  236  240  241  255
    pins = (0, 15, 16, 17, 128, 234, 235, 236, 240, 241, 255)
    assert [int(ymap[v]) for v in pins] == [0, 0, 0, 1, 130, 254, 255, 255, 255, 255, 255]
    assert [int(cmap[v]) for v in pins] == [0, 0, 0, 1, 128, 248, 249, 250, 255, 255, 255]
    assert cmap[128] == 128                                           # neutral chroma stays neutral
    for tab, lo, hi in ((ymap, 16, 235), (cmap, 16, 240)):
        assert np.all(np.diff(tab.astype(int)) >= 0)                  # monotone
        assert np.all(tab[:lo + 1] == 0) and np.all(tab[hi:] == 255)  # everything outside the nominal range clamps
        assert tab[lo + 1] > 0 and tab[hi - 1] < 255                  # ... and nothing inside it does
        assert set(np.diff(tab[lo:hi + 1].astype(int))) == {1, 2}     # strictly increasing inside: an expansion
    # the fixed-point forms equal the definition for every t (and their products fit 24 and 16 bits)
    for t in range(220):
        assert rm.luma_mad24(t) == rm.luma_split16(t) == int(ymap[t + 16]), t
    for t in range(225):
        assert rm.chroma_mad24(t) == rm.chroma_split16(t) == int(cmap[t + 16]), t
    assert 2385 * 219 + 986 < 1 << 20 and 4663 * 224 + 2032 < 1 << 20
    assert 81 * 219 + 986 < 1 << 15 and 9 * 219 + 255 < 1 << 15 and 55 * 224 + 2032 < 1 << 15 and 18 * 224 + 255 < 1 << 15
    y = np.arange(256, dtype=np.uint8).reshape(16, 16)
    ey, ecb, ecr = rm.expand((y, y, y.T))
    assert np.array_equal(ey, ymap.reshape(16, 16)) and np.array_equal(ecb, cmap.reshape(16, 16)) and np.array_equal(ecr, ecb.T)


def _fake_context():
    """A block of zeros where the context would be: a check that came too late would read it."""
    fake = (C.c_uint8 * (1 << 16))()
    return fake, C.cast(fake, C.c_void_p)


def _call(jpegamd, ctx, imgs, count, sub, rng, outs=True, sizes=True):
    n = max(len(imgs), 1)
    arr = (jpegamd.YCbCrImage * n)(*imgs) if imgs else None
    out_arr = (C.c_void_p * 40)(*([C.c_void_p(0x1000)] * 40)) if outs else None
    size_arr = (C.c_void_p * 40)(*([C.c_void_p(0x2000)] * 40)) if sizes else None
    return jpegamd.lib.jpegamd_encode_ycbcr_range_batch_async(ctx, arr, count, sub, rng, out_arr, CAP, size_arr, None)


def test_range_argument_checks_come_before_the_context(jpegamd):
    keep, ctx = _fake_context()
    s420, s444, s422 = jpegamd.SUBSAMPLE_420, jpegamd.SUBSAMPLE_444, jpegamd.SUBSAMPLE_422
    w, h = 64, 32

    def img(i=0, layout=jpegamd.CHROMA_PLANES, ys=w, cs=w, q=0, y=None):
        base = 0x100000 * (i + 1)
        return jpegamd.Encoder.ycbcr_image(base if y is None else y, base + 0x10000, base + 0x20000, w, h, ys, cs, layout, q)

    good = [img(i) for i in range(40)]
    packed = [img(i, jpegamd.CHROMA_YUYV, ys=2 * w) for i in range(2)]
    # an unknown range: otherwise perfect arguments, every subsampling and count
    for rng in (-1, 2, 3):
        for sub in (s444, s420, s422):
            assert _call(jpegamd, ctx, good[:1], 1, sub, rng) == ERR_ARG, (rng, sub)
            assert _call(jpegamd, ctx, good[:3], 3, sub, rng) == ERR_ARG, (rng, sub)
        assert _call(jpegamd, ctx, packed, 2, s422, rng) == ERR_ARG, rng
    # a valid range: every refusal of the full-range entry still fires, before the context is read
    for rng in (jpegamd.RANGE_FULL, jpegamd.RANGE_LIMITED):
        assert _call(jpegamd, None, good[:2], 2, s420, rng) == ERR_ARG                     # null context
        assert _call(jpegamd, ctx, [], 1, s420, rng) == ERR_ARG                            # null array
        assert _call(jpegamd, ctx, good[:1], 0, s420, rng) == ERR_ARG                      # count out of range
        assert _call(jpegamd, ctx, good[:1], -1, s420, rng) == ERR_ARG
        assert _call(jpegamd, ctx, good[:33], 33, s420, rng) == ERR_ARG
        assert _call(jpegamd, ctx, good[:2], 2, s420, rng, outs=False) == ERR_ARG
        assert _call(jpegamd, ctx, good[:2], 2, s420, rng, sizes=False) == ERR_ARG
        for sub in (s444, s420):                                                            # a packed layout is 4:2:2 alone
            assert _call(jpegamd, ctx, packed, 2, sub, rng) == ERR_ARG, sub
        for sub in (0, 3, -1):                                                              # an unknown subsampling
            assert _call(jpegamd, ctx, good[:2], 2, sub, rng) == ERR_ARG, sub
        for kw in (dict(ys=w - 1), dict(cs=w - 1), dict(cs=0), dict(layout=jpegamd.CHROMA_CBCR, cs=2 * w - 1)):   # a stride too short
            assert _call(jpegamd, ctx, [img(**kw)], 1, s444, rng) == ERR_ARG, kw
        assert _call(jpegamd, ctx, [img(0, jpegamd.CHROMA_UYVY, ys=2 * w - 1)], 1, s422, rng) == ERR_ARG
        assert _call(jpegamd, ctx, [img(layout=3)], 1, s444, rng) == ERR_ARG               # an unknown layout
        assert _call(jpegamd, ctx, [img(y=0)], 1, s444, rng) == ERR_ARG                    # a null plane
        assert _call(jpegamd, ctx, [good[0], img(1, q=90)], 2, s444, rng) == ERR_ARG       # mixed geometry


def test_a_bad_sample_range_is_a_value_error_on_host_tensors(jpegamd):
    torch = pytest.importorskip("torch")
    y, cb, cr = (torch.zeros(2, 8, 8, dtype=torch.uint8), torch.zeros(2, 4, 4, dtype=torch.uint8), torch.zeros(2, 4, 4, dtype=torch.uint8))
    frames = torch.zeros(2, 8, 8, 2, dtype=torch.uint8)
    for bad in ("video", "LIMITED", "", None, 1, jpegamd.RANGE_LIMITED, b"limited"):
        with pytest.raises(ValueError, match="sample_range"):
            jpegamd.encode_ycbcr_batch(y, cb, cr, sample_range=bad)
        with pytest.raises(ValueError, match="sample_range"):
            jpegamd.encode_yuyv_batch(frames, sample_range=bad)
    # a good one passes that check: well-formed host tensors then only lack a device
    for ok in ("full", "limited"):
        with pytest.raises(ValueError, match="device tensor"):
            jpegamd.encode_ycbcr_batch(y, cb, cr, sample_range=ok)
        with pytest.raises(ValueError, match="device tensor"):
            jpegamd.encode_yuyv_batch(frames, sample_range=ok)
