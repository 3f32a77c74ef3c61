"""10-bit YCbCr input on the CPU: the exported symbol and the three format constants, the maps themselves (from their definition, and
the fixed-point forms that must equal it), what one rounding from ten bits gains over two, the argument checks of
jpegamd_encode_ycbcr_samples_batch_async that return before the context is touched, and the host-only checks of the tensor entry.
Nothing here needs a device."""
from __future__ import annotations

import ctypes as C
import re

import numpy as np
import pytest

import depth_model as dm
import range_model as rm

ERR_ARG = -1
CAP = 1 << 20
NAME = "jpegamd_encode_ycbcr_samples_batch_async"
PINS = (0, 63, 64, 65, 512, 939, 940, 941, 960, 961, 1023)


def test_samples_symbol_and_constants(jpegamd):
    header = jpegamd.HEADER_PATH.read_text()
    assert NAME in jpegamd.EXPORTED
    assert hasattr(C.CDLL(str(jpegamd.LIB_PATH)), NAME)
    assert re.search(rf"int32_t\s+{NAME}\s*\(", header)
    for name, value in (("8", 0), ("10_MSB", 1), ("10_LSB", 2)):
        assert re.search(rf"#define\s+JPEGAMD_SAMPLES_{name}\s+{value}\b", header), name
        assert getattr(jpegamd, f"SAMPLES_{name}") == value
    for older in ("jpegamd_encode_ycbcr_batch_async", "jpegamd_encode_ycbcr_range_batch_async"):
        assert older in jpegamd.EXPORTED and hasattr(jpegamd.lib, older)
    # the prototype: the format sits between the range and the outputs
    proto = re.search(rf"{NAME}\s*\((.*?)\)\s*;", header, re.S).group(1)
    names = [re.sub(r".*[\s*]", "", p.strip()) for p in proto.split(",")]
    assert names == ["enc", "imgs", "count", "subsampling", "sample_range", "sample_format", "outs_dev", "out_capacity", "out_sizes_dev",
                     "stream"]
    assert len(getattr(jpegamd.lib, NAME).argtypes) == len(names)
    # the header carries the maps, and says what is not taken
    for text in ("(v + 2) >> 2", "clamp(v, 64, 940) - 64) + 438) / 876", "clamp(v, 64, 960) - 64) + 448) / 896", "w >> 6", "min(w, 1023)", "Y210"):
        assert text in header, text


def test_the_maps():
    full, ymap, cmap = dm.full_table(), dm.luma_table(), dm.chroma_table()
    for tab in (full, ymap, cmap):
        assert tab.shape == (1024,) and tab.dtype == np.uint8
    assert dm.table(dm.FULL, False) is not None and np.array_equal(dm.table(dm.FULL, True), full)
    assert np.array_equal(dm.table(dm.LIMITED, False), ymap) and np.array_equal(dm.table(dm.LIMITED, True), cmap)
    #                                            0  63  64  65  512  939  940  941  960  961  1023
    assert [int(full[v]) for v in PINS] == [0, 16, 16, 16, 128, 235, 235, 235, 240, 240, 255]
    assert [int(ymap[v]) for v in PINS] == [0, 0, 0, 0, 130, 255, 255, 255, 255, 255, 255]
    assert [int(cmap[v]) for v in PINS] == [0, 0, 0, 0, 128, 249, 249, 250, 255, 255, 255]
    assert full[512] == 128 and cmap[512] == 128                       # neutral chroma stays 128
    assert full[1] == 0 and full[2] == 1 and full[1021] == 255 and full[1017] == 254      # round half up, then the cap
    for tab in (full, ymap, cmap):
        assert np.all(np.diff(tab.astype(int)) >= 0)                  # monotone
        assert set(tab.tolist()) == set(range(256))                   # every output level is reached
    for tab, lo, hi in ((ymap, 64, 940), (cmap, 64, 960)):
        assert np.all(tab[:lo + 1] == 0) and np.all(tab[hi:] == 255)  # everything outside the nominal range clamps
        assert tab[lo + 2] > 0 and tab[hi - 2] < 255                  # ... and the ends are reached at the ends (within a rounding step)
        assert set(np.diff(tab[lo:hi + 1].astype(int))) == {0, 1}     # a narrowing: no level skipped


def test_the_fixed_point_forms_equal_the_definition():
    full, ymap, cmap = dm.full_table(), dm.luma_table(), dm.chroma_table()
    # the limited maps: every t of the clamped range, and every 16-bit v in front of the clamp
    for v in range(65536):
        vy, ty = dm.kernel_luma(v)
        vc, tc = dm.kernel_chroma(v)
        assert vy == int(ymap[min(v, 1023)]) and vc == int(cmap[min(v, 1023)]), v
        assert ty[0] <= 876 and ty[1] < 1 << 24 and 19077 < 1 << 24    # a 24-bit multiply-add whose byte 2 is the result
        assert ty[1] >> 24 == 0 and (ty[1] >> 16) <= 255
        assert tc[0] <= 896 and all(0 <= x < 1 << 16 for x in tc)
    assert {dm.kernel_luma(t + 64)[0] for t in range(877)} == set(range(256))
    # the chroma addend: the whole stated window works, its neighbours do not
    def chroma_with(addend):
        return all((18 * t + ((55 * t + addend) >> 8)) >> 6 == int(cmap[t + 64]) for t in range(897))
    assert all(chroma_with(a) for a in range(8128, 8146)) and not chroma_with(8127) and not chroma_with(8146)
    # the full map: any 16-bit v (an LSB-aligned word is clamped inside the form)
    for v in range(65536):
        s, terms = dm.kernel_full(v)
        assert s == int(full[min(v, 1023)]) and all(0 <= x < 1 << 16 for x in terms), v
    # ... and the one-add form of an MSB-aligned word
    for w in range(65536):
        s, terms = dm.kernel_msb_full(w)
        assert s == int(full[w >> 6]) and terms[0] < 1 << 16, w


def test_alignments_over_every_word():
    msb, lsb = dm.value_table(dm.MSB), dm.value_table(dm.LSB)
    w = np.arange(65536)
    assert msb.shape == lsb.shape == (65536,)
    assert np.array_equal(msb, w >> 6) and msb.max() == 1023
    assert np.array_equal(msb[w & ~63], msb) and np.array_equal(msb[w | 63], msb)       # the low six bits are ignored
    assert np.array_equal(lsb[:1024], w[:1024]) and np.all(lsb[1024:] == 1023)           # larger words clamp
    for shift, tab in ((6, msb), (0, lsb)):
        assert all(min(dm.kernel_value(int(x), shift), 1023) == int(tab[x]) for x in range(0, 65536, 7))
    # narrow(): the bit pattern counts (int16 = uint16), planes keep their shapes
    rng = np.random.default_rng(5)
    planes = tuple(rng.integers(0, 65536, s).astype(np.uint16) for s in ((9, 17), (5, 9), (5, 9)))
    for sr in (dm.FULL, dm.LIMITED):
        for al in (dm.MSB, dm.LSB):
            got = dm.narrow(planes, sr, al)
            assert [g.shape for g in got] == [p.shape for p in planes] and all(g.dtype == np.uint8 for g in got)
            again = dm.narrow(tuple(p.view(np.int16) for p in planes), sr, al)
            assert all(np.array_equal(a, b) for a, b in zip(got, again))
            val = dm.value_table(al)
            assert np.array_equal(got[0], dm.table(sr, False)[val[planes[0]]]) and np.array_equal(got[2], dm.table(sr, True)[val[planes[2]]])


def test_one_rounding_beats_two():
    """Limited range the long way round -- narrow to 8 bits ((v + 2) >> 2), then the 8-bit JPEGAMD_RANGE_LIMITED map -- against the
    direct map, over all 1024 values: the detour is off by one on 252 (Y) and 255 (Cb / Cr) of them, never by more, and reaches 220 and
    225 of the 256 output levels where the direct map reaches them all."""
    eight = dm.full_table()
    for direct, detour_map, differs, levels in ((dm.luma_table(), rm.luma_table(), 252, 220), (dm.chroma_table(), rm.chroma_table(), 255, 225)):
        detour = detour_map[eight]
        diff = direct.astype(int) - detour.astype(int)
        assert int(np.count_nonzero(diff)) == differs
        assert int(np.abs(diff).max()) == 1
        assert len(set(detour.tolist())) == levels and len(set(direct.tolist())) == 256


def _fake_context():
    """A block of zeros where the context would be: a check that came too late would read it."""
    fake = (C.c_uint8 * (1 << 16))()
    return fake, C.cast(fake, C.c_void_p)


def _call(jpegamd, ctx, imgs, count, sub, rng, fmt, outs=True, sizes=True):
    n = max(len(imgs), 1)
    arr = (jpegamd.YCbCrImage * n)(*imgs) if imgs else None
    out_arr = (C.c_void_p * 40)(*([C.c_void_p(0x1000)] * 40)) if outs else None
    size_arr = (C.c_void_p * 40)(*([C.c_void_p(0x2000)] * 40)) if sizes else None
    return getattr(jpegamd.lib, NAME)(ctx, arr, count, sub, rng, fmt, out_arr, CAP, size_arr, None)


def test_samples_argument_checks_come_before_the_context(jpegamd):
    keep, ctx = _fake_context()
    s420, s444, s422 = jpegamd.SUBSAMPLE_420, jpegamd.SUBSAMPLE_444, jpegamd.SUBSAMPLE_422
    planes_l, cbcr, crcb = jpegamd.CHROMA_PLANES, jpegamd.CHROMA_CBCR, jpegamd.CHROMA_CRCB
    w, h = 64, 32

    def img(i=0, layout=planes_l, ys=2 * w, cs=4 * w, q=0, y=None):
        base = 0x100000 * (i + 1)
        return jpegamd.Encoder.ycbcr_image(base if y is None else y, base + 0x10000, base + 0x20000, w, h, ys, cs, layout, q)

    good = [img(i) for i in range(40)]
    ranges = (jpegamd.RANGE_FULL, jpegamd.RANGE_LIMITED)
    wide = (jpegamd.SAMPLES_10_MSB, jpegamd.SAMPLES_10_LSB)
    # an unknown format: otherwise perfect arguments
    for fmt in (-1, 3, 4, 16):
        for rng in ranges:
            for sub in (s444, s420, s422):
                assert _call(jpegamd, ctx, good[:1], 1, sub, rng, fmt) == ERR_ARG, (fmt, rng, sub)
                assert _call(jpegamd, ctx, good[:3], 3, sub, rng, fmt) == ERR_ARG, (fmt, rng, sub)
    for fmt in wide:
        for rng in ranges:
            # a packed layout with a 16-bit format (Y210), whatever its stride
            for layout in (jpegamd.CHROMA_YUYV, jpegamd.CHROMA_UYVY):
                for ys in (2 * w, 4 * w, 8 * w):
                    assert _call(jpegamd, ctx, [img(0, layout, ys=ys)], 1, s422, rng, fmt) == ERR_ARG, (fmt, layout, ys)
            # strides one byte short, layout by layout and subsampling by subsampling (cw = w, or w / 2)
            for sub, cw in ((s444, w), (s420, w // 2), (s422, w // 2)):
                for layout, row in ((planes_l, 2 * cw), (cbcr, 4 * cw), (crcb, 4 * cw)):
                    assert _call(jpegamd, ctx, [img(0, layout, ys=2 * w - 1, cs=row)], 1, sub, rng, fmt) == ERR_ARG, (fmt, sub, layout)
                    assert _call(jpegamd, ctx, [img(0, layout, ys=2 * w, cs=row - 1)], 1, sub, rng, fmt) == ERR_ARG, (fmt, sub, layout)
            assert _call(jpegamd, ctx, [img(ys=w)], 1, s444, rng, fmt) == ERR_ARG            # the 8-bit minimum is not enough
            assert _call(jpegamd, ctx, [img(layout=cbcr, cs=2 * w)], 1, s444, rng, fmt) == ERR_ARG
            # a mixed batch
            for other in (img(1, q=90), img(1, ys=2 * w + 4), img(1, cs=4 * w + 4), img(1, layout=cbcr)):
                assert _call(jpegamd, ctx, [good[0], other], 2, s444, rng, fmt) == ERR_ARG
            # what the older entries refuse
            assert _call(jpegamd, None, good[:2], 2, s420, rng, fmt) == ERR_ARG               # null context
            assert _call(jpegamd, ctx, [], 1, s420, rng, fmt) == ERR_ARG                      # null array
            for count in (0, -1, 33):
                assert _call(jpegamd, ctx, good[:max(count, 1)], count, s420, rng, fmt) == ERR_ARG
            assert _call(jpegamd, ctx, good[:2], 2, s420, rng, fmt, outs=False) == ERR_ARG
            assert _call(jpegamd, ctx, good[:2], 2, s420, rng, fmt, sizes=False) == ERR_ARG
            for sub in (0, 3, -1):
                assert _call(jpegamd, ctx, good[:2], 2, sub, rng, fmt) == ERR_ARG, sub
            assert _call(jpegamd, ctx, [img(layout=3)], 1, s444, rng, fmt) == ERR_ARG         # an unknown layout
            assert _call(jpegamd, ctx, [img(y=0)], 1, s444, rng, fmt) == ERR_ARG              # a null plane
        for rng in (-1, 2):
            assert _call(jpegamd, ctx, good[:2], 2, s420, rng, fmt) == ERR_ARG                # an unknown range


def test_samples_8_reaches_the_checks_of_the_range_entry(jpegamd):
    """One byte per sample through the new entry: the strides are counted in samples of one byte again, and every refusal fires."""
    keep, ctx = _fake_context()
    s420, s444, s422 = jpegamd.SUBSAMPLE_420, jpegamd.SUBSAMPLE_444, jpegamd.SUBSAMPLE_422
    w, h = 64, 32
    fmt = jpegamd.SAMPLES_8

    def img(i=0, layout=jpegamd.CHROMA_PLANES, ys=w, cs=w, q=0, y=None):
        base = 0x100000 * (i + 1)
        return jpegamd.Encoder.ycbcr_image(base if y is None else y, base + 0x10000, base + 0x20000, w, h, ys, cs, layout, q)

    good = [img(i) for i in range(40)]
    packed = [img(i, jpegamd.CHROMA_YUYV, ys=2 * w) for i in range(2)]
    for rng in (jpegamd.RANGE_FULL, jpegamd.RANGE_LIMITED):
        for kw in (dict(ys=w - 1), dict(cs=w - 1), dict(cs=0), dict(layout=jpegamd.CHROMA_CBCR, cs=2 * w - 1)):
            assert _call(jpegamd, ctx, [img(**kw)], 1, s444, rng, fmt) == ERR_ARG, kw
        assert _call(jpegamd, ctx, [img(0, jpegamd.CHROMA_UYVY, ys=2 * w - 1)], 1, s422, rng, fmt) == ERR_ARG
        for sub in (s444, s420):                                                            # a packed layout is 4:2:2 alone
            assert _call(jpegamd, ctx, packed, 2, sub, rng, fmt) == ERR_ARG, sub
        assert _call(jpegamd, None, good[:2], 2, s420, rng, fmt) == ERR_ARG
        assert _call(jpegamd, ctx, good[:33], 33, s420, rng, fmt) == ERR_ARG
        assert _call(jpegamd, ctx, [img(layout=3)], 1, s444, rng, fmt) == ERR_ARG
        assert _call(jpegamd, ctx, [img(y=0)], 1, s444, rng, fmt) == ERR_ARG
        assert _call(jpegamd, ctx, [good[0], img(1, q=90)], 2, s444, rng, fmt) == ERR_ARG
    for rng in (-1, 2, 3):
        assert _call(jpegamd, ctx, good[:1], 1, s420, rng, fmt) == ERR_ARG
        assert _call(jpegamd, ctx, packed, 2, s422, rng, fmt) == ERR_ARG


def test_ycbcr16_layout_accepts_and_refuses(jpegamd):
    torch = pytest.importorskip("torch")
    lay = jpegamd._ycbcr16_layout
    s420, s444, s422 = jpegamd.SUBSAMPLE_420, jpegamd.SUBSAMPLE_444, jpegamd.SUBSAMPLE_422
    n, h, w = 2, 9, 17
    for dt in (torch.int16, torch.uint16):
        y = torch.zeros(n, h, w, dtype=dt)
        for sub, (ch, cw) in ((s444, (9, 17)), (s420, (5, 9)), (s422, (9, 9))):
            cb, cr, pairs = torch.zeros(n, ch, cw, dtype=dt), torch.zeros(n, ch, cw, dtype=dt), torch.zeros(n, ch, cw, 2, dtype=dt)
            assert lay(y, cb, cr, sub, "cbcr") == (n, h, w, 2 * w, 2 * cw, jpegamd.CHROMA_PLANES)      # strides in BYTES
            assert lay(y, pairs, None, sub, "cbcr") == (n, h, w, 2 * w, 4 * cw, jpegamd.CHROMA_CBCR)
            assert lay(y, pairs, None, sub, "crcb") == (n, h, w, 2 * w, 4 * cw, jpegamd.CHROMA_CRCB)
    # strided rows and pictures
    big = torch.zeros(5, h, w + 5, dtype=torch.int16)
    cbig = torch.zeros(5, 5, 9 + 3, 2, dtype=torch.int16)
    assert lay(big[::2, :, :w], cbig[::2, :, :9], None, s420, "cbcr") == (3, h, w, 2 * (w + 5), 4 * (9 + 3), jpegamd.CHROMA_CBCR)
    planes = torch.zeros(2, 2, 5, 9 + 1, dtype=torch.int16)
    assert lay(big[:2, :, :w], planes[:, 0, :, :9], planes[:, 1, :, :9], s420, "cbcr")[3:5] == (2 * (w + 5), 2 * (9 + 1))
    # a single row: the stride is the row
    assert lay(torch.zeros(1, 1, 3, dtype=torch.int16), torch.zeros(1, 1, 2, 2, dtype=torch.int16), None, s420, "cbcr")[3:5] == (6, 8)
    y = torch.zeros(n, h, w, dtype=torch.int16)
    cb = torch.zeros(n, 5, 9, dtype=torch.int16)
    pairs = torch.zeros(n, 5, 9, 2, dtype=torch.int16)
    bad = [
        (dict(y=y.to(torch.uint8)), "int16 or uint16"),
        (dict(y=y.to(torch.int32)), "int16 or uint16"),
        (dict(cb=cb.to(torch.uint8)), "int16 or uint16"),
        (dict(cr=cb.to(torch.float16)), "int16 or uint16"),
        (dict(y=y.numpy()), "int16 or uint16"),
        (dict(y=y[0]), r"\[N, H, W\]"),
        (dict(cb=cb[:, :4]), "must be"),
        (dict(cb=pairs, cr=None, sub=s444), "pairs of words"),
        (dict(cb=cb, cr=None), "pairs of words"),
        (dict(cb=torch.zeros(n, 5, 9, 4, dtype=torch.int16)[..., ::2], cr=None), "packed"),
        (dict(cb=torch.zeros(n, 5, 18, dtype=torch.int16)[..., ::2]), "packed"),
        (dict(y=torch.zeros(n, h, 2 * w, dtype=torch.int16)[..., ::2]), "packed"),
        (dict(cr=torch.zeros(n, 5, 11, dtype=torch.int16)[..., :9]), "one row stride"),
        (dict(y=y[:, :1].expand(n, h, w)), "overlap"),
        (dict(order="crcb"), "crcb"),
        (dict(order="uv"), "order"),
        (dict(sub=3), "subsampling"),
    ]
    for kw, match in bad:
        a = dict(y=y, cb=cb, cr=cb.clone(), sub=s420, order="cbcr")
        a.update(kw)
        with pytest.raises(ValueError, match=match):
            lay(a["y"], a["cb"], a["cr"], a["sub"], a["order"])
    # the public entry: its own two arguments, then the device
    for bad_align in ("MSB", "", None, 6, b"msb"):
        with pytest.raises(ValueError, match="align"):
            jpegamd.encode_ycbcr16_batch(y, pairs, align=bad_align)
    with pytest.raises(ValueError, match="sample_range"):
        jpegamd.encode_ycbcr16_batch(y, pairs, sample_range="video")
    for align in ("msb", "lsb"):
        with pytest.raises(ValueError, match="device tensors"):
            jpegamd.encode_ycbcr16_batch(y, pairs, align=align, sample_range="limited")
    # encode_ycbcr_batch is unchanged: it still refuses 16-bit tensors
    with pytest.raises(ValueError, match="uint8"):
        jpegamd.encode_ycbcr_batch(y, pairs)
