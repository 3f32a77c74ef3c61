"""Resized pictures on the CPU: the numpy restatement of the map (tests/resize_model.py) against an independent evaluation in
fractions.Fraction, against the reduced map at whole factors and against plain box means; the division the kernel runs, through the
library's own host restatement; jpegamd_resize_check; the header, the exported symbols and their prototypes; the argument checks of the
resized entries, which return before the context is touched; the layout function, fit_size and the ValueErrors of the Python functions.
Nothing here needs a device."""
from __future__ import annotations

import ctypes as C
import math
import re
import time
from fractions import Fraction

import numpy as np
import pytest

import reduce_model as rdm
import resize_model as rz

torch = pytest.importorskip("torch")

ERR_ARG = -1
CAP = 1 << 20
NAMES = ("jpegamd_encode_resized_batch_async", "jpegamd_encode_resized_interleaved_batch_async",
         "jpegamd_encode_resized_progressive_script_batch_async")
DEBUG_NAMES = ("jpegamd_debug_resized_planes", "jpegamd_debug_resize_divide")
# (W, H, ow, oh): D odd and even, ratios just under 1, one axis the identity, a height of 1
FRACTION_SIZES = ((13, 9, 5, 4), (33, 31, 32, 30), (17, 5, 3, 5), (100, 3, 7, 1), (7, 7, 2, 3))


# ---- the map ------------------------------------------------------------------------------------------------------------------------
def fraction_resize(a: np.ndarray, ow: int, oh: int) -> np.ndarray:
    """floor(mean + 1/2), the mean of the source over the footprint [X W / ow, (X + 1) W / ow) x [Y H / oh, (Y + 1) H / oh) with every
    sample weighted by the length of its unit interval inside, in exact rationals."""
    h, w = a.shape

    def shares(n, on, big):
        lo, hi = Fraction(big * n, on), Fraction((big + 1) * n, on)
        return [(x, min(hi, Fraction(x + 1)) - max(lo, Fraction(x))) for x in range(math.floor(lo), math.ceil(hi))]

    out = np.zeros((oh, ow), np.uint8)
    for big_y in range(oh):
        for big_x in range(ow):
            total = sum(sy * sx * int(a[y, x]) for y, sy in shares(h, oh, big_y) for x, sx in shares(w, ow, big_x))
            mean = total / (Fraction(w, ow) * Fraction(h, oh))
            out[big_y, big_x] = math.floor(mean + Fraction(1, 2))
    return out


@pytest.mark.parametrize("w,h,ow,oh", FRACTION_SIZES)
def test_model_matches_fractions(w, h, ow, oh):
    rng = np.random.default_rng(w * 1000 + h)
    for a in (rng.integers(0, 256, (h, w), np.uint8), rng.integers(0, 2, (h, w), np.uint8) * 255, rng.integers(126, 130, (h, w), np.uint8)):
        got = rz.resize_plane(a, ow, oh)
        assert got.shape == (oh, ow)
        assert np.array_equal(got, fraction_resize(a, ow, oh)), (w, h, ow, oh)


def test_weights_sum_to_the_source_and_taps_are_few():
    for n, on in ((13, 5), (33, 32), (17, 3), (100, 7), (7, 2), (5, 5), (128, 2), (4100, 65), (65535, 1024), (1, 1)):
        idx, wgt = rz.taps(n, on)
        assert idx.shape == wgt.shape == (on, -(-n // on) + 1)
        assert np.all(wgt.sum(axis=1) == n) and wgt.min() >= 0 and wgt.max() <= on
        assert idx.min() == 0 and idx.max() == n - 1
        # every source sample is given out exactly once: its weights over the targets add up to `on`
        per_sample = np.zeros(n, np.int64)
        np.add.at(per_sample, idx.ravel(), wgt.ravel())
        assert np.all(per_sample == on), (n, on)


@pytest.mark.parametrize("f", range(1, rdm.MAX_REDUCE + 1))
def test_model_is_the_reduced_map_on_exact_multiples(f):
    rng = np.random.default_rng(70 + f)
    for ow, oh in ((5, 3), (1, 1), (9, 2)):
        a = rng.integers(0, 256, (f * oh, f * ow), np.uint8)
        assert np.array_equal(rz.resize_plane(a, ow, oh), rdm.reduce_plane(a, f)), (f, ow, oh)


def test_anamorphic_whole_ratio_is_the_box_mean():
    rng = np.random.default_rng(3512)
    a = rng.integers(0, 256, (12, 35), np.uint8)                   # 35 x 12 -> 5 x 4: boxes of 7 x 3
    s = a.astype(np.int64).reshape(4, 3, 5, 7).sum(axis=(1, 3))
    assert np.array_equal(rz.resize_plane(a, 5, 4), ((s + 10) // 21).astype(np.uint8))
    assert np.array_equal(rz.resize_plane(a, 5, 4), fraction_resize(a, 5, 4))


def test_identity_and_flat_pictures():
    rng = np.random.default_rng(9)
    for w, h in ((23, 17), (1, 1), (64, 3)):
        a = rng.integers(0, 256, (h, w), np.uint8)
        assert np.array_equal(rz.resize_plane(a, w, h), a)
    for w, h, ow, oh in FRACTION_SIZES + ((128, 64, 2, 1), (130, 67, 3, 2)):
        for value in (0, 255, 1, 254):
            assert np.all(rz.resize_plane(np.full((h, w), value, np.uint8), ow, oh) == value), (w, h, ow, oh, value)
    pic = rng.integers(0, 256, (9, 13, 3), np.uint8)
    small = rz.resize_picture(pic, 5, 4)
    assert small.shape == (4, 5, 3) and all(np.array_equal(small[:, :, c], rz.resize_plane(pic[:, :, c], 5, 4)) for c in range(3))


def test_planted_ties_round_up():
    """D even: S = k D + D / 2 is a mean of exactly k + 1/2 and goes up.  D odd: no mean is a tie, and the two sums on either side of
    k + 1/2 part at D >> 1."""
    for k in (0, 7, 128, 253):
        # 4 x 4 -> 2 x 2: D = 16, every weight 4; a box that sums to 4 k + 2
        a = np.full((4, 4), k, np.uint8)
        a[0, 0] = a[1, 1] = k + 1
        want = np.full((2, 2), k, np.uint8)
        want[0, 0] = k + 1
        assert np.array_equal(rz.resize_plane(a, 2, 2), want) and np.array_equal(fraction_resize(a, 2, 2), want)
        # 3 x 2 -> 2 x 1, a ratio of 3 / 2: D = 6, wx = (2, 1, 0) and (0, 1, 2), wy = (1, 1); both sums are
        # 2 (k + k) + (k + 1) + (k + 2) = 6 k + 3: up
        a = np.array([[k, k + 1, k], [k, k + 2, k]], np.uint8)
        want = np.array([[k + 1, k + 1]], np.uint8)
        assert np.array_equal(rz.resize_plane(a, 2, 1), want) and np.array_equal(fraction_resize(a, 2, 1), want)
        if k:
            a[0, 2] = k - 1                                        # S(1) = 6 k + 1: below the tie
            want[0, 1] = k
            assert np.array_equal(rz.resize_plane(a, 2, 1), want) and np.array_equal(fraction_resize(a, 2, 1), want)
        # 3 x 3 -> 1 x 1: D = 9, every weight 1; S = 9 k + 4 stays at k, 9 k + 5 goes to k + 1
        for extra, up in ((4, 0), (5, 1)):
            a = np.full(9, k, np.uint8)
            a[:extra] = k + 1
            a = a.reshape(3, 3)
            assert rz.resize_plane(a, 1, 1)[0, 0] == k + up == fraction_resize(a, 1, 1)[0, 0]


def test_the_large_case_is_quick():
    a = np.full((4100, 4100), 254, np.uint8)
    t0 = time.perf_counter()
    out = rz.resize_plane(a, 65, 65)
    assert time.perf_counter() - t0 < 1.0                          # (well under a second, as the large GPU case needs)
    assert out.shape == (65, 65) and np.all(out == 254)
    # 254 * 4100^2 is 0.6% short of 2^32; 4200^2 is past it, and the model's int64 holds both
    assert 254 * 4100 * 4100 < 1 << 32 < 254 * 4200 * 4200
    assert np.all(rz.resize_plane(np.full((4200, 4200), 254, np.uint8), 66, 66) == 254)


# ---- the division ---------------------------------------------------------------------------------------------------------------------
DIVISORS = (1, 2, 3, 117, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, 65535 ** 2, 65535 * 65521)


@pytest.mark.parametrize("d", DIVISORS)
def test_the_kernels_division_is_exact(jpegamd, d):
    """(s + (d >> 1)) // d by the text the kernel runs, at the sums around every quotient's two edges."""
    q = C.c_uint32(0xFFFFFFFF)
    div = jpegamd.lib.jpegamd_debug_resize_divide
    seen = set()
    for k in range(256):
        for s in (k * d - 1, k * d, k * d + (d >> 1) - 1, k * d + (d >> 1)):
            if s < 0:
                continue
            assert div(d, s, C.byref(q)) == 0, (d, s)
            assert q.value == (s + (d >> 1)) // d, (d, s, q.value)
            seen.add(q.value)
    assert set(range(256)) <= seen
    assert div(0, 0, C.byref(q)) == ERR_ARG and div(d, 0, None) == ERR_ARG
    assert div(d, 255 * d + (d >> 1) + 1, C.byref(q)) == ERR_ARG   # no sum of bytes is that large


# ---- the C surface ------------------------------------------------------------------------------------------------------------------
def test_resize_check(jpegamd):
    chk = jpegamd.lib.jpegamd_resize_check
    good = [(1, 1, 1, 1), (13, 9, 5, 4), (13, 9, 13, 9), (65535, 65535, 65535, 65535), (65535, 65535, 1024, 1024), (8192, 8192, 160, 128),
            (64, 64, 1, 1), (128, 64, 2, 1), (640, 7, 10, 7), (7, 640, 7, 10), (65535, 2, 1024, 1)]
    bad = [(13, 9, 14, 9), (13, 9, 13, 10), (13, 9, 0, 4), (13, 9, 5, 0), (13, 9, -1, 4), (13, 9, 5, -3),       # enlargement; nothing
           (65, 64, 1, 1), (64, 65, 1, 1), (129, 64, 2, 1), (128, 129, 2, 2),                                    # 64 ow + 1
           (0, 9, 1, 1), (13, 0, 1, 1), (65536, 9, 1024, 9), (13, 65536, 13, 1024), (-5, 9, 1, 1), (65536, 65536, 65536, 65536)]
    for args in good:
        assert chk(*args) == 0 and rz.check(*args), args
        jpegamd.resize_check(*args)
    for args in bad:
        assert chk(*args) == ERR_ARG and not rz.check(*args), args
        with pytest.raises(ValueError, match="resized picture"):
            jpegamd.resize_check(*args)
    for ow in (1, 3, 1023):                                        # the ratio's bound, each way
        assert chk(64 * ow, 5, ow, 5) == 0 and chk(5, 64 * ow, 5, ow) == 0
        if 64 * ow + 1 <= 65535:
            assert chk(64 * ow + 1, 5, ow, 5) == ERR_ARG and chk(5, 64 * ow + 1, 5, ow) == ERR_ARG
    with pytest.raises(ValueError, match="resized picture"):
        jpegamd.resize_check(8, 8, 4.0, 4)


def test_symbols_constants_and_prototypes(jpegamd):
    header = jpegamd.HEADER_PATH.read_text()
    raw = C.CDLL(str(jpegamd.LIB_PATH))
    for name in NAMES + ("jpegamd_resize_check",):
        assert name in jpegamd.EXPORTED and name in jpegamd._BASE and hasattr(raw, name), name
        assert re.search(rf"int32_t\s+{name}\s*\(", header), name
    assert re.search(r"#define\s+JPEGAMD_MAX_RESIZE_RATIO\s+64\b", header) and jpegamd.MAX_RESIZE_RATIO == 64 == rz.MAX_RESIZE_RATIO
    # the header states the map and what it leaves out
    for text in ("Resized pictures", "wx(X, x) = max(0, min((X + 1) W, (x + 1) ow) - max(X W, x ow))",
                 "wy(Y, y) = max(0, min((Y + 1) H, (y + 1) oh) - max(Y H, y oh))", "v(X, Y)  = (S + (D >> 1)) / D", "no enlargement",
                 "floor(mean + 1/2)", "is the identity", "ceil(W / ow) + 1"):
        assert text in header, text

    def params(name):
        proto = re.search(rf"int32_t\s+{name}\s*\((.*?)\)\s*;", header, re.S).group(1)
        return [re.sub(r".*[\s*]", "", p.strip()) for p in proto.split(",")]

    front = ["enc", "imgs", "count", "subsampling", "out_width", "out_height"]
    back = ["outs_dev", "out_capacity", "out_sizes_dev", "stream"]
    assert params(NAMES[0]) == front + back
    assert params(NAMES[1]) == front + ["restart_interval"] + back
    assert params(NAMES[2]) == front + ["scans", "scan_count"] + back
    assert params("jpegamd_resize_check") == ["width", "height", "out_width", "out_height"]
    for name in NAMES + ("jpegamd_resize_check",):
        assert len(getattr(jpegamd.lib, name).argtypes) == len(params(name))
    # the debug exports are in the library and nowhere public
    for name in DEBUG_NAMES:
        assert hasattr(raw, name) and name not in header and name not in jpegamd.EXPORTED and name not in jpegamd._HIDDEN, name
    assert len(jpegamd.lib.jpegamd_debug_resized_planes.argtypes) == 10
    for method in ("encode_resized_batch_async", "encode_resized_interleaved_batch_async", "encode_resized_progressive_script_batch_async"):
        assert hasattr(jpegamd.Encoder, method) and method in vars(jpegamd._ResizedEntries) and method not in vars(jpegamd.Encoder), method
    assert issubclass(jpegamd._ResizedEntries, jpegamd._ReducedEntries) and issubclass(jpegamd.Encoder, jpegamd._ResizedEntries)


def _fake_context():
    """A block of zeros where the context would be: a check that came too late would read it."""
    fake = (C.c_uint8 * (1 << 16))()
    return fake, C.cast(fake, C.c_void_p)


W, H = 64, 32


def _img(jpegamd, i=0, planes=3, ps=1, rs=None, q=0, w=W, h=H, ptrs=None):
    base = 0x100000 * (i + 1) + 1                                  # (any alignment is taken)
    rs = 2 * ps * w if rs is None else rs
    ptrs = ptrs if ptrs is not None else [base + 0x10000 * k if k < planes else 0 for k in range(3)]
    return jpegamd.Encoder.strided_image(ptrs, w, h, rs, ps, q)


def _calls(jpegamd, ctx, imgs, count, sub, size=(40, 20), outs=True, sizes=True, null_at=None):
    """The four entries with these arguments -> their results."""
    n = max(len(imgs), 1)
    arr = (jpegamd.StridedImage * n)(*imgs) if imgs else None
    out_list = [C.c_void_p(0x1000)] * 40
    size_list = [C.c_void_p(0x2000)] * 40
    if null_at is not None:
        out_list = list(out_list)
        out_list[null_at] = C.c_void_p(0)
    out_arr = (C.c_void_p * 40)(*out_list) if outs else None
    size_arr = (C.c_void_p * 40)(*size_list) if sizes else None
    lib = jpegamd.lib
    buf = C.c_void_p(0x3000)
    ow, oh = size
    res = [lib.jpegamd_encode_resized_batch_async(ctx, arr, count, sub, ow, oh, out_arr, CAP, size_arr, None),
           lib.jpegamd_encode_resized_interleaved_batch_async(ctx, arr, count, sub, ow, oh, 0, out_arr, CAP, size_arr, None),
           lib.jpegamd_encode_resized_progressive_script_batch_async(ctx, arr, count, sub, ow, oh, None, 0, out_arr, CAP, size_arr, None)]
    if outs and sizes and null_at is None:
        res.append(lib.jpegamd_debug_resized_planes(ctx, arr, count, sub, ow, oh, buf, buf, buf, None))
    return res


def test_argument_checks_come_before_the_context(jpegamd):
    keep, ctx = _fake_context()
    j = jpegamd
    s444, s420, s422 = j.SUBSAMPLE_444, j.SUBSAMPLE_420, j.SUBSAMPLE_422
    good = [_img(j, i) for i in range(40)]
    single = [_img(j, i, planes=1) for i in range(2)]

    def refused(*a, **kw):
        res = _calls(j, ctx, *a, **kw)
        assert all(r == ERR_ARG for r in res), (res, a[1:], kw)

    refused([], 1, s420)                                           # a null array
    assert all(r == ERR_ARG for r in _calls(j, None, good[:2], 2, s420))       # a null context
    refused(good[:2], 2, s420, outs=False)
    refused(good[:2], 2, s420, sizes=False)
    refused(good[:2], 2, s420, null_at=1)                          # a null element
    for count in (0, -1, 33):
        refused(good[:max(count, 1)], count, s420)
    # the size: nothing, an enlargement either way, a ratio above 64 either way
    for size in ((0, 20), (40, 0), (-1, 20), (40, -1), (W + 1, 20), (40, H + 1), (1 << 20, 20)):
        refused(good[:2], 2, s420, size=size)
    refused([_img(j, w=65, h=H)], 1, s444, size=(1, H))
    refused([_img(j, w=W, h=129)], 1, s444, size=(W, 2))
    for sub in (3, -1, 5, 8):                                      # an unknown subsampling
        refused(good[:2], 2, sub)
    refused([_img(j, ptrs=[0, 0x20000, 0x30000])], 1, s444)        # no plane[0]
    refused([_img(j, ptrs=[0x10000, 0x20000, 0])], 1, s444)        # exactly one of plane[1] / plane[2]
    refused([_img(j, ptrs=[0x10000, 0, 0x30000])], 1, s444)
    for sub in (s444, s420, s422):                                 # one channel is a grayscale file alone
        refused(single, 2, sub)
    refused([good[0], single[1]], 2, 0)                            # one channel and three in one call
    for size in ((W, H), (40, 20), (1, 1)):
        refused([_img(j, ps=0)], 1, s444, size=size)               # a pixel stride below 1
        refused([_img(j, ps=-1)], 1, s444, size=size)
        refused([_img(j, rs=W - 1)], 1, s444, size=size)           # a row stride below a row
        refused([_img(j, ps=3, rs=3 * W - 1)], 1, s444, size=size)
        refused([_img(j, rs=-W)], 1, s444, size=size)
    refused([_img(j, ps=1 << 30, rs=(1 << 31) - 1, w=65535)], 1, s444, size=(1024, 20))        # the product is taken in 64 bits
    for kw in (dict(w=0), dict(h=0), dict(w=65536), dict(h=65536), dict(w=-1)):
        refused([_img(j, **kw)], 1, s444, size=(1024, 20) if kw.get("w", 0) > W else (40, 20))
    for kw in (dict(w=W + 1), dict(h=H + 1), dict(rs=4 * W), dict(ps=2, rs=2 * W), dict(q=90)):        # pictures of different geometry
        refused([good[0], _img(j, 1, **kw)], 2, s444)
    # the one-scan entry checks its interval, the progressive entry its script, the plane export its buffers
    arr = (j.StridedImage * 2)(*good[:2])
    outs = (C.c_void_p * 2)(C.c_void_p(0x1000), C.c_void_p(0x1000))
    for ri in (-1, 65536):
        assert j.lib.jpegamd_encode_resized_interleaved_batch_async(ctx, arr, 2, s420, 40, 20, ri, outs, CAP, outs, None) == ERR_ARG
    bad_script = (j.Scan * 1)(j.Scan(7, 1, 63, 0, 0))
    assert j.lib.jpegamd_encode_resized_progressive_script_batch_async(ctx, arr, 2, s420, 40, 20, bad_script, 1, outs, CAP, outs, None) == ERR_ARG
    gray_script = (j.Scan * 2)(j.Scan(1, 0, 0, 0, 0), j.Scan(1, 1, 63, 0, 0))
    assert j.lib.jpegamd_encode_resized_progressive_script_batch_async(ctx, arr, 2, s420, 40, 20, gray_script, 2, outs, CAP, outs, None) == ERR_ARG
    buf = C.c_void_p(0x3000)
    assert j.lib.jpegamd_debug_resized_planes(ctx, arr, 2, s420, 40, 20, None, buf, buf, None) == ERR_ARG
    assert j.lib.jpegamd_debug_resized_planes(ctx, arr, 2, s420, 40, 20, buf, None, buf, None) == ERR_ARG
    assert not any(keep)


# ---- Python -------------------------------------------------------------------------------------------------------------------------
def test_the_layout_function_is_the_reduced_one(jpegamd):
    """Bytes at any stride, described once: what the resized functions queue is what the reduced functions queue."""
    n, h, w = 3, 6, 10
    chw = torch.zeros(n, 3, h, w, dtype=torch.uint8)

    def layout(t, name, single=False):
        n_, h_, w_, row, pixel, sample_type, channels, ptr, _ = jpegamd._float_layout(t, name, single, byte=True)
        assert sample_type == 0
        return (n_, h_, w_, row, pixel, channels), ptr

    info, ptr = layout(chw, "chw")
    assert info == (n, h, w, w, 1, 3) and ptr(1) == tuple(chw[1, k].data_ptr() for k in range(3))
    cl = chw.contiguous(memory_format=torch.channels_last)
    info, ptr = layout(cl, "chw")
    assert info == (n, h, w, 3 * w, 3, 3) and ptr(1) == tuple(cl[1].data_ptr() + k for k in range(3))
    crop = chw[:, :, 1:5, 2:9]
    info, ptr = layout(crop, "chw")
    assert info == (n, 4, 7, w, 1, 3) and ptr(0)[0] == chw.data_ptr() + (w + 2)
    info, ptr = layout(chw[::2], "chw")
    assert info[0] == 2 and ptr(1)[0] == chw[2].data_ptr()
    px4 = torch.zeros(n, h, w, 4, dtype=torch.uint8)
    info, ptr = layout(px4, "bgra")
    assert info == (n, h, w, 4 * w, 4, 3) and ptr(0) == tuple(px4.data_ptr() + k for k in (2, 1, 0))
    info, ptr = layout(torch.zeros(h, w, dtype=torch.uint8), "gray", single=True)
    assert info == (1, h, w, w, 1, 1)
    import inspect
    assert "_float_layout(t, layout, single, byte=True)" in inspect.getsource(jpegamd._encode_resized)


def test_fit_size(jpegamd):
    fit = jpegamd.fit_size
    assert fit(640, 480, 1024, 1024) == (640, 480) and fit(1024, 1024, 1024, 1024) == (1024, 1024)
    assert fit(4096, 2304, 1920, 1080) == (1920, 1080)
    assert fit(4096, 2304, 1024, 1024) == (1024, 576)
    assert fit(2304, 4096, 1024, 1024) == (576, 1024)
    assert fit(4000, 3000, 320, 320) == (320, 240) and fit(3000, 4000, 320, 320) == (240, 320)
    assert fit(1000, 3, 100, 100) == (100, 1) and fit(3, 1000, 100, 100) == (1, 100)         # at least 1
    assert fit(1001, 667, 500, 500) == (500, (667 * 500 + 500) // 1001)                      # rounded half up
    assert fit(100, 50, 30, 1000) == (30, 15) and fit(100, 50, 1000, 10) == (20, 10)
    rng = np.random.default_rng(5)
    for w, h, mw, mh in rng.integers(1, 5000, (200, 4)).tolist():
        got = fit(w, h, mw, mh)
        assert got == rz.fit_size(w, h, mw, mh)
        assert 1 <= got[0] <= max(mw, 1) and 1 <= got[1] <= max(mh, 1) and got[0] <= w and got[1] <= h
        assert all(isinstance(v, int) for v in got)
    for bad in ((0, 5, 5, 5), (5, 5, 0, 5), (5.0, 5, 5, 5), (5, 5, 5, None), (True, 5, 5, 5)):
        with pytest.raises(ValueError, match="fit_size"):
            fit(*bad)


def test_python_checks_run_before_the_device(jpegamd):
    import jpegamd.mjpeg as mj
    import jpegamd.progressive_script as ps
    b = torch.zeros(2, 3, 8, 8, dtype=torch.uint8)
    for fn in (jpegamd.encode_resized_batch, mj.encode_resized_batch, ps.encode_resized_batch):
        with pytest.raises(ValueError, match="device tensors"):
            fn(b, size=(5, 3))
        for size in (None, 5, (5,), (5, 3, 1), (5.0, 3), (True, 3), "53"):
            with pytest.raises(ValueError, match="size must be"):
                fn(b, size=size)
        for size in ((9, 8), (8, 9), (0, 4), (4, 0), (-1, 4)):
            with pytest.raises(ValueError, match="resized picture"):
                fn(b, size=size)
        with pytest.raises(ValueError, match="subsampling"):
            fn(b, subsampling=3, size=(5, 3))
        with pytest.raises(ValueError, match="layout"):
            fn(b, layout="nchw", size=(5, 3))
        with pytest.raises(ValueError, match="uint8 tensors"):
            fn(b.float(), size=(5, 3))
    wide = torch.zeros(1, 3, 2, 130, dtype=torch.uint8)
    with pytest.raises(ValueError, match="resized picture"):
        jpegamd.encode_resized_batch(wide, size=(2, 2))             # a ratio of 65
    with pytest.raises(ValueError, match="device tensors"):
        jpegamd.encode_resized_batch(wide, size=(3, 2))
    with pytest.raises(ValueError, match="device tensors"):
        jpegamd.encode_resized(b[0], size=(8, 8))
    with pytest.raises(ValueError, match="device tensors"):
        jpegamd.encode_resized_batch(b[:, 0], layout="gray", subsampling=jpegamd.SUBSAMPLE_444, size=(3, 3))
    with pytest.raises(ValueError, match="huffman"):
        mj.encode_resized_batch(b, size=(5, 3), huffman="best")
    with pytest.raises(ValueError, match="restart_interval"):
        mj.encode_resized_batch(b, size=(5, 3), restart_interval=-1)
    with pytest.raises(ValueError, match="scan"):
        ps.encode_resized_batch(b, size=(5, 3), scans=[((0, 1, 2), 1, 63, 0, 0)])
