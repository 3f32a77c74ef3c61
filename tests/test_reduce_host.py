"""Reduced pictures on the CPU: the numpy restatement of the map (tests/reduce_model.py) against an independent float64 evaluation; the
reciprocal the kernel divides with, exhaustively; jpegamd_reduced_size; the header, the exported symbols and their prototypes; the
argument checks of the reduced entries, which return before the context is touched; and the layout function of the Python functions on
host tensors of bytes.  Nothing here needs a device."""
from __future__ import annotations

import ctypes as C
import re

import numpy as np
import pytest

import reduce_model as rm

torch = pytest.importorskip("torch")

ERR_ARG = -1
CAP = 1 << 20
NAMES = ("jpegamd_encode_reduced_batch_async", "jpegamd_encode_reduced_interleaved_batch_async",
         "jpegamd_encode_reduced_progressive_script_batch_async")
DEBUG_NAMES = ("jpegamd_debug_reduced_planes", "jpegamd_debug_reduce_reciprocal")
FACTORS = range(1, rm.MAX_REDUCE + 1)


# ---- the map ------------------------------------------------------------------------------------------------------------------------
def float64_reduce(a: np.ndarray, f: int) -> np.ndarray:
    """floor(mean + 0.5) over the samples present, box by box in float64: exact at these magnitudes (sums below 2^14, n <= 64, and a
    tie is a multiple of 1 / 2)."""
    h, w = a.shape
    ow, oh = -(-w // f), -(-h // f)
    out = np.zeros((oh, ow), np.uint8)
    for y in range(oh):
        for x in range(ow):
            box = a[f * y:min(f * y + f, h), f * x:min(f * x + f, w)].astype(np.float64)
            out[y, x] = int(np.floor(box.sum() / box.size + 0.5))
    return out


@pytest.mark.parametrize("f", FACTORS)
def test_model_matches_float64(f):
    rng = np.random.default_rng(f)
    for rw in range(f):
        for rh in range(f):
            w, h = f * 2 + rw, f * 3 + rh
            for a in (rng.integers(0, 256, (h, w), np.uint8), np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)):
                got = rm.reduce_plane(a, f)
                assert got.shape == (rm.reduced_size(w, h, f)[1], rm.reduced_size(w, h, f)[0])
                assert np.array_equal(got, float64_reduce(a, f)), (f, w, h)
            assert rm.reduce_plane(np.full((h, w), 255, np.uint8), f).min() == 255
    if f == 1:
        a = rng.integers(0, 256, (5, 7), np.uint8)
        assert np.array_equal(rm.reduce_plane(a, 1), a)              # the identity map


@pytest.mark.parametrize("f", [2, 4, 6, 8, 3])
def test_ties_round_up(f):
    """Boxes whose sum sits exactly on a tie (S = k n + n / 2, n even): the mean goes up to k + 1."""
    rng = np.random.default_rng(40 + f)
    planted = 0
    for w, h in ((2 * f, 2 * f), (2 * f + 1, 2 * f + 2), (3 * f - 1, f + 2)):
        a = rng.integers(0, 256, (h, w), np.uint8)
        counts = rm.box_counts(w, h, f)
        want = rm.reduce_plane(a, f).astype(int)
        for (by, bx), n in np.ndenumerate(counts):
            if n % 2:
                continue
            k = int(rng.integers(0, 255))
            box = a[f * by:f * by + f, f * bx:f * bx + f]            # a view: clipped at the picture's edge
            flat = np.full(n, k, np.uint8)
            flat[:n // 2] = k + 1                                    # S = k n + n / 2
            box[...] = rng.permutation(flat).reshape(box.shape)
            want[by, bx] = k + 1
            planted += 1
        assert np.array_equal(rm.reduce_plane(a, f), want) and np.array_equal(float64_reduce(a, f), want)
    assert planted > 0


def test_reciprocal_is_exact(jpegamd):
    """((S + (n >> 1)) * M[n]) >> s == (S + (n >> 1)) // n for every n and every S a box can have, with the library's own constants;
    the product fits 32 bits."""
    for n in range(1, rm.MAX_REDUCE ** 2 + 1):
        m, s = C.c_uint32(0), C.c_int32(0)
        assert jpegamd.lib.jpegamd_debug_reduce_reciprocal(n, C.byref(m), C.byref(s)) == 0
        assert (m.value, s.value) == (rm.reciprocal(n), rm.SHIFT), n
        x = np.arange(0, 255 * n + 1, dtype=np.uint64) + np.uint64(n >> 1)
        prod = x * np.uint64(m.value)
        assert int(prod.max()) < 1 << 32
        assert np.array_equal(prod >> np.uint64(s.value), x // np.uint64(n)), n
    m, s = C.c_uint32(0), C.c_int32(0)
    for bad in (0, -1, 65):
        assert jpegamd.lib.jpegamd_debug_reduce_reciprocal(bad, C.byref(m), C.byref(s)) == ERR_ARG


# ---- the C surface ------------------------------------------------------------------------------------------------------------------
def test_reduced_size(jpegamd):
    ow, oh = C.c_int32(-7), C.c_int32(-7)
    for f in FACTORS:
        for w, h in ((1, 1), (f, f), (f + 1, 2 * f - 1), (65535, 1), (1, 65535), (65535, 65535), (4096, 2160), (333, 250)):
            assert jpegamd.lib.jpegamd_reduced_size(w, h, f, C.byref(ow), C.byref(oh)) == 0
            assert (ow.value, oh.value) == (-(-w // f), -(-h // f)) == rm.reduced_size(w, h, f) == jpegamd.reduced_size(w, h, f)
    for w, h, f in ((0, 1, 1), (1, 0, 1), (-1, 5, 2), (65536, 1, 1), (1, 65536, 8), (8, 8, 0), (8, 8, 9), (8, 8, -2)):
        assert jpegamd.lib.jpegamd_reduced_size(w, h, f, C.byref(ow), C.byref(oh)) == ERR_ARG
        with pytest.raises(ValueError, match="reduced_size"):
            jpegamd.reduced_size(w, h, f)
    assert jpegamd.lib.jpegamd_reduced_size(8, 8, 2, None, C.byref(oh)) == ERR_ARG
    assert jpegamd.lib.jpegamd_reduced_size(8, 8, 2, C.byref(ow), None) == ERR_ARG


def test_symbols_constants_and_prototypes(jpegamd):
    header = jpegamd.HEADER_PATH.read_text()
    raw = C.CDLL(str(jpegamd.LIB_PATH))
    for name in NAMES + ("jpegamd_reduced_size",):
        assert name in jpegamd.EXPORTED and hasattr(raw, name), name
        assert re.search(rf"int32_t\s+{name}\s*\(", header), name
    assert re.search(r"#define\s+JPEGAMD_MAX_REDUCE\s+8\b", header) and jpegamd.MAX_REDUCE == 8 == rm.MAX_REDUCE
    struct = re.search(r"typedef struct JpegAmdStridedImage \{(.*?)\} JpegAmdStridedImage;", header, re.S).group(1)
    for field in ("plane[3]", "width, height", "row_stride", "pixel_stride", "quality"):
        assert field in struct, field
    assert [f[0] for f in jpegamd.StridedImage._fields_] == ["plane", "width", "height", "row_stride", "pixel_stride", "quality"]
    assert C.sizeof(jpegamd.StridedImage) == 3 * 8 + 5 * 4 + 4
    # the header states the map and what it leaves out
    for text in ("(S + (n >> 1)) / n", "nothing is replicated", "identity map", "linear light is out of scope", "top-down only"):
        assert text in header, text

    def params(name):
        proto = re.search(rf"int32_t\s+{name}\s*\((.*?)\)\s*;", header, re.S).group(1)
        return [re.sub(r".*[\s*]", "", p.strip()) for p in proto.split(",")]

    front = ["enc", "imgs", "count", "subsampling", "factor"]
    back = ["outs_dev", "out_capacity", "out_sizes_dev", "stream"]
    assert params(NAMES[0]) == front + back
    assert params(NAMES[1]) == front + ["restart_interval"] + back
    assert params(NAMES[2]) == front + ["scans", "scan_count"] + back
    assert params("jpegamd_reduced_size") == ["width", "height", "factor", "out_width", "out_height"]
    for name in NAMES:
        assert len(getattr(jpegamd.lib, name).argtypes) == len(params(name))
    # the debug exports are in the library and nowhere public
    for name in DEBUG_NAMES:
        assert hasattr(raw, name) and name not in header and name not in jpegamd.EXPORTED, name
    assert len(jpegamd.lib.jpegamd_debug_reduced_planes.argtypes) == 9
    for method in ("encode_reduced_batch_async", "encode_reduced_interleaved_batch_async", "encode_reduced_progressive_script_batch_async",
                   "strided_image"):
        assert hasattr(jpegamd.Encoder, method), method


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


def _calls(jpegamd, ctx, imgs, count, sub, factor=2, outs=True, sizes=True, null_at=None):
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
    res = [lib.jpegamd_encode_reduced_batch_async(ctx, arr, count, sub, factor, out_arr, CAP, size_arr, None),
           lib.jpegamd_encode_reduced_interleaved_batch_async(ctx, arr, count, sub, factor, 0, out_arr, CAP, size_arr, None),
           lib.jpegamd_encode_reduced_progressive_script_batch_async(ctx, arr, count, sub, factor, None, 0, out_arr, CAP, size_arr, None)]
    if outs and sizes and null_at is None:
        res.append(lib.jpegamd_debug_reduced_planes(ctx, arr, count, sub, factor, buf, buf, buf, None))
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
    for factor in (0, -1, 9, 16, 1 << 20):
        refused(good[:2], 2, s420, factor=factor)
    for sub in (3, -1, 5, 8):                                      # an unknown subsampling
        refused(good[:2], 2, sub)
    refused([_img(j, ptrs=[0, 0x20000, 0x30000])], 1, s444)        # no plane[0]
    refused([_img(j, ptrs=[0x10000, 0x20000, 0])], 1, s444)        # exactly one of plane[1] / plane[2]
    refused([_img(j, ptrs=[0x10000, 0, 0x30000])], 1, s444)
    for sub in (s444, s420, s422):                                 # one channel is a grayscale file alone
        refused(single, 2, sub)
    refused([good[0], single[1]], 2, 0)                            # one channel and three in one call
    for f in (1, 2, 3, 8):
        refused([_img(j, ps=0)], 1, s444, factor=f)                # a pixel stride below 1
        refused([_img(j, ps=-1)], 1, s444, factor=f)
        refused([_img(j, rs=W - 1)], 1, s444, factor=f)            # a row stride below a row
        refused([_img(j, ps=3, rs=3 * W - 1)], 1, s444, factor=f)
        refused([_img(j, rs=-W)], 1, s444, factor=f)
        refused([_img(j, ps=1 << 30, rs=(1 << 31) - 1, w=65535)], 1, s444, factor=f)       # the product is taken in 64 bits
    for kw in (dict(w=0), dict(h=0), dict(w=65536), dict(h=65536), dict(w=-1)):
        refused([_img(j, **kw)], 1, s444)
    for kw in (dict(w=W + 1), dict(h=H + 1), dict(rs=4 * W), dict(ps=2, rs=2 * W), dict(q=90)):        # pictures of different geometry
        refused([good[0], _img(j, 1, **kw)], 2, s444)
    # the one-scan entry checks its interval, the progressive entry its script, the plane export its buffers
    arr = (j.StridedImage * 2)(*good[:2])
    outs = (C.c_void_p * 2)(C.c_void_p(0x1000), C.c_void_p(0x1000))
    for ri in (-1, 65536):
        assert j.lib.jpegamd_encode_reduced_interleaved_batch_async(ctx, arr, 2, s420, 2, ri, outs, CAP, outs, None) == ERR_ARG
    bad_script = (j.Scan * 1)(j.Scan(7, 1, 63, 0, 0))
    assert j.lib.jpegamd_encode_reduced_progressive_script_batch_async(ctx, arr, 2, s420, 2, bad_script, 1, outs, CAP, outs, None) == ERR_ARG
    gray_script = (j.Scan * 2)(j.Scan(1, 0, 0, 0, 0), j.Scan(1, 1, 63, 0, 0))
    assert j.lib.jpegamd_encode_reduced_progressive_script_batch_async(ctx, arr, 2, s420, 2, gray_script, 2, outs, CAP, outs, None) == ERR_ARG
    buf = C.c_void_p(0x3000)
    assert j.lib.jpegamd_debug_reduced_planes(ctx, arr, 2, s420, 2, None, buf, buf, None) == ERR_ARG
    assert j.lib.jpegamd_debug_reduced_planes(ctx, arr, 2, s420, 2, buf, None, buf, None) == ERR_ARG
    assert not any(keep)


# ---- Python -------------------------------------------------------------------------------------------------------------------------
def _layout(jpegamd, t, layout, single=False):
    n, h, w, row, pixel, sample_type, channels, ptr, planes = jpegamd._float_layout(t, layout, single, byte=True)
    assert sample_type == 0
    return (n, h, w, row, pixel, channels), ptr, planes


def test_layouts_of_host_tensors(jpegamd):
    n, h, w = 3, 6, 10
    chw = torch.zeros(n, 3, h, w, dtype=torch.uint8)
    info, ptr, planes = _layout(jpegamd, chw, "chw")
    assert info == (n, h, w, w, 1, 3)
    assert ptr(1) == tuple(chw[1, k].data_ptr() for k in range(3))
    assert all(p.data_ptr() == chw[:, k].data_ptr() for k, p in enumerate(planes))          # views: nothing was copied
    hwc = torch.zeros(n, h, w, 3, dtype=torch.uint8)
    info, ptr, _ = _layout(jpegamd, hwc, "hwc")
    assert info == (n, h, w, 3 * w, 3, 3)
    assert ptr(2) == tuple(hwc[2].data_ptr() + k for k in range(3))
    for name, order in (("rgba", (0, 1, 2)), ("bgra", (2, 1, 0))):
        px4 = torch.zeros(n, h, w, 4, dtype=torch.uint8)
        info, ptr, _ = _layout(jpegamd, px4, name)
        assert info == (n, h, w, 4 * w, 4, 3)
        assert ptr(0) == tuple(px4.data_ptr() + k for k in order)
    gray = torch.zeros(n, h, w, dtype=torch.uint8)
    info, ptr, _ = _layout(jpegamd, gray, "gray")
    assert info == (n, h, w, w, 1, 1) and ptr(1) == (gray[1].data_ptr(),)
    three = [torch.zeros(n, h, w, dtype=torch.uint8) for _ in range(3)]
    info, ptr, _ = _layout(jpegamd, three, "chw")
    assert info == (n, h, w, w, 1, 3) and ptr(1) == tuple(p[1].data_ptr() for p in three)
    # channels_last: the memory of [N, H, W, 3] under the shape [N, 3, H, W]
    cl = chw.contiguous(memory_format=torch.channels_last)
    info, ptr, _ = _layout(jpegamd, cl, "chw")
    assert info == (n, h, w, 3 * w, 3, 3)
    assert ptr(1) == tuple(cl[1].data_ptr() + k for k in range(3))
    assert (cl.stride(3), cl.stride(2)) == (3, 3 * w)
    # a crop, every second picture, every second row, every second column
    crop = chw[:, :, 1:5, 2:9]
    info, ptr, _ = _layout(jpegamd, crop, "chw")
    assert info == (n, 4, 7, w, 1, 3) and ptr(0)[0] == chw.data_ptr() + (w + 2) and crop.stride(2) == w
    info, ptr, _ = _layout(jpegamd, chw[::2], "chw")
    assert info[0] == 2 and ptr(1)[0] == chw[2].data_ptr()
    info, _, _ = _layout(jpegamd, chw[:, :, ::2], "chw")
    assert info == (n, 3, w, 2 * w, 1, 3)
    info, _, _ = _layout(jpegamd, chw[:, :, :, ::2], "chw")
    assert info == (n, h, 5, w, 2, 3)
    # one picture
    info, ptr, _ = _layout(jpegamd, chw[0], "chw", single=True)
    assert info == (1, h, w, w, 1, 3) and ptr(0) == tuple(chw[0, k].data_ptr() for k in range(3))
    info, _, _ = _layout(jpegamd, gray[0], "gray", single=True)
    assert info == (1, h, w, w, 1, 1)


def test_layout_value_errors(jpegamd):
    b = torch.zeros(2, 3, 6, 10, dtype=torch.uint8)
    z = lambda *shape: torch.zeros(*shape, dtype=torch.uint8)
    cases = [
        (b, "nchw", "layout must be"), (b, None, "layout must be"), (b.float(), "chw", "uint8 tensors"), (b.to(torch.int8), "chw", "uint8 tensors"),
        (b.numpy(), "chw", "uint8 tensors"), ([b[:, 0], b[:, 1]], "chw", "three of them"),
        ([b[:, 0], b[:, 1], b[:, 2].float()], "chw", "uint8 tensors"), ([b[:, 0], b[:, 1], b[:, 2, :5]], "chw", "one shape"),
        (b[0], "chw", r"\[N, 3, H, W\]"), (b[:, :2], "chw", r"\[N, 3, H, W\]"), (z(2, 6, 10, 4), "hwc", r"\[N, H, W, 3\]"),
        (z(2, 6, 10, 3), "rgba", r"\[N, H, W, 4\]"), (b, "gray", r"\[N, H, W\]"), (z(0, 3, 6, 10), "chw", "at least one picture"),
        (z(1, 3, 2, 65536), "chw", "1..65535"), (b[:, :, :, :1].expand(2, 3, 6, 10), "chw", "positive stride"),
        (b[:, :, :1].expand(2, 3, 6, 10), "chw", "rows overlap"), (b.transpose(2, 3), "chw", "rows overlap"),
        ([b[:, 0], b[:, 1], z(2, 6, 20)[:, :, ::2]], "chw", "one pixel stride"),
        ([b[:, 0], b[:, 1], z(2, 6, 12)[:, :, :10]], "chw", "one row stride"),
    ]
    for t, layout, match in cases:
        with pytest.raises(ValueError, match=match):
            jpegamd._float_layout(t, layout, False, byte=True)
    with pytest.raises(ValueError, match=r"\[3, H, W\]"):
        jpegamd._float_layout(b, "chw", True, byte=True)
    # the float functions keep refusing bytes
    with pytest.raises(ValueError, match="float32, float16 or bfloat16"):
        jpegamd._float_layout(b, "chw", False)


def test_python_checks_run_before_the_device(jpegamd):
    import jpegamd.mjpeg as mj
    import jpegamd.progressive_script as ps
    b = torch.zeros(2, 3, 8, 8, dtype=torch.uint8)
    for fn in (jpegamd.encode_reduced_batch, mj.encode_reduced_batch, ps.encode_reduced_batch):
        with pytest.raises(ValueError, match="device tensors"):
            fn(b)
        for factor in (0, 9, 2.0, None, True):
            with pytest.raises(ValueError, match="factor"):
                fn(b, factor=factor)
        with pytest.raises(ValueError, match="subsampling"):
            fn(b, subsampling=3)
        with pytest.raises(ValueError, match="layout"):
            fn(b, layout="nchw")
        with pytest.raises(ValueError, match="uint8 tensors"):
            fn(b.float())
    with pytest.raises(ValueError, match="device tensors"):
        jpegamd.encode_reduced(b[0])
    with pytest.raises(ValueError, match="device tensors"):
        jpegamd.encode_reduced_batch(b[:, 0], layout="gray", subsampling=jpegamd.SUBSAMPLE_444)     # (one channel: whatever the subsampling)
    with pytest.raises(ValueError, match="huffman"):
        mj.encode_reduced_batch(b, huffman="best")
    with pytest.raises(ValueError, match="restart_interval"):
        mj.encode_reduced_batch(b, restart_interval=-1)
    with pytest.raises(ValueError, match="scan"):
        ps.encode_reduced_batch(b, scans=[((0, 1, 2), 1, 63, 0, 0)])
