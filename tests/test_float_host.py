"""Float pictures on the CPU: the numpy restatement of the map (tests/float_model.py) against torch over every float16 and bfloat16 bit
pattern and over random and edge float32 patterns; the header, the exported symbols and their prototypes; the argument checks of the float
entries, which return before the context is touched; value_range; and the layout function of the Python functions on host tensors.
Nothing here needs a device."""
from __future__ import annotations

import ctypes as C
import re

import numpy as np
import pytest

import float_model as fm

torch = pytest.importorskip("torch")

ERR_ARG = -1
CAP = 1 << 20
NAMES = ("jpegamd_encode_float_batch_async", "jpegamd_encode_float_interleaved_batch_async",
         "jpegamd_encode_float_progressive_script_batch_async")
DEBUG_NAME = "jpegamd_debug_float_planes"
TORCH_TYPES = {fm.F32: torch.float32, fm.F16: torch.float16, fm.BF16: torch.bfloat16}


def torch_samples(bits: np.ndarray, sample_type: int):
    """The bit patterns as a torch tensor of the sample type."""
    signed = np.ascontiguousarray(bits).view(np.int32 if sample_type == fm.F32 else np.int16)
    return torch.from_numpy(signed.copy()).view(TORCH_TYPES[sample_type])


def torch_bytes(x, scale: float, offset: float) -> np.ndarray:
    """What a caller computes today, with the NaN and infinity cases pinned."""
    t = x.float().mul(scale).add(offset)
    return torch.nan_to_num(t, nan=0.0, posinf=255.0, neginf=0.0).round().clamp(0, 255).to(torch.uint8).numpy()


# ---- the map ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample_type", [fm.F16, fm.BF16])
def test_every_half_width_pattern_matches_torch(sample_type):
    bits = fm.all_half_patterns()
    assert np.unique(bits).size == 65536
    x = torch_samples(bits, sample_type)
    for scale, offset in fm.PAIRS:
        got = fm.bytes_of(bits, sample_type, scale, offset)
        assert np.array_equal(got, torch_bytes(x, scale, offset)), (sample_type, scale, offset)
        assert got.min() == 0 and got.max() == 255


def test_f32_patterns_match_torch():
    rng = np.random.default_rng(20)
    bits = np.concatenate([rng.integers(0, 1 << 32, 200_000, dtype=np.uint64).astype(np.uint32), fm.f32_edge_picture(3).reshape(-1)])
    # patterns near the byte range as well: random bits are mostly huge, tiny or NaN
    near = (rng.random(100_000) * 300.0 - 20.0).astype(np.float32)
    bits = np.concatenate([bits, near.view(np.uint32), (near / np.float32(255)).astype(np.float32).view(np.uint32)])
    assert bits.size >= 200_000
    x = torch_samples(bits, fm.F32)
    for scale, offset in fm.PAIRS:
        assert np.array_equal(fm.bytes_of(bits, fm.F32, scale, offset), torch_bytes(x, scale, offset)), (scale, offset)


def test_named_values_of_the_map():
    def one(value, scale, offset, sample_type=fm.F32):
        if sample_type == fm.F32:
            bits = fm.f32_bits([value])
        else:
            bits = np.array([value], dtype=np.uint16)
        return int(fm.bytes_of(bits, sample_type, scale, offset)[0])

    assert one(0.0, 127.5, 127.5) == 128                           # the tie of (-1, 1) goes to the even byte
    assert [one(k + 0.5, 1, 0) for k in range(4)] == [0, 2, 2, 4]   # round half to even, both directions
    assert one(254.5, 1, 0) == 254 and one(255.5, 1, 0) == 255 and one(255.49998, 1, 0) == 255
    assert one(-0.5, 1, 0) == 0 and one(-0.0, 1, 0) == 0
    assert one(np.inf, 1, 0) == 255 and one(-np.inf, 1, 0) == 0 and one(np.nan, 1, 0) == 0
    assert one(np.inf, -1, 0) == 0                                 # the sign of the scale counts
    assert one(0x03FF, 65536, 0, fm.F16) == 4                      # the largest float16 subnormal: 1023 * 2^-24 * 2^16 = 3.996
    assert one(0x0001, 65536, 0, fm.F16) == 0
    # no float32 or bfloat16 subnormal reaches 0.5 at the largest scale: the denormal mode of the device cannot matter
    largest = np.array([0x007FFFFF], dtype=np.uint32).view(np.float32)[0]
    assert float(largest) * fm.SCALE_MAX < 0.5
    assert one(float(largest), fm.SCALE_MAX, 0) == 0 and one(0x007F, fm.SCALE_MAX, 0, fm.BF16) == 0
    # the product and the sum round separately: a fused multiply-add would give another byte here
    x, s, o = np.float32(1.0000001), np.float32(127.5), np.float32(-127.0)
    separate = np.float32(np.float32(x * s) + o)
    fused = np.float32(np.float64(x) * np.float64(s) + np.float64(o))
    assert separate != fused


def test_the_edge_picture_cannot_pass_vacuously():
    pic = fm.f32_edge_picture(1)
    for scale, offset in ((1.0, 0.0), (255.0, 0.0)):
        got = fm.bytes_of(pic, fm.F32, scale, offset)
        assert {0, 255} <= set(got.ravel().tolist())
    ties = fm.f32_bits(np.arange(256, dtype=np.float32) + np.float32(0.5))
    b = fm.bytes_of(ties, fm.F32, 1.0, 0.0).astype(int)
    k = np.arange(256)
    assert ((b == k) & (k % 2 == 0)).sum() == 128 and ((b == np.minimum(k + 1, 255)) & (k % 2 == 1)).sum() == 128     # down and up


def test_planes_are_the_colour_model_s(jpegamd):
    import scan_model as sm
    rng = np.random.default_rng(2)
    rgb = rng.integers(0, 256, (5, 7, 3), np.uint8)
    for sub, shape in ((jpegamd.SUBSAMPLE_444, (5, 7)), (jpegamd.SUBSAMPLE_422, (5, 4)), (jpegamd.SUBSAMPLE_420, (3, 4))):
        y, cb, cr = fm.planes(rgb, sub)
        assert y.shape == (5, 7) and cb.shape == cr.shape == shape
        assert np.array_equal(y, sm.luma_plane(rgb))
    assert len(fm.planes(rgb, 0)) == 1


# ---- the C surface ------------------------------------------------------------------------------------------------------------------
def test_symbols_constants_and_prototypes(jpegamd):
    header = jpegamd.HEADER_PATH.read_text()
    raw = C.CDLL(str(jpegamd.LIB_PATH))
    for name in NAMES:
        assert name in jpegamd.EXPORTED and hasattr(raw, name), name
        assert re.search(rf"int32_t\s+{name}\s*\(", header), name
    for name, value in (("F32", 0), ("F16", 1), ("BF16", 2)):
        assert re.search(rf"#define\s+JPEGAMD_FLOAT_{name}\s+{value}\b", header), name
        assert getattr(jpegamd, f"FLOAT_{name}") == value
    struct = re.search(r"typedef struct JpegAmdFloatImage \{(.*?)\} JpegAmdFloatImage;", header, re.S).group(1)
    for field in ("plane[3]", "width, height", "row_stride", "pixel_stride", "quality"):
        assert field in struct, field
    assert [f[0] for f in jpegamd.FloatImage._fields_] == ["plane", "width", "height", "row_stride", "pixel_stride", "quality"]
    assert C.sizeof(jpegamd.FloatImage) == 3 * 8 + 5 * 4 + 4
    # the header states the map and its limits
    for text in ("rounded once to float32", "NOT fused", "round half to even", "16777216", "if t is NaN"):
        assert text in header, text

    def params(name):
        proto = re.search(rf"{name}\s*\((.*?)\)\s*;", header, re.S).group(1)
        return [re.sub(r".*[\s*]", "", p.strip()) for p in proto.split(",")]

    front = ["enc", "imgs", "count", "subsampling", "sample_type", "scale", "offset"]
    back = ["outs_dev", "out_capacity", "out_sizes_dev", "stream"]
    assert params(NAMES[0]) == front + back
    assert params(NAMES[1]) == front + ["restart_interval"] + back
    assert params(NAMES[2]) == front + ["scans", "scan_count"] + back
    for name in NAMES:
        assert len(getattr(jpegamd.lib, name).argtypes) == len(params(name))
        assert getattr(jpegamd.lib, name).argtypes[5:7] == [C.c_float, C.c_float]
    # the debug export is in the library and nowhere public
    assert hasattr(raw, DEBUG_NAME) and DEBUG_NAME not in header and DEBUG_NAME not in jpegamd.EXPORTED
    assert len(getattr(jpegamd.lib, DEBUG_NAME).argtypes) == 11
    for method in ("encode_float_batch_async", "encode_float_interleaved_batch_async", "encode_float_progressive_script_batch_async",
                   "float_image"):
        assert hasattr(jpegamd.Encoder, method), method


def _fake_context():
    """A block of zeros where the context would be: a check that came too late would read it."""
    fake = (C.c_uint8 * (1 << 16))()
    return fake, C.cast(fake, C.c_void_p)


W, H = 64, 32


def _img(jpegamd, i=0, size=4, planes=3, ps=None, rs=None, q=0, w=W, h=H, shift=0, ptrs=None):
    base = 0x100000 * (i + 1) + shift
    ps = size if ps is None else ps
    rs = 2 * ps * w if rs is None else rs
    ptrs = ptrs if ptrs is not None else [base + 0x10000 * k if k < planes else 0 for k in range(3)]
    return jpegamd.Encoder.float_image(ptrs, w, h, rs, ps, q)


def _calls(jpegamd, ctx, imgs, count, sub, sample_type=0, scale=255.0, offset=0.0, outs=True, sizes=True, null_at=None):
    """The four entries with these arguments -> their results."""
    n = max(len(imgs), 1)
    arr = (jpegamd.FloatImage * n)(*imgs) if imgs else None
    out_list = [C.c_void_p(0x1000)] * 40
    size_list = [C.c_void_p(0x2000)] * 40
    if null_at is not None:
        out_list = list(out_list)
        out_list[null_at] = C.c_void_p(0)
    out_arr = (C.c_void_p * 40)(*out_list) if outs else None
    size_arr = (C.c_void_p * 40)(*size_list) if sizes else None
    lib = jpegamd.lib
    s, o = C.c_float(scale), C.c_float(offset)
    buf = C.c_void_p(0x3000)
    res = [lib.jpegamd_encode_float_batch_async(ctx, arr, count, sub, sample_type, s, o, out_arr, CAP, size_arr, None),
           lib.jpegamd_encode_float_interleaved_batch_async(ctx, arr, count, sub, sample_type, s, o, 0, out_arr, CAP, size_arr, None),
           lib.jpegamd_encode_float_progressive_script_batch_async(ctx, arr, count, sub, sample_type, s, o, None, 0, out_arr, CAP, size_arr, None)]
    if outs and sizes and null_at is None:
        res.append(lib.jpegamd_debug_float_planes(ctx, arr, count, sub, sample_type, s, o, buf, buf, buf, None))
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
    for sub in (3, -1, 5, 8):                                      # an unknown subsampling
        refused(good[:2], 2, sub)
    for sample_type in (-1, 3, 16):
        refused(good[:2], 2, s420, sample_type=sample_type)
    for scale in (float("nan"), float("inf"), -float("inf"), 16777218.0, -16777218.0, 3.0e38):
        refused(good[:2], 2, s420, scale=scale)
    for offset in (float("nan"), float("inf"), -float("inf")):
        refused(good[:2], 2, s420, offset=offset)
    refused([_img(j, ptrs=[0, 0x20000, 0x30000])], 1, s444)        # no plane[0]
    refused([_img(j, ptrs=[0x10000, 0x20000, 0])], 1, s444)        # exactly one of plane[1] / plane[2]
    refused([_img(j, ptrs=[0x10000, 0, 0x30000])], 1, s444)
    for sub in (s444, s420, s422):                                 # one channel is a grayscale file alone
        refused(single, 2, sub)
    refused([good[0], single[1]], 2, 0)                            # one channel and three in one call
    for size, sample_type in ((4, j.FLOAT_F32), (2, j.FLOAT_F16), (2, j.FLOAT_BF16)):
        ok = dict(size=size)
        refused([_img(j, shift=1, **ok)], 1, s444, sample_type=sample_type)                    # a pointer off the sample grid
        refused([_img(j, ptrs=[0x10000, 0x20000 + size // 2, 0x30000], **ok)], 1, s444, sample_type=sample_type)
        refused([_img(j, ps=size + 1, rs=4 * size * W, **ok)], 1, s444, sample_type=sample_type)   # strides off the grid
        refused([_img(j, rs=size * W + 1, **ok)], 1, s444, sample_type=sample_type)
        refused([_img(j, ps=size // 2, **ok)], 1, s444, sample_type=sample_type)               # a pixel stride below the sample
        refused([_img(j, ps=0, **ok)], 1, s444, sample_type=sample_type)
        refused([_img(j, ps=-size, **ok)], 1, s444, sample_type=sample_type)
        refused([_img(j, rs=size * W - size, **ok)], 1, s444, sample_type=sample_type)         # a row stride below a row
        refused([_img(j, ps=3 * size, rs=3 * size * W - size, **ok)], 1, s444, sample_type=sample_type)
    refused([_img(j, size=2)], 1, s444, sample_type=j.FLOAT_F32)    # float32 samples at a 2-byte stride
    for kw in (dict(w=0), dict(h=0), dict(w=65536), dict(h=65536), dict(w=-1)):
        refused([_img(j, **kw)], 1, s444)
    for kw in (dict(w=W + 1), dict(h=H + 1), dict(rs=4 * 4 * W), dict(ps=8), dict(q=90)):      # pictures of different geometry
        refused([good[0], _img(j, 1, **kw)], 2, s444)
    # the one-scan entry checks its interval, the progressive entry its script, the plane export its buffers
    arr = (j.FloatImage * 2)(*good[:2])
    outs = (C.c_void_p * 2)(C.c_void_p(0x1000), C.c_void_p(0x1000))
    one, zero = C.c_float(1.0), C.c_float(0.0)
    for ri in (-1, 65536):
        assert j.lib.jpegamd_encode_float_interleaved_batch_async(ctx, arr, 2, s420, 0, one, zero, ri, outs, CAP, outs, None) == ERR_ARG
    bad_script = (j.Scan * 1)(j.Scan(7, 1, 63, 0, 0))
    assert j.lib.jpegamd_encode_float_progressive_script_batch_async(ctx, arr, 2, s420, 0, one, zero, bad_script, 1, outs, CAP, outs, None) == ERR_ARG
    gray_script = (j.Scan * 2)(j.Scan(1, 0, 0, 0, 0), j.Scan(1, 1, 63, 0, 0))
    assert j.lib.jpegamd_encode_float_progressive_script_batch_async(ctx, arr, 2, s420, 0, one, zero, gray_script, 2, outs, CAP, outs, None) == ERR_ARG
    buf = C.c_void_p(0x3000)
    assert j.lib.jpegamd_debug_float_planes(ctx, arr, 2, s420, 0, one, zero, None, buf, buf, None) == ERR_ARG
    assert j.lib.jpegamd_debug_float_planes(ctx, arr, 2, s420, 0, one, zero, buf, None, buf, None) == ERR_ARG
    assert not any(keep)


# ---- Python -------------------------------------------------------------------------------------------------------------------------
def test_value_range(jpegamd):
    vr = jpegamd._value_range
    assert vr((0, 1)) == (255.0, 0.0) and vr((-1, 1)) == (127.5, 127.5) and vr((0, 255)) == (1.0, 0.0)
    assert vr((0.0, 1.0)) == fm.value_range(0, 1)
    for lo, hi in ((0.1, 0.9), (-3, 7), (16, 235), (1, 0), (-0.5, 0.5)):
        scale, offset = vr((lo, hi))
        assert (scale, offset) == fm.value_range(lo, hi)
        assert scale == float(np.float32(255.0 / (hi - lo))) and offset == float(np.float32(-lo * (255.0 / (hi - lo))))
    assert vr((1, 0)) == (-255.0, 255.0)                            # an inverted range inverts the picture
    for bad in (None, 1.0, (0,), (0, 1, 2), ("a", "b"), (0, 0), (1.0, 1.0), (float("nan"), 1), (0, float("inf")), (0, 1e-6), (0, 1e-40)):
        with pytest.raises(ValueError, match="value_range"):
            vr(bad)


def _layout(jpegamd, t, layout, single=False):
    n, h, w, row, pixel, sample_type, channels, ptr, planes = jpegamd._float_layout(t, layout, single)
    return (n, h, w, row, pixel, sample_type, channels), ptr, planes


@pytest.mark.parametrize("dtype,sample_type,size", [(torch.float32, fm.F32, 4), (torch.float16, fm.F16, 2), (torch.bfloat16, fm.BF16, 2)])
def test_layouts_of_host_tensors(jpegamd, dtype, sample_type, size):
    n, h, w = 3, 6, 10
    chw = torch.zeros(n, 3, h, w, dtype=dtype)
    info, ptr, planes = _layout(jpegamd, chw, "chw")
    assert info == (n, h, w, size * w, size, sample_type, 3)
    assert ptr(1) == tuple(chw[1, k].data_ptr() for k in range(3))
    assert all(p.data_ptr() == chw[:, k].data_ptr() for k, p in enumerate(planes))          # views: nothing was copied
    hwc = torch.zeros(n, h, w, 3, dtype=dtype)
    info, ptr, _ = _layout(jpegamd, hwc, "hwc")
    assert info == (n, h, w, 3 * size * w, 3 * size, sample_type, 3)
    assert ptr(2) == tuple(hwc[2].data_ptr() + k * size for k in range(3))
    for name, order in (("rgba", (0, 1, 2)), ("bgra", (2, 1, 0))):
        px4 = torch.zeros(n, h, w, 4, dtype=dtype)
        info, ptr, _ = _layout(jpegamd, px4, name)
        assert info == (n, h, w, 4 * size * w, 4 * size, sample_type, 3)
        assert ptr(0) == tuple(px4.data_ptr() + k * size for k in order)
    gray = torch.zeros(n, h, w, dtype=dtype)
    info, ptr, _ = _layout(jpegamd, gray, "gray")
    assert info == (n, h, w, size * w, size, sample_type, 1) and ptr(1) == (gray[1].data_ptr(),)
    three = [torch.zeros(n, h, w, dtype=dtype) for _ in range(3)]
    info, ptr, _ = _layout(jpegamd, three, "chw")
    assert info == (n, h, w, size * w, size, sample_type, 3) and ptr(1) == tuple(p[1].data_ptr() for p in three)
    # channels_last: the memory of [N, H, W, 3] under the shape [N, 3, H, W]
    cl = chw.contiguous(memory_format=torch.channels_last)
    info, ptr, _ = _layout(jpegamd, cl, "chw")
    assert info == (n, h, w, 3 * size * w, 3 * size, sample_type, 3)
    assert ptr(1) == tuple(cl[1].data_ptr() + k * size for k in range(3))
    # a crop, every second picture, every second row, every second column
    crop = chw[:, :, 1:5, 2:9]
    info, ptr, _ = _layout(jpegamd, crop, "chw")
    assert info == (n, 4, 7, size * w, size, sample_type, 3) and ptr(0)[0] == chw.data_ptr() + size * (w + 2)
    info, ptr, _ = _layout(jpegamd, chw[::2], "chw")
    assert info[0] == 2 and ptr(1)[0] == chw[2].data_ptr()
    info, _, _ = _layout(jpegamd, chw[:, :, ::2], "chw")
    assert info == (n, 3, w, 2 * size * w, size, sample_type, 3)
    info, _, _ = _layout(jpegamd, chw[:, :, :, ::2], "chw")
    assert info == (n, h, 5, size * w, 2 * size, sample_type, 3)
    # one picture
    info, ptr, _ = _layout(jpegamd, chw[0], "chw", single=True)
    assert info == (1, h, w, size * w, size, sample_type, 3) and ptr(0) == tuple(chw[0, k].data_ptr() for k in range(3))
    info, _, _ = _layout(jpegamd, gray[0], "gray", single=True)
    assert info == (1, h, w, size * w, size, sample_type, 1)
    # one row, one column: the stride of a dimension of one does not count
    info, _, _ = _layout(jpegamd, chw[:, :, :1], "chw")
    assert info == (n, 1, w, size * w, size, sample_type, 3)
    info, _, _ = _layout(jpegamd, chw[:, :, :, :1], "chw")
    assert info == (n, h, 1, size * w, size, sample_type, 3)


def test_layout_value_errors(jpegamd):
    f = torch.zeros(2, 3, 6, 10)
    cases = [
        (f, "nchw", "layout must be"), (f, None, "layout must be"), (f.to(torch.uint8), "chw", "float32, float16 or bfloat16"),
        (f.double(), "chw", "float32, float16 or bfloat16"), (f.numpy(), "chw", "float32, float16 or bfloat16"),
        ([f[:, 0], f[:, 1]], "chw", "three of them"), ([f[:, 0], f[:, 1], f[:, 2].half()], "chw", "one dtype"),
        ([f[:, 0], f[:, 1], f[:, 2, :5]], "chw", "one shape"), (f[0], "chw", r"\[N, 3, H, W\]"), (f[:, :2], "chw", r"\[N, 3, H, W\]"),
        (torch.zeros(2, 6, 10, 4), "hwc", r"\[N, H, W, 3\]"), (torch.zeros(2, 6, 10, 3), "rgba", r"\[N, H, W, 4\]"),
        (f, "gray", r"\[N, H, W\]"), (torch.zeros(0, 3, 6, 10), "chw", "at least one picture"),
        (torch.zeros(1, 3, 2, 65536), "chw", "1..65535"),
        (f[:, :, :, :1].expand(2, 3, 6, 10), "chw", "positive stride"),
        (f[:, :, :1].expand(2, 3, 6, 10), "chw", "rows overlap"), (f.transpose(2, 3), "chw", "rows overlap"),
        ([f[:, 0], f[:, 1], torch.zeros(2, 6, 20)[:, :, ::2]], "chw", "one pixel stride"),
        ([f[:, 0], f[:, 1], torch.zeros(2, 6, 12)[:, :, :10]], "chw", "one row stride"),
    ]
    for t, layout, match in cases:
        with pytest.raises(ValueError, match=match):
            jpegamd._float_layout(t, layout, False)
    with pytest.raises(ValueError, match=r"\[3, H, W\]"):
        jpegamd._float_layout(f, "chw", True)


def test_python_checks_run_before_the_device(jpegamd):
    import jpegamd.mjpeg as mj
    import jpegamd.progressive as pg
    import jpegamd.progressive_optimized as po
    import jpegamd.progressive_script as ps
    f = torch.zeros(2, 3, 8, 8)
    for fn in (jpegamd.encode_float_batch, mj.encode_float_batch, ps.encode_float_batch):
        with pytest.raises(ValueError, match="device tensors"):
            fn(f)
        with pytest.raises(ValueError, match="value_range"):
            fn(f, value_range=(1, 1))
        with pytest.raises(ValueError, match="subsampling"):
            fn(f, subsampling=3)
        with pytest.raises(ValueError, match="layout"):
            fn(f, layout="nchw")
    with pytest.raises(ValueError, match="device tensors"):
        jpegamd.encode_float(f[0])
    with pytest.raises(ValueError, match="device tensors"):
        jpegamd.encode_float_batch(torch.zeros(2, 8, 8, dtype=torch.bfloat16), layout="gray")     # (one channel: whatever the subsampling)
    with pytest.raises(ValueError, match="huffman"):
        mj.encode_float_batch(f, huffman="best")
    with pytest.raises(ValueError, match="restart_interval"):
        mj.encode_float_batch(f, restart_interval=-1)
    with pytest.raises(ValueError, match="scan"):
        ps.encode_float_batch(f, scans=[((0, 1, 2), 1, 63, 0, 0)])
    # the existing functions keep refusing floats; the progressive modules without a float entry say where to go
    hwc = torch.zeros(2, 8, 8, 3)
    with pytest.raises(ValueError, match="uint8"):
        jpegamd.encode_tensor_batch(hwc)
    with pytest.raises(ValueError, match="uint8"):
        jpegamd.encode_tensor_batch(f, layout="chw")
    for mod in (pg, po):
        with pytest.raises(ValueError, match="progressive_script"):
            mod.encode_tensor_batch(hwc)
