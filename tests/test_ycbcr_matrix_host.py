"""BT.709 YCbCr input on the CPU: the six integers (derived with fractions from the four K constants, and as the library holds them), the
error bound of the integer terms, the map's fixed points and clamps, pinned colours, the order in which the range / depth maps and the
matrix compose, the exported symbol with its constants and prototype, the argument checks of jpegamd_encode_ycbcr_matrix_batch_async
that return before the context is touched, and the matrix argument of the tensor entries.  Nothing here needs a device."""
from __future__ import annotations

import ctypes as C
import re
from fractions import Fraction as F

import numpy as np
import pytest

import depth_model as dm
import matrix_model as mm
import range_model as rm

ERR_ARG = -1
CAP = 1 << 20
NAME = "jpegamd_encode_ycbcr_matrix_batch_async"
DEBUG_NAMES = ("jpegamd_debug_matrix_coeffs", "jpegamd_debug_ycbcr_matrix_planes")


def _lib_coeffs(jpegamd, matrix):
    out = (C.c_int32 * 7)()
    assert jpegamd.lib.jpegamd_debug_matrix_coeffs(matrix, out) == 0
    return list(out)


def test_the_derivation_gives_the_library_s_integers(jpegamd):
    assert mm.coeffs() == [1664, 3213, 16218, -1813, -1187, 16112]
    assert _lib_coeffs(jpegamd, jpegamd.MATRIX_BT709) == mm.coeffs() + [mm.SHIFT]
    assert _lib_coeffs(jpegamd, jpegamd.MATRIX_BT601) == [0, 0, 1 << 14, 0, 0, 1 << 14, 14]      # the identity
    real = [[round(float(c), 6) for c in row] for row in mm.real_matrix()]
    assert real == [[0.101579, 0.196076], [0.989854, -0.110653], [-0.072453, 0.983398]]
    for bad in (-1, 2, 709):
        assert jpegamd.lib.jpegamd_debug_matrix_coeffs(bad, (C.c_int32 * 7)()) == ERR_ARG
    assert jpegamd.lib.jpegamd_debug_matrix_coeffs(jpegamd.MATRIX_BT709, None) == ERR_ARG


def test_every_term_is_within_0_51_of_the_real_one():
    """The rounding half plus two coefficient errors of at most 2^-15 * 128 each: 0.5 + 2 / 256 < 0.51."""
    m, c = mm.real_matrix(), mm.coeffs()
    for k in range(6):
        assert abs(F(c[k], 1 << mm.SHIFT) - m[k // 2][k % 2]) <= F(1, 1 << 15)
    cr, cb = np.meshgrid(np.arange(-128, 128, dtype=np.int64), np.arange(-128, 128, dtype=np.int64), indexing="ij")
    got = mm.terms(cb, cr)
    worst = []
    for k in range(3):
        # exact: the difference scaled by the common denominator of the two fractions, in Python integers
        den = m[k][0].denominator * m[k][1].denominator
        na, nb = m[k][0].numerator * m[k][1].denominator, m[k][1].numerator * m[k][0].denominator
        err = max(abs(int(g) * den - (na * int(b) + nb * int(r))) for g, b, r in zip(got[k].ravel(), cb.ravel(), cr.ravel()))
        worst.append(F(err, den))
        assert worst[-1] <= F(51, 100), (k, float(worst[-1]))
    assert [round(float(x), 4) for x in worst] == [0.5043, 0.5017, 0.5005]
    # the sums stay far inside 32 bits
    assert max(abs(c[2 * k]) + abs(c[2 * k + 1]) for k in range(3)) * 128 + 8192 < 2_400_000


def test_grey_stays_grey_and_both_clamps_of_y_are_reached():
    y = np.arange(256, dtype=np.uint8).reshape(16, 16)
    grey = np.full((16, 16), 128, np.uint8)
    ny, nb, nr = mm.convert((y, grey, grey), mm.SUB_444)
    assert np.array_equal(ny, y) and np.array_equal(nb, grey) and np.array_equal(nr, grey)
    assert mm.terms(0, 0) == (0, 0, 0)
    # every (cb, cr) with Y = 0 and Y = 255: the luma term goes both ways, so both clamps are hit
    cr, cb = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    ty = mm.terms(cb.astype(np.int64) - 128, cr.astype(np.int64) - 128)[0]
    assert ty.min() < 0 < ty.max()
    lo = mm.convert((np.zeros((256, 256), np.uint8), cb, cr), mm.SUB_444)[0]
    hi = mm.convert((np.full((256, 256), 255, np.uint8), cb, cr), mm.SUB_444)[0]
    assert np.array_equal(lo, np.maximum(ty, 0)) and np.array_equal(hi, np.minimum(255 + ty, 255))
    assert (lo == 0).sum() > 256 and (hi == 255).sum() > 256 and lo.max() > 0 and hi.min() < 255


def test_pinned_colours():
    """The BT.709 primaries and white: BT.709 YCbCr of the colour -> what the real-valued matrix gives, rounded -> the integer map."""
    pins = {(255, 0, 0): ((54, 99, 255), (76, 85, 255)), (0, 255, 0): ((182, 30, 12), (149, 44, 21)),
            (0, 0, 255): ((18, 255, 116), (29, 255, 107)), (255, 255, 255): ((255, 128, 128), (255, 128, 128))}
    for rgb, (ycc709, ycc601) in pins.items():
        assert mm.bt709_ycbcr(*rgb) == ycc709, rgb
        assert mm.convert_real(*ycc709) == ycc601, rgb
        got = mm.convert(tuple(np.full((1, 1), v, np.uint8) for v in ycc709), mm.SUB_444)
        assert tuple(int(p[0, 0]) for p in got) == ycc601, rgb
    # ... which is the BT.601 YCbCr of the same colour, up to the double rounding (one level)
    for rgb, (_, ycc601) in pins.items():
        r, g, b = rgb
        y = F(299, 1000) * r + F(587, 1000) * g + F(114, 1000) * b
        direct = (y, 128 + (b - y) / F(1772, 1000), 128 + (r - y) / F(1402, 1000))
        assert all(abs(min(max(d, 0), 255) - v) <= 1 for d, v in zip(direct, ycc601)), rgb


def test_subsampled_sites():
    """Luma (x, y) takes chroma (x >> 1, y) at 4:2:2 and (x >> 1, y >> 1) at 4:2:0: the last odd column and row have a sample of their own."""
    rng = np.random.default_rng(5)
    y = rng.integers(0, 256, (5, 7), np.uint8)
    for sub, shape in ((mm.SUB_444, (5, 7)), (mm.SUB_422, (5, 4)), (mm.SUB_420, (3, 4))):
        cb, cr = rng.integers(0, 256, shape, np.uint8), rng.integers(0, 256, shape, np.uint8)
        ny, nb, nr = mm.convert((y, cb, cr), sub)
        assert ny.shape == y.shape and nb.shape == nr.shape == shape
        for yy in range(5):
            for xx in range(7):
                cy, cx = (yy >> 1 if sub == mm.SUB_420 else yy), (xx if sub == mm.SUB_444 else xx >> 1)
                t = mm.terms(int(cb[cy, cx]) - 128, int(cr[cy, cx]) - 128)
                assert ny[yy, xx] == min(max(int(y[yy, xx]) + t[0], 0), 255)
                if (yy, xx) == (4, 6):
                    assert nb[cy, cx] == min(max(128 + t[1], 0), 255) and nr[cy, cx] == min(max(128 + t[2], 0), 255)


def test_the_maps_come_first_and_the_matrix_works_on_their_bytes():
    """What the GPU tests expect of limited-range and 10-bit BT.709 input: convert(expand(p)), convert(narrow(p16))."""
    rng = np.random.default_rng(11)
    y, cb, cr = (rng.integers(0, 256, s, np.uint8) for s in ((6, 6), (3, 3), (3, 3)))
    ey, ecb, ecr = rm.expand((y, cb, cr))
    want = mm.convert((ey, ecb, ecr), mm.SUB_420)
    # ... and not the other order: the matrix on limited-range bytes, then the expansion
    other = rm.expand(mm.convert((y, cb, cr), mm.SUB_420))
    assert not all(np.array_equal(a, b) for a, b in zip(want, other))
    assert want[0][0, 0] == min(max(int(ey[0, 0]) + mm.terms(int(ecb[0, 0]) - 128, int(ecr[0, 0]) - 128)[0], 0), 255)
    p16 = tuple(rng.integers(0, 65536, s, np.uint16) for s in ((6, 6), (3, 3), (3, 3)))
    for sample_range in (dm.FULL, dm.LIMITED):
        for align in (dm.MSB, dm.LSB):
            n = dm.narrow(p16, sample_range, align)
            got = mm.convert(n, mm.SUB_420)
            assert all(g.dtype == np.uint8 for g in got)
            t = mm.terms(int(n[1][2, 2]) - 128, int(n[2][2, 2]) - 128)
            assert got[0][5, 5] == min(max(int(n[0][5, 5]) + t[0], 0), 255)


def test_matrix_symbol_constants_and_prototype(jpegamd):
    header = jpegamd.HEADER_PATH.read_text()
    raw = C.CDLL(str(jpegamd.LIB_PATH))
    assert NAME in jpegamd.EXPORTED and hasattr(raw, NAME)
    assert re.search(rf"int32_t\s+{NAME}\s*\(", header)
    for name, value in (("BT601", 0), ("BT709", 1)):
        assert re.search(rf"#define\s+JPEGAMD_MATRIX_{name}\s+{value}\b", header), name
        assert getattr(jpegamd, f"MATRIX_{name}") == value
    for older in ("jpegamd_encode_ycbcr_batch_async", "jpegamd_encode_ycbcr_range_batch_async", "jpegamd_encode_ycbcr_samples_batch_async"):
        assert older in jpegamd.EXPORTED and hasattr(jpegamd.lib, older)
    assert "no range or matrix conversion" in header.lower()
    # the header states the map: the six integers and the shift
    for number in ("1664", "3213", "16218", "1813", "1187", "16112", ">> 14"):
        assert number in header, number
    proto = re.search(rf"{NAME}\s*\((.*?)\)\s*;", header, re.S).group(1)
    names = [re.sub(r".*[\s*]", "", p.strip()) for p in proto.split(",")]
    assert names == ["enc", "imgs", "count", "subsampling", "sample_range", "sample_format", "matrix", "outs_dev", "out_capacity",
                     "out_sizes_dev", "stream"]
    assert len(jpegamd.lib.jpegamd_encode_ycbcr_matrix_batch_async.argtypes) == len(names)
    # the debug exports are in the library and nowhere public
    for name in DEBUG_NAMES:
        assert hasattr(raw, name) and name not in header and name not in jpegamd.EXPORTED
    assert len(jpegamd.lib.jpegamd_debug_ycbcr_matrix_planes.argtypes) == 11


def _fake_context():
    """A block of zeros where the context would be: a check that came too late would read it."""
    fake = (C.c_uint8 * (1 << 16))()
    return fake, C.cast(fake, C.c_void_p)


def _call(jpegamd, ctx, imgs, count, sub, rng, fmt, matrix, outs=True, sizes=True):
    n = max(len(imgs), 1)
    arr = (jpegamd.YCbCrImage * n)(*imgs) if imgs else None
    out_arr = (C.c_void_p * 40)(*([C.c_void_p(0x1000)] * 40)) if outs else None
    size_arr = (C.c_void_p * 40)(*([C.c_void_p(0x2000)] * 40)) if sizes else None
    return jpegamd.lib.jpegamd_encode_ycbcr_matrix_batch_async(ctx, arr, count, sub, rng, fmt, matrix, out_arr, CAP, size_arr, None)


def test_matrix_argument_checks_come_before_the_context(jpegamd):
    keep, ctx = _fake_context()
    s420, s444, s422 = jpegamd.SUBSAMPLE_420, jpegamd.SUBSAMPLE_444, jpegamd.SUBSAMPLE_422
    full, lim, s8, msb, lsb = jpegamd.RANGE_FULL, jpegamd.RANGE_LIMITED, jpegamd.SAMPLES_8, jpegamd.SAMPLES_10_MSB, jpegamd.SAMPLES_10_LSB
    w, h = 64, 32

    def img(i=0, layout=jpegamd.CHROMA_PLANES, ys=2 * w, cs=2 * w, q=0, y=None):
        base = 0x100000 * (i + 1)
        return jpegamd.Encoder.ycbcr_image(base if y is None else y, base + 0x10000, base + 0x20000, w, h, ys, cs, layout, q)

    good = [img(i) for i in range(40)]
    packed = [img(i, jpegamd.CHROMA_YUYV) for i in range(2)]
    # every bad matrix: otherwise perfect arguments, every subsampling, range, format and count
    for matrix in (-1, 2, 3, 601, 709, 1 << 16):
        for sub in (s444, s420, s422):
            for rng in (full, lim):
                for fmt in (s8, msb, lsb):
                    assert _call(jpegamd, ctx, good[:1], 1, sub, rng, fmt, matrix) == ERR_ARG, (matrix, sub, rng, fmt)
                    assert _call(jpegamd, ctx, good[:3], 3, sub, rng, fmt, matrix) == ERR_ARG, (matrix, sub, rng, fmt)
        assert _call(jpegamd, ctx, packed, 2, s422, full, s8, matrix) == ERR_ARG, matrix
    # a valid matrix: every refusal of the samples entry still fires, before the context is read
    for matrix in (jpegamd.MATRIX_BT601, jpegamd.MATRIX_BT709):
        assert _call(jpegamd, None, good[:2], 2, s420, full, s8, matrix) == ERR_ARG                # null context
        assert _call(jpegamd, ctx, [], 1, s420, full, s8, matrix) == ERR_ARG                       # null array
        for count in (0, -1, 33):
            assert _call(jpegamd, ctx, good[:max(count, 1)], count, s420, full, s8, matrix) == ERR_ARG, count
        assert _call(jpegamd, ctx, good[:2], 2, s420, full, s8, matrix, outs=False) == ERR_ARG
        assert _call(jpegamd, ctx, good[:2], 2, s420, full, s8, matrix, sizes=False) == ERR_ARG
        for rng in (-1, 2):
            assert _call(jpegamd, ctx, good[:2], 2, s420, rng, s8, matrix) == ERR_ARG, rng
        for fmt in (-1, 3):
            assert _call(jpegamd, ctx, good[:2], 2, s420, full, fmt, matrix) == ERR_ARG, fmt
        for sub in (s444, s420):                                                                    # a packed layout is 4:2:2 alone
            assert _call(jpegamd, ctx, packed, 2, sub, full, s8, matrix) == ERR_ARG, sub
        assert _call(jpegamd, ctx, packed, 2, s422, full, msb, matrix) == ERR_ARG                  # ... and one byte per sample
        for sub in (0, 3, -1):                                                                      # an unknown subsampling
            assert _call(jpegamd, ctx, good[:2], 2, sub, full, s8, matrix) == ERR_ARG, sub
        for kw in (dict(ys=w - 1), dict(cs=w - 1), dict(cs=0), dict(layout=jpegamd.CHROMA_CBCR, cs=2 * w - 1)):     # a stride too short
            assert _call(jpegamd, ctx, [img(**kw)], 1, s444, full, s8, matrix) == ERR_ARG, kw
        assert _call(jpegamd, ctx, [img(ys=2 * w - 1)], 1, s444, full, msb, matrix) == ERR_ARG     # (16-bit words: twice the bytes)
        assert _call(jpegamd, ctx, [img(layout=3)], 1, s444, full, s8, matrix) == ERR_ARG          # an unknown layout
        assert _call(jpegamd, ctx, [img(y=0)], 1, s444, full, s8, matrix) == ERR_ARG               # a null plane
        assert _call(jpegamd, ctx, [good[0], img(1, q=90)], 2, s444, full, s8, matrix) == ERR_ARG  # mixed geometry
    # the plane export checks the same arguments, and has a pass for BT709 alone
    arr = (jpegamd.YCbCrImage * 2)(*good[:2])
    buf = C.c_void_p(0x3000)
    planes = jpegamd.lib.jpegamd_debug_ycbcr_matrix_planes
    assert planes(ctx, arr, 2, s420, full, s8, 2, buf, buf, buf, None) == ERR_ARG
    assert planes(ctx, arr, 2, s420, full, s8, jpegamd.MATRIX_BT601, buf, buf, buf, None) == ERR_ARG
    assert planes(ctx, arr, 2, 0, full, s8, jpegamd.MATRIX_BT709, buf, buf, buf, None) == ERR_ARG
    assert planes(None, arr, 2, s420, full, s8, jpegamd.MATRIX_BT709, buf, buf, buf, None) == ERR_ARG
    assert planes(ctx, arr, 2, s420, full, s8, jpegamd.MATRIX_BT709, None, buf, buf, None) == ERR_ARG
    assert not any(keep)


def test_a_bad_matrix_is_a_value_error_on_host_tensors(jpegamd):
    torch = pytest.importorskip("torch")
    y, cb, cr = (torch.zeros(2, 8, 8, dtype=torch.uint8), torch.zeros(2, 4, 4, dtype=torch.uint8), torch.zeros(2, 4, 4, dtype=torch.uint8))
    y16, cb16, cr16 = y.to(torch.int16), cb.to(torch.int16), cr.to(torch.int16)
    frames = torch.zeros(2, 8, 8, 2, dtype=torch.uint8)
    for bad in ("709", "BT709", "rec709", "", None, 1, jpegamd.MATRIX_BT709, b"bt709"):
        with pytest.raises(ValueError, match="matrix"):
            jpegamd.encode_ycbcr_batch(y, cb, cr, matrix=bad)
        with pytest.raises(ValueError, match="matrix"):
            jpegamd.encode_ycbcr16_batch(y16, cb16, cr16, matrix=bad)
        with pytest.raises(ValueError, match="matrix"):
            jpegamd.encode_yuyv_batch(frames, matrix=bad)
    # a good one passes that check: well-formed host tensors then only lack a device
    for ok in ("bt601", "bt709"):
        with pytest.raises(ValueError, match="device tensor"):
            jpegamd.encode_ycbcr_batch(y, cb, cr, matrix=ok)
        with pytest.raises(ValueError, match="device tensor"):
            jpegamd.encode_ycbcr16_batch(y16, cb16, cr16, matrix=ok)
        with pytest.raises(ValueError, match="device tensor"):
            jpegamd.encode_yuyv_batch(frames, matrix=ok)
