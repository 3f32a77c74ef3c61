"""The one-scan files from every source on the GPU (jpegamd_encode_ycbcr_interleaved_matrix_batch_async,
jpegamd_encode_color_interleaved_pixels_batch_async, jpegamd_encode_planar_interleaved_batch_async, jpegamd.mjpeg): every device file
is compared byte for byte with the CPU models (interleaved_model / restart_model over the planes that depth_model, range_model and
matrix_model make of the stored samples).  tests/test_mjpeg_host.py asserts on the CPU that these inputs exercise what the cases claim.
Every test needs an MI355X."""
from __future__ import annotations

import numpy as np
import pytest

import color_model as cm
import gpu_support as gs
import interleaved_model as im
import mjpeg_support as ms
from gpu_support import dev  # noqa: F401
from mjpeg_support import CBCR, CRCB, PLANES, S420, S422, S444, SUBS, UYVY, YUYV

torch = gs.torch
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def enc(jpegamd, dev):
    e = jpegamd.Encoder(512, gs.rows_for(32, 16))
    yield e
    e.close()


def check(jpegamd, oracle, enc, dev, kind, planes, sub, layout, ri=0, q=0, **kw):
    """One batch of stored planes through the new YCbCr entry: files and counters are the model's."""
    models = [ms.ycc_model(oracle, ms.mapped_planes(kind, p, sub), q, sub, ri) for p in planes]
    files, st = ms.ycc_files(jpegamd, enc, kind, planes, dev, sub, layout, ri, q, **kw)
    assert files == [m.file for m in models], (kind.name, sub, layout, ri, kw)
    assert st.entropy_bits == sum(m.scan_bits for m in models) and st.stuffed_bytes == sum(m.stuffed for m in models), (kind.name, sub, layout, ri)
    return files, st


# ---- 1. kinds -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(17, 9), (200, 120)])
@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("kind", ms.KINDS, ids=lambda k: k.name)
def test_kinds(jpegamd, oracle, dev, enc, kind, sub, w, h):
    planes = [ms.stored_planes(kind, w, h, sub, 100 + w)]
    for layout in (PLANES, CBCR, CRCB):
        check(jpegamd, oracle, enc, dev, kind, planes, sub, layout, q=75)


@pytest.mark.parametrize("w,h", [(18, 9), (200, 120)])
@pytest.mark.parametrize("kind", (ms.FULL8, ms.LIMITED8), ids=lambda k: k.name)
def test_packed_422(jpegamd, oracle, dev, enc, kind, w, h):
    planes = [ms.stored_planes(kind, w, h, S422, 200 + w)]
    for layout in (YUYV, UYVY):
        check(jpegamd, oracle, enc, dev, kind, planes, S422, layout, q=75)


BT709_CASES = [("nv12-limited", ms.LIMITED8_709, CBCR, S420, 17), ("i420", ms.FULL8_709, PLANES, S420, 17),
               ("p010-limited", ms.LIMITED10_709, CBCR, S420, 17), ("yuyv", ms.FULL8_709, YUYV, S422, 18)]      # (a packed frame has an even width)


@pytest.mark.parametrize("name,kind,layout,sub,w,h", [c + (9,) for c in BT709_CASES] + [c[:4] + (200, 120) for c in BT709_CASES],
                         ids=[f"{c[0]}-{s}" for s in ("small", "200x120") for c in BT709_CASES])
def test_bt709(jpegamd, oracle, dev, enc, name, kind, layout, sub, w, h):
    check(jpegamd, oracle, enc, dev, kind, [ms.stored_planes(kind, w, h, sub, 300 + w)], sub, layout, q=75)


# ---- 2. equivalence on the device -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,layout,sub", [(ms.LIMITED8, CBCR, S420), (ms.MSB10, CBCR, S420), (ms.FULL8, YUYV, S422), (ms.LIMITED8_709, CBCR, S420)],
                         ids=["nv12-limited", "p010", "yuyv", "bt709"])
def test_new_entry_equals_the_old_entry_over_mapped_planes(jpegamd, oracle, dev, enc, kind, layout, sub):
    stored = ms.stored_planes(kind, 72, 40, sub, 41)
    mapped = ms.mapped_planes(kind, stored, sub)
    for ri in (0, 3):
        (new,), _ = ms.ycc_files(jpegamd, enc, kind, [stored], dev, sub, layout, ri, 50)
        (old,), _ = gs.finish_files(enc, ms.OldYccCall(jpegamd, enc, [mapped], dev, sub, PLANES, ri, 50))
        assert new == old == ms.ycc_model(oracle, mapped, 50, sub, ri).file, ri


# ---- 3. the old kinds through the new entry -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", (CBCR, PLANES), ids=["nv12", "i420"])
def test_old_kinds_through_the_new_entry(jpegamd, oracle, dev, enc, layout):
    planes = [ms.stored_planes(ms.FULL8, 72, 40, S420, 51 + k, smooth=bool(k)) for k in range(2)]
    for ri in (0, 2):
        new, _ = ms.ycc_files(jpegamd, enc, ms.FULL8, planes, dev, S420, layout, ri, 50)
        old, _ = gs.finish_files(enc, ms.OldYccCall(jpegamd, enc, planes, dev, S420, layout, ri, 50))
        assert new == old == [ms.ycc_model(oracle, p, 50, S420, ri).file for p in planes], ri


# ---- 4. loaders -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", SUBS)
def test_odd_addresses_and_strides(jpegamd, oracle, dev, enc, sub):
    """33 x 17, every plane one byte into its allocation, row strides off the dword grid: the clamped byte loader of every source."""
    w, h = 33, 17
    cw, _ = gs.chroma_dims(w, h, sub)
    odd = dict(y_shifts=[1], c_shifts=[1])
    assert cw % 2 == 1                                               # 33 or 17 samples
    p8 = [ms.stored_planes(ms.LIMITED8, w, h, sub, 61)]
    check(jpegamd, oracle, enc, dev, ms.LIMITED8, p8, sub, CRCB, ri=3, y_stride=37, c_stride=2 * cw + 3, **odd)
    check(jpegamd, oracle, enc, dev, ms.LIMITED8, p8, sub, PLANES, y_stride=35, c_stride=cw + 2, **odd)
    for kind in (ms.MSB10, ms.LIMITED10, ms.LSB10):
        p16 = [ms.stored_planes(kind, w, h, sub, 62)]
        check(jpegamd, oracle, enc, dev, kind, p16, sub, PLANES, y_stride=2 * w, c_stride=2 * cw, **odd)        # an odd number of words per row
        check(jpegamd, oracle, enc, dev, kind, p16, sub, CBCR, ri=2, y_stride=2 * w, c_stride=4 * cw + 2, **odd)
    if sub == S422:
        pk = [ms.stored_planes(ms.LIMITED8, 34, h, sub, 63)]
        for layout in (YUYV, UYVY):
            check(jpegamd, oracle, enc, dev, ms.LIMITED8, pk, sub, layout, ri=1, y_stride=4 * 17 + 1, **odd)
    rgb = ms.synth_rgb(w, h, 64)
    want = ms.rgb_model(oracle, rgb, 50, sub, 2).file
    (f,), _ = gs.finish_files(enc, ms.PixelsCall(jpegamd, enc, [rgb], dev, sub, "rgba", 2, 50, stride=4 * w + 3, shift=1))
    assert f == want
    (f,), _ = gs.finish_files(enc, ms.PlanarCall(jpegamd, enc, [rgb], dev, sub, 2, 50, stride=w + 2, shifts=(1, 1, 1)))
    assert f == want
    (f,), _ = gs.finish_files(enc, ms.PlanarCall(jpegamd, enc, [rgb], dev, sub, 2, 50, stride=w + 3, shifts=(0, 1, 0)))      # G alone misaligned
    assert f == want


def test_planar_with_only_the_g_plane_misaligned(jpegamd, oracle, dev, enc):
    """An aligned stride and aligned R and B planes: the dword loader would be taken if the answer came from the R pointer alone."""
    rgbs = gs.pictures(jpegamd, 72, 40, 2, seed=7)
    want = [ms.rgb_model(oracle, r, 50, S420).file for r in rgbs]
    for shifts in ((0, 1, 0), (0, 0, 2), (0, 0, 0)):
        files, _ = gs.finish_files(enc, ms.PlanarCall(jpegamd, enc, rgbs, dev, S420, 0, 50, stride=72, shifts=shifts))
        assert files == want, shifts


# ---- 5. RGB layouts -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(17, 9), (40, 24)])
@pytest.mark.parametrize("sub", SUBS)
def test_rgb_layouts(jpegamd, oracle, dev, enc, sub, w, h):
    rgbs = gs.pictures(jpegamd, w, h, 2, seed=w)
    want = [ms.rgb_model(oracle, r, 75, sub).file for r in rgbs]
    old, _ = gs.finish_files(enc, ms.OldRgbCall(jpegamd, enc, rgbs, dev, sub, 0, 75))
    assert old == want
    calls = [lambda: ms.PixelsCall(jpegamd, enc, rgbs, dev, sub, "rgba", 0, 75), lambda: ms.PixelsCall(jpegamd, enc, rgbs, dev, sub, "bgra", 0, 75),
             lambda: ms.PixelsCall(jpegamd, enc, rgbs, dev, sub, "bgra", 0, 75, bottom_up=True),
             lambda: ms.PixelsCall(jpegamd, enc, rgbs, dev, sub, "rgba", 0, 75, stride=4 * w + 64),
             lambda: ms.PixelsCall(jpegamd, enc, rgbs, dev, sub, "rgb", 0, 75), lambda: ms.PixelsCall(jpegamd, enc, rgbs, dev, sub, "bgr", 0, 75),
             lambda: ms.PlanarCall(jpegamd, enc, rgbs, dev, sub, 0, 75), lambda: ms.PlanarCall(jpegamd, enc, rgbs, dev, sub, 0, 75, bottom_up=True),
             lambda: ms.PlanarCall(jpegamd, enc, rgbs, dev, sub, 0, 75, stride=w + 12)]
    for i, call in enumerate(calls):
        files, _ = gs.finish_files(enc, call())
        assert files == want, i


# ---- 6. restart intervals ---------------------------------------------------------------------------------------------------------------------
FAMILIES = [("nv12-limited", ms.LIMITED8, CBCR, S420), ("p010", ms.MSB10, CBCR, S420), ("yuyv", ms.FULL8, YUYV, S422),
            ("bt709", ms.LIMITED8_709, CBCR, S420), ("rgba", None, None, S444)]


@pytest.mark.parametrize("w,h", [(24, 40), (200, 120)])
@pytest.mark.parametrize("name,kind,layout,sub", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_restart_intervals(jpegamd, oracle, dev, enc, name, kind, layout, sub, w, h):
    _, _, _, _, mx, my = im.geometry(w, h, sub)
    assert ms.row_interval(w, sub) == mx
    rgb = ms.synth_rgb(w, h, 70 + w)
    planes = None if kind is None else [ms.stored_planes(kind, w, h, sub, 71 + w)]
    for ri in sorted({1, mx + 1, mx, mx * my + 5}):
        if kind is not None:
            check(jpegamd, oracle, enc, dev, kind, planes, sub, layout, ri, 75)
            continue
        m = ms.rgb_model(oracle, rgb, 75, sub, ri)
        (f,), st = gs.finish_files(enc, ms.PixelsCall(jpegamd, enc, [rgb], dev, sub, "rgba", ri, 75))
        assert f == m.file, ri
        assert st.entropy_bits == m.scan_bits and st.stuffed_bytes == m.stuffed, ri


# ---- 7. batches ---------------------------------------------------------------------------------------------------------------------------
def test_batch_of_three_crcb_limited(jpegamd, oracle, dev, enc):
    planes = [ms.stored_planes(ms.LIMITED8, 40, 24, S420, 80 + k, smooth=bool(k % 2)) for k in range(3)]
    files, _ = check(jpegamd, oracle, enc, dev, ms.LIMITED8, planes, S420, CRCB, q=50)
    assert len(set(files)) == 3
    check(jpegamd, oracle, enc, dev, ms.LIMITED8, planes, S420, CRCB, ri=2, q=50)


def test_batch_of_thirty_two_p010(jpegamd, oracle, dev, enc):
    planes = [ms.stored_planes(ms.MSB10, 16, 16, S420, 90 + k, smooth=bool(k % 2)) for k in range(32)]
    check(jpegamd, oracle, enc, dev, ms.MSB10, planes, S420, CBCR, q=90)


def test_bt709_batch_grows_both_scratches_on_a_fresh_context(jpegamd, oracle, dev):
    e = jpegamd.Encoder(512, gs.rows_for(32, 16))
    try:
        five = [ms.stored_planes(ms.LIMITED8_709, 72, 40, S420, 95 + k, smooth=True) for k in range(5)]
        check(jpegamd, oracle, e, dev, ms.LIMITED8_709, five, S420, CBCR, q=50)
        check(jpegamd, oracle, e, dev, ms.LIMITED8_709, five[3:4], S420, CBCR, q=50)
        check(jpegamd, oracle, e, dev, ms.FULL8_709, [ms.stored_planes(ms.FULL8_709, 24, 16, S444, 99)], S444, PLANES, ri=1, q=50)
    finally:
        e.close()


# ---- 8. neighbours ------------------------------------------------------------------------------------------------------------------------
def test_neighbours_on_the_same_context_are_unchanged(jpegamd, oracle, dev, enc):
    planes = [ms.stored_planes(ms.LIMITED8, 72, 40, S420, 110 + k, smooth=True) for k in range(3)]
    mapped = [ms.mapped_planes(ms.LIMITED8, p, S420) for p in planes]
    grays = [p[0] for p in mapped]
    want_three = [ms.three_scan_model(oracle, p, 50, S420) for p in mapped]
    want_gray = [cm.memo(cm.gray_file, oracle, g, 50) for g in grays]
    for _ in range(2):                                              # each before and after the others
        files, _ = gs.finish_files(enc, gs.YccBatch(jpegamd, enc, planes, dev, S420, CBCR, quality=50, sample_range=jpegamd.RANGE_LIMITED))
        assert files == want_three
        check(jpegamd, oracle, enc, dev, ms.LIMITED8, planes, S420, CBCR, q=50)
        files, _ = gs.encode_gray_planes(jpegamd, enc, grays, dev, 50)
        assert files == want_gray
        check(jpegamd, oracle, enc, dev, ms.LIMITED8, planes, S420, CBCR, ri=5, q=50)


# ---- 9. exact_fallbacks -------------------------------------------------------------------------------------------------------------------
def test_exact_fallbacks_equal_the_three_scan_figure(jpegamd, oracle, dev, enc):
    planes = [ms.stored_planes(ms.LIMITED8, 200, 120, S420, 120, smooth=False)]         # noise: the quantiser meets ties
    _, st3 = gs.finish_files(enc, gs.YccBatch(jpegamd, enc, planes, dev, S420, CBCR, quality=90, sample_range=jpegamd.RANGE_LIMITED))
    _, st1 = check(jpegamd, oracle, enc, dev, ms.LIMITED8, planes, S420, CBCR, q=90)
    print(f"exact_fallbacks: three-scan {st3.exact_fallbacks}, one scan {st1.exact_fallbacks}")
    assert st1.exact_fallbacks == st3.exact_fallbacks > 0


# ---- 10. capacity -------------------------------------------------------------------------------------------------------------------------
def test_capacity_one_byte_short_for_the_middle_picture(jpegamd, oracle, dev, enc):
    kind = ms.MSB10
    small = ms.stored_planes(kind, 40, 24, S420, 130, smooth=True)
    big = ms.stored_planes(kind, 40, 24, S420, 131, smooth=False)
    planes = [small, big, tuple(np.ascontiguousarray(p[::-1]) for p in small)]
    models = [ms.ycc_model(oracle, ms.mapped_planes(kind, p, S420), 50, S420, 2) for p in planes]
    cap = len(models[1].file) - 1
    assert len(models[0].file) < cap and len(models[2].file) < cap
    call = ms.ycc_call(jpegamd, enc, kind, planes, dev, S420, CBCR, 2, 50, cap=cap)
    with pytest.raises(jpegamd.JpegAmdError) as err:
        enc.finish()
    assert err.value.code == -8                                     # JPEGAMD_ERR_HUFF_CAPACITY
    files = gs.intact_files(call)                                   # the guard behind out_capacity is untouched
    assert call.sizes.cpu().tolist() == [len(models[0].file), 0, len(models[2].file)]
    assert files[0] == models[0].file and files[2] == models[2].file
    check(jpegamd, oracle, enc, dev, kind, [big], S420, CBCR, ri=2, q=50)                 # the context is usable again


# ---- 11. an independent decoder -------------------------------------------------------------------------------------------------------------
class WithMatrix:
    """An Encoder as gpu_support.YccBatch sees it, with the matrix added to its three-scan YCbCr calls."""

    def __init__(self, jpegamd, enc, matrix):
        self.enc, self.matrix = enc, matrix

    def encode_ycbcr_batch_async(self, imgs, subsampling, out_ptrs, out_cap, size_ptrs, stream=0, sample_range=0, sample_format=0):
        self.enc.encode_ycbcr_batch_async(imgs, subsampling, out_ptrs, out_cap, size_ptrs, stream, sample_range, sample_format=sample_format,
                                          matrix=self.matrix)


def test_independent_decoder_sees_the_pixels_of_the_three_scan_file(jpegamd, oracle, dev, enc):
    for kind in (ms.LIMITED8_709, ms.MSB10):
        planes = [ms.stored_planes(kind, 200, 120, S420, 140, smooth=True)]
        rng, fmt, matrix = kind.args(jpegamd)
        (three,), _ = gs.finish_files(enc, gs.YccBatch(jpegamd, WithMatrix(jpegamd, enc, matrix), planes, dev, S420, CBCR, quality=75,
                                                       sample_range=rng, sample_format=fmt))
        want = ms.decode(three)
        assert want.shape == (120, 200, 3)
        for ri in (0, 13):
            (one,), _ = ms.ycc_files(jpegamd, enc, kind, planes, dev, S420, CBCR, ri, 75)
            assert np.array_equal(ms.decode(one), want), (kind.name, ri)
    rgb = ms.synth_rgb(200, 120, 141)
    (three,), _ = gs.finish_files(enc, gs.ColorBatch(jpegamd, enc, [rgb], dev, S420, 75))
    for ri in (0, 13):
        (one,), _ = gs.finish_files(enc, ms.PixelsCall(jpegamd, enc, [rgb], dev, S420, "rgba", ri, 75))
        assert np.array_equal(ms.decode(one), ms.decode(three)), ri


# ---- 12. the binding ----------------------------------------------------------------------------------------------------------------------
def test_binding(jpegamd, oracle, dev):
    from jpegamd import mjpeg
    w, h, sub = 24, 40, S420
    row = ms.row_interval(w, sub)

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def want(kind, stored, s, ri):
        return [ms.ycc_model(oracle, ms.mapped_planes(kind, p, s), 0, s, ri).file for p in stored]

    for arg, ri in ((None, 0), ("row", row)):
        # 8-bit: NV12 limited BT.709, I420 limited
        kind = ms.LIMITED8_709
        stored = [ms.stored_planes(kind, w, h, sub, 150 + k, smooth=True) for k in range(2)]
        y, cb, cr = (np.stack([p[k] for p in stored]) for k in range(3))
        pairs = np.stack([cb, cr], axis=3)
        assert mjpeg.encode_ycbcr_batch(t(y), t(pairs), restart_interval=arg, **kind.binding()) == want(kind, stored, sub, ri)
        assert mjpeg.encode_ycbcr_batch(t(y), t(cb), t(cr), sample_range="limited", restart_interval=arg) == want(ms.LIMITED8, stored, sub, ri)
        # 16-bit: P010 limited
        kind = ms.LIMITED10
        stored = [ms.stored_planes(kind, w, h, sub, 152 + k, smooth=True) for k in range(2)]
        y, cb, cr = (np.stack([p[k] for p in stored]).view(np.int16) for k in range(3))
        assert mjpeg.encode_ycbcr16_batch(t(y), t(np.stack([cb, cr], axis=3)), restart_interval=arg, **kind.binding()) == want(kind, stored, sub, ri)
        # packed 4:2:2: UYVY limited
        kind = ms.LIMITED8
        stored = [ms.stored_planes(kind, w, h, S422, 154 + k, smooth=True) for k in range(2)]
        frames = np.stack([ms.m422.pack_yuyv(*p, "uyvy") for p in stored]).reshape(2, h, w, 2)
        assert mjpeg.encode_yuyv_batch(t(frames), order="uyvy", sample_range="limited", restart_interval=arg) == want(kind, stored, S422, ri)
        # tensors
        rgbs = gs.pictures(jpegamd, w, h, 2, seed=15)
        files = [ms.rgb_model(oracle, r, 0, sub, ri).file for r in rgbs]
        hwc = np.stack(rgbs)
        rgba = np.concatenate([hwc, np.full(hwc.shape[:3] + (1,), 9, np.uint8)], axis=3)
        assert mjpeg.encode_tensor_batch(t(hwc), restart_interval=arg) == files
        assert mjpeg.encode_tensor_batch(t(rgba), layout="rgba", restart_interval=arg) == files
        assert mjpeg.encode_tensor_batch(t(rgba[..., [2, 1, 0, 3]]), layout="bgra", restart_interval=arg) == files
        assert mjpeg.encode_tensor_batch(t(hwc.transpose(0, 3, 1, 2)), layout="chw", restart_interval=arg) == files
        assert mjpeg.encode_tensor(t(hwc[1]), restart_interval=arg) == files[1]
        assert mjpeg.encode_tensor(t(hwc[0].transpose(2, 0, 1)), layout="chw", restart_interval=arg) == files[0]
        assert mjpeg.encode_tensor(t(rgba[1]), layout="rgba", restart_interval=arg) == files[1]
