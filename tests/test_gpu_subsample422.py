"""4:2:2 colour files (JPEGAMD_SUBSAMPLE_422) and I422 / NV16 / NV61 / YUY2 / UYVY input through the C-ABI into the HIP kernels,
byte for byte against the CPU model of tests/color_model_422.py.  Every test needs an MI355X."""
from __future__ import annotations

import numpy as np
import pytest

import color_model as cm
import color_model_422 as m422
import scan_model as sm
from gpu_support import (PLANES, CBCR, CRCB, S422, UYVY, YUYV, ColorBatch, ColorCall, YccBatch, dev, finish_files, random_planes,     # noqa: F401
                         rows_for, run_ycc, stream, synth_rgb, upload, ycc_file)
from gpu_support import LAYOUTS_422 as YCC_LAYOUTS
from gpu_support import model

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


# W x H                  why
RGB_SIZES = [(1, 1),     # the smallest picture
             (2, 1),     # one whole pixel pair
             (7, 9),     # odd both ways: the last column replicated, edge blocks only
             (17, 33),
             (513, 17),  # cw = 257: one sample past a 32-block tile
             (2049, 3),  # cw = 1025: one sample past a k_chroma_planes_batch workgroup span
             (333, 250)]
YCC_SIZES = [(1, 1), (2, 2),
             (7, 9),     # odd W: the second Y byte of a packed row's last group is never read
             (258, 9),   # cw = 129: Y has an interior tile and an edge tile, chroma an edge tile alone
             (513, 17),  # cw = 257: an interior chroma tile and one sample more
             (640, 16)]  # cw = 320, every row a multiple of 4 bytes: interior tiles on the fast loaders


def want_rgb(oracle, rgb, q):
    return model(oracle, rgb, q, S422)


def want_ycc(oracle, planes, q):
    return ycc_file(oracle, planes, q, S422)


def two_pictures(jpegamd, w, h, seed=0):
    """Photo-like and noise."""
    return [synth_rgb(jpegamd, w, h, 11 + seed, 0), synth_rgb(jpegamd, w, h, 12 + seed, 1)]


def finish_batch(enc, b):
    return finish_files(enc, b)[0]                               # (the canaries behind every output, and Stats.jfif_bytes)


def single(jpegamd, enc, rgb, dev, q=0, bgr=False, bottom_up=False):
    """jpegamd_encode_color_async of one picture at 4:2:2."""
    call = ColorCall(jpegamd, enc, rgb, dev, S422, quality=q, bgr=bgr, bottom_up=bottom_up)
    enc.finish()
    got, intact = call.result()
    assert intact
    return got


# ---- 1. RGB -> 4:2:2 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", RGB_SIZES)
def test_rgb_at_422_is_the_model_file(jpegamd, oracle, dev, w, h):
    rgbs = two_pictures(jpegamd, w, h) + [synth_rgb(jpegamd, w, h, 13, 0, 1)]
    qualities = (0, 50, 10, 100) if (w, h) in ((17, 33), (513, 17)) else (0,)
    enc = jpegamd.Encoder(w, rows_for(3, h))
    for q in qualities:
        want = [want_rgb(oracle, r, q) for r in rgbs]
        if q in (0, 50):
            assert want_rgb(oracle, rgbs[0], 0) == want_rgb(oracle, rgbs[0], 50)          # quality 0 means 50
        for k in range(2):
            assert single(jpegamd, enc, rgbs[k], dev, q) == want[k], (w, h, q, k)
        assert finish_batch(enc, ColorBatch(jpegamd, enc, rgbs[1:2], dev, S422, quality=q)) == want[1:2], (w, h, q)
        assert finish_batch(enc, ColorBatch(jpegamd, enc, rgbs, dev, S422, quality=q)) == want, (w, h, q)
    t = torch.from_numpy(np.stack(rgbs)).to(dev)
    want = [want_rgb(oracle, r, 0) for r in rgbs]
    assert jpegamd.encode_tensor_batch(t, subsampling=S422) == want
    assert jpegamd.encode_tensor(t[1], subsampling=S422) == want[1]
    if (w, h) == (17, 33):
        assert jpegamd.encode_bmp_bytes_color(cm.write_bmp(rgbs[0]), 10, S422) == want_rgb(oracle, rgbs[0], 10)


def test_bgr_and_bottom_up_at_422(jpegamd, oracle, dev):
    w, h = 203, 37
    rgbs = two_pictures(jpegamd, w, h, 5)
    want = [want_rgb(oracle, r, 0) for r in rgbs]
    enc = jpegamd.Encoder(w, rows_for(2, h))
    assert finish_batch(enc, ColorBatch(jpegamd, enc, rgbs, dev, S422, bgr=True)) == want
    assert finish_batch(enc, ColorBatch(jpegamd, enc, rgbs, dev, S422, bottom_up=True)) == want
    assert single(jpegamd, enc, rgbs[0], dev, bgr=True) == want[0]
    assert single(jpegamd, enc, rgbs[1], dev, bottom_up=True) == want[1]
    # a shifted base and a row stride off the dword grid: the planes kernels' byte gather
    assert finish_batch(enc, ColorBatch(jpegamd, enc, rgbs, dev, S422, stride=3 * w + 5, shifts=[1, 2])) == want


@pytest.mark.parametrize("pipeline", ["PIPELINE_PAIR", "PIPELINE_STITCH"])
def test_rgb_at_422_on_both_pipelines(jpegamd, oracle, dev, pipeline):
    w, h = 513, 17
    rgbs = two_pictures(jpegamd, w, h) + [synth_rgb(jpegamd, w, h, 13, 0, 1)]      # (the pictures of the size test: the model files are shared)
    want = [want_rgb(oracle, r, 0) for r in rgbs]
    enc = jpegamd.Encoder(w, rows_for(3, h))
    enc.set_pipeline(getattr(jpegamd, pipeline))
    assert single(jpegamd, enc, rgbs[0], dev) == want[0]
    assert finish_batch(enc, ColorBatch(jpegamd, enc, rgbs, dev, S422)) == want


# ---- 2. every layout gives the packed-RGB file -----------------------------------------------------------------------------------------
def _strided(host: np.ndarray, dev, shift: int, row_stride: int, row_axis: int):
    """`host` as a device view whose first byte lies `shift` bytes into an allocation and whose rows (axis row_axis) are `row_stride`
    bytes apart; every other axis keeps its contiguous order."""
    shape = host.shape
    strides = [int(s) for s in host.strides]
    inner = int(np.prod(shape[row_axis + 1:]))
    assert row_stride >= inner
    strides[row_axis] = row_stride
    for a in range(row_axis - 1, -1, -1):
        strides[a] = strides[a + 1] * shape[a + 1]
    size = shift + sum((n - 1) * s for n, s in zip(shape, strides)) + 1
    buf = torch.zeros(size + 16, dtype=torch.uint8, device=dev)
    view = buf.as_strided(shape, strides, shift)
    view.copy_(torch.from_numpy(host).to(dev))
    return view


@pytest.mark.parametrize("w,h", [(17, 33), (513, 17)])
def test_every_layout_gives_the_packed_rgb_file_at_422(jpegamd, oracle, dev, w, h):
    rgbs = two_pictures(jpegamd, w, h) + [synth_rgb(jpegamd, w, h, 13, 0, 1)]
    want = [want_rgb(oracle, r, 0) for r in rgbs]
    hwc = np.stack(rgbs)                                          # [N, H, W, 3]
    x = np.random.default_rng(w).integers(0, 256, hwc.shape[:3] + (1,), np.uint8)
    sources = {"hwc": (hwc, 3 * w, 1), "chw": (np.ascontiguousarray(hwc.transpose(0, 3, 1, 2)), w, 2),       # (samples, row bytes, row axis)
               "rgba": (np.concatenate([hwc, x], axis=3), 4 * w, 1), "bgra": (np.concatenate([hwc[..., ::-1], x], axis=3), 4 * w, 1)}
    for layout, (host, row, axis) in sources.items():
        aligned = (row + 3) // 4 * 4
        for shift, stride in ((0, aligned), (1, aligned), (0, aligned + 3), (1, row + (1 if row % 4 != 3 else 2))):
            assert (shift % 4, stride % 4) != (0, 0) or (shift, stride) == (0, aligned)
            t = _strided(host, dev, shift, stride, axis)
            assert t.data_ptr() % 4 == shift
            assert jpegamd.encode_tensor_batch(t, subsampling=S422, layout=layout) == want, (layout, shift, stride)
        assert jpegamd.encode_tensor(_strided(host[1], dev, 1, aligned + 1, axis - 1), subsampling=S422, layout=layout) == want[1], layout


# ---- 3. the YCbCr entry -----------------------------------------------------------------------------------------------------------------
def test_the_rgb_paths_own_planes_give_the_rgb_paths_file_at_422(jpegamd, oracle, dev):
    w, h = 513, 17
    rgbs = two_pictures(jpegamd, w, h) + [synth_rgb(jpegamd, w, h, 13, 0, 1)]
    want = [want_rgb(oracle, r, 0) for r in rgbs]
    enc = jpegamd.Encoder(w, rows_for(3, h))
    assert finish_batch(enc, ColorBatch(jpegamd, enc, rgbs, dev, S422)) == want      # what the colour path writes
    planes = [sm.planes_of(r, S422) for r in rgbs]
    for layout in YCC_LAYOUTS:
        assert run_ycc(jpegamd, enc, planes, dev, S422, layout) == want, layout


@pytest.mark.parametrize("w,h", YCC_SIZES)
def test_every_ycbcr_layout_gives_the_file_by_definition(jpegamd, oracle, dev, w, h):
    planes = [random_planes(w, h, S422, 1000 * w + h + k) for k in range(2)]
    enc = jpegamd.Encoder(w, rows_for(2, h))
    for q in ((0, 10, 100) if (w, h) in ((7, 9), (513, 17)) else (0,)):
        want = [want_ycc(oracle, p, q) for p in planes]
        for layout in YCC_LAYOUTS:
            assert run_ycc(jpegamd, enc, planes, dev, S422, layout, quality=q) == want, (w, h, q, layout)
    if w % 2:                                                     # another poison value in the byte that is never read: the same files
        want = [want_ycc(oracle, p, 0) for p in planes]
        cw = (w + 1) // 2
        for layout, order in ((YUYV, "yuyv"), (UYVY, "uyvy")):
            ups = [upload(m422.pack_yuyv(*p, order, poison=0xC3), dev, 4 * cw) for p in planes]
            imgs = [jpegamd.Encoder.ycbcr_image(ptr, 0, 0, w, h, 4 * cw, 0, layout, 0) for _, ptr in ups]
            cap = jpegamd.max_jfif_bytes_color(w, h, S422)
            outs = torch.zeros((2, cap), dtype=torch.uint8, device=dev)
            sizes = torch.zeros(2, dtype=torch.int64, device=dev)
            enc.encode_ycbcr_batch_async(imgs, S422, [outs[i].data_ptr() for i in range(2)], cap, [sizes.data_ptr() + 8 * i for i in range(2)],
                                         stream())
            enc.finish()
            assert [bytes(outs[i, :int(sizes[i])].cpu().numpy()) for i in range(2)] == want, layout


@pytest.mark.parametrize("pipeline", ["PIPELINE_PAIR", "PIPELINE_STITCH"])
@pytest.mark.parametrize("count", [1, 3, 5])
def test_an_odd_chroma_group_starts_a_launch_on_a_cr_plane(jpegamd, oracle, dev, count, pipeline):
    """A context of exactly `count` pictures' rows: a 640-wide picture has three tiles per block row and its 320-wide plane two, so
    the context holds 1.5 x count planes (rounded down) -- the 2 x count planes go as two launches of `count`, and for odd counts the
    second launch starts on a Cr plane."""
    w, h = 640, 16
    pipe = getattr(jpegamd, pipeline)
    group, launches, _, _ = jpegamd._chroma_groups(w, rows_for(count, h), w, h, count, S422, pipe)
    assert group % 2 == 1 and launches == 2 and group == count, (group, launches)
    enc = jpegamd.Encoder(w, rows_for(count, h))
    enc.set_pipeline(pipe)
    planes = [random_planes(w, h, S422, 90 + k) for k in range(count)]
    want = [want_ycc(oracle, p, 0) for p in planes]
    assert len(set(want)) == count                               # every picture distinct
    for layout in YCC_LAYOUTS:
        assert run_ycc(jpegamd, enc, planes, dev, S422, layout) == want, (count, layout)


@pytest.mark.parametrize("layout", [YUYV, UYVY])
def test_packed_planes_off_the_dword_grid(jpegamd, oracle, dev, layout):
    w, h = 513, 17
    row = 4 * ((w + 1) // 2)
    planes = [random_planes(w, h, S422, 70 + k) for k in range(3)]
    want = [want_ycc(oracle, p, 0) for p in planes]
    enc = jpegamd.Encoder(w, rows_for(3, h))
    cases = [dict(y_stride=row + 8),                              # aligned, rows apart: the fast loaders
             dict(y_shifts=[0, 1, 0]),                            # one picture's base off the grid: the gather for all
             dict(y_shifts=[2, 2, 2], y_stride=row + 4),
             dict(y_shifts=[3, 0, 1]),
             dict(y_stride=row + 1), dict(y_stride=row + 2), dict(y_stride=row + 3),     # a stride off the grid
             dict(y_shifts=[1, 1, 1], y_stride=row + 3)]
    for kw in cases:
        assert run_ycc(jpegamd, enc, planes, dev, S422, layout, **kw) == want, (layout, kw)


def test_i422_and_nv16_off_the_dword_grid(jpegamd, oracle, dev):
    w, h = 513, 17
    cw = (w + 1) // 2
    planes = [random_planes(w, h, S422, 70 + k) for k in range(3)]
    want = [want_ycc(oracle, p, 0) for p in planes]
    enc = jpegamd.Encoder(w, rows_for(3, h))
    for layout, row in ((PLANES, cw), (CBCR, 2 * cw), (CRCB, 2 * cw)):
        aligned = (row + 3) // 4 * 4
        for kw in (dict(y_stride=w + 3, c_stride=aligned), dict(y_stride=w + 3, c_stride=aligned, c_shifts=[0, 0, 1]),
                   dict(y_stride=w + 3, c_stride=aligned + 1), dict(y_stride=w + 2, c_stride=aligned, y_shifts=[0, 3, 0])):
            assert run_ycc(jpegamd, enc, planes, dev, S422, layout, **kw) == want, (layout, kw)


def test_encode_yuyv_batch(jpegamd, oracle, dev):
    w, h = 48, 16
    n = jpegamd.MAX_BATCH + 1                                     # two calls
    rng = np.random.default_rng(8)
    host = rng.integers(0, 256, (2 * n, h, w, 2), np.uint8)
    frames = torch.from_numpy(host).to(dev)

    def want(i, order):
        iy, (icb, icr) = (0, (1, 3)) if order == "yuyv" else (1, (0, 2))
        groups = host[i].reshape(h, w // 2, 4)
        return want_ycc(oracle, (np.ascontiguousarray(host[i, :, :, iy]), np.ascontiguousarray(groups[:, :, icb]),
                                 np.ascontiguousarray(groups[:, :, icr])), 0)

    assert jpegamd.encode_yuyv_batch(frames[::2]) == [want(2 * i, "yuyv") for i in range(n)]          # a strided view, 33 pictures
    assert jpegamd.encode_yuyv_batch(frames[1:4], order="uyvy") == [want(i, "uyvy") for i in (1, 2, 3)]
    crop = frames[:2, 3:3 + 9, 6:6 + 26]                          # strided rows; the first byte of a row off the dword grid by 12: aligned
    odd = frames[:2, :, 1:1 + 26]                                 # ... and by 2: the gather
    for view in (crop, odd):
        files = jpegamd.encode_yuyv_batch(view, quality=90)
        hv = view.cpu().numpy()
        for i in range(2):
            g = np.ascontiguousarray(hv[i]).reshape(hv.shape[1], 13, 4)
            assert files[i] == want_ycc(oracle, (np.ascontiguousarray(hv[i, :, :, 0]), np.ascontiguousarray(g[:, :, 1]),
                                                 np.ascontiguousarray(g[:, :, 3])), 90)
    # I422 and NV16 through encode_ycbcr_batch: the same samples, the same files
    groups = host[:3].reshape(3, h, w // 2, 4)
    y = torch.from_numpy(np.ascontiguousarray(host[:3, :, :, 0])).to(dev)
    cb, cr = (torch.from_numpy(np.ascontiguousarray(groups[..., k])).to(dev) for k in (1, 3))
    files = [want(i, "yuyv") for i in range(3)]
    assert jpegamd.encode_ycbcr_batch(y, cb, cr, subsampling=S422) == files
    assert jpegamd.encode_ycbcr_batch(y, torch.stack([cb, cr], dim=3), subsampling=S422) == files
    assert jpegamd.encode_ycbcr_batch(y, torch.stack([cr, cb], dim=3), subsampling=S422, order="crcb") == files


# ---- 4. capacity ------------------------------------------------------------------------------------------------------------------------
def test_one_picture_of_a_422_batch_one_byte_short(jpegamd, oracle, dev):
    w, h = 160, 48
    rgbs = [synth_rgb(jpegamd, w, h, 7, 0), synth_rgb(jpegamd, w, h, 9, 1), synth_rgb(jpegamd, w, h, 8, 0)]     # the noise picture is the large one
    exp = [want_rgb(oracle, r, 0) for r in rgbs]
    cap = len(exp[1]) - 1
    assert cap > max(len(exp[0]), len(exp[2]))
    enc = jpegamd.Encoder(w, rows_for(3, h))
    planes = [sm.planes_of(r, S422) for r in rgbs]
    jobs = [lambda c: ColorBatch(jpegamd, enc, rgbs, dev, S422, cap=c), lambda c: YccBatch(jpegamd, enc, planes, dev, S422, YUYV, cap=c),
            lambda c: YccBatch(jpegamd, enc, planes, dev, S422, PLANES, cap=c)]
    for k, job in enumerate(jobs):
        b = job(cap)
        with pytest.raises(jpegamd.JpegAmdError) as err:
            enc.finish()
        assert err.value.code == -8
        res = b.results()
        assert all(ok for _, ok in res)                          # nothing behind any capacity
        assert int(b.sizes[1].item()) == 0
        assert [res[0][0], res[2][0]] == [exp[0], exp[2]], k
        assert finish_batch(enc, job(cap + 1)) == exp, k         # the exact capacity fits
