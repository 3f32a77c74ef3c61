"""Limited-range YCbCr input (jpegamd_encode_ycbcr_range_batch_async, sample_range="limited") through the C-ABI into the HIP kernels,
byte for byte against the file the header defines: the full-range file -- the CPU models of tests/color_model.py and
tests/color_model_422.py -- of the planes mapped with numpy by the tables of tests/range_model.py.  Every test needs an MI355X."""
from __future__ import annotations

import numpy as np
import pytest

import range_model as rm
from gpu_support import (CBCR, LAYOUTS, PLANES, S420, S422, S444, WIDE_STRIDE, YUYV, YccBatch, chroma_dims, dev, intact_files,     # noqa: F401
                         random_planes, rows_for, run_ycc, smooth_planes)
from gpu_support import LAYOUTS_422 as YCC_LAYOUTS
from gpu_support import ycc_file as expected

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def run(jpegamd, enc, planes, dev, sub, layout, **kw):
    """A limited-range batch through Encoder, which takes jpegamd_encode_ycbcr_range_batch_async for RANGE_LIMITED alone."""
    return run_ycc(jpegamd, enc, planes, dev, sub, layout, sample_range=jpegamd.RANGE_LIMITED, **kw)


def want(oracle, planes, q, sub):
    """The file by definition: the full-range file of the numpy-mapped planes."""
    return expected(oracle, rm.expand(planes), q, sub)


# ---- 1. every input value ----------------------------------------------------------------------------------------------------------
def test_every_input_value(jpegamd, oracle, dev):
    """16 x 16 at 4:4:4: one block row of two blocks (the edge path), every byte value once in every plane."""
    v = np.arange(256, dtype=np.uint8).reshape(16, 16)
    t = np.ascontiguousarray(v.T)
    planes = [(v, v, v), (t, t, t)]
    enc = jpegamd.Encoder(16, rows_for(2, 16))
    for q in (0, 100):
        files = [want(oracle, p, q, S444) for p in planes]
        assert files[0] != files[1] and files[0] != expected(oracle, planes[0], q, S444)      # (the map changes the file)
        for layout in LAYOUTS:
            assert run(jpegamd, enc, planes, dev, S444, layout, quality=q) == files, (q, layout)


# ---- 2. sizes, subsamplings, layouts, qualities --------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", [S444, S420])
@pytest.mark.parametrize("w,h", [(1, 1), (17, 9), (48, 32), (522, 38)])
def test_sizes(jpegamd, oracle, dev, w, h, sub):
    """Uniform noise over 0 .. 255: about a quarter of the samples clamp.  (522, 38): a full 32-block interior chroma tile plus an
    edge tile at 4:2:0."""
    planes = [random_planes(w, h, sub, 2000 * w + 10 * h + sub + k) for k in range(2)]
    enc = jpegamd.Encoder(w, rows_for(2, h))
    for q in (0, 90):
        files = [want(oracle, p, q, sub) for p in planes]
        for layout in LAYOUTS:
            assert run(jpegamd, enc, planes, dev, sub, layout, quality=q) == files, (w, h, sub, q, layout)


# ---- 3. 4:2:2 and packed frames: the pair loader with the luma tables, and the quad loader ------------------------------------------
@pytest.mark.parametrize("w,h", [(522, 38), (18, 9)])
def test_422_and_packed(jpegamd, oracle, dev, w, h):
    planes = [random_planes(w, h, S422, 3000 * w + h + k) for k in range(2)]
    files = [expected(oracle, rm.expand(p), 0, S422) for p in planes]
    enc = jpegamd.Encoder(w, rows_for(2, h))
    for layout in YCC_LAYOUTS:                                    # I422, NV16, NV61, YUYV, UYVY
        assert run(jpegamd, enc, planes, dev, S422, layout) == files, (w, h, layout)


# ---- 4. loader paths ---------------------------------------------------------------------------------------------------------------
def test_loader_paths_give_one_file(jpegamd, oracle, dev):
    """Dword loaders, the clamped byte gather (a shifted plane, a stride off the grid) and 64-bit addresses (a stride of 2^24 and
    more) end in the same fragment registers: one map behind them, one file."""
    w, h = 522, 38
    enc = jpegamd.Encoder(w, rows_for(3, h))
    for sub in (S420, S444):
        cw, _ = chroma_dims(w, h, sub)
        planes = [random_planes(w, h, sub, 17 + k) for k in range(3)]
        files = [want(oracle, p, 0, sub) for p in planes]
        for layout in LAYOUTS:
            row = cw if layout == PLANES else 2 * cw
            aligned = -row % 4 + row
            assert run(jpegamd, enc, planes, dev, sub, layout, y_stride=w + 2, c_stride=aligned) == files       # the aligned case
            for kw in (dict(y_shifts=[0, 1, 0], y_stride=w + 2, c_stride=aligned),       # one Y plane off a dword boundary
                       dict(c_shifts=[0, 0, 1], y_stride=w + 2, c_stride=aligned),       # one chroma plane
                       dict(y_stride=w + 1, c_stride=aligned),                           # strides off multiples of 4
                       dict(y_stride=w + 2, c_stride=aligned + 3)):
                assert run(jpegamd, enc, planes, dev, sub, layout, **kw) == files, (sub, layout, kw)
    w, h = 17, 9
    enc = jpegamd.Encoder(w, rows_for(1, h))
    planes = [random_planes(w, h, S420, 78)]
    assert run(jpegamd, enc, planes, dev, S420, CBCR, c_stride=WIDE_STRIDE) == [want(oracle, planes[0], 0, S420)]


# ---- 5. both pipelines, and a chroma launch that starts on a Cr plane ----------------------------------------------------------------
@pytest.mark.parametrize("pipeline", ["PIPELINE_PAIR", "PIPELINE_STITCH"])
def test_pipelines_with_a_launch_that_starts_on_a_cr_plane(jpegamd, oracle, dev, pipeline):
    w, h, count = 522, 38, 3
    pipe = getattr(jpegamd, pipeline)
    group, launches, _, _ = jpegamd._chroma_groups(w, rows_for(count, h), w, h, count, S444, pipe)
    assert group % 2 == 1 and launches > 1, (group, launches)
    enc = jpegamd.Encoder(w, rows_for(count, h))
    enc.set_pipeline(pipe)
    planes = [random_planes(w, h, S444, 190 + k) for k in range(count)]
    files = [want(oracle, p, 0, S444) for p in planes]
    assert len(set(files)) == count
    for layout in LAYOUTS:
        assert run(jpegamd, enc, planes, dev, S444, layout) == files, layout


# ---- 6. full stays full ------------------------------------------------------------------------------------------------------------
def test_full_range_stays_full_range_between_limited_calls(jpegamd, oracle, dev):
    """One context, three calls queued without a finish in between: limited, RANGE_FULL through the new entry, the old entry."""
    w, h = 522, 38
    enc = jpegamd.Encoder(w, rows_for(2, h))
    for sub, layout in ((S420, CBCR), (S444, PLANES)):
        planes = [random_planes(w, h, sub, 300 + sub + k) for k in range(2)]
        a = YccBatch(jpegamd, enc, planes, dev, sub, layout, sample_range=jpegamd.RANGE_LIMITED)
        b = YccBatch(jpegamd, enc, planes, dev, sub, layout, sample_range=jpegamd.RANGE_FULL, entry="range")
        c = YccBatch(jpegamd, enc, planes, dev, sub, layout)
        enc.finish()
        fa, fb, fc = intact_files(a), intact_files(b), intact_files(c)
        full = [expected(oracle, p, 0, sub) for p in planes]
        assert fb == full and fc == full, (sub, layout)
        assert fa == [want(oracle, p, 0, sub) for p in planes], (sub, layout)
        assert fa != full
    # the 4:2:2 entry the same way, from a packed plane
    planes = [random_planes(w, h, S422, 310 + k) for k in range(2)]
    a = YccBatch(jpegamd, enc, planes, dev, S422, YUYV, sample_range=jpegamd.RANGE_LIMITED)
    b = YccBatch(jpegamd, enc, planes, dev, S422, YUYV, sample_range=jpegamd.RANGE_FULL, entry="range")
    c = YccBatch(jpegamd, enc, planes, dev, S422, YUYV)
    enc.finish()
    full = [expected(oracle, p, 0, S422) for p in planes]
    assert [f for f, _ in b.results()] == full and [f for f, _ in c.results()] == full
    assert [f for f, _ in a.results()] == [expected(oracle, rm.expand(p), 0, S422) for p in planes]


# ---- 7. planes that are limited range already: the tensor entries ---------------------------------------------------------------------
def test_tensor_entries_on_nominal_range_planes(jpegamd, oracle, dev):
    """Samples inside the nominal ranges: the limited file is the full-range file of the planes mapped with torch on the device."""
    w, h, n = 48, 32, jpegamd.MAX_BATCH + 1                       # 33 pictures: the call splits
    rng = np.random.default_rng(21)
    hy = rng.integers(16, 236, (n, h, w), np.uint8)
    hc = rng.integers(16, 241, (n, h // 2, w // 2, 2), np.uint8)
    ylut, clut = torch.from_numpy(rm.luma_table()).to(dev), torch.from_numpy(rm.chroma_table()).to(dev)
    y, cbcr = torch.from_numpy(hy).to(dev), torch.from_numpy(hc).to(dev)
    files = jpegamd.encode_ycbcr_batch(y, cbcr, sample_range="limited")
    assert files == jpegamd.encode_ycbcr_batch(ylut[y.long()], clut[cbcr.long()])
    assert files == jpegamd.encode_ycbcr_batch(ylut[y.long()], clut[cbcr.long()], sample_range="full")
    for i in (0, n - 1):
        assert files[i] == want(oracle, (hy[i], np.ascontiguousarray(hc[i, :, :, 0]), np.ascontiguousarray(hc[i, :, :, 1])), 0, S420)
    assert files[:3] != jpegamd.encode_ycbcr_batch(y[:3], cbcr[:3])
    cb, cr = cbcr[:3, :, :, 0].contiguous(), cbcr[:3, :, :, 1].contiguous()
    assert jpegamd.encode_ycbcr_batch(y[:3], cb, cr, sample_range="limited") == files[:3]
    # packed frames: Y in byte 0 of every pixel, Cb / Cr in byte 1
    frames = torch.stack([torch.from_numpy(rng.integers(16, 236, (3, h, w), np.uint8)), torch.from_numpy(rng.integers(16, 241, (3, h, w), np.uint8))], dim=3).to(dev)
    mapped = torch.stack([ylut[frames[..., 0].long()], clut[frames[..., 1].long()]], dim=3)
    got = jpegamd.encode_yuyv_batch(frames, sample_range="limited")
    assert got == jpegamd.encode_yuyv_batch(mapped) and got != jpegamd.encode_yuyv_batch(frames)
    swapped, swapped_mapped = frames.flip(3).contiguous(), mapped.flip(3).contiguous()
    assert jpegamd.encode_yuyv_batch(swapped, order="uyvy", sample_range="limited") == got
    assert jpegamd.encode_yuyv_batch(swapped_mapped, order="uyvy") == got
    fh = frames[0].cpu().numpy().reshape(h, w // 2, 4)
    assert got[0] == expected(oracle, rm.expand((np.ascontiguousarray(frames[0, :, :, 0].cpu().numpy()), np.ascontiguousarray(fh[:, :, 1]),
                                                 np.ascontiguousarray(fh[:, :, 3]))), 0, S422)


# ---- 8. capacity -------------------------------------------------------------------------------------------------------------------
def test_one_picture_of_a_limited_batch_one_byte_short(jpegamd, oracle, dev):
    w, h = 160, 96
    enc = jpegamd.Encoder(w, rows_for(4, h))
    for sub, layout in ((S420, CBCR), (S444, PLANES)):
        planes = [smooth_planes(w, h, sub, 7), random_planes(w, h, sub, 9), smooth_planes(w, h, sub, 8), smooth_planes(w, h, sub, 6)]
        exp = [want(oracle, p, 0, sub) for p in planes]
        cap = len(exp[1]) - 1                                    # one byte short for the noise picture alone
        assert cap > max(len(exp[k]) for k in (0, 2, 3))
        b = YccBatch(jpegamd, enc, planes, dev, sub, layout, cap=cap, sample_range=jpegamd.RANGE_LIMITED)
        with pytest.raises(jpegamd.JpegAmdError) as err:
            enc.finish()
        assert err.value.code == -8
        res = b.results()
        assert all(ok for _, ok in res)                          # the canaries: nothing behind any capacity
        assert int(b.sizes[1].item()) == 0
        assert [res[k][0] for k in (0, 2, 3)] == [exp[k] for k in (0, 2, 3)], (sub, layout)
        assert run(jpegamd, enc, planes, dev, sub, layout, cap=cap + 1) == exp, (sub, layout)     # the exact capacity fits
