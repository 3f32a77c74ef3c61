"""YCbCr input (jpegamd_encode_ycbcr_batch_async, encode_ycbcr_batch) through the C-ABI into the HIP kernels, byte for byte against
the file the header defines: the colour prefix, the oracle's grayscale scan of the Y plane, and the chroma pipeline of
tests/color_model.py over the Cb and Cr planes exactly as given.  Every test needs an MI355X."""
from __future__ import annotations

import numpy as np
import pytest

import color_model as cm
import scan_model as sm
from gpu_support import (CBCR, CRCB, LAYOUTS, PLANES, S420, S444, WIDE_STRIDE, ColorBatch, YccBatch, chroma_dims, dev, model, pictures,     # noqa: F401
                         random_planes, rows_for, run_ycc, smooth_planes, stream, upload)
from gpu_support import ycc_file as expected

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


# W x H                 why
SIZES = [(1, 1),        # the smallest picture
         (16, 16),      # one chroma block
         (17, 9),       # odd both ways; chroma is 9 x 5 with edge blocks only
         (48, 32),      # an interior partial tile
         (522, 38),     # 4:2:0 chroma is 261 wide: a full 32-block interior tile plus an edge tile, with a bottom edge
         (1030, 24)]    # three chroma tiles per row


# ---- 1. sizes, subsamplings, layouts, qualities -----------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", [S444, S420])
@pytest.mark.parametrize("w,h", SIZES)
def test_every_layout_gives_the_file_by_definition(jpegamd, oracle, dev, w, h, sub):
    planes = [random_planes(w, h, sub, 1000 * w + 10 * h + sub + k) for k in range(2)]
    enc = jpegamd.Encoder(w, rows_for(2, h))
    for q in (0, 10, 90):
        want = [expected(oracle, p, q, sub) for p in planes]
        for layout in LAYOUTS:
            assert run_ycc(jpegamd, enc, planes, dev, sub, layout, quality=q) == want, (w, h, sub, q, layout)


# ---- 2. the identity with the RGB path ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", [S444, S420])
def test_the_rgb_paths_own_planes_give_the_rgb_paths_file(jpegamd, dev, sub):
    w, h = 522, 38
    rgbs = [cm.read_bmp_rgb(jpegamd.synth_bmp(w, h, 5 + k, k, 0)) for k in range(2)]
    enc = jpegamd.Encoder(w, rows_for(2, h))
    b = ColorBatch(jpegamd, enc, rgbs, dev, sub)
    enc.finish()
    want = [f for f, _ in b.results()]
    assert all(len(f) > 700 for f in want)
    planes = [sm.planes_of(rgb, sub) for rgb in rgbs]
    for layout in LAYOUTS:
        assert run_ycc(jpegamd, enc, planes, dev, sub, layout) == want, (sub, layout)


# ---- 3. extreme planes -------------------------------------------------------------------------------------------------------------
def test_extreme_planes_at_quality_100(jpegamd, oracle, dev):
    w, h = 264, 24                                               # a full interior tile and an edge tile per block row
    sub = S444
    board = ((np.indices((h, w)).sum(0) % 2) * 255).astype(np.uint8)
    noise = np.random.default_rng(3).integers(0, 256, (3, h, w), np.uint8)
    planes = [(np.zeros((h, w), np.uint8),) * 3, (np.full((h, w), 255, np.uint8),) * 3, (board, board, 255 - board),
              (noise[0], noise[1], noise[2])]
    enc = jpegamd.Encoder(w, rows_for(len(planes), h))
    want = [expected(oracle, p, 100, sub) for p in planes]
    for layout in LAYOUTS:
        assert run_ycc(jpegamd, enc, planes, dev, sub, layout, quality=100) == want, layout
    # the same at 4:2:0: the chroma planes cut to 132 x 12
    sub = S420
    planes = [(y, cb[:12, :132].copy(), cr[:12, :132].copy()) for y, cb, cr in planes]
    want = [expected(oracle, p, 100, sub) for p in planes]
    for layout in (PLANES, CRCB):
        assert run_ycc(jpegamd, enc, planes, dev, sub, layout, quality=100) == want, layout


# ---- 4. alignment and strides ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [1, 2, 3])
def test_shifted_pointers_and_odd_strides(jpegamd, oracle, dev, shift):
    w, h = 522, 38
    enc = jpegamd.Encoder(w, rows_for(3, h))
    for sub in (S420, S444):
        cw, _ = chroma_dims(w, h, sub)
        planes = [random_planes(w, h, sub, 7 * shift + k) for k in range(3)]
        want = [expected(oracle, p, 0, sub) for p in planes]
        for layout in LAYOUTS:
            row = cw if layout == PLANES else 2 * cw
            aligned = -row % 4 + row                              # the next multiple of 4
            assert run_ycc(jpegamd, enc, planes, dev, sub, layout, y_stride=w + 2, c_stride=aligned) == want     # the packed, aligned case
            cases = [dict(y_shifts=[0, shift, 0], y_stride=w + 2, c_stride=aligned),                 # one y off a dword boundary
                     dict(c_shifts=[0, 0, shift], y_stride=w + 2, c_stride=aligned),                 # one cb / cr / pair plane
                     dict(y_shifts=[shift] * 3, c_shifts=[shift] * 3, y_stride=w + 2, c_stride=aligned),
                     dict(y_stride=w + shift, c_stride=aligned),                                     # strides off multiples of 4
                     dict(y_stride=w + 2, c_stride=aligned + shift),
                     dict(y_stride=w + 2, c_stride=aligned + 4096)]                                  # rows far apart
            for kw in cases:
                assert run_ycc(jpegamd, enc, planes, dev, sub, layout, **kw) == want, (shift, sub, layout, kw)


def test_strides_of_16_mib_take_the_gather(jpegamd, oracle, dev):
    w, h = 17, 9
    enc = jpegamd.Encoder(w, rows_for(1, h))
    for sub, layout in ((S420, CBCR), (S444, PLANES)):
        planes = [random_planes(w, h, sub, 77)]
        want = [expected(oracle, planes[0], 0, sub)]
        assert run_ycc(jpegamd, enc, planes, dev, sub, layout, c_stride=WIDE_STRIDE) == want, (sub, layout)
    assert run_ycc(jpegamd, enc, planes, dev, S444, PLANES, y_stride=WIDE_STRIDE) == want


def test_strided_views(jpegamd, oracle, dev):
    """Crops of larger tensors: rows and pictures strided, the first sample of a row off a dword boundary."""
    w, h, n = 522, 38, 3
    rng = np.random.default_rng(11)
    big_y = torch.from_numpy(rng.integers(0, 256, (2 * n, h + 6, w + 10), np.uint8)).to(dev)
    for sub in (S420, S444):
        cw, ch = chroma_dims(w, h, sub)
        big_c = torch.from_numpy(rng.integers(0, 256, (2 * n, 2, ch + 3, cw + 7), np.uint8)).to(dev)
        big_p = torch.from_numpy(rng.integers(0, 256, (2 * n, ch + 3, cw + 5, 2), np.uint8)).to(dev)
        y = big_y[1::2, 3:3 + h, 5:5 + w]
        cb, cr = big_c[1::2, 0, 1:1 + ch, 3:3 + cw], big_c[1::2, 1, 1:1 + ch, 3:3 + cw]
        pairs = big_p[::2, 2:2 + ch, 1:1 + cw]
        files = jpegamd.encode_ycbcr_batch(y, cb, cr, subsampling=sub)
        assert files == [expected(oracle, (y[i].cpu().numpy(), cb[i].cpu().numpy(), cr[i].cpu().numpy()), 0, sub) for i in range(n)], sub
        for order, (c0, c1) in (("cbcr", (0, 1)), ("crcb", (1, 0))):
            files = jpegamd.encode_ycbcr_batch(y, pairs, quality=90, subsampling=sub, order=order)
            host = pairs.cpu().numpy()
            assert files == [expected(oracle, (y[i].cpu().numpy(), np.ascontiguousarray(host[i, :, :, c0]),
                                               np.ascontiguousarray(host[i, :, :, c1])), 90, sub) for i in range(n)], (sub, order)


# ---- 5. counts, and a chroma launch that starts on a Cr plane -------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 2, 5, 32])
def test_counts(jpegamd, oracle, dev, count):
    w, h = 48, 32
    enc = jpegamd.Encoder(w, rows_for(count, h))
    for sub, layout in ((S420, CBCR), (S444, CRCB), (S420, PLANES)):
        planes = [random_planes(w, h, sub, 31 * count + k) for k in range(count)]
        want = [expected(oracle, p, 0, sub) for p in planes]
        assert len(set(want)) == count
        assert run_ycc(jpegamd, enc, planes, dev, sub, layout) == want, (count, sub, layout)


@pytest.mark.parametrize("pipeline", ["PIPELINE_PAIR", "PIPELINE_STITCH"])
def test_an_odd_chroma_group_starts_a_launch_on_a_cr_plane(jpegamd, oracle, dev, pipeline):
    """4:4:4, three pictures, a context of exactly three pictures' rows: the six chroma planes go as two launches of three, so
    the second launch starts on picture 1's Cr plane."""
    w, h, count = 522, 38, 3
    pipe = getattr(jpegamd, pipeline)
    group, launches, _, _ = jpegamd._chroma_groups(w, rows_for(count, h), w, h, count, S444, pipe)
    assert group % 2 == 1 and launches > 1 and group * launches >= 2 * count, (group, launches)
    enc = jpegamd.Encoder(w, rows_for(count, h))
    enc.set_pipeline(pipe)
    planes = [random_planes(w, h, S444, 90 + k) for k in range(count)]
    want = [expected(oracle, p, 0, S444) for p in planes]
    assert len(set(want)) == count                               # every picture distinct
    for layout in LAYOUTS:
        assert run_ycc(jpegamd, enc, planes, dev, S444, layout) == want, layout


# ---- 6. pipelines ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", ["PIPELINE_PAIR", "PIPELINE_STITCH"])
def test_pipelines(jpegamd, oracle, dev, pipeline):
    w, h, count = 522, 38, 4
    enc = jpegamd.Encoder(w, rows_for(count, h))
    enc.set_pipeline(getattr(jpegamd, pipeline))
    enc.set_profiling(2)
    for sub in (S420, S444):
        planes = [random_planes(w, h, sub, 50 + k) for k in range(count)]
        want = [expected(oracle, p, 0, sub) for p in planes]
        for layout in LAYOUTS:
            b = YccBatch(jpegamd, enc, planes, dev, sub, layout)
            st = enc.finish()
            assert [f for f, _ in b.results()] == want, (pipeline, sub, layout)
            assert st.entropy_bits > 0 and 0 < st.ns_total < 50_000_000       # the profiling ring spans the call


# ---- 7. capacity -------------------------------------------------------------------------------------------------------------------
def test_one_picture_of_a_ycbcr_batch_one_byte_short(jpegamd, oracle, dev):
    w, h = 160, 96
    enc = jpegamd.Encoder(w, rows_for(4, h))
    for sub in (S420, S444):
        planes = [smooth_planes(w, h, sub, 7), random_planes(w, h, sub, 9), smooth_planes(w, h, sub, 8), smooth_planes(w, h, sub, 6)]
        exp = [expected(oracle, p, 0, sub) for p in planes]
        cap = len(exp[1]) - 1                                    # one byte short for the noise picture alone
        assert cap > max(len(exp[k]) for k in (0, 2, 3))
        for layout in (PLANES, CBCR):
            b = YccBatch(jpegamd, enc, planes, dev, sub, layout, cap=cap)
            with pytest.raises(jpegamd.JpegAmdError) as err:
                enc.finish()
            assert err.value.code == -8
            res = b.results()
            assert all(ok for _, ok in res)                      # nothing behind any capacity
            assert int(b.sizes[1].item()) == 0
            assert [res[k][0] for k in (0, 2, 3)] == [exp[k] for k in (0, 2, 3)], (sub, layout)
            assert run_ycc(jpegamd, enc, planes, dev, sub, layout, cap=cap + 1) == exp, (sub, layout)     # the exact capacity fits


# ---- 8. one context, calls queued back to back ---------------------------------------------------------------------------------------
def test_one_context_interleaves_rgb_gray_and_ycbcr(jpegamd, oracle, dev):
    w, h = 96, 64
    enc = jpegamd.Encoder(2 * w, rows_for(4, h))
    keep, checks = [], []

    def ycc(planes, sub, layout, q=0):
        b = YccBatch(jpegamd, enc, planes, dev, sub, layout, quality=q)
        keep.append(b)
        for k, p in enumerate(planes):
            checks.append(((lambda b=b, k=k: b.results()[k][0]), expected(oracle, p, q, sub)))

    def rgb_batch(rgbs, sub, q=0):
        b = ColorBatch(jpegamd, enc, rgbs, dev, sub, quality=q)
        keep.append(b)
        for k, r in enumerate(rgbs):
            checks.append(((lambda b=b, k=k: b.results()[k][0]), model(oracle, r, q, sub)))

    def gray(plane, q=0):
        hh, ww = plane.shape
        t, ptr = upload(plane, dev, ww)
        cap = jpegamd.max_jfif_bytes(ww, hh)
        out = torch.empty(cap, dtype=torch.uint8, device=dev)
        size = torch.zeros(1, dtype=torch.int64, device=dev)
        enc.encode_async(jpegamd.Encoder.image(ptr, ww, hh, ww, False, jpegamd.ORDER_GRAY, q), out.data_ptr(), cap, size.data_ptr(),
                         True, stream())
        keep.append((t, out, size))
        bmp = cm.write_bmp(np.stack([plane] * 3, axis=2))
        checks.append(((lambda: bytes(out[:int(size.item())].cpu().numpy())), oracle.encode_bmp(bmp, quality=q) if q else oracle.encode_bmp(bmp)))

    small = pictures(jpegamd, w, h, 4, seed=41)
    ycc([random_planes(33, 17, S420, k) for k in range(2)], S420, CBCR)             # the context's first colour call
    rgb_batch(small, S420)                                                          # allocates the plane scratch
    ycc([random_planes(w, h, S444, 10 + k) for k in range(4)], S444, CRCB)          # larger scan slots: grown behind queued work
    gray(random_planes(w, h, S444, 3)[0])
    ycc([random_planes(2 * w, h, S420, 20 + k) for k in range(2)], S420, PLANES, 90)    # another size, a quality change
    rgb_batch(small[:2], S444, 90)
    ycc([random_planes(2 * w, h, S444, 30 + k) for k in range(2)], S444, CBCR, 90)
    gray(random_planes(2 * w, h, S444, 4)[0], 10)
    ycc([random_planes(17, 9, S420, 40)], S420, CRCB, 10)
    rgb_batch(small[1:], S420, 10)
    enc.finish()
    for i, (got, want) in enumerate(checks):
        assert got() == want, i


# ---- 9. encode_ycbcr_batch -----------------------------------------------------------------------------------------------------------
def test_encode_ycbcr_batch_on_nv12_frames(jpegamd, oracle, dev):
    w, h, n = 48, 32, 40
    host = np.random.default_rng(5).integers(0, 256, (n, 3 * h // 2, w), np.uint8)
    frames = torch.from_numpy(host).to(dev)                       # [N, 3 H / 2, W]: H rows of Y, H / 2 rows of Cb Cr pairs
    y, cbcr = frames[:, :h], frames[:, h:].unflatten(2, (w // 2, 2))
    pairs = host[:, h:].reshape(n, h // 2, w // 2, 2)
    want = [expected(oracle, (host[i, :h], np.ascontiguousarray(pairs[i, :, :, 0]), np.ascontiguousarray(pairs[i, :, :, 1])), 0, S420)
            for i in range(n)]
    assert jpegamd.encode_ycbcr_batch(y, cbcr) == want            # 40 pictures: two calls
    assert jpegamd.encode_ycbcr_batch(y[::2], cbcr[::2]) == want[::2]
    one = frames[3]                                               # one frame, sliced as the docstring shows
    assert jpegamd.encode_ycbcr_batch(one[:h].unsqueeze(0), one[h:].view(h // 2, w // 2, 2).unsqueeze(0)) == [want[3]]
    # the same chroma as two planes, and as NV21
    cb, cr = cbcr[..., 0].contiguous(), cbcr[..., 1].contiguous()
    assert jpegamd.encode_ycbcr_batch(y[:5], cb[:5], cr[:5]) == want[:5]
    assert jpegamd.encode_ycbcr_batch(y[:5], cbcr[:5].flip(3).contiguous(), order="crcb") == want[:5]
