"""Colour batches (jpegamd_encode_color_batch_async, encode_tensor_batch) through the C-ABI into the HIP kernels, byte for byte:
small and medium pictures against the CPU model of tests/color_model.py, the largest against jpegamd_encode_color_async (which the
colour suites pin to the model at those sizes).  Every test needs an MI355X."""
from __future__ import annotations

import numpy as np
import pytest

import color_model as cm
from gpu_support import (S420, S444, WIDE_STRIDE, ColorBatch, dev, finish_files, model, pictures, rows_for, stored_rows, stream,     # noqa: F401
                         synth_rgb, upload)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def single(jpegamd, enc, rgb, dev, sub, quality=0):
    """jpegamd_encode_color_async of one picture (RGB, top-down) -> (file, stats)."""
    h, w, _ = rgb.shape
    t, ptr = upload(stored_rows(rgb, False, False), dev, 3 * w)
    cap = jpegamd.max_jfif_bytes_color(w, h, sub)
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    size = torch.zeros(1, dtype=torch.int64, device=dev)
    enc.encode_color_async(jpegamd.Encoder.image(ptr, w, h, 3 * w, False, jpegamd.ORDER_RGB, quality), sub, out.data_ptr(), cap,
                           size.data_ptr(), stream())
    st = enc.finish()
    return bytes(out[:int(size.item())].cpu().numpy()), st


def run_batch(jpegamd, enc, rgbs, dev, sub, **kw):
    return finish_files(enc, ColorBatch(jpegamd, enc, rgbs, dev, sub, **kw))


# ---- batch sizes, content, quality, subsampling ---------------------------------------------------------------------------
@pytest.mark.parametrize("count,w,h", [(1, 1, 1), (1, 257, 129), (2, 33, 17), (3, 257, 129), (8, 203, 117), (16, 64, 48),
                                       (17, 33, 17), (32, 33, 17), (32, 96, 40)])
def test_batch_matches_the_model(jpegamd, oracle, dev, count, w, h):
    enc = jpegamd.Encoder(w, rows_for(count, h))
    rgbs = pictures(jpegamd, w, h, count, seed=count)
    for i, (sub, q) in enumerate([(S420, 0), (S444, 10), (S420, 90)]):
        got, _ = run_batch(jpegamd, enc, rgbs, dev, sub, quality=q)
        for k, rgb in enumerate(rgbs):
            assert got[k] == model(oracle, rgb, q, sub), (count, w, h, sub, q, k)


# ---- pipelines --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", ["PIPELINE_PAIR", "PIPELINE_STITCH", "PIPELINE_AUTO"])
def test_pipelines(jpegamd, oracle, dev, pipeline):
    enc = jpegamd.Encoder(257, rows_for(5, 129))
    enc.set_pipeline(getattr(jpegamd, pipeline))
    for count, seed in ((1, 5), (3, 6), (5, 7)):
        rgbs = pictures(jpegamd, 257, 129, count, seed)
        for sub, q in ((S420, 0), (S444, 90)):
            got, _ = run_batch(jpegamd, enc, rgbs, dev, sub, quality=q)
            assert got == [model(oracle, r, q, sub) for r in rgbs], (pipeline, count, sub, q)


def test_auto_with_y_and_chroma_on_different_pipelines(jpegamd, dev):
    """AUTO at 2056 x 65535: the Y scans (16 384 segments each) take k_stitch, the 4:2:0 planes the pair."""
    w, h = 2056, 65535
    assert jpegamd._chroma_groups(w, rows_for(2, h), w, h, 2, S420)[3] is False
    rgbs = [synth_rgb(jpegamd, w, h, 3 + i, i) for i in range(2)]
    enc = jpegamd.Encoder(w, rows_for(2, h))
    got, _ = run_batch(jpegamd, enc, rgbs, dev, S420)
    del enc
    one = jpegamd.Encoder(w, h)
    for k, rgb in enumerate(rgbs):
        assert got[k] == single(jpegamd, one, rgb, dev, S420)[0], k


# ---- limits -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(65535, 8), (8, 65535), (4097, 9)])
def test_dimension_limits(jpegamd, oracle, dev, w, h):
    rgbs = pictures(jpegamd, w, h, 2, seed=w)
    enc = jpegamd.Encoder(w, rows_for(2, h))
    for sub in (S420, S444):
        got, _ = run_batch(jpegamd, enc, rgbs, dev, sub)
        assert got == [model(oracle, r, 0, sub) for r in rgbs], (w, h, sub)


# ---- chroma in several launches ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count,w,h", [(1, 40, 24), (3, 257, 129), (8, 64, 64), (17, 33, 17)])
def test_444_chroma_split_over_several_launches(jpegamd, oracle, dev, count, w, h):
    assert jpegamd._chroma_groups(w, rows_for(count, h), w, h, count, S444)[1] > 1
    rgbs = pictures(jpegamd, w, h, count, seed=11)
    for pipeline in (jpegamd.PIPELINE_PAIR, jpegamd.PIPELINE_STITCH):
        enc = jpegamd.Encoder(w, rows_for(count, h))
        enc.set_pipeline(pipeline)
        got, _ = run_batch(jpegamd, enc, rgbs, dev, S444, quality=90)
        assert got == [model(oracle, r, 90, S444) for r in rgbs], (count, w, h, pipeline)


# ---- stored layouts ---------------------------------------------------------------------------------------------------------
def test_layouts(jpegamd, oracle, dev):
    w, h = 203, 117
    rgbs = pictures(jpegamd, w, h, 3, seed=21)
    enc = jpegamd.Encoder(w, rows_for(3, h))
    for sub in (S420, S444):
        want = [model(oracle, r, 0, sub) for r in rgbs]
        for kw in (dict(bgr=True, bottom_up=True), dict(), dict(bgr=True), dict(bottom_up=True), dict(stride=3 * w + 5),
                   dict(stride=3 * w + 64, bgr=True, bottom_up=True), dict(stride=WIDE_STRIDE)):
            got, _ = run_batch(jpegamd, enc, rgbs, dev, sub, **kw)
            assert got == want, (sub, kw)


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_one_picture_off_alignment(jpegamd, oracle, dev, shift):
    w, h = 1031, 37
    rgbs = pictures(jpegamd, w, h, 4, seed=shift)
    enc = jpegamd.Encoder(w, rows_for(4, h))
    for sub in (S420, S444):
        for stride in (3 * w, 3 * w + 1):
            got, _ = run_batch(jpegamd, enc, rgbs, dev, sub, stride=stride, shifts=[0, shift, 0, 0], bgr=shift == 2)
            assert got == [model(oracle, r, 0, sub) for r in rgbs], (shift, sub, stride)


# ---- capacity ---------------------------------------------------------------------------------------------------------------
def test_one_picture_too_large(jpegamd, oracle, dev):
    w, h = 160, 96
    flat = [synth_rgb(jpegamd, w, h, 7 + i, 2) for i in range(3)]
    noise = synth_rgb(jpegamd, w, h, 9, 1)
    rgbs = [flat[0], noise, flat[1], flat[2]]
    enc = jpegamd.Encoder(w, rows_for(4, h))
    for sub in (S420, S444):
        want = [model(oracle, r, 0, sub) for r in rgbs]
        cap = max(len(want[0]), len(want[2]), len(want[3])) + 3
        assert len(want[1]) > cap
        b = ColorBatch(jpegamd, enc, rgbs, dev, sub, cap=cap)
        with pytest.raises(jpegamd.JpegAmdError) as err:
            enc.finish()
        assert err.value.code == -8
        res = b.results()
        assert all(ok for _, ok in res)
        assert res[1][0] == b"" and [res[k][0] for k in (0, 2, 3)] == [want[k] for k in (0, 2, 3)]
        # the exact capacity of the large one fits everything; the context is clean again
        got, _ = run_batch(jpegamd, enc, rgbs, dev, sub, cap=len(want[1]))
        assert got == want
        # the large picture last: jfif_bytes reports its 0
        b = ColorBatch(jpegamd, enc, [flat[0], noise], dev, sub, cap=cap)
        with pytest.raises(jpegamd.JpegAmdError):
            enc.finish()
        assert [f for f, _ in b.results()] == [want[0], b""]


# ---- statistics -------------------------------------------------------------------------------------------------------------
def test_statistics_are_the_sums_of_single_calls(jpegamd, dev):
    w, h = 333, 250
    rgbs = pictures(jpegamd, w, h, 5, seed=31)
    for pipeline in (jpegamd.PIPELINE_PAIR, jpegamd.PIPELINE_STITCH):
        for sub, q in ((S420, 0), (S444, 97)):
            one = jpegamd.Encoder(w, h)
            one.set_pipeline(pipeline)
            singles = [single(jpegamd, one, r, dev, sub, q) for r in rgbs]
            enc = jpegamd.Encoder(w, rows_for(5, h))
            enc.set_pipeline(pipeline)
            enc.set_profiling(2)
            got, st = run_batch(jpegamd, enc, rgbs, dev, sub, quality=q)
            assert got == [f for f, _ in singles]
            assert st.jfif_bytes == singles[-1][1].jfif_bytes
            for field in ("entropy_bits", "stuffed_bytes", "exact_fallbacks"):
                assert getattr(st, field) == sum(getattr(s, field) for _, s in singles), (pipeline, sub, q, field)
            assert st.entropy_bits > 0 and st.stuffed_bytes > 0
            assert 0 < st.ns_total < 50_000_000


# ---- one context, calls queued back to back -----------------------------------------------------------------------------------
def test_one_context_mixed_calls_without_finish(jpegamd, oracle, dev):
    w, h = 96, 64
    enc = jpegamd.Encoder(w, rows_for(4, h))
    keep, checks = [], []

    def gray_file(rgb, q):
        bmp = cm.write_bmp(rgb)
        return oracle.encode_bmp(bmp, quality=q) if q else oracle.encode_bmp(bmp)

    def gray_single(rgb, q):
        t, ptr = upload(stored_rows(rgb, True, True), dev, 3 * w)
        cap = jpegamd.max_jfif_bytes(w, h)
        out = torch.empty(cap, dtype=torch.uint8, device=dev)
        size = torch.zeros(1, dtype=torch.int64, device=dev)
        enc.encode_async(jpegamd.Encoder.image(ptr, w, h, 3 * w, True, jpegamd.ORDER_BGR, q), out.data_ptr(), cap, size.data_ptr(),
                         True, stream())
        keep.append((t, out, size))
        checks.append((lambda: bytes(out[:int(size.item())].cpu().numpy()), gray_file(rgb, q)))

    def gray_batch(rgbs, q):
        ups = [upload(stored_rows(r, True, True), dev, 3 * w) for r in rgbs]
        cap = jpegamd.max_jfif_bytes(w, h)
        outs = [torch.empty(cap, dtype=torch.uint8, device=dev) for _ in rgbs]
        sizes = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in rgbs]
        imgs = [jpegamd.Encoder.image(p, w, h, 3 * w, True, jpegamd.ORDER_BGR, q) for _, p in ups]
        enc.encode_batch_async(imgs, [o.data_ptr() for o in outs], cap, [s.data_ptr() for s in sizes], True, stream())
        keep.append((ups, outs, sizes))
        for r, o, s in zip(rgbs, outs, sizes):
            checks.append(((lambda o=o, s=s: bytes(o[:int(s.item())].cpu().numpy())), gray_file(r, q)))

    def color_single(rgb, sub, q):
        hh, ww, _ = rgb.shape
        t, ptr = upload(stored_rows(rgb, False, False), dev, 3 * ww)
        cap = jpegamd.max_jfif_bytes_color(ww, hh, sub)
        out = torch.empty(cap, dtype=torch.uint8, device=dev)
        size = torch.zeros(1, dtype=torch.int64, device=dev)
        enc.encode_color_async(jpegamd.Encoder.image(ptr, ww, hh, 3 * ww, False, jpegamd.ORDER_RGB, q), sub, out.data_ptr(), cap,
                               size.data_ptr(), stream())
        keep.append((t, out, size))
        checks.append((lambda: bytes(out[:int(size.item())].cpu().numpy()), model(oracle, rgb, q, sub)))

    def color_batch(rgbs, sub, q):
        b = ColorBatch(jpegamd, enc, rgbs, dev, sub, quality=q)
        keep.append(b)
        for k, r in enumerate(rgbs):
            checks.append(((lambda k=k: b.results()[k][0]), model(oracle, r, q, sub)))

    small = pictures(jpegamd, w, h, 4, seed=41)
    wide = pictures(jpegamd, 2 * w, h, 2, seed=43)            # (the same tiles per row: the context holds two of them)
    gray_single(small[0], 0)
    color_batch(small, S420, 0)
    gray_batch(small[:3], 0)
    color_single(small[1], S444, 0)
    color_batch(small[:2], S444, 0)
    color_batch(wide, S444, 0)                                # more colour scratch than the context holds: grown behind queued work
    gray_single(small[2], 0)
    color_batch(small[1:], S420, 90)                          # a quality change
    color_single(small[3], S420, 90)
    color_batch(wide, S420, 10)
    enc.finish()
    for i, (got, want) in enumerate(checks):
        assert got() == want, i


# ---- k_stitch's epoch wrap ----------------------------------------------------------------------------------------------------
def test_stitch_epoch_wrap_between_y_and_chroma(jpegamd, oracle, dev):
    """Under PIPELINE_STITCH a fresh context starts at epoch 0 and every k_stitch launch takes the next of 1 .. 16383; the
    granules are cleared in front of launch 16384.  A colour batch whose chroma goes in one launch launches k_stitch twice (Y,
    chroma).  The first batch runs at epochs 1 and 2; 16 x 16 GRAY fillers take launches 3 .. 16382; the second batch's Y scans run
    at epoch 16383 and its chroma, after the clear, at epoch 1 again -- where the first batch's Y granules would still lie."""
    w, h = 8200, 520
    count = 2
    enc = jpegamd.Encoder(w, rows_for(count, h))
    enc.set_pipeline(jpegamd.PIPELINE_STITCH)
    assert jpegamd._chroma_groups(w, rows_for(count, h), w, h, count, S420, jpegamd.PIPELINE_STITCH)[1] == 1
    rgbs = pictures(jpegamd, w, h, count, seed=51)
    one = jpegamd.Encoder(w, h)
    want = [single(jpegamd, one, r, dev, S420)[0] for r in rgbs]
    del one
    got, _ = run_batch(jpegamd, enc, rgbs, dev, S420)
    assert got == want
    small = np.random.default_rng(1).integers(0, 256, (16, 16), np.uint8)
    st, sptr = upload(small, dev, 16)
    scap = jpegamd.max_jfif_bytes(16, 16)
    sout = torch.empty(scap, dtype=torch.uint8, device=dev)
    ssize = torch.zeros(1, dtype=torch.int64, device=dev)
    simg = jpegamd.Encoder.image(sptr, 16, 16, 16, False, jpegamd.ORDER_GRAY, 0)
    for n in range(3, 16383):
        enc.encode_async(simg, sout.data_ptr(), scap, ssize.data_ptr(), True, stream())
        if n % 1000 == 0:
            enc.finish()
    enc.finish()
    assert bytes(sout[:int(ssize.item())].cpu().numpy()) == oracle.encode_bmp(cm.write_bmp(np.repeat(small[:, :, None], 3, axis=2)))
    got, _ = run_batch(jpegamd, enc, rgbs[::-1], dev, S420)
    assert got == want[::-1]
    got, _ = run_batch(jpegamd, enc, rgbs, dev, S420)
    assert got == want


# ---- encode_tensor_batch ------------------------------------------------------------------------------------------------------
def test_encode_tensor_batch(jpegamd, dev):
    w, h = 72, 40
    host = np.stack(pictures(jpegamd, w, h, 80, seed=61))
    t = torch.from_numpy(host).to(dev)                           # [80, H, W, 3]
    gray = t[:, :, :, 1].contiguous()                            # [80, H, W]
    for sub in (S420, S444):
        for view in (t[:5], t[::2][:5], t[:40]):
            files = jpegamd.encode_tensor_batch(view, quality=0, subsampling=sub)
            assert len(files) == view.shape[0]
            assert files == [jpegamd.encode_tensor(view[i], 0, sub) for i in range(view.shape[0])], (sub, view.shape)
    for view in (gray[:5], gray[::2][:5], gray[:40]):
        files = jpegamd.encode_tensor_batch(view, quality=90)
        assert files == [jpegamd.encode_tensor(view[i], 90) for i in range(view.shape[0])], view.shape


@pytest.mark.parametrize("n,w,h", [(2, 33, 17), (8, 299, 299), (4, 64, 100), (3, 17, 1)])
def test_encode_tensor_batch_heights_off_the_block_grid(jpegamd, dev, n, w, h):
    """A batch needs n x the block rows of one picture: with H not a multiple of 8 that is more than n x H rows.  Every case starts
    from no cached context, so encode_tensor_batch sizes the context itself."""
    host = np.stack(pictures(jpegamd, w, h, 2 * n, seed=h))
    t = torch.from_numpy(host).to(dev)
    g = t[:, :, :, 0].contiguous()
    cases = [(t[:n], dict(subsampling=S420)), (t[::2], dict(subsampling=S444)), (g[:n], {}), (g[::2], {})]
    for view, kw in cases:
        for enc, _, _ in list(jpegamd._tensor_encoders.values()):
            enc.close()
        jpegamd._tensor_encoders.clear()
        files = jpegamd.encode_tensor_batch(view, quality=0, **kw)
        assert files == [jpegamd.encode_tensor(view[i], 0, **kw) for i in range(n)], (n, w, h, view.shape, kw)


# ---- full size ----------------------------------------------------------------------------------------------------------------
def test_eight_8192_pictures_420(jpegamd, dev):
    w = h = 8192
    rgbs = [synth_rgb(jpegamd, w, h, 71 + i, i % 2) for i in range(8)]
    enc = jpegamd.Encoder(w, rows_for(8, h))
    got, _ = run_batch(jpegamd, enc, rgbs, dev, S420, quality=50, cap=2 * w * h + (1 << 20))
    del enc
    one = jpegamd.Encoder(w, h)
    for k, rgb in enumerate(rgbs):
        assert got[k] == single(jpegamd, one, rgb, dev, S420, 50)[0], k


def test_thirty_two_1024_pictures_444(jpegamd, dev):
    w = h = 1024
    rgbs = [synth_rgb(jpegamd, w, h, 81 + i, (0, 1, 3)[i % 3]) for i in range(32)]
    enc = jpegamd.Encoder(w, rows_for(32, h))
    got, _ = run_batch(jpegamd, enc, rgbs, dev, S444)
    one = jpegamd.Encoder(w, h)
    for k, rgb in enumerate(rgbs):
        assert got[k] == single(jpegamd, one, rgb, dev, S444)[0], k
