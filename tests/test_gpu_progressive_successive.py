"""Progressive colour files with successive approximation on the GPU (DESIGN.md 4.6.14:
jpegamd_encode_color_progressive_successive_batch_async, jpegamd_encode_ycbcr_progressive_successive_batch_async): every device file is
compared byte for byte with the CPU model (tests/progressive_successive_model.py).  What a fixture exercises is proven on the model's
counters in test_progressive_successive_host.py."""
from __future__ import annotations

import numpy as np
import pytest

import color_model as cm
import gpu_support as gs
import huffman_model as hm
import interleaved_model as im
import mjpeg_support as ms
import progressive_successive_fixtures as fx
import progressive_successive_model as psm
from gpu_support import PLANES, S420, S422, S444, dev  # noqa: F401

torch = gs.torch
pytestmark = pytest.mark.gpu
ERR_ARG = -1


def model(oracle, rgb, q, sub):
    return cm.memo(psm.rgb_file, oracle, rgb, q, sub)


class PixelsCall(gs.Outputs):
    """One batch of RGB pictures through jpegamd_encode_color_progressive_successive_batch_async."""

    def __init__(self, jpegamd, enc, rgbs, dev, sub, q=0, cap=None, order=None):
        h, w, _ = rgbs[0].shape
        self.px = [gs.upload(gs.stored_rows(r, False), dev, 3 * w) for r in rgbs]
        super().__init__(dev, len(rgbs), cap if cap is not None else jpegamd.max_jfif_bytes_progressive_successive(w, h, sub))
        imgs = [jpegamd.Encoder.image(ptr, w, h, 3 * w, False, jpegamd.ORDER_RGB if order is None else order, q) for _, ptr in self.px]
        enc.encode_color_progressive_successive_batch_async(imgs, sub, self.out_ptrs, self.cap, self.size_ptrs, gs.stream())


class Successive:
    """An Encoder as gpu_support.YccBatch sees it: every YCbCr call goes to jpegamd_encode_ycbcr_progressive_successive_batch_async."""

    def __init__(self, enc, matrix):
        self.enc, self.matrix = enc, matrix

    def encode_ycbcr_batch_async(self, imgs, subsampling, out_ptrs, out_cap, size_ptrs, stream=0, sample_range=0, sample_format=0):
        self.enc.encode_ycbcr_progressive_successive_batch_async(imgs, subsampling, sample_range, sample_format, self.matrix, out_ptrs, out_cap,
                                                                 size_ptrs, stream)


def ycc_files(jpegamd, enc, kind, planes, dev, sub, layout, q=0):
    h, w = planes[0][0].shape
    rng, fmt, matrix = kind.args(jpegamd)
    call = gs.YccBatch(jpegamd, Successive(enc, matrix), planes, dev, sub, layout, quality=q,
                       cap=jpegamd.max_jfif_bytes_progressive_successive(w, h, sub), sample_range=rng, sample_format=fmt)
    return gs.finish_files(enc, call)


def rgb_files(jpegamd, enc, rgbs, dev, sub, q=0, **kw):
    return gs.finish_files(enc, PixelsCall(jpegamd, enc, rgbs, dev, sub, q, **kw))


def check(jpegamd, files, st, models, w, h, sub):
    """For every call: the files, finish's statistics are the models', every file is within the bound."""
    assert files == [m.file for m in models]
    assert st.entropy_bits == sum(m.bits for m in models)
    assert st.stuffed_bytes == sum(sum(m.stuffed) for m in models)
    assert all(len(f) <= jpegamd.max_jfif_bytes_progressive_successive(w, h, sub) for f in files)


def device_counts(jpegamd, enc, n):
    counts = np.zeros((n, psm.TABLES, 256), np.uint64)
    assert jpegamd.lib.jpegamd_debug_progressive_successive_counts(enc._h, counts.ctypes.data) == 0
    return counts.astype(np.int64)


@pytest.fixture(scope="module")
def enc(jpegamd, dev):
    e = jpegamd.Encoder(512, gs.rows_for(3, 250))               # (the largest calls: three pictures of 333 x 250, one of 512 x 512)
    yield e
    e.close()


# ---- flat pictures: the shortest segments, one-symbol tables, pad blocks ------------------------------------------------------------------
@pytest.mark.parametrize("w,h,value,sub", fx.FLAT + [fx.FLAT_513], ids=["8x8", "7x5", "513-blocks"])
def test_flat(jpegamd, oracle, dev, enc, w, h, value, sub):
    rgb = fx.flat_rgb(w, h, value)
    m = model(oracle, rgb, 50, sub)
    assert all(s[-1] <= 2 for k, s in enumerate(m.seg_bits) if k not in (0, 6))     # a last segment of 1 or 2 bits behind segments of 9
    files, st = rgb_files(jpegamd, enc, [rgb], dev, sub, 50)
    check(jpegamd, files, st, [m], w, h, sub)
    assert np.array_equal(device_counts(jpegamd, enc, 1)[0], m.counts)


def test_chain_of_nine_bit_segments_at_every_phase(jpegamd, oracle, dev):
    """2049 flat blocks a component: in the first AND the refinement AC scans eight FULL segments of 9 bits (one EOB8 run each) start
    at the bit phases 0, 1, .. 7 of the scan, then a last segment of 2 bits."""
    w, h, value, sub = fx.CHAIN
    rgb = fx.flat_rgb(w, h, value)
    m = model(oracle, rgb, 50, sub)
    assert all(m.seg_bits[k] == (9,) * 8 + (2,) for k in (1, 2, 3, 4, 5, 7, 8, 9))
    e = jpegamd.Encoder(w, h)
    try:
        files, st = rgb_files(jpegamd, e, [rgb], dev, sub, 50)
        check(jpegamd, files, st, [m], w, h, sub)
    finally:
        e.close()


# ---- a photograph ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", (S444, S420, S422))
@pytest.mark.parametrize("q", (10, 50, 90))
def test_photograph_crop(jpegamd, oracle, dev, enc, q, sub):
    rgb = fx.lena_crop()
    files, st = rgb_files(jpegamd, enc, [rgb], dev, sub, q)
    check(jpegamd, files, st, [model(oracle, rgb, q, sub)], 128, 128, sub)


def test_photograph_whole_and_an_independent_decoder(jpegamd, oracle, dev, enc):
    rgb = fx.lena()
    m = model(oracle, rgb, 50, S420)
    files, st = rgb_files(jpegamd, enc, [rgb], dev, S420, 50)
    check(jpegamd, files, st, [m], 512, 512, S420)
    assert np.array_equal(device_counts(jpegamd, enc, 1)[0], m.counts)
    assert np.array_equal(ms.decode(files[0]), ms.decode(cm.memo(im.interleaved_file, oracle, rgb, 50, S420).file))


# ---- dense blocks: long B and tails, ZRLs with bits; the runs' edges ---------------------------------------------------------------------
def test_noise(jpegamd, oracle, dev, enc):
    rgb = fx.noise_rgb()
    m = model(oracle, rgb, fx.NOISE_Q, S444)
    files, st = rgb_files(jpegamd, enc, [rgb], dev, S444, fx.NOISE_Q)
    check(jpegamd, files, st, [m], fx.NOISE_W, fx.NOISE_H, S444)
    assert np.array_equal(device_counts(jpegamd, enc, 1)[0], m.counts)


def test_run_edges(jpegamd, oracle, dev, enc):
    m = fx.edge_model(oracle)
    h, w = fx.edge_planes()[0].shape
    files, st = ycc_files(jpegamd, enc, ms.FULL8, [fx.edge_planes()], dev, S444, PLANES, fx.EDGE_Q)
    check(jpegamd, files, st, [m], w, h, S444)
    assert np.array_equal(device_counts(jpegamd, enc, 1)[0], m.counts)


# ---- batches ------------------------------------------------------------------------------------------------------------------------------
def test_batch_of_three_with_counts_and_tables(jpegamd, oracle, dev, enc):
    import progressive_runs_model as prm
    rgbs = fx.synth_batch()
    models = [model(oracle, r, 50, S420) for r in rgbs]
    files, st = rgb_files(jpegamd, enc, rgbs, dev, S420, 50)
    check(jpegamd, files, st, models, 333, 250, S420)
    counts = device_counts(jpegamd, enc, 3)
    for f, m, c in zip(files, models, counts):
        assert np.array_equal(c, m.counts)
        assert prm.parse_tables(f) == [(psm.table_id(k), list(b), list(v)) for k, (b, v, _) in enumerate(m.tables)]
    old = np.zeros((3, 8, 256), np.uint64)                       # the seven-scan file's counts are not this call's
    assert jpegamd.lib.jpegamd_debug_progressive_counts(enc._h, old.ctypes.data) == ERR_ARG


# ---- one YCbCr source of each kind: the plumbing ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,sub,layout", [(ms.LIMITED8, S420, gs.CBCR), (ms.MSB10, S420, gs.CBCR), (ms.FULL8_709, S422, gs.YUYV)],
                         ids=["nv12-limited", "p010", "yuyv-bt709"])
def test_sources(jpegamd, oracle, dev, enc, kind, sub, layout):
    w, h = 40, 24
    planes = [ms.stored_planes(kind, w, h, sub, 61)]
    m = cm.memo(psm.ycbcr_file, oracle, *ms.mapped_planes(kind, planes[0], sub), 75, sub)
    files, st = ycc_files(jpegamd, enc, kind, planes, dev, sub, layout, 75)
    check(jpegamd, files, st, [m], w, h, sub)


# ---- capacity -----------------------------------------------------------------------------------------------------------------------------
def test_one_picture_of_a_batch_does_not_fit(jpegamd, oracle, dev, enc):
    rgbs = [gs.synth_rgb(jpegamd, 200, 120, 50, 0), np.random.default_rng(8).integers(0, 256, (120, 200, 3), np.uint8),
            gs.synth_rgb(jpegamd, 200, 120, 52, 3)]
    models = [model(oracle, r, 50, S420) for r in rgbs]
    sizes = [len(m.file) for m in models]
    cap = sizes[1] - 1
    assert max(sizes[0], sizes[2]) <= cap
    call = PixelsCall(jpegamd, enc, rgbs, dev, S420, 50, cap=cap)
    with pytest.raises(jpegamd.JpegAmdError) as err:
        enc.finish()
    assert err.value.code == -8                                 # JPEGAMD_ERR_HUFF_CAPACITY
    files = gs.intact_files(call)                               # nothing written past out_capacity
    assert call.sizes.cpu().tolist() == [sizes[0], 0, sizes[2]]
    assert files[0] == models[0].file and files[2] == models[2].file
    files, st = rgb_files(jpegamd, enc, rgbs, dev, S420, 50, cap=sizes[1])       # the context is usable, and at exactly its size the file is whole
    check(jpegamd, files, st, models, 200, 120, S420)


# ---- refusals, the context's Huffman mode -------------------------------------------------------------------------------------------------
def test_refusals_and_the_huffman_mode(jpegamd, oracle, dev):
    rgb = gs.synth_rgb(jpegamd, 40, 24, 80, 0)
    want = model(oracle, rgb, 50, S420).file
    std = cm.memo(im.interleaved_file, oracle, rgb, 50, S420).file
    opt = cm.memo(hm.rgb_file, oracle, rgb, 50, S420).file
    e = jpegamd.Encoder(64, 64)
    try:
        with pytest.raises(jpegamd.JpegAmdError) as err:
            PixelsCall(jpegamd, e, [rgb], dev, 3, 50, cap=1 << 16)
        assert err.value.code == ERR_ARG
        with pytest.raises(jpegamd.JpegAmdError) as err:
            PixelsCall(jpegamd, e, [rgb], dev, S420, 50, cap=1 << 16, order=jpegamd.ORDER_GRAY)
        assert err.value.code == ERR_ARG
        counts = np.zeros((1, psm.TABLES, 256), np.uint64)
        assert jpegamd.lib.jpegamd_debug_progressive_successive_counts(e._h, counts.ctypes.data) == ERR_ARG    # no such call yet
        for mode, one in ((jpegamd.HUFFMAN_STANDARD, std), (jpegamd.HUFFMAN_OPTIMIZED, opt)):
            e.set_huffman(mode)
            (f,), _ = gs.finish_files(e, ms.PixelsCall(jpegamd, e, [rgb], dev, S420, "rgb", 0, 50))
            assert f == one
            (f,), _ = rgb_files(jpegamd, e, [rgb], dev, S420, 50)
            assert f == want                                    # the mode is not read ...
            (f,), _ = gs.finish_files(e, ms.PixelsCall(jpegamd, e, [rgb], dev, S420, "rgb", 0, 50))
            assert f == one                                     # ... and is what it was
    finally:
        e.close()


# ---- Python -------------------------------------------------------------------------------------------------------------------------------
def test_module(jpegamd, oracle, dev):
    import jpegamd.progressive_successive as ps
    rgbs = gs.pictures(jpegamd, 24, 40, 2, seed=4)
    t = torch.from_numpy(np.stack(rgbs)).to(dev)
    want = [model(oracle, r, 0, S420).file for r in rgbs]
    assert ps.encode_tensor_batch(t) == want
    assert ps.encode_tensor(t[1]) == want[1]
    y, cb, cr = ms.derived_planes(gs.synth_rgb(jpegamd, 24, 40, 8, 0), S422)
    files = ps.encode_ycbcr_batch(torch.from_numpy(y[None]).to(dev), torch.from_numpy(cb[None]).to(dev), torch.from_numpy(cr[None]).to(dev),
                                  subsampling=S422)
    assert files == [cm.memo(psm.ycbcr_file, oracle, y, cb, cr, 0, S422).file]
