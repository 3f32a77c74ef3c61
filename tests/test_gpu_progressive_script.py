"""Progressive files with a scan script of the caller's, and grayscale progressive files, on the GPU (DESIGN.md 4.6.15:
jpegamd_encode_color_progressive_script_batch_async, jpegamd_encode_ycbcr_progressive_script_batch_async,
jpegamd_encode_gray_progressive_script_batch_async): every device file is compared byte for byte with the CPU model
(tests/progressive_script_model.py).  What a script or a picture exercises is proven on the model's counters in
test_progressive_script_host.py."""
from __future__ import annotations

import numpy as np
import pytest

import color_model as cm
import gpu_support as gs
import huffman_model as hm
import interleaved_model as im
import mjpeg_support as ms
import progressive_runs_model as prm
import progressive_script_fixtures as fx
import progressive_script_model as scm
import progressive_successive_fixtures as sfx
import progressive_successive_model as psm
import scan_model as sm
from gpu_support import PLANES, S420, S422, S444, dev  # noqa: F401

torch = gs.torch
pytestmark = pytest.mark.gpu
ERR_ARG = -1


class PixelsCall(gs.Outputs):
    """One batch of RGB pictures through jpegamd_encode_color_progressive_script_batch_async."""

    def __init__(self, jpegamd, enc, rgbs, dev, sub, script, q=0, cap=None, order=None):
        h, w, _ = rgbs[0].shape
        self.px = [gs.upload(gs.stored_rows(r, False), dev, 3 * w) for r in rgbs]
        super().__init__(dev, len(rgbs), cap if cap is not None else jpegamd.max_jfif_bytes_progressive_script(w, h, sub, script))
        imgs = [jpegamd.Encoder.image(ptr, w, h, 3 * w, False, jpegamd.ORDER_RGB if order is None else order, q) for _, ptr in self.px]
        enc.encode_color_progressive_script_batch_async(imgs, sub, script, self.out_ptrs, self.cap, self.size_ptrs, gs.stream())


class GrayCall(gs.Outputs):
    """One batch of pictures (rows as they are stored, in `order`) through jpegamd_encode_gray_progressive_script_batch_async."""

    def __init__(self, jpegamd, enc, rows, w, h, dev, script, q=0, order=None):
        self.px = [gs.upload(r, dev, r.shape[1]) for r in rows]
        super().__init__(dev, len(rows), jpegamd.max_jfif_bytes_progressive_script(w, h, 0, script))
        imgs = [jpegamd.Encoder.image(ptr, w, h, r.shape[1], False, jpegamd.ORDER_GRAY if order is None else order, q) for r, (_, ptr) in zip(rows, self.px)]
        enc.encode_gray_progressive_script_batch_async(imgs, script, self.out_ptrs, self.cap, self.size_ptrs, gs.stream())


class Scripted:
    """An Encoder as gpu_support.YccBatch sees it: every YCbCr call goes to jpegamd_encode_ycbcr_progressive_script_batch_async."""

    def __init__(self, enc, matrix, script):
        self.enc, self.matrix, self.script = enc, matrix, script

    def encode_ycbcr_batch_async(self, imgs, subsampling, out_ptrs, out_cap, size_ptrs, stream=0, sample_range=0, sample_format=0):
        self.enc.encode_ycbcr_progressive_script_batch_async(imgs, subsampling, sample_range, sample_format, self.matrix, self.script, out_ptrs,
                                                             out_cap, size_ptrs, stream)


def rgb_files(jpegamd, enc, rgbs, dev, sub, script, q=0, **kw):
    return gs.finish_files(enc, PixelsCall(jpegamd, enc, rgbs, dev, sub, script, q, **kw))


def gray_files(jpegamd, enc, planes, dev, script, q=0):
    h, w = planes[0].shape
    return gs.finish_files(enc, GrayCall(jpegamd, enc, [gs.stored_rows(p, False) for p in planes], w, h, dev, script, q))


def check(jpegamd, files, st, models, w, h, sub, script):
    """For every call: the files, finish's statistics are the models', every file is within the bound."""
    assert [len(f) for f in files] == [len(m.file) for m in models]
    assert files == [m.file for m in models]
    assert st.entropy_bits == sum(m.bits for m in models)
    assert st.stuffed_bytes == sum(sum(m.stuffed) for m in models)
    bound = jpegamd.max_jfif_bytes_progressive_script(w, h, sub, script)
    assert bound > 0 and all(len(f) <= bound for f in files)


def device_counts(jpegamd, enc, n, tables):
    counts = np.zeros((n, tables, 256), np.uint64)
    assert jpegamd.lib.jpegamd_debug_progressive_script_counts(enc._h, counts.ctypes.data, tables) == 0
    return counts.astype(np.int64)


@pytest.fixture(scope="module")
def enc(jpegamd, dev):
    e = jpegamd.Encoder(512, gs.rows_for(3, 250))               # (the largest calls: three pictures of 333 x 250, one of 512 x 512)
    yield e
    e.close()


# ---- flat pictures: one block, one MCU with three pad blocks, one-symbol tables ---------------------------------------------------------------
@pytest.mark.parametrize("name", ("SPLIT", "DC_FORMS", "Y_CB", "DC_ONLY"))
@pytest.mark.parametrize("sub", (S420, S444))
@pytest.mark.parametrize("w,h,value", fx.FLAT, ids=["8x8", "7x5"])
def test_flat(jpegamd, oracle, dev, enc, w, h, value, sub, name):
    script, rgb = fx.COLOUR[name], fx.flat_rgb(w, h, value)
    m = fx.model(oracle, rgb, 50, sub, script)
    files, st = rgb_files(jpegamd, enc, [rgb], dev, sub, script, 50)
    check(jpegamd, files, st, [m], w, h, sub, script)
    assert np.array_equal(device_counts(jpegamd, enc, 1, len(m.ids))[0], m.counts)


# ---- segment edges ------------------------------------------------------------------------------------------------------------------------
def test_gray_dc_refinement_ends_with_a_one_bit_segment(jpegamd, oracle, dev):
    w, h = fx.GRAY_257
    plane = fx.gray_plane(w, h)
    m = fx.gray_model(oracle, plane, 50, fx.GRAY_SUCCESSIVE)
    assert m.seg_bits[4] == (256, 1)
    e = jpegamd.Encoder(w, h)
    try:
        files, st = gray_files(jpegamd, e, [plane], dev, None, 50)   # the default script
        check(jpegamd, files, st, [m], w, h, 0, None)
    finally:
        e.close()


def test_one_component_dc_scans_of_six_segments(jpegamd, oracle, dev, enc):
    rgb = sfx.synth_batch()[0]
    m = fx.model(oracle, rgb, 50, S420, fx.DC_FORMS)
    assert m.seg_bits[3] == (256,) * 5 + (64,)
    files, st = rgb_files(jpegamd, enc, [rgb], dev, S420, fx.DC_FORMS, 50)
    check(jpegamd, files, st, [m], 333, 250, S420, fx.DC_FORMS)
    assert np.array_equal(device_counts(jpegamd, enc, 1, len(m.ids))[0], m.counts)


def test_two_component_scan_with_pad_blocks_over_several_mcus(jpegamd, oracle, dev, enc):
    rgb = fx.crop_67x43()
    for sub in (S420, S422):
        m = fx.model(oracle, rgb, 50, sub, fx.Y_CB)
        assert m.pad_blocks[0] > 0
        files, st = rgb_files(jpegamd, enc, [rgb], dev, sub, fx.Y_CB, 50)
        check(jpegamd, files, st, [m], 67, 43, sub, fx.Y_CB)


def test_chain_of_nine_bit_segments_under_deep(jpegamd, oracle, dev):
    w, h, value, sub = fx.CHAIN
    rgb = fx.flat_rgb(w, h, value)
    m = fx.model(oracle, rgb, 50, sub, fx.DEEP)
    e = jpegamd.Encoder(w, h)
    try:
        files, st = rgb_files(jpegamd, e, [rgb], dev, sub, fx.DEEP, 50)
        check(jpegamd, files, st, [m], w, h, sub, fx.DEEP)
    finally:
        e.close()


# ---- a photograph, noise ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,sub", [("SPLIT", S420), ("DEEP", S444), ("EDGES", S422)])
@pytest.mark.parametrize("q", (10, 50, 90))
def test_photograph_crop(jpegamd, oracle, dev, enc, q, name, sub):
    rgb, script = sfx.lena_crop(), fx.COLOUR[name]
    files, st = rgb_files(jpegamd, enc, [rgb], dev, sub, script, q)
    check(jpegamd, files, st, [fx.model(oracle, rgb, q, sub, script)], 128, 128, sub, script)


def test_photograph_whole_and_an_independent_decoder(jpegamd, oracle, dev, enc):
    rgb = sfx.lena()
    m = fx.model(oracle, rgb, 50, S420, fx.SPLIT)
    files, st = rgb_files(jpegamd, enc, [rgb], dev, S420, fx.SPLIT, 50)
    check(jpegamd, files, st, [m], 512, 512, S420, fx.SPLIT)
    assert np.array_equal(ms.decode(files[0]), ms.decode(cm.memo(im.interleaved_file, oracle, rgb, 50, S420).file))


@pytest.mark.parametrize("name", ("DEEP", "LIMIT"))
def test_noise(jpegamd, oracle, dev, enc, name):
    rgb, script = sfx.noise_rgb(), fx.COLOUR[name]
    m = fx.model(oracle, rgb, sfx.NOISE_Q, S444, script)
    files, st = rgb_files(jpegamd, enc, [rgb], dev, S444, script, sfx.NOISE_Q)
    check(jpegamd, files, st, [m], sfx.NOISE_W, sfx.NOISE_H, S444, script)
    assert np.array_equal(device_counts(jpegamd, enc, 1, len(m.ids))[0], m.counts)


# ---- the default and the built-in scripts: the existing models' bytes ------------------------------------------------------------------------
def test_default_and_built_in_scripts(jpegamd, oracle, dev, enc):
    rgb = sfx.lena_crop()
    for sub in (S420, S444):
        succ = cm.memo(psm.rgb_file, oracle, rgb, 50, sub).file
        (f,), _ = rgb_files(jpegamd, enc, [rgb], dev, sub, None, 50)
        assert f == succ
        (f,), _ = rgb_files(jpegamd, enc, [rgb], dev, sub, fx.SUCCESSIVE, 50)
        assert f == succ
        (f,), _ = rgb_files(jpegamd, enc, [rgb], dev, sub, fx.SPECTRAL, 50)
        assert f == cm.memo(prm.rgb_file, oracle, rgb, 50, sub).file


# ---- grayscale ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("GRAY_SUCCESSIVE", "GRAY_SPLIT"))
@pytest.mark.parametrize("w,h", [(1, 1), (7, 9), (333, 250)])
def test_gray(jpegamd, oracle, dev, enc, w, h, name):
    script = fx.GRAYS[name]
    plane = fx.gray_plane(w, h)
    m = fx.gray_model(oracle, plane, 50, script)
    files, st = gray_files(jpegamd, enc, [plane], dev, None if name == "GRAY_SUCCESSIVE" else script, 50)
    check(jpegamd, files, st, [m], w, h, 0, script)
    assert np.array_equal(device_counts(jpegamd, enc, 1, len(m.ids))[0], m.counts)


def test_gray_codes_the_luma_of_bgr_pixels(jpegamd, oracle, dev, enc):
    rgb = gs.synth_rgb(jpegamd, 40, 24, 7, 0)
    m = fx.gray_model(oracle, np.ascontiguousarray(sm.luma_plane(rgb)), 75, fx.GRAY_SPLIT)
    call = GrayCall(jpegamd, enc, [gs.stored_rows(rgb, False, True)], 40, 24, dev, fx.GRAY_SPLIT, 75, jpegamd.ORDER_BGR)
    files, st = gs.finish_files(enc, call)
    check(jpegamd, files, st, [m], 40, 24, 0, fx.GRAY_SPLIT)


# ---- batches, sources, capacity -----------------------------------------------------------------------------------------------------------
def test_batch_of_three_with_counts_and_tables(jpegamd, oracle, dev, enc):
    rgbs = sfx.synth_batch()
    models = [fx.model(oracle, r, 50, S420, fx.SPLIT) for r in rgbs]
    files, st = rgb_files(jpegamd, enc, rgbs, dev, S420, fx.SPLIT, 50)
    check(jpegamd, files, st, models, 333, 250, S420, fx.SPLIT)
    counts = device_counts(jpegamd, enc, 3, len(models[0].ids))
    for f, m, c in zip(files, models, counts):
        assert np.array_equal(c, m.counts)
        assert prm.parse_tables(f) == [(i, list(b), list(v)) for i, (b, v, _) in zip(m.ids, m.tables)]


def test_nv12_limited_range_source(jpegamd, oracle, dev, enc):
    kind, sub, w, h = ms.LIMITED8, S420, 40, 24
    planes = [ms.stored_planes(kind, w, h, sub, 61)]
    m = cm.memo(scm.ycbcr_file, oracle, *ms.mapped_planes(kind, planes[0], sub), 75, sub, scm._key(fx.SPLIT))
    rng, fmt, matrix = kind.args(jpegamd)
    call = gs.YccBatch(jpegamd, Scripted(enc, matrix, fx.SPLIT), planes, dev, sub, gs.CBCR, quality=75,
                       cap=jpegamd.max_jfif_bytes_progressive_script(w, h, sub, fx.SPLIT), sample_range=rng, sample_format=fmt)
    files, st = gs.finish_files(enc, call)
    check(jpegamd, files, st, [m], w, h, sub, fx.SPLIT)


def test_one_picture_of_a_batch_does_not_fit(jpegamd, oracle, dev, enc):
    rgbs = [gs.synth_rgb(jpegamd, 200, 120, 50, 0), np.random.default_rng(8).integers(0, 256, (120, 200, 3), np.uint8),
            gs.synth_rgb(jpegamd, 200, 120, 52, 3)]
    models = [fx.model(oracle, r, 50, S420, fx.SPLIT) for r in rgbs]
    sizes = [len(m.file) for m in models]
    cap = sizes[1] - 1
    assert max(sizes[0], sizes[2]) <= cap
    call = PixelsCall(jpegamd, enc, rgbs, dev, S420, fx.SPLIT, 50, cap=cap)
    with pytest.raises(jpegamd.JpegAmdError) as err:
        enc.finish()
    assert err.value.code == -8                                 # JPEGAMD_ERR_HUFF_CAPACITY
    files = gs.intact_files(call)                               # nothing written past out_capacity
    assert call.sizes.cpu().tolist() == [sizes[0], 0, sizes[2]]
    assert files[0] == models[0].file and files[2] == models[2].file
    files, st = rgb_files(jpegamd, enc, rgbs, dev, S420, fx.SPLIT, 50, cap=sizes[1])      # the context is usable, and at exactly its size the file is whole
    check(jpegamd, files, st, models, 200, 120, S420, fx.SPLIT)


# ---- refusals, the context's Huffman mode, the debug counts -----------------------------------------------------------------------------------
def test_refusals_and_the_huffman_mode(jpegamd, oracle, dev):
    rgb = gs.synth_rgb(jpegamd, 40, 24, 80, 0)
    split = fx.model(oracle, rgb, 50, S420, fx.SPLIT)
    want, tables = split.file, len(split.ids)
    std = cm.memo(im.interleaved_file, oracle, rgb, 50, S420).file
    opt = cm.memo(hm.rgb_file, oracle, rgb, 50, S420).file
    invalid = [(fx.ALL, 0, 0, 0, 0), (fx.Y, 1, 63, 2, 1)]        # a refinement without a first scan
    e = jpegamd.Encoder(64, 64)
    try:
        counts = np.zeros((1, 16, 256), np.uint64)
        assert jpegamd.lib.jpegamd_debug_progressive_script_counts(e._h, counts.ctypes.data, tables) == ERR_ARG     # no such call yet
        (f,), _ = rgb_files(jpegamd, e, [rgb], dev, S420, fx.SPLIT, 50)
        assert f == want
        for bad in (dict(script=invalid), dict(script=fx.SPLIT, sub=3), dict(script=fx.GRAY_SPLIT)):
            with pytest.raises(jpegamd.JpegAmdError) as err:
                PixelsCall(jpegamd, e, [rgb], dev, bad.get("sub", S420), bad["script"], 50, cap=1 << 16)
            assert err.value.code == ERR_ARG
            assert np.array_equal(device_counts(jpegamd, e, 1, tables)[0], split.counts)      # the context is as it was
        with pytest.raises(jpegamd.JpegAmdError) as err:          # a colour script on the grayscale entry
            GrayCall(jpegamd, e, [gs.stored_rows(sm.luma_plane(rgb), False)], 40, 24, dev, fx.SPLIT)
        assert err.value.code == ERR_ARG
        (f,), _ = rgb_files(jpegamd, e, [rgb], dev, S420, fx.SPLIT, 50)
        assert f == want                                        # the next valid call on the same context
        old = np.zeros((1, 10, 256), np.uint64)                  # the older entries' counts are not a script call's, and the other way round
        assert jpegamd.lib.jpegamd_debug_progressive_successive_counts(e._h, old.ctypes.data) == ERR_ARG
        assert jpegamd.lib.jpegamd_debug_progressive_counts(e._h, old.ctypes.data) == ERR_ARG
        (f,), _ = rgb_files(jpegamd, e, [rgb], dev, S420, None, 50)      # ten tables, as the successive entry's -- still a script call
        assert jpegamd.lib.jpegamd_debug_progressive_successive_counts(e._h, old.ctypes.data) == ERR_ARG
        assert jpegamd.lib.jpegamd_debug_progressive_script_counts(e._h, old.ctypes.data, 10) == 0
        imgs = [jpegamd.Encoder.image(gs.upload(gs.stored_rows(rgb, False), dev, 120)[1], 40, 24, 120, False, jpegamd.ORDER_RGB, 50)]
        out = gs.Outputs(dev, 1, jpegamd.max_jfif_bytes_progressive_successive(40, 24, S420))
        e.encode_color_progressive_successive_batch_async(imgs, S420, out.out_ptrs, out.cap, out.size_ptrs, gs.stream())
        e.finish()
        assert jpegamd.lib.jpegamd_debug_progressive_script_counts(e._h, old.ctypes.data, 10) == ERR_ARG
        for mode, one in ((jpegamd.HUFFMAN_STANDARD, std), (jpegamd.HUFFMAN_OPTIMIZED, opt)):
            e.set_huffman(mode)
            (f,), _ = gs.finish_files(e, ms.PixelsCall(jpegamd, e, [rgb], dev, S420, "rgb", 0, 50))
            assert f == one
            (f,), _ = rgb_files(jpegamd, e, [rgb], dev, S420, fx.SPLIT, 50)
            assert f == want                                    # the mode is not read ...
            (f,), _ = gs.finish_files(e, ms.PixelsCall(jpegamd, e, [rgb], dev, S420, "rgb", 0, 50))
            assert f == one                                     # ... and is what it was
    finally:
        e.close()


# ---- Python -------------------------------------------------------------------------------------------------------------------------------
def test_module(jpegamd, oracle, dev):
    import jpegamd.progressive_script as ps
    rgbs = gs.pictures(jpegamd, 24, 40, 2, seed=4)
    t = torch.from_numpy(np.stack(rgbs)).to(dev)
    want = [fx.model(oracle, r, 0, S420, fx.SPLIT).file for r in rgbs]
    assert ps.encode_tensor_batch(t, scans=fx.SPLIT) == want
    assert ps.encode_tensor(t[1], scans=ps.parse_scan_script(fx.libjpeg_text(fx.SPLIT))) == want[1]
    assert ps.encode_tensor_batch(t) == [cm.memo(psm.rgb_file, oracle, r, 0, S420).file for r in rgbs]
    y, cb, cr = ms.derived_planes(gs.synth_rgb(jpegamd, 24, 40, 8, 0), S422)
    files = ps.encode_ycbcr_batch(torch.from_numpy(y[None]).to(dev), torch.from_numpy(cb[None]).to(dev), torch.from_numpy(cr[None]).to(dev),
                                  subsampling=S422, scans=fx.Y_CB)
    assert files == [cm.memo(scm.ycbcr_file, oracle, y, cb, cr, 0, S422, scm._key(fx.Y_CB)).file]
    planes = [fx.gray_plane(24, 40, 3), fx.gray_plane(24, 40, 4)]
    g = torch.from_numpy(np.stack(planes)).to(dev)
    assert ps.encode_gray_batch(g) == [fx.gray_model(oracle, p, 0, fx.GRAY_SUCCESSIVE).file for p in planes]
    assert ps.encode_gray(g[1], quality=60, scans=fx.GRAY_SPLIT) == fx.gray_model(oracle, planes[1], 60, fx.GRAY_SPLIT).file
    with pytest.raises(jpegamd.JpegAmdError):
        ps.encode_tensor_batch(t, scans=[(fx.ALL, 0, 5, 0, 0)])
