"""Caller-supplied quantisation tables on the GPU (jpegamd_encoder_set_quant_tables).  No kernel changed for them: what
is settled here is that nothing in the pipeline depended on the tables being Annex K shaped, and that the context's caches of constants
and headers follow the tables.  Every comparison is byte or pixel equality -- against the quality-driven models for tables equal to a
quality's (every entry family), against tests/qtables_model.py for tables outside the family, or against another file of the library
that the model has verified.  Every test needs an MI355X."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import color_model as cm
import gpu_support as gs
import gray_scan_fixtures as gf
import huffman_model as hm
import interleaved_model as im
import mjpeg_support as ms
import progressive_model as pm
import progressive_runs_model as prm
import progressive_script_fixtures as fx
import progressive_successive_model as psm
import qtables_fixtures as qx
import qtables_model as qtm
import quant_model as qm
import scan_model as sm
from gpu_support import CBCR, PLANES, S420, S422, S444, YUYV, dev  # noqa: F401

torch = gs.torch
pytestmark = pytest.mark.gpu
ERR_ARG = -1
W, H = 72, 40                                                   # 9 x 5 blocks: a partial MCU at 4:2:0
Q_UNUSED = 37                                                   # the pictures' own quality while tables are set: it selects nothing
ROW = {sub: im.row_interval(W, sub) for sub in (S444, S420, S422)}


@pytest.fixture(scope="module")
def enc(jpegamd, dev):
    e = jpegamd.Encoder(2056, gs.rows_for(3, H))
    yield e
    e.set_quant_tables(None)
    e.close()


@pytest.fixture(scope="module")
def pics():
    """Colour pictures by name, and their luma as the grayscale entries' planes."""
    rgb = {"photo": cm.synth_rgb(W, H, 11, 0), "noise": cm.synth_rgb(W, H, 12, 1), "extreme": qx.extreme_rgb(W, H), "photo2": cm.synth_rgb(W, H, 13, 0),
           "small": cm.synth_rgb(9, 9, 14, 1)}
    gray = {k: np.ascontiguousarray(sm.luma_plane(v)) for k, v in rgb.items()}
    gray["extreme"] = qx.extreme(W, H)
    return rgb, gray


# ---- calls ------------------------------------------------------------------------------------------------------------------------------
def rgb_images(jpegamd, rgbs, dev, q=Q_UNUSED):
    h, w, _ = rgbs[0].shape
    keep = [gs.upload(gs.stored_rows(r, False), dev, 3 * w) for r in rgbs]
    return keep, [jpegamd.Encoder.image(ptr, w, h, 3 * w, False, jpegamd.ORDER_RGB, q) for _, ptr in keep]


def gray_images(jpegamd, planes, dev, q=Q_UNUSED):
    h, w = planes[0].shape
    keep = [gs.upload(p, dev, w) for p in planes]
    return keep, [jpegamd.Encoder.image(ptr, w, h, w, False, jpegamd.ORDER_GRAY, q) for _, ptr in keep]


def queue(dev, n, cap, call):
    """Guarded outputs of `cap` bytes and call(out_ptrs, cap, size_ptrs, stream) queued on them -> the Outputs."""
    o = gs.Outputs(dev, n, cap)
    call(o.out_ptrs, o.cap, o.size_ptrs, gs.stream())
    return o


def run(enc, dev, n, cap, call):
    return gs.finish_files(enc, queue(dev, n, cap, call))


def gray_fused(jpegamd, enc, planes, dev, q=Q_UNUSED):
    """jpegamd_encode_async for one plane, jpegamd_encode_batch_async for more."""
    h, w = planes[0].shape
    keep, imgs = gray_images(jpegamd, planes, dev, q)
    if len(planes) == 1:
        return run(enc, dev, 1, jpegamd.max_jfif_bytes(w, h), lambda o, cap, s, st: enc.encode_async(imgs[0], o[0], cap, s[0], True, st))
    return run(enc, dev, len(planes), jpegamd.max_jfif_bytes(w, h), lambda o, cap, s, st: enc.encode_batch_async(imgs, o, cap, s, True, st))


def three_scan(jpegamd, enc, rgbs, dev, sub, q=Q_UNUSED):
    return gs.finish_files(enc, gs.ColorBatch(jpegamd, enc, rgbs, dev, sub, quality=q))


def one_scan(jpegamd, enc, rgbs, dev, sub, ri=0, q=Q_UNUSED):
    return gs.finish_files(enc, ms.OldRgbCall(jpegamd, enc, rgbs, dev, sub, ri, q))


def gray_scan(jpegamd, enc, planes, dev, ri, optimized, q=Q_UNUSED):
    h, w = planes[0].shape
    keep, imgs = gray_images(jpegamd, planes, dev, q)
    enc.set_huffman(jpegamd.HUFFMAN_OPTIMIZED if optimized else jpegamd.HUFFMAN_STANDARD)
    try:
        return run(enc, dev, len(planes), jpegamd.max_jfif_bytes_gray_scan(w, h, ri),
                   lambda o, cap, s, st: enc.encode_gray_scan_batch_async(imgs, ri, o, cap, s, st))
    finally:
        enc.set_huffman(jpegamd.HUFFMAN_STANDARD)


def optimized_one_scan(jpegamd, enc, rgbs, dev, sub, ri=0, q=Q_UNUSED):
    enc.set_huffman(jpegamd.HUFFMAN_OPTIMIZED)
    try:
        return one_scan(jpegamd, enc, rgbs, dev, sub, ri, q)
    finally:
        enc.set_huffman(jpegamd.HUFFMAN_STANDARD)


PROGRESSIVE = {"spectral": ("encode_color_progressive_batch_async", "max_jfif_bytes_progressive"),
               "optimized": ("encode_color_progressive_optimized_batch_async", "max_jfif_bytes_progressive_optimized"),
               "successive": ("encode_color_progressive_successive_batch_async", "max_jfif_bytes_progressive_successive")}


def progressive(jpegamd, enc, rgbs, dev, sub, kind, q=Q_UNUSED):
    h, w, _ = rgbs[0].shape
    keep, imgs = rgb_images(jpegamd, rgbs, dev, q)
    method, bound = PROGRESSIVE[kind]
    return run(enc, dev, len(rgbs), getattr(jpegamd, bound)(w, h, sub), lambda o, cap, s, st: getattr(enc, method)(imgs, sub, o, cap, s, st))


def scripted(jpegamd, enc, rgbs, dev, sub, script, q=Q_UNUSED):
    h, w, _ = rgbs[0].shape
    keep, imgs = rgb_images(jpegamd, rgbs, dev, q)
    return run(enc, dev, len(rgbs), jpegamd.max_jfif_bytes_progressive_script(w, h, sub, script),
               lambda o, cap, s, st: enc.encode_color_progressive_script_batch_async(imgs, sub, script, o, cap, s, st))


def scripted_gray(jpegamd, enc, planes, dev, script, q=Q_UNUSED):
    h, w = planes[0].shape
    keep, imgs = gray_images(jpegamd, planes, dev, q)
    return run(enc, dev, len(planes), jpegamd.max_jfif_bytes_progressive_script(w, h, 0, script),
               lambda o, cap, s, st: enc.encode_gray_progressive_script_batch_async(imgs, script, o, cap, s, st))


class Matrix:
    """An Encoder as gpu_support.YccBatch sees it: every YCbCr call goes to the three-scan entry with this matrix."""

    def __init__(self, enc, matrix):
        self.enc, self.matrix = enc, matrix

    def encode_ycbcr_batch_async(self, imgs, subsampling, out_ptrs, out_cap, size_ptrs, stream=0, sample_range=0, sample_format=0):
        self.enc.encode_ycbcr_batch_async(imgs, subsampling, out_ptrs, out_cap, size_ptrs, stream, sample_range, sample_format, self.matrix)


def ycc_kind(jpegamd, enc, kind, planes, dev, sub, layout, q=Q_UNUSED):
    """Stored planes of a mjpeg_support.Kind through the three-scan YCbCr entries."""
    rng, fmt, matrix = kind.args(jpegamd)
    return gs.finish_files(enc, gs.YccBatch(jpegamd, Matrix(enc, matrix), planes, dev, sub, layout, quality=q, sample_range=rng, sample_format=fmt))


def rows_then_finalize(jpegamd, enc, plane, dev, split, q=Q_UNUSED):
    """jpegamd_encode_rows_async over the block rows [0, split) and [split, end), then jpegamd_finalize_async."""
    h, w = plane.shape
    keep, (img,) = gray_images(jpegamd, [plane], dev, q)
    enc.encode_rows_async(img, 0, split, gs.stream())
    enc.encode_rows_async(img, split, (h + 7) // 8, gs.stream())
    return run(enc, dev, 1, jpegamd.max_jfif_bytes(w, h), lambda o, cap, s, st: enc.finalize_async(img, o[0], cap, s[0], True, st))


def flags_of(jpegamd, oracle, plane, table, q):
    return int(qm.plane_model(jpegamd, oracle, plane, table, q).flags.sum())


# ---- 1. equivalence: the tables of a quality through every entry family ------------------------------------------------------------------------
def fam_gray_single(j, o, e, d, rgb, gray, q):
    files, st = gray_fused(j, e, [gray["photo"]], d)
    return files, [cm.memo(cm.gray_file, o, gray["photo"], q)], st, dict(exact_fallbacks=flags_of(j, o, gray["photo"], "luma", q))


def fam_gray_batch(j, o, e, d, rgb, gray, q):
    planes = [gray["photo"], gray["noise"]]
    files, st = gray_fused(j, e, planes, d)
    return files, [cm.memo(cm.gray_file, o, p, q) for p in planes], st, dict(exact_fallbacks=sum(flags_of(j, o, p, "luma", q) for p in planes))


def three_scan_flags(j, o, rgbs, sub, q):
    return sum(flags_of(j, o, np.ascontiguousarray(p), "chroma" if k else "luma", q) for r in rgbs for k, p in enumerate(sm.planes_of(r, sub)))


def fam_color_single(sub):
    def fam(j, o, e, d, rgb, gray, q):
        files, st = gs.finish_files(e, gs.ColorCall(j, e, rgb["photo"], d, sub, quality=Q_UNUSED))
        return files, [gs.model(o, rgb["photo"], q, sub)], st, dict(exact_fallbacks=three_scan_flags(j, o, [rgb["photo"]], sub, q))
    return fam


def fam_color_batch(sub):
    def fam(j, o, e, d, rgb, gray, q):
        rgbs = [rgb["photo"], rgb["noise"]]
        files, st = three_scan(j, e, rgbs, d, sub)
        return files, [gs.model(o, r, q, sub) for r in rgbs], st, dict(exact_fallbacks=three_scan_flags(j, o, rgbs, sub, q))
    return fam


def fam_planar(j, o, e, d, rgb, gray, q):
    r = rgb["photo"]
    keep = [gs.upload(np.ascontiguousarray(r[:, :, k]), d, W) for k in range(3)]
    imgs = [j.Encoder.planar_image(tuple(p for _, p in keep), W, H, W, False, Q_UNUSED)]
    files, st = run(e, d, 1, j.max_jfif_bytes_color(W, H, S420), lambda out, cap, s, stream: e.encode_planar_batch_async(imgs, S420, out, cap, s, stream))
    return files, [gs.model(o, r, q, S420)], st, {}


def fam_ycc(sub, layout, kind=ms.FULL8):
    def fam(j, o, e, d, rgb, gray, q):
        planes = ms.stored_planes(kind, W, H, sub, 21)
        files, st = ycc_kind(j, e, kind, [planes], d, sub, layout)
        return files, [gs.ycc_file(o, ms.mapped_planes(kind, planes, sub), q, sub)], st, {}
    return fam


def fam_one_scan(ri_of=lambda sub: 0, source="rgb", optimized=False):
    def fam(j, o, e, d, rgb, gray, q):
        sub, ri = S420, ri_of(S420)
        if source == "ycc":
            planes = gs.smooth_planes(W, H, sub, 22)
            files, st = gs.finish_files(e, ms.OldYccCall(j, e, [planes], d, sub, PLANES, ri, Q_UNUSED))
            m = ms.ycc_model(o, planes, q, sub, ri)
        elif optimized:
            files, st = optimized_one_scan(j, e, [rgb["photo"]], d, sub, ri)
            m = cm.memo(hm.rgb_file, o, rgb["photo"], q, sub, ri)
        else:
            files, st = one_scan(j, e, [rgb["photo"]], d, sub, ri)
            m = ms.rgb_model(o, rgb["photo"], q, sub, ri)
        return files, [m.file], st, dict(entropy_bits=m.scan_bits, stuffed_bytes=m.stuffed)
    return fam


def fam_gray_scan(ri, optimized):
    def fam(j, o, e, d, rgb, gray, q):
        files, st = gray_scan(j, e, [gray["photo"]], d, ri, optimized)
        m = gf.model(o, gray["photo"], q, ri, optimized)
        return files, [m.file], st, dict(entropy_bits=m.scan_bits, stuffed_bytes=m.stuffed)
    return fam


def fam_progressive(kind):
    model = {"spectral": pm.progressive_file, "optimized": prm.rgb_file, "successive": psm.rgb_file}[kind]

    def fam(j, o, e, d, rgb, gray, q):
        files, st = progressive(j, e, [rgb["photo"]], d, S420, kind)
        m = cm.memo(model, o, rgb["photo"], q, S420)
        return files, [m.file], st, dict(entropy_bits=m.bits, stuffed_bytes=sum(m.stuffed))
    return fam


def fam_script_colour(j, o, e, d, rgb, gray, q):
    files, st = scripted(j, e, [rgb["photo"]], d, S420, fx.SPLIT)
    m = fx.model(o, rgb["photo"], q, S420, fx.SPLIT)
    return files, [m.file], st, dict(entropy_bits=m.bits, stuffed_bytes=sum(m.stuffed))


def fam_script_gray(j, o, e, d, rgb, gray, q):
    files, st = scripted_gray(j, e, [gray["photo"]], d, None)
    m = fx.gray_model(o, gray["photo"], q, fx.GRAY_SUCCESSIVE)
    return files, [m.file], st, dict(entropy_bits=m.bits, stuffed_bytes=sum(m.stuffed))


def fam_rows(j, o, e, d, rgb, gray, q):
    files, st = rows_then_finalize(j, e, gray["photo"], d, 2)
    return files, [cm.memo(cm.gray_file, o, gray["photo"], q)], st, {}


FAMILIES = {
    "encode_async": fam_gray_single, "encode_batch_async": fam_gray_batch,
    "color_444": fam_color_single(S444), "color_420": fam_color_single(S420), "color_422": fam_color_single(S422),
    "color_batch_444": fam_color_batch(S444), "color_batch_420": fam_color_batch(S420), "color_batch_422": fam_color_batch(S422),
    "planar": fam_planar,
    "ycbcr_planes": fam_ycc(S420, PLANES), "nv12": fam_ycc(S420, CBCR), "yuyv": fam_ycc(S422, YUYV),
    "limited_range": fam_ycc(S420, PLANES, ms.LIMITED8), "msb10": fam_ycc(S420, CBCR, ms.MSB10), "bt709": fam_ycc(S420, PLANES, ms.FULL8_709),
    "one_scan_rgb": fam_one_scan(), "one_scan_ycbcr": fam_one_scan(source="ycc"), "one_scan_row": fam_one_scan(lambda sub: ROW[sub]),
    "one_scan_optimized": fam_one_scan(optimized=True),
    "gray_scan_interval": fam_gray_scan(9, False), "gray_scan_optimized": fam_gray_scan(0, True),
    "progressive": fam_progressive("spectral"), "progressive_optimized": fam_progressive("optimized"),
    "progressive_successive": fam_progressive("successive"), "script_colour": fam_script_colour, "script_gray": fam_script_gray,
    "rows_finalize": fam_rows,
}


@pytest.mark.parametrize("q", (10, 90))
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_the_tables_of_a_quality_write_the_file_of_that_quality(jpegamd, oracle, dev, enc, pics, family, q):
    """With the tables of jpegamd_quant_tables_for_quality(q) set and the pictures' own quality at 37, every entry writes the file its
    model gives for quality q, and reports that file's counters."""
    rgb, gray = pics
    enc.set_quant_tables(*jpegamd.quant_tables_for_quality(q))
    try:
        files, want, st, counters = FAMILIES[family](jpegamd, oracle, enc, dev, rgb, gray, q)
    finally:
        enc.set_quant_tables(None)
    assert [len(f) for f in files] == [len(m) for m in want]
    assert files == want
    for name, value in counters.items():
        assert getattr(st, name) == value, (name, getattr(st, name), value)


# ---- 2. tables outside the family, byte for byte -------------------------------------------------------------------------------------------
def custom_models(oracle, rgb, plane, lq, cq):
    """The five files of test 2 by the model: fused gray, three scans at 4:2:0 and 4:4:4, one scan at 4:2:0 without and with intervals."""
    return {"gray": qtm.array(qtm.gray_file, oracle, plane, lq),
            "three_420": qtm.array(qtm.rgb_color_file, oracle, rgb, lq, cq, S420), "three_444": qtm.array(qtm.rgb_color_file, oracle, rgb, lq, cq, S444),
            "one_420": qtm.array(qtm.rgb_one_scan_file, oracle, rgb, lq, cq, S420, 0),
            "one_420_row": qtm.array(qtm.rgb_one_scan_file, oracle, rgb, lq, cq, S420, ROW[S420])}


def custom_files(jpegamd, enc, dev, rgb, plane):
    return {"gray": gray_fused(jpegamd, enc, [plane], dev)[0][0],
            "three_420": three_scan(jpegamd, enc, [rgb], dev, S420)[0][0], "three_444": three_scan(jpegamd, enc, [rgb], dev, S444)[0][0],
            "one_420": one_scan(jpegamd, enc, [rgb], dev, S420)[0][0], "one_420_row": one_scan(jpegamd, enc, [rgb], dev, S420, ROW[S420])[0][0]}


@pytest.mark.parametrize("name", sorted(qx.PAIRS))
def test_arbitrary_tables_byte_for_byte(jpegamd, oracle, dev, enc, pics, name):
    rgb, gray = pics
    lq, cq = qx.both(qx.PAIRS[name])
    enc.set_quant_tables(*qx.PAIRS[name])                        # (luma_only: chroma None -- one table for all components)
    try:
        held = enc.quant_tables()
        assert np.array_equal(held[0], lq) and np.array_equal(held[1], cq)
        for pic in ("photo", "noise", "extreme"):
            got = custom_files(jpegamd, enc, dev, rgb[pic], gray[pic])
            want = custom_models(oracle, rgb[pic], gray[pic], lq, cq)
            for key in want:
                assert len(got[key]) == len(want[key]) and got[key] == want[key], (name, pic, key)
    finally:
        enc.set_quant_tables(None)
    if name == "split":                                          # the luma and the chroma constants are not swapped: the swap is another file
        assert want["three_420"] != qtm.array(qtm.rgb_color_file, oracle, rgb["extreme"], cq, lq, S420)


# ---- 3. tables outside the family, the files the model does not build ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("checker", "random", "split"))
def test_arbitrary_tables_in_the_other_files(jpegamd, oracle, dev, enc, pics, name):
    """The optimised, gray-scan and progressive files carry exactly these tables and decode to the very pixels of the standard one-scan
    file (gray: of the fused file) that test 2 pins to the model: the coefficients are the same, and so is the decoder."""
    rgb, gray = pics
    r, p = rgb["photo"], gray["photo"]
    lq, cq = qx.both(qx.PAIRS[name])
    enc.set_quant_tables(lq, cq)
    try:
        colour = {"optimized": optimized_one_scan(jpegamd, enc, [r], dev, S420)[0][0],
                  "spectral": progressive(jpegamd, enc, [r], dev, S420, "spectral")[0][0],
                  "runs": progressive(jpegamd, enc, [r], dev, S420, "optimized")[0][0],
                  "successive": progressive(jpegamd, enc, [r], dev, S420, "successive")[0][0],
                  "script": scripted(jpegamd, enc, [r], dev, S420, fx.SPLIT)[0][0]}
        grays = {"gray_scan": gray_scan(jpegamd, enc, [p], dev, 0, True)[0][0], "gray_script": scripted_gray(jpegamd, enc, [p], dev, None)[0][0]}
    finally:
        enc.set_quant_tables(None)
    want = qtm.decode(qtm.array(qtm.rgb_one_scan_file, oracle, r, lq, cq, S420, 0))
    assert want.shape == (H, W, 3)
    for key, f in colour.items():
        t = qtm.dqt_tables(f)
        assert sorted(t) == [0, 1] and np.array_equal(t[0], lq) and np.array_equal(t[1], cq), (name, key)
        assert np.array_equal(qtm.decode(f), want), (name, key)
    want = qtm.decode(qtm.array(qtm.gray_file, oracle, p, lq))
    assert want.shape == (H, W)
    for key, f in grays.items():
        t = qtm.dqt_tables(f)
        assert sorted(t) == [0] and np.array_equal(t[0], lq), (name, key)
        assert np.array_equal(qtm.decode(f), want), (name, key)


# ---- 4. the quantiser's decisions --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def decision_plane():
    """256 blocks of noise over three block rows of `extreme`."""
    return np.ascontiguousarray(np.vstack([np.random.default_rng(31).integers(0, 256, (64, 256), np.uint8), qx.extreme(256, 24)]))


@pytest.mark.parametrize("name", ("ones", "max", "checker_a", "random1"))
def test_quantiser_decisions(jpegamd, oracle, dev, enc, decision_plane, name):
    table = qx.SINGLES[name]
    plane = decision_plane
    h, w = plane.shape
    blocks = qm.plane_blocks(plane)
    n = len(blocks)
    want_zz = oracle.quantise_blocks(oracle.dct_blocks(blocks.reshape(n, 8, 8).astype(np.int8)), table)
    assert np.array_equal(want_zz, sm.plane_zigzag(oracle, plane, table))
    m = qtm.decisions(jpegamd, blocks, table)
    enc.set_quant_tables(table)
    try:
        t, ptr = gs.upload(plane, dev, w)
        zz = torch.zeros(n * 64, dtype=torch.int16, device=dev)
        mask = torch.zeros(n, dtype=torch.int64, device=dev)
        enc.debug_stages(jpegamd.Encoder.image(ptr, w, h, w, False, jpegamd.ORDER_GRAY, Q_UNUSED), 0, zz.data_ptr(), mask.data_ptr())
        got_zz, got_mask = zz.cpu().numpy().reshape(n, 64), mask.cpu().numpy().view(np.uint64)
        files, st = gray_fused(jpegamd, enc, [plane], dev)
    finally:
        enc.set_quant_tables(None)
    bad = np.nonzero((got_zz != want_zz).any(axis=1))[0]
    assert not len(bad), (name, "blocks whose coefficients differ", bad[:8].tolist())
    bad = np.nonzero(got_mask != m.mask)[0]
    assert not len(bad), (name, "blocks whose flagged set differs", [(int(i), hex(int(got_mask[i])), hex(int(m.mask[i]))) for i in bad[:8]])
    assert st.exact_fallbacks == int(m.flags.sum()), (name, st.exact_fallbacks, int(m.flags.sum()))
    assert files == [qtm.array(qtm.gray_file, oracle, plane, table)]


def test_fused_gray_with_a_second_segment(jpegamd, oracle, dev, enc):
    """2056 x 8: 257 blocks, so the fused entry's second segment, under tables outside the family."""
    plane = np.ascontiguousarray(np.hstack([np.random.default_rng(32).integers(0, 256, (8, 1024), np.uint8), qx.extreme(1032, 8)]))
    assert plane.shape == (8, 2056)
    for name in ("ones", "checker_b", "random1"):
        enc.set_quant_tables(qx.SINGLES[name])
        try:
            files, _ = gray_fused(jpegamd, enc, [plane], dev)
        finally:
            enc.set_quant_tables(None)
        assert files == [qtm.array(qtm.gray_file, oracle, plane, qx.SINGLES[name])], name


# ---- 5. caches and state -------------------------------------------------------------------------------------------------------------------
def step_files(jpegamd, enc, dev, rgb, plane, q=50):
    """One call each through the three header caches: fused gray, three scans, one scan."""
    return {"gray": gray_fused(jpegamd, enc, [plane], dev, q)[0][0], "three_420": three_scan(jpegamd, enc, [rgb], dev, S420, q)[0][0],
            "one_420": one_scan(jpegamd, enc, [rgb], dev, S420, 0, q)[0][0]}


def step_models(oracle, rgb, plane, tables, q=50):
    if tables is None:
        return {"gray": cm.memo(cm.gray_file, oracle, plane, q), "three_420": gs.model(oracle, rgb, q, S420), "one_420": ms.rgb_model(oracle, rgb, q, S420).file}
    lq, cq = qx.both(tables)
    m = custom_models(oracle, rgb, plane, lq, cq)
    return {k: m[k] for k in ("gray", "three_420", "one_420")}


def test_one_context_follows_every_switch(jpegamd, oracle, dev, pics):
    """quality 50 -> A -> B -> reset -> quality 50 -> A at one geometry, then A at a second geometry and at the first again, gray,
    three-scan and one-scan calls interleaved at every step: every file is its model's."""
    rgb, gray = pics
    a, b = qx.PAIRS["checker"], qx.PAIRS["split"]
    e = jpegamd.Encoder(W, H)
    try:
        steps = [(None, "photo"), (a, "photo"), (b, "photo"), (None, "photo"), (a, "photo"), (a, "small"), (a, "photo"), (b, "small"), (None, "small")]
        for i, (tables, pic) in enumerate(steps):
            if tables is None:
                e.set_quant_tables(None)
                assert e.quant_tables() is None
            else:
                e.set_quant_tables(*tables)
            got = step_files(jpegamd, e, dev, rgb[pic], gray[pic])
            want = step_models(oracle, rgb[pic], gray[pic], tables)
            for key in want:
                assert got[key] == want[key], (i, pic, key)
        # the same tables set again are a new key all the same: nothing stale, nothing lost
        e.set_quant_tables(*a)
        e.set_quant_tables(*a)
        assert step_files(jpegamd, e, dev, rgb["photo"], gray["photo"]) == step_models(oracle, rgb["photo"], gray["photo"], a)
    finally:
        e.close()


def test_quality_changes_while_tables_are_set_select_nothing(jpegamd, oracle, dev, pics):
    rgb, gray = pics
    a = qx.PAIRS["random"]
    e = jpegamd.Encoder(W, H)
    try:
        e.set_quant_tables(*a)
        want = step_models(oracle, rgb["photo"], gray["photo"], a)
        for q in (10, 90, 0):
            assert step_files(jpegamd, e, dev, rgb["photo"], gray["photo"], q) == want, q
        e.set_quant_tables(None)
        assert step_files(jpegamd, e, dev, rgb["photo"], gray["photo"], 90) == step_models(oracle, rgb["photo"], gray["photo"], None, 90)
    finally:
        e.close()


def test_the_setter_does_not_disturb_queued_work(jpegamd, oracle, dev, pics):
    """Three encodes queued without a finish between them, the tables set, changed and taken off in between: every file is correct."""
    rgb, gray = pics
    a, b = qx.CHECKER_A, qx.RANDOM(1)
    big = np.ascontiguousarray(np.tile(gray["noise"], (4, 4)))    # (enough work to be still running when the setter is called)
    h, w = big.shape
    e = jpegamd.Encoder(w, h)
    try:
        cap = jpegamd.max_jfif_bytes(w, h)
        keep, (img,) = gray_images(jpegamd, [big], dev)
        e.set_quant_tables(a)
        first = queue(dev, 1, cap, lambda o, c, s, st: e.encode_async(img, o[0], c, s[0], True, st))
        e.set_quant_tables(b)
        second = queue(dev, 1, cap, lambda o, c, s, st: e.encode_async(img, o[0], c, s[0], True, st))
        e.set_quant_tables(None)
        third = queue(dev, 1, cap, lambda o, c, s, st: e.encode_async(img, o[0], c, s[0], True, st))
        e.finish()
        assert gs.intact_files(first) == [qtm.array(qtm.gray_file, oracle, big, a)]
        assert gs.intact_files(second) == [qtm.array(qtm.gray_file, oracle, big, b)]
        assert gs.intact_files(third) == [cm.memo(cm.gray_file, oracle, big, Q_UNUSED)]      # (back on quality: the picture's own)
    finally:
        e.close()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_keep_what_was_set(jpegamd, oracle, dev, pics):
    rgb, gray = pics
    lib = jpegamd.lib
    a_l, a_c = qx.SPLIT
    zero_l, zero_c = qx.RANDOM(8).copy(), qx.RANDOM(9).copy()
    zero_l[63], zero_c[0] = 0, 0
    good = qx.RANDOM(8)
    e = jpegamd.Encoder(W, H)

    def held():
        luma, chroma, custom = np.full(64, 7, np.uint8), np.full(64, 7, np.uint8), C.c_int32(-1)
        assert lib.jpegamd_encoder_get_quant_tables(e._h, luma.ctypes.data, chroma.ctypes.data, C.byref(custom)) == 0
        return luma, chroma, custom.value

    try:
        luma, chroma, custom = held()
        assert custom == 0 and (luma == 7).all() and (chroma == 7).all()          # quality-driven: the tables are untouched
        assert lib.jpegamd_encoder_set_quant_tables(e._h, zero_l.ctypes.data, None) == ERR_ARG
        assert held()[2] == 0
        e.set_quant_tables(a_l, a_c)
        for luma_arg, chroma_arg in ((zero_l, None), (zero_l, good), (good, zero_c), (None, good)):
            rc = lib.jpegamd_encoder_set_quant_tables(e._h, None if luma_arg is None else luma_arg.ctypes.data,
                                                      None if chroma_arg is None else chroma_arg.ctypes.data)
            assert rc == ERR_ARG
            luma, chroma, custom = held()
            assert custom == 1 and np.array_equal(luma, a_l) and np.array_equal(chroma, a_c)
        assert lib.jpegamd_encoder_get_quant_tables(e._h, None, None, None) == ERR_ARG
        with pytest.raises(ValueError):
            e.set_quant_tables(None, good)
        with pytest.raises(ValueError):
            e.set_quant_tables(zero_l)
        got = step_files(jpegamd, e, dev, rgb["photo"], gray["photo"])
        assert got == step_models(oracle, rgb["photo"], gray["photo"], (a_l, a_c))       # the next files are the kept tables'
        e.set_quant_tables(None)
        assert held()[2] == 0 and e.quant_tables() is None
    finally:
        e.close()


# ---- 7. the bounds -------------------------------------------------------------------------------------------------------------------------
def test_bounds_hold_under_the_all_ones_table(jpegamd, dev, enc, pics):
    """The finest table there is, on noise and on `extreme`: no file is longer than its bound (the outputs are exactly as long as the
    bounds, with guards behind them)."""
    rgb, gray = pics
    enc.set_quant_tables(qx.ONES)
    try:
        for pic in ("noise", "extreme"):
            r, p = rgb[pic], gray[pic]
            sizes = [(len(gray_fused(jpegamd, enc, [p], dev)[0][0]), jpegamd.max_jfif_bytes(W, H))]
            for sub in (S444, S420):
                sizes.append((len(three_scan(jpegamd, enc, [r], dev, sub)[0][0]), jpegamd.max_jfif_bytes_color(W, H, sub)))
                sizes.append((len(one_scan(jpegamd, enc, [r], dev, sub)[0][0]), jpegamd.max_jfif_bytes_interleaved(W, H, sub)))
                sizes.append((len(one_scan(jpegamd, enc, [r], dev, sub, ROW[sub])[0][0]), jpegamd.max_jfif_bytes_interleaved_restart(W, H, sub, ROW[sub])))
                sizes.append((len(progressive(jpegamd, enc, [r], dev, sub, "successive")[0][0]), jpegamd.max_jfif_bytes_progressive_successive(W, H, sub)))
            for got, bound in sizes:
                assert 0 < got <= bound, (pic, sizes)
            # (nothing is quantised away: noise keeps several bits a sample; `extreme` is mostly flat blocks and stays short)
            assert pic != "noise" or sizes[0][0] > W * H // 2
    finally:
        enc.set_quant_tables(None)


# ---- 8. the Python block -------------------------------------------------------------------------------------------------------------------
def test_the_block_governs_the_module_level_functions(jpegamd, oracle, dev, pics):
    import jpegamd.mjpeg
    import jpegamd.progressive_successive
    rgb, gray = pics
    a = qx.PAIRS["split"]
    lq, cq = qx.both(a)
    rgbs = [rgb["photo"], rgb["noise"]]
    t = torch.from_numpy(np.stack(rgbs)).to(dev)

    def calls():
        return (jpegamd.encode_tensor_batch(t), jpegamd.mjpeg.encode_tensor_batch(t, restart_interval="row"),
                jpegamd.progressive_successive.encode_tensor(t[0]), jpegamd.encode_tensor(t[0, :, :, 0].contiguous()))

    def by_quality(got):
        three, one, successive, fused = got
        assert three == [gs.model(oracle, r, 0, S420) for r in rgbs]
        assert one == [ms.rgb_model(oracle, r, 0, S420, ROW[S420]).file for r in rgbs]
        assert successive == cm.memo(psm.rgb_file, oracle, rgbs[0], 0, S420).file
        assert fused == cm.memo(cm.gray_file, oracle, np.ascontiguousarray(rgbs[0][:, :, 0]), 50)

    by_quality(calls())
    with jpegamd.quant_tables(*a):
        three, one, successive, fused = calls()
    assert three == [qtm.array(qtm.rgb_color_file, oracle, r, lq, cq, S420) for r in rgbs]
    assert one == [qtm.array(qtm.rgb_one_scan_file, oracle, r, lq, cq, S420, ROW[S420]) for r in rgbs]
    tables = qtm.dqt_tables(successive)
    assert np.array_equal(tables[0], lq) and np.array_equal(tables[1], cq)
    assert np.array_equal(qtm.decode(successive), qtm.decode(qtm.array(qtm.rgb_one_scan_file, oracle, rgbs[0], lq, cq, S420, 0)))
    assert fused == qtm.array(qtm.gray_file, oracle, np.ascontiguousarray(rgbs[0][:, :, 0]), lq)
    by_quality(calls())
    with pytest.raises(RuntimeError, match="left by exception"):
        with jpegamd.quant_tables(qx.MAX):
            assert jpegamd.encode_tensor_batch(t[:1]) == [qtm.array(qtm.rgb_color_file, oracle, rgbs[0], qx.MAX, qx.MAX, S420)]
            raise RuntimeError("left by exception")
    assert all(e.quant_tables() is None for e, _, _ in jpegamd._tensor_encoders.values())
    by_quality(calls())
