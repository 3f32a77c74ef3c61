"""Grayscale files with restart intervals and optimised Huffman tables on the GPU (jpegamd_encode_gray_scan_batch_async, DESIGN.md
4.6.11): every device file is compared byte for byte with the CPU model (tests/gray_scan_model.py).  tests/test_gray_scan_host.py proves
on the CPU that the model without intervals is the oracle's file and that the pictures of tests/gray_scan_fixtures.py sit on the edges
the cases claim.  Every test needs an MI355X."""
from __future__ import annotations

import numpy as np
import pytest

import color_model as cm
import gpu_support as gs
import gray_scan_fixtures as gf
import gray_scan_model as gm
import huffman_fixtures as hf
import huffman_model as hm
import mjpeg_support as ms
import scan_model as sm
from gpu_support import dev  # noqa: F401

torch = gs.torch
pytestmark = pytest.mark.gpu
ERR_HUFF_CAPACITY = -8
SHAPES = gf.shapes()
GEOMETRY = ("1x1", "9x9", "72x40", "2040x8", "2048x8", "2056x8", "40x520")


@pytest.fixture(scope="module")
def enc(jpegamd, dev):
    e = jpegamd.Encoder(6400, gs.rows_for(3, 520))
    yield e
    e.close()


class GrayScanCall(gs.Outputs):
    """One batch through jpegamd_encode_gray_scan_batch_async: `rows` are the pictures' stored rows ([H, row bytes]) in `order`."""

    def __init__(self, jpegamd, enc, rows, w, h, dev, ri, q, order=None, bottom_up=False, stride=None, shift=0, cap=None):
        order = jpegamd.ORDER_GRAY if order is None else order
        stride = stride or rows[0].shape[1]
        self.px = [gs.upload(r, dev, stride, shift) for r in rows]
        super().__init__(dev, len(rows), cap if cap is not None else jpegamd.max_jfif_bytes_gray_scan(w, h, ri))
        imgs = [jpegamd.Encoder.image(ptr, w, h, stride, bottom_up, order, q) for _, ptr in self.px]
        enc.encode_gray_scan_batch_async(imgs, ri, self.out_ptrs, self.cap, self.size_ptrs, gs.stream())


def gray_files(jpegamd, enc, planes, dev, ri, q, optimized, **kw):
    """GRAY planes of one geometry through the entry in the given mode -> (files, Stats); the context is left in STANDARD."""
    h, w = planes[0].shape
    enc.set_huffman(jpegamd.HUFFMAN_OPTIMIZED if optimized else jpegamd.HUFFMAN_STANDARD)
    try:
        return gs.finish_files(enc, GrayScanCall(jpegamd, enc, [gs.stored_rows(p, False) for p in planes], w, h, dev, ri, q, **kw))
    finally:
        enc.set_huffman(jpegamd.HUFFMAN_STANDARD)


def check(jpegamd, oracle, enc, dev, planes, ri, q, optimized):
    models = [gf.model(oracle, p, q, ri, optimized) for p in planes]
    files, st = gray_files(jpegamd, enc, planes, dev, ri, q, optimized)
    for f, m in zip(files, models):
        assert f[:m.prefix_len] == m.file[:m.prefix_len], (ri, q, optimized)
        assert f == m.file, (ri, q, optimized)
    assert st.entropy_bits == sum(m.scan_bits for m in models) and st.stuffed_bytes == sum(m.stuffed for m in models), (ri, q, optimized)
    return models, files, st


# ---- 1. geometry x interval x mode ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", (50, 90))
@pytest.mark.parametrize("name", GEOMETRY)
def test_geometry_interval_and_mode(jpegamd, oracle, dev, enc, name, q):
    p = next(p for n, p, _ in SHAPES if n == name)
    wrapped = False
    for ri in gf.INTERVALS:
        ri = gf.interval(ri, p.shape[1])
        for opt in gf.MODES:
            (m,), _, _ = check(jpegamd, oracle, enc, dev, [p], ri, q, opt)
            wrapped |= m.markers > 8
    assert wrapped or name != "40x520"                              # RSTn wraps past D7


def test_no_intervals_and_standard_tables_is_the_grayscale_entry(jpegamd, oracle, dev):
    planes = [gf.synth_luma(200, 120, 3), gf.noise(200, 120, 4)]
    e = jpegamd.Encoder(200, gs.rows_for(2, 120))
    try:
        e.set_profiling(4)
        want, st_old = gs.encode_gray_planes(jpegamd, e, planes, dev, 75)
        old = e.profile(0)
        files, st = gray_files(jpegamd, e, planes, dev, 0, 75, False)
        new = e.profile(1)
    finally:
        e.close()
    assert files == want == [cm.gray_file(oracle, p, 75) for p in planes]
    for field in ("jfif_bytes", "entropy_bits", "stuffed_bytes", "exact_fallbacks"):
        assert getattr(st, field) == getattr(st_old, field), field
    for field, _ in jpegamd.Stats._fields_:                          # the same profiling fields are filled
        if field.startswith("ns_"):
            assert (getattr(new, field) > 0) == (getattr(old, field) > 0), field


@pytest.mark.parametrize("name", GEOMETRY + ("128x128",))
def test_one_interval_is_the_grayscale_entrys_file_with_dri(jpegamd, oracle, dev, enc, name):
    """The coefficient route against reference-verified bytes: the file of jpegamd_encode_async with the DRI segment inserted."""
    p, q = next((p, q) for n, p, q in SHAPES if n == name)
    ref = gs.encode_gray(jpegamd, enc, p, dev, quality=q)
    assert ref == cm.gray_file(oracle, p, q)
    blocks = gm.block_count(p.shape[1], p.shape[0])
    for ri in sorted({blocks, 65535}):
        (f,), st = gray_files(jpegamd, enc, [p], dev, ri, q, False)
        assert f == gm.with_dri(ref, ri), ri


# ---- 2. sources -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("optimized", gf.MODES)
def test_every_order_row_order_and_a_padded_stride(jpegamd, oracle, dev, enc, optimized):
    w, h, q, ri = 72, 40, 75, 5
    rgb = hf.synth_rgb(w, h, 21)
    y = sm.luma_plane(rgb)
    want = gf.model(oracle, y, q, ri, optimized).file
    enc.set_huffman(jpegamd.HUFFMAN_OPTIMIZED if optimized else jpegamd.HUFFMAN_STANDARD)
    try:
        for bottom_up in (False, True):
            sources = {jpegamd.ORDER_GRAY: gs.stored_rows(y, bottom_up), jpegamd.ORDER_RGB: gs.stored_rows(rgb, bottom_up),
                       jpegamd.ORDER_BGR: gs.stored_rows(rgb, bottom_up, True), jpegamd.ORDER_RGBA: ms.px4_rows(rgb, bottom_up, False),
                       jpegamd.ORDER_BGRA: ms.px4_rows(rgb, bottom_up, True)}
            for order, rows in sources.items():
                for stride, shift in ((None, 0), (rows.shape[1] + 13, 3)):
                    call = GrayScanCall(jpegamd, enc, [rows], w, h, dev, ri, q, order, bottom_up, stride, shift)
                    (f,), _ = gs.finish_files(enc, call)
                    assert f == want, (order, bottom_up, stride)
    finally:
        enc.set_huffman(jpegamd.HUFFMAN_STANDARD)


# ---- 3. a batch: tables, counts, statistics -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ri", (0, 5))
def test_batch_of_three_tables_counts_and_statistics(jpegamd, oracle, dev, enc, ri):
    planes = gf.batch_of_three()
    _, st_gray = gs.encode_gray_planes(jpegamd, enc, planes, dev, 75)
    for opt in gf.MODES:
        if not opt and not ri:
            continue                                                 # (the grayscale entry itself: tested above)
        models, files, st = check(jpegamd, oracle, enc, dev, planes, ri, 75, opt)
        assert st.exact_fallbacks == st_gray.exact_fallbacks
        if opt:
            assert len({m.prefix_len for m in models}) == 3 and len({repr(m.tables) for m in models}) == 3
            counts = np.zeros((3, 4, 256), np.uint64)
            assert jpegamd.lib.jpegamd_debug_huffman_counts(enc._h, counts.ctypes.data) == 0
            for c, m in zip(counts, models):
                assert (c[:2].astype(np.int64) == m.counts).all() and not c[2:].any(), ri


def test_exact_fallbacks_are_the_grayscale_entrys(jpegamd, oracle, dev, enc):
    p = gf.noise(128, 128, 7)                                         # noise at quality 100: coefficients near the rounding edge
    _, st_gray = gs.encode_gray_planes(jpegamd, enc, [p], dev, 100)
    for ri, opt in ((16, False), (0, True)):
        _, _, st = check(jpegamd, oracle, enc, dev, [p], ri, 100, opt)
        assert st.exact_fallbacks == st_gray.exact_fallbacks


# ---- 4. the named fixtures ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", gf.FLAT)
def test_flat_pictures_and_their_shortest_segments(jpegamd, oracle, dev, enc, w, h):
    for ri in gf.FLAT_INTERVALS:
        for opt in gf.MODES:
            if not opt and not ri:
                continue
            (m,), _, _ = check(jpegamd, oracle, enc, dev, [gf.flat(w, h)], ri, 50, opt)
            if opt:
                assert [len(t[1]) for t in m.tables] == [1, 1]


def test_segments_of_two_to_five_bits(jpegamd, oracle, dev, enc):
    seen = set()
    for p in gf.STEPS:
        for ri in gf.STEP_INTERVALS:
            (m,), _, _ = check(jpegamd, oracle, enc, dev, [p], ri, 50, True)
            seen |= {b for s in m.segment_bits for b in s}
            check(jpegamd, oracle, enc, dev, [p], ri, 50, False)
    assert {2, 3, 4, 5} <= seen
    check(jpegamd, oracle, enc, dev, gf.STEPS, 1, 50, True)          # ... and as one batch


@pytest.mark.parametrize("name,ri", gf.PAD_FF)
def test_padded_bytes_that_come_out_ff_and_aligned_intervals(jpegamd, oracle, dev, enc, name, ri):
    p, q = next((p, q) for n, p, q in SHAPES if n == name)
    for opt in gf.MODES:
        (m,), _, _ = check(jpegamd, oracle, enc, dev, [p], ri, q, opt)
        assert m.pad_ff >= 1 and m.aligned >= 1


def test_ff_byte_across_a_segment_boundary(jpegamd, oracle, dev, enc):
    p, q = gf.straddle()
    for opt in gf.MODES:
        (m,), _, _ = check(jpegamd, oracle, enc, dev, [p], 0, q, opt)
        assert m.straddle_ff >= 1
    check(jpegamd, oracle, enc, dev, [p], 300, q, False)              # the same boundary at the start of a byte, another inside


def test_short_tails_that_borrow_bits_of_the_segment_in_front(jpegamd, oracle, dev, enc):
    p, q = gf.tail_standard()
    (m,), _, _ = check(jpegamd, oracle, enc, dev, [p], 257, q, False)
    assert m.borrowed_tails >= 1
    (m,), _, _ = check(jpegamd, oracle, enc, dev, [np.ascontiguousarray(p[:, :2056])], 257, q, False)    # one interval: the flushed byte
    assert m.borrowed_tails == 1 and m.intervals == 1
    for blocks, ri in ((257, 0), (771, 257)):
        p, q = gf.tail_optimized(blocks)
        (m,), _, _ = check(jpegamd, oracle, enc, dev, [p], ri, q, True)
        assert m.borrowed_tails == m.intervals and m.min_segment_bits == 2


def test_segment_longer_than_the_coders_window(jpegamd, oracle, dev, enc):
    p, q = next((p, q) for n, p, q in SHAPES if n == gf.MULTI_ROUND)
    for ri, opt in ((0, True), (256, False), (256, True), (255, True), (1, True)):
        (m,), _, _ = check(jpegamd, oracle, enc, dev, [p], ri, q, opt)
        assert m.max_segment_bits > 65536 or ri == 1


@pytest.mark.parametrize("w,h,kind,seed,q", gf.LONG_CODES[:1])
def test_lengths_beyond_16_are_limited(jpegamd, oracle, dev, enc, w, h, kind, seed, q):
    p = gf.long_code_plane(w, h, kind, seed)
    (m,), _, _ = check(jpegamd, oracle, enc, dev, [p], 0, q, True)
    assert m.tables[1][2] > 16


# ---- 5. capacity ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ri,optimized", ((5, False), (0, True), (5, True)))
def test_buffer_one_byte_too_small(jpegamd, oracle, dev, enc, ri, optimized):
    planes = gf.batch_of_three()
    models = [gf.model(oracle, p, 75, ri, optimized) for p in planes]
    order = sorted(range(3), key=lambda i: -len(models[i].file))
    big = order[0]
    assert len(models[big].file) > len(models[order[1]].file)
    enc.set_huffman(jpegamd.HUFFMAN_OPTIMIZED if optimized else jpegamd.HUFFMAN_STANDARD)
    try:
        call = GrayScanCall(jpegamd, enc, [gs.stored_rows(p, False) for p in planes], 72, 40, dev, ri, 75, cap=len(models[big].file) - 1)
        with pytest.raises(jpegamd.JpegAmdError) as err:
            enc.finish()
    finally:
        enc.set_huffman(jpegamd.HUFFMAN_STANDARD)
    assert err.value.code == ERR_HUFF_CAPACITY
    sizes = call.sizes.cpu().tolist()
    files = gs.intact_files(call)                                    # nothing written past the capacity
    assert sizes[big] == 0
    for i in order[1:]:
        assert sizes[i] == len(models[i].file) and files[i] == models[i].file
    check(jpegamd, oracle, enc, dev, planes, ri, 75, optimized)      # the context is usable afterwards


# ---- 6. mode hygiene --------------------------------------------------------------------------------------------------------------------
def test_standard_after_optimized_is_todays_file(jpegamd, oracle, dev):
    p = gf.synth_luma(72, 40, 5)
    e = jpegamd.Encoder(512, 64)
    try:
        for ri in (0, 3):
            std = gf.model(oracle, p, 50, ri, False).file
            (before,), _ = gray_files(jpegamd, e, [p], dev, ri, 50, False)
            (opt,), _ = gray_files(jpegamd, e, [p], dev, ri, 50, True)
            (after,), _ = gray_files(jpegamd, e, [p], dev, ri, 50, False)
            assert before == after == std and opt == gf.model(oracle, p, 50, ri, True).file and len(opt) < len(std)
        assert gf.model(oracle, p, 50, 0, False).file == cm.gray_file(oracle, p, 50)
    finally:
        e.close()


def test_mjpeg_functions_leave_the_shared_context_in_standard(jpegamd, oracle, dev):
    import jpegamd.mjpeg as mj
    planes = gf.batch_of_three()
    t = torch.from_numpy(np.stack(planes)).to(dev)
    for ri in (None, 4, "row"):
        n = gf.interval(ri, 72) if ri else 0
        want = [gf.model(oracle, p, 50, n, True).file for p in planes]
        std = [gf.model(oracle, p, 50, n, False).file for p in planes]
        assert mj.encode_gray_batch(t, 50, restart_interval=ri, huffman="optimized") == want
        assert mj.encode_gray_batch(t, 50, restart_interval=ri) == std                     # the shared context is back in STANDARD
        assert mj.encode_gray(t[1], 50, restart_interval=ri, huffman="optimized") == want[1]
    assert jpegamd.encode_tensor_batch(t, 50) == [cm.gray_file(oracle, p, 50) for p in planes]
    wide = torch.zeros(3, 40, 96, dtype=torch.uint8, device=dev)
    wide[:, :, 8:80] = t
    assert mj.encode_gray_batch(wide[:, :, 8:80], 50, restart_interval=4) == [gf.model(oracle, p, 50, 4, False).file for p in planes]


def test_other_entries_on_the_same_context_keep_their_files(jpegamd, oracle, dev):
    """A one-scan colour call and a plain grayscale call before and after grayscale-scan calls of another geometry: the shared scratch
    is regrown for each."""
    rgb = hf.synth_rgb(72, 40, 31)
    p_small, p_big = gf.synth_luma(72, 40, 32), gf.noise(200, 120, 33)
    color = {opt: (hf.model(oracle, rgb, 50, hf.S420, 3).file if opt else hm.standard_file(oracle, rgb, 50, hf.S420, 3)) for opt in gf.MODES}
    e = jpegamd.Encoder(512, 256)
    try:
        def color_file(opt):
            e.set_huffman(jpegamd.HUFFMAN_OPTIMIZED if opt else jpegamd.HUFFMAN_STANDARD)
            try:
                return gs.finish_files(e, ms.PixelsCall(jpegamd, e, [rgb], dev, hf.S420, "rgb", 3, 50))[0][0]
            finally:
                e.set_huffman(jpegamd.HUFFMAN_STANDARD)
        for round_ in range(2):
            for opt in gf.MODES:
                assert color_file(opt) == color[opt]
            assert gs.encode_gray(jpegamd, e, p_small, dev, quality=50) == cm.gray_file(oracle, p_small, 50)
            check(jpegamd, oracle, e, dev, [p_small], 1, 50, True)
            check(jpegamd, oracle, e, dev, [p_big, p_big[::-1].copy()], 7, 90, round_ == 0)
            check(jpegamd, oracle, e, dev, [p_small], 0, 50, True)
    finally:
        e.close()


def test_table_kernel_with_two_jobs(jpegamd, dev, enc):
    tables = hf.count_tables()[:2]
    freq = np.ascontiguousarray(np.stack(tables), np.uint64)
    bits, vals, nvals = np.zeros((2, 16), np.uint8), np.zeros((2, 256), np.uint8), np.zeros(2, np.int32)
    assert jpegamd.lib.jpegamd_debug_optimal_huffman(enc._h, freq.ctypes.data, 2, bits.ctypes.data, vals.ctypes.data, nvals.ctypes.data) == 0
    for i, f in enumerate(tables):
        want_bits, want_vals, _ = hm.optimal_table(f)
        assert (bits[i].tolist(), vals[i, :nvals[i]].tolist()) == (want_bits, want_vals) and not vals[i, nvals[i]:].any()
