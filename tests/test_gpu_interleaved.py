"""Interleaved-MCU colour files on the GPU (jpegamd_encode_color_interleaved_batch_async, jpegamd_encode_ycbcr_interleaved_batch_async):
every device file is compared byte for byte with the CPU model (tests/interleaved_model.py).  The model's counters are asserted for
every property a case claims to exercise, so none passes vacuously."""
from __future__ import annotations

import io

import numpy as np
import pytest

import color_model as cm
import gpu_support as gs
import interleaved_model as im
import scan_model as sm
from gpu_support import CBCR, CRCB, PLANES, S420, S422, S444, dev  # noqa: F401

torch = gs.torch
pytestmark = pytest.mark.gpu
SUBS = (S444, S420, S422)
WINDOW_BITS = 2048 * 32                                         # k_mcu_segments' LDS window: a longer segment leaves in pieces


def model(oracle, rgb, q, sub):
    return cm.memo(im.interleaved_file, oracle, rgb, q, sub)


class RgbCall(gs.Outputs):
    """One interleaved RGB batch queued on `enc`."""

    def __init__(self, jpegamd, enc, rgbs, dev, sub, quality=0, bgr=False, bottom_up=False, stride=None, cap=None):
        h, w, _ = rgbs[0].shape
        stride = stride or 3 * w
        self.px = [gs.upload(gs.stored_rows(r, bottom_up, bgr), dev, stride) for r in rgbs]
        super().__init__(dev, len(rgbs), cap if cap is not None else jpegamd.max_jfif_bytes_interleaved(w, h, sub))
        order = jpegamd.ORDER_BGR if bgr else jpegamd.ORDER_RGB
        imgs = [jpegamd.Encoder.image(ptr, w, h, stride, bottom_up, order, quality) for _, ptr in self.px]
        enc.encode_color_interleaved_batch_async(imgs, sub, self.out_ptrs, self.cap, self.size_ptrs, gs.stream())


class YccCall(gs.Outputs):
    """One interleaved YCbCr batch queued on `enc`: planes stored `shift` bytes into their allocations, rows `stride` bytes apart."""

    def __init__(self, jpegamd, enc, planes, dev, sub, layout, quality=0, y_stride=None, c_stride=None, shift=0):
        h, w = planes[0][0].shape
        cw, ch = gs.chroma_dims(w, h, sub)
        y_stride = y_stride or w
        c_stride = c_stride or (cw if layout == PLANES else 2 * cw)
        self.keep, imgs = [], []
        for y, cb, cr in planes:
            ty, py = gs.upload(y, dev, y_stride, shift)
            ups = [gs.upload(rows, dev, c_stride, shift) for rows in cm.chroma_rows(cb, cr, layout)]
            self.keep.append((ty, ups))
            imgs.append(jpegamd.Encoder.ycbcr_image(py, ups[0][1], ups[1][1] if layout == PLANES else 0, w, h, y_stride, c_stride, layout, quality))
        super().__init__(dev, len(planes), jpegamd.max_jfif_bytes_interleaved(w, h, sub))
        enc.encode_ycbcr_interleaved_batch_async(imgs, sub, self.out_ptrs, self.cap, self.size_ptrs, gs.stream())


def derived_planes(rgb, sub):
    """(y, cb, cr) as the RGB entries derive them at `sub`."""
    return tuple(np.ascontiguousarray(p) for p in sm.planes_of(rgb, sub))


def rgb_files(jpegamd, enc, rgbs, dev, sub, q=0, **kw):
    return gs.finish_files(enc, RgbCall(jpegamd, enc, rgbs, dev, sub, q, **kw))


def decode(data: bytes) -> np.ndarray:
    image = pytest.importorskip("PIL.Image")
    with image.open(io.BytesIO(data)) as f:
        return np.asarray(f.convert("RGB"))


@pytest.fixture(scope="module")
def enc(jpegamd, dev):
    e = jpegamd.Encoder(512, gs.rows_for(32, 16))
    yield e
    e.close()


# ---- geometry -------------------------------------------------------------------------------------------------------------------------
GEOMETRY = [(1, 1), (8, 8), (16, 16), (17, 9), (24, 40), (257, 31), (200, 120)]
SEGMENTS = {(200, 120, S420): 3, (200, 120, S444): 5, (320, 280, S444): 17, (16, 16, S420): 1, (257, 31, S444): 2}
PADS = {(16, 16): (0, 0, 0), (17, 9): (0, 2, 2), (24, 40): (0, 9, 5)}      # pad blocks at 4:4:4 / 4:2:0 / 4:2:2


def expected_segments(w, h, sub):
    """From S = 256 // (blocks per MCU), as the issue states it."""
    hs, vs = im.sampling(sub)
    mcus = -(-w // (8 * hs)) * -(-h // (8 * vs))
    s = 256 // (hs * vs + 2)
    assert s == {S444: 85, S420: 42, S422: 64}[sub]
    return -(-mcus // s)


@pytest.mark.parametrize("w,h,sub", [(w, h, sub) for (w, h) in GEOMETRY for sub in SUBS] + [(320, 280, S444)])
def test_geometry(jpegamd, oracle, dev, enc, w, h, sub):
    rgb = gs.synth_rgb(jpegamd, w, h, 5 + w, 0)
    m = model(oracle, rgb, 50, sub)
    if (w, h, sub) in SEGMENTS:
        assert expected_segments(w, h, sub) == SEGMENTS[(w, h, sub)] == im.segment_count(w, h, sub)
    if (w, h) in PADS:
        assert m.pad_blocks == PADS[(w, h)][SUBS.index(sub)]
    (f,), st = rgb_files(jpegamd, enc, [rgb], dev, sub, 50)
    assert f == m.file
    assert st.entropy_bits == m.scan_bits and st.stuffed_bytes == m.stuffed


def test_seventeen_segments_pass_one_finalize_chunk():
    assert expected_segments(320, 280, S444) == 17 > 16           # k_finalize works on chunks of 16 segments
    mx = 200 // 16 + 1                                              # 200 x 120 at 4:2:0: 13 MCUs per row, segments of 42
    assert 42 % mx != 0 and 42 > mx                                 # a segment starts mid-row and spans MCU rows


@pytest.mark.parametrize("kw", [dict(bgr=True), dict(bottom_up=True), dict(bgr=True, bottom_up=True, stride=3 * 33 + 5)])
def test_stored_orders(jpegamd, oracle, dev, enc, kw):
    rgb = gs.synth_rgb(jpegamd, 33, 17, 9, 0)
    for sub in SUBS:
        (f,), _ = rgb_files(jpegamd, enc, [rgb], dev, sub, 50, **kw)
        assert f == model(oracle, rgb, 50, sub).file, (sub, kw)


# ---- content --------------------------------------------------------------------------------------------------------------------------
def checker_picture():
    """Isolated high-frequency coefficients: a pixel checkerboard in luma, a 2 x 2 one in chroma (it survives the chroma averaging)."""
    yy, xx = np.mgrid[0:32, 0:48]
    c1, c2 = ((xx + yy) & 1) * 2 - 1, (((xx // 2) + (yy // 2)) & 1) * 2 - 1
    r, g, b = 128 + 40 * c1 + 60 * c2, 128 + 40 * c1 - 30 * c2, 128 + 40 * c1 - 60 * c2
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


def block_checker():
    yy, xx = np.mgrid[0:32, 0:48]
    p = np.where(((xx // 8) + (yy // 8)) & 1, 255, 0).astype(np.uint8)
    return np.stack([p, p, p], axis=2)


@pytest.mark.parametrize("sub", SUBS)
def test_dense_noise(jpegamd, oracle, dev, enc, sub):
    rgb = np.random.default_rng(1).integers(0, 256, (64, 64, 3), np.uint8)
    m = model(oracle, rgb, 100, sub)
    assert im.segment_count(64, 64, sub) == 1 and m.no_eob_blocks > 0 and m.stuffed > 0
    if sub != S420:
        assert m.scan_bits > WINDOW_BITS                            # one segment, longer than the LDS window
    (f,), st = rgb_files(jpegamd, enc, [rgb], dev, sub, 100)
    assert f == m.file
    assert st.stuffed_bytes == m.stuffed and st.entropy_bits == m.scan_bits


def test_dense_noise_window_at_420(jpegamd, oracle, dev, enc):
    """4:2:0 has the fewest blocks per picture: 96 x 96 of noise fills one segment (36 of 42 MCUs) past the window."""
    rgb = np.random.default_rng(2).integers(0, 256, (96, 96, 3), np.uint8)
    m = model(oracle, rgb, 100, S420)
    assert im.segment_count(96, 96, S420) == 1 and m.scan_bits > WINDOW_BITS and m.no_eob_blocks > 0
    (f,), st = rgb_files(jpegamd, enc, [rgb], dev, S420, 100)
    assert f == m.file and st.stuffed_bytes == m.stuffed > 0


@pytest.mark.parametrize("sub", SUBS)
def test_zero_runs(jpegamd, oracle, dev, enc, sub):
    rgb = checker_picture()
    m = model(oracle, rgb, 50, sub)
    assert m.zrl_luma > 0
    if sub != S444:
        assert m.zrl_chroma > 0
    (f,), _ = rgb_files(jpegamd, enc, [rgb], dev, sub, 50)
    assert f == m.file


def test_zero_runs_in_chroma_at_444(jpegamd, oracle, dev, enc):
    """At 4:4:4 the chroma planes are not averaged: the YCbCr entry is fed a pixel checkerboard in Cb and Cr directly."""
    yy, xx = np.mgrid[0:16, 0:24]
    c1 = (((xx + yy) & 1) * 2 - 1)
    planes = (np.full((16, 24), 90, np.uint8), (128 + 60 * c1).astype(np.uint8), (128 - 60 * c1).astype(np.uint8))
    m = cm.memo(im.interleaved_ycbcr_file, oracle, *planes, 50, S444)
    assert m.zrl_chroma > 0
    (f,), _ = gs.finish_files(enc, YccCall(jpegamd, enc, [planes], dev, S444, PLANES, 50))
    assert f == m.file


@pytest.mark.parametrize("sub", SUBS)
def test_largest_dc_and_flat(jpegamd, oracle, dev, enc, sub):
    bw = block_checker()
    m = model(oracle, bw, 100, sub)
    assert m.dc_size_luma == 11
    (f,), _ = rgb_files(jpegamd, enc, [bw], dev, sub, 100)
    assert f == m.file
    flat = np.full((24, 40, 3), 77, np.uint8)
    m = model(oracle, flat, 50, sub)
    assert m.zrl_luma == m.zrl_chroma == m.no_eob_blocks == m.stuffed == 0
    # every block is DC-only: the first Y block a size-5 difference and EOB (3 + 5 + 4 bits), every other Y block, pad blocks included,
    # a zero difference and EOB (2 + 4), every chroma block a zero difference and EOB (2 + 2)
    assert m.scan_bits == 12 + 6 * (15 + m.pad_blocks - 1) + 4 * 2 * {S444: 15, S420: 6, S422: 9}[sub]
    (f,), st = rgb_files(jpegamd, enc, [flat], dev, sub, 50)
    assert f == m.file and st.stuffed_bytes == 0 and st.entropy_bits == m.scan_bits


# ---- batches --------------------------------------------------------------------------------------------------------------------------
def test_batch_of_three(jpegamd, oracle, dev, enc):
    rgbs = gs.pictures(jpegamd, 40, 24, 3)
    ms = [model(oracle, r, 50, S420) for r in rgbs]
    assert len({m.file for m in ms}) == 3
    files, st = rgb_files(jpegamd, enc, rgbs, dev, S420, 50)
    assert files == [m.file for m in ms]
    assert st.entropy_bits == sum(m.scan_bits for m in ms) and st.stuffed_bytes == sum(m.stuffed for m in ms)


def test_batch_of_thirty_two(jpegamd, oracle, dev, enc):
    rgbs = gs.pictures(jpegamd, 16, 16, 32, seed=3)
    ms = [model(oracle, r, 90, S444) for r in rgbs]
    files, st = rgb_files(jpegamd, enc, rgbs, dev, S444, 90)
    assert files == [m.file for m in ms]
    assert st.entropy_bits == sum(m.scan_bits for m in ms) and st.stuffed_bytes == sum(m.stuffed for m in ms)


def scratch_need(count, w, h, sub):
    """(coefficients, segments) the path's scratch must hold for one call, as the host sizes it: per picture every Y block and every
    chroma block of every MCU at 64 coefficients, and the segments of a picture padded to a multiple of 4 (one group of k_finalize's
    aggregates); a call this small goes through as one group of `count` pictures."""
    _, _, bw, bh, mx, my = im.geometry(w, h, sub)
    return count * (bw * bh + 2 * mx * my) * 64, count * -(-im.segment_count(w, h, sub) // 4) * 4


def test_scratch_grown_behind_queued_work(jpegamd, oracle, dev):
    """Four calls queued on a fresh context with one finish at the end.  The first sizes the scratch.  The second (the 200 x 120
    picture, five segments where the first had one per picture) needs larger coefficient planes but, padded, no more segments; the
    third (twelve small pictures) needs more segments but no more coefficients, so the segment arrays are replaced on their own; the
    fourth is the first again, on the scratch the others left.  Every file is compared byte for byte.  The needs are asserted from
    the model so that each replacement does happen; whether a replacement waits for the queued work is not something a passing run
    can show."""
    small = gs.pictures(jpegamd, 16, 16, 2, seed=61)
    large = gs.synth_rgb(jpegamd, 200, 120, 62, 0)
    many = gs.pictures(jpegamd, 16, 16, 12, seed=63)
    assert im.segment_count(16, 16, S420) == 1 and im.segment_count(200, 120, S444) == 5
    needs = [scratch_need(2, 16, 16, S420), scratch_need(1, 200, 120, S444), scratch_need(12, 16, 16, S420)]
    assert needs == [(768, 8), (72000, 8), (4608, 48)]              # coefficients grow in the second call, segments in the third
    want_small = [model(oracle, r, 50, S420).file for r in small]
    e = jpegamd.Encoder(512, gs.rows_for(32, 16))
    try:
        calls = [RgbCall(jpegamd, e, small, dev, S420, 50), RgbCall(jpegamd, e, [large], dev, S444, 50),
                 RgbCall(jpegamd, e, many, dev, S420, 50), RgbCall(jpegamd, e, small, dev, S420, 50)]
        e.finish()
        got = [gs.intact_files(c) for c in calls]
    finally:
        e.close()
    assert got == [want_small, [model(oracle, large, 50, S444).file], [model(oracle, r, 50, S420).file for r in many], want_small]


# ---- the YCbCr entry ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", SUBS)
def test_ycbcr_layouts_give_one_file(jpegamd, oracle, dev, enc, sub):
    planes = [gs.random_planes(40, 24, sub, 21), derived_planes(gs.synth_rgb(jpegamd, 40, 24, 22, 0), sub)]
    want = [cm.memo(im.interleaved_ycbcr_file, oracle, *p, 75, sub).file for p in planes]
    for layout in (PLANES, CBCR, CRCB):
        files, _ = gs.finish_files(enc, YccCall(jpegamd, enc, planes, dev, sub, layout, 75))
        assert files == want, layout


@pytest.mark.parametrize("sub", SUBS)
def test_ycbcr_entry_fed_the_rgb_planes_gives_the_rgb_file(jpegamd, oracle, dev, enc, sub):
    rgb = gs.synth_rgb(jpegamd, 72, 24, 31, 0)
    (f,), _ = gs.finish_files(enc, YccCall(jpegamd, enc, [derived_planes(rgb, sub)], dev, sub, CBCR, 50))
    (g,), _ = rgb_files(jpegamd, enc, [rgb], dev, sub, 50)
    assert f == g == model(oracle, rgb, 50, sub).file


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("layout", (PLANES, CRCB))
def test_ycbcr_odd_address_and_stride(jpegamd, oracle, dev, enc, sub, layout):
    planes = gs.random_planes(33, 17, sub, 40 + sub)
    cw, _ = gs.chroma_dims(33, 17, sub)
    call = YccCall(jpegamd, enc, [planes], dev, sub, layout, 50, y_stride=37, c_stride=2 * cw + 3, shift=1)   # the byte loader
    (f,), _ = gs.finish_files(enc, call)
    assert f == cm.memo(im.interleaved_ycbcr_file, oracle, *planes, 50, sub).file


# ---- capacity, decoder, neighbours, statistics ------------------------------------------------------------------------------------------
def test_capacity_one_byte_short_for_the_middle_picture(jpegamd, oracle, dev, enc):
    small = gs.synth_rgb(jpegamd, 40, 24, 50, 0)
    big = np.random.default_rng(5).integers(0, 256, (24, 40, 3), np.uint8)
    rgbs = [small, big, np.ascontiguousarray(small[::-1])]
    ms = [model(oracle, r, 50, S420) for r in rgbs]
    cap = len(ms[1].file) - 1
    assert len(ms[0].file) < cap and len(ms[2].file) < cap
    call = RgbCall(jpegamd, enc, rgbs, dev, S420, 50, cap=cap)
    with pytest.raises(jpegamd.JpegAmdError) as err:
        enc.finish()
    assert err.value.code == -8                                 # JPEGAMD_ERR_HUFF_CAPACITY
    files = gs.intact_files(call)                                   # the guard behind out_capacity is untouched
    assert call.sizes.cpu().tolist() == [len(ms[0].file), 0, len(ms[2].file)]
    assert files[0] == ms[0].file and files[2] == ms[2].file
    # the context is usable again, and the status was cleared
    (f,), _ = rgb_files(jpegamd, enc, [big], dev, S420, 50)
    assert f == ms[1].file


@pytest.mark.parametrize("sub", SUBS)
def test_independent_decoder_sees_the_three_scan_pixels(jpegamd, oracle, dev, enc, sub):
    rgb = gs.synth_rgb(jpegamd, 200, 120, 77, 0)
    (one,), _ = rgb_files(jpegamd, enc, [rgb], dev, sub, 75)
    (three,), _ = gs.finish_files(enc, gs.ColorBatch(jpegamd, enc, [rgb], dev, sub, 75))
    assert three == gs.model(oracle, rgb, 75, sub)
    got = decode(one)
    assert got.shape == (120, 200, 3) and np.array_equal(got, decode(three))


def test_neighbours_on_the_same_context_are_unchanged(jpegamd, oracle, dev, enc):
    rgbs = gs.pictures(jpegamd, 72, 40, 4, seed=9)
    grays = [sm.luma_plane(r) for r in rgbs]
    want_color = [gs.model(oracle, r, 50, S420) for r in rgbs]
    want_gray = [cm.memo(cm.gray_file, oracle, p, 50) for p in grays]
    want_one = [model(oracle, r, 50, S420).file for r in rgbs]
    for _ in range(2):                                              # before and after an interleaved call
        files, _ = gs.finish_files(enc, gs.ColorBatch(jpegamd, enc, rgbs, dev, S420, 50))
        assert files == want_color
        files, _ = gs.encode_gray_planes(jpegamd, enc, grays, dev, 50)
        assert files == want_gray
        files, _ = rgb_files(jpegamd, enc, rgbs, dev, S420, 50)
        assert files == want_one


def test_exact_fallbacks_equal_the_three_scan_figure(jpegamd, oracle, dev, enc):
    rgb = gs.synth_rgb(jpegamd, 200, 120, 13, 1)                    # noise: the quantiser meets ties
    for sub in (S420, S444):
        _, st3 = gs.finish_files(enc, gs.ColorBatch(jpegamd, enc, [rgb], dev, sub, 90))
        (f,), st1 = rgb_files(jpegamd, enc, [rgb], dev, sub, 90)
        print(f"exact_fallbacks sub {sub}: three-scan {st3.exact_fallbacks}, interleaved {st1.exact_fallbacks}")
        assert f == model(oracle, rgb, 90, sub).file
        assert st1.exact_fallbacks == st3.exact_fallbacks > 0
    assert model(oracle, rgb, 90, S420).pad_blocks > 0              # pad blocks add none


def test_profiled_call_reports_the_span(jpegamd, oracle, dev):
    e = jpegamd.Encoder(64, 64)
    try:
        e.set_profiling(4)
        rgb = gs.synth_rgb(jpegamd, 40, 24, 3, 0)
        (f,), st = rgb_files(jpegamd, e, [rgb], dev, S422, 50)
        assert f == model(oracle, rgb, 50, S422).file
        assert st.ns_total > 0
    finally:
        e.close()


def test_binding_scan_interleaved(jpegamd, oracle, dev):
    rgbs = gs.pictures(jpegamd, 24, 40, 2, seed=4)
    t = torch.from_numpy(np.stack(rgbs)).to(dev)
    want = [model(oracle, r, 0, S420).file for r in rgbs]
    assert jpegamd.encode_tensor_batch(t, scan="interleaved") == want
    assert jpegamd.encode_tensor(t[1], scan="interleaved") == want[1]
    assert jpegamd.encode_tensor_batch(t, scan="separate") == jpegamd.encode_tensor_batch(t) == [gs.model(oracle, r, 0, S420) for r in rgbs]
    y, cb, cr = derived_planes(gs.synth_rgb(jpegamd, 24, 40, 8, 0), S422)
    files = jpegamd.encode_ycbcr_batch(torch.from_numpy(y[None]).to(dev), torch.from_numpy(cb[None]).to(dev), torch.from_numpy(cr[None]).to(dev),
                                       subsampling=S422, scan="interleaved")
    assert files == [cm.memo(im.interleaved_ycbcr_file, oracle, y, cb, cr, 0, S422).file]
