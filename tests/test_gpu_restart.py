"""Restart intervals in the one-scan colour files on the GPU (jpegamd_encode_color_interleaved_restart_batch_async,
jpegamd_encode_ycbcr_interleaved_restart_batch_async): every device file is compared byte for byte with the CPU model
(tests/restart_model.py).  The model's counters are asserted for every property a case claims to exercise, so none passes vacuously.
The one exception are the two pictures large enough to take the offsets kernel through several rounds: too large for the CPU model,
they are checked by a walk of the scan and by an independent decoder against the device's own file without restart intervals."""
from __future__ import annotations

import io

import numpy as np
import pytest

import color_model as cm
import gpu_support as gs
import interleaved_model as im
import restart_model as rm
import scan_model as sm
from gpu_support import CBCR, CRCB, PLANES, S420, S422, S444, dev  # noqa: F401

torch = gs.torch
pytestmark = pytest.mark.gpu
SUBS = (S444, S420, S422)
WINDOW_BITS = 2048 * 32                                         # k_mcu_segments' LDS window: a longer segment leaves in pieces


def model(oracle, rgb, q, sub, ri):
    return cm.memo(rm.restart_file, oracle, rgb, q, sub, ri)


def plain_model(oracle, rgb, q, sub):
    return cm.memo(im.interleaved_file, oracle, rgb, q, sub)


class RgbCall(gs.Outputs):
    """One RGB batch with restart interval `ri` queued on `enc`."""

    def __init__(self, jpegamd, enc, rgbs, dev, sub, ri, quality=0, cap=None):
        h, w, _ = rgbs[0].shape
        self.px = [gs.upload(gs.stored_rows(r, False), dev, 3 * w) for r in rgbs]
        super().__init__(dev, len(rgbs), cap if cap is not None else jpegamd.max_jfif_bytes_interleaved_restart(w, h, sub, ri))
        imgs = [jpegamd.Encoder.image(ptr, w, h, 3 * w, False, jpegamd.ORDER_RGB, quality) for _, ptr in self.px]
        enc.encode_color_interleaved_restart_batch_async(imgs, sub, ri, self.out_ptrs, self.cap, self.size_ptrs, gs.stream())


class YccCall(gs.Outputs):
    """One YCbCr batch with restart interval `ri`: planes stored `shift` bytes into their allocations, rows `stride` bytes apart."""

    def __init__(self, jpegamd, enc, planes, dev, sub, layout, ri, quality=0, y_stride=None, c_stride=None, shift=0):
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
        super().__init__(dev, len(planes), jpegamd.max_jfif_bytes_interleaved_restart(w, h, sub, ri))
        enc.encode_ycbcr_interleaved_restart_batch_async(imgs, sub, ri, self.out_ptrs, self.cap, self.size_ptrs, gs.stream())


def rgb_files(jpegamd, enc, rgbs, dev, sub, ri, q=0, **kw):
    return gs.finish_files(enc, RgbCall(jpegamd, enc, rgbs, dev, sub, ri, q, **kw))


def derived_planes(rgb, sub):
    """(y, cb, cr) as the RGB entries derive them at `sub`."""
    return tuple(np.ascontiguousarray(p) for p in sm.planes_of(rgb, sub))


def decode(data: bytes) -> np.ndarray:
    image = pytest.importorskip("PIL.Image")
    with image.open(io.BytesIO(data)) as f:
        return np.asarray(f.convert("RGB"))


def noise(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), np.uint8)


@pytest.fixture(scope="module")
def enc(jpegamd, dev):
    e = jpegamd.Encoder(512, gs.rows_for(32, 16))
    yield e
    e.close()


# ---- geometry x interval ----------------------------------------------------------------------------------------------------------------
GEOMETRY = [(16, 16), (17, 9), (24, 40), (200, 120)]


def intervals_for(w, h, sub):
    """1, an MCU row, a row and one MCU (a boundary mid-row), a coder segment, a segment and one MCU (an interval of two segments, the
    second of one MCU), the whole scan, the largest value."""
    _, _, _, _, mx, my = im.geometry(w, h, sub)
    s = rm.seg_mcus(sub)
    return sorted({1, mx, mx + 1, s, s + 1, mx * my, 65535})


@pytest.mark.parametrize("w,h,sub", [(w, h, sub) for (w, h) in GEOMETRY for sub in SUBS])
def test_geometry_and_interval(jpegamd, oracle, dev, enc, w, h, sub):
    rgb = gs.synth_rgb(jpegamd, w, h, 5 + w, 0)
    _, _, _, _, mx, my = im.geometry(w, h, sub)
    seen_two = 0
    for ri in intervals_for(w, h, sub):
        m = model(oracle, rgb, 75, sub, ri)
        assert m.intervals == -(-(mx * my) // ri) == m.markers + 1
        seen_two += m.two_segment_intervals
        (f,), st = rgb_files(jpegamd, enc, [rgb], dev, sub, ri, 75)
        assert f == m.file, ri
        assert st.entropy_bits == m.scan_bits and st.stuffed_bytes == m.stuffed, ri
    if (w, h) == (200, 120):
        assert seen_two > 0                                         # Ri = S + 1 and Ri = M: intervals of several coder segments
        assert sm.walk_scan(model(oracle, rgb, 75, sub, 1).file, im.SOS3)[0][8] == 0         # the marker counter wrapped


def test_one_interval_is_the_plain_file_with_dri(jpegamd, oracle, dev, enc):
    rgb = gs.synth_rgb(jpegamd, 200, 120, 8, 0)
    for sub in SUBS:
        (f,), _ = rgb_files(jpegamd, enc, [rgb], dev, sub, 65535, 50)
        assert f == rm.with_dri(plain_model(oracle, rgb, 50, sub).file, 65535)


@pytest.mark.parametrize("sub", SUBS)
def test_interval_zero_is_the_existing_entry(jpegamd, oracle, dev, enc, sub):
    rgb = gs.synth_rgb(jpegamd, 72, 40, 31, 0)
    m = plain_model(oracle, rgb, 50, sub)
    (f,), st = rgb_files(jpegamd, enc, [rgb], dev, sub, 0, 50)
    assert f == m.file and b"\xff\xdd" not in f[:f.index(im.SOS3)]
    assert st.entropy_bits == m.scan_bits and st.stuffed_bytes == m.stuffed
    assert jpegamd.max_jfif_bytes_interleaved_restart(72, 40, sub, 0) == jpegamd.max_jfif_bytes_interleaved(72, 40, sub)
    planes = derived_planes(rgb, sub)
    (g,), _ = gs.finish_files(enc, YccCall(jpegamd, enc, [planes], dev, sub, CBCR, 0, 50))
    assert g == m.file == cm.memo(im.interleaved_ycbcr_file, oracle, *planes, 50, sub).file


# ---- content ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", SUBS)
def test_padded_bytes_that_are_ff_and_aligned_intervals(jpegamd, oracle, dev, enc, sub):
    """Dense noise, one MCU per interval: some intervals end in enough 1-bits for the padded byte to be 0xFF (stuffed), some end on a
    byte and get no padding."""
    rgb = noise(1, 64, 64)
    m = model(oracle, rgb, 100, sub, 1)
    assert m.pad_ff > 0 and m.aligned > 0 and m.stuffed > 0
    (f,), st = rgb_files(jpegamd, enc, [rgb], dev, sub, 1, 100)
    assert f == m.file
    assert st.stuffed_bytes == m.stuffed and st.entropy_bits == m.scan_bits


@pytest.mark.parametrize("sub", SUBS)
def test_intervals_of_two_segments_past_the_window(jpegamd, oracle, dev, enc, sub):
    rgb = noise(1, 112, 128)                                         # 128 x 112 pixels
    ri = rm.seg_mcus(sub) + 1
    m = model(oracle, rgb, 100, sub, ri)
    assert m.two_segment_intervals > 0 and m.max_segment_bits > WINDOW_BITS and m.intervals > 1
    (f,), st = rgb_files(jpegamd, enc, [rgb], dev, sub, ri, 100)
    assert f == m.file
    assert st.stuffed_bytes == m.stuffed > 0 and st.entropy_bits == m.scan_bits


STRADDLE_SEED = 393       # the first of seeds 0 .. 399 whose 112 x 112 noise, 4:2:0, quality 100, Ri = 43 has such a byte (a CPU search with the model)


def test_stuffed_byte_straddling_two_segments_of_an_interval(jpegamd, oracle, dev, enc):
    rgb = noise(STRADDLE_SEED, 112, 112)
    m = model(oracle, rgb, 100, S420, 43)                            # 49 MCUs: an interval of 42 + 1, one of 6
    assert m.straddle_ff > 0 and m.straddle_phases == (5,) and m.intervals == 2
    (f,), st = rgb_files(jpegamd, enc, [rgb], dev, S420, 43, 100)
    assert f == m.file and st.stuffed_bytes == m.stuffed


OFFSET_ROUND = 8192                                             # segments k_mcu_restart_offsets takes per round: more go round by round, sums carried


@pytest.mark.parametrize("size,ri", [(1024, 1), (4752, 86)])
def test_more_segments_than_one_round_of_the_offsets_kernel(jpegamd, dev, size, ri):
    """Pictures whose segments do not fit one round of the kernel that places them: one MCU per interval (every interval one segment),
    and intervals of two segments (S + 1 MCUs), where the bit offsets inside an interval come from a running sum that is carried
    across rounds as well.  No CPU model at this size: the scan is walked (every marker in order, every 0xFF accounted for), and an
    independent decoder must see the pixels of the device's file without restart intervals."""
    assert rm.seg_mcus(S444) + 1 == 86
    entries = rm.segment_entries(size, size, S444, ri)
    n = rm.interval_count(size, size, S444, ri)
    assert entries > OFFSET_ROUND and entries == n * (2 if ri == 86 else 1)
    ramp = np.arange(size, dtype=np.int16)
    base = (ramp * 3 // 32)[None, :] + (ramp * 2 // 32)[:, None] + np.random.default_rng(size).integers(-6, 7, (size, size), np.int16)
    rgb = np.stack([base & 255, (base >> 1) & 255, 255 - (base & 255)], axis=2).astype(np.uint8)       # ramps with a little noise
    e = jpegamd.Encoder(size, size)
    try:
        (plain,), _ = rgb_files(jpegamd, e, [rgb], dev, S444, 0, 50, cap=size * size)
        (f,), st = rgb_files(jpegamd, e, [rgb], dev, S444, ri, 50, cap=size * size)
    finally:
        e.close()
    at = f.index(im.SOS3)
    assert f[at - 6:at] == rm.dri(ri) and f[:at - 6] == plain[:at - 6]
    markers, stuffed = sm.walk_scan(f, im.SOS3)
    assert len(markers) == n - 1 and markers == [i % 8 for i in range(n - 1)]
    assert stuffed == st.stuffed_bytes
    assert np.array_equal(decode(f), decode(plain))


# ---- batches ----------------------------------------------------------------------------------------------------------------------------
def test_batch_of_three(jpegamd, oracle, dev, enc):
    rgbs = gs.pictures(jpegamd, 40, 24, 3)
    ms = [model(oracle, r, 50, S420, 2) for r in rgbs]
    assert len({m.file for m in ms}) == 3 and ms[0].intervals == 3
    files, st = rgb_files(jpegamd, enc, rgbs, dev, S420, 2, 50)
    assert files == [m.file for m in ms]
    assert st.entropy_bits == sum(m.scan_bits for m in ms) and st.stuffed_bytes == sum(m.stuffed for m in ms)


def test_batch_of_thirty_two(jpegamd, oracle, dev, enc):
    rgbs = gs.pictures(jpegamd, 16, 16, 32, seed=3)
    ms = [model(oracle, r, 90, S444, 1) for r in rgbs]
    files, st = rgb_files(jpegamd, enc, rgbs, dev, S444, 1, 90)
    assert files == [m.file for m in ms]
    assert st.entropy_bits == sum(m.scan_bits for m in ms) and st.stuffed_bytes == sum(m.stuffed for m in ms)


def test_capacity_one_byte_short_for_the_middle_picture(jpegamd, oracle, dev, enc):
    small = gs.synth_rgb(jpegamd, 40, 24, 50, 0)
    big = noise(5, 24, 40)
    rgbs = [small, big, np.ascontiguousarray(small[::-1])]
    ms = [model(oracle, r, 50, S420, 2) for r in rgbs]
    cap = len(ms[1].file) - 1
    assert len(ms[0].file) < cap and len(ms[2].file) < cap
    call = RgbCall(jpegamd, enc, rgbs, dev, S420, 2, 50, cap=cap)
    with pytest.raises(jpegamd.JpegAmdError) as err:
        enc.finish()
    assert err.value.code == -8                                 # JPEGAMD_ERR_HUFF_CAPACITY
    files = gs.intact_files(call)                                   # the guard behind out_capacity is untouched
    assert call.sizes.cpu().tolist() == [len(ms[0].file), 0, len(ms[2].file)]
    assert files[0] == ms[0].file and files[2] == ms[2].file
    # the context is usable again, and the status was cleared
    (f,), _ = rgb_files(jpegamd, enc, [big], dev, S420, 2, 50)
    assert f == ms[1].file


def padded(n):
    return -(-n // 4) * 4


def test_scratch_grown_behind_queued_work(jpegamd, oracle, dev):
    """Four calls queued on a fresh context with one finish at the end.  The first (no restart intervals) sizes the scratch: one segment
    per picture.  The second, one MCU per interval, needs 375 segments for its one picture, and each reserves a string for 3 blocks
    where the first call's reserved 256; the third (twelve small pictures, one MCU per interval) needs fewer again; the fourth is the
    first, on the scratch the others left.  The needs are asserted from the model."""
    small = gs.pictures(jpegamd, 16, 16, 2, seed=61)
    large = gs.synth_rgb(jpegamd, 200, 120, 62, 0)
    many = gs.pictures(jpegamd, 16, 16, 12, seed=63)
    needs = [2 * padded(im.segment_count(16, 16, S420)), padded(rm.segment_entries(200, 120, S444, 1)), 12 * padded(rm.segment_entries(16, 16, S420, 1))]
    assert needs == [8, 376, 48]
    want_small = [plain_model(oracle, r, 50, S420).file for r in small]
    e = jpegamd.Encoder(512, gs.rows_for(32, 16))
    try:
        calls = [RgbCall(jpegamd, e, small, dev, S420, 0, 50), RgbCall(jpegamd, e, [large], dev, S444, 1, 50),
                 RgbCall(jpegamd, e, many, dev, S420, 1, 50), RgbCall(jpegamd, e, small, dev, S420, 0, 50)]
        e.finish()
        got = [gs.intact_files(c) for c in calls]
    finally:
        e.close()
    assert got == [want_small, [model(oracle, large, 50, S444, 1).file], [model(oracle, r, 50, S420, 1).file for r in many], want_small]


# ---- the YCbCr entry --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", SUBS)
def test_ycbcr_layouts_give_one_file(jpegamd, oracle, dev, enc, sub):
    planes = [gs.random_planes(40, 24, sub, 21), derived_planes(gs.synth_rgb(jpegamd, 40, 24, 22, 0), sub)]
    want = [cm.memo(rm.restart_ycbcr_file, oracle, *p, 75, sub, 2).file for p in planes]
    for layout in (PLANES, CBCR, CRCB):
        files, _ = gs.finish_files(enc, YccCall(jpegamd, enc, planes, dev, sub, layout, 2, 75))
        assert files == want, layout
    (f,), _ = rgb_files(jpegamd, enc, [gs.synth_rgb(jpegamd, 40, 24, 22, 0)], dev, sub, 2, 75)
    assert f == want[1]                                             # the RGB entry's file of the picture those planes derive from


@pytest.mark.parametrize("sub", SUBS)
@pytest.mark.parametrize("layout", (PLANES, CRCB))
def test_ycbcr_odd_address_and_stride(jpegamd, oracle, dev, enc, sub, layout):
    planes = gs.random_planes(33, 17, sub, 40 + sub)
    cw, _ = gs.chroma_dims(33, 17, sub)
    call = YccCall(jpegamd, enc, [planes], dev, sub, layout, 3, 50, y_stride=37, c_stride=2 * cw + 3, shift=1)   # the byte loader
    (f,), _ = gs.finish_files(enc, call)
    assert f == cm.memo(rm.restart_ycbcr_file, oracle, *planes, 50, sub, 3).file


# ---- neighbours, decoder, binding -------------------------------------------------------------------------------------------------------
def test_neighbours_on_the_same_context_are_unchanged(jpegamd, oracle, dev, enc):
    rgbs = gs.pictures(jpegamd, 72, 40, 4, seed=9)
    grays = [sm.luma_plane(r) for r in rgbs]
    want_color = [gs.model(oracle, r, 50, S420) for r in rgbs]
    want_gray = [cm.memo(cm.gray_file, oracle, p, 50) for p in grays]
    want_one = [plain_model(oracle, r, 50, S420).file for r in rgbs]
    want_restart = [model(oracle, r, 50, S420, 5).file for r in rgbs]
    for _ in range(2):                                              # before and after a call with restart intervals
        files, _ = gs.finish_files(enc, gs.ColorBatch(jpegamd, enc, rgbs, dev, S420, 50))
        assert files == want_color
        files, _ = gs.encode_gray_planes(jpegamd, enc, grays, dev, 50)
        assert files == want_gray
        files, _ = rgb_files(jpegamd, enc, rgbs, dev, S420, 0, 50)
        assert files == want_one
        files, _ = rgb_files(jpegamd, enc, rgbs, dev, S420, 5, 50)
        assert files == want_restart


@pytest.mark.parametrize("sub", SUBS)
def test_independent_decoder_sees_the_pixels_of_the_plain_file(jpegamd, oracle, dev, enc, sub):
    rgb = gs.synth_rgb(jpegamd, 200, 120, 77, 0)
    (plain,), _ = rgb_files(jpegamd, enc, [rgb], dev, sub, 0, 75)
    want = decode(plain)
    assert want.shape == (120, 200, 3)
    _, _, _, _, mx, _ = im.geometry(200, 120, sub)
    for ri in (1, mx, mx + 1):
        (f,), _ = rgb_files(jpegamd, enc, [rgb], dev, sub, ri, 75)
        assert np.array_equal(decode(f), want), ri


def test_profiled_call_reports_the_span(jpegamd, oracle, dev):
    e = jpegamd.Encoder(64, 64)
    try:
        e.set_profiling(4)
        rgb = gs.synth_rgb(jpegamd, 40, 24, 3, 0)
        (f,), st = rgb_files(jpegamd, e, [rgb], dev, S422, 2, 50)
        assert f == model(oracle, rgb, 50, S422, 2).file
        assert st.ns_total > 0
    finally:
        e.close()


def test_binding_restart_interval(jpegamd, oracle, dev):
    rgbs = gs.pictures(jpegamd, 24, 40, 2, seed=4)
    t = torch.from_numpy(np.stack(rgbs)).to(dev)
    for ri, arg in ((2, 2), (2, "row"), (1, 1)):                     # 24 pixels at 4:2:0: an MCU row is 2 MCUs
        want = [model(oracle, r, 0, S420, ri).file for r in rgbs]
        assert jpegamd.encode_tensor_batch(t, scan="interleaved", restart_interval=arg) == want
        assert jpegamd.encode_tensor(t[1], scan="interleaved", restart_interval=arg) == want[1]
    plain = [plain_model(oracle, r, 0, S420).file for r in rgbs]
    assert jpegamd.encode_tensor_batch(t, scan="interleaved", restart_interval=0) == plain
    assert jpegamd.encode_tensor_batch(t, scan="interleaved", restart_interval=None) == plain
    y, cb, cr = derived_planes(gs.synth_rgb(jpegamd, 24, 40, 8, 0), S422)
    ty, tcb, tcr = (torch.from_numpy(p[None]).to(dev) for p in (y, cb, cr))
    for ri, arg in ((2, "row"), (3, 3)):
        files = jpegamd.encode_ycbcr_batch(ty, tcb, tcr, subsampling=S422, scan="interleaved", restart_interval=arg)
        assert files == [cm.memo(rm.restart_ycbcr_file, oracle, y, cb, cr, 0, S422, ri).file]
    for kw in (dict(restart_interval=2), dict(scan="separate", restart_interval="row"), dict(scan="interleaved", restart_interval=65536),
               dict(scan="interleaved", restart_interval=-1), dict(scan="interleaved", restart_interval="mcu")):
        with pytest.raises(ValueError):
            jpegamd.encode_tensor_batch(t, **kw)
        with pytest.raises(ValueError):
            jpegamd.encode_tensor(t[0], **kw)
        with pytest.raises(ValueError):
            jpegamd.encode_ycbcr_batch(ty, tcb, tcr, subsampling=S422, **kw)
