"""Progressive colour files on the GPU (jpegamd_encode_color_progressive_batch_async, jpegamd_encode_ycbcr_progressive_batch_async): every
device file is compared byte for byte with the CPU model (tests/progressive_model.py).  The model's counters are asserted for every
property a case claims to exercise, so none passes vacuously."""
from __future__ import annotations

import numpy as np
import pytest

import color_model as cm
import gpu_support as gs
import interleaved_model as im
import mjpeg_support as ms
import progressive_model as pm
from gpu_support import CBCR, PLANES, S420, S422, S444, YUYV, dev  # noqa: F401

torch = gs.torch
pytestmark = pytest.mark.gpu
SUBS = (S444, S420, S422)
WINDOW_BITS = 2048 * 32                                         # the coder's LDS window: a longer segment leaves in pieces
ERR_ARG = -1


def model(oracle, rgb, q, sub):
    return cm.memo(pm.progressive_file, oracle, rgb, q, sub)


def ycc_model(oracle, planes8, q, sub):
    return cm.memo(pm.progressive_ycbcr_file, oracle, *planes8, q, sub)


class PixelsCall(gs.Outputs):
    """One batch through jpegamd_encode_color_progressive_batch_async: order "rgb" / "bgr" / "rgba" / "bgra"."""

    def __init__(self, jpegamd, enc, rgbs, dev, sub, q=0, order="rgb", bottom_up=False, stride=None, shift=0, cap=None):
        h, w, _ = rgbs[0].shape
        px4, blue = order in ("rgba", "bgra"), order in ("bgr", "bgra")
        stride = stride or (4 if px4 else 3) * w
        rows = [ms.px4_rows(r, bottom_up, blue) if px4 else gs.stored_rows(r, bottom_up, blue) for r in rgbs]
        self.px = [gs.upload(r, dev, stride, shift) for r in rows]
        super().__init__(dev, len(rgbs), cap if cap is not None else jpegamd.max_jfif_bytes_progressive(w, h, sub))
        code = {"rgb": jpegamd.ORDER_RGB, "bgr": jpegamd.ORDER_BGR, "rgba": jpegamd.ORDER_RGBA, "bgra": jpegamd.ORDER_BGRA}[order]
        imgs = [jpegamd.Encoder.image(ptr, w, h, stride, bottom_up, code, q) for _, ptr in self.px]
        enc.encode_color_progressive_batch_async(imgs, sub, self.out_ptrs, self.cap, self.size_ptrs, gs.stream())


class Progressive:
    """An Encoder as gpu_support.YccBatch sees it: every YCbCr call goes to jpegamd_encode_ycbcr_progressive_batch_async with this matrix."""

    def __init__(self, enc, matrix):
        self.enc, self.matrix = enc, matrix

    def encode_ycbcr_batch_async(self, imgs, subsampling, out_ptrs, out_cap, size_ptrs, stream=0, sample_range=0, sample_format=0):
        self.enc.encode_ycbcr_progressive_batch_async(imgs, subsampling, sample_range, sample_format, self.matrix, out_ptrs, out_cap, size_ptrs, stream)


def ycc_files(jpegamd, enc, kind, planes, dev, sub, layout, q=0):
    h, w = planes[0][0].shape
    rng, fmt, matrix = kind.args(jpegamd)
    call = gs.YccBatch(jpegamd, Progressive(enc, matrix), planes, dev, sub, layout, quality=q, cap=jpegamd.max_jfif_bytes_progressive(w, h, sub),
                       sample_range=rng, sample_format=fmt)
    return gs.finish_files(enc, call)


def rgb_files(jpegamd, enc, rgbs, dev, sub, q=0, **kw):
    return gs.finish_files(enc, PixelsCall(jpegamd, enc, rgbs, dev, sub, q, **kw))


def check_stats(st, models):
    assert st.entropy_bits == sum(m.bits for m in models)
    assert st.stuffed_bytes == sum(sum(m.stuffed) for m in models)


@pytest.fixture(scope="module")
def enc(jpegamd, dev):
    e = jpegamd.Encoder(4112, gs.rows_for(32, 40))
    yield e
    e.close()


# ---- 1. geometry ----------------------------------------------------------------------------------------------------------------------
GEOMETRY = [(1, 1), (8, 8), (17, 9), (24, 40), (257, 31), (200, 120)]


@pytest.mark.parametrize("w,h,sub", [(w, h, sub) for (w, h) in GEOMETRY for sub in SUBS])
def test_geometry(jpegamd, oracle, dev, enc, w, h, sub):
    rgb = gs.synth_rgb(jpegamd, w, h, 5 + w, 0)
    m = model(oracle, rgb, 50, sub)
    hs, vs, bw, bh, mx, my = im.geometry(w, h, sub)
    assert m.pad_blocks == mx * my * hs * vs - bw * bh
    # pad blocks exist in the DC scan alone: an AC scan of Y has the plane's own blocks
    assert len(m.seg_bits[0]) == -(-mx * my // (256 // (hs * vs + 2)))
    assert [len(s) for s in m.seg_bits[1:]] == [-(-bw * bh // 256), -(-mx * my // 256), -(-mx * my // 256)] * 2
    (f,), st = rgb_files(jpegamd, enc, [rgb], dev, sub, 50)
    assert f == m.file
    check_stats(st, [m])


def test_geometry_cases_have_pad_blocks(jpegamd, oracle):
    pads = {sub: sum(model(oracle, gs.synth_rgb(jpegamd, w, h, 5 + w, 0), 50, sub).pad_blocks for w, h in GEOMETRY) for sub in SUBS}
    assert pads[S444] == 0 and pads[S420] > 0 and pads[S422] > 0


# ---- 2. segment edges -----------------------------------------------------------------------------------------------------------------
def test_last_segment_of_one_block_at_444(jpegamd, oracle, dev, enc):
    rgb = gs.synth_rgb(jpegamd, 2056, 8, 91, 0)
    m = model(oracle, rgb, 50, S444)
    assert [len(s) for s in m.seg_bits] == [4, 2, 2, 2, 2, 2, 2]            # 257 MCUs: 85 + 85 + 85 + 2; 257 blocks: 256 + 1
    (f,), st = rgb_files(jpegamd, enc, [rgb], dev, S444, 50)
    assert f == m.file
    check_stats(st, [m])


def test_last_chroma_segment_of_one_block_at_420(jpegamd, oracle, dev, enc):
    rgb = gs.synth_rgb(jpegamd, 4112, 16, 92, 0)
    m = model(oracle, rgb, 50, S420)
    assert [len(s) for s in m.seg_bits] == [7, 5, 2, 2, 5, 2, 2]            # 257 MCUs of 6 blocks: 6 x 42 + 5; Y 1028 blocks; chroma 257
    (f,), st = rgb_files(jpegamd, enc, [rgb], dev, S420, 50)
    assert f == m.file
    check_stats(st, [m])


def test_flat_grey_last_segments_of_two_and_four_bits(jpegamd, oracle, dev, enc):
    rgb = np.full((8, 2056, 3), 128, np.uint8)
    m = model(oracle, rgb, 50, S444)
    assert [s[-1] for s in m.seg_bits] == [2 * 6, 4, 2, 2, 4, 2, 2]         # "00 00 00" per flat MCU; EOB is 1010 (luma) / 00 (chroma)
    assert m.eob_only == (3 * 257, 3 * 257)
    (f,), st = rgb_files(jpegamd, enc, [rgb], dev, S444, 50)
    assert f == m.file
    check_stats(st, [m])


def test_one_flat_mcu_is_six_bits(jpegamd, oracle, dev, enc):
    rgb = np.full((8, 8, 3), 128, np.uint8)
    m = model(oracle, rgb, 50, S444)
    assert m.seg_bits == ((6,), (4,), (2,), (2,), (4,), (2,), (2,))
    (f,), _ = rgb_files(jpegamd, enc, [rgb], dev, S444, 50)
    assert f == m.file


# ---- 3. window rounds -----------------------------------------------------------------------------------------------------------------
def test_dense_noise_takes_several_window_rounds(jpegamd, oracle, dev, enc):
    rgb = np.random.default_rng(7).integers(0, 256, (128, 128, 3), np.uint8)
    m = model(oracle, rgb, 100, S444)
    assert max(max(s) for s in m.seg_bits[4:]) > WINDOW_BITS               # a band 6..63 segment leaves in pieces
    (f,), st = rgb_files(jpegamd, enc, [rgb], dev, S444, 100)
    assert f == m.file
    check_stats(st, [m])


# ---- 4. symbols -----------------------------------------------------------------------------------------------------------------------
def symbols_plane(seed):
    """128 x 16 samples, blocks left to right: four of noise (no end symbol in either band, 0xFF bytes), four flat black and white in
    turn (DC size 11 at quality 96, the end symbol alone), four of alternating columns (coefficients 1, 6, 15 and 28: a zero run that
    ends at the band edge), four of one high DCT basis function each (coefficient 62 or 57 alone: ZRLs)."""
    rng = np.random.default_rng(seed)
    x = np.arange(8)
    p = np.full((16, 128), 128, np.uint8)
    p[:, 0:32] = rng.integers(0, 256, (16, 32))
    for b in range(4):
        p[:, 32 + 8 * b:40 + 8 * b] = 0 if b % 2 == 0 else 255
    for b, amp in enumerate((20, 60, 100, 127)):
        p[:, 64 + 8 * b:72 + 8 * b] = 128 + amp * np.where(x % 2 == 0, 1, -1)
    for b, (u, v, amp) in enumerate(((6, 7, 6), (6, 7, 12), (4, 7, 12), (4, 7, 24))):
        block = np.rint(128 + amp * np.outer(np.cos((2 * x + 1) * v * np.pi / 16), np.cos((2 * x + 1) * u * np.pi / 16))).astype(np.uint8)
        p[0:8, 96 + 8 * b:104 + 8 * b] = p[8:16, 96 + 8 * b:104 + 8 * b] = block
    return p


def test_symbols(jpegamd, oracle, dev, enc):
    planes = tuple(symbols_plane(s) for s in (4, 5, 6))
    m = ycc_model(oracle, planes, 96, S444)
    assert m.zrl[(1, False)] > 0 and m.zrl[(1, True)] > 0
    assert min(m.no_end) > 0 and min(m.eob_only) > 0
    assert m.edge_runs > 0 and m.dc_size == 11
    assert sum(1 for s in m.stuffed if s) >= 2
    (f,), st = ycc_files(jpegamd, enc, ms.FULL8, [planes], dev, S444, PLANES, 96)
    assert f == m.file
    check_stats(st, [m])


# ---- 5. batches -----------------------------------------------------------------------------------------------------------------------
def test_batch_of_three(jpegamd, oracle, dev, enc):
    rgbs = gs.pictures(jpegamd, 200, 120, 3)
    models = [model(oracle, r, 50, S420) for r in rgbs]
    assert len({m.file for m in models}) == 3
    files, st = rgb_files(jpegamd, enc, rgbs, dev, S420, 50)
    assert files == [m.file for m in models]
    check_stats(st, models)


def test_batch_of_thirty_two(jpegamd, oracle, dev, enc):
    rgbs = gs.pictures(jpegamd, 24, 40, 32, seed=3)
    models = [model(oracle, r, 90, S422) for r in rgbs]
    files, st = rgb_files(jpegamd, enc, rgbs, dev, S422, 90)
    assert files == [m.file for m in models]
    check_stats(st, models)


def test_exact_fallbacks_are_the_one_scan_figure(jpegamd, oracle, dev, enc):
    rgb = gs.synth_rgb(jpegamd, 200, 120, 13, 1)                    # noise: the quantiser meets ties
    (one,), st1 = gs.finish_files(enc, ms.PixelsCall(jpegamd, enc, [rgb], dev, S420, "rgb", 0, 90))
    (f,), st = rgb_files(jpegamd, enc, [rgb], dev, S420, 90)
    assert one == cm.memo(im.interleaved_file, oracle, rgb, 90, S420).file and f == model(oracle, rgb, 90, S420).file
    assert st.exact_fallbacks == st1.exact_fallbacks > 0            # the three tap launches, counted once over the seven scans


# ---- 6. capacity ----------------------------------------------------------------------------------------------------------------------
def test_capacity_one_byte_short_and_exact(jpegamd, oracle, dev, enc):
    rgb = gs.synth_rgb(jpegamd, 200, 120, 50, 0)
    m = model(oracle, rgb, 50, S420)
    call = PixelsCall(jpegamd, enc, [rgb], dev, S420, 50, cap=len(m.file) - 1)
    with pytest.raises(jpegamd.JpegAmdError) as err:
        enc.finish()
    assert err.value.code == -8                                 # JPEGAMD_ERR_HUFF_CAPACITY
    gs.intact_files(call)                                           # the guard behind out_capacity is untouched
    assert call.sizes.cpu().tolist() == [0]
    # the context is usable again, and at exactly the file's size the file is intact
    (f,), st = rgb_files(jpegamd, enc, [rgb], dev, S420, 50, cap=len(m.file))
    assert f == m.file
    check_stats(st, [m])


def test_capacity_short_inside_the_first_scan(jpegamd, oracle, dev, enc):
    rgbs = [gs.synth_rgb(jpegamd, 200, 120, 51, 0), np.random.default_rng(8).integers(0, 256, (120, 200, 3), np.uint8)]
    models = [model(oracle, r, 50, S444) for r in rgbs]
    cap = len(pm.prefix(200, 120, 50, S444)) + 40                   # the DC scan itself outgrows it, for both pictures
    assert all(m.scan_bits[0] // 8 > 40 for m in models)
    call = PixelsCall(jpegamd, enc, rgbs, dev, S444, 50, cap=cap)
    with pytest.raises(jpegamd.JpegAmdError) as err:
        enc.finish()
    assert err.value.code == -8
    gs.intact_files(call)
    assert call.sizes.cpu().tolist() == [0, 0]
    files, _ = rgb_files(jpegamd, enc, rgbs, dev, S444, 50)
    assert files == [m.file for m in models]


# ---- 7. sources -----------------------------------------------------------------------------------------------------------------------
SOURCES = [("nv12", ms.FULL8, S420, CBCR), ("i422", ms.FULL8, S422, PLANES), ("yuy2", ms.FULL8, S422, YUYV),
           ("limited", ms.LIMITED8, S420, PLANES), ("msb10", ms.MSB10, S420, CBCR), ("bt709", ms.FULL8_709, S444, PLANES)]


@pytest.mark.parametrize("name,kind,sub,layout", SOURCES, ids=[s[0] for s in SOURCES])
def test_ycbcr_sources(jpegamd, oracle, dev, enc, name, kind, sub, layout):
    w, h = (40, 24) if layout == YUYV else (33, 17)
    planes = [ms.stored_planes(kind, w, h, sub, 60 + i) for i in range(2)]
    models = [ycc_model(oracle, ms.mapped_planes(kind, p, sub), 75, sub) for p in planes]
    files, st = ycc_files(jpegamd, enc, kind, planes, dev, sub, layout, 75)
    assert files == [m.file for m in models]
    check_stats(st, models)


def test_pixel_sources(jpegamd, oracle, dev, enc):
    rgb = gs.synth_rgb(jpegamd, 33, 17, 70, 0)
    want = model(oracle, rgb, 50, S420).file
    (f,), _ = rgb_files(jpegamd, enc, [rgb], dev, S420, 50, order="bgr", bottom_up=True, stride=3 * 33 + 5)
    assert f == want
    (f,), _ = rgb_files(jpegamd, enc, [rgb], dev, S420, 50, order="rgba")
    assert f == want


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_as_it_was(jpegamd, oracle, dev):
    rgb = gs.synth_rgb(jpegamd, 40, 24, 80, 0)
    one = cm.memo(im.interleaved_file, oracle, rgb, 50, S420).file
    e = jpegamd.Encoder(64, 64)
    try:
        def refused(**kw):
            with pytest.raises(jpegamd.JpegAmdError) as err:
                PixelsCall(jpegamd, e, [rgb], dev, kw.pop("sub", S420), 50, **kw)
            assert err.value.code == ERR_ARG

        e.set_huffman(jpegamd.HUFFMAN_OPTIMIZED)
        refused()
        e.set_huffman(jpegamd.HUFFMAN_STANDARD)
        refused(sub=3, cap=1 << 16)
        t, ptr = gs.upload(np.ascontiguousarray(rgb[:, :, 0]), dev, 40)
        out = gs.Outputs(dev, 1, 1 << 16)
        with pytest.raises(jpegamd.JpegAmdError) as err:
            e.encode_color_progressive_batch_async([jpegamd.Encoder.image(ptr, 40, 24, 40, False, jpegamd.ORDER_GRAY, 50)], S420, out.out_ptrs,
                                                   out.cap, out.size_ptrs, gs.stream())
        assert err.value.code == ERR_ARG
        (f,), _ = gs.finish_files(e, ms.PixelsCall(jpegamd, e, [rgb], dev, S420, "rgb", 0, 50))
        assert f == one
        (f,), _ = rgb_files(jpegamd, e, [rgb], dev, S420, 50)
        assert f == model(oracle, rgb, 50, S420).file
        (f,), _ = gs.finish_files(e, ms.PixelsCall(jpegamd, e, [rgb], dev, S420, "rgb", 0, 50))
        assert f == one                                             # ... and behind a progressive call: the prefix is the baseline one again
    finally:
        e.close()


# ---- 9. Python ------------------------------------------------------------------------------------------------------------------------
def test_binding(jpegamd, oracle, dev):
    import jpegamd.mjpeg as mj
    import jpegamd.progressive as prog
    rgbs = gs.pictures(jpegamd, 24, 40, 2, seed=4)
    t = torch.from_numpy(np.stack(rgbs)).to(dev)
    want = [model(oracle, r, 0, S420).file for r in rgbs]
    files = prog.encode_tensor_batch(t)
    assert files == want
    assert prog.encode_tensor(t[1]) == want[1]
    got, base = ms.decode(files[0]), ms.decode(mj.encode_tensor_batch(t)[0])
    assert got.shape == (40, 24, 3) and np.array_equal(got, base)
    y, cb, cr = ms.derived_planes(gs.synth_rgb(jpegamd, 24, 40, 8, 0), S422)
    files = prog.encode_ycbcr_batch(torch.from_numpy(y[None]).to(dev), torch.from_numpy(cb[None]).to(dev), torch.from_numpy(cr[None]).to(dev),
                                    subsampling=S422)
    assert files == [ycc_model(oracle, (y, cb, cr), 0, S422).file]
