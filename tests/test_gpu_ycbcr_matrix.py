"""BT.709 YCbCr input (jpegamd_encode_ycbcr_matrix_batch_async, matrix="bt709") through the C-ABI into the HIP kernels.  Two exact
comparisons against the definition in the header: the planes k_ycbcr_matrix_batch leaves in scratch (jpegamd_debug_ycbcr_matrix_planes),
sample for sample against tests/matrix_model.py behind the range / depth maps of tests/range_model.py and tests/depth_model.py; and the
files, byte for byte the full-range files (tests/color_model.py, tests/color_model_422.py) of those planes.  Every test needs an MI355X."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import depth_model as dm
import matrix_model as mm
import range_model as rm
from gpu_support import (CBCR, LAYOUTS, PLANES, S420, S422, S444, UYVY, WIDE_STRIDE, YUYV, ColorBatch, YccBatch, chroma_dims, dev,     # noqa: F401
                         finish_files, intact_files, model, pictures, random_planes, rows_for, smooth_planes)
from gpu_support import LAYOUTS_422 as YCC_LAYOUTS
from gpu_support import stream as current_stream
from gpu_support import ycc_file as expected

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


class Bt709:
    """An Encoder as YccBatch sees it, with the matrix added to every YCbCr call.  direct: the C entry itself, whatever entry Encoder
    would take (Encoder keeps BT601 calls to the older entries).  keep_planes: before each call, the planes of the pass alone (which
    waits for the stream: not for a test about calls queued back to back)."""

    def __init__(self, jpegamd, enc, matrix=None, direct=False, keep_planes=None):
        self.jpegamd, self.enc, self.direct, self.dev = jpegamd, enc, direct, keep_planes
        self.matrix = jpegamd.MATRIX_BT709 if matrix is None else matrix
        self.planes = None

    @property
    def _h(self):
        return self.enc._h

    def finish(self):
        return self.enc.finish()

    def encode_ycbcr_batch_async(self, imgs, subsampling, out_ptrs, out_cap, size_ptrs, stream=0, sample_range=0, sample_format=0):
        j = self.jpegamd
        if self.dev is not None:
            self.planes = pass_planes(j, self.enc, imgs, subsampling, sample_range, sample_format, self.dev)
        if not self.direct:
            return self.enc.encode_ycbcr_batch_async(imgs, subsampling, out_ptrs, out_cap, size_ptrs, stream, sample_range,
                                                     sample_format=sample_format, matrix=self.matrix)
        n = len(imgs)
        arr = (j.YCbCrImage * n)(*imgs)
        outs = (C.c_void_p * n)(*[C.c_void_p(p) for p in out_ptrs])
        sizes = (C.c_void_p * n)(*[C.c_void_p(p) for p in size_ptrs])
        rc = j.lib.jpegamd_encode_ycbcr_matrix_batch_async(self.enc._h, arr, n, int(subsampling), int(sample_range), int(sample_format),
                                                           int(self.matrix), outs, out_cap, sizes, C.c_void_p(stream))
        assert rc == 0, rc


def pass_planes(jpegamd, enc, imgs, sub, sample_range, sample_format, dev):
    """jpegamd_debug_ycbcr_matrix_planes -> [(y, cb, cr)] picture by picture, as numpy."""
    n, w, h = len(imgs), imgs[0].width, imgs[0].height
    cw, ch = chroma_dims(w, h, sub)
    bufs = [torch.full((n, hh, ww), 0xA5, dtype=torch.uint8, device=dev) for hh, ww in ((h, w), (ch, cw), (ch, cw))]
    arr = (jpegamd.YCbCrImage * n)(*imgs)
    rc = jpegamd.lib.jpegamd_debug_ycbcr_matrix_planes(enc._h, arr, n, int(sub), int(sample_range), int(sample_format), jpegamd.MATRIX_BT709,
                                                       *[C.c_void_p(b.data_ptr()) for b in bufs], C.c_void_p(current_stream()))
    assert rc == 0, rc
    host = [b.cpu().numpy() for b in bufs]
    return [tuple(p[i] for p in host) for i in range(n)]


def run(jpegamd, enc, planes, dev, sub, layout, **kw):
    """One BT.709 batch -> (files, the planes of its pass)."""
    via = Bt709(jpegamd, enc, keep_planes=dev)
    files = finish_files(via, YccBatch(jpegamd, via, planes, dev, sub, layout, **kw))[0]
    return files, via.planes


def files_only(jpegamd, enc, planes, dev, sub, layout, **kw):
    return finish_files(enc, YccBatch(jpegamd, Bt709(jpegamd, enc), planes, dev, sub, layout, **kw))[0]


def same_planes(got, want):
    return len(got) == len(want) and all(np.array_equal(g, w) for gp, wp in zip(got, want) for g, w in zip(gp, wp))


def want(oracle, planes8, q, sub):
    """The file by definition: the full-range file of the converted planes."""
    return expected(oracle, mm.convert(planes8, sub), q, sub)


def check(jpegamd, oracle, enc, planes8, dev, sub, layout, q=0, stored=None, **kw):
    """One batch: planes8 are the 8-bit full-range BT.709 planes of what is stored (`stored`: the stored samples where they differ)."""
    files, got = run(jpegamd, enc, stored or planes8, dev, sub, layout, quality=q, **kw)
    assert same_planes(got, [mm.convert(p, sub) for p in planes8]), ("planes", sub, layout, q, kw)
    assert files == [want(oracle, p, q, sub) for p in planes8], ("files", sub, layout, q, kw)


# ---- 1. every (cb, cr) pair ----------------------------------------------------------------------------------------------------------
def every_pair_picture():
    """256 x 256 at 4:4:4: Cb = column, Cr = row; Y cycles through 0, 255, the values whose sums land on 0 and 255 exactly, and values
    five levels past either: both clamps of Y' fire, and both are just missed."""
    cr, cb = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    ty = mm.terms(cb.astype(np.int64) - 128, cr.astype(np.int64) - 128)[0]
    choice = (np.arange(256)[:, None] * 3 + np.arange(256)[None, :]) % 6
    cands = [np.zeros_like(ty), np.full_like(ty, 255), -ty, 255 - ty, -ty - 5, 255 - ty + 5]
    y = np.clip(np.choose(choice, cands), 0, 255).astype(np.uint8)
    raw = y.astype(np.int64) + ty
    assert raw.min() < 0 and raw.max() > 255 and (raw == 0).any() and (raw == 255).any() and (y == 0).any() and (y == 255).any()
    return y, cb, cr


def test_every_pair(jpegamd, oracle, dev):
    p = every_pair_picture()
    enc = jpegamd.Encoder(256, rows_for(1, 256))
    conv = mm.convert(p, S444)
    assert set(conv[0].ravel()) >= {0, 255} and set(conv[1].ravel()) >= {0, 255} and set(conv[2].ravel()) >= {0, 255}
    for q in (0, 100):
        assert want(oracle, p, q, S444) != expected(oracle, p, q, S444)                # the matrix changes the file
        for layout in LAYOUTS:
            check(jpegamd, oracle, enc, [p], dev, S444, layout, q)


# ---- 2. sizes, subsamplings, layouts -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", [S444, S420])
@pytest.mark.parametrize("w,h", [(1, 1), (17, 9), (48, 32), (522, 38)])
def test_sizes(jpegamd, oracle, dev, w, h, sub):
    """(522, 38): a full 32-block interior chroma tile plus an edge tile at 4:2:0, and more than one thread row of the pass; the odd
    sizes put the last luma column and row on a chroma sample of their own."""
    planes = [random_planes(w, h, sub, 4000 * w + 10 * h + sub + k) for k in range(2)]
    enc = jpegamd.Encoder(w, rows_for(2, h))
    for q in (0, 90):
        for layout in LAYOUTS:
            check(jpegamd, oracle, enc, planes, dev, sub, layout, q)


# ---- 3. 4:2:2 and packed frames ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(522, 38), (18, 9)])
def test_422_and_packed(jpegamd, oracle, dev, w, h):
    planes = [random_planes(w, h, S422, 5000 * w + h + k) for k in range(2)]
    enc = jpegamd.Encoder(w, rows_for(2, h))
    for layout in YCC_LAYOUTS:                                    # I422, NV16, NV61, YUYV, UYVY
        check(jpegamd, oracle, enc, planes, dev, S422, layout)


def test_packed_odd_width(jpegamd, oracle, dev):
    """The second Y byte of a row's last group is not part of the picture (pack_yuyv poisons it): the byte path of the right edge."""
    w, h = 17, 9
    planes = [random_planes(w, h, S422, 61 + k) for k in range(2)]
    enc = jpegamd.Encoder(w, rows_for(2, h))
    for layout in (YUYV, UYVY):
        check(jpegamd, oracle, enc, planes, dev, S422, layout)


# ---- 4. loader paths -----------------------------------------------------------------------------------------------------------------
def test_loader_paths_give_one_result(jpegamd, oracle, dev):
    """Vector and dword loads, the byte path (a shifted plane, a stride off the grid) and 64-bit row addresses (a stride of 2^24 and
    more) give the same planes and the same file."""
    w, h = 522, 38
    enc = jpegamd.Encoder(w, rows_for(3, h))
    for sub in (S420, S444):
        cw, _ = chroma_dims(w, h, sub)
        planes = [random_planes(w, h, sub, 27 + k) for k in range(3)]
        for layout in LAYOUTS:
            row = cw if layout == PLANES else 2 * cw
            aligned = -row % 4 + row
            for kw in (dict(y_stride=w + 2, c_stride=aligned),                           # the aligned case
                       dict(y_shifts=[0, 1, 0], y_stride=w + 2, c_stride=aligned),       # one Y plane off a dword boundary
                       dict(c_shifts=[0, 0, 1], y_stride=w + 2, c_stride=aligned),       # one chroma plane
                       dict(y_stride=w + 1, c_stride=aligned),                           # strides off multiples of 4
                       dict(y_stride=w + 2, c_stride=aligned + 3)):
                check(jpegamd, oracle, enc, planes, dev, sub, layout, **kw)
    w, h = 17, 9
    enc = jpegamd.Encoder(w, rows_for(1, h))
    planes = [random_planes(w, h, S420, 88)]
    check(jpegamd, oracle, enc, planes, dev, S420, CBCR, c_stride=WIDE_STRIDE)
    check(jpegamd, oracle, enc, planes, dev, S420, PLANES, y_stride=WIDE_STRIDE)


# ---- 5. range and depth: the maps first, the matrix on their bytes ---------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(522, 38), (17, 9)])
def test_limited_range(jpegamd, oracle, dev, w, h):
    """Uniform noise over 0 .. 255: about a quarter of the samples clamp in the range map, either way."""
    stored = [random_planes(w, h, S420, 6000 * w + h + k) for k in range(2)]
    enc = jpegamd.Encoder(w, rows_for(2, h))
    for layout in (PLANES, CBCR):
        check(jpegamd, oracle, enc, [rm.expand(p) for p in stored], dev, S420, layout, stored=stored, sample_range=jpegamd.RANGE_LIMITED)


@pytest.mark.parametrize("align", [dm.MSB, dm.LSB])
@pytest.mark.parametrize("sample_range", [dm.FULL, dm.LIMITED])
@pytest.mark.parametrize("w,h", [(522, 38), (17, 9)])
def test_ten_bit(jpegamd, oracle, dev, w, h, sample_range, align):
    """Words uniform over 0 .. 65535: LSB-aligned words beyond 1023 clamp, and both clamps of the limited maps occur."""
    cw, ch = chroma_dims(w, h, S420)
    stored = []
    for k in range(2):
        rng = np.random.default_rng(7000 * w + h + k)
        stored.append(tuple(rng.integers(0, 65536, s).astype(np.uint16) for s in ((h, w), (ch, cw), (ch, cw))))
    enc = jpegamd.Encoder(w, rows_for(2, h))
    fmt = jpegamd.SAMPLES_10_MSB if align == dm.MSB else jpegamd.SAMPLES_10_LSB
    srange = jpegamd.RANGE_LIMITED if sample_range == dm.LIMITED else jpegamd.RANGE_FULL
    for layout in (PLANES, CBCR):
        check(jpegamd, oracle, enc, [dm.narrow(p, sample_range, align) for p in stored], dev, S420, layout, stored=stored,
              sample_range=srange, sample_format=fmt)


# ---- 6. neighbours on one context ------------------------------------------------------------------------------------------------------
def test_neighbours_queued_on_one_context(jpegamd, oracle, dev):
    """Five calls without a finish in between: BT.709, an RGB colour batch (it shares the plane scratch), BT.601 through the new entry,
    the old entry, then BT.709 of a larger geometry (the scratch grows)."""
    w, h, w2, h2 = 160, 40, 522, 38
    enc = jpegamd.Encoder(w2, rows_for(2, max(h, h2)))
    for sub, layout in ((S420, CBCR), (S444, PLANES)):
        planes = [random_planes(w, h, sub, 400 + sub + k) for k in range(2)]
        larger = [random_planes(w2, h2, sub, 410 + sub + k) for k in range(2)]
        rgbs = pictures(jpegamd, w, h, 2, seed=sub)
        a = YccBatch(jpegamd, Bt709(jpegamd, enc), planes, dev, sub, layout)
        b = ColorBatch(jpegamd, enc, rgbs, dev, sub)
        c = YccBatch(jpegamd, Bt709(jpegamd, enc, matrix=jpegamd.MATRIX_BT601, direct=True), planes, dev, sub, layout)
        d = YccBatch(jpegamd, enc, planes, dev, sub, layout)
        e = YccBatch(jpegamd, Bt709(jpegamd, enc, direct=True), larger, dev, sub, layout)
        enc.finish()
        plain = [expected(oracle, p, 0, sub) for p in planes]
        converted = [want(oracle, p, 0, sub) for p in planes]
        assert intact_files(a) == converted and converted != plain, (sub, layout)
        assert intact_files(b) == [model(oracle, r, 0, sub) for r in rgbs], (sub, layout)
        assert intact_files(c) == plain and intact_files(d) == plain, (sub, layout)
        assert intact_files(e) == [want(oracle, p, 0, sub) for p in larger], (sub, layout)
    # the older entries' files for the same planes, on a context that never saw a BT.709 call
    fresh = jpegamd.Encoder(w, rows_for(2, h))
    assert finish_files(fresh, YccBatch(jpegamd, fresh, planes, dev, S444, PLANES, entry="samples", sample_range=jpegamd.RANGE_FULL))[0] == plain


# ---- 7. both pipelines, and a chroma launch that starts on a Cr plane ------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", ["PIPELINE_PAIR", "PIPELINE_STITCH"])
def test_pipelines_with_a_launch_that_starts_on_a_cr_plane(jpegamd, oracle, dev, pipeline):
    w, h, count = 522, 38, 3
    pipe = getattr(jpegamd, pipeline)
    group, launches, _, _ = jpegamd._chroma_groups(w, rows_for(count, h), w, h, count, S444, pipe)
    assert group % 2 == 1 and launches > 1, (group, launches)
    enc = jpegamd.Encoder(w, rows_for(count, h))
    enc.set_pipeline(pipe)
    planes = [random_planes(w, h, S444, 290 + k) for k in range(count)]
    files = [want(oracle, p, 0, S444) for p in planes]
    assert len(set(files)) == count
    for layout in LAYOUTS:
        assert files_only(jpegamd, enc, planes, dev, S444, layout) == files, layout


# ---- 8. capacity -----------------------------------------------------------------------------------------------------------------------
def test_one_picture_of_a_bt709_batch_one_byte_short(jpegamd, oracle, dev):
    w, h = 160, 96
    enc = jpegamd.Encoder(w, rows_for(4, h))
    for sub, layout in ((S420, CBCR), (S444, PLANES)):
        planes = [smooth_planes(w, h, sub, 7), random_planes(w, h, sub, 9), smooth_planes(w, h, sub, 8), smooth_planes(w, h, sub, 6)]
        exp = [want(oracle, p, 0, sub) for p in planes]
        cap = len(exp[1]) - 1                                    # one byte short for the noise picture alone
        assert cap > max(len(exp[k]) for k in (0, 2, 3))
        b = YccBatch(jpegamd, Bt709(jpegamd, enc), planes, dev, sub, layout, cap=cap)
        with pytest.raises(jpegamd.JpegAmdError) as err:
            enc.finish()
        assert err.value.code == -8
        res = b.results()
        assert all(ok for _, ok in res)                          # the canaries: nothing behind any capacity
        assert int(b.sizes[1].item()) == 0
        assert [res[k][0] for k in (0, 2, 3)] == [exp[k] for k in (0, 2, 3)], (sub, layout)
        assert files_only(jpegamd, enc, planes, dev, sub, layout, cap=cap + 1) == exp, (sub, layout)     # the exact capacity fits


# ---- 9. the tensor entries -------------------------------------------------------------------------------------------------------------
def torch_convert_444(y, cb, cr):
    """The definition in torch integer ops on the device (4:4:4: every plane has the luma's shape)."""
    c = mm.coeffs()
    b, r = cb.to(torch.int32) - 128, cr.to(torch.int32) - 128
    t = [(c[2 * k] * b + c[2 * k + 1] * r + (1 << (mm.SHIFT - 1))) >> mm.SHIFT for k in range(3)]
    return ((y.to(torch.int32) + t[0]).clamp(0, 255).to(torch.uint8), (128 + t[1]).clamp(0, 255).to(torch.uint8),
            (128 + t[2]).clamp(0, 255).to(torch.uint8))


def test_tensor_entry_against_torch(jpegamd, oracle, dev):
    w, h, n = 48, 32, jpegamd.MAX_BATCH + 1                       # 33 pictures: the call splits
    rng = np.random.default_rng(31)
    hy, hcb, hcr = (rng.integers(0, 256, (n, h, w), np.uint8) for _ in range(3))
    y, cb, cr = (torch.from_numpy(p).to(dev) for p in (hy, hcb, hcr))
    files = jpegamd.encode_ycbcr_batch(y, cb, cr, subsampling=S444, matrix="bt709")
    ny, ncb, ncr = torch_convert_444(y, cb, cr)
    assert files == jpegamd.encode_ycbcr_batch(ny, ncb, ncr, subsampling=S444)
    assert files == jpegamd.encode_ycbcr_batch(ny, ncb, ncr, subsampling=S444, matrix="bt601")
    for i in (0, n - 1):
        assert files[i] == want(oracle, (hy[i], hcb[i], hcr[i]), 0, S444)
    assert files[:3] != jpegamd.encode_ycbcr_batch(y[:3], cb[:3], cr[:3], subsampling=S444)
    pairs = torch.stack([cb, cr], dim=3)
    assert jpegamd.encode_ycbcr_batch(y, pairs, subsampling=S444, matrix="bt709") == files
    assert jpegamd.encode_ycbcr_batch(y, pairs.flip(3).contiguous(), subsampling=S444, order="crcb", matrix="bt709") == files
    # grey chroma: the matrix is the identity there
    grey = torch.full_like(cb[:2], 128)
    assert jpegamd.encode_ycbcr_batch(y[:2], grey, grey, subsampling=S444, matrix="bt709") == \
        jpegamd.encode_ycbcr_batch(y[:2], grey, grey, subsampling=S444)


def test_tensor_entries_16_bit_and_packed(jpegamd, oracle, dev):
    w, h, n = 48, 32, 3
    rng = np.random.default_rng(37)
    y16 = rng.integers(0, 65536, (n, h, w)).astype(np.uint16)
    c16 = rng.integers(0, 65536, (n, h // 2, w // 2, 2)).astype(np.uint16)
    ty, tc = torch.from_numpy(y16.view(np.int16)).to(dev), torch.from_numpy(c16.view(np.int16)).to(dev)
    for align, srange in ((dm.MSB, dm.LIMITED), (dm.LSB, dm.FULL)):
        files = jpegamd.encode_ycbcr16_batch(ty, tc, sample_range=srange, align=align, matrix="bt709")
        for i in range(n):
            p8 = dm.narrow((y16[i], np.ascontiguousarray(c16[i, :, :, 0]), np.ascontiguousarray(c16[i, :, :, 1])), srange, align)
            assert files[i] == want(oracle, p8, 0, S420), (align, srange, i)
        assert files != jpegamd.encode_ycbcr16_batch(ty, tc, sample_range=srange, align=align)
    # packed frames: Y in byte 0 of every pixel, Cb / Cr in byte 1
    frames = torch.from_numpy(rng.integers(0, 256, (n, h, w, 2), np.uint8)).to(dev)
    got = jpegamd.encode_yuyv_batch(frames, matrix="bt709")
    assert got != jpegamd.encode_yuyv_batch(frames) and got == jpegamd.encode_yuyv_batch(frames.flip(3).contiguous(), order="uyvy", matrix="bt709")
    for i in range(n):
        fh = frames[i].cpu().numpy().reshape(h, w // 2, 4)
        p8 = (np.ascontiguousarray(frames[i, :, :, 0].cpu().numpy()), np.ascontiguousarray(fh[:, :, 1]), np.ascontiguousarray(fh[:, :, 3]))
        assert got[i] == want(oracle, p8, 0, S422), i
    lim = jpegamd.encode_yuyv_batch(frames[:1], sample_range="limited", matrix="bt709")
    fh = frames[0].cpu().numpy().reshape(h, w // 2, 4)
    p8 = rm.expand((np.ascontiguousarray(frames[0, :, :, 0].cpu().numpy()), np.ascontiguousarray(fh[:, :, 1]), np.ascontiguousarray(fh[:, :, 3])))
    assert lim == [want(oracle, p8, 0, S422)]
