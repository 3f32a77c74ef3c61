"""10-bit YCbCr input (jpegamd_encode_ycbcr_samples_batch_async, encode_ycbcr16_batch) through the C-ABI into the HIP kernels, byte for
byte against the file the header defines: the 8-bit full-range file -- the CPU models of tests/color_model.py and
tests/color_model_422.py -- of the planes narrowed with numpy by the tables of tests/depth_model.py.  Every test needs an MI355X."""
from __future__ import annotations

import numpy as np
import pytest

import depth_model as dm
import range_model as rm
from gpu_support import (CBCR, CRCB, LAYOUTS, PLANES, S420, S422, S444, WIDE_STRIDE, YccBatch, chroma_dims, dev, intact_files,     # noqa: F401
                         rows_for, run_ycc, smooth_planes)
from gpu_support import ycc_file as expected

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

RANGES = (dm.FULL, dm.LIMITED)
ALIGNS = (dm.MSB, dm.LSB)


def noise_planes(w, h, sub, seed):
    """(y, cb, cr) of uniform noise over ALL 65 536 words: clamps, and junk in the low six bits, occur everywhere."""
    rng = np.random.default_rng(seed)
    cw, ch = chroma_dims(w, h, sub)
    return tuple(rng.integers(0, 65536, s).astype(np.uint16) for s in ((h, w), (ch, cw), (ch, cw)))


def words_of(values, align, seed):
    """10-bit values -> 16-bit words of that alignment; MSB-aligned words get junk in the six bits the map ignores."""
    v = values.astype(np.uint16)
    if align == dm.LSB:
        return v
    return (v << 6) | np.random.default_rng(seed).integers(0, 64, v.shape).astype(np.uint16)


def want(oracle, planes16, q, sub, sample_range, align):
    """The file by definition: the 8-bit full-range file of the numpy-narrowed planes (computed once per distinct input)."""
    return expected(oracle, dm.narrow(planes16, sample_range, align), q, sub)


def fmt_of(jpegamd, align):
    return jpegamd.SAMPLES_10_MSB if align == dm.MSB else jpegamd.SAMPLES_10_LSB


def rng_of(jpegamd, sample_range):
    return jpegamd.RANGE_LIMITED if sample_range == dm.LIMITED else jpegamd.RANGE_FULL


def samples16(jpegamd, sample_range, align):
    """YccBatch's arguments for 16-bit planes of that range and alignment."""
    return dict(sample_range=rng_of(jpegamd, sample_range), sample_format=fmt_of(jpegamd, align))


def run(jpegamd, enc, planes, dev, sub, layout, sample_range, align, **kw):
    return run_ycc(jpegamd, enc, planes, dev, sub, layout, **samples16(jpegamd, sample_range, align), **kw)


# ---- 1. every value, both loaders ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample_range", RANGES)
@pytest.mark.parametrize("w,h", [(32, 32), (522, 38)])
def test_every_value(jpegamd, oracle, dev, w, h, sample_range):
    """All 1024 values of v in every plane.  32 x 32 at 4:4:4: four blocks a row, edge tiles only (the clamped gather); 522 x 38: a
    full 32-block interior tile (the dword loaders) plus an edge tile.  Rounding is really tested: a narrowing that truncates gives
    another file."""
    n = w * h
    a = (np.arange(n) * 37 % 1024).reshape(h, w)                  # 37 is coprime to 1024: every value, neighbours far apart
    b = (np.arange(n)[::-1] * 5 % 1024).reshape(h, w)
    c = np.arange(n).reshape(h, w) % 1024                         # ... and a ramp: neighbours one apart
    for p in (a, b, c):
        assert set(p.ravel().tolist()) == set(range(1024))
    values = [(a, b, c), (c, a, b)]
    enc = jpegamd.Encoder(w, rows_for(2, h))
    for q in (0, 100):
        files = {}
        for align in ALIGNS:
            planes = [tuple(words_of(p, align, 11 + i + 3 * k) for i, p in enumerate(pic)) for k, pic in enumerate(values)]
            files[align] = [want(oracle, p, q, S444, sample_range, align) for p in planes]
            cut = [expected(oracle, dm.narrow_truncating(p, align) if sample_range == dm.FULL
                            else rm.expand(dm.narrow_truncating(p, align)), q, S444) for p in planes]
            assert all(f != t for f, t in zip(files[align], cut))                            # (rounding changes the file)
            for layout in LAYOUTS:
                assert run(jpegamd, enc, planes, dev, S444, layout, sample_range, align, quality=q) == files[align], (q, align, layout)
        assert files[dm.MSB] == files[dm.LSB] and files[dm.MSB][0] != files[dm.MSB][1]       # the junk bits change nothing


# ---- 2. sizes, subsamplings, layouts --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", [S444, S420, S422])
@pytest.mark.parametrize("w,h", [(1, 1), (17, 9), (48, 32), (522, 38)])
def test_sizes(jpegamd, oracle, dev, w, h, sub):
    """Uniform noise over all 65 536 words, two pictures per batch.  (522, 38): a full interior tile plus an edge tile in the Y
    launch everywhere and in the chroma launches at 4:4:4; 261 wide chroma -- a full tile and an edge tile again -- at 4:2:0 / 4:2:2."""
    planes = [noise_planes(w, h, sub, 5000 * w + 10 * h + sub + k) for k in range(2)]
    enc = jpegamd.Encoder(w, rows_for(2, h))
    for sample_range in RANGES:
        for align in ALIGNS:
            files = [want(oracle, p, 0, sub, sample_range, align) for p in planes]
            for layout in LAYOUTS:
                assert run(jpegamd, enc, planes, dev, sub, layout, sample_range, align) == files, (w, h, sub, sample_range, align, layout)


# ---- 3. loader paths ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample_range,align", [(dm.LIMITED, dm.MSB), (dm.FULL, dm.LSB)])
def test_loader_paths_give_one_file(jpegamd, oracle, dev, sample_range, align):
    """Dword loaders, the clamped gather that reads its two bytes separately (a plane shifted by one byte -- words on odd addresses --
    or by two, a stride off the grid, an odd stride) and 64-bit addresses (strides of 2^24 and more) end in the same fragment
    registers: one map behind them, one file."""
    w, h = 522, 38
    enc = jpegamd.Encoder(w, rows_for(3, h))
    for sub in (S420, S444):
        cw, _ = chroma_dims(w, h, sub)
        planes = [noise_planes(w, h, sub, 23 + k) for k in range(3)]
        files = [want(oracle, p, 0, sub, sample_range, align) for p in planes]
        for layout in LAYOUTS:
            row = 2 * cw if layout == PLANES else 4 * cw
            aligned = -row % 4 + row
            base = dict(y_stride=2 * w + 4, c_stride=aligned + 4)
            assert run(jpegamd, enc, planes, dev, sub, layout, sample_range, align, **base) == files           # the aligned case
            for kw in (dict(base, y_shifts=[0, 1, 0]),                                    # one Y plane on odd addresses
                       dict(base, y_shifts=[0, 2, 0]),                                    # ... on word, not dword, boundaries
                       dict(base, c_shifts=[0, 0, 1]),                                    # one chroma plane
                       dict(base, c_shifts=[2, 0, 0]),
                       dict(base, y_stride=2 * w + 2), dict(base, c_stride=aligned + 2),  # strides off multiples of 4
                       dict(base, y_stride=2 * w + 3), dict(base, c_stride=aligned + 1)): # odd strides: every other row on odd addresses
                assert run(jpegamd, enc, planes, dev, sub, layout, sample_range, align, **kw) == files, (sub, layout, kw)
    w, h = 17, 9
    enc = jpegamd.Encoder(w, rows_for(1, h))
    planes = [noise_planes(w, h, S420, 79)]
    files = [want(oracle, planes[0], 0, S420, sample_range, align)]
    assert run(jpegamd, enc, planes, dev, S420, CBCR, sample_range, align, y_stride=1 << 24, c_stride=WIDE_STRIDE) == files
    assert run(jpegamd, enc, planes, dev, S420, PLANES, sample_range, align, c_stride=WIDE_STRIDE) == files


# ---- 4. both pipelines, and a chroma launch that starts on a Cr plane -------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", ["PIPELINE_PAIR", "PIPELINE_STITCH"])
def test_pipelines_with_a_launch_that_starts_on_a_cr_plane(jpegamd, oracle, dev, pipeline):
    w, h, count = 522, 38, 3
    pipe = getattr(jpegamd, pipeline)
    group, launches, _, _ = jpegamd._chroma_groups(w, rows_for(count, h), w, h, count, S444, pipe)
    assert group % 2 == 1 and launches > 1, (group, launches)
    enc = jpegamd.Encoder(w, rows_for(count, h))
    enc.set_pipeline(pipe)
    planes = [noise_planes(w, h, S444, 290 + k) for k in range(count)]
    for sample_range, align in ((dm.LIMITED, dm.MSB), (dm.FULL, dm.LSB)):
        files = [want(oracle, p, 0, S444, sample_range, align) for p in planes]
        assert len(set(files)) == count
        for layout in LAYOUTS:
            assert run(jpegamd, enc, planes, dev, S444, layout, sample_range, align) == files, (sample_range, align, layout)


# ---- 5. 8-bit and 16-bit calls queued on one context ------------------------------------------------------------------------------------
def test_8_bit_and_16_bit_calls_queued_on_one_context(jpegamd, oracle, dev):
    """No finish between the calls: each gives its own file, and the 8-bit files -- through the old entries and through the new one
    with JPEGAMD_SAMPLES_8 -- are what they were."""

    w, h = 522, 38
    enc = jpegamd.Encoder(w, rows_for(2, h))
    for sub, layout in ((S420, CBCR), (S444, PLANES)):
        p16 = [noise_planes(w, h, sub, 400 + sub + k) for k in range(2)]
        p8 = [tuple((p >> 8).astype(np.uint8) for p in pic) for pic in p16]
        a = YccBatch(jpegamd, enc, p16, dev, sub, layout, **samples16(jpegamd, dm.LIMITED, dm.MSB))
        b = YccBatch(jpegamd, enc, p8, dev, sub, layout)
        c = YccBatch(jpegamd, enc, p16, dev, sub, layout, **samples16(jpegamd, dm.FULL, dm.LSB))
        d = YccBatch(jpegamd, enc, p8, dev, sub, layout, sample_range=jpegamd.RANGE_LIMITED)
        e = YccBatch(jpegamd, enc, p16, dev, sub, layout, **samples16(jpegamd, dm.FULL, dm.MSB))
        # 8-bit planes through jpegamd_encode_ycbcr_samples_batch_async itself (Encoder never takes it for SAMPLES_8)
        f = YccBatch(jpegamd, enc, p8, dev, sub, layout, sample_range=jpegamd.RANGE_FULL, entry="samples")
        g = YccBatch(jpegamd, enc, p8, dev, sub, layout, sample_range=jpegamd.RANGE_LIMITED, entry="samples")
        enc.finish()
        fa, fb, fc, fd, fe, ff, fg = (intact_files(x) for x in (a, b, c, d, e, f, g))
        full8 = [expected(oracle, p, 0, sub) for p in p8]
        limited8 = [expected(oracle, rm.expand(p), 0, sub) for p in p8]
        assert fb == full8 and ff == full8 and fd == limited8 and fg == limited8, (sub, layout)
        assert fa == [want(oracle, p, 0, sub, dm.LIMITED, dm.MSB) for p in p16], (sub, layout)
        assert fc == [want(oracle, p, 0, sub, dm.FULL, dm.LSB) for p in p16], (sub, layout)
        assert fe == [want(oracle, p, 0, sub, dm.FULL, dm.MSB) for p in p16], (sub, layout)
        assert len({tuple(x) for x in (fa, fb, fc, fd, fe)}) == 5


# ---- 6. the tensor entry ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("align", ALIGNS)
def test_tensor_entry(jpegamd, oracle, dev, align):
    """33 pictures, so the call splits; int16 and uint16 tensors of one bit pattern; against encode_ycbcr_batch of the planes
    narrowed with torch on the device."""
    w, h, n = 48, 32, jpegamd.MAX_BATCH + 1
    rng = np.random.default_rng(31)
    hy = rng.integers(0, 65536, (n, h, w)).astype(np.uint16)
    hc = rng.integers(0, 65536, (n, h // 2, w // 2, 2)).astype(np.uint16)
    y, cbcr = torch.from_numpy(hy.view(np.int16)).to(dev), torch.from_numpy(hc.view(np.int16)).to(dev)
    val = torch.from_numpy(dm.value_table(align).astype(np.int64)).to(dev)

    def narrowed(t, lut):
        return torch.from_numpy(lut).to(dev)[val[t.to(torch.int64) & 0xFFFF]]

    for sample_range in RANGES:
        files = jpegamd.encode_ycbcr16_batch(y, cbcr, sample_range=sample_range, align=align)
        assert len(files) == n
        assert files == jpegamd.encode_ycbcr_batch(narrowed(y, dm.table(sample_range, False)), narrowed(cbcr, dm.table(sample_range, True)))
        assert files == jpegamd.encode_ycbcr16_batch(y.view(torch.uint16), cbcr.view(torch.uint16), sample_range=sample_range, align=align)
        for i in (0, n - 1):
            assert files[i] == want(oracle, (hy[i], hc[i, :, :, 0], hc[i, :, :, 1]), 0, S420, sample_range, align)
        # two planes, strided rows and pictures, Cr first, another subsampling
        cb, cr = cbcr[:3, :, :, 0].contiguous(), cbcr[:3, :, :, 1].contiguous()
        assert jpegamd.encode_ycbcr16_batch(y[:3], cb, cr, sample_range=sample_range, align=align) == files[:3]
        assert jpegamd.encode_ycbcr16_batch(y[:3], cbcr[:3].flip(3).contiguous(), order="crcb", sample_range=sample_range, align=align) == files[:3]
        wide = torch.zeros(6, h, w + 6, dtype=torch.int16, device=dev)
        wide[::2, :, 3:w + 3] = y[:3]
        assert jpegamd.encode_ycbcr16_batch(wide[::2, :, 3:w + 3], cbcr[:3], sample_range=sample_range, align=align) == files[:3]
        c444 = torch.from_numpy(rng.integers(0, 65536, (2, h, w, 2)).astype(np.uint16).view(np.int16)).to(dev)
        got = jpegamd.encode_ycbcr16_batch(y[:2], c444, subsampling=S444, quality=90, sample_range=sample_range, align=align)
        assert got == jpegamd.encode_ycbcr_batch(narrowed(y[:2], dm.table(sample_range, False)), narrowed(c444, dm.table(sample_range, True)),
                                                 subsampling=S444, quality=90)
    assert jpegamd.encode_ycbcr16_batch(y[:2], cbcr[:2], align=align) != jpegamd.encode_ycbcr16_batch(y[:2], cbcr[:2], align=align, sample_range="limited")


# ---- 7. capacity ------------------------------------------------------------------------------------------------------------------------
def test_one_picture_of_a_16_bit_batch_one_byte_short(jpegamd, oracle, dev):
    w, h = 160, 96
    enc = jpegamd.Encoder(w, rows_for(4, h))

    def widen(planes8, align, seed):                               # photo-like 8-bit planes as 10-bit words: v = 4 s
        return tuple(words_of(p.astype(np.uint16) << 2, align, seed + i) for i, p in enumerate(planes8))

    for sub, layout, sample_range, align in ((S420, CBCR, dm.FULL, dm.MSB), (S444, PLANES, dm.LIMITED, dm.LSB), (S420, CRCB, dm.LIMITED, dm.MSB)):
        planes = [widen(smooth_planes(w, h, sub, 7), align, 1), noise_planes(w, h, sub, 9), widen(smooth_planes(w, h, sub, 8), align, 2),
                  widen(smooth_planes(w, h, sub, 6), align, 3)]
        exp = [want(oracle, p, 0, sub, sample_range, align) for p in planes]
        cap = len(exp[1]) - 1                                    # one byte short for the noise picture alone
        assert cap > max(len(exp[k]) for k in (0, 2, 3))
        b = YccBatch(jpegamd, enc, planes, dev, sub, layout, cap=cap, **samples16(jpegamd, sample_range, align))
        with pytest.raises(jpegamd.JpegAmdError) as err:
            enc.finish()
        assert err.value.code == -8
        res = b.results()
        assert all(ok for _, ok in res)                          # the canaries: nothing behind any capacity
        assert int(b.sizes[1].item()) == 0
        assert [res[k][0] for k in (0, 2, 3)] == [exp[k] for k in (0, 2, 3)], (sub, layout)
        assert run(jpegamd, enc, planes, dev, sub, layout, sample_range, align, cap=cap + 1) == exp, (sub, layout)     # the exact capacity fits
