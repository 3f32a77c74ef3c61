"""Float pictures (jpegamd_encode_float_batch_async and its twins) through the C-ABI into the HIP kernels.  Two exact comparisons
throughout: the planes k_float_planes_batch leaves in scratch (jpegamd_debug_float_planes), sample for sample against tests/float_model.py;
and the files, byte for byte against BOTH the Python file model of the quantised bytes and the existing uint8 entry run on those bytes.
Every test needs an MI355X.

The cross product of section 3 is reduced: every walk x sample type x subsampling runs at two geometries, one of them odd both ways or
narrower than a thread's run, chosen in rotation so that all ten geometries of the list appear; the plan is asserted below."""
from __future__ import annotations

import ctypes as C
import itertools
from pathlib import Path

import numpy as np
import pytest

import float_model as fm
import gray_scan_fixtures as gfx
import huffman_model as hm
import metadata_model as meta
import mjpeg_support as msup
import progressive_script_fixtures as pfx
import scan_model as sm
from gpu_support import GRAY, S420, S422, S444, Outputs, dev, intact_files, model, rows_for     # noqa: F401
from gpu_support import stream as current_stream

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

WALKS = ("planar", "packed3", "rgba", "bgr", "wide", "shifted")
# what is encoded: a colour subsampling, the luma of three planes, or a single channel
TARGETS = (S444, S420, S422, "luma", "single")
GEOMETRIES = [(1, 1), (2, 2), (3, 3), (7, 1), (8, 2), (9, 3), (15, 5), (16, 16), (17, 9), (33, 31)]
ODD = [(1, 1), (3, 3), (7, 1), (9, 3), (15, 5), (17, 9), (33, 31)]
SCANS_DIR = Path(__file__).resolve().parents[1] / "tools" / "scans"


def plan():
    """(walk, sample type, target) -> its two geometries."""
    out = {}
    for k, combo in enumerate(itertools.product(WALKS, fm.TYPES, TARGETS)):
        out[combo] = (ODD[k % len(ODD)], GEOMETRIES[(3 * k + 1) % len(GEOMETRIES)])
    return out


PLAN = plan()
assert all(g[0] in ODD for g in PLAN.values()) and {g for pair in PLAN.values() for g in pair} == set(GEOMETRIES)


# ---- samples ------------------------------------------------------------------------------------------------------------------------
def random_bits(rng, shape, sample_type):
    """Mostly samples a little beyond [0, 1], every twentieth an arbitrary bit pattern."""
    vals = (rng.random(shape) * 1.2 - 0.1).astype(np.float32)
    if sample_type == fm.F32:
        bits = vals.view(np.uint32).copy()
    elif sample_type == fm.F16:
        bits = vals.astype(np.float16).view(np.uint16).copy()
    else:
        bits = (vals.view(np.uint32) >> 16).astype(np.uint16)
    wild = rng.integers(0, 1 << (8 * fm.SAMPLE_BYTES[sample_type]), shape, dtype=np.uint64).astype(bits.dtype)
    return np.where(rng.integers(0, 20, shape) == 0, wild, bits)


def to_device(arr, dev):
    """An array of bit patterns -> a device tensor of the same bytes."""
    signed = np.ascontiguousarray(arr).view(np.int32 if arr.dtype == np.uint32 else np.int16)
    return torch.from_numpy(signed.copy()).to(dev)


class Stored:
    """One picture's samples (bits [H, W, C], C = 3 or 1) on the device as `walk` says -> .ptrs (R, G, B), .row, .pixel in bytes."""

    def __init__(self, bits, sample_type, walk, dev, rng):
        h, w, c = bits.shape
        size = fm.SAMPLE_BYTES[sample_type]
        filler = lambda shape: random_bits(rng, shape, sample_type)
        if walk in ("planar", "wide", "shifted"):
            pad = 5 if walk == "wide" else 0
            lead = 1 if walk == "shifted" else 0                   # one sample in: no 16-byte load applies to an aligned allocation
            buf = filler((lead + c * h * (w + pad),))
            view = buf[lead:].reshape(c, h, w + pad)
            view[:, :, :w] = bits.transpose(2, 0, 1)
            self.t = to_device(buf, dev)
            base = self.t.data_ptr() + lead * size
            self.ptrs = tuple(base + k * h * (w + pad) * size for k in range(c))
            self.row, self.pixel = (w + pad) * size, size
        else:
            group = 4 if walk == "rgba" else 3
            buf = filler((h, w, group))
            order = (2, 1, 0) if walk == "bgr" else (0, 1, 2)
            for k in range(c):
                buf[:, :, order[k]] = bits[:, :, k]
            self.t = to_device(buf, dev)
            self.ptrs = tuple(self.t.data_ptr() + order[k] * size for k in range(c))
            self.row, self.pixel = group * w * size, group * size

    def image(self, jpegamd, w, h, q=0):
        return jpegamd.Encoder.float_image(self.ptrs, w, h, self.row, self.pixel, q)


def float_planes(jpegamd, enc, imgs, sub, sample_type, scale, offset, dev):
    """jpegamd_debug_float_planes -> [(y, cb, cr)] or [(y,)] picture by picture, as numpy."""
    n, w, h = len(imgs), imgs[0].width, imgs[0].height
    cw, ch = (w if sub == S444 else (w + 1) // 2), ((h + 1) // 2 if sub == S420 else h)
    shapes = [(h, w)] + ([(ch, cw), (ch, cw)] if sub else [])
    bufs = [torch.full((n, hh, ww), 0xA5, dtype=torch.uint8, device=dev) for hh, ww in shapes]
    ptrs = [C.c_void_p(b.data_ptr()) for b in bufs] + [None] * (3 - len(bufs))
    arr = (jpegamd.FloatImage * n)(*imgs)
    rc = jpegamd.lib.jpegamd_debug_float_planes(enc._h, arr, n, int(sub), int(sample_type), C.c_float(scale), C.c_float(offset), *ptrs,
                                                C.c_void_p(current_stream()))
    assert rc == 0, rc
    host = [b.cpu().numpy() for b in bufs]
    return [tuple(p[i] for p in host) for i in range(n)]


def same_planes(got, want):
    return len(got) == len(want) and all(len(g) == len(w) and all(np.array_equal(a, b) for a, b in zip(g, w)) for g, w in zip(got, want))


# ---- the three routes: a float call, the uint8 call of the same bytes, the model ------------------------------------------------------
def capacity(jpegamd, route, w, h, sub, ri, scans):
    if route == "prog":
        return jpegamd.max_jfif_bytes_progressive_script(w, h, sub, scans)
    if route == "one":
        return jpegamd.max_jfif_bytes_gray_scan(w, h, ri) if sub == 0 else jpegamd.max_jfif_bytes_interleaved_restart(w, h, sub, ri)
    return jpegamd.max_jfif_bytes(w, h) if sub == 0 else jpegamd.max_jfif_bytes_color(w, h, sub)


def queue_float(jpegamd, enc, imgs, dev, route, sub, sample_type, scale, offset, ri=0, scans=None, extra=0):
    w, h = imgs[0].width, imgs[0].height
    out = Outputs(dev, len(imgs), capacity(jpegamd, route, w, h, sub, ri, scans) + extra)
    args = (imgs, sub, sample_type, scale, offset)
    if route == "prog":
        enc.encode_float_progressive_script_batch_async(*args, scans, out.out_ptrs, out.cap, out.size_ptrs, current_stream())
    elif route == "one":
        enc.encode_float_interleaved_batch_async(*args, ri, out.out_ptrs, out.cap, out.size_ptrs, current_stream())
    else:
        enc.encode_float_batch_async(*args, out.out_ptrs, out.cap, out.size_ptrs, current_stream())
    return out


def queue_bytes(jpegamd, enc, pics, dev, route, sub, q=0, ri=0, scans=None, extra=0):
    """The existing uint8 entry of the route on pictures of bytes [H, W, 3] or [H, W, 1] -> (Outputs, what must stay alive)."""
    j = jpegamd
    h, w, c = pics[0].shape
    out = Outputs(dev, len(pics), capacity(j, route, w, h, sub, ri, scans) + extra)
    tail = (out.out_ptrs, out.cap, out.size_ptrs, current_stream())
    if c == 3 and route == "three":                                # the planar entry: colour, or (sub 0) the luma
        keep = [torch.from_numpy(np.ascontiguousarray(p.transpose(2, 0, 1))).to(dev) for p in pics]
        imgs = [j.Encoder.planar_image(tuple(t[k].data_ptr() for k in range(3)), w, h, w, False, q) for t in keep]
        enc.encode_planar_batch_async(imgs, sub, *tail)
    elif c == 3 and route == "one" and sub:
        keep = [torch.from_numpy(np.ascontiguousarray(p.transpose(2, 0, 1))).to(dev) for p in pics]
        imgs = [j.Encoder.planar_image(tuple(t[k].data_ptr() for k in range(3)), w, h, w, False, q) for t in keep]
        enc.encode_planar_interleaved_batch_async(imgs, sub, ri, *tail)
    else:                                                          # packed RGB, or the single channel as a GRAY picture
        keep = [torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p in pics]
        order = j.ORDER_RGB if c == 3 else j.ORDER_GRAY
        imgs = [j.Encoder.image(t.data_ptr(), w, h, c * w, False, order, q) for t in keep]
        if route == "three":
            enc.encode_batch_async(imgs, out.out_ptrs, out.cap, out.size_ptrs, True, current_stream())
        elif route == "one":
            enc.encode_gray_scan_batch_async(imgs, ri, *tail)
        elif sub:
            enc.encode_color_progressive_script_batch_async(imgs, sub, scans, *tail)
        else:
            enc.encode_gray_progressive_script_batch_async(imgs, scans, *tail)
    return out, keep


def as_rgb(pic):
    return pic if pic.shape[2] == 3 else np.repeat(pic, 3, axis=2)       # (the luma of (p, p, p) is p)


def model_file(oracle, pic, route, sub, q=0, ri=0, optimized=False, script=None):
    """The file by definition of a picture of bytes."""
    rgb = as_rgb(pic)
    if route == "three":
        return model(oracle, rgb, q, sub)
    if route == "one":
        if sub == 0:
            return gfx.model(oracle, np.ascontiguousarray(sm.luma_plane(rgb)), q, ri, optimized).file
        return hm.rgb_file(oracle, rgb, q, sub, ri).file if optimized else msup.rgb_model(oracle, rgb, q, sub, ri).file
    if sub == 0:
        return pfx.gray_model(oracle, np.ascontiguousarray(sm.luma_plane(rgb)), q, script or pfx.GRAY_SUCCESSIVE).file
    return pfx.model(oracle, rgb, q, sub, script or pfx.SUCCESSIVE).file


def check_files(jpegamd, oracle, enc, dev, imgs, pics, route, sub, sample_type, scale, offset, q=0, ri=0, scans=None, optimized=False):
    """One float call, finished; the uint8 call of the same bytes, finished; both equal to the model."""
    a = queue_float(jpegamd, enc, imgs, dev, route, sub, sample_type, scale, offset, ri, scans)
    st = enc.finish()
    got = intact_files(a)
    assert st.jfif_bytes == len(got[-1])
    b, keep = queue_bytes(jpegamd, enc, pics, dev, route, sub, q, ri, scans)
    enc.finish()
    ref = intact_files(b)
    del keep
    assert got == ref, ("float entry vs uint8 entry", route, sub, sample_type, scale, offset, q, ri)
    want = [model_file(oracle, p, route, sub, q, ri, optimized, scans) for p in pics]
    assert got == want, ("float entry vs model", route, sub, sample_type, scale, offset, q, ri)
    return got


def check_planes(jpegamd, enc, dev, imgs, pics, sub, sample_type, scale, offset):
    got = float_planes(jpegamd, enc, imgs, sub, sample_type, scale, offset, dev)
    want = [fm.planes(p, sub) if p.shape[2] == 3 else (p[:, :, 0],) for p in pics]
    assert same_planes(got, want), ("planes", sub, sample_type, scale, offset)


def target_of(target):
    """-> (channels, subsampling of the call)."""
    return (1, 0) if target == "single" else ((3, 0) if target == "luma" else (3, target))


# ---- 1. every half-width value --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample_type", [fm.F16, fm.BF16])
def test_every_half_width_value(jpegamd, oracle, dev, sample_type):
    rng = np.random.default_rng(7 + sample_type)
    bits = fm.all_half_patterns()
    enc = jpegamd.Encoder(256, rows_for(1, 256))
    single = Stored(bits[:, :, None], sample_type, "planar", dev, rng)
    perm = [bits, bits.reshape(-1)[rng.permutation(65536)].reshape(256, 256), bits.reshape(-1)[rng.permutation(65536)].reshape(256, 256)]
    colour_bits = np.stack(perm, axis=2)
    colour = Stored(colour_bits, sample_type, "planar", dev, rng)
    for scale, offset in fm.PAIRS:
        pic = fm.bytes_of(bits, sample_type, scale, offset)[:, :, None]
        assert {0, 255} <= set(pic.ravel().tolist())
        check_planes(jpegamd, enc, dev, [single.image(jpegamd, 256, 256)], [pic], 0, sample_type, scale, offset)
        rgb = fm.bytes_of(colour_bits, sample_type, scale, offset)
        check_planes(jpegamd, enc, dev, [colour.image(jpegamd, 256, 256)], [rgb], S444, sample_type, scale, offset)
    scale, offset = fm.PAIRS[0]
    rgb = fm.bytes_of(colour_bits, sample_type, scale, offset)
    check_files(jpegamd, oracle, enc, dev, [colour.image(jpegamd, 256, 256)], [rgb], "three", S444, sample_type, scale, offset)


# ---- 2. float32 edges -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale,offset", [(1.0, 0.0), (255.0, 0.0)])
def test_f32_edges(jpegamd, oracle, dev, scale, offset):
    rng = np.random.default_rng(31)
    bits = np.stack([fm.f32_edge_picture(40 + k) for k in range(3)], axis=2)
    bits[:, :, 1] = np.roll(bits[:, :, 1], 7, axis=1)              # the planted blocks of the three channels do not line up
    bits[:, :, 2] = bits[::-1, :, 2].copy()
    rgb = fm.bytes_of(bits, fm.F32, scale, offset)
    values = set(rgb.ravel().tolist())
    assert {0, 255} <= values
    if scale == 1.0:                                               # both tie directions are in the picture
        ties = fm.bytes_of(fm.f32_bits(np.arange(256, dtype=np.float32) + np.float32(0.5)), fm.F32, 1.0, 0.0)
        assert (ties[0::2] == np.arange(0, 256, 2)).all() and (ties[1:255:2] == np.arange(2, 256, 2)).all()
        assert np.array_equal(rgb[:, :, 0].reshape(-1)[:256], ties)
    enc = jpegamd.Encoder(256, rows_for(1, 256))
    for walk in ("planar", "packed3"):
        s = Stored(bits, fm.F32, walk, dev, rng)
        check_planes(jpegamd, enc, dev, [s.image(jpegamd, 256, 256)], [rgb], S444, fm.F32, scale, offset)
        check_planes(jpegamd, enc, dev, [s.image(jpegamd, 256, 256)], [rgb], S420, fm.F32, scale, offset)
    single = Stored(bits[:, :, :1], fm.F32, "planar", dev, rng)
    check_planes(jpegamd, enc, dev, [single.image(jpegamd, 256, 256)], [rgb[:, :, :1]], 0, fm.F32, scale, offset)
    check_files(jpegamd, oracle, enc, dev, [s.image(jpegamd, 256, 256)], [rgb], "three", S420, fm.F32, scale, offset)


# ---- 3. walks and edges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample_type", fm.TYPES)
@pytest.mark.parametrize("walk", WALKS)
def test_walks_and_edges(jpegamd, oracle, dev, walk, sample_type):
    rng = np.random.default_rng(100 * WALKS.index(walk) + sample_type)
    scale, offset = fm.PAIRS[sample_type % 2]                      # (255, 0) and (127.5, 127.5) in turn
    enc = jpegamd.Encoder(40, rows_for(2, 32))
    for target in TARGETS:
        channels, sub = target_of(target)
        for w, h in PLAN[(walk, sample_type, target)]:
            bits = [random_bits(rng, (h, w, channels), sample_type) for _ in range(2)]
            stored = [Stored(b, sample_type, walk, dev, rng) for b in bits]
            pics = [fm.bytes_of(b, sample_type, scale, offset) for b in bits]
            imgs = [s.image(jpegamd, w, h) for s in stored]
            check_planes(jpegamd, enc, dev, imgs, pics, sub, sample_type, scale, offset)
            check_files(jpegamd, oracle, enc, dev, imgs, pics, "three", sub, sample_type, scale, offset)


@pytest.mark.parametrize("sample_type,walk,sub", [(fm.F32, "planar", S420), (fm.F16, "packed3", S444), (fm.BF16, "rgba", S422)])
def test_a_second_workgroup_in_x(jpegamd, oracle, dev, sample_type, walk, sub):
    w, h = 2049, 2
    rng = np.random.default_rng(5 + sample_type)
    bits = random_bits(rng, (h, w, 3), sample_type)
    s = Stored(bits, sample_type, walk, dev, rng)
    rgb = fm.bytes_of(bits, sample_type, 255.0, 0.0)
    enc = jpegamd.Encoder(w, rows_for(1, h))
    check_planes(jpegamd, enc, dev, [s.image(jpegamd, w, h)], [rgb], sub, sample_type, 255.0, 0.0)
    check_files(jpegamd, oracle, enc, dev, [s.image(jpegamd, w, h)], [rgb], "three", sub, sample_type, 255.0, 0.0)


# ---- 4. batches -----------------------------------------------------------------------------------------------------------------------
def test_batches_of_32_and_of_one(jpegamd, oracle, dev):
    rng = np.random.default_rng(64)
    w = h = 16
    enc = jpegamd.Encoder(w, rows_for(32, h))
    bits = [random_bits(rng, (h, w, 3), fm.F16) for _ in range(32)]
    stored = [Stored(b, fm.F16, "packed3", dev, rng) for b in bits]
    pics = [fm.bytes_of(b, fm.F16, 255.0, 0.0) for b in bits]
    imgs = [s.image(jpegamd, w, h) for s in stored]
    files = check_files(jpegamd, oracle, enc, dev, imgs, pics, "three", S420, fm.F16, 255.0, 0.0)
    assert len(set(files)) == 32
    check_planes(jpegamd, enc, dev, imgs, pics, S420, fm.F16, 255.0, 0.0)
    assert check_files(jpegamd, oracle, enc, dev, imgs[5:6], pics[5:6], "three", S420, fm.F16, 255.0, 0.0) == files[5:6]
    assert check_files(jpegamd, oracle, enc, dev, imgs[:32], pics[:32], "one", S444, fm.F16, 255.0, 0.0)


def test_every_second_picture_of_a_tensor(jpegamd, dev):
    g = torch.Generator().manual_seed(3)
    t = torch.rand(6, 3, 24, 40, generator=g).to(dev)
    q8 = t.mul(255).round().clamp(0, 255).to(torch.uint8)
    assert jpegamd.encode_float_batch(t[::2], subsampling=S444) == jpegamd.encode_tensor_batch(q8[::2], subsampling=S444, layout="chw")
    assert jpegamd.encode_float_batch(t[1::2, :, 3:20, 5:38]) == jpegamd.encode_tensor_batch(q8[1::2, :, 3:20, 5:38].contiguous(), layout="chw")


def test_scratch_growth_then_a_uint8_call_on_one_stream(jpegamd, oracle, dev):
    rng = np.random.default_rng(12)
    enc = jpegamd.Encoder(48, rows_for(3, 40))
    small = [random_bits(rng, (16, 16, 3), fm.F32) for _ in range(2)]
    large = [random_bits(rng, (40, 48, 3), fm.F32) for _ in range(3)]
    s_small = [Stored(b, fm.F32, "planar", dev, rng) for b in small]
    s_large = [Stored(b, fm.F32, "packed3", dev, rng) for b in large]
    p_small = [fm.bytes_of(b, fm.F32, 255.0, 0.0) for b in small]
    p_large = [fm.bytes_of(b, fm.F32, 255.0, 0.0) for b in large]
    # queued back to back, finished once
    a = queue_float(jpegamd, enc, [s.image(jpegamd, 16, 16) for s in s_small], dev, "three", S420, fm.F32, 255.0, 0.0)
    b = queue_float(jpegamd, enc, [s.image(jpegamd, 48, 40) for s in s_large], dev, "three", S420, fm.F32, 255.0, 0.0)
    c, keep = queue_bytes(jpegamd, enc, p_large, dev, "three", S420)
    d = queue_float(jpegamd, enc, [s.image(jpegamd, 48, 40) for s in s_large], dev, "one", 0, fm.F32, 255.0, 0.0)
    enc.finish()
    assert intact_files(a) == [model_file(oracle, p, "three", S420) for p in p_small]
    want = [model_file(oracle, p, "three", S420) for p in p_large]
    assert intact_files(b) == want and intact_files(c) == want
    assert intact_files(d) == [model_file(oracle, p, "three", 0) for p in p_large]     # (the plain grayscale file is the fused entry's)


# ---- 5. one scan ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(17, 9), (33, 31)])
@pytest.mark.parametrize("sub", [S420, S444])
def test_one_scan(jpegamd, oracle, dev, w, h, sub):
    rng = np.random.default_rng(1000 * w + sub)
    enc = jpegamd.Encoder(w, rows_for(2, h))
    sample_type = fm.F32 if sub == S420 else fm.BF16
    bits = [random_bits(rng, (h, w, 3), sample_type) for _ in range(2)]
    stored = [Stored(b, sample_type, "packed3" if w == 17 else "planar", dev, rng) for b in bits]
    pics = [fm.bytes_of(b, sample_type, 255.0, 0.0) for b in bits]
    imgs = [s.image(jpegamd, w, h) for s in stored]
    row = msup.row_interval(w, sub)
    for ri in (0, 1, row):
        check_files(jpegamd, oracle, enc, dev, imgs, pics, "one", sub, sample_type, 255.0, 0.0, ri=ri)
    enc.set_huffman(jpegamd.HUFFMAN_OPTIMIZED)
    try:
        for ri in (0, row):
            check_files(jpegamd, oracle, enc, dev, imgs, pics, "one", sub, sample_type, 255.0, 0.0, ri=ri, optimized=True)
    finally:
        enc.set_huffman(jpegamd.HUFFMAN_STANDARD)


@pytest.mark.parametrize("channels", [1, 3])
def test_gray_scan(jpegamd, oracle, dev, channels):
    w, h = 33, 31
    rng = np.random.default_rng(77 + channels)
    enc = jpegamd.Encoder(w, rows_for(2, h))
    bits = [random_bits(rng, (h, w, channels), fm.F16) for _ in range(2)]
    stored = [Stored(b, fm.F16, "planar" if channels == 1 else "rgba", dev, rng) for b in bits]
    pics = [fm.bytes_of(b, fm.F16, 127.5, 127.5) for b in bits]
    imgs = [s.image(jpegamd, w, h) for s in stored]
    for ri in (0, 3, gfx.interval("row", w)):
        check_files(jpegamd, oracle, enc, dev, imgs, pics, "one", 0, fm.F16, 127.5, 127.5, ri=ri)
    enc.set_huffman(jpegamd.HUFFMAN_OPTIMIZED)
    try:
        check_files(jpegamd, oracle, enc, dev, imgs, pics, "one", 0, fm.F16, 127.5, 127.5, ri=3, optimized=True)
        check_files(jpegamd, oracle, enc, dev, imgs, pics, "one", 0, fm.F16, 127.5, 127.5, ri=0, optimized=True)
    finally:
        enc.set_huffman(jpegamd.HUFFMAN_STANDARD)


# ---- 6. progressive -------------------------------------------------------------------------------------------------------------------
def test_progressive(jpegamd, oracle, dev):
    import jpegamd.progressive_script as ps
    w, h = 33, 31
    rng = np.random.default_rng(606)
    enc = jpegamd.Encoder(w, rows_for(2, h))
    split = ps.parse_scan_script((SCANS_DIR / "split.txt").read_text())
    jpegamd.validate_scan_script(split, 3)
    bits = [random_bits(rng, (h, w, 3), fm.BF16) for _ in range(2)]
    stored = [Stored(b, fm.BF16, "packed3", dev, rng) for b in bits]
    pics = [fm.bytes_of(b, fm.BF16, 255.0, 0.0) for b in bits]
    imgs = [s.image(jpegamd, w, h) for s in stored]
    for scans in (None, split):
        check_files(jpegamd, oracle, enc, dev, imgs, pics, "prog", S420, fm.BF16, 255.0, 0.0, scans=scans)
    for scans in (None, pfx.GRAY_SPLIT):
        check_files(jpegamd, oracle, enc, dev, imgs, pics, "prog", 0, fm.BF16, 255.0, 0.0, scans=scans)
    one = [random_bits(rng, (h, w, 1), fm.F32)]
    s1 = Stored(one[0], fm.F32, "wide", dev, rng)
    check_files(jpegamd, oracle, enc, dev, [s1.image(jpegamd, w, h)], [fm.bytes_of(one[0], fm.F32, 255.0, 0.0)], "prog", 0, fm.F32, 255.0, 0.0,
                scans=pfx.GRAY_SPLIT)


# ---- 7. context settings carry over ---------------------------------------------------------------------------------------------------
def test_quant_tables_and_metadata_carry_over(jpegamd, oracle, dev):
    w, h = 33, 31
    rng = np.random.default_rng(707)
    enc = jpegamd.Encoder(w, rows_for(2, h))
    luma = np.clip(np.arange(64) * 2 + 3, 1, 255).astype(np.uint8)
    chroma = np.clip(200 - np.arange(64) * 3, 1, 255).astype(np.uint8)
    enc.set_quant_tables(luma, chroma)
    enc.set_metadata(comment="float source", icc_profile=meta.icc_like(70000))
    extra = enc.metadata_bytes()
    assert extra > 70000
    bits = [random_bits(rng, (h, w, 3), fm.F32) for _ in range(2)]
    stored = [Stored(b, fm.F32, "planar", dev, rng) for b in bits]
    pics = [fm.bytes_of(b, fm.F32, 255.0, 0.0) for b in bits]
    imgs = [s.image(jpegamd, w, h) for s in stored]
    plain = None
    for route, sub in (("three", S420), ("one", S422), ("prog", S444), ("three", 0)):
        a = queue_float(jpegamd, enc, imgs, dev, route, sub, fm.F32, 255.0, 0.0, extra=extra)
        enc.finish()
        b, keep = queue_bytes(jpegamd, enc, pics, dev, route, sub, extra=extra)
        enc.finish()
        got = intact_files(a)
        assert got == intact_files(b), (route, sub)
        assert all(b"float source" in f[:200000] and len(f) > extra for f in got)
        if route == "three" and sub == S420:
            plain = got
    enc.set_quant_tables(None)
    enc.set_metadata(None)
    back = check_files(jpegamd, oracle, enc, dev, imgs, pics, "three", S420, fm.F32, 255.0, 0.0)
    assert back != plain


# ---- 8. Python ------------------------------------------------------------------------------------------------------------------------
def torch_bytes(t, lo, hi):
    scale, offset = fm.value_range(lo, hi)
    return t.float().mul(scale).add(offset).round().clamp(0, 255).to(torch.uint8)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("lo,hi", [(0.0, 1.0), (-1.0, 1.0)])
def test_python_matches_the_uint8_route(jpegamd, dev, dtype, lo, hi):
    g = torch.Generator().manual_seed(11)
    t = (torch.rand(3, 3, 31, 33, generator=g) * (hi - lo) + lo).to(dtype).to(dev)
    q8 = torch_bytes(t, lo, hi)
    for sub in (S420, S444):
        assert jpegamd.encode_float_batch(t, subsampling=sub, value_range=(lo, hi)) == jpegamd.encode_tensor_batch(q8, subsampling=sub, layout="chw")
    assert jpegamd.encode_float(t[1], value_range=(lo, hi)) == jpegamd.encode_tensor(q8[1], layout="chw")
    hwc = t.permute(0, 2, 3, 1).contiguous()
    assert jpegamd.encode_float_batch(hwc, layout="hwc", value_range=(lo, hi)) == jpegamd.encode_tensor_batch(q8, layout="chw")
    assert jpegamd.encode_float_batch(t[:, 0], layout="gray", value_range=(lo, hi)) == jpegamd.encode_tensor_batch(q8[:, 0].contiguous())
    assert jpegamd.encode_float_batch(t, subsampling=0, value_range=(lo, hi)) == jpegamd.encode_tensor_batch(q8, subsampling=0, layout="chw")


def test_views_go_through_without_a_copy(jpegamd, dev, monkeypatch):
    g = torch.Generator().manual_seed(13)
    t = torch.rand(2, 3, 24, 40, generator=g).to(dev)
    cl = t.contiguous(memory_format=torch.channels_last)
    crop = t[:, :, 2:21, 3:38]
    q8 = torch_bytes(t, 0.0, 1.0)
    seen = []
    real = jpegamd.Encoder.encode_float_batch_async

    def spy(self, imgs, *a, **kw):
        seen.append([(tuple(i.plane), i.row_stride, i.pixel_stride) for i in imgs])
        return real(self, imgs, *a, **kw)

    monkeypatch.setattr(jpegamd.Encoder, "encode_float_batch_async", spy)
    want = jpegamd.encode_tensor_batch(q8, layout="chw")
    assert jpegamd.encode_float_batch(cl) == want
    assert seen[-1] == [(tuple(cl[i].data_ptr() + 4 * k for k in range(3)), 12 * 40, 12) for i in range(2)]
    assert jpegamd.encode_float_batch(crop) == jpegamd.encode_tensor_batch(q8[:, :, 2:21, 3:38].contiguous(), layout="chw")
    assert seen[-1] == [(tuple(crop[i, k].data_ptr() for k in range(3)), 4 * 40, 4) for i in range(2)]
    assert jpegamd.encode_float_batch(cl[:, :, 2:21, 3:38]) == jpegamd.encode_tensor_batch(q8[:, :, 2:21, 3:38].contiguous(), layout="chw")
    assert seen[-1][0][0][0] == cl.data_ptr() + 4 * 3 * (2 * 40 + 3)


def test_python_twins(jpegamd, dev):
    import jpegamd.mjpeg as mj
    import jpegamd.progressive_script as ps
    g = torch.Generator().manual_seed(17)
    t = torch.rand(2, 3, 31, 33, generator=g).to(torch.float16).to(dev)
    q8 = torch_bytes(t, 0.0, 1.0)
    assert mj.encode_float_batch(t, restart_interval="row", huffman="optimized") == \
        mj.encode_tensor_batch(q8, layout="chw", restart_interval="row", huffman="optimized")
    assert mj.encode_float(t[0], subsampling=S444) == mj.encode_tensor(q8[0], subsampling=S444, layout="chw")
    assert mj.encode_float_batch(t[:, 1], layout="gray", restart_interval=2) == mj.encode_gray_batch(q8[:, 1].contiguous(), restart_interval=2)
    hwc8 = q8.permute(0, 2, 3, 1).contiguous()
    assert ps.encode_float_batch(t, scans=pfx.SPLIT) == ps.encode_tensor_batch(hwc8, scans=pfx.SPLIT)
    assert ps.encode_float(t[1]) == ps.encode_tensor(hwc8[1])
    assert ps.encode_float_batch(t[:, 2], layout="gray") == ps.encode_gray_batch(q8[:, 2].contiguous())
    with jpegamd.quant_tables(np.full(64, 9, np.uint8)), jpegamd.metadata(comment="twin"):
        assert jpegamd.encode_float_batch(t) == jpegamd.encode_tensor_batch(q8, layout="chw")
