"""Reduced pictures (jpegamd_encode_reduced_batch_async and its twins) through the C-ABI into the HIP kernels.  Two exact comparisons
throughout: the planes k_reduce_planes_batch leaves in scratch (jpegamd_debug_reduced_planes), sample for sample against
tests/reduce_model.py; and the files, byte for byte against the existing uint8 entry run on the model's reduced bytes.  Every source is
surrounded by random filler bytes (rows wider than the picture, a lead-in byte, RGBA's fourth byte): a read outside the picture that gets
USED changes the result.  Every test needs an MI355X.

The cross product of section 2 is reduced: every walk x target runs at two reduced geometries, one of them odd both ways, with two of the
factors 1, 2, 3, 8 each, chosen in rotation so that every width and height of the lists and, for every walk and every target, every
factor appears; the plan is asserted below."""
from __future__ import annotations

import ctypes as C
import itertools
from pathlib import Path

import numpy as np
import pytest

import float_model as fm
import metadata_model as meta
import mjpeg_support as msup
import progressive_script_fixtures as pfx
import reduce_model as rm
from gpu_support import GRAY, S420, S422, S444, Outputs, dev, intact_files, rows_for     # noqa: F401
from gpu_support import stream as current_stream

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

WALKS = ("planar", "packed3", "rgba", "bgr", "wide", "shifted")
# what is encoded: a colour subsampling, the luma of three planes, or a single channel
TARGETS = (S444, S420, S422, "luma", "single")
FACTORS = (1, 2, 3, 8)
WIDTHS = (1, 2, 3, 4, 5, 7, 8, 9, 17, 33)
HEIGHTS = (1, 2, 3, 9, 16, 31)
# reduced geometries: every width and every height of the lists
GEOMETRIES = [(1, 1), (2, 2), (3, 3), (4, 9), (5, 16), (7, 31), (8, 1), (9, 2), (17, 3), (33, 9), (3, 16), (33, 31)]
ODD = [g for g in GEOMETRIES if g[0] % 2 and g[1] % 2]
SCANS_DIR = Path(__file__).resolve().parents[1] / "tools" / "scans"


def plan():
    """(walk, target) -> its two (reduced geometry, factor)."""
    out = {}
    for k, combo in enumerate(itertools.product(WALKS, TARGETS)):
        out[combo] = ((ODD[k % len(ODD)], FACTORS[k % 4]), (GEOMETRIES[(5 * k + 1) % len(GEOMETRIES)], FACTORS[(k + 2) % 4]))
    return out


PLAN = plan()
assert len(ODD) >= 5 and all(pair[0][0] in ODD for pair in PLAN.values())
assert {g for pair in PLAN.values() for g, _ in pair} == set(GEOMETRIES)
assert {g[0] for g in GEOMETRIES} == set(WIDTHS) and {g[1] for g in GEOMETRIES} == set(HEIGHTS)
for _walk in WALKS:
    assert {f for (wk, _), pair in PLAN.items() if wk == _walk for _, f in pair} == set(FACTORS), _walk
for _target in TARGETS:
    assert {f for (_, tg), pair in PLAN.items() if tg == _target for _, f in pair} == set(FACTORS), _target


def source_size(rw, rh, f, k=0):
    """A source of reduced size rw x rh that is no multiple of f either way (f > 1)."""
    if f == 1:
        return rw, rh
    w, h = f * rw - 1 - k % (f - 1), f * rh - 1 - (k + 1) % (f - 1)
    assert w % f and h % f and rm.reduced_size(w, h, f) == (rw, rh)
    return w, h


# ---- sources ------------------------------------------------------------------------------------------------------------------------
class Stored:
    """One picture's bytes ([H, W, C], C = 3 or 1) on the device as `walk` says, random filler around them -> .ptrs (R, G, B), .row,
    .pixel in bytes."""

    def __init__(self, pic, walk, dev, rng):
        h, w, c = pic.shape
        filler = lambda shape: rng.integers(0, 256, shape, np.uint8)
        if walk in ("planar", "wide", "shifted"):
            pad = 5 if walk == "wide" else 0
            lead = 1 if walk == "shifted" else 0                   # one byte in: no vector load applies to an aligned allocation
            buf = filler((lead + c * h * (w + pad),))
            view = buf[lead:].reshape(c, h, w + pad)
            view[:, :, :w] = pic.transpose(2, 0, 1)
            self.t = torch.from_numpy(buf).to(dev)
            base = self.t.data_ptr() + lead
            self.ptrs = tuple(base + k * h * (w + pad) for k in range(c))
            self.row, self.pixel = w + pad, 1
        else:
            group = 4 if walk == "rgba" else 3
            buf = filler((h, w, group))
            order = (2, 1, 0) if walk == "bgr" else (0, 1, 2)
            for k in range(c):
                buf[:, :, order[k]] = pic[:, :, k]
            self.t = torch.from_numpy(buf).to(dev)
            self.ptrs = tuple(self.t.data_ptr() + order[k] for k in range(c))
            self.row, self.pixel = group * w, group

    def image(self, jpegamd, w, h, q=0):
        return jpegamd.Encoder.strided_image(self.ptrs, w, h, self.row, self.pixel, q)


def random_pics(rng, n, w, h, c):
    return [rng.integers(0, 256, (h, w, c), np.uint8) for _ in range(n)]


def reduced_planes(jpegamd, enc, imgs, sub, f, dev):
    """jpegamd_debug_reduced_planes -> [(y, cb, cr)] or [(y,)] picture by picture, as numpy."""
    n = len(imgs)
    w, h = rm.reduced_size(imgs[0].width, imgs[0].height, f)
    cw, ch = (w if sub == S444 else (w + 1) // 2), ((h + 1) // 2 if sub == S420 else h)
    shapes = [(h, w)] + ([(ch, cw), (ch, cw)] if sub else [])
    bufs = [torch.full((n, hh, ww), 0xA5, dtype=torch.uint8, device=dev) for hh, ww in shapes]
    ptrs = [C.c_void_p(b.data_ptr()) for b in bufs] + [None] * (3 - len(bufs))
    arr = (jpegamd.StridedImage * n)(*imgs)
    rc = jpegamd.lib.jpegamd_debug_reduced_planes(enc._h, arr, n, int(sub), int(f), *ptrs, C.c_void_p(current_stream()))
    assert rc == 0, rc
    host = [b.cpu().numpy() for b in bufs]
    return [tuple(p[i] for p in host) for i in range(n)]


def same_planes(got, want):
    return len(got) == len(want) and all(len(g) == len(w) and all(np.array_equal(a, b) for a, b in zip(g, w)) for g, w in zip(got, want))


def check_planes(jpegamd, enc, dev, imgs, pics, sub, f):
    got = reduced_planes(jpegamd, enc, imgs, sub, f, dev)
    small = [rm.reduce_picture(p, f) for p in pics]
    want = [fm.planes(p, sub) if p.shape[2] == 3 else (p[:, :, 0],) for p in small]
    assert same_planes(got, want), ("planes", sub, f, pics[0].shape)


# ---- the two routes: a reduced call, and the uint8 call of the model's reduced bytes -------------------------------------------------
def capacity(jpegamd, route, w, h, sub, ri, scans):
    if route == "prog":
        return jpegamd.max_jfif_bytes_progressive_script(w, h, sub, scans)
    if route == "one":
        return jpegamd.max_jfif_bytes_gray_scan(w, h, ri) if sub == 0 else jpegamd.max_jfif_bytes_interleaved_restart(w, h, sub, ri)
    return jpegamd.max_jfif_bytes(w, h) if sub == 0 else jpegamd.max_jfif_bytes_color(w, h, sub)


def queue_reduced(jpegamd, enc, imgs, dev, route, sub, f, ri=0, scans=None, extra=0):
    w, h = jpegamd.reduced_size(imgs[0].width, imgs[0].height, f)
    out = Outputs(dev, len(imgs), capacity(jpegamd, route, w, h, sub, ri, scans) + extra)
    if route == "prog":
        enc.encode_reduced_progressive_script_batch_async(imgs, sub, f, scans, out.out_ptrs, out.cap, out.size_ptrs, current_stream())
    elif route == "one":
        enc.encode_reduced_interleaved_batch_async(imgs, sub, f, ri, out.out_ptrs, out.cap, out.size_ptrs, current_stream())
    else:
        enc.encode_reduced_batch_async(imgs, sub, f, out.out_ptrs, out.cap, out.size_ptrs, current_stream())
    return out


def queue_bytes(jpegamd, enc, pics, dev, route, sub, q=0, ri=0, scans=None, extra=0):
    """The existing uint8 entry of the route on pictures of bytes stored as packed RGB ([H, W, 3]) or as ORDER_GRAY ([H, W, 1]) ->
    (Outputs, what must stay alive)."""
    j = jpegamd
    h, w, c = pics[0].shape
    out = Outputs(dev, len(pics), capacity(j, route, w, h, sub, ri, scans) + extra)
    tail = (out.out_ptrs, out.cap, out.size_ptrs, current_stream())
    keep = [torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p in pics]
    imgs = [j.Encoder.image(t.data_ptr(), w, h, c * w, False, j.ORDER_RGB if c == 3 else j.ORDER_GRAY, q) for t in keep]
    if c == 1 or sub == 0:                                         # the grayscale files: of the single channel, or of packed RGB's luma
        if route == "three":
            enc.encode_batch_async(imgs, out.out_ptrs, out.cap, out.size_ptrs, True, current_stream())
        elif route == "one":
            enc.encode_gray_scan_batch_async(imgs, ri, *tail)
        else:
            enc.encode_gray_progressive_script_batch_async(imgs, scans, *tail)
    elif route == "three":
        enc.encode_color_batch_async(imgs, sub, *tail)
    elif route == "one":
        enc.encode_color_interleaved_pixels_batch_async(imgs, sub, ri, *tail)
    else:
        enc.encode_color_progressive_script_batch_async(imgs, sub, scans, *tail)
    return out, keep


def check_files(jpegamd, enc, dev, imgs, pics, route, sub, f, q=0, ri=0, scans=None):
    """One reduced call, finished; the uint8 call of the model's reduced bytes, finished; equal byte for byte."""
    a = queue_reduced(jpegamd, enc, imgs, dev, route, sub, f, ri, scans)
    st = enc.finish()
    got = intact_files(a)
    assert st.jfif_bytes == len(got[-1])
    small = [rm.reduce_picture(p, f) for p in pics]
    b, keep = queue_bytes(jpegamd, enc, small, dev, route, sub, q, ri, scans)
    enc.finish()
    ref = intact_files(b)
    del keep
    assert all(len(x) > 100 and x[:2] == b"\xff\xd8" and x[-2:] == b"\xff\xd9" for x in ref)
    assert got == ref, ("reduced entry vs uint8 entry", route, sub, f, q, ri, pics[0].shape)
    return got


def target_of(target):
    """-> (channels, subsampling of the call)."""
    return (1, 0) if target == "single" else ((3, 0) if target == "luma" else (3, target))


# ---- 1. every edge count --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", range(2, rm.MAX_REDUCE + 1))
def test_every_edge_count(jpegamd, dev, f):
    """(f + bw) x (f + bh) for every bw, bh in 1..f: the corner box has n = bw bh, the last column / row boxes bw f / f bh."""
    rng = np.random.default_rng(900 + f)
    enc = jpegamd.Encoder(8, rows_for(1, 8))
    seen = set()
    for bw in range(1, f + 1):
        for bh in range(1, f + 1):
            w, h = f + bw, f + bh
            counts = rm.box_counts(w, h, f)
            assert counts.shape == (2, 2) and counts[1, 1] == bw * bh and counts[0, 1] == bw * f and counts[1, 0] == f * bh
            seen |= set(counts.ravel().tolist())
            pics = random_pics(rng, 1, w, h, 1)
            s = Stored(pics[0], "planar", dev, rng)
            check_planes(jpegamd, enc, dev, [s.image(jpegamd, w, h)], pics, 0, f)
    assert seen == {a * b for a in range(1, f + 1) for b in range(1, f + 1)}
    w = h = 2 * f - 1
    white = np.full((h, w, 1), 255, np.uint8)
    s = Stored(white, "planar", dev, rng)
    got = reduced_planes(jpegamd, enc, [s.image(jpegamd, w, h)], 0, f, dev)
    assert got[0][0].min() == 255 and got[0][0].shape == (2, 2)


# ---- 2. walks, targets and seams ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("walk", WALKS)
def test_walks_and_seams(jpegamd, dev, walk):
    rng = np.random.default_rng(100 * WALKS.index(walk))
    enc = jpegamd.Encoder(40, rows_for(2, 32))
    for target in TARGETS:
        channels, sub = target_of(target)
        for k, ((rw, rh), f) in enumerate(PLAN[(walk, target)]):
            w, h = source_size(rw, rh, f, k + WALKS.index(walk))
            pics = random_pics(rng, 2, w, h, channels)
            stored = [Stored(p, walk, dev, rng) for p in pics]
            imgs = [s.image(jpegamd, w, h) for s in stored]
            check_planes(jpegamd, enc, dev, imgs, pics, sub, f)
            check_files(jpegamd, enc, dev, imgs, pics, "three", sub, f)


@pytest.mark.parametrize("f", [1, 8])
@pytest.mark.parametrize("walk,sub", [("planar", S420), ("packed3", S444), ("rgba", S422), ("shifted", 0)])
def test_a_second_workgroup_in_x(jpegamd, dev, walk, sub, f):
    rw, rh = 2049, 2
    w, h = (rw, rh) if f == 1 else (16385, 9)
    assert rm.reduced_size(w, h, f) == (rw, rh)
    rng = np.random.default_rng(5 + f)
    pics = random_pics(rng, 1, w, h, 3)
    s = Stored(pics[0], walk, dev, rng)
    enc = jpegamd.Encoder(rw, rows_for(1, rh))
    check_planes(jpegamd, enc, dev, [s.image(jpegamd, w, h)], pics, sub, f)
    check_files(jpegamd, enc, dev, [s.image(jpegamd, w, h)], pics, "three", sub, f)


# ---- 3. batches -----------------------------------------------------------------------------------------------------------------------
def test_batches_of_32_and_of_one(jpegamd, dev):
    rng = np.random.default_rng(64)
    f, w, h = 2, 31, 33
    rw, rh = rm.reduced_size(w, h, f)
    enc = jpegamd.Encoder(rw, rows_for(32, rh))
    pics = random_pics(rng, 32, w, h, 3)
    stored = [Stored(p, "packed3", dev, rng) for p in pics]
    imgs = [s.image(jpegamd, w, h) for s in stored]
    files = check_files(jpegamd, enc, dev, imgs, pics, "three", S420, f)
    assert len(set(files)) == 32
    check_planes(jpegamd, enc, dev, imgs, pics, S420, f)
    assert check_files(jpegamd, enc, dev, imgs[5:6], pics[5:6], "three", S420, f) == files[5:6]
    assert check_files(jpegamd, enc, dev, imgs, pics, "one", S444, f)


def test_scratch_growth_then_a_uint8_call_on_one_stream(jpegamd, dev):
    rng = np.random.default_rng(12)
    enc = jpegamd.Encoder(48, rows_for(3, 40))
    small = random_pics(rng, 2, 31, 29, 3)                         # reduced by 2: 16 x 15
    large = random_pics(rng, 3, 143, 119, 3)                       # reduced by 3: 48 x 40
    s_small = [Stored(p, "planar", dev, rng) for p in small]
    s_large = [Stored(p, "packed3", dev, rng) for p in large]
    r_small = [rm.reduce_picture(p, 2) for p in small]
    r_large = [rm.reduce_picture(p, 3) for p in large]
    assert r_large[0].shape == (40, 48, 3)
    # queued back to back, finished once
    a = queue_reduced(jpegamd, enc, [s.image(jpegamd, 31, 29) for s in s_small], dev, "three", S420, 2)
    b = queue_reduced(jpegamd, enc, [s.image(jpegamd, 143, 119) for s in s_large], dev, "three", S420, 3)
    c, keep = queue_bytes(jpegamd, enc, r_large, dev, "three", S420)
    d = queue_reduced(jpegamd, enc, [s.image(jpegamd, 143, 119) for s in s_large], dev, "one", 0, 3)
    enc.finish()
    got_a, got_b, got_c, got_d = intact_files(a), intact_files(b), intact_files(c), intact_files(d)
    # the references, each in a call of its own
    ra, keep_a = queue_bytes(jpegamd, enc, r_small, dev, "three", S420)
    enc.finish()
    rd, keep_d = queue_bytes(jpegamd, enc, r_large, dev, "three", 0)
    enc.finish()
    assert got_a == intact_files(ra)
    assert got_b == got_c and len(set(got_b)) == 3
    assert got_d == intact_files(rd)                               # (the plain grayscale file is the fused entry's)


# ---- 4. routes ------------------------------------------------------------------------------------------------------------------------
ODD_W, ODD_H, ODD_F = 97, 92, 3                                    # reduced 33 x 31, the last boxes 1 wide and 2 tall


@pytest.mark.parametrize("sub", [S420, S444])
def test_one_scan(jpegamd, dev, sub):
    rng = np.random.default_rng(1000 + sub)
    rw, rh = rm.reduced_size(ODD_W, ODD_H, ODD_F)
    assert (rw, rh) == (33, 31)
    enc = jpegamd.Encoder(rw, rows_for(2, rh))
    pics = random_pics(rng, 2, ODD_W, ODD_H, 3)
    stored = [Stored(p, "packed3" if sub == S420 else "planar", dev, rng) for p in pics]
    imgs = [s.image(jpegamd, ODD_W, ODD_H) for s in stored]
    row = msup.row_interval(rw, sub)
    for ri in (0, 1, row):
        check_files(jpegamd, enc, dev, imgs, pics, "one", sub, ODD_F, ri=ri)
    enc.set_huffman(jpegamd.HUFFMAN_OPTIMIZED)
    try:
        for ri in (0, 1, row):
            check_files(jpegamd, enc, dev, imgs, pics, "one", sub, ODD_F, ri=ri)
    finally:
        enc.set_huffman(jpegamd.HUFFMAN_STANDARD)


@pytest.mark.parametrize("channels", [1, 3])
def test_gray_scan(jpegamd, dev, channels):
    rng = np.random.default_rng(77 + channels)
    rw, rh = rm.reduced_size(ODD_W, ODD_H, ODD_F)
    enc = jpegamd.Encoder(rw, rows_for(2, rh))
    pics = random_pics(rng, 2, ODD_W, ODD_H, channels)
    stored = [Stored(p, "wide" if channels == 1 else "rgba", dev, rng) for p in pics]
    imgs = [s.image(jpegamd, ODD_W, ODD_H) for s in stored]
    for ri in (0, 3, -(-rw // 8)):
        check_files(jpegamd, enc, dev, imgs, pics, "one", 0, ODD_F, ri=ri)
    enc.set_huffman(jpegamd.HUFFMAN_OPTIMIZED)
    try:
        for ri in (3, 0):
            check_files(jpegamd, enc, dev, imgs, pics, "one", 0, ODD_F, ri=ri)
    finally:
        enc.set_huffman(jpegamd.HUFFMAN_STANDARD)


def test_progressive(jpegamd, dev):
    import jpegamd.progressive_script as ps
    rng = np.random.default_rng(606)
    rw, rh = rm.reduced_size(ODD_W, ODD_H, ODD_F)
    enc = jpegamd.Encoder(rw, rows_for(2, rh))
    split = ps.parse_scan_script((SCANS_DIR / "split.txt").read_text())
    jpegamd.validate_scan_script(split, 3)
    pics = random_pics(rng, 2, ODD_W, ODD_H, 3)
    stored = [Stored(p, "packed3", dev, rng) for p in pics]
    imgs = [s.image(jpegamd, ODD_W, ODD_H) for s in stored]
    for scans in (None, split):
        check_files(jpegamd, enc, dev, imgs, pics, "prog", S420, ODD_F, scans=scans)
    for scans in (None, pfx.GRAY_SPLIT):
        check_files(jpegamd, enc, dev, imgs, pics, "prog", 0, ODD_F, scans=scans)
    one = random_pics(rng, 1, ODD_W, ODD_H, 1)
    s1 = Stored(one[0], "shifted", dev, rng)
    check_files(jpegamd, enc, dev, [s1.image(jpegamd, ODD_W, ODD_H)], one, "prog", 0, ODD_F, scans=pfx.GRAY_SPLIT)


def test_quant_tables_and_metadata_carry_over(jpegamd, dev):
    rng = np.random.default_rng(707)
    rw, rh = rm.reduced_size(ODD_W, ODD_H, ODD_F)
    enc = jpegamd.Encoder(rw, rows_for(2, rh))
    luma = np.clip(np.arange(64) * 2 + 3, 1, 255).astype(np.uint8)
    chroma = np.clip(200 - np.arange(64) * 3, 1, 255).astype(np.uint8)
    enc.set_quant_tables(luma, chroma)
    enc.set_metadata(comment="reduced source", icc_profile=meta.icc_like(70000))
    extra = enc.metadata_bytes()
    assert extra > 70000
    pics = random_pics(rng, 2, ODD_W, ODD_H, 3)
    small = [rm.reduce_picture(p, ODD_F) for p in pics]
    stored = [Stored(p, "planar", dev, rng) for p in pics]
    imgs = [s.image(jpegamd, ODD_W, ODD_H) for s in stored]
    plain = None
    for route, sub in (("three", S420), ("one", S422), ("prog", S444), ("three", 0)):
        a = queue_reduced(jpegamd, enc, imgs, dev, route, sub, ODD_F, extra=extra)
        enc.finish()
        b, keep = queue_bytes(jpegamd, enc, small, dev, route, sub, extra=extra)
        enc.finish()
        got = intact_files(a)
        assert got == intact_files(b), (route, sub)
        assert all(b"reduced source" in f[:200000] and len(f) > extra for f in got)
        if route == "three" and sub == S420:
            plain = got
    enc.set_quant_tables(None)
    enc.set_metadata(None)
    back = check_files(jpegamd, enc, dev, imgs, pics, "three", S420, ODD_F)
    assert back != plain


# ---- 5. Python ------------------------------------------------------------------------------------------------------------------------
def model_tensor(t, f):
    """[N, 3, H, W] device bytes -> the model's reduced bytes, [N, 3, oh, ow] on the same device."""
    host = t.cpu().numpy()
    small = np.stack([rm.reduce_picture(p.transpose(1, 2, 0), f).transpose(2, 0, 1) for p in host])
    return torch.from_numpy(np.ascontiguousarray(small)).to(t.device)


@pytest.mark.parametrize("f", [1, 2, 3, 8])
def test_python_matches_the_uint8_route(jpegamd, dev, f):
    g = torch.Generator().manual_seed(11 + f)
    t = torch.randint(0, 256, (3, 3, 45, 67), generator=g, dtype=torch.uint8).to(dev)
    q8 = model_tensor(t, f)
    assert tuple(q8.shape[2:]) == jpegamd.reduced_size(67, 45, f)[::-1]
    for sub in (S420, S444):
        assert jpegamd.encode_reduced_batch(t, subsampling=sub, factor=f) == jpegamd.encode_tensor_batch(q8, subsampling=sub, layout="chw")
    assert jpegamd.encode_reduced(t[1], factor=f) == jpegamd.encode_tensor(q8[1], layout="chw")
    hwc = t.permute(0, 2, 3, 1).contiguous()
    assert jpegamd.encode_reduced_batch(hwc, factor=f, layout="hwc") == jpegamd.encode_tensor_batch(q8, layout="chw")
    rgba = torch.cat([hwc, torch.randint(0, 256, (3, 45, 67, 1), generator=g, dtype=torch.uint8).to(dev)], dim=3)
    assert jpegamd.encode_reduced_batch(rgba, factor=f, layout="rgba") == jpegamd.encode_tensor_batch(q8, layout="chw")
    bgra = torch.cat([hwc.flip(3), rgba[..., 3:]], dim=3)
    assert jpegamd.encode_reduced_batch(bgra, factor=f, layout="bgra") == jpegamd.encode_tensor_batch(q8, layout="chw")
    assert jpegamd.encode_reduced_batch(t[:, 0], factor=f, layout="gray") == jpegamd.encode_tensor_batch(q8[:, 0].contiguous())
    assert jpegamd.encode_reduced_batch(t, subsampling=0, factor=f) == jpegamd.encode_tensor_batch(q8, subsampling=0, layout="chw")
    assert jpegamd.encode_reduced_batch([t[:, 0], t[:, 1], t[:, 2]], factor=f) == jpegamd.encode_tensor_batch(q8, layout="chw")


def test_views_go_through_without_a_copy(jpegamd, dev, monkeypatch):
    g = torch.Generator().manual_seed(13)
    t = torch.randint(0, 256, (4, 3, 24, 40), generator=g, dtype=torch.uint8).to(dev)
    cl = t.contiguous(memory_format=torch.channels_last)
    crop = t[:, :, 2:21, 3:38]
    seen = []
    real = jpegamd.Encoder.encode_reduced_batch_async

    def spy(self, imgs, *a, **kw):
        seen.append([(tuple(i.plane), i.width, i.height, i.row_stride, i.pixel_stride) for i in imgs])
        return real(self, imgs, *a, **kw)

    monkeypatch.setattr(jpegamd.Encoder, "encode_reduced_batch_async", spy)
    want = jpegamd.encode_tensor_batch(model_tensor(t, 2), layout="chw")
    assert jpegamd.encode_reduced_batch(cl, factor=2) == want
    assert seen[-1] == [(tuple(cl[i].data_ptr() + k for k in range(3)), 40, 24, 3 * 40, 3) for i in range(4)]
    want_crop = jpegamd.encode_tensor_batch(model_tensor(crop.contiguous(), 2), layout="chw")
    assert jpegamd.encode_reduced_batch(crop, factor=2) == want_crop
    assert seen[-1] == [(tuple(crop[i, k].data_ptr() for k in range(3)), 35, 19, 40, 1) for i in range(4)]
    assert jpegamd.encode_reduced_batch(cl[:, :, 2:21, 3:38], factor=2) == want_crop
    assert seen[-1][0][0][0] == cl.data_ptr() + 3 * (2 * 40 + 3)
    # every second picture; factor 1: the strided tensor itself
    assert jpegamd.encode_reduced_batch(t[::2], factor=2) == want[::2]
    assert [s[0][0] for s in seen[-1]] == [t[0].data_ptr(), t[2].data_ptr()]
    assert jpegamd.encode_reduced_batch(crop[1::2], factor=1) == jpegamd.encode_tensor_batch(crop[1::2].contiguous(), layout="chw")


def test_python_twins(jpegamd, dev):
    import jpegamd.mjpeg as mj
    import jpegamd.progressive_script as ps
    g = torch.Generator().manual_seed(17)
    f = 3
    t = torch.randint(0, 256, (2, 3, ODD_H, ODD_W), generator=g, dtype=torch.uint8).to(dev)
    q8 = model_tensor(t, f)
    assert mj.encode_reduced_batch(t, factor=f, restart_interval="row", huffman="optimized") == \
        mj.encode_tensor_batch(q8, layout="chw", restart_interval="row", huffman="optimized")
    assert mj.encode_reduced(t[0], subsampling=S444, factor=f) == mj.encode_tensor(q8[0], subsampling=S444, layout="chw")
    assert mj.encode_reduced_batch(t[:, 1], factor=f, layout="gray", restart_interval=2) == mj.encode_gray_batch(q8[:, 1].contiguous(), restart_interval=2)
    hwc8 = q8.permute(0, 2, 3, 1).contiguous()
    assert ps.encode_reduced_batch(t, factor=f, scans=pfx.SPLIT) == ps.encode_tensor_batch(hwc8, scans=pfx.SPLIT)
    assert ps.encode_reduced(t[1], factor=f) == ps.encode_tensor(hwc8[1])
    assert ps.encode_reduced_batch(t[:, 2], factor=f, layout="gray") == ps.encode_gray_batch(q8[:, 2].contiguous())
    with jpegamd.quant_tables(np.full(64, 9, np.uint8)), jpegamd.metadata(comment="twin"):
        assert jpegamd.encode_reduced_batch(t, factor=f) == jpegamd.encode_tensor_batch(q8, layout="chw")
