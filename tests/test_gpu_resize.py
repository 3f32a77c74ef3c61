"""Resized pictures (jpegamd_encode_resized_batch_async and its twins) through the C-ABI into the HIP kernels.  Two exact comparisons
throughout: the planes k_resize_planes_batch leaves in scratch (jpegamd_debug_resized_planes), sample for sample against
tests/resize_model.py; and the files, byte for byte against the existing uint8 entry run on the model's resized bytes.  Every source is
surrounded by random filler bytes (rows longer than the picture, lead-in bytes, the bytes between strided samples, RGBA's fourth byte):
a read outside the picture that gets USED changes the result.  Every test needs an MI355X.

Section 1 runs the whole cross product walk x target x geometry; the plan is asserted below."""
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
import resize_model as rz
from gpu_support import GRAY, S420, S422, S444, Outputs, dev, intact_files, rows_for     # noqa: F401
from gpu_support import stream as current_stream

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

# planes; packed R G B; packed B G R; RGBA at stride 4; a strided column walk (every second byte of three planes); one channel
WALKS = ("planar", "packed3", "bgr", "rgba", "column", "one")
CONTIGUOUS = ("planar", "packed3", "bgr", "rgba", "one")
# what is encoded: a colour subsampling, the luma of three channels, or a single channel
TARGETS = (S444, S420, S422, "luma", "single")
# (W, H, ow, oh)
GEOMETRIES = [(37, 29, 13, 11), (33, 31, 32, 30), (40, 9, 5, 9), (23, 17, 23, 17), (24, 16, 12, 8), (24, 16, 6, 4), (24, 16, 3, 2),
              (128, 64, 2, 1), (130, 67, 3, 2), (5, 3, 1, 1), (1, 1, 1, 1)]
WHOLE = {(24, 16, 12, 8): 2, (24, 16, 6, 4): 4, (24, 16, 3, 2): 8}                  # also the reduced pass's planes at this factor
SCANS_DIR = Path(__file__).resolve().parents[1] / "tools" / "scans"


def plan():
    """walk -> [(target, geometry, lead)]: one channel goes with the single-channel target alone, every other walk with the four
    targets of three channels; every geometry each time; the pointer's offset from a dword boundary in rotation."""
    out = {}
    for walk in WALKS:
        targets = ("single",) if walk == "one" else TARGETS[:4]
        out[walk] = [(t, g, (3 * k + i) % 4) for i, t in enumerate(targets) for k, g in enumerate(GEOMETRIES)]
    return out


PLAN = plan()
assert all(rz.check(*g) for g in GEOMETRIES) and len(GEOMETRIES) == 11
assert sum(len(v) for v in PLAN.values()) == 5 * 4 * 11 + 11
assert {(w, t, g) for w, v in PLAN.items() for t, g, _ in v} == \
    {(w, t, g) for w, t, g in itertools.product(WALKS, TARGETS, GEOMETRIES) if (w == "one") == (t == "single")}
for _walk in CONTIGUOUS:
    assert {lead for _, _, lead in PLAN[_walk]} == {0, 1, 2, 3}, _walk
    for _g in ((37, 29, 13, 11), (33, 31, 32, 30)):
        assert len({lead for _, g, lead in PLAN[_walk] if g == _g}) == (1 if _walk == "one" else 4)
assert any(g[0] == 64 * g[2] and g[1] == 64 * g[3] for g in GEOMETRIES)             # a ratio of exactly 64 both ways


# ---- sources ------------------------------------------------------------------------------------------------------------------------
class Stored:
    """One picture's bytes ([H, W, C], C = 3 or 1) on the device as `walk` says, `lead` bytes into a fresh allocation, random filler
    around them -> .ptrs (R, G, B), .row, .pixel in bytes."""

    def __init__(self, pic, walk, dev, rng, lead=0):
        h, w, c = pic.shape
        if walk in ("planar", "column", "one"):
            step = 2 if walk == "column" else 1
            row = step * w + 5
            buf = rng.integers(0, 256, (lead + c * h * row,), np.uint8)
            view = buf[lead:].reshape(c, h, row)
            view[:, :, 0:step * w:step] = pic.transpose(2, 0, 1)
            self.t = torch.from_numpy(buf).to(dev)
            base = self.t.data_ptr() + lead
            self.ptrs = tuple(base + k * h * row for k in range(c))
            self.row, self.pixel = row, step
        else:
            group = 4 if walk == "rgba" else 3
            row = group * w + 7
            order = (2, 1, 0) if walk == "bgr" else (0, 1, 2)
            buf = rng.integers(0, 256, (lead + h * row,), np.uint8)
            view = buf[lead:].reshape(h, row)
            for k in range(c):
                view[:, order[k]:group * w:group] = pic[:, :, k]
            self.t = torch.from_numpy(buf).to(dev)
            self.ptrs = tuple(self.t.data_ptr() + lead + order[k] for k in range(c))
            self.row, self.pixel = row, group
        assert self.t.data_ptr() % 16 == 0

    def image(self, jpegamd, w, h, q=0):
        return jpegamd.Encoder.strided_image(self.ptrs, w, h, self.row, self.pixel, q)


def random_pics(rng, n, w, h, c):
    return [rng.integers(0, 256, (h, w, c), np.uint8) for _ in range(n)]


def plane_shapes(w, h, sub):
    cw, ch = (w if sub == S444 else (w + 1) // 2), ((h + 1) // 2 if sub == S420 else h)
    return [(h, w)] + ([(ch, cw), (ch, cw)] if sub else [])


def resized_planes(jpegamd, enc, imgs, sub, ow, oh, dev, reduce=0):
    """jpegamd_debug_resized_planes (reduce: jpegamd_debug_reduced_planes at that factor) -> [(y, cb, cr)] or [(y,)] picture by
    picture, as numpy."""
    n = len(imgs)
    bufs = [torch.full((n, hh, ww), 0xA5, dtype=torch.uint8, device=dev) for hh, ww in plane_shapes(ow, oh, sub)]
    ptrs = [C.c_void_p(b.data_ptr()) for b in bufs] + [None] * (3 - len(bufs))
    arr = (jpegamd.StridedImage * n)(*imgs)
    if reduce:
        rc = jpegamd.lib.jpegamd_debug_reduced_planes(enc._h, arr, n, int(sub), reduce, *ptrs, C.c_void_p(current_stream()))
    else:
        rc = jpegamd.lib.jpegamd_debug_resized_planes(enc._h, arr, n, int(sub), ow, oh, *ptrs, C.c_void_p(current_stream()))
    assert rc == 0, rc
    host = [b.cpu().numpy() for b in bufs]
    return [tuple(p[i] for p in host) for i in range(n)]


def same_planes(got, want):
    return len(got) == len(want) and all(len(g) == len(w) and all(np.array_equal(a, b) for a, b in zip(g, w)) for g, w in zip(got, want))


def model_planes(pics, sub, ow, oh):
    small = [rz.resize_picture(p, ow, oh) for p in pics]
    return [fm.planes(p, sub) if p.shape[2] == 3 else (p[:, :, 0],) for p in small]


def check_planes(jpegamd, enc, dev, imgs, pics, sub, ow, oh):
    got = resized_planes(jpegamd, enc, imgs, sub, ow, oh, dev)
    assert same_planes(got, model_planes(pics, sub, ow, oh)), ("planes", sub, pics[0].shape, ow, oh)
    return got


# ---- the two routes: a resized call, and the uint8 call of the model's resized bytes -------------------------------------------------
def capacity(jpegamd, route, w, h, sub, ri, scans):
    if route == "prog":
        return jpegamd.max_jfif_bytes_progressive_script(w, h, sub, scans)
    if route == "one":
        return jpegamd.max_jfif_bytes_gray_scan(w, h, ri) if sub == 0 else jpegamd.max_jfif_bytes_interleaved_restart(w, h, sub, ri)
    return jpegamd.max_jfif_bytes(w, h) if sub == 0 else jpegamd.max_jfif_bytes_color(w, h, sub)


def queue_resized(jpegamd, enc, imgs, dev, route, sub, ow, oh, ri=0, scans=None, extra=0, cap=None):
    out = Outputs(dev, len(imgs), cap if cap is not None else capacity(jpegamd, route, ow, oh, sub, ri, scans) + extra)
    if route == "prog":
        enc.encode_resized_progressive_script_batch_async(imgs, sub, ow, oh, scans, out.out_ptrs, out.cap, out.size_ptrs, current_stream())
    elif route == "one":
        enc.encode_resized_interleaved_batch_async(imgs, sub, ow, oh, ri, out.out_ptrs, out.cap, out.size_ptrs, current_stream())
    else:
        enc.encode_resized_batch_async(imgs, sub, ow, oh, out.out_ptrs, out.cap, out.size_ptrs, current_stream())
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


def check_files(jpegamd, enc, dev, imgs, pics, route, sub, ow, oh, q=0, ri=0, scans=None, small=None):
    """One resized call, finished; the uint8 call of the model's resized bytes, finished; equal byte for byte."""
    a = queue_resized(jpegamd, enc, imgs, dev, route, sub, ow, oh, ri, scans)
    st = enc.finish()
    got = intact_files(a)
    assert st.jfif_bytes == len(got[-1])
    small = small if small is not None else [rz.resize_picture(p, ow, oh) for p in pics]
    b, keep = queue_bytes(jpegamd, enc, small, dev, route, sub, q, ri, scans)
    enc.finish()
    ref = intact_files(b)
    del keep
    assert all(len(x) > 100 and x[:2] == b"\xff\xd8" and x[-2:] == b"\xff\xd9" for x in ref)
    assert got == ref, ("resized entry vs uint8 entry", route, sub, q, ri, pics[0].shape, ow, oh)
    return got


def target_of(target):
    """-> (channels, subsampling of the call)."""
    return (1, 0) if target == "single" else ((3, 0) if target == "luma" else (3, target))


# ---- 1. walks x targets x geometries: the planes of the pass alone ---------------------------------------------------------------------
@pytest.mark.parametrize("walk", WALKS)
def test_planes_of_every_walk_target_and_geometry(jpegamd, dev, walk):
    rng = np.random.default_rng(100 * WALKS.index(walk) + 7)
    enc = jpegamd.Encoder(32, rows_for(2, 30))
    ran = 0
    for target, (w, h, ow, oh), lead in PLAN[walk]:
        channels, sub = target_of(target)
        pics = random_pics(rng, 2, w, h, channels)
        stored = [Stored(p, walk, dev, rng, lead) for p in pics]
        assert all(s.ptrs[0] % 4 == (lead + (2 if walk == "bgr" else 0)) % 4 for s in stored)
        imgs = [s.image(jpegamd, w, h) for s in stored]
        got = check_planes(jpegamd, enc, dev, imgs, pics, sub, ow, oh)
        if (w, h, ow, oh) in WHOLE:
            assert same_planes(got, resized_planes(jpegamd, enc, imgs, sub, ow, oh, dev, reduce=WHOLE[(w, h, ow, oh)]))
        if (w, h) == (ow, oh) and channels == 1:
            assert np.array_equal(got[0][0], pics[0][:, :, 0])     # the identity
        ran += 1
    assert ran == (11 if walk == "one" else 44)


# ---- 2. sizes that cross what 32 bits and one workgroup hold ----------------------------------------------------------------------------
@pytest.mark.parametrize("side,out", [(4100, 65), (4200, 66)])
def test_sums_past_32_bits(jpegamd, dev, side, out):
    """One channel, all 254 with planted 0s and 255s: S is 254 W H less a little -- 0.6% short of 2^32 at 4100 x 4100, past it at
    4200 x 4200 -- and S times anything is past it at both; a 32-bit sum, product or division shows as a wrong byte."""
    rng = np.random.default_rng(side)
    pic = np.full((side, side, 1), 254, np.uint8)
    ys, xs = rng.integers(0, side, 4000), rng.integers(0, side, 4000)
    pic[ys[:2000], xs[:2000], 0] = 0
    pic[ys[2000:], xs[2000:], 0] = 255
    pic[:70, :140, 0] = 255                                        # whole footprints of 255 and of 0
    pic[-70:, -140:, 0] = 0
    want = rz.resize_plane(pic[:, :, 0], out, out)
    assert want[0, 0] == 255 and want[-1, -1] == 0 and len(np.unique(want)) > 3
    t = torch.from_numpy(pic[:, :, 0].copy()).to(dev)
    enc = jpegamd.Encoder(out, rows_for(1, out))
    img = jpegamd.Encoder.strided_image((t.data_ptr(),), side, side, side, 1, 0)
    got = resized_planes(jpegamd, enc, [img], 0, out, out, dev)
    assert np.array_equal(got[0][0], want)
    check_files(jpegamd, enc, dev, [img], [pic], "three", 0, out, out, small=[want[:, :, None]])


@pytest.mark.parametrize("walk,sub,channels", [("planar", S420, 3), ("packed3", S444, 3), ("rgba", S422, 3), ("one", 0, 1)])
def test_a_second_workgroup_in_x(jpegamd, dev, walk, sub, channels):
    w, h, ow, oh = 16385, 9, 2049, 2
    rng = np.random.default_rng(5 + channels + sub)
    pics = random_pics(rng, 1, w, h, channels)
    s = Stored(pics[0], walk, dev, rng, 1)
    enc = jpegamd.Encoder(ow, rows_for(1, oh))
    check_planes(jpegamd, enc, dev, [s.image(jpegamd, w, h)], pics, sub, ow, oh)
    check_files(jpegamd, enc, dev, [s.image(jpegamd, w, h)], pics, "three", sub, ow, oh)


@pytest.mark.parametrize("walk,sub,channels", [("one", 0, 1), ("bgr", S420, 3)])
def test_the_widest_source(jpegamd, dev, walk, sub, channels):
    w, h, ow, oh = 65535, 2, 1024, 1                               # (a few hundred KB: memory allows)
    rng = np.random.default_rng(65535 + channels)
    pics = random_pics(rng, 1, w, h, channels)
    s = Stored(pics[0], walk, dev, rng, 3)
    enc = jpegamd.Encoder(ow, rows_for(1, oh))
    check_planes(jpegamd, enc, dev, [s.image(jpegamd, w, h)], pics, sub, ow, oh)


# ---- 3. files ---------------------------------------------------------------------------------------------------------------------------
FW, FH, FOW, FOH = 151, 113, 97, 92


def file_sources(jpegamd, dev, rng, walk, channels=3, n=2):
    pics = random_pics(rng, n, FW, FH, channels)
    stored = [Stored(p, walk, dev, rng, 1) for p in pics]
    return pics, stored, [s.image(jpegamd, FW, FH) for s in stored], [rz.resize_picture(p, FOW, FOH) for p in pics]


def test_three_scans_and_the_grayscale_file(jpegamd, dev):
    rng = np.random.default_rng(31)
    enc = jpegamd.Encoder(FOW, rows_for(2, FOH))
    for walk, sub in (("planar", S444), ("packed3", S420), ("rgba", S422), ("bgr", 0)):
        pics, stored, imgs, small = file_sources(jpegamd, dev, rng, walk)
        check_planes(jpegamd, enc, dev, imgs, pics, sub, FOW, FOH)
        check_files(jpegamd, enc, dev, imgs, pics, "three", sub, FOW, FOH, small=small)
    pics, stored, imgs, small = file_sources(jpegamd, dev, rng, "column", channels=1)
    check_files(jpegamd, enc, dev, imgs, pics, "three", 0, FOW, FOH, small=small)


@pytest.mark.parametrize("sub", [S420, S444])
def test_one_scan(jpegamd, dev, sub):
    rng = np.random.default_rng(1000 + sub)
    enc = jpegamd.Encoder(FOW, rows_for(2, FOH))
    pics, stored, imgs, small = file_sources(jpegamd, dev, rng, "packed3" if sub == S420 else "planar")
    row = msup.row_interval(FOW, sub)
    for ri in (0, 1, row):
        check_files(jpegamd, enc, dev, imgs, pics, "one", sub, FOW, FOH, ri=ri, small=small)
    enc.set_huffman(jpegamd.HUFFMAN_OPTIMIZED)
    try:
        for ri in (0, 1, row):
            check_files(jpegamd, enc, dev, imgs, pics, "one", sub, FOW, FOH, ri=ri, small=small)
    finally:
        enc.set_huffman(jpegamd.HUFFMAN_STANDARD)


@pytest.mark.parametrize("channels", [1, 3])
def test_gray_scan(jpegamd, dev, channels):
    rng = np.random.default_rng(77 + channels)
    enc = jpegamd.Encoder(FOW, rows_for(2, FOH))
    pics, stored, imgs, small = file_sources(jpegamd, dev, rng, "one" if channels == 1 else "rgba", channels=channels)
    for ri in (0, 3, -(-FOW // 8)):
        check_files(jpegamd, enc, dev, imgs, pics, "one", 0, FOW, FOH, ri=ri, small=small)
    enc.set_huffman(jpegamd.HUFFMAN_OPTIMIZED)
    try:
        for ri in (3, 0):
            check_files(jpegamd, enc, dev, imgs, pics, "one", 0, FOW, FOH, ri=ri, small=small)
    finally:
        enc.set_huffman(jpegamd.HUFFMAN_STANDARD)


def test_progressive(jpegamd, dev):
    import jpegamd.progressive_script as ps
    rng = np.random.default_rng(606)
    enc = jpegamd.Encoder(FOW, rows_for(2, FOH))
    split = ps.parse_scan_script((SCANS_DIR / "split.txt").read_text())
    jpegamd.validate_scan_script(split, 3)
    pics, stored, imgs, small = file_sources(jpegamd, dev, rng, "packed3")
    for scans in (None, split):
        check_files(jpegamd, enc, dev, imgs, pics, "prog", S420, FOW, FOH, scans=scans, small=small)
    for scans in (None, pfx.GRAY_SPLIT):
        check_files(jpegamd, enc, dev, imgs, pics, "prog", 0, FOW, FOH, scans=scans, small=small)
    pics, stored, imgs, small = file_sources(jpegamd, dev, rng, "one", channels=1, n=1)
    check_files(jpegamd, enc, dev, imgs, pics, "prog", 0, FOW, FOH, scans=pfx.GRAY_SPLIT, small=small)


def test_quant_tables_and_metadata_carry_over(jpegamd, dev):
    rng = np.random.default_rng(707)
    enc = jpegamd.Encoder(FOW, rows_for(2, FOH))
    luma = np.clip(np.arange(64) * 2 + 3, 1, 255).astype(np.uint8)
    chroma = np.clip(200 - np.arange(64) * 3, 1, 255).astype(np.uint8)
    enc.set_quant_tables(luma, chroma)
    enc.set_metadata(comment="resized source", icc_profile=meta.icc_like(70000))
    extra = enc.metadata_bytes()
    assert extra > 70000
    pics, stored, imgs, small = file_sources(jpegamd, dev, rng, "planar")
    plain = None
    for route, sub in (("three", S420), ("one", S422), ("prog", S444), ("three", 0)):
        a = queue_resized(jpegamd, enc, imgs, dev, route, sub, FOW, FOH, extra=extra)
        enc.finish()
        b, keep = queue_bytes(jpegamd, enc, small, dev, route, sub, extra=extra)
        enc.finish()
        got = intact_files(a)
        assert got == intact_files(b), (route, sub)
        assert all(b"resized source" in f[:200000] and len(f) > extra for f in got)
        if route == "three" and sub == S420:
            plain = got
    enc.set_quant_tables(None)
    enc.set_metadata(None)
    back = check_files(jpegamd, enc, dev, imgs, pics, "three", S420, FOW, FOH, small=small)
    assert back != plain


# ---- 4. batches and scratch ---------------------------------------------------------------------------------------------------------------
def test_batches_of_32_and_of_one(jpegamd, dev):
    rng = np.random.default_rng(64)
    w, h, ow, oh = 31, 33, 19, 14
    enc = jpegamd.Encoder(ow, rows_for(32, oh))
    pics = random_pics(rng, 32, w, h, 3)
    stored = [Stored(p, "packed3", dev, rng, i % 4) for i, p in enumerate(pics)]
    imgs = [s.image(jpegamd, w, h) for s in stored]
    small = [rz.resize_picture(p, ow, oh) for p in pics]
    files = check_files(jpegamd, enc, dev, imgs, pics, "three", S420, ow, oh, small=small)
    assert len(set(files)) == 32
    check_planes(jpegamd, enc, dev, imgs, pics, S420, ow, oh)
    assert check_files(jpegamd, enc, dev, imgs[5:6], pics[5:6], "three", S420, ow, oh, small=small[5:6]) == files[5:6]
    assert check_files(jpegamd, enc, dev, imgs, pics, "one", S444, ow, oh, small=small)


def test_scratch_growth_and_other_calls_on_one_stream(jpegamd, dev):
    """A small resized call, a larger one, the uint8 call of the larger one's bytes, a reduced call and a resized gray scan, queued
    back to back on one stream and finished once."""
    import reduce_model as rdm
    rng = np.random.default_rng(12)
    enc = jpegamd.Encoder(48, rows_for(3, 40))
    little = random_pics(rng, 2, 31, 29, 3)                        # -> 16 x 15
    large = random_pics(rng, 3, 143, 119, 3)                       # -> 48 x 40; reduced by 3: 48 x 40 too
    s_little = [Stored(p, "planar", dev, rng) for p in little]
    s_large = [Stored(p, "packed3", dev, rng, 2) for p in large]
    r_little = [rz.resize_picture(p, 16, 15) for p in little]
    r_large = [rz.resize_picture(p, 48, 40) for p in large]
    i_little = [s.image(jpegamd, 31, 29) for s in s_little]
    i_large = [s.image(jpegamd, 143, 119) for s in s_large]
    a = queue_resized(jpegamd, enc, i_little, dev, "three", S420, 16, 15)
    b = queue_resized(jpegamd, enc, i_large, dev, "three", S420, 48, 40)
    c, keep = queue_bytes(jpegamd, enc, r_large, dev, "three", S420)
    red = Outputs(dev, 3, jpegamd.max_jfif_bytes_color(48, 40, S420))
    enc.encode_reduced_batch_async(i_large, S420, 3, red.out_ptrs, red.cap, red.size_ptrs, current_stream())
    d = queue_resized(jpegamd, enc, i_large, dev, "one", 0, 48, 40)
    enc.finish()
    got_a, got_b, got_c, got_red, got_d = (intact_files(x) for x in (a, b, c, red, d))
    # the references, each in a call of its own
    ra, keep_a = queue_bytes(jpegamd, enc, r_little, dev, "three", S420)
    enc.finish()
    rd, keep_d = queue_bytes(jpegamd, enc, r_large, dev, "three", 0)
    enc.finish()
    rr, keep_r = queue_bytes(jpegamd, enc, [rdm.reduce_picture(p, 3) for p in large], dev, "three", S420)
    enc.finish()
    assert got_a == intact_files(ra)
    assert got_b == got_c and len(set(got_b)) == 3
    assert got_red == intact_files(rr)
    assert got_d == intact_files(rd)                               # (the plain grayscale file is the fused entry's)


def test_capacity_one_byte_short(jpegamd, dev):
    rng = np.random.default_rng(8)
    enc = jpegamd.Encoder(FOW, rows_for(1, FOH))
    pics, stored, imgs, small = file_sources(jpegamd, dev, rng, "planar", n=1)
    for route, sub in (("three", S420), ("one", S444), ("prog", S420), ("three", 0)):
        full = check_files(jpegamd, enc, dev, imgs, pics, route, sub, FOW, FOH, small=small)[0]
        short = queue_resized(jpegamd, enc, imgs, dev, route, sub, FOW, FOH, cap=len(full) - 1)
        with pytest.raises(jpegamd.JpegAmdError) as err:
            enc.finish()
        assert err.value.code == -8, (route, sub)
        assert all(ok for _, ok in short.results())               # nothing was written past the buffer
        assert check_files(jpegamd, enc, dev, imgs, pics, route, sub, FOW, FOH, small=small)[0] == full


# ---- 5. Python ------------------------------------------------------------------------------------------------------------------------
def model_tensor(t, ow, oh):
    """[N, 3, H, W] device bytes -> the model's resized bytes, [N, 3, oh, ow] on the same device."""
    host = t.cpu().numpy()
    small = np.stack([rz.resize_picture(p.transpose(1, 2, 0), ow, oh).transpose(2, 0, 1) for p in host])
    return torch.from_numpy(np.ascontiguousarray(small)).to(t.device)


@pytest.mark.parametrize("size", [(67, 45), (40, 30), (13, 7), (2, 2)])
def test_python_matches_the_uint8_route(jpegamd, dev, size):
    g = torch.Generator().manual_seed(11 + size[0])
    t = torch.randint(0, 256, (3, 3, 45, 67), generator=g, dtype=torch.uint8).to(dev)
    q8 = model_tensor(t, *size)
    assert tuple(q8.shape[2:]) == size[::-1]
    for sub in (S420, S444):
        assert jpegamd.encode_resized_batch(t, subsampling=sub, size=size) == jpegamd.encode_tensor_batch(q8, subsampling=sub, layout="chw")
    assert jpegamd.encode_resized(t[1], size=size) == jpegamd.encode_tensor(q8[1], layout="chw")
    hwc = t.permute(0, 2, 3, 1).contiguous()
    assert jpegamd.encode_resized_batch(hwc, size=size, layout="hwc") == jpegamd.encode_tensor_batch(q8, layout="chw")
    rgba = torch.cat([hwc, torch.randint(0, 256, (3, 45, 67, 1), generator=g, dtype=torch.uint8).to(dev)], dim=3)
    assert jpegamd.encode_resized_batch(rgba, size=size, layout="rgba") == jpegamd.encode_tensor_batch(q8, layout="chw")
    bgra = torch.cat([hwc.flip(3), rgba[..., 3:]], dim=3)
    assert jpegamd.encode_resized_batch(bgra, size=size, layout="bgra") == jpegamd.encode_tensor_batch(q8, layout="chw")
    assert jpegamd.encode_resized_batch(t[:, 0], size=size, layout="gray") == jpegamd.encode_tensor_batch(q8[:, 0].contiguous())
    assert jpegamd.encode_resized_batch(t, subsampling=0, size=size) == jpegamd.encode_tensor_batch(q8, subsampling=0, layout="chw")
    assert jpegamd.encode_resized_batch([t[:, 0], t[:, 1], t[:, 2]], size=size) == jpegamd.encode_tensor_batch(q8, layout="chw")
    assert jpegamd.encode_resized_batch(t, size=list(jpegamd.fit_size(67, 45, *size))) == \
        jpegamd.encode_tensor_batch(model_tensor(t, *jpegamd.fit_size(67, 45, *size)), layout="chw")


def test_views_go_through_without_a_copy(jpegamd, dev, monkeypatch):
    g = torch.Generator().manual_seed(13)
    t = torch.randint(0, 256, (4, 3, 24, 40), generator=g, dtype=torch.uint8).to(dev)
    cl = t.contiguous(memory_format=torch.channels_last)
    crop = t[:, :, 2:21, 3:38]
    seen = []
    real = jpegamd.Encoder.encode_resized_batch_async

    def spy(self, imgs, sub, ow, oh, *a, **kw):
        seen.append(([(tuple(i.plane), i.width, i.height, i.row_stride, i.pixel_stride) for i in imgs], (ow, oh)))
        return real(self, imgs, sub, ow, oh, *a, **kw)

    monkeypatch.setattr(jpegamd._ResizedEntries, "encode_resized_batch_async", spy)
    want = jpegamd.encode_tensor_batch(model_tensor(t, 25, 11), layout="chw")
    assert jpegamd.encode_resized_batch(cl, size=(25, 11)) == want
    assert seen[-1] == ([(tuple(cl[i].data_ptr() + k for k in range(3)), 40, 24, 3 * 40, 3) for i in range(4)], (25, 11))
    want_crop = jpegamd.encode_tensor_batch(model_tensor(crop.contiguous(), 20, 19), layout="chw")
    assert jpegamd.encode_resized_batch(crop, size=(20, 19)) == want_crop
    assert seen[-1] == ([(tuple(crop[i, k].data_ptr() for k in range(3)), 35, 19, 40, 1) for i in range(4)], (20, 19))
    assert jpegamd.encode_resized_batch(cl[:, :, 2:21, 3:38], size=(20, 19)) == want_crop
    assert seen[-1][0][0][0][0] == cl.data_ptr() + 3 * (2 * 40 + 3)
    # every second picture; the identity: the strided tensor itself
    assert jpegamd.encode_resized_batch(t[::2], size=(25, 11)) == want[::2]
    assert [s[0][0] for s in seen[-1][0]] == [t[0].data_ptr(), t[2].data_ptr()]
    assert jpegamd.encode_resized_batch(crop[1::2], size=(35, 19)) == jpegamd.encode_tensor_batch(crop[1::2].contiguous(), layout="chw")


def test_python_twins(jpegamd, dev):
    import jpegamd.mjpeg as mj
    import jpegamd.progressive_script as ps
    g = torch.Generator().manual_seed(17)
    size = (FOW, FOH)
    t = torch.randint(0, 256, (2, 3, FH, FW), generator=g, dtype=torch.uint8).to(dev)
    q8 = model_tensor(t, *size)
    assert mj.encode_resized_batch(t, size=size, restart_interval="row", huffman="optimized") == \
        mj.encode_tensor_batch(q8, layout="chw", restart_interval="row", huffman="optimized")
    assert mj.encode_resized(t[0], subsampling=S444, size=size) == mj.encode_tensor(q8[0], subsampling=S444, layout="chw")
    assert mj.encode_resized_batch(t[:, 1], size=size, layout="gray", restart_interval=2) == mj.encode_gray_batch(q8[:, 1].contiguous(), restart_interval=2)
    hwc8 = q8.permute(0, 2, 3, 1).contiguous()
    assert ps.encode_resized_batch(t, size=size, scans=pfx.SPLIT) == ps.encode_tensor_batch(hwc8, scans=pfx.SPLIT)
    assert ps.encode_resized(t[1], size=size) == ps.encode_tensor(hwc8[1])
    assert ps.encode_resized_batch(t[:, 2], size=size, layout="gray") == ps.encode_gray_batch(q8[:, 2].contiguous())
    with jpegamd.quant_tables(np.full(64, 9, np.uint8)), jpegamd.metadata(comment="twin"):
        assert jpegamd.encode_resized_batch(t, size=size) == jpegamd.encode_tensor_batch(q8, layout="chw")
