"""Planar (channels-first) and 4-byte-pixel pictures through the C-ABI into the HIP kernels, byte for byte.  The output of every
new layout is defined by the packed path: colour files are color_model.color_file of the same R, G, B values, grayscale files are
oracle.encode_bmp of the same picture as a BMP; the largest case is compared with the packed batch entry, which the colour suites
pin at that size.  Every test needs an MI355X."""
from __future__ import annotations

import functools
import hashlib

import numpy as np
import pytest

import color_fixtures as cf
import gpu_support
from gpu_support import GRAY, S420, S444, WIDE_STRIDE, Outputs, dev, intact_files, rows_for, stream, synth_rgb, upload     # noqa: F401
from gpu_support import model as want                           # (memoised: many layouts share one picture)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (7, 9), (203, 117), (333, 250), (520, 16), (1024, 64), (2056, 40)]
pictures = functools.partial(gpu_support.pictures, base=300, step=41)


_rng = np.random.default_rng(2024)


def px4_rows(rgb: np.ndarray, bottom_up: bool, bgra: bool) -> np.ndarray:
    """[H, 4 W]: R, G, B, x (or B, G, R, x) with a random fourth byte in every pixel."""
    s = rgb[::-1] if bottom_up else rgb
    if bgra:
        s = s[:, :, ::-1]
    x = _rng.integers(0, 256, s.shape[:2] + (1,), np.uint8)
    return np.concatenate([s, x], axis=2).reshape(s.shape[0], -1)


def cap_for(jpegamd, w, h, sub):
    return jpegamd.max_jfif_bytes(w, h) if sub == GRAY else jpegamd.max_jfif_bytes_color(w, h, sub)


def queue_px4(jpegamd, enc, rgbs, dev, sub, order, quality=0, bottom_up=False, stride=None, shifts=None, cap=None, single=False):
    """RGBA / BGRA pictures through the packed entries (single: the one-picture entries) -> (Outputs, tensors to keep alive)."""
    h, w, _ = rgbs[0].shape
    stride = stride or 4 * w
    shifts = shifts or [0] * len(rgbs)
    px = [upload(px4_rows(r, bottom_up, order == jpegamd.ORDER_BGRA), dev, stride, s) for r, s in zip(rgbs, shifts)]
    o = Outputs(dev, len(rgbs), cap if cap is not None else cap_for(jpegamd, w, h, sub))
    imgs = [jpegamd.Encoder.image(ptr, w, h, stride, bottom_up, order, quality) for _, ptr in px]
    if single:
        assert len(rgbs) == 1
        if sub == GRAY:
            enc.encode_async(imgs[0], o.out_ptrs[0], o.cap, o.size_ptrs[0], True, stream())
        else:
            enc.encode_color_async(imgs[0], sub, o.out_ptrs[0], o.cap, o.size_ptrs[0], stream())
    elif sub == GRAY:
        enc.encode_batch_async(imgs, o.out_ptrs, o.cap, o.size_ptrs, True, stream())
    else:
        enc.encode_color_batch_async(imgs, sub, o.out_ptrs, o.cap, o.size_ptrs, stream())
    return o, px


def planes_of(rgb, bottom_up):
    s = rgb[::-1] if bottom_up else rgb
    return [np.ascontiguousarray(s[:, :, k]) for k in range(3)]


def planar_sources(rgbs, dev, how, bottom_up=False, stride=None, shifts=(0, 0, 0)):
    """-> (per picture (R, G, B) pointers, row stride, tensors to keep alive).  how: "one" a contiguous [3, H, W] tensor per picture,
    "three" three separate allocations (row stride `stride`, plane k shifted by shifts[k] bytes), "crop" a view into a larger
    [3, H + 5, W + 11] tensor."""
    h, w, _ = rgbs[0].shape
    ptrs, keep = [], []
    for rgb in rgbs:
        pl = planes_of(rgb, bottom_up)
        if how == "one":
            t = torch.from_numpy(np.stack(pl)).to(dev)
            keep.append(t)
            ptrs.append(tuple(t[k].data_ptr() for k in range(3)))
            st = w
        elif how == "crop":
            big = torch.from_numpy(_rng.integers(0, 256, (3, h + 5, w + 11), np.uint8)).to(dev)
            view = big[:, 2:2 + h, 7:7 + w]
            view.copy_(torch.from_numpy(np.stack(pl)).to(dev))
            keep.append(big)
            ptrs.append(tuple(view[k].data_ptr() for k in range(3)))
            st = w + 11
        else:
            st = stride or w
            ups = [upload(p, dev, st, s) for p, s in zip(pl, shifts)]
            keep.append(ups)
            ptrs.append(tuple(p for _, p in ups))
    return ptrs, st, keep


def queue_planar(jpegamd, enc, rgbs, dev, sub, how="one", quality=0, bottom_up=False, stride=None, shifts=(0, 0, 0), cap=None):
    h, w, _ = rgbs[0].shape
    ptrs, st, keep = planar_sources(rgbs, dev, how, bottom_up, stride, shifts)
    o = Outputs(dev, len(rgbs), cap if cap is not None else cap_for(jpegamd, w, h, sub))
    imgs = [jpegamd.Encoder.planar_image(p, w, h, st, bottom_up, quality) for p in ptrs]
    enc.encode_planar_batch_async(imgs, sub, o.out_ptrs, o.cap, o.size_ptrs, stream())
    return o, keep


def finished(enc, job):
    o, keep = job
    enc.finish()
    return intact_files(o)


# ---- sizes x outputs x qualities x row orders x layouts ----------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
def test_every_layout_matches_the_packed_path(jpegamd, oracle, dev, w, h):
    rgbs = pictures(jpegamd, w, h, 3, seed=w)                   # photo-like, noise, photo-like
    rgbs[2] = synth_rgb(jpegamd, w, h, 5, 2)                    # ... and flat
    enc = jpegamd.Encoder(w, rows_for(3, h))
    for sub in (S420, S444, GRAY):
        for q in (0, 10, 90):
            exp = [want(oracle, r, q, sub) for r in rgbs]
            for bottom_up in (False, True):
                for order in (jpegamd.ORDER_RGBA, jpegamd.ORDER_BGRA):
                    got = finished(enc, queue_px4(jpegamd, enc, rgbs, dev, sub, order, q, bottom_up))
                    assert got == exp, (w, h, sub, q, bottom_up, order)
                for how in ("one", "three", "crop"):
                    got = finished(enc, queue_planar(jpegamd, enc, rgbs, dev, sub, how, q, bottom_up))
                    assert got == exp, (w, h, sub, q, bottom_up, how)
            # the one-picture entries
            for k, order in ((0, jpegamd.ORDER_RGBA), (1, jpegamd.ORDER_BGRA)):
                got = finished(enc, queue_px4(jpegamd, enc, [rgbs[k]], dev, sub, order, q, single=True))
                assert got == [exp[k]], (w, h, sub, q, order, "single")


def test_extreme_blocks_in_every_layout(jpegamd, oracle, dev):
    """(p, p, p) of the plane that pushes the transform's subnormal operand hardest: Y = p."""
    p = cf.extreme_plane(jpegamd.cos_lut())
    rgb = np.repeat(p[:, :, None], 3, axis=2)
    h, w = p.shape
    enc = jpegamd.Encoder(w, rows_for(1, h))
    for sub, q in ((GRAY, 0), (S444, 90), (S420, 10)):
        exp = [want(oracle, rgb, q, sub)]
        assert finished(enc, queue_px4(jpegamd, enc, [rgb], dev, sub, jpegamd.ORDER_BGRA, q)) == exp, (sub, q)
        assert finished(enc, queue_planar(jpegamd, enc, [rgb], dev, sub, "one", q)) == exp, (sub, q)
        assert finished(enc, queue_planar(jpegamd, enc, [rgb], dev, sub, "three", q, stride=w + 3)) == exp, (sub, q)


# ---- strides and alignment -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(203, 117), (1024, 64), (2056, 40)])
def test_row_strides(jpegamd, oracle, dev, w, h):
    rgbs = pictures(jpegamd, w, h, 2, seed=h)
    enc = jpegamd.Encoder(w, rows_for(2, h))
    for sub in (S420, S444, GRAY):
        exp = [want(oracle, r, 0, sub) for r in rgbs]
        for extra in (4, 64, 1, 7):                              # multiples of 4 (the dword loader), and not (the gather)
            for order, bottom_up in ((jpegamd.ORDER_RGBA, False), (jpegamd.ORDER_BGRA, True)):
                got = finished(enc, queue_px4(jpegamd, enc, rgbs, dev, sub, order, 0, bottom_up, stride=4 * w + extra))
                assert got == exp, (w, h, sub, extra, order)
            for bottom_up in (False, True):
                got = finished(enc, queue_planar(jpegamd, enc, rgbs, dev, sub, "three", 0, bottom_up, stride=w + extra))
                assert got == exp, (w, h, sub, extra, bottom_up)


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_base_pointers_off_alignment(jpegamd, oracle, dev, shift):
    w, h = 1031, 37
    rgbs = pictures(jpegamd, w, h, 3, seed=shift)
    enc = jpegamd.Encoder(w, rows_for(3, h))
    for sub in (S420, S444, GRAY):
        exp = [want(oracle, r, 0, sub) for r in rgbs]
        for stride_extra in (0, 1):
            got = finished(enc, queue_px4(jpegamd, enc, rgbs, dev, sub, jpegamd.ORDER_RGBA, stride=4 * w + 4 * stride_extra,
                                              shifts=[0, shift, 0]))
            assert got == exp, (shift, sub, stride_extra)
            for plane in range(3):                               # one plane of every picture off the dword grid
                shifts = [0, 0, 0]
                shifts[plane] = shift
                got = finished(enc, queue_planar(jpegamd, enc, rgbs, dev, sub, "three", stride=w + 1 + 3 * stride_extra,
                                                     shifts=tuple(shifts)))
                assert got == exp, (shift, sub, stride_extra, plane)
        got = finished(enc, queue_planar(jpegamd, enc, rgbs, dev, sub, "three", stride=w + 1, shifts=(shift, shift, shift)))
        assert got == exp, (shift, sub, "all planes")


def test_row_stride_above_2_pow_24(jpegamd, oracle, dev):
    w, h = 520, 16
    rgbs = pictures(jpegamd, w, h, 1, seed=9)
    enc = jpegamd.Encoder(w, rows_for(1, h))
    for sub in (S420, GRAY):
        exp = [want(oracle, rgbs[0], 0, sub)]
        assert finished(enc, queue_px4(jpegamd, enc, rgbs, dev, sub, jpegamd.ORDER_RGBA, stride=WIDE_STRIDE)) == exp, sub
        assert finished(enc, queue_planar(jpegamd, enc, rgbs, dev, sub, "three", stride=WIDE_STRIDE)) == exp, sub


# ---- batch counts ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 2, 5, 8, 32])
def test_batch_counts(jpegamd, oracle, dev, count):
    w, h = 203, 117
    rgbs = pictures(jpegamd, w, h, count, seed=count)
    enc = jpegamd.Encoder(w, rows_for(count, h))
    for sub, q in ((S420, 0), (S444, 90), (GRAY, 10)):
        exp = [want(oracle, r, q, sub) for r in rgbs]
        assert finished(enc, queue_px4(jpegamd, enc, rgbs, dev, sub, jpegamd.ORDER_RGBA, q)) == exp, (count, sub)
        assert finished(enc, queue_px4(jpegamd, enc, rgbs, dev, sub, jpegamd.ORDER_BGRA, q, bottom_up=True)) == exp, (count, sub)
        assert finished(enc, queue_planar(jpegamd, enc, rgbs, dev, sub, "one", q)) == exp, (count, sub)
        assert finished(enc, queue_planar(jpegamd, enc, rgbs, dev, sub, "crop", q, bottom_up=True)) == exp, (count, sub)


def test_forty_pictures_through_encode_tensor_batch(jpegamd, oracle, dev):
    w, h = 72, 40
    rgbs = pictures(jpegamd, w, h, 40, seed=61)
    host = np.stack(rgbs)                                        # [40, H, W, 3]
    chw = torch.from_numpy(np.ascontiguousarray(host.transpose(0, 3, 1, 2))).to(dev)
    x = _rng.integers(0, 256, (40, h, w, 1), np.uint8)
    rgba = torch.from_numpy(np.concatenate([host, x], axis=3)).to(dev)
    bgra = torch.from_numpy(np.concatenate([host[..., ::-1], x], axis=3)).to(dev)
    for sub in (S420, S444):
        exp = [want(oracle, r, 0, sub) for r in rgbs]
        assert jpegamd.encode_tensor_batch(chw, 0, sub, layout="chw") == exp, sub
        assert jpegamd.encode_tensor_batch(rgba, 0, sub, layout="rgba") == exp, sub
        assert jpegamd.encode_tensor_batch(bgra, 0, sub, layout="bgra") == exp, sub
    exp = [want(oracle, r, 90, S420) for r in rgbs]
    assert jpegamd.encode_tensor_batch(chw[::2], 90, layout="chw") == exp[::2]
    assert jpegamd.encode_tensor_batch([chw[:, k].contiguous() for k in range(3)], 90, layout="chw") == exp
    assert jpegamd.encode_tensor_batch(torch.from_numpy(host).to(dev), 90, layout="hwc") == exp
    assert jpegamd.encode_tensor_batch(chw[:5], 0, 0, layout="chw") == [want(oracle, r, 0, GRAY) for r in rgbs[:5]]


def test_encode_tensor_layouts(jpegamd, oracle, dev):
    for (w, h) in ((203, 117), (64, 48), (7, 9)):
        rgb = synth_rgb(jpegamd, w, h, 77, 0)
        chw = torch.from_numpy(np.ascontiguousarray(rgb.transpose(2, 0, 1))).to(dev)
        x = _rng.integers(0, 256, (h, w, 1), np.uint8)
        bgra = torch.from_numpy(np.concatenate([rgb[..., ::-1], x], axis=2)).to(dev)
        big = torch.zeros(3, h + 4, w + 9, dtype=torch.uint8, device=dev)
        big[:, 1:1 + h, 3:3 + w] = chw
        for sub, q in ((S420, 0), (S444, 90)):
            exp = want(oracle, rgb, q, sub)
            assert jpegamd.encode_tensor(chw, q, sub, layout="chw") == exp, (w, h, sub)
            assert jpegamd.encode_tensor(big[:, 1:1 + h, 3:3 + w], q, sub, layout="chw") == exp, (w, h, sub)
            assert jpegamd.encode_tensor(bgra, q, sub, layout="bgra") == exp, (w, h, sub)
            assert jpegamd.encode_tensor(torch.from_numpy(rgb).to(dev), q, sub, layout="hwc") == exp, (w, h, sub)


# ---- capacity ---------------------------------------------------------------------------------------------------------------
def test_one_picture_of_a_batch_one_byte_short(jpegamd, oracle, dev):
    """A capacity one byte short for one picture of a batch: jpegamd_encoder_finish answers JPEGAMD_ERR_HUFF_CAPACITY (-8), nothing is
    written behind any capacity, the other pictures are correct, and the short picture's size is what the entry the call stands
    for reports -- 0 from the colour batch (jpegamd_encode_color_batch_async), the size the file would have had from the grayscale
    batch (jpegamd_encode_batch_async: a size above the capacity marks a cut stream, which jpegamd_gather_streams and
    tests/test_gpu_parity.py rely on).  The new layouts take both contracts as they are."""
    w, h = 160, 96
    flat = [synth_rgb(jpegamd, w, h, 7 + i, 2) for i in range(3)]
    noise = synth_rgb(jpegamd, w, h, 9, 1)
    rgbs = [flat[0], noise, flat[1], flat[2]]
    enc = jpegamd.Encoder(w, rows_for(4, h))
    for sub in (S420, S444, GRAY):
        exp = [want(oracle, r, 0, sub) for r in rgbs]
        cap = len(exp[1]) - 1                                    # one byte short for the noise picture alone
        assert cap > max(len(exp[k]) for k in (0, 2, 3))
        for queue in (lambda c: queue_px4(jpegamd, enc, rgbs, dev, sub, jpegamd.ORDER_RGBA, cap=c),
                      lambda c: queue_planar(jpegamd, enc, rgbs, dev, sub, "one", cap=c)):
            o, keep = queue(cap)
            with pytest.raises(jpegamd.JpegAmdError) as err:
                enc.finish()
            assert err.value.code == -8
            got = intact_files(o)                                      # (checks the guard bytes; a file is cut at the capacity)
            assert int(o.sizes[1].item()) == (len(exp[1]) if sub == GRAY else 0), sub
            assert [got[k] for k in (0, 2, 3)] == [exp[k] for k in (0, 2, 3)], sub
            assert finished(enc, queue(cap + 1)) == exp, sub    # the exact capacity fits; the context is clean again


# ---- one context, interleaved ---------------------------------------------------------------------------------------------
def test_one_context_interleaved_sources(jpegamd, oracle, dev):
    """Packed RGB colour, planar colour, GRAY, RGBA grayscale, packed again, queued on one context without a finish between them:
    the new sources must not disturb the constant sets or the scratch of the others."""
    w, h = 203, 117
    rgbs = pictures(jpegamd, w, h, 3, seed=71)
    enc = jpegamd.Encoder(w, rows_for(3, h))
    jobs = []

    def packed(sub, q):
        px = [upload(np.ascontiguousarray(r).reshape(h, -1), dev, 3 * w) for r in rgbs]
        o = Outputs(dev, 3, cap_for(jpegamd, w, h, sub))
        imgs = [jpegamd.Encoder.image(ptr, w, h, 3 * w, False, jpegamd.ORDER_RGB, q) for _, ptr in px]
        enc.encode_color_batch_async(imgs, sub, o.out_ptrs, o.cap, o.size_ptrs, stream())
        jobs.append((o, px, [want(oracle, r, q, sub) for r in rgbs]))

    def gray(q):
        lum = [((r.astype(np.int64) * (77, 150, 29)).sum(axis=2) >> 8).astype(np.uint8) for r in rgbs]
        px = [upload(y, dev, w) for y in lum]
        o = Outputs(dev, 3, cap_for(jpegamd, w, h, GRAY))
        imgs = [jpegamd.Encoder.image(ptr, w, h, w, False, jpegamd.ORDER_GRAY, q) for _, ptr in px]
        enc.encode_batch_async(imgs, o.out_ptrs, o.cap, o.size_ptrs, True, stream())
        jobs.append((o, px, [want(oracle, r, q, GRAY) for r in rgbs]))

    packed(S420, 0)
    jobs.append(queue_planar(jpegamd, enc, rgbs, dev, S444, "crop", 90) + ([want(oracle, r, 90, S444) for r in rgbs],))
    gray(0)
    jobs.append(queue_px4(jpegamd, enc, rgbs, dev, GRAY, jpegamd.ORDER_RGBA, 10) + ([want(oracle, r, 10, GRAY) for r in rgbs],))
    packed(S444, 10)
    jobs.append(queue_planar(jpegamd, enc, rgbs, dev, GRAY, "three", 0, stride=w + 1) + ([want(oracle, r, 0, GRAY) for r in rgbs],))
    jobs.append(queue_px4(jpegamd, enc, rgbs, dev, S420, jpegamd.ORDER_BGRA, 90, bottom_up=True) + ([want(oracle, r, 90, S420) for r in rgbs],))
    packed(S420, 90)
    enc.finish()
    for i, (o, keep, exp) in enumerate(jobs):
        assert intact_files(o) == exp, i


# ---- full size --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", ["PIPELINE_PAIR", "PIPELINE_STITCH"])
def test_four_4096_pictures_per_layout(jpegamd, dev, pipeline):
    """4096 x 4096, Q = 50, 4:2:0, a batch of 4: every layout against the packed batch entry on the same pixels, by hash."""
    w = h = 4096
    rgbs = [synth_rgb(jpegamd, w, h, 91 + i, i % 2) for i in range(4)]
    enc = jpegamd.Encoder(w, rows_for(4, h))
    enc.set_pipeline(getattr(jpegamd, pipeline))
    cap = 2 * w * h + (1 << 20)

    def digests(files):
        assert all(len(f) > 1000 for f in files)
        return [hashlib.sha256(f).hexdigest() for f in files]

    px = [upload(np.ascontiguousarray(r).reshape(h, -1), dev, 3 * w) for r in rgbs]
    o = Outputs(dev, 4, cap)
    imgs = [jpegamd.Encoder.image(ptr, w, h, 3 * w, False, jpegamd.ORDER_RGB, 50) for _, ptr in px]
    enc.encode_color_batch_async(imgs, S420, o.out_ptrs, o.cap, o.size_ptrs, stream())
    enc.finish()
    exp = digests(intact_files(o))
    del px, o
    assert digests(finished(enc, queue_px4(jpegamd, enc, rgbs, dev, S420, jpegamd.ORDER_RGBA, 50, cap=cap))) == exp
    assert digests(finished(enc, queue_px4(jpegamd, enc, rgbs, dev, S420, jpegamd.ORDER_BGRA, 50, cap=cap))) == exp
    assert digests(finished(enc, queue_planar(jpegamd, enc, rgbs, dev, S420, "one", 50, cap=cap))) == exp
