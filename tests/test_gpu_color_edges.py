"""The colour path (jpegamd_encode_color_async) and single-channel input (JPEGAMD_ORDER_GRAY) at the edges the grayscale suite pins
(tests/test_gpu_edges.py, tests/test_gpu_parity.py): declared limits through both pipelines, every stored layout, 16 MiB strides,
the extreme blocks of the subnormal matrix operand, chroma planes chosen sample by sample (tests/color_fixtures.py), exact
capacities, unaligned outputs, calls queued back to back, and the wrap of k_stitch's 14-bit epoch.  Byte for byte: GRAY against
the oracle, colour against the CPU model of tests/color_model.py.  Every test needs an MI355X; nothing here reads /root/reference."""
from __future__ import annotations

import random

import numpy as np
import pytest

import color_fixtures as cf
import color_model as cm
import scan_model as sm
from gpu_support import WIDE_STRIDE, ColorCall, dev, encode_gray, model, rows_for, stored_rows, stream, synth_rgb, upload     # noqa: F401
from gpu_support import gray_bmp_sized as gray_bmp

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def encode_gray_batch(jpegamd, enc, planes, dev, quality=0):
    h, w = planes[0].shape
    keep = [upload(stored_rows(p, False), dev, w) for p in planes]
    cap = jpegamd.max_jfif_bytes(w, h)
    outs = [torch.empty(cap, dtype=torch.uint8, device=dev) for _ in planes]
    sizes = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in planes]
    imgs = [jpegamd.Encoder.image(ptr, w, h, w, False, jpegamd.ORDER_GRAY, quality) for _, ptr in keep]
    enc.encode_batch_async(imgs, [o.data_ptr() for o in outs], cap, [s.data_ptr() for s in sizes], True, stream())
    enc.finish()
    return [bytes(o[:int(s.item())].cpu().numpy()) for o, s in zip(outs, sizes)]


def encode_color(jpegamd, enc, rgb, dev, sub, **kw):
    call = ColorCall(jpegamd, enc, rgb, dev, sub, **kw)
    st = enc.finish()
    got, intact = call.result()
    assert len(got) == st.jfif_bytes and intact
    return got, st


# ---- GRAY input -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(65535, 8), (8, 65535), (65528, 24), (4104, 8), (4096, 8), (65535, 1), (1, 65535)])
def test_gray_dimension_limits(jpegamd, oracle, dev, w, h):
    """test_dimension_limits for one-byte input: each shape alone and as a batch of two, through both pipelines."""
    enc = jpegamd.Encoder(w, rows_for(2, h))
    for kind, q in ((0, 0), (1, 90)):
        planes = [synth_rgb(jpegamd, w, h, 80 + i + kind, kind)[:, :, 1 + i].copy() for i in range(2)]
        want = [oracle.encode_bmp(gray_bmp(p), q or 50) for p in planes]
        for pipeline in (jpegamd.PIPELINE_PAIR, jpegamd.PIPELINE_STITCH):
            enc.set_pipeline(pipeline)
            assert encode_gray(jpegamd, enc, planes[0], dev, quality=q) == want[0], (w, h, kind, pipeline, "single")
            assert encode_gray_batch(jpegamd, enc, planes, dev, quality=q) == want, (w, h, kind, pipeline, "batch of two")


def test_gray_layouts(jpegamd, oracle, dev):
    """Bottom-up and top-down rows, through the dword (v_perm) loader -- aligned pointer and stride -- and the clamped byte loader
    (pointer shifted by 1..3, odd strides), both pipelines."""
    for (w, h) in ((203, 117), (64, 40), (9, 7), (520, 33)):
        p = synth_rgb(jpegamd, w, h, w + h, 0)[:, :, 0].copy()
        p[:, :min(w, 8)] = np.arange(min(w, 8))[None, :] * 36
        want = oracle.encode_bmp(gray_bmp(p))
        enc = jpegamd.Encoder(w, h)
        for pipeline in (jpegamd.PIPELINE_PAIR, jpegamd.PIPELINE_STITCH):
            enc.set_pipeline(pipeline)
            for bottom_up in (True, False):
                for stride, shift in (((w + 3) & ~3, 0), ((w + 3) // 4 * 4 + 64, 0), (w, 1), (w + 5, 2), ((w + 3) & ~3, 3), (w | 1, 0)):
                    got = encode_gray(jpegamd, enc, p, dev, bottom_up=bottom_up, stride=stride, shift=shift)
                    assert got == want, (w, h, pipeline, bottom_up, stride, shift)


def test_gray_row_stride_of_16_mib_and_more(jpegamd, oracle, dev):
    w, h = 200, 20
    p = synth_rgb(jpegamd, w, h, 31, 0)[:, :, 2].copy()
    want = oracle.encode_bmp(gray_bmp(p))
    enc = jpegamd.Encoder(w, h)
    for bottom_up in (False, True):
        assert encode_gray(jpegamd, enc, p, dev, bottom_up=bottom_up, stride=WIDE_STRIDE) == want, bottom_up


def test_gray_extreme_blocks_through_the_subnormal_matrix_operand(jpegamd, oracle, dev):
    """test_extreme_blocks_through_the_subnormal_matrix_operand as a GRAY plane: Q = 100 / 50 / 10, through the dword loader and
    with a shifted pointer; the stage taps equal the oracle's quantised coefficients."""
    p = cf.extreme_plane(jpegamd.cos_lut())
    h, w = p.shape
    enc = jpegamd.Encoder(w, h)
    for q in (100, 50, 10):
        want = oracle.encode_bmp(gray_bmp(p), q)
        assert encode_gray(jpegamd, enc, p, dev, quality=q) == want, (q, "dword loader")
        assert encode_gray(jpegamd, enc, p, dev, stride=w + 1, shift=1, quality=q) == want, (q, "byte loader")
    st = oracle.stages(gray_bmp(p))
    n = st["zigzag"].shape[0]
    for stride, shift in ((w, 0), (w + 1, 1)):
        t, ptr = upload(stored_rows(p, False), dev, stride, shift)
        zz = torch.zeros(n * 64, dtype=torch.int16, device=dev)
        enc.debug_stages(jpegamd.Encoder.image(ptr, w, h, stride, False, jpegamd.ORDER_GRAY, 0), 0, zz.data_ptr(), 0)
        assert np.array_equal(zz.cpu().numpy().reshape(n, 64), st["zigzag"]), shift


# ---- chroma content through the kernel -------------------------------------------------------------------------------------
def test_extreme_chroma_blocks(jpegamd, oracle, dev):
    """The same extreme blocks as Cb, then as Cr (tests/color_fixtures.py: RGB whose chroma plane is exactly the block set), at 4:4:4
    and 4:2:0, Q = 100 / 50 / 10 / 1: the chroma guard band on the hardware."""
    plane = cf.extreme_plane(jpegamd.cos_lut())
    enc = jpegamd.Encoder(2 * plane.shape[1], 2 * plane.shape[0])
    for which in ("cb", "cr"):
        for sub in (cm.SUB_444, cm.SUB_420):
            rgb = cf.rgb_for_plane(plane, which, sub, base=plane[::-1])
            for q in (100, 50, 10, 1):
                got, _ = encode_color(jpegamd, enc, rgb, dev, sub, quality=q, bottom_up=q == 50)
                assert got == model(oracle, rgb, q, sub), (which, sub, q)


def test_chroma_symbol_coverage(jpegamd, oracle, dev):
    """Every DC size, every AC size, every run, the 10-bit chroma ZRL, EOB and a block without EOB (asserted on the CPU in
    test_color_host.py) in the chroma scans, both pipelines."""
    plane = cf.symbol_plane(oracle)
    q = cf.SYMBOL_QUALITY
    enc = jpegamd.Encoder(2 * plane.shape[1], 2 * plane.shape[0])
    for pipeline in (jpegamd.PIPELINE_PAIR, jpegamd.PIPELINE_STITCH):
        enc.set_pipeline(pipeline)
        for which in ("cb", "cr"):
            for sub in (cm.SUB_444, cm.SUB_420):
                rgb = cf.rgb_for_plane(plane, which, sub)
                got, _ = encode_color(jpegamd, enc, rgb, dev, sub, quality=q)
                assert got == model(oracle, rgb, q, sub), (pipeline, which, sub)


def test_chroma_ties_take_the_exact_order_fallback(jpegamd, oracle, dev):
    """Chroma coefficients next to rounding ties: the colour call's fallbacks minus those of the grayscale encode of the same picture
    (its Y scan) are the chroma scans' own, and must be above 0; the bytes equal the model's."""
    plane = cf.tie_plane()
    q = cf.TIE_QUALITY
    enc = jpegamd.Encoder(2 * plane.shape[1], 2 * plane.shape[0])
    for which in ("cb", "cr"):
        for sub in (cm.SUB_444, cm.SUB_420):
            rgb = cf.rgb_for_plane(plane, which, sub)
            got, st = encode_color(jpegamd, enc, rgb, dev, sub, quality=q)
            assert got == model(oracle, rgb, q, sub), (which, sub)
            h, w, _ = rgb.shape
            t, ptr = upload(stored_rows(rgb, False), dev, 3 * w)
            cap = jpegamd.max_jfif_bytes(w, h)
            out = torch.empty(cap, dtype=torch.uint8, device=dev)
            size = torch.zeros(1, dtype=torch.int64, device=dev)
            enc.encode_async(jpegamd.Encoder.image(ptr, w, h, 3 * w, False, jpegamd.ORDER_RGB, q), out.data_ptr(), cap, size.data_ptr(),
                             True, stream())
            gray = enc.finish().exact_fallbacks
            assert st.exact_fallbacks - gray > 0, (which, sub, st.exact_fallbacks, gray)


# ---- colour geometry, layouts, capacity ------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(65535, 8), (8, 65535), (65535, 1), (1, 65535), (4104, 8), (4097, 9)])
def test_color_dimension_limits(jpegamd, oracle, dev, w, h):
    rgb = synth_rgb(jpegamd, w, h, 90 + w % 7, 0)
    enc = jpegamd.Encoder(w, h)
    for sub in (cm.SUB_420, cm.SUB_444):
        want = model(oracle, rgb, 0, sub)
        for pipeline in (jpegamd.PIPELINE_PAIR, jpegamd.PIPELINE_STITCH):
            enc.set_pipeline(pipeline)
            got, _ = encode_color(jpegamd, enc, rgb, dev, sub, bgr=pipeline == jpegamd.PIPELINE_STITCH)
            assert got == want, (w, h, sub, pipeline)


def _chroma_scan_model(oracle, rgb, quality, sub, rows=2048):
    """The model's Cb and Cr scans of a large picture, its planes made `rows` picture rows at a time (bounded memory)."""
    cq = cm.scaled_table(cm.CHROMA_Q, quality)
    parts = [[], []]
    for y in range(0, rgb.shape[0], rows):
        for k, plane in enumerate(cm.chroma_planes(rgb[y:y + rows], sub)):
            parts[k].append(plane)
    out = []
    for comp, k in ((2, 0), (3, 1)):
        out += [cm.sos(comp), sm.pack_scan(oracle, cm.plane_zigzag(oracle, np.concatenate(parts[k]), cq), True)]
    return b"".join(out)


def test_auto_with_mixed_pipelines(jpegamd, oracle, dev):
    """2056 x 65535 under AUTO: at 4:2:0 the Y scan takes k_stitch (16 384 segments) and the 1028 x 32768 chroma scans the pair;
    against the model.  At 4:4:4 all three scans take k_stitch: against the pair's output of the same picture, and its Y scan
    against the grayscale oracle."""
    w, h = 2056, 65535
    bmp = jpegamd.synth_bmp(w, h, 11, 0, 0)
    rgb = cm.read_bmp_rgb(bmp)
    y_scan = cm.gray_scan(oracle, bmp, 0)
    want = cm.color_prefix(w, h, 0, cm.SUB_420) + y_scan + _chroma_scan_model(oracle, rgb, 0, cm.SUB_420) + b"\xff\xd9"
    enc = jpegamd.Encoder(w, h)
    got, _ = encode_color(jpegamd, enc, rgb, dev, cm.SUB_420)
    assert got == want
    auto, _ = encode_color(jpegamd, enc, rgb, dev, cm.SUB_444, bgr=True, bottom_up=True)
    enc.set_pipeline(jpegamd.PIPELINE_PAIR)
    pair, _ = encode_color(jpegamd, enc, rgb, dev, cm.SUB_444)
    assert auto == pair
    prefix = cm.color_prefix(w, h, 0, cm.SUB_444)
    assert auto[:len(prefix)] == prefix and auto[len(prefix):len(prefix) + len(y_scan) + len(cm.sos(2))] == y_scan + cm.sos(2)


def test_color_layouts(jpegamd, oracle, dev):
    """RGB / BGR x top-down / bottom-up, row pointers shifted by 0..3, strides 3w, 3w + 1, 3w + 5 and a multiple of 4; widths 8k,
    8k + 1, 8k + 7 around k_chroma_planes' whole-dword test (x0 + kPix <= width), odd heights."""
    enc = jpegamd.Encoder(600, 64)
    layouts = [(0, 0), (1, 1), (2, 5), (3, -4), (0, -4), (3, 0), (1, 5), (2, 1)]      # (shift, stride - 3w; -4: the next multiple of 4)
    i = 0
    for w in (1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 519, 520, 521, 527):
        for h in (1, 9, 33):
            rgb = synth_rgb(jpegamd, w, h, w * 3 + h, (w + h) % 4)
            for sub in (cm.SUB_420, cm.SUB_444):
                want = model(oracle, rgb, 0, sub)
                for bgr in (False, True):
                    for bottom_up in (False, True):
                        shift, extra = layouts[i % len(layouts)]
                        i += 1
                        stride = (3 * w + 3) // 4 * 4 if extra == -4 else 3 * w + extra
                        got, _ = encode_color(jpegamd, enc, rgb, dev, sub, bgr=bgr, bottom_up=bottom_up, stride=stride, shift=shift)
                        assert got == want, (w, h, sub, bgr, bottom_up, shift, stride)


def test_color_row_stride_of_16_mib_and_more(jpegamd, oracle, dev):
    w, h = 67, 9
    rgb = synth_rgb(jpegamd, w, h, 5, 0)
    enc = jpegamd.Encoder(w, h)
    for sub, bgr, bottom_up in ((cm.SUB_420, False, True), (cm.SUB_444, True, False)):
        got, _ = encode_color(jpegamd, enc, rgb, dev, sub, bgr=bgr, bottom_up=bottom_up, stride=WIDE_STRIDE, shift=1)
        assert got == model(oracle, rgb, 0, sub), (sub, bgr, bottom_up)


def test_color_capacity_edges(jpegamd, oracle, dev):
    """A capacity of exactly the file's size succeeds; one where the prefix and Y fit but Cb does not, and one where everything but
    the Cr scan and EOI fits, end in -8 with a size of 0 and nothing written behind the capacity.  Outputs 1..15 bytes past a
    16-byte boundary (k_append_scans writes single bytes at any offset)."""
    w, h = 333, 250
    rgb = synth_rgb(jpegamd, w, h, 4, 0)
    enc = jpegamd.Encoder(w, h)
    full = model(oracle, rgb, 0, cm.SUB_420)
    got, _ = encode_color(jpegamd, enc, rgb, dev, cm.SUB_420, cap=len(full))
    assert got == full
    cb_at = full.index(cm.sos(2), len(cm.color_prefix(w, h, 0, cm.SUB_420)))
    cr_at = full.index(cm.sos(3), cb_at)
    for cap in (cb_at + 4, cr_at + len(cm.sos(3))):
        for out_off in (0, 7):
            call = ColorCall(jpegamd, enc, rgb, dev, cm.SUB_420, cap=cap, out_off=out_off)
            with pytest.raises(jpegamd.JpegAmdError) as ei:
                enc.finish()
            assert ei.value.code == -8, cap
            _, intact = call.result()
            assert int(call.size.item()) == 0 and intact, (cap, out_off)
    for out_off in range(1, 16):
        got, _ = encode_color(jpegamd, enc, rgb, dev, cm.SUB_420 if out_off % 2 else cm.SUB_444, cap=None, out_off=out_off)
        assert got == (full if out_off % 2 else model(oracle, rgb, 0, cm.SUB_444)), out_off
    got, _ = encode_color(jpegamd, enc, rgb, dev, cm.SUB_420, cap=len(full), out_off=13)
    assert got == full


def test_color_sweep_slice_through_one_context(jpegamd, oracle, dev):
    """150 fixed-seed random colour calls: 1 x 1 .. 2000 x 900, every synthetic kind, qualities 1..100, both subsamplings, all four
    stored layouts, both pipelines, through ONE context whose colour scratch grows and is reused."""
    rng = random.Random(15)
    enc = jpegamd.Encoder(2000, 900)
    for i in range(150):
        cls = rng.random()
        if cls < 0.5:
            w, h = rng.randint(1, 300), rng.randint(1, 200)
        elif cls < 0.8:
            w, h = rng.randint(250, 2000), rng.randint(1, 64)
        else:
            w, h = rng.randint(300, 2000), rng.randint(200, 900)
        seed, kind, flags = rng.randint(1, 10 ** 6), rng.randint(0, 3), rng.randint(0, 3)
        q = rng.choice([50, 10, 90, rng.randint(1, 100), rng.randint(1, 100)])
        sub = rng.choice([cm.SUB_420, cm.SUB_444])
        bgr, bottom_up = rng.random() < 0.5, rng.random() < 0.5
        enc.set_pipeline(rng.choice([jpegamd.PIPELINE_PAIR, jpegamd.PIPELINE_STITCH]))
        rgb = synth_rgb(jpegamd, w, h, seed, kind, flags)
        got, _ = encode_color(jpegamd, enc, rgb, dev, sub, quality=q, bgr=bgr, bottom_up=bottom_up)
        assert got == model(oracle, rgb, q, sub), (i, w, h, seed, kind, flags, q, sub, bgr, bottom_up)


# ---- state across calls ---------------------------------------------------------------------------------------------------
def test_pipelined_colour_calls(jpegamd, oracle, dev):
    """Colour calls queued on one context and one stream with no finish between them, each changing what the context caches: a
    larger picture (the colour scratch is reallocated behind queued work), another quality (chroma constants re-uploaded), the
    other subsampling alone (a new header).  One finish; every output equals its model."""
    a = synth_rgb(jpegamd, 320, 200, 1, 0)
    b = synth_rgb(jpegamd, 1100, 700, 2, 3)
    steps = [(a, 50, cm.SUB_420), (b, 50, cm.SUB_420), (b, 80, cm.SUB_420), (b, 80, cm.SUB_444), (a, 80, cm.SUB_444)]
    enc = jpegamd.Encoder(1100, 700)
    calls = [ColorCall(jpegamd, enc, rgb, dev, sub, quality=q, bgr=i % 2 == 1) for i, (rgb, q, sub) in enumerate(steps)]
    enc.finish()
    for i, (call, (rgb, q, sub)) in enumerate(zip(calls, steps)):
        got, intact = call.result()
        assert intact and got == model(oracle, rgb, q, sub), (i, q, sub)


def test_stitch_epoch_wrap(jpegamd, oracle, dev):
    """k_stitch tags its hand-off granules with a 14-bit epoch; run_stitch clears them when the tag would pass 16383.

    How the launches are counted: a fresh context starts at epoch 0, and under PIPELINE_STITCH every grayscale encode (or batch)
    launches k_stitch once and every colour call three times (Y, Cb, Cr), in that order; nothing else launches it.  Launch n
    (1-based) therefore runs at epoch ((n - 1) mod 16383) + 1, and launches 16384, 32767 and 49150 are the first after a clear.
    Tiny 16 x 16 GRAY fillers advance the count; 8200 x 520 pictures (hundreds of workgroups) run around each wrap and at the
    epochs just before it, so that stale granules with the re-used tags fill every slot: between two grayscale encodes, between
    the Y and Cb scans of a colour call, and between its Cb and Cr scans."""
    period = 16383
    w, h = 8200, 520
    enc = jpegamd.Encoder(w, h)
    enc.set_pipeline(jpegamd.PIPELINE_STITCH)
    big_p = synth_rgb(jpegamd, w, h, 41, 0)[:, :, 1].copy()
    big_rgb = synth_rgb(jpegamd, w, h, 42, 0)
    want_p = oracle.encode_bmp(gray_bmp(big_p))
    want_rgb = model(oracle, big_rgb, 0, cm.SUB_420)
    small = np.random.default_rng(1).integers(0, 256, (16, 16), np.uint8)
    want_small = oracle.encode_bmp(gray_bmp(small))
    st, sptr = upload(small, dev, 16)
    scap = jpegamd.max_jfif_bytes(16, 16)
    sout = torch.empty(scap, dtype=torch.uint8, device=dev)
    ssize = torch.zeros(1, dtype=torch.int64, device=dev)
    simg = jpegamd.Encoder.image(sptr, 16, 16, 16, False, jpegamd.ORDER_GRAY, 0)
    n = 0                                                                  # k_stitch launches so far

    def fill_to(last):
        nonlocal n
        while n < last:
            enc.encode_async(simg, sout.data_ptr(), scap, ssize.data_ptr(), True, stream())
            n += 1
            if n % 1000 == 0 or n == last:
                enc.finish()
        assert bytes(sout[:int(ssize.item())].cpu().numpy()) == want_small, n

    def big_gray():
        nonlocal n
        assert encode_gray(jpegamd, enc, big_p, dev) == want_p, n + 1
        n += 1

    def big_color():
        nonlocal n
        got, _ = encode_color(jpegamd, enc, big_rgb, dev, cm.SUB_420)
        assert got == want_rgb, n + 1
        n += 3

    for _ in range(3):
        big_gray()                                                         # epochs 1..3 of the first period
    wrap = period + 1
    fill_to(wrap - 4)
    for _ in range(6):
        big_gray()                                                         # launches wrap - 3 .. wrap + 2: the wrap between two of them
    assert n == wrap + 2
    wrap = 2 * period + 1
    fill_to(wrap - 5)
    big_color()                                                            # wrap - 4 .. wrap - 2
    big_color()                                                            # Y at wrap - 1, Cb at the wrap, Cr after it
    assert n == wrap + 1
    wrap = 3 * period + 1
    fill_to(wrap - 6)
    big_color()                                                            # wrap - 5 .. wrap - 3
    big_color()                                                            # Y at wrap - 2, Cb at wrap - 1, Cr at the wrap
    assert n == wrap
    big_color()
    big_gray()
    fill_to(n + 10)
