"""Colour files and single-channel (GRAY) input through the C-ABI into the HIP kernels, byte for byte against the oracle
(GRAY) and the CPU model of tests/color_model.py (colour).  Every test needs an MI355X."""
from __future__ import annotations

import io

import numpy as np
import pytest

import color_model as cm
from gpu_support import ColorCall, dev, encode_gray, stream, synth_rgb, upload     # noqa: F401
from gpu_support import gray_bmp_sized as gray_bmp

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def encode_color(jpegamd, enc, rgb, dev, sub, quality=0, bgr_bottom_up=False, cap=None, stride=None, shift=0):
    call = ColorCall(jpegamd, enc, rgb, dev, sub, quality=quality, bgr=bgr_bottom_up, bottom_up=bgr_bottom_up, stride=stride, shift=shift, cap=cap)
    st = enc.finish()
    got, intact = call.result()
    n = int(call.size.item())
    assert n == st.jfif_bytes and n <= call.cap
    assert intact
    return got, st


def decode_rgb(jf: bytes):
    from PIL import Image
    img = Image.open(io.BytesIO(jf))
    img.load()
    return img


# ---- GRAY input ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(1, 1), (7, 9), (333, 250), (1024, 64), (4097, 33)])
def test_gray_input_matches_the_oracle(jpegamd, oracle, dev, w, h):
    rng = np.random.default_rng(w * 7 + h)
    p = synth_rgb(jpegamd, w, h, w + h, 0)[:, :, 1].copy() if w * h > 1 else rng.integers(0, 256, (h, w), np.uint8)
    enc = jpegamd.Encoder(w, h)
    got = encode_gray(jpegamd, enc, p, dev)
    assert got == oracle.encode_bmp(gray_bmp(p))


def test_gray_input_unaligned_and_odd_stride(jpegamd, oracle, dev):
    w, h = 203, 117
    p = np.random.default_rng(3).integers(0, 256, (h, w), np.uint8)
    p[:, :64] = np.linspace(0, 255, 64, dtype=np.uint8)[None, :]
    enc = jpegamd.Encoder(w, h)
    want = oracle.encode_bmp(gray_bmp(p))
    assert encode_gray(jpegamd, enc, p, dev, stride=w, shift=1) == want            # unaligned pointer
    assert encode_gray(jpegamd, enc, p, dev, stride=w + 7, shift=0) == want        # odd stride
    assert encode_gray(jpegamd, enc, p, dev, stride=w + 13, shift=3) == want
    q90 = oracle.encode_bmp(gray_bmp(p), 90)
    assert encode_gray(jpegamd, enc, p, dev, stride=256, quality=90) == q90        # aligned stride: the dword loader


def test_gray_batch_of_eight(jpegamd, oracle, dev):
    w, h, n = 300, 72, 8
    enc = jpegamd.Encoder(w, n * h)
    planes = [synth_rgb(jpegamd, w, h, 11 + i, i % 4)[:, :, i % 3].copy() for i in range(n)]
    ts = [upload(p, dev, w)[0] for p in planes]
    cap = jpegamd.max_jfif_bytes(w, h)
    outs = [torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(n)]
    sizes = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(n)]
    imgs = [jpegamd.Encoder.image(t.data_ptr(), w, h, w, False, jpegamd.ORDER_GRAY, 0) for t in ts]
    enc.encode_batch_async(imgs, [o.data_ptr() for o in outs], cap, [s.data_ptr() for s in sizes], True, stream())
    enc.finish()
    for i in range(n):
        got = bytes(outs[i][:int(sizes[i].item())].cpu().numpy())
        assert got == oracle.encode_bmp(gray_bmp(planes[i])), i


def test_gray_stage_taps(jpegamd, oracle, dev):
    w, h = 70, 20
    p = synth_rgb(jpegamd, w, h, 5, 0)[:, :, 0].copy()
    enc = jpegamd.Encoder(w, h)
    t, ptr = upload(p, dev, w)
    nb = ((w + 7) // 8) * ((h + 7) // 8)
    zz = torch.zeros(nb * 64, dtype=torch.int16, device=dev)
    enc.debug_stages(jpegamd.Encoder.image(ptr, w, h, w, False, jpegamd.ORDER_GRAY, 0), 0, zz.data_ptr(), 0)
    st = oracle.stages(gray_bmp(p))
    assert np.array_equal(zz.cpu().numpy().reshape(nb, 64), st["zigzag"])


# ---- colour ---------------------------------------------------------------------------------------------------------------
COLOR_CASES = [(1, 1, 1, 0), (7, 9, 2, 1), (17, 33, 3, 2), (333, 250, 4, 0), (640, 360, 5, 3)]


@pytest.mark.parametrize("sub", [2, 1])
def test_color_matches_the_model(jpegamd, oracle, dev, sub):
    enc = jpegamd.Encoder(640, 360)
    for i, (w, h, seed, kind) in enumerate(COLOR_CASES):
        for q in (10, 50, 90, 100):
            bmp = jpegamd.synth_bmp(w, h, seed, kind, 0)
            want = cm.color_file(oracle, bmp, q, sub)
            rgb = cm.read_bmp_rgb(bmp)
            got, _ = encode_color(jpegamd, enc, rgb, dev, sub, quality=q, bgr_bottom_up=(i + q) % 2 == 0)
            assert got == want, (w, h, kind, q, sub, len(got), len(want))
            img = decode_rgb(got)
            assert img.mode == "RGB" and img.size == (w, h)


def test_color_bmp_entry_and_y_scan(jpegamd, oracle, dev):
    bmp = jpegamd.synth_bmp(333, 250, 9, 0, 0)
    for sub in (1, 2):
        got = jpegamd.encode_bmp_bytes_color(bmp, 0, sub)
        assert got == cm.color_file(oracle, bmp, 0, sub)
        prefix = cm.color_prefix(333, 250, 0, sub)
        y_end = got.index(cm.sos(2), len(prefix))
        assert got[len(prefix):y_end] == oracle.encode_bmp(bmp)[328:-2]       # the Y scan IS the grayscale file's segment
    with pytest.raises(jpegamd.JpegAmdError):
        jpegamd.encode_bmp_bytes_color(bmp, 0, 3)


def test_color_8192_square(jpegamd, oracle, dev):
    bmp = jpegamd.synth_bmp(8192, 8192, 7, 0, 0)
    enc = jpegamd.Encoder(8192, 8192)
    rgb = cm.read_bmp_rgb(bmp)
    got, st = encode_color(jpegamd, enc, rgb, dev, 2, bgr_bottom_up=True)
    assert got == cm.color_file(oracle, bmp, 0, 2)
    assert st.entropy_bits > 0 and st.ns_total == 0
    assert decode_rgb(got).size == (8192, 8192)


def test_color_pair_and_stitch_agree(jpegamd, oracle, dev):
    rgb = synth_rgb(jpegamd, 1500, 700, 12, 0)
    enc = jpegamd.Encoder(1500, 700)
    enc.set_pipeline(jpegamd.PIPELINE_PAIR)
    pair, sp = encode_color(jpegamd, enc, rgb, dev, 2)
    enc.set_pipeline(jpegamd.PIPELINE_STITCH)
    stitch, ss = encode_color(jpegamd, enc, rgb, dev, 2)
    assert pair == stitch
    assert (sp.entropy_bits, sp.stuffed_bytes, sp.exact_fallbacks) == (ss.entropy_bits, ss.stuffed_bytes, ss.exact_fallbacks)
    enc.set_pipeline(jpegamd.PIPELINE_STITCH)
    s444, _ = encode_color(jpegamd, enc, rgb, dev, 1)
    assert s444 == cm.color_file(oracle, cm.write_bmp(rgb), 0, 1)


def test_color_capacity_one_byte_short(jpegamd, dev):
    rgb = synth_rgb(jpegamd, 333, 250, 4, 0)
    enc = jpegamd.Encoder(333, 250)
    full, _ = encode_color(jpegamd, enc, rgb, dev, 2)
    for cap in (len(full) - 1, len(full) // 2, 100):
        call = ColorCall(jpegamd, enc, rgb, dev, 2, cap=cap)
        with pytest.raises(jpegamd.JpegAmdError) as ei:
            enc.finish()
        assert ei.value.code == -8
        assert int(call.size.item()) == 0
        assert call.result()[1], cap
    again, _ = encode_color(jpegamd, enc, rgb, dev, 2)                   # the context is fine afterwards
    assert again == full


def test_color_stats_are_sums_over_the_scans(jpegamd, dev):
    rgb = synth_rgb(jpegamd, 640, 360, 5, 0)
    enc = jpegamd.Encoder(640, 360)
    _, st = encode_color(jpegamd, enc, rgb, dev, 2)
    gray_bits = encode_gray_stats(jpegamd, dev, rgb)
    assert st.entropy_bits > gray_bits > 0
    enc.set_profiling(2)
    _, st2 = encode_color(jpegamd, enc, rgb, dev, 2)
    ns = enc.color_profile(0)
    assert all(v > 0 for i, v in enumerate(ns) if i not in (2, 5, 8)) and st2.ns_total >= max(ns)
    assert st2.ns_transform == ns[0] + ns[1] + ns[4] + ns[7]
    enc.set_profiling(1)                                                  # one slot: a grayscale call takes it over from a colour one
    encode_color(jpegamd, enc, rgb, dev, 2)
    encode_gray(jpegamd, enc, rgb[:, :, 0].copy(), dev)
    with pytest.raises(jpegamd.JpegAmdError):
        enc.color_profile(0)
    st3 = enc.profile(0)
    assert st3.ns_transform > 0 and st3.ns_total >= st3.ns_transform


def encode_gray_stats(jpegamd, dev, rgb):
    bmp = cm.write_bmp(rgb)
    img, off = jpegamd.parse_bmp(bmp)
    t = torch.frombuffer(bytearray(bmp[off:off + img.row_stride * img.height]), dtype=torch.uint8).to(dev)
    enc = jpegamd.Encoder(img.width, img.height)
    cap = jpegamd.max_jfif_bytes(img.width, img.height)
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    size = torch.zeros(1, dtype=torch.int64, device=dev)
    enc.encode_async(jpegamd.Encoder.image(t.data_ptr(), img.width, img.height, img.row_stride, True, jpegamd.ORDER_BGR, 0),
                     out.data_ptr(), cap, size.data_ptr(), True, stream())
    return enc.finish().entropy_bits


def test_no_state_leak_between_gray_and_colour(jpegamd, oracle, dev):
    w, h = 333, 250
    p = synth_rgb(jpegamd, w, h, 21, 0)[:, :, 1].copy()
    rgb = synth_rgb(jpegamd, w, h, 22, 3)
    enc = jpegamd.Encoder(w, h)
    g1 = encode_gray(jpegamd, enc, p, dev, quality=75)
    col, _ = encode_color(jpegamd, enc, rgb, dev, 2, quality=30)
    g2 = encode_gray(jpegamd, enc, p, dev, quality=90)
    assert g1 == oracle.encode_bmp(gray_bmp(p), 75)
    assert g2 == oracle.encode_bmp(gray_bmp(p), 90)
    assert col == cm.color_file(oracle, cm.write_bmp(rgb), 30, 2)


def test_colour_rejects_gray_and_bad_subsampling(jpegamd, dev):
    enc = jpegamd.Encoder(64, 64)
    t = torch.zeros(64 * 64 * 3, dtype=torch.uint8, device=dev)
    out = torch.empty(1 << 16, dtype=torch.uint8, device=dev)
    size = torch.zeros(1, dtype=torch.int64, device=dev)
    for order, sub in ((jpegamd.ORDER_GRAY, 2), (jpegamd.ORDER_RGB, 0), (jpegamd.ORDER_RGB, 3)):
        with pytest.raises(jpegamd.JpegAmdError) as ei:
            enc.encode_color_async(jpegamd.Encoder.image(t.data_ptr(), 64, 64, 192, False, order, 0), sub, out.data_ptr(), 1 << 16,
                                   size.data_ptr(), stream())
        assert ei.value.code == -1


def test_encode_tensor(jpegamd, oracle, dev):
    rgb = synth_rgb(jpegamd, 301, 123, 8, 0)
    t3 = torch.from_numpy(rgb).to(dev)
    assert jpegamd.encode_tensor(t3) == cm.color_file(oracle, cm.write_bmp(rgb), 0, 2)
    assert jpegamd.encode_tensor(t3, quality=90, subsampling=1) == cm.color_file(oracle, cm.write_bmp(rgb), 90, 1)
    big = torch.zeros((123, 320), dtype=torch.uint8, device=dev)           # strided rows: a view into a wider buffer
    big[:, 5:306] = t3[:, :, 0]
    view = big[:, 5:306]
    assert view.stride(0) == 320
    assert jpegamd.encode_tensor(view) == oracle.encode_bmp(gray_bmp(rgb[:, :, 0].copy()))
