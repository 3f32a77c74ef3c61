"""Progressive colour files with end-of-band runs and per-scan optimised tables on the CPU: the model of the file
(tests/progressive_runs_model.py) against recorded sizes, an independent decoder, the one-scan and the standard progressive models, the
size bound, the fixtures of the GPU suite proven on their edges, and the checks of jpegamd.progressive_optimized.  No device is needed."""
from __future__ import annotations

import io
from pathlib import Path

import numpy as np
import pytest

import color_model as cm
import interleaved_model as im
import progressive_model as pm
import progressive_runs_fixtures as fx
import progressive_runs_model as prm
import test_binding_host as tb
from test_binding_host import enc, rec  # noqa: F401  (the recording stand-in for jpegamd.lib, and a context on it)

torch = pytest.importorskip("torch")
image = pytest.importorskip("PIL.Image")
S444, S420, S422 = fx.S444, fx.S420, fx.S422
NAMES = ("jpegamd_encode_color_progressive_optimized_batch_async", "jpegamd_encode_ycbcr_progressive_optimized_batch_async",
         "jpegamd_max_jfif_bytes_progressive_optimized", "jpegamd_debug_progressive_counts")


def _lena():
    with image.open(Path(__file__).parent / "golden" / "assets" / "lena.bmp") as f:
        return np.ascontiguousarray(np.asarray(f.convert("RGB")))


def _sized():
    """(name, rgb, quality, sub, recorded size of the file)"""
    lena = _lena()
    assert lena.shape == (512, 512, 3)
    return [("lena q50 420", lena, 50, S420, 23481), ("lena q50 444", lena, 50, S444, 29954), ("lena q90 420", lena, 90, S420, 65699),
            ("lena q10 420", lena, 10, S420, 7626), ("lena128 q50 420", np.ascontiguousarray(lena[:128, :128]), 50, S420, 1230),
            ("flat 216x152", fx.flat_rgb(216, 152, 90), 50, S444, 644), ("flat 8x8", fx.flat_rgb(8, 8, 128), 50, S444, 432),
            ("flat 7x5", fx.flat_rgb(7, 5, 17), 50, S420, 434)]


def _decode(data: bytes):
    with image.open(io.BytesIO(data)) as f:
        return f.info.get("progressive"), np.asarray(f.convert("RGB"))


def test_recorded_sizes_decoded_pixels_and_the_standard_progressive_file(oracle):
    for name, rgb, q, sub, size in _sized():
        m = cm.memo(prm.rgb_file, oracle, rgb, q, sub)
        assert len(m.file) == size, name
        progressive, got = _decode(m.file)
        _, want = _decode(cm.memo(im.interleaved_file, oracle, rgb, q, sub).file)
        assert progressive == 1 and np.array_equal(got, want), name
        assert len(m.file) < len(cm.memo(pm.progressive_file, oracle, rgb, q, sub).file), name
        h, w, _ = rgb.shape
        assert m.file[:len(prm.head(w, h, q, sub))] == prm.head(w, h, q, sub)
        assert [(t, b, v) for t, b, v in prm.parse_tables(m.file)] == [(prm.table_id(k), list(b), list(v)) for k, (b, v, _) in enumerate(m.tables)]


def test_short_full_segments_appear_in_a_photograph(oracle):
    m = cm.memo(prm.rgb_file, oracle, _lena(), 10, S420)
    full = [b for s in m.seg_bits[1:] for b in s[:-1]]
    assert min(full) == 9 and m.run_hist[256] >= 1             # a FULL segment of 256 empty blocks: EOB8 with a 1-bit code and 8 more bits


@pytest.mark.parametrize("sub", (S444, S420, S422))
def test_bound(jpegamd, oracle, sub):
    j = jpegamd
    for w, h in ((1, 1), (8, 8), (333, 250), (4096, 17)):
        assert j.max_jfif_bytes_progressive_optimized(w, h, sub) == j.max_jfif_bytes_progressive(w, h, sub) + 780
    assert 780 == 2 * (21 + 12) + 6 * (21 + 160 + 1 + 9) - 432
    for bad in ((0, 8, sub), (8, 0, sub), (65536, 8, sub), (8, 8, 0), (8, 8, 3)):
        assert j.max_jfif_bytes_progressive_optimized(*bad) == 0
    for rgb, q in ((np.random.default_rng(5).integers(0, 256, (40, 56, 3), np.uint8), 100), (fx.flat_rgb(8, 8, 128), 50)):
        m = cm.memo(prm.rgb_file, oracle, rgb, q, sub)
        assert len(m.file) <= j.max_jfif_bytes_progressive_optimized(rgb.shape[1], rgb.shape[0], sub)
        assert all(len(v) <= (12 if k < 2 else 170) for k, (_, v, _) in enumerate(m.tables))


def test_flat_fixtures_have_one_symbol_tables_and_the_shortest_segments(oracle):
    for (w, h, value, sub), dc_bits in zip(fx.FLAT, (3, 13)):           # the DC scan: three 1-bit codes; four Y blocks (three of them pad blocks), Cb, Cr
        m = cm.memo(prm.rgb_file, oracle, fx.flat_rgb(w, h, value), 50, sub)
        assert m.seg_bits == ((dc_bits,),) + ((1,),) * 6
        assert all(len(v) == 1 and b[0] == 1 for b, v, _ in m.tables[2:])      # one used symbol: the 1-bit code 0
        assert m.run_hist == {1: 6}
    m = cm.memo(prm.rgb_file, oracle, fx.flat_rgb(*fx.FLAT_513[:3]), 50, fx.FLAT_513[3])
    assert m.seg_bits[1:] == ((9, 9, 2),) * 6 and m.run_hist == {256: 12, 1: 6} and m.cut_runs == 12


def test_edge_fixture_has_every_run_it_claims(oracle):
    m = fx.edge_model(oracle)
    runs = {(r.scan, r.start): r for r in m.runs}
    assert all(len(s) == 2 for s in m.seg_bits[1:])                                # 320 blocks: 256 + 64
    assert {1, 2, 3, 4, 127, 128, 255, 256} <= set(m.run_hist)
    whole = runs[(2, 0)]
    assert whole.length == 256 and whole.cut and (2, 256) in runs                  # blocks 255 and 256 both empty: the run is cut
    lane = runs[(5, 59)]
    assert lane.length == 12 and not lane.starter_empty                            # blocks 59 .. 70: across the lane round, its non-empty starter included
    assert runs[(3, 0)].length == 127 and not runs[(3, 0)].starter_empty
    assert runs[(3, 128)].length == 128 and runs[(3, 128)].behind_nonzero_se
    assert runs[(4, 1)].length == 255 and runs[(4, 1)].behind_nonzero_se and runs[(4, 1)].cut
    assert all(runs[(s, at)].length == n for s in (2, 5) for at, n in ((258, 1), (260, 2), (263, 3), (267, 4)))
    assert min(m.starters) > 0


def test_noise_fixture_has_zrls_and_large_tables(oracle):
    m = cm.memo(prm.rgb_file, oracle, fx.noise_rgb(), 90, S444)
    assert m.zrl > 0 and max(len(v) for _, v, _ in m.tables) > 24 and max(t for _, _, t in m.tables) >= 9


def test_synth_fixtures_have_pad_blocks_and_distinct_headers(oracle):
    """333 x 250 is 42 x 32 blocks, whole MCUs at every subsampling, so the GPU suite also codes 325 x 243 (41 x 31 blocks), where scan 1
    has pad blocks at 4:2:0 and 4:2:2."""
    for (w, h), pads in zip(fx.SYNTH, (False, True)):
        for sub in (S420, S422):
            assert (cm.memo(prm.rgb_file, oracle, cm.synth_rgb(w, h, 100, 0, 0), 50, sub).pad_blocks > 0) == pads
    models = [cm.memo(prm.rgb_file, oracle, r, 50, S420) for r in fx.synth_batch()]
    assert len({m.header_len for m in models}) == 3                                # header lengths differ per picture


# ---- the binding ----------------------------------------------------------------------------------------------------------------------
def test_entry_table_has_the_names(jpegamd):
    for name in NAMES:
        assert getattr(jpegamd.lib, name) is not None
    header = (Path(__file__).resolve().parents[1] / "include" / "jpeg_compression.h").read_text()
    assert all(name + "(" in header for name in NAMES)


def test_encoder_methods_marshal_like_their_twins(jpegamd, enc, rec):
    enc.encode_color_progressive_optimized_batch_async(tb.pictures(jpegamd, jpegamd.Image), tb.SUB, tb.OUTS, tb.CAP, tb.SIZES, tb.STREAM)
    enc.encode_color_progressive_batch_async(tb.pictures(jpegamd, jpegamd.Image), tb.SUB, tb.OUTS, tb.CAP, tb.SIZES, tb.STREAM)
    (n1, a1), (n2, a2) = rec.calls[-2:]
    assert n1 == "jpegamd_encode_color_progressive_optimized_batch_async" and n2 == "jpegamd_encode_color_progressive_batch_async"
    assert len(a1) == len(a2)


def test_c_entries_refuse_before_the_context_is_read(jpegamd):
    import ctypes as C
    import mjpeg_support as ms
    keep, ctx = ms.fake_context()
    j = jpegamd
    outs, sizes = (C.c_void_p * 1)(C.c_void_p(0x1000)), (C.c_void_p * 1)(C.c_void_p(0x2000))

    def pixels(img, sub, count=1):
        return j.lib.jpegamd_encode_color_progressive_optimized_batch_async(ctx, (j.Image * 1)(img), count, sub, outs, 1 << 20, sizes, None)

    good = j.Encoder.image(0x4000, 16, 16, 48, False, j.ORDER_RGB, 50)
    assert pixels(j.Encoder.image(0x4000, 16, 16, 16, False, j.ORDER_GRAY, 50), S420) == -1
    assert [pixels(good, sub) for sub in (0, 3, 5)] == [-1] * 3 and pixels(good, S420, 0) == -1
    ycc = j.Encoder.ycbcr_image(0x4000, 0x5000, 0x6000, 16, 16, 16, 8, j.CHROMA_PLANES, 50)
    for sub, rng, fmt, mat in ((3, 0, 0, 0), (S420, 2, 0, 0), (S420, 0, 3, 0), (S420, 0, 0, 2)):
        assert j.lib.jpegamd_encode_ycbcr_progressive_optimized_batch_async(ctx, (j.YCbCrImage * 1)(ycc), 1, sub, rng, fmt, mat, outs, 1 << 20, sizes,
                                                                            None) == -1
    assert j.lib.jpegamd_debug_progressive_counts(None, 0x1000) == -1
    assert not any(keep)


def test_module_functions_raise_before_any_device_work(jpegamd):
    import jpegamd.progressive as prog
    import jpegamd.progressive_optimized as po
    assert {n for n in dir(po) if n.startswith("encode_")} == {n for n in dir(prog) if n.startswith("encode_")}
    t = torch.zeros((2, 16, 16, 3), dtype=torch.uint8)
    for kw in (dict(t=t, subsampling=0), dict(t=t, subsampling=3), dict(t=t, layout="nope"), dict(t=torch.zeros((2, 16, 16), dtype=torch.uint8)),
               dict(t=torch.zeros((2, 3, 16, 16), dtype=torch.uint8), layout="chw"), dict(t=t)):
        with pytest.raises(ValueError):
            po.encode_tensor_batch(**kw)
    with pytest.raises(ValueError):
        po.encode_tensor(torch.zeros((16, 16), dtype=torch.uint8))
    with pytest.raises(TypeError):
        po.encode_tensor_batch(t, huffman="optimized")
    y, c = torch.zeros((1, 16, 16), dtype=torch.uint8), torch.zeros((1, 8, 8), dtype=torch.uint8)
    for kw in (dict(y=y, cb=c, cr=c, subsampling=3), dict(y=y, cb=c, cr=c, matrix="bt2020"), dict(y=y, cb=c, cr=c)):
        with pytest.raises(ValueError):
            po.encode_ycbcr_batch(**kw)
    with pytest.raises(ValueError):
        po.encode_ycbcr16_batch(y.to(torch.int16), c.to(torch.int16), c.to(torch.int16), align="middle")
    with pytest.raises(ValueError):
        po.encode_yuyv_batch(torch.zeros((1, 16, 16, 2), dtype=torch.uint8))
