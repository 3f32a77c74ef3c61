"""Progressive colour files with successive approximation on the CPU: the model of the file
(tests/progressive_successive_model.py) against an independent decoder and an independent writer of the same scan script, the size
bound, the fixtures of the GPU suite proven on their edges, and the checks of jpegamd.progressive_successive.  No device is needed."""
from __future__ import annotations

import io
from pathlib import Path

import numpy as np
import pytest

import color_model as cm
import interleaved_model as im
import progressive_runs_model as prm
import progressive_successive_fixtures as fx
import progressive_successive_model as psm
import test_binding_host as tb
from test_binding_host import enc, rec  # noqa: F401  (the recording stand-in for jpegamd.lib, and a context on it)

torch = pytest.importorskip("torch")
image = pytest.importorskip("PIL.Image")
S444, S420, S422 = fx.S444, fx.S420, fx.S422
NAMES = ("jpegamd_encode_color_progressive_successive_batch_async", "jpegamd_encode_ycbcr_progressive_successive_batch_async",
         "jpegamd_max_jfif_bytes_progressive_successive", "jpegamd_debug_progressive_successive_counts")


def _decode(data: bytes):
    with image.open(io.BytesIO(data)) as f:
        return f.info.get("progressive"), np.asarray(f.convert("RGB"))


def model(oracle, rgb, q, sub):
    return cm.memo(psm.rgb_file, oracle, rgb, q, sub)


# ---- decoding, the script ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", fx.SUBS)
def test_pillow_decodes_the_model_file_to_the_one_scan_pixels(oracle, sub):
    crop = fx.lena_crop()
    pictures = [(crop, 10), (crop, 50), (crop, 95), (np.ascontiguousarray(crop[:43, :67]), 50), (fx.flat_rgb(7, 5, 17), 50),
                (np.ascontiguousarray(fx.noise_rgb()[:40, :56]), 95)]                 # (67 x 43 -- 9 x 6 blocks --, 7 x 5: pad blocks at 4:2:0 and 4:2:2)
    for rgb, q in pictures:
        m = model(oracle, rgb, q, sub)
        progressive, got = _decode(m.file)
        _, want = _decode(cm.memo(im.interleaved_file, oracle, rgb, q, sub).file)
        assert progressive == 1 and np.array_equal(got, want), (rgb.shape, q, sub)
    assert model(oracle, pictures[3][0], 50, sub).pad_blocks > 0 or sub == S444


def test_the_script_is_the_one_pillow_writes(oracle):
    """An independent check of the ten scans: libjpeg's own script for a YCbCr picture, read back from a file it wrote."""
    buf = io.BytesIO()
    image.fromarray(fx.lena_crop()).save(buf, "JPEG", progressive=True, quality=50)
    theirs = psm.sos_parameters(buf.getvalue())
    ours = psm.sos_parameters(model(oracle, fx.lena_crop(), 50, S420).file)
    assert ours == theirs and len(ours) == psm.SCANS
    assert ours == [(tuple(c + 1 for c in comps), ss, se, ah, al) for comps, ss, se, ah, al, _ in psm.SCRIPT]


def test_headers_and_tables_as_a_reader_finds_them(oracle):
    rgb = fx.lena_crop()
    m = model(oracle, rgb, 50, S420)
    assert m.file[:len(prm.head(128, 128, 50, S420))] == prm.head(128, 128, 50, S420)
    assert prm.parse_tables(m.file) == [(psm.table_id(k), list(b), list(v)) for k, (b, v, _) in enumerate(m.tables)]
    assert [psm.table_id(k) for k in range(psm.TABLES)] == [0x00, 0x01, 0x10, 0x11, 0x11, 0x10, 0x10, 0x11, 0x11, 0x10]
    assert m.header_len[6] == 14                                 # scan 7: its SOS alone
    used = np.nonzero(m.counts[6:].sum(axis=0))[0]
    assert len(used) > 3 and all(s & 15 <= 1 for s in used)      # refinement scans: EOBn, ZRL and symbols of size 1 alone


# ---- what the fixtures exercise ---------------------------------------------------------------------------------------------------------
def test_photograph_crop_has_zrls_with_pending_bits_and_a_block_with_two(oracle):
    m = model(oracle, fx.lena_crop(), 90, S444)
    assert m.zrl_with_bits > 0 and m.multi_zrl_blocks > 0
    assert sum(m.zrl[s - 1] for s in fx.REFINEMENT_SCANS) >= 2


def test_noise_has_b_and_tail_beyond_32_bits(oracle):
    m = model(oracle, fx.noise_rgb(), fx.NOISE_Q, S444)
    assert m.longest_b > 32 and m.longest_tail > 32


def test_edge_fixture_has_every_run_it_claims(oracle):
    m = fx.edge_model(oracle)
    runs = {(r.scan, r.start): r for r in m.runs}
    whole = runs[(6, 0)]                                            # a run over a whole segment whose covered blocks carry correction bits
    assert whole.length == 256 and whole.covered_bits > 0 and whole.cut
    assert any(r.starter_empty and r.behind_new_se and r.scan in fx.REFINEMENT_SCANS for r in m.runs)
    assert any(r.cut for r in m.runs if r.scan in fx.REFINEMENT_SCANS)
    assert m.runs_with_covered_bits > 0 and m.empty_starters > 0 and m.cut_runs > 0


def test_flat_fixtures_have_the_shortest_segments_and_one_symbol_tables(oracle):
    for (w, h, value, sub), blocks in zip(fx.FLAT, (3, 6)):
        m = model(oracle, fx.flat_rgb(w, h, value), 50, sub)
        assert m.seg_bits[6] == (blocks,)                          # the DC refinement scan: one bit per block, pad blocks too
        assert all(m.seg_bits[k] == (1,) for k in range(1, 10) if k != 6)
        assert all(len(m.tables[t][1]) == 1 for t in (6, 7, 8, 9))  # a refinement scan whose table has one symbol, coded once: EOB0
        assert all(m.counts[t].sum() == 1 for t in (6, 7, 8, 9))
    m = model(oracle, fx.flat_rgb(*fx.FLAT_513[:3]), 50, fx.FLAT_513[3])
    assert all(m.seg_bits[k] == (9, 9, 2) for k in range(1, 10) if k != 6)           # FULL segments of 9 bits in first and refinement scans
    assert m.seg_bits[6] == (255,) * 6 + (9,)
    m = model(oracle, fx.flat_rgb(*fx.CHAIN[:3]), 50, fx.CHAIN[3])
    assert all(m.seg_bits[k] == (9,) * 8 + (2,) for k in range(1, 10) if k != 6)


# ---- the bound --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", fx.SUBS)
def test_bound(jpegamd, oracle, sub):
    j = jpegamd
    for bad in ((0, 8, sub), (8, 0, sub), (65536, 8, sub), (8, 8, 0), (8, 8, 3)):
        assert j.max_jfif_bytes_progressive_successive(*bad) == 0
    hs, vs = (1, 1) if sub == S444 else ((2, 2) if sub == S420 else (2, 1))
    for w, h in ((1, 1), (8, 8), (333, 250), (4096, 17)):
        mx, my = -(-((w + 7) // 8) // hs), -(-((h + 7) // 8) // vs)
        blocks = mx * my * (hs * vs + 2)
        assert j.max_jfif_bytes_progressive_successive(w, h, sub) == 640 + 2 * ((blocks * 3824 + 7) // 8 + 1) + 18 + 18 + 8 * 10 + 14 + 1162
    assert 3824 == 27 + 1 + 63 * 26 + 2 * (62 * 17 + 25) and 1162 == 2 * 33 + 8 * 191 - 432
    for seed, (w, h) in enumerate(((56, 40), (67, 43), (8, 8))):
        rgb = np.random.default_rng(5 + seed).integers(0, 256, (h, w, 3), np.uint8)
        m = model(oracle, rgb, 100, sub)
        assert len(m.file) <= j.max_jfif_bytes_progressive_successive(w, h, sub)
        assert all(len(v) <= (12 if k < 2 else 170) for k, (_, v, _) in enumerate(m.tables))


# ---- the binding ------------------------------------------------------------------------------------------------------------------------
def test_entry_table_has_the_names(jpegamd):
    for name in NAMES:
        assert getattr(jpegamd.lib, name) is not None
        assert name in jpegamd.EXPORTED
    header = (Path(__file__).resolve().parents[1] / "include" / "jpeg_compression.h").read_text()
    assert all(name + "(" in header for name in NAMES)


def test_encoder_methods_marshal_like_their_twins(jpegamd, enc, rec):
    enc.encode_color_progressive_successive_batch_async(tb.pictures(jpegamd, jpegamd.Image), tb.SUB, tb.OUTS, tb.CAP, tb.SIZES, tb.STREAM)
    enc.encode_color_progressive_optimized_batch_async(tb.pictures(jpegamd, jpegamd.Image), tb.SUB, tb.OUTS, tb.CAP, tb.SIZES, tb.STREAM)
    (n1, a1), (n2, a2) = rec.calls[-2:]
    assert n1 == "jpegamd_encode_color_progressive_successive_batch_async" and n2 == "jpegamd_encode_color_progressive_optimized_batch_async"
    assert len(a1) == len(a2)
    enc.encode_ycbcr_progressive_successive_batch_async(tb.pictures(jpegamd, jpegamd.YCbCrImage), tb.SUB, 0, 0, 0, tb.OUTS, tb.CAP, tb.SIZES, tb.STREAM)
    enc.encode_ycbcr_progressive_optimized_batch_async(tb.pictures(jpegamd, jpegamd.YCbCrImage), tb.SUB, 0, 0, 0, tb.OUTS, tb.CAP, tb.SIZES, tb.STREAM)
    (n1, a1), (n2, a2) = rec.calls[-2:]
    assert n1 == "jpegamd_encode_ycbcr_progressive_successive_batch_async" and len(a1) == len(a2)
    assert "encode_color_progressive_successive_batch_async" in vars(jpegamd._ProgressiveEntries)


def test_c_entries_refuse_before_the_context_is_read(jpegamd):
    import ctypes as C
    import mjpeg_support as ms
    keep, ctx = ms.fake_context()
    j = jpegamd
    outs, sizes = (C.c_void_p * 1)(C.c_void_p(0x1000)), (C.c_void_p * 1)(C.c_void_p(0x2000))

    def pixels(img, sub, count=1):
        return j.lib.jpegamd_encode_color_progressive_successive_batch_async(ctx, (j.Image * 1)(img), count, sub, outs, 1 << 20, sizes, None)

    good = j.Encoder.image(0x4000, 16, 16, 48, False, j.ORDER_RGB, 50)
    assert pixels(j.Encoder.image(0x4000, 16, 16, 16, False, j.ORDER_GRAY, 50), S420) == -1
    assert [pixels(good, sub) for sub in (0, 3, 5)] == [-1] * 3 and pixels(good, S420, 0) == -1
    ycc = j.Encoder.ycbcr_image(0x4000, 0x5000, 0x6000, 16, 16, 16, 8, j.CHROMA_PLANES, 50)
    for sub, rng, fmt, mat in ((3, 0, 0, 0), (S420, 2, 0, 0), (S420, 0, 3, 0), (S420, 0, 0, 2)):
        assert j.lib.jpegamd_encode_ycbcr_progressive_successive_batch_async(ctx, (j.YCbCrImage * 1)(ycc), 1, sub, rng, fmt, mat, outs, 1 << 20, sizes,
                                                                             None) == -1
    assert j.lib.jpegamd_debug_progressive_successive_counts(None, 0x1000) == -1
    assert not any(keep)


def test_module_functions_raise_before_any_device_work(jpegamd):
    import jpegamd.progressive_optimized as po
    import jpegamd.progressive_successive as ps
    assert {n for n in dir(ps) if n.startswith("encode_")} == {n for n in dir(po) if n.startswith("encode_")}
    t = torch.zeros((2, 16, 16, 3), dtype=torch.uint8)
    for kw in (dict(t=t, subsampling=0), dict(t=t, subsampling=3), dict(t=t, layout="nope"), dict(t=torch.zeros((2, 16, 16), dtype=torch.uint8)),
               dict(t=torch.zeros((2, 3, 16, 16), dtype=torch.uint8), layout="chw"), dict(t=t)):
        with pytest.raises(ValueError):
            ps.encode_tensor_batch(**kw)
    with pytest.raises(ValueError):
        ps.encode_tensor(torch.zeros((16, 16), dtype=torch.uint8))
    with pytest.raises(TypeError):
        ps.encode_tensor_batch(t, huffman="optimized")
    y, c = torch.zeros((1, 16, 16), dtype=torch.uint8), torch.zeros((1, 8, 8), dtype=torch.uint8)
    for kw in (dict(y=y, cb=c, cr=c, subsampling=3), dict(y=y, cb=c, cr=c, matrix="bt2020"), dict(y=y, cb=c, cr=c)):
        with pytest.raises(ValueError):
            ps.encode_ycbcr_batch(**kw)
    with pytest.raises(ValueError):
        ps.encode_ycbcr16_batch(y.to(torch.int16), c.to(torch.int16), c.to(torch.int16), align="middle")
    with pytest.raises(ValueError):
        ps.encode_yuyv_batch(torch.zeros((1, 16, 16, 2), dtype=torch.uint8))
