"""Grayscale files with restart intervals and optimised Huffman tables on the CPU: tests/gray_scan_model.py against
the oracle's grayscale file and an independent decoder, proof that every picture of tests/gray_scan_fixtures.py has the property its GPU
case claims, the exported symbols, the bound, and the refusals that need no device."""
from __future__ import annotations

import ctypes as C
import io

import numpy as np
import pytest

import color_model as cm
import gray_scan_fixtures as gf
import gray_scan_model as gm
import mjpeg_support as ms
import scan_model as sm

ERR_ARG, ERR_TOO_LARGE = -1, -5
NAMES = ("jpegamd_encode_gray_scan_batch_async", "jpegamd_max_jfif_bytes_gray_scan")


def _decode(data: bytes) -> np.ndarray:
    image = pytest.importorskip("PIL.Image")
    with image.open(io.BytesIO(data)) as f:
        assert f.mode == "L"
        return np.asarray(f)


@pytest.fixture(scope="module")
def shapes():
    return gf.shapes()


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def test_model_without_intervals_is_the_oracles_file(oracle, shapes):
    for name, p, q in shapes:
        ref = cm.gray_file(oracle, p, q)
        assert ref[:328] == gm.std_prefix(p.shape[1], p.shape[0], q), name
        m = gf.model(oracle, p, q)
        assert m.file == ref, name
        assert m.blocks == gm.block_count(p.shape[1], p.shape[0]) and m.intervals == 1 and m.markers == 0 and m.prefix_len == 328


def test_model_with_one_interval_is_that_file_with_dri(oracle, shapes):
    for name, p, q in shapes:
        ref = cm.gray_file(oracle, p, q)
        blocks = gm.block_count(p.shape[1], p.shape[0])
        for ri in sorted({blocks, blocks + 1, 65535}):
            m = gf.model(oracle, p, q, ri)
            assert m.file == gm.with_dri(ref, ri) and m.intervals == 1, (name, ri)
            assert gf.model(oracle, p, q, ri, True).file == gm.with_dri(gf.model(oracle, p, q, 0, True).file, ri), (name, ri)


def test_every_variant_decodes_to_the_reference_pixels(oracle, shapes):
    for name, p, q in shapes:
        h, w = p.shape
        want = _decode(cm.gray_file(oracle, p, q))
        assert want.shape == (h, w)
        blocks = gm.block_count(w, h)
        for ri in gf.INTERVALS:
            ri = gf.interval(ri, w)
            for opt in gf.MODES:
                m = gf.model(oracle, p, q, ri, opt)
                assert np.array_equal(_decode(m.file), want), (name, ri, opt)
                markers, stuffed = sm.walk_scan(m.file, gm.SOS1)
                n = -(-blocks // ri) if ri else 1
                assert markers == [i % 8 for i in range(n - 1)] and stuffed == m.stuffed, (name, ri, opt)
                assert m.intervals == n and m.markers == n - 1
                if opt:
                    std = gf.model(oracle, p, q, ri, False)
                    assert len(m.file) <= len(std.file) and m.scan_bits <= std.scan_bits, (name, ri)
                    assert m.counts.sum() == std.counts.sum() and np.array_equal(m.counts, std.counts)
    assert max(-(-gm.block_count(p.shape[1], p.shape[0]) // gf.interval("row", p.shape[1])) for _, p, _ in shapes) > 8      # RSTn wraps


def test_dc_counts_depend_on_the_interval(oracle, shapes):
    p, q = next((p, q) for name, p, q in shapes if name == "72x40")
    a, b = gf.model(oracle, p, q, 0, True), gf.model(oracle, p, q, 1, True)
    assert not np.array_equal(a.counts[0], b.counts[0]) and np.array_equal(a.counts[1], b.counts[1])
    assert a.counts[0].sum() == b.counts[0].sum() == a.blocks


# ---- the fixtures -----------------------------------------------------------------------------------------------------------------------
def test_noise_fixtures_have_ff_pads_and_aligned_intervals(oracle, shapes):
    by_name = {name: (p, q) for name, p, q in shapes}
    for name, ri in gf.PAD_FF:
        for opt in gf.MODES:
            m = gf.model(oracle, *by_name[name], ri, opt)
            assert m.pad_ff >= 1 and m.aligned >= 1, (name, opt)


def test_straddle_fixture(oracle):
    p, q = gf.straddle()
    for opt in gf.MODES:
        m = gf.model(oracle, p, q, 0, opt)
        assert m.intervals == 1 and len(m.segment_bits[0]) == 3       # 256 + 256 + 1 blocks
        assert m.straddle_ff >= 1 and all(1 <= ph <= 7 for ph in m.straddle_phases), opt


def test_borrowed_tail_fixtures(oracle):
    p, q = gf.tail_standard()
    m = gf.model(oracle, p, q, 257, False)
    assert m.intervals == 3 and all(len(s) == 2 and s[1] == 6 for s in m.segment_bits) and m.borrowed_tails >= 1
    m = gf.model(oracle, np.ascontiguousarray(p[:, :2056]), q, 0, False)
    assert m.segment_bits[0][1] == 6 and m.borrowed_tails == 1 and m.min_segment_bits == 6
    for blocks, ri in ((257, 0), (771, 257)):
        p, q = gf.tail_optimized(blocks)
        m = gf.model(oracle, p, q, ri, True)
        assert all(s == (516, 2) for s in m.segment_bits) and m.borrowed_tails == len(m.segment_bits) == (3 if ri else 1)


def test_multi_round_fixture(oracle, shapes):
    p, q = next((p, q) for name, p, q in shapes if name == gf.MULTI_ROUND)
    for opt in gf.MODES:
        for ri in (0, 256, 65535):
            assert gf.model(oracle, p, q, ri, opt).max_segment_bits > 65536


def test_flat_fixtures_have_single_symbol_tables_and_the_shortest_segments(oracle):
    for w, h in gf.FLAT:
        for ri in gf.FLAT_INTERVALS:
            for opt in gf.MODES:
                m = gf.model(oracle, gf.flat(w, h), 50, ri, opt)
                per = 2 if opt else 6
                assert m.scan_bits == per * m.blocks
                if opt:
                    assert [(t[0], t[1]) for t in m.tables] == [([1] + [0] * 15, [0])] * 2
                assert all(b % per == 0 for s in m.segment_bits for b in s)
    assert gf.model(oracle, gf.flat(24, 8), 50, 1, False).min_segment_bits == 6
    assert gf.model(oracle, gf.flat(24, 8), 50, 1, True).min_segment_bits == 2
    m = gf.model(oracle, gf.flat(2056, 8), 50, 0, True)
    assert m.segment_bits == ((512, 2),) and m.min_segment_bits == 2         # the 257th block alone
    assert gf.model(oracle, gf.flat(2056, 8), 50, 0, False).segment_bits == ((1536, 6),)


def test_step_fixtures_have_segments_of_two_to_five_bits(oracle):
    seen = set()
    for p in gf.STEPS:
        m = gf.model(oracle, p, 50, 1, True)
        seen |= {b for s in m.segment_bits for b in s}
    assert seen == {2, 3, 4, 5}


def test_long_code_fixtures_exceed_16(oracle):
    tops = [gf.model(oracle, gf.long_code_plane(w, h, kind, seed), q, 0, True).tables[1][2] for w, h, kind, seed, q in gf.LONG_CODES]
    assert max(tops) > 16


def test_batch_of_three_has_three_table_pairs_and_prefix_lengths(oracle):
    models = [gf.model(oracle, p, 75, 5, True) for p in gf.batch_of_three()]
    assert len({m.prefix_len for m in models}) == 3 and len({repr(m.tables) for m in models}) == 3


# ---- the C surface ------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_documented(jpegamd):
    header = jpegamd.HEADER_PATH.read_text()
    lib = C.CDLL(str(jpegamd.LIB_PATH))
    for name in NAMES:
        assert name in jpegamd.EXPORTED and hasattr(lib, name) and name in header, name
    assert hasattr(jpegamd.Encoder, "encode_gray_scan_batch_async") and hasattr(jpegamd, "max_jfif_bytes_gray_scan")
    import jpegamd.mjpeg as mj
    assert hasattr(mj, "encode_gray_batch") and hasattr(mj, "encode_gray")


def _call(jpegamd, ctx, imgs, ri=0, count=None, outs=True, sizes=True):
    arr = (jpegamd.Image * max(len(imgs), 1))(*imgs) if imgs is not None else None
    out_arr, size_arr = ms.out_arrays()
    return jpegamd.lib.jpegamd_encode_gray_scan_batch_async(ctx, arr, len(imgs) if count is None else count, ri, out_arr if outs else None,
                                                           1 << 20, size_arr if sizes else None, None)


def test_entry_refuses_bad_arguments_without_a_device(jpegamd):
    keep, ctx = ms.fake_context()
    img = lambda **kw: jpegamd.Encoder.image(kw.get("ptr", 0x1000), kw.get("w", 16), kw.get("h", 16), kw.get("stride", 16), False,
                                             kw.get("order", jpegamd.ORDER_GRAY), 50)
    good = [img(), img()]
    for ri in (0, 1, 65535):                                          # well-formed: the zeroed context holds no picture at all
        assert _call(jpegamd, ctx, good, ri=ri) == ERR_TOO_LARGE, ri
    huge = [img(w=65535, h=65535, stride=65535)]                      # ... nor the path's budget this one's scratch at Ri = 1
    assert _call(jpegamd, ctx, huge, ri=1) == ERR_TOO_LARGE
    assert _call(jpegamd, None, good) == ERR_ARG
    assert _call(jpegamd, ctx, None, count=2) == ERR_ARG
    assert _call(jpegamd, ctx, good, outs=False) == ERR_ARG and _call(jpegamd, ctx, good, sizes=False) == ERR_ARG
    for count in (0, -1, 33):
        assert _call(jpegamd, ctx, [img()] * 4, count=count) == ERR_ARG, count
    for ri in (-1, 65536, 1 << 20):
        assert _call(jpegamd, ctx, good, ri=ri) == ERR_ARG, ri
    for order in (5, -1, 0x100):
        assert _call(jpegamd, ctx, [img(order=order)] * 2) == ERR_ARG, order
    assert _call(jpegamd, ctx, [img(ptr=0)]) == ERR_ARG
    assert _call(jpegamd, ctx, [img(w=0)]) == ERR_ARG and _call(jpegamd, ctx, [img(h=70000)]) == ERR_ARG
    assert _call(jpegamd, ctx, [img(stride=15)]) == ERR_ARG
    assert _call(jpegamd, ctx, [img(order=jpegamd.ORDER_RGBA, stride=63)]) == ERR_ARG
    for other in (img(w=15), img(h=8), img(stride=32), img(order=jpegamd.ORDER_RGB, stride=48)):       # mixed geometry in a batch
        assert _call(jpegamd, ctx, [img(), other], ri=1) == ERR_ARG


def test_bound(jpegamd):
    bound = jpegamd.max_jfif_bytes_gray_scan
    for args in ((0, 8, 0), (8, 0, 0), (-1, 8, 0), (65536, 8, 0), (8, 65536, 0), (8, 8, -1), (8, 8, 65536)):
        assert bound(*args) == 0, args
    for w, h in ((1, 1), (9, 9), (2056, 8), (65535, 65535)):
        m = gm.block_count(w, h)
        plain = 328 + 2 * ((m * 1723 + 7) // 8 + 1) + 2 + 16
        assert bound(w, h, 0) == plain
        for ri in (1, 7, 256, 65535):
            assert bound(w, h, ri) == plain + 6 + 4 * (-(-m // ri) - 1), (w, h, ri)
    assert 27 + 63 * 26 <= 1723


def test_model_files_fit_the_bound(jpegamd, oracle, shapes):
    for name, p, q in shapes:
        for ri in (0, 1):
            for opt in gf.MODES:
                assert len(gf.model(oracle, p, q, ri, opt).file) <= jpegamd.max_jfif_bytes_gray_scan(p.shape[1], p.shape[0], ri)


def test_python_functions_refuse_bad_values_on_the_cpu(jpegamd):
    torch = pytest.importorskip("torch")
    import jpegamd.mjpeg as mj
    t = torch.zeros(2, 16, 24, dtype=torch.uint8)
    calls = {"batch": lambda x=t, **kw: mj.encode_gray_batch(x, **kw), "one": lambda x=t[0], **kw: mj.encode_gray(x, **kw)}
    for name, call in calls.items():
        for bad in (-1, 65536, "rows", 1.5, True):
            with pytest.raises(ValueError, match="restart_interval") as err:
                call(restart_interval=bad)
            assert "device tensor" not in str(err.value), (name, bad)
        for bad in ("optimised", "", None, 1):
            with pytest.raises(ValueError, match="huffman must be"):
                call(huffman=bad)
        for good in (dict(), dict(restart_interval="row", huffman="optimized"), dict(restart_interval=0), dict(restart_interval=65535)):
            with pytest.raises(ValueError, match="device tensor"):      # well-formed calls only lack a device
                call(**good)
    for bad in (t.to(torch.int16), t.float(), torch.zeros(2, 16, 24, 3, dtype=torch.uint8), torch.zeros(16, dtype=torch.uint8), t.transpose(1, 2),
                torch.zeros(2, 0, 24, dtype=torch.uint8), "x"):
        with pytest.raises(ValueError) as err:
            mj.encode_gray_batch(bad)
        assert "device tensor" not in str(err.value)
    for bad in (t, torch.zeros(16, dtype=torch.uint8), t[0].to(torch.int32)):
        with pytest.raises(ValueError) as err:
            mj.encode_gray(bad)
        assert "device tensor" not in str(err.value)
    with pytest.raises(ValueError, match="device tensor"):              # rows apart by a stride are fine
        mj.encode_gray_batch(torch.zeros(2, 16, 32, dtype=torch.uint8)[:, :, :24])
