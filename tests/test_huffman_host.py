"""Per-picture optimised Huffman tables of the one-scan colour files on the CPU: the table construction of
tests/huffman_model.py against the tables an independent encoder (PIL / libjpeg) makes of the same counts, its properties on random
and Fibonacci-like counts, the model's files against an independent decoder, proof that every picture of tests/huffman_fixtures.py sits
on the edge its GPU case claims, the exported symbols, and the refusals that need no device."""
from __future__ import annotations

import ctypes as C
import io

import numpy as np
import pytest

import color_model as cm
import huffman_fixtures as hf
import huffman_model as hm
import interleaved_model as im
import mjpeg_support as ms
import restart_model as rm
import scan_model as sm
from huffman_fixtures import S420, S422, S444, SUBS

ERR_ARG = -1
NAMES = ("jpegamd_encoder_set_huffman", "jpegamd_debug_optimal_huffman", "jpegamd_debug_huffman_counts")


def _decode(data: bytes) -> np.ndarray:
    image = pytest.importorskip("PIL.Image")
    with image.open(io.BytesIO(data)) as f:
        return np.asarray(f.convert("RGB"))


# ---- the construction -------------------------------------------------------------------------------------------------------------------
# (w, h, synth kind, seed, quality, PIL subsampling): the last two are noise at 4:2:0 whose AC tables merge to lengths beyond 16
PIL_CASES = [(64, 48, 0, 3, 50, 0), (200, 120, 0, 3, 75, 0), (200, 120, 1, 4, 90, 2), (61, 45, 0, 5, 95, 2), (384, 288, 1, 1, 90, 2),
             (384, 288, 1, 1, 97, 2)]


def test_builder_makes_pils_tables_of_pils_counts():
    """PIL writes files with optimize=True; their scans are decoded into symbol counts with the files' own tables; the construction on
    those counts must give the files' BITS and HUFFVAL."""
    image = pytest.importorskip("PIL.Image")
    deepest = 0
    for w, h, kind, seed, q, ss in PIL_CASES:
        buf = io.BytesIO()
        image.fromarray(hf.synth_rgb(w, h, seed, kind)).save(buf, "JPEG", quality=q, optimize=True, subsampling=ss)
        data = buf.getvalue()
        tabs = hm.parse_dht(data)
        assert sorted(tabs) == sorted(hm.TABLE_IDS)
        for counts, t in zip(hm.scan_symbol_counts(data), hm.TABLE_IDS):
            bits, vals, top = hm.optimal_table(counts)
            assert (bits, vals) == tabs[t], (w, h, q, ss, hex(t))
            deepest = max(deepest, top)
    assert deepest > 16


def test_properties_on_random_and_fibonacci_counts():
    tables = hf.count_tables()
    assert max(hm.code_sizes(tables[0])) >= 40 and max(hm.code_sizes(tables[1])) >= 59        # the merge's chains are that deep
    for f in tables:
        bits, vals, top = hm.optimal_table(f)
        used = [s for s in range(256) if f[s]]
        assert sorted(vals) == used and len(set(vals)) == len(vals)          # HUFFVAL: exactly the symbols with non-zero counts
        assert len(bits) == 16 and sum(bits) == len(vals)                    # all lengths <= 16
        if not used:
            assert bits == [0] * 16
            continue
        kraft = sum(n << (16 - l) for l, n in enumerate(bits, 1))
        longest = max(l for l, n in enumerate(bits, 1) if n)
        assert kraft + (1 << (16 - longest)) <= 1 << 16                      # room for the reserved point at the longest length
        codes = cm.canonical(bits, vals)
        assert all(c != (1 << ln) - 1 for c, ln in codes.values())          # no code word is all ones
        lengths = [codes[s][1] for s in vals]
        assert lengths == sorted(lengths)
        if len(used) == 1:
            assert codes[used[0]] == (0, 1)                                  # one used symbol: the 1-bit code 0
    # the counts of a symbol do not move a rarer symbol in front of it
    f = hf.fibonacci_counts(40)
    codes = cm.canonical(*hm.optimal_table(f)[:2])
    order = sorted((s for s in range(256) if f[s]), key=lambda s: -int(f[s]))
    assert all(codes[a][1] <= codes[b][1] for a, b in zip(order, order[1:]))


# ---- the model's files ------------------------------------------------------------------------------------------------------------------
def _fixture_files(oracle):
    """(name, optimised model, standard model file) of every RGB picture the GPU suite encodes."""
    for w, h, kind, q in hf.CONTENT:
        rgb = hf.content_rgb(w, h, kind)
        for sub in SUBS:
            for ri in hf.INTERVALS:
                r = hf.interval(ri, w, sub)
                yield f"content-{w}x{h}-{kind}-{sub}-{ri}", hf.model(oracle, rgb, q, sub, r), hm.standard_file(oracle, rgb, q, sub, r)
    for w, h, sub in hf.FLAT:
        for ri in hf.FLAT_INTERVALS:
            yield f"flat-{w}x{h}-{sub}-{ri}", hf.model(oracle, hf.flat(w, h), 50, sub, ri), hm.standard_file(oracle, hf.flat(w, h), 50, sub, ri)
    for w, h, kind, seed, q in hf.LONG_CODES:
        rgb = hf.synth_rgb(w, h, seed, kind)
        yield f"long-{kind}", hf.model(oracle, rgb, q, S420, 0), hm.standard_file(oracle, rgb, q, S420, 0)


def _standard_planes_file(oracle, planes, q, sub, ri):
    return ms.ycc_model(oracle, planes, q, sub, ri).file


def test_model_files_decode_to_the_standard_files_pixels_and_are_smaller(jpegamd, oracle):
    n = 0
    for name, m, std in _fixture_files(oracle):
        assert len(m.file) < len(std), name
        assert np.array_equal(_decode(m.file), _decode(std)), name
        at = m.file.index(im.SOS3)
        assert at + len(im.SOS3) == m.prefix_len <= std.index(im.SOS3) + len(im.SOS3), name      # never longer than the standard prefix
        n += 1
    assert n == len(hf.CONTENT) * 3 * 4 + len(hf.FLAT) * 3 + 2
    for case in (hf.BORROWED, hf.AGAINST_FF):
        for ri in (0, 86):
            planes = hf.short_tail_planes(case, ri)
            m = hf.planes_model(oracle, planes, case["quality"], S444, ri)
            std = _standard_planes_file(oracle, planes, case["quality"], S444, ri)
            assert len(m.file) < len(std) and np.array_equal(_decode(m.file), _decode(std))


def test_optimised_file_differs_from_the_standard_one_in_dht_and_scan_alone(jpegamd, oracle):
    rgb = hf.content_rgb(200, 120, 0)
    for sub in SUBS:
        for ri in (0, 5):
            m, std = hf.model(oracle, rgb, 75, sub, ri), hm.standard_file(oracle, rgb, 75, sub, ri)
            tail = len(im.SOS3) + (6 if ri else 0)
            head = std.index(b"\xff\xc4")
            assert m.file[:head] == std[:head]
            s_at = std.index(im.SOS3) + len(im.SOS3)
            assert m.file[m.prefix_len - tail:m.prefix_len] == std[s_at - tail:s_at]
            assert sm.walk_scan(m.file, im.SOS3)[0] == sm.walk_scan(std, im.SOS3)[0] and sm.walk_scan(m.file, im.SOS3)[1] == m.stuffed
            assert len(m.file) <= (jpegamd.max_jfif_bytes_interleaved_restart(200, 120, sub, ri))
    # the counts depend on the interval: a DC difference against 0 at every interval's start
    a, b = hf.model(oracle, rgb, 75, S420, 0), hf.model(oracle, rgb, 75, S420, 1)
    assert not np.array_equal(a.counts[0], b.counts[0]) and np.array_equal(a.counts[1], b.counts[1])
    assert a.counts[0].sum() == b.counts[0].sum() == 4 * 13 * 8 and a.pad_blocks > 0


# ---- every fixture sits on its edge -----------------------------------------------------------------------------------------------------
def test_content_fixtures_have_pad_blocks_and_distinct_tables(jpegamd, oracle):
    for w, h, kind, q in hf.CONTENT:
        rgb = hf.content_rgb(w, h, kind)
        for sub in (S420, S422):
            assert hf.model(oracle, rgb, q, sub, 0).pad_blocks > 0, (w, h, sub)
        for sub in SUBS:
            per_interval = {repr(hf.model(oracle, rgb, q, sub, hf.interval(ri, w, sub)).tables) for ri in hf.INTERVALS}
            assert len(per_interval) > 1                               # the tables follow the interval
    for sub in SUBS:
        for ri in (0, 5):
            models = [hf.model(oracle, r, 75, sub, ri) for r in hf.batch_of_three()]
            assert len({m.prefix_len for m in models}) == 3 and len({repr(m.tables) for m in models}) == 3


def test_flat_fixtures_have_single_symbol_tables_and_the_shortest_segments(oracle):
    bits_per_mcu = {S444: 6, S422: 8, S420: 12}                       # two 1-bit symbols a block
    for w, h, sub in hf.FLAT:
        _, _, _, _, mx, my = im.geometry(w, h, sub)
        mcus, s = mx * my, rm.seg_mcus(sub)
        for ri in hf.FLAT_INTERVALS:
            m = hf.model(oracle, hf.flat(w, h), 50, sub, ri)
            assert [(t[0], t[1]) for t in m.tables] == [([1] + [0] * 15, [0])] * 4
            assert m.scan_bits == bits_per_mcu[sub] * mcus
            shortest = min(ri, mcus - (m.intervals - 1) * ri) if ri else (mcus - 1) % s + 1       # MCUs of the shortest coder segment
            assert ri < s and m.min_segment_bits == bits_per_mcu[sub] * shortest
    assert hf.model(oracle, hf.flat(688, 8), 50, S444, 5).min_segment_bits == 6 == hf.model(oracle, hf.flat(688, 8), 50, S444, 1).min_segment_bits
    m = hf.model(oracle, hf.flat(688, 8), 50, S444, 0)
    assert m.segment_bits == ((85 * 6, 6),)                               # the scan's last segment: one MCU of 6 bits


def test_short_tail_fixtures(oracle):
    for ri in (0, 86):
        m = hf.planes_model(oracle, hf.short_tail_planes(hf.BORROWED, ri), hf.BORROWED["quality"], S444, ri)
        first = m.segment_bits[0]
        assert len(first) == 2 and first[1] == 6 and (first[0] + first[1]) % 8 == 7 > first[1]
        assert m.borrowed_tails >= 1 and m.intervals == (3 if ri else 1)
        m = hf.planes_model(oracle, hf.short_tail_planes(hf.AGAINST_FF, ri), hf.AGAINST_FF["quality"], S444, ri)
        first = m.segment_bits[0]
        assert len(first) == 2 and first[1] == 13 < 14 and first[0] % 8 == 5
        assert m.short_against_ff == 1 and m.stuffed >= 1
        luma_dc = cm.canonical(*m.tables[0][:2])
        assert luma_dc[4] == (0b1110, 4)                                 # the last MCU begins 1110: three 1-bits complete the byte
        assert 0xE5 in m.tables[3][1]                                    # (run 14, size 5): coefficient 63 of the Cr block = 31
    # at 4:2:2 and 4:2:0 an MCU is never shorter than 8 bits: no tail there can borrow
    assert hf.model(oracle, hf.flat(24, 24), 50, S422, 1).min_segment_bits == 8
    assert hf.model(oracle, hf.flat(24, 24), 50, S420, 1).min_segment_bits == 12


def test_long_code_fixtures_exceed_16(oracle):
    tops = [[t[2] for t in hf.model(oracle, hf.synth_rgb(w, h, seed, kind), q, S420, 0).tables] for w, h, kind, seed, q in hf.LONG_CODES]
    assert tops[0][1] > 16 and tops[0][3] > 16 and tops[1][1] > 16


# ---- the C surface ------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_documented(jpegamd):
    header = jpegamd.HEADER_PATH.read_text()
    lib = C.CDLL(str(jpegamd.LIB_PATH))
    for name in NAMES:
        assert name in jpegamd.EXPORTED and hasattr(lib, name) and name in header, name
    for text in ("#define JPEGAMD_HUFFMAN_STANDARD  0", "#define JPEGAMD_HUFFMAN_OPTIMIZED 1", "are a follow-up", "27 + 63 x 26"):
        assert text in header, text
    assert hasattr(jpegamd.Encoder, "set_huffman") and (jpegamd.HUFFMAN_STANDARD, jpegamd.HUFFMAN_OPTIMIZED) == (0, 1)


def test_entries_refuse_bad_arguments_without_a_device(jpegamd):
    keep, ctx = ms.fake_context()
    lib = jpegamd.lib
    assert lib.jpegamd_encoder_set_huffman(None, 0) == ERR_ARG and lib.jpegamd_encoder_set_huffman(None, 1) == ERR_ARG
    for bad in (-1, 2, 3, 1 << 20):
        assert lib.jpegamd_encoder_set_huffman(ctx, bad) == ERR_ARG, bad
    freq = np.ones((2, 256), np.uint64)
    bits, vals, nvals = np.zeros((2, 16), np.uint8), np.zeros((2, 256), np.uint8), np.zeros(2, np.int32)
    p = [freq.ctypes.data, 2, bits.ctypes.data, vals.ctypes.data, nvals.ctypes.data]
    assert lib.jpegamd_debug_optimal_huffman(None, *p) == ERR_ARG
    for k in (0, 2, 3, 4):
        q = list(p)
        q[k] = 0
        assert lib.jpegamd_debug_optimal_huffman(ctx, *q) == ERR_ARG, k
    for n in (-1, 4097):
        assert lib.jpegamd_debug_optimal_huffman(ctx, p[0], n, *p[2:]) == ERR_ARG
    freq[1, 7] = 1 << 54                                              # a count the merge key cannot hold
    assert lib.jpegamd_debug_optimal_huffman(ctx, *p) == ERR_ARG
    freq[1, 7] = (1 << 54) - 255                                      # ... and a sum it cannot hold
    assert lib.jpegamd_debug_optimal_huffman(ctx, *p) == ERR_ARG
    counts = np.zeros((1, 4, 256), np.uint64)
    assert lib.jpegamd_debug_huffman_counts(None, counts.ctypes.data) == ERR_ARG
    assert lib.jpegamd_debug_huffman_counts(ctx, None) == ERR_ARG
    assert lib.jpegamd_debug_huffman_counts(ctx, counts.ctypes.data) == ERR_ARG        # a context that made no optimised call


def test_python_functions_refuse_an_unknown_huffman_on_the_cpu(jpegamd):
    torch = pytest.importorskip("torch")
    import jpegamd.mjpeg as mj
    u8 = torch.uint8
    hwc = torch.zeros(2, 8, 8, 3, dtype=u8)
    y, cb, cr = torch.zeros(2, 8, 8, dtype=u8), torch.zeros(2, 4, 4, dtype=u8), torch.zeros(2, 4, 4, dtype=u8)
    y16, c16 = torch.zeros(2, 8, 8, dtype=torch.int16), torch.zeros(2, 4, 4, dtype=torch.int16)
    yuyv = torch.zeros(2, 8, 8, 2, dtype=u8)
    calls = {"tensor": lambda **kw: mj.encode_tensor(hwc[0], **kw), "tensor_batch": lambda **kw: mj.encode_tensor_batch(hwc, **kw),
             "ycbcr": lambda **kw: mj.encode_ycbcr_batch(y, cb, cr, **kw), "ycbcr16": lambda **kw: mj.encode_ycbcr16_batch(y16, c16, c16, **kw),
             "yuyv": lambda **kw: mj.encode_yuyv_batch(yuyv, **kw)}
    for name, call in calls.items():
        for bad in ("optimised", "OPTIMIZED", "", None, 1, True):
            with pytest.raises(ValueError, match="huffman must be") as err:
                call(huffman=bad)
            assert "device tensor" not in str(err.value), (name, bad)
        for good in ("standard", "optimized"):                           # well-formed calls only lack a device
            with pytest.raises(ValueError, match="device tensor"):
                call(huffman=good)
    with pytest.raises(ValueError, match="interleaved"):
        jpegamd.encode_tensor_batch(hwc, _huffman=1)
