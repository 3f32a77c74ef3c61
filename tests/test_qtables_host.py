"""Caller-supplied quantisation tables on the CPU: the C-ABI surface, the fast quantiser's constants for tables outside
the quality family, the model of tests/qtables_model.py anchored on the quality-driven models, and the Python helpers.  No compute calls
are made here."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import color_model as cm
import color_model_422 as m422
import interleaved_model as im
import qtables_fixtures as qx
import qtables_model as qtm
import restart_model as rm
import scan_model as sm
from conftest import ROOT

f32, f64 = np.float32, np.float64
NEW = ("jpegamd_quant_tables_for_quality", "jpegamd_encoder_set_quant_tables", "jpegamd_encoder_get_quant_tables",
       "jpegamd_debug_table_consts")
SUBS = (sm.SUB_444, sm.SUB_420, sm.SUB_422)
ALL_TABLES = dict(qx.SINGLES, **{f"random_dense{s}": qx.RANDOM(100 + s) for s in range(25)},
                  **{f"random_sparse{s}": qx.sparse_random(200 + s) for s in range(25)})


@pytest.fixture(scope="module")
def rgbs():
    return {(72, 40): cm.synth_rgb(72, 40, 11, 0), (9, 9): cm.synth_rgb(9, 9, 12, 1)}


# ---- 1. the surface ---------------------------------------------------------------------------------------------------------------------
def test_symbols_and_tables_of_a_quality(jpegamd):
    header = jpegamd.HEADER_PATH.read_text()
    raw = C.CDLL(str(jpegamd.LIB_PATH))
    for name in NEW:
        assert name in jpegamd.EXPORTED and hasattr(raw, name) and name in header, name
    for q in (0, 1, 10, 50, 90, 100):
        luma, chroma = jpegamd.quant_tables_for_quality(q)
        assert np.array_equal(luma, jpegamd.quant_table(q)) and np.array_equal(chroma, jpegamd.chroma_quant_table(q)), q
        assert luma.dtype == chroma.dtype == np.uint8 and luma.shape == chroma.shape == (64,)
    only = np.zeros(64, np.uint8)
    assert jpegamd.lib.jpegamd_quant_tables_for_quality(90, None, only.ctypes.data) == 0      # either pointer may be NULL
    assert np.array_equal(only, jpegamd.chroma_quant_table(90))
    assert jpegamd.lib.jpegamd_quant_tables_for_quality(90, None, None) == 0


def test_the_debug_entry_refuses_a_zero_entry_and_takes_null_outputs(jpegamd):
    t = qx.RANDOM(1).copy()
    none = [None] * 8
    assert jpegamd.lib.jpegamd_debug_table_consts(t.ctypes.data, *none) == 0
    assert jpegamd.lib.jpegamd_debug_table_consts(None, *none) == -1
    t[17] = 0
    assert jpegamd.lib.jpegamd_debug_table_consts(t.ctypes.data, *none) == -1


def test_a_context_is_needed_to_set_or_get(jpegamd):
    t, custom = qx.ONES.copy(), C.c_int32(7)
    assert jpegamd.lib.jpegamd_encoder_set_quant_tables(None, t.ctypes.data, None) == -1
    assert jpegamd.lib.jpegamd_encoder_get_quant_tables(None, None, None, C.byref(custom)) == -1


# ---- 2. the constants of a quality, through the table ------------------------------------------------------------------------------------
def test_table_consts_of_a_qualitys_tables_are_the_by_quality_constants(jpegamd):
    for q in (10, 50, 90):
        for chroma, table in enumerate(jpegamd.quant_tables_for_quality(q)):
            got = jpegamd.table_consts(table)
            want = jpegamd.chroma_mfma_consts(q) if chroma else jpegamd.mfma_consts(q)
            for key in ("qmul", "qthr", "bias", "zoff", "qadd"):
                assert got[key].dtype == np.float32 and got[key].tobytes() == want[key].astype(np.float32).tobytes(), (q, chroma, key)
            assert got["delta"].tobytes() == want["delta"].tobytes(), (q, chroma)
            thr, lob = jpegamd.group_thresholds(q, with_lo_bound=True, chroma=bool(chroma))
            assert got["grp_thr"].tobytes() == thr.tobytes() and got["lo_bound"].tobytes() == lob.tobytes(), (q, chroma)


# ---- 3. the constants of tables outside the family are on the safe side ---------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ALL_TABLES))
def test_constants_are_safe_for(jpegamd, name):
    """What test_mfma_constants_are_on_the_safe_side and test_group_zero_thresholds_are_safe (tests/test_host.py) assert of a quality's
    constants, of this table's: the band bias - 0.5 >= delta, the flag threshold 2 bias - 1 exactly and below 0.01, and at +- the
    bound of every coefficient group fl(a qmul + qadd) inside (qthr, 1)."""
    table = ALL_TABLES[name]
    c = jpegamd.table_consts(table)
    for z in range(64):
        k = cm.ZIGZAG[z]
        db = f64(f32(c["bias"][z])) - 0.5
        assert db >= c["delta"][k], z
        assert f32(c["qthr"][z]) == f32(f32(2.0) * f32(c["bias"][z]) - f32(1.0)), z
        assert f64(c["qthr"][z]) == 2.0 * db, z
        assert f64(c["qthr"][z]) >= db + c["delta"][k], z
        assert float(c["qthr"][z]) < 0.01, z
        assert f32(c["qadd"][z]) == f32(f64(f32(c["bias"][z])) + f64(f32(c["zoff"][z]))), z
        assert f32(c["qthr"][z]) < f32(c["qadd"][z]) < f32(1.0), z
    thr, lob = c["grp_thr"], c["lo_bound"]
    assert (thr > 0).all() and (lob > 0).all()
    for g in range(4):
        for h in range(2):
            t = f32((f64(thr[g, h]) + f64(lob[g, h])) * (1.0 + 2.0 ** -23))
            for j in range(8):
                z = 16 * g + 8 * h + j
                for a in (t, -t, np.nextafter(t, f32(0)), -np.nextafter(t, f32(0))):
                    zc = f32(f64(a) * f64(c["qmul"][z]) + f64(f32(c["qadd"][z])))          # one rounding, like v_fma_f32
                    assert f32(c["qthr"][z]) < zc < f32(1.0), (g, h, j, float(a), float(zc))


# ---- 4. the model, anchored -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", (10, 50, 90))
@pytest.mark.parametrize("size", ((72, 40), (9, 9)))
def test_model_files_are_the_quality_models_files(jpegamd, oracle, rgbs, size, q):
    rgb = rgbs[size]
    lq, cq = sm.scaled_table(sm.LUMA_Q, q), sm.scaled_table(sm.CHROMA_Q, q)
    assert np.array_equal(lq, jpegamd.quant_table(q)) and np.array_equal(cq, jpegamd.chroma_quant_table(q))
    luma = sm.luma_plane(rgb)
    assert qtm.gray_file(oracle, luma, lq) == cm.gray_file(oracle, luma, q) == oracle.encode_bmp(cm.write_bmp(rgb), q)
    for sub in SUBS:
        want = m422.color_file_422(oracle, cm.write_bmp(rgb), q) if sub == sm.SUB_422 else cm.rgb_file(oracle, rgb, q, sub)
        assert qtm.rgb_color_file(oracle, rgb, lq, cq, sub) == want, sub
        assert qtm.rgb_one_scan_file(oracle, rgb, lq, cq, sub) == im.interleaved_file(oracle, rgb, q, sub).file, sub
        for ri in (1, im.row_interval(size[0], sub)):
            assert qtm.rgb_one_scan_file(oracle, rgb, lq, cq, sub, ri) == rm.restart_file(oracle, rgb, q, sub, ri).file, (sub, ri)


# ---- 5. the model's files are files, and carry the tables ---------------------------------------------------------------------------------
def own_dqt_walk(data: bytes):
    """The quantisation tables of a file as they lie ON THE WIRE (zigzag order), by id: a walk of this test's own over the segments."""
    at, out = 2, {}
    while data[at + 1] != 0xDA:
        assert data[at] == 0xFF
        n = (data[at + 2] << 8) | data[at + 3]
        if data[at + 1] == 0xDB:
            for k in range(at + 4, at + 2 + n, 65):
                out[data[k]] = data[k + 1:k + 65]
        at += 2 + n
    return out


@pytest.mark.parametrize("name", sorted(qx.PAIRS))
def test_model_files_decode_and_carry_the_tables(oracle, rgbs, name):
    from PIL import Image
    import io
    lq, cq = qx.both(qx.PAIRS[name])
    rgb = rgbs[(72, 40)]
    files = {"gray": qtm.gray_file(oracle, sm.luma_plane(rgb), lq)}
    for sub in SUBS:
        files[("three", sub)] = qtm.rgb_color_file(oracle, rgb, lq, cq, sub)
        files[("one", sub)] = qtm.rgb_one_scan_file(oracle, rgb, lq, cq, sub)
    files[("one", "row")] = qtm.rgb_one_scan_file(oracle, rgb, lq, cq, sm.SUB_420, im.row_interval(72, sm.SUB_420))
    zz = np.array(cm.ZIGZAG)
    for key, data in files.items():
        img = Image.open(io.BytesIO(data))
        img.load()
        assert img.size == (72, 40) and img.mode == ("L" if key == "gray" else "RGB"), key
        wire = own_dqt_walk(data)
        assert wire == ({0: bytes(lq[zz])} if key == "gray" else {0: bytes(lq[zz]), 1: bytes(cq[zz])}), key
        got = qtm.dqt_tables(data)
        assert sorted(got) == sorted(wire) and np.array_equal(got[0], lq) and (key == "gray" or np.array_equal(got[1], cq)), key
        # what PIL read, as it numbers them (its own order handling is not relied on: only the multiset)
        assert sorted(img.quantization) == sorted(wire) and all(sorted(img.quantization[i]) == sorted(wire[i]) for i in wire), key


# ---- 6. the extreme picture ------------------------------------------------------------------------------------------------------------------
def test_extreme_reaches_the_largest_sizes_under_ones(oracle):
    p = qx.extreme()
    assert p.shape == (40, 72)
    zz = sm.plane_zigzag(oracle, p, qx.ONES).astype(np.int64)
    assert np.abs(zz[:, 1:]).max() >= 512 and np.abs(zz[:, 1:]).max() < 1024                  # an AC of size 10, none beyond
    sym, _, alen, is_dc, _ = sm.symbols(oracle, zz)
    assert int(sym[is_dc].max()) == 11                                                       # a DC difference of size 11
    assert int((sym[~is_dc] & 15).max()) == 10 and int(alen[~is_dc].max()) == 10
    size, _ = sm.dc_symbols(zz[:, 0], len(zz))
    assert int(size.max()) == 11
    rgb = qx.extreme_rgb()
    for plane in sm.planes_of(rgb, sm.SUB_420)[1:]:                                          # the chroma of the colour version is not flat
        assert np.abs(sm.plane_zigzag(oracle, plane, qx.ONES).astype(np.int64)[:, 1:]).max() >= 256


# ---- 7. the Python helpers --------------------------------------------------------------------------------------------------------------------
def test_as_quant_table(jpegamd):
    t = qx.RANDOM(5)
    for given in (t, t.tolist(), t.reshape(8, 8), t.reshape(8, 8).tolist(), t.astype(np.int64), t.astype(np.float64), tuple(t.tolist())):
        got = jpegamd.as_quant_table(given)
        assert got.dtype == np.uint8 and got.shape == (64,) and got.flags["C_CONTIGUOUS"] and np.array_equal(got, t)
    got = jpegamd.as_quant_table(t)
    got[0] ^= 0xFF
    assert np.array_equal(t, qx.RANDOM(5))                       # a copy: the caller's array is not the one that is kept
    bad = [t[:63], np.zeros((4, 16), np.uint8) + 1, t.reshape(2, 32), [[1] * 8] * 7, 5, None, "x" * 64,
           np.r_[t[:63], 0], np.r_[t[:63].astype(np.int64), 256], np.r_[t[:63].astype(np.int64), -1], t.astype(np.float64) + 0.5]
    for given in bad:
        with pytest.raises(ValueError):
            jpegamd.as_quant_table(given)


def test_parse_qtables(jpegamd):
    a, b = qx.RANDOM(6), qx.RANDOM(7)
    text = "# luma\n" + "\n".join(" ".join(f"{v:3d}" for v in a[r * 8:r * 8 + 8]) for r in range(8)) + "\n"
    luma, chroma = jpegamd.parse_qtables(text)
    assert np.array_equal(luma, a) and chroma is None
    two = text + "\n# chroma follows  1 2 3\n" + "\t".join(str(int(v)) for v in b) + "   # trailing comment"
    luma, chroma = jpegamd.parse_qtables(two)
    assert np.array_equal(luma, a) and np.array_equal(chroma, b)
    assert luma.dtype == chroma.dtype == np.uint8
    for text, count in ((" ".join(["1"] * 63), 63), (" ".join(["1"] * 65), 65), (" ".join(["1"] * 192), 192), ("# nothing\n", 0), ("", 0)):
        with pytest.raises(ValueError, match=rf"\b{count}\b"):
            jpegamd.parse_qtables(text)
    for text in (" ".join(["1"] * 63 + ["0"]), " ".join(["1"] * 63 + ["256"]), " ".join(["1"] * 63 + ["1.5"]), " ".join(["1"] * 63 + ["-3"]),
                 " ".join(["1"] * 63 + ["0x10"])):
        with pytest.raises(ValueError):
            jpegamd.parse_qtables(text)


def test_example_files_are_what_their_names_say(jpegamd):
    folder = ROOT / "tools" / "qtables"
    assert sorted(p.name for p in folder.glob("*.txt")) == ["flat16.txt", "luma_q90_chroma_q50.txt"]
    luma, chroma = jpegamd.parse_qtables((folder / "flat16.txt").read_text())
    assert np.array_equal(luma, qx.FLAT16) and chroma is None
    luma, chroma = jpegamd.parse_qtables((folder / "luma_q90_chroma_q50.txt").read_text())
    assert np.array_equal(luma, jpegamd.quant_table(90)) and np.array_equal(chroma, jpegamd.chroma_quant_table(50))


def test_the_block_is_thread_local_and_restores(jpegamd):
    """jpegamd.quant_tables without a device: the tables are this thread's, nest, and are gone behind the block, also by exception;
    a bad table is refused before anything is set."""
    import threading
    state = lambda: getattr(jpegamd._block_tables, "tables", None)
    assert state() is None
    seen = []
    with jpegamd.quant_tables(qx.FLAT16, qx.ONES.reshape(8, 8)):
        assert np.array_equal(state()[0], qx.FLAT16) and np.array_equal(state()[1], qx.ONES)
        th = threading.Thread(target=lambda: seen.append(state()))
        th.start()
        th.join()
        with jpegamd.quant_tables(qx.MAX):
            assert np.array_equal(state()[0], qx.MAX) and state()[1] is None
        assert np.array_equal(state()[0], qx.FLAT16)
    assert state() is None and seen == [None]
    with pytest.raises(KeyError):
        with jpegamd.quant_tables(qx.FLAT16):
            raise KeyError("x")
    assert state() is None
    with pytest.raises(ValueError):
        with jpegamd.quant_tables(np.zeros(64, np.uint8)):
            pass
    assert state() is None
