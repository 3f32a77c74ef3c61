"""Progressive files with a scan script of the caller's on the CPU: the model of the file
(tests/progressive_script_model.py) against the models of the built-in scripts and an independent decoder, the validator and the bound
through the library (no device is needed), jpegamd.progressive_script.parse_scan_script, and the fixtures of the GPU suite proven on
the model's counters."""
from __future__ import annotations

import ctypes as C
import io

import numpy as np
import pytest

import color_model as cm
import interleaved_model as im
import progressive_runs_model as prm
import progressive_script_fixtures as fx
import progressive_script_model as scm
import progressive_successive_fixtures as sfx
import progressive_successive_model as psm

image = pytest.importorskip("PIL.Image")
S444, S420, S422 = fx.S444, fx.S420, fx.S422
ERR_ARG = -1
Y, CB, CR, ALL = fx.Y, fx.CB, fx.CR, fx.ALL


def _decode(data: bytes, mode="RGB"):
    with image.open(io.BytesIO(data)) as f:
        return f.info.get("progressive"), np.asarray(f.convert(mode))


# ---- the model against the existing yardsticks -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rgb,sub", [("crop", S420), ("crop", S444), ("flat", S420)], ids=["crop-420", "crop-444", "7x5"])
def test_built_in_scripts_give_the_existing_models_files(oracle, rgb, sub):
    rgb = sfx.lena_crop() if rgb == "crop" else fx.flat_rgb(7, 5, 200)
    assert fx.model(oracle, rgb, 50, sub, fx.SPECTRAL).file == cm.memo(prm.rgb_file, oracle, rgb, 50, sub).file
    want = cm.memo(psm.rgb_file, oracle, rgb, 50, sub)
    got = fx.model(oracle, rgb, 50, sub, fx.SUCCESSIVE)
    assert got.file == want.file and np.array_equal(got.counts, want.counts) and got.seg_bits == want.seg_bits
    assert got.stuffed == want.stuffed and got.scan_bits == want.scan_bits


@pytest.mark.parametrize("name", fx.COMPLETE)
def test_pillow_decodes_every_complete_script_to_the_one_scan_pixels(oracle, name):
    for rgb, q, sub in ((sfx.lena_crop(), 50, S420), (np.ascontiguousarray(sfx.lena_crop()[:43, :67]), 90, S422), (fx.flat_rgb(7, 5, 17), 50, S420)):
        progressive, got = _decode(fx.model(oracle, rgb, q, sub, fx.COLOUR[name]).file)
        _, want = _decode(cm.memo(im.interleaved_file, oracle, rgb, q, sub).file)
        assert progressive == 1 and np.array_equal(got, want), (name, rgb.shape, q, sub)


@pytest.mark.parametrize("name", sorted(fx.GRAYS))
def test_pillow_decodes_the_grayscale_files_to_the_oracle_files_pixels(oracle, name):
    for plane, q in ((fx.gray_plane(67, 43), 50), (fx.gray_plane(7, 9), 90), (np.full((1, 1), 77, np.uint8), 50)):
        m = fx.gray_model(oracle, plane, q, fx.GRAYS[name])
        progressive, got = _decode(m.file, "L")
        _, want = _decode(cm.gray_file(oracle, plane, q), "L")
        assert progressive == 1 and np.array_equal(got, want), (name, plane.shape, q)
        assert m.ids == ((0x00, 0x10, 0x10) if name == "GRAY_SPLIT" else (0x00, 0x10, 0x10, 0x10, 0x10))


def test_pillow_opens_the_dc_only_file(oracle):
    m = fx.model(oracle, sfx.lena_crop(), 50, S420, fx.DC_ONLY)
    progressive, got = _decode(m.file)
    assert progressive == 1 and got.shape == (128, 128, 3) and len(m.scan_bits) == 1
    _, whole = _decode(cm.memo(im.interleaved_file, oracle, sfx.lena_crop(), 50, S420).file)
    assert np.abs(got.astype(int).mean() - whole.astype(int).mean()) < 2      # the block averages alone: the same picture, coarsely


def test_headers_sos_and_table_ids(oracle):
    m = fx.model(oracle, sfx.lena_crop(), 50, S420, fx.Y_CB)
    assert m.ids == (0x00, 0x01, 0x01, 0x10, 0x11, 0x11)
    assert prm.parse_tables(m.file) == [(i, list(b), list(v)) for i, (b, v, _) in zip(m.ids, m.tables)]
    assert psm.sos_parameters(m.file) == [(tuple(c + 1 for c in comps), ss, se, ah, al) for comps, ss, se, ah, al in fx.Y_CB]
    assert scm.sos(((1, 2), 0, 0, 1, 0)) == bytes([0xFF, 0xDA, 0, 10, 2, 2, 0x11, 3, 0x11, 0, 0, 0x10])
    m = fx.model(oracle, sfx.lena_crop(), 50, S420, fx.DC_FORMS)
    assert m.ids == (0x00, 0x01, 0x01, 0x10, 0x11, 0x11) and m.header_len[3] == 10 and m.header_len[4] == 12   # refinements: the SOS alone
    assert len(fx.LIMIT) == 16 and len(fx.model(oracle, fx.flat_rgb(8, 8, 90), 50, S444, fx.LIMIT).ids) == 16


# ---- the validator, through the library -------------------------------------------------------------------------------------------------
def _validate(jpegamd, script, comps):
    arr, n = jpegamd._scan_array(script)
    bad = C.c_int32(99)
    rc = jpegamd.lib.jpegamd_validate_scan_script(arr, n, comps, C.byref(bad))
    assert jpegamd.lib.jpegamd_validate_scan_script(arr, n, comps, None) == rc       # bad_scan may be NULL
    return rc, bad.value


def test_every_fixture_script_is_accepted(jpegamd):
    import jpegamd.progressive_script as ps
    for script in fx.COLOUR.values():
        assert _validate(jpegamd, script, 3) == (0, -1)
        jpegamd.validate_scan_script(script, 3)
    for script in fx.GRAYS.values():
        assert _validate(jpegamd, script, 1) == (0, -1)
    assert (ps.SPECTRAL, ps.SUCCESSIVE, ps.GRAY_SUCCESSIVE) == (fx.SPECTRAL, fx.SUCCESSIVE, fx.GRAY_SUCCESSIVE)


DC = (ALL, 0, 0, 0, 0)
REFUSALS = [
    ("17 scans", [DC] + [(Y, k, k, 0, 0) for k in range(1, 17)], 3, -1),
    ("17 tables with 16 scans", [DC] + [(Y, k, k, 0, 0) for k in range(1, 16)], 3, -1),
    ("empty component set", [DC, ((), 1, 63, 0, 0)], 3, 1),
    ("Cb in a grayscale script", [(Y, 0, 0, 0, 0), (CB, 0, 0, 0, 0)], 1, 1),
    ("ss = 0, se = 5", [(ALL, 0, 5, 0, 0)], 3, 0),
    ("AC scan with two components", [DC, ((0, 1), 1, 63, 0, 0)], 3, 1),
    ("se < ss", [DC, (Y, 6, 5, 0, 0)], 3, 1),
    ("se = 64", [DC, (Y, 1, 64, 0, 0)], 3, 1),
    ("al = 14", [(ALL, 0, 0, 0, 14)], 3, 0),
    ("ah = 2, al = 0", [(ALL, 0, 0, 0, 2), (ALL, 0, 0, 2, 0)], 3, 1),
    ("a refinement without a first scan", [DC, (Y, 1, 63, 2, 1)], 3, 1),
    ("a first scan repeated", [DC, (Y, 1, 63, 0, 0), (Y, 1, 5, 0, 0)], 3, 2),
    ("ah not the previous al", [DC, (Y, 1, 63, 0, 2), (Y, 1, 63, 1, 0)], 3, 2),
    ("an interleaved refinement over different al", [(Y, 0, 0, 0, 1), ((1, 2), 0, 0, 0, 2), (ALL, 0, 0, 1, 0)], 3, 2),
    ("AC before that component's DC", [(Y, 0, 0, 0, 0), (CB, 1, 63, 0, 0), ((1, 2), 0, 0, 0, 0)], 3, 1),
    ("a component without DC", [((0, 1), 0, 0, 0, 0), (Y, 1, 63, 0, 0)], 3, -1),
    ("no scan", [], 3, -1),
    ("two components in the file", [DC], 2, -1),
]


@pytest.mark.parametrize("what,script,comps,bad", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_name_the_scan(jpegamd, what, script, comps, bad):
    assert _validate(jpegamd, script, comps) == (ERR_ARG, bad)
    if comps in (1, 3) and script:
        with pytest.raises(ValueError, match="whole" if bad < 0 else f"scan {bad}"):
            jpegamd.validate_scan_script(script, comps)
        assert jpegamd.max_jfif_bytes_progressive_script(64, 64, S420 if comps == 3 else 0, script) == 0


def test_the_17_tables_script_has_16_scans():
    script = REFUSALS[1][1]
    assert len(script) == 16 and sum(scm.scan_tables(s) for s in script) == 17 and len(REFUSALS[0][1]) == 17


# ---- the bound --------------------------------------------------------------------------------------------------------------------------
def test_bound_is_zero_for_bad_arguments_and_holds_the_models_files(jpegamd, oracle):
    bound = jpegamd.max_jfif_bytes_progressive_script
    assert bound(0, 8, S420) == 0 and bound(8, 65536, S420) == 0 and bound(8, 8, 7) == 0
    assert bound(8, 8, 0, fx.SPLIT) == 0 and bound(8, 8, S420, fx.GRAY_SPLIT) == 0    # a colour script for a grayscale file; Cb and Cr without DC
    assert bound(8, 8, 0) > 0 and bound(8, 8, S444) > 0
    rgb = sfx.noise_rgb()
    for name in ("DEEP", "LIMIT", "SPLIT", "DC_ONLY"):
        assert len(fx.model(oracle, rgb, sfx.NOISE_Q, S444, fx.COLOUR[name]).file) <= bound(sfx.NOISE_W, sfx.NOISE_H, S444, fx.COLOUR[name])
    # a DC-only file's bound is far below a whole file's
    assert bound(512, 512, S420, fx.DC_ONLY) * 20 < bound(512, 512, S420, fx.DEEP)
    # the default colour script: the built-in entry's scans, bounded scan by scan -- no more than that entry's bound, which charges
    # every block of every MCU (pad blocks, and chroma blocks at Y's cost) for all ten scans
    assert 0 < bound(512, 512, S420) <= jpegamd.max_jfif_bytes_progressive_successive(512, 512, S420)


# ---- parse_scan_script ------------------------------------------------------------------------------------------------------------------
def test_fixture_scripts_survive_libjpegs_text_form():
    import jpegamd.progressive_script as ps
    for script in list(fx.COLOUR.values()) + list(fx.GRAYS.values()):
        assert ps.parse_scan_script(fx.libjpeg_text(script)) == script
    text = "# a comment\n0 1 2: 0-0, 0, 1 ;   # interleaved DC\n0: 1-5 0 2;\n\n2:1-63,0,1;"
    assert ps.parse_scan_script(text) == [(ALL, 0, 0, 0, 1), (Y, 1, 5, 0, 2), (CR, 1, 63, 0, 1)]


@pytest.mark.parametrize("text", ["0 1 2 ;", "0,1,2;\n", "", "# nothing\n", "0: 0-0, 0, 1", "0: 0-0, 0 ;", "0: 0, 0, 0, 1 ;", "x: 0-0, 0, 1 ;",
                                  "0: 1-5, 0, 2 ; garbage", "0:: 1-5, 0, 2 ;", "0: -1-5, 0, 2 ;"])
def test_the_colon_less_form_and_garbage_are_refused(text):
    import jpegamd.progressive_script as ps
    with pytest.raises(ValueError):
        ps.parse_scan_script(text)


# ---- what the fixtures exercise ---------------------------------------------------------------------------------------------------------
def test_flat_pictures_are_one_block_and_one_mcu_with_pad_blocks(oracle):
    for name in ("SPLIT", "DC_FORMS", "Y_CB", "DC_ONLY"):
        m = fx.model(oracle, fx.flat_rgb(7, 5, 200), 50, S420, fx.COLOUR[name])
        inter_y = [k for k, (c, ss, *_) in enumerate(fx.COLOUR[name]) if ss == 0 and len(c) > 1 and 0 in c]
        assert [m.pad_blocks[k] for k in inter_y] == [3] * len(inter_y)
        assert all(sum(b) <= 2 for b, _, _ in m.tables)          # tables of one symbol, or two (an interleaved Y: its first block, then its pad blocks)
        assert all(len(s) == 1 for s in m.seg_bits)
        one = fx.model(oracle, fx.flat_rgb(8, 8, 90), 50, S444, fx.COLOUR[name])
        assert all(sum(b) == 1 for b, _, _ in one.tables) and sum(one.pad_blocks) == 0      # one block a component: one-symbol tables
    assert fx.model(oracle, fx.flat_rgb(7, 5, 200), 50, S420, fx.Y_CB).pad_blocks[0] == 3


def test_gray_257_blocks_end_the_dc_refinement_with_a_one_bit_segment(oracle):
    w, h = fx.GRAY_257
    m = fx.gray_model(oracle, fx.gray_plane(w, h), 50, fx.GRAY_SUCCESSIVE)
    assert m.seg_bits[4] == (256, 1) and m.header_len[4] == 10
    assert all(len(s) == 2 for s in m.seg_bits)


def test_1344_y_blocks_are_five_full_segments_and_one_of_64(oracle):
    w, h = fx.SIZE_1344
    m = fx.model(oracle, sfx.synth_batch()[0], 50, S420, fx.DC_FORMS)
    assert m.seg_bits[3] == (256,) * 5 + (64,)                   # the one-component DC refinement of Y
    assert len(m.seg_bits[0]) == 6 and m.seg_bits[4] == (256,) * 2 + (160,)         # {Cb, Cr}: 336 MCUs of two blocks, 128 to a segment
    m = fx.model(oracle, sfx.synth_batch()[0], 50, S420, fx.Y_CB)
    assert len(m.seg_bits[0]) == -(-336 // 51)                   # {Y, Cb}: five blocks to an MCU, 51 MCUs to a segment
    m = fx.model(oracle, fx.crop_67x43(), 50, S420, fx.Y_CB)     # 9 x 6 blocks under 5 x 3 MCUs: Y pad blocks in a two-component scan of several MCUs
    assert m.pad_blocks[0] == 15 * 4 - 9 * 6 and len(m.seg_bits[0]) == 1


def test_deep_has_zrls_with_pending_bits_and_four_depths(oracle):
    m = fx.model(oracle, sfx.lena_crop(), 90, S444, fx.DEEP)
    assert m.zrl_with_bits > 0 and sum(m.zrl[2:5]) > 0 and [s[3:] for s in fx.DEEP[1:5]] == [(0, 3), (3, 2), (2, 1), (1, 0)]
    m = fx.model(oracle, sfx.noise_rgb(), sfx.NOISE_Q, S444, fx.DEEP)
    assert max(max(s) for s in m.seg_bits) > 65536               # dense blocks: a segment beyond one round of the coder's window


def test_edges_has_single_coefficient_bands_with_runs(oracle):
    m = fx.model(oracle, sfx.lena_crop(), 50, S422, fx.EDGES)
    assert {r.scan for r in m.runs} >= {2, 3, 4, 5, 6}
    assert any(r.length > 1 for r in m.runs if r.scan == 6)      # band 63 .. 63: long runs of empty blocks
