"""The threshold fixtures (tests/threshold_fixtures.py, tests/golden/thresholds.json) sit where they claim -- on the CPU.

The path model (tests/path_model.py) is first checked against the oracle: its bit, symbol and 0xFF totals are the oracle's on every
fixture and on a handful of synthetic pictures.  Then every fixture is rebuilt from its parameters and the model must place it
exactly on its targets with the constants of the kernel sources AS THEY ARE NOW: a changed buffer size fails here, naming the
fixtures that left their edge, instead of quietly leaving the edge uncovered.  Nothing here reads the reference tree."""
from __future__ import annotations

import numpy as np
import pytest

import path_model as pm
import scan_model as sm
import threshold_fixtures as tf

MAX_UNREACHABLE = 3


@pytest.fixture(scope="module")
def doc():
    return tf.load()


@pytest.fixture(scope="module")
def reports(doc):
    return {s["name"]: (s,) + tf.report_of(s) for s in doc["fixtures"]}


def _totals_match(oracle, rep, zz, scan, chroma):
    """bits -- to the bit: the oracle's run/size symbols with the code lengths of T.81's tables, and the scan's zero-bit flush --,
    symbols, 0xFF bytes"""
    sym, _, alen, is_dc, _ = sm.symbols(oracle, zz)
    tab = pm.CHROMA if chroma else pm.LUMA
    assert rep["total_bits"] == int((alen + np.where(is_dc, tab.dc_len[sym & 15], tab.ac_len[sym])).sum())
    stream = pm.unstuff(scan)
    assert (rep["total_bits"] + 7) // 8 == len(stream)
    if rep["total_bits"] % 8:
        assert int(stream[-1]) & ((1 << (8 - rep["total_bits"] % 8)) - 1) == 0
    assert rep["symbols"] == len(sym)
    if not chroma:
        assert rep["symbols"] == len(oracle.rle_symbols(zz))
    assert rep["ff_total"] == scan.count(b"\xff\x00")
    assert sum(t["str_bits"] + t["dc_bits"] for t in rep["tiles"]) == rep["total_bits"]
    for T, r in rep["seg"].items():
        assert sum(s["seg_bits"] for s in r["segs"]) == rep["total_bits"]
        assert all(s["stitch_part_ends"][-1] == s["seg_bits"] for s in r["segs"])
        # every 0xFF byte lies inside one stitch workgroup at that workgroup's true byte phase, or across a workgroup boundary
        offs = [r["segs"][g]["offset"] for g in range(0, len(r["segs"]), pm.K["kStWaves"])]
        assert sum(w[o % 8] for w, o in zip(r["wg_ff"], offs)) + r["ff_at"]["stitch_workgroup"] == rep["ff_total"]


@pytest.mark.parametrize("w,h,seed,kind,q", [(2048, 16, 3, 1, 50), (520, 40, 2, 0, 90), (4104, 8, 1, 1, 100), (333, 250, 4, 0, 50), (264, 64, 5, 2, 10),
                                             (8, 264, 6, 1, 95)])
def test_model_totals_are_the_oracles_on_synthetic_pictures(jpegamd, oracle, w, h, seed, kind, q):
    bmp = jpegamd.synth_bmp(w, h, seed, kind, 0)
    zz = oracle.stages(bmp, q)["zigzag"]
    scan = oracle.entropy(zz)
    rep = pm.picture_report(zz, (w + 7) // 8, (h + 7) // 8, pm.LUMA, scan)
    _totals_match(oracle, rep, zz, scan, False)
    assert oracle.encode_bmp(bmp, q)[328:-2] == scan


def test_model_totals_are_the_oracles_on_every_fixture(oracle, reports):
    for name, (spec, rep, zz, scan) in reports.items():
        _totals_match(oracle, rep, zz, scan, spec["plane"] == "cb")


def test_constants_are_those_the_fixtures_were_tuned_for(doc, reports):
    """The message a changed buffer size should give: which constant moved, and which fixtures no longer sit on their edge."""
    moved = {k: (v, pm.K[k]) for k, v in doc["constants"].items() if pm.K.get(k) != v}
    off = sorted(name for name, (spec, rep, _, _) in reports.items() if tf.targets_met(spec, rep) != spec["targets"])
    assert not moved and not off, (f"kernel constants changed since the fixtures were tuned (recorded, now): {moved}; fixtures off their edge: {off}; "
                                   "regenerate with python -m tests.threshold_fixtures --search")


def test_every_fixture_lands_on_its_targets(reports):
    off = {}
    for name, (spec, rep, _, _) in reports.items():
        missed = [t for t in spec["targets"] if t not in tf.targets_met(spec, rep)]
        if missed:
            off[name] = (missed, tf.model_numbers(rep))
    assert not off, f"fixtures that no longer sit on their edge (regenerate with python -m tests.threshold_fixtures --search): {off}"
    for name, (spec, rep, _, _) in reports.items():
        assert tf.model_numbers(rep) == spec["model"], (name, "the recorded numbers are not the model's")


def test_coverage_is_the_target_list_less_the_declared_unreachable(doc, reports):
    """At this commit every target has a fixture and none is declared unreachable."""
    met = {t for name, (spec, rep, _, _) in reports.items() for t in tf.targets_met(spec, rep)}
    unreachable = set(doc["unreachable"])
    assert unreachable <= set(tf.TARGETS)
    assert all(isinstance(r, str) and r for r in doc["unreachable"].values())
    assert met == set(tf.TARGETS) - unreachable, (sorted(set(tf.TARGETS) - unreachable - met), sorted(met & unreachable))
    assert len(unreachable) <= MAX_UNREACHABLE, sorted(unreachable)
    assert not [p for p in tf.EXACT_PAIRS if unreachable & set(p)], "an exact at / one-above pair is not covered"


def test_luma_fixtures_are_the_same_picture_as_bgr_and_top_down(oracle, doc):
    """R = G = B: the BMP's luma is the one-byte plane, stored bottom-up or top-down."""
    for spec in doc["fixtures"]:
        if spec["plane"] != "luma" or spec["w"] * spec["h"] > 1 << 17:
            continue
        y = tf.plane_of(spec)
        a, b = oracle.stages(tf.gray_bmp(y), spec["quality"]), oracle.stages(tf.gray_bmp(y, top_down=True), spec["quality"])
        assert (a["y"].astype(int) + 128 == y).all() and (a["zigzag"] == b["zigzag"]).all(), spec["name"]


def test_json_holds_parameters_only(doc):
    assert tf.JSON_PATH.stat().st_size < 512 * 1024
    assert set(doc) == {"constants", "unreachable", "fixtures"}
    for s in doc["fixtures"]:
        assert set(s) == {"name", "w", "h", "quality", "plane", "rows", "over", "targets", "model"}, s["name"]
        assert all(isinstance(c, int) and isinstance(a, int) and 0 <= a <= 255 for row in s["rows"] for c, a in row)
