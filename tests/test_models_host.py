"""A pin of the CPU models (tests/*_model.py): every field of every model result over a fixed set of small pictures, digested and compared
with tests/golden/model_digests.json.  The models define the files the GPU suites accept, so a change to what any of them computes --
the packer, the MCU merge, the interval framing, a counter -- must show up here, whichever suite it would otherwise have slipped
through.  `python tests/test_models_host.py --record` rewrites the JSON: only for a deliberate change of a model's definition."""
from __future__ import annotations

import dataclasses
import hashlib
import json
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
if __name__ == "__main__":
    for _p in (str(HERE), str(HERE.parent), str(HERE.parent / "jpeg-image-compression_amd" / "python")):
        if _p not in sys.path:
            sys.path.insert(0, _p)

import color_fixtures as cf       # noqa: E402
import color_model as cm          # noqa: E402
import color_model_422 as m422    # noqa: E402
import gray_scan_fixtures as gf   # noqa: E402
import gray_scan_model as gm      # noqa: E402
import huffman_fixtures as hf     # noqa: E402
import huffman_model as hm        # noqa: E402
import interleaved_model as im    # noqa: E402
import progressive_model as pm    # noqa: E402
import restart_model as rm        # noqa: E402
import scan_model as sm           # noqa: E402

JSON_PATH = HERE / "golden" / "model_digests.json"
SUBS = (("444", cm.SUB_444), ("420", cm.SUB_420), ("422", m422.SUB_422))
# (w, h, synth kind, seed, quality): photo-like, noise, gradient, flat.  9 x 5, 25 x 15, 9 x 5 and 3 x 3 blocks: odd counts, so 4:2:0 and
# 4:2:2 have pad blocks
PICTURES = [(72, 40, 0, 21, 50), (200, 120, 1, 22, 90), (68, 40, 3, 23, 0), (24, 24, 2, 24, 75)]
# integer counters that a host test asserts to be non-zero somewhere: each must be non-zero in at least one case here
COUNTERS = {"Interleaved": ("pad_blocks", "zrl_luma", "zrl_chroma", "no_eob_blocks", "stuffed"),
            "Restart": ("markers", "pad_ff", "aligned", "stuffed", "two_segment_intervals"),
            "Optimized": ("pad_blocks", "stuffed", "borrowed_tails", "short_against_ff"),
            "GrayScan": ("markers", "pad_ff", "aligned", "straddle_ff", "borrowed_tails", "stuffed"),
            "Progressive": ("pad_blocks", "edge_runs")}


# ---- the canonical form -----------------------------------------------------------------------------------------------------------------
def norm(x):
    """bytes -> length + SHA-1, arrays -> shape + SHA-1 of the int64 contents, sequences and dicts recursively, integers as they are."""
    if isinstance(x, (bytes, bytearray)):
        return ["bytes", len(x), hashlib.sha1(x).hexdigest()]
    if isinstance(x, np.ndarray):
        return ["array", list(x.shape), hashlib.sha1(np.ascontiguousarray(x, np.int64)).hexdigest()]
    if isinstance(x, (tuple, list)):
        return [norm(v) for v in x]
    if isinstance(x, dict):
        return {repr(k): norm(v) for k, v in sorted(x.items())}
    assert isinstance(x, (int, np.integer, np.bool_)), type(x)
    return int(x)


def fields_of(result) -> dict:
    """field name -> canonical JSON text; a bare file (the three-scan models return bytes) is its only field."""
    named = {f.name: getattr(result, f.name) for f in dataclasses.fields(result)} if dataclasses.is_dataclass(result) else {"file": result}
    return {k: json.dumps(norm(v), sort_keys=True) for k, v in named.items()}


def digest(result) -> str:
    """SHA-1 of the whole canonical form, then -- so that a mismatch can name its field -- one byte of every field's own SHA-1."""
    f = fields_of(result)
    whole = hashlib.sha1(json.dumps(f, sort_keys=True).encode()).hexdigest()
    return whole + ":" + "".join(hashlib.sha1(t.encode()).hexdigest()[:2] for t in f.values())


def first_difference(result, recorded: str) -> str:
    tags = recorded.split(":")[1]
    for i, (name, text) in enumerate(fields_of(result).items()):
        if hashlib.sha1(text.encode()).hexdigest()[:2] != tags[2 * i:2 * i + 2]:
            return name
    return "(a field whose one-byte tag happens to agree)"


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def picture_cases(oracle, w, h, kind, seed, q, sub):
    """name -> result for one picture at one subsampling: every colour model, at the intervals around a row, a coder segment and the scan."""
    rgb = cm.synth_rgb(w, h, seed, kind)
    _, _, _, _, mx, my = im.geometry(w, h, sub)
    out = {"three-scan": im.three_scan_file(oracle, rgb, q, sub), "one-scan": im.interleaved_file(oracle, rgb, q, sub),
           "progressive": pm.progressive_file(oracle, rgb, q, sub)}
    for ri in sorted({1, mx, mx + 1, rm.seg_mcus(sub) + 1, mx * my + 5, 65535}):
        out[f"restart-{ri}"] = rm.restart_file(oracle, rgb, q, sub, ri)
    for ri in (0, 1, mx + 1):
        out[f"optimised-{ri}"] = hm.rgb_file(oracle, rgb, q, sub, ri)
    return out


def gray_cases(oracle, w, h, kind, seed, q):
    luma = sm.luma_plane(cm.synth_rgb(w, h, seed, kind))
    return {f"gray-{ri}-{'optimised' if opt else 'standard'}": gm.plane_file(oracle, luma, q, ri, opt)
            for ri in (0, 1, -(-w // 8), 257) for opt in (False, True)}


def fixture_cases(oracle):
    """The pictures of the other suites that reach the rare counters."""
    out = {}
    for name, (p, q), ris in (("straddle", gf.straddle(), (0,)), ("tail-standard", gf.tail_standard(), (0, 257)),
                              ("tail-optimised", gf.tail_optimized(771), (0, 257)), ("flat-2056x8", (gf.flat(2056, 8), 50), (0, 1, 256, 257))):
        for ri in ris:
            for opt in gf.MODES:
                out[f"gray-{name}-{ri}-{'optimised' if opt else 'standard'}"] = gm.plane_file(oracle, p, q, ri, opt)
    for name, case in (("borrowed", hf.BORROWED), ("against-ff", hf.AGAINST_FF)):
        for ri in (0, 86):
            out[f"optimised-{name}-{ri}"] = hm.ycbcr_file(oracle, *hf.short_tail_planes(case, ri), case["quality"], cm.SUB_444, ri)
    for ri in (0, 1, 5):
        out[f"optimised-flat-688x8-{ri}"] = hm.rgb_file(oracle, hf.flat(688, 8), 50, cm.SUB_444, ri)
    out["restart-flat-688x8-86"] = rm.restart_file(oracle, hf.flat(688, 8), 50, cm.SUB_444, 86)
    # every chroma symbol, ZRLs among them: the symbol plane as Cb, its mirror images as Cr and as Y (long runs with the luma table too)
    cb = cf.symbol_plane(oracle)
    cr, y = np.ascontiguousarray(cb[:, ::-1]), np.ascontiguousarray(cb[::-1])
    q = cf.SYMBOL_QUALITY
    out["symbols-three-scan"] = cm.ycbcr_file(oracle, y, cb, cr, q, cm.SUB_444)
    out["symbols-one-scan"] = im.interleaved_ycbcr_file(oracle, y, cb, cr, q, cm.SUB_444)
    out["symbols-restart-9"] = rm.restart_ycbcr_file(oracle, y, cb, cr, q, cm.SUB_444, 9)
    out["symbols-optimised-9"] = hm.ycbcr_file(oracle, y, cb, cr, q, cm.SUB_444, 9)
    out["symbols-progressive"] = pm.progressive_ycbcr_file(oracle, y, cb, cr, q, cm.SUB_444)
    out["symbols-three-scan-422"] = m422.ycbcr_file_422(oracle, y, cb[:, ::2].copy(), cr[:, ::2].copy(), q)
    return out


def groups(oracle):
    """group name -> a function that computes its cases."""
    out = {}
    for w, h, kind, seed, q in PICTURES:
        for sname, sub in SUBS:
            out[f"{w}x{h}-{sname}"] = lambda a=(w, h, kind, seed, q, sub): picture_cases(oracle, *a)
        out[f"{w}x{h}-gray"] = lambda a=(w, h, kind, seed, q): gray_cases(oracle, *a)
    out["fixtures"] = lambda: fixture_cases(oracle)
    return out


GROUPS = [f"{w}x{h}-{s}" for w, h, _, _, _ in PICTURES for s in ("444", "420", "422", "gray")] + ["fixtures"]


@pytest.fixture(scope="module")
def results(oracle):
    """group -> name -> result, every model run once."""
    return {g: fn() for g, fn in groups(oracle).items()}


@pytest.fixture(scope="module")
def recorded():
    return json.loads(JSON_PATH.read_text())


# ---- the tests --------------------------------------------------------------------------------------------------------------------------
def test_the_record_holds_these_cases_and_no_others(results, recorded):
    assert list(results) == GROUPS
    assert {g: sorted(r) for g, r in results.items()} == {g: sorted(r) for g, r in recorded.items()}


@pytest.mark.parametrize("group", GROUPS)
def test_models_compute_what_was_recorded(results, recorded, group):
    for name, result in results[group].items():
        want = recorded[group][name]
        assert digest(result) == want, f"{group} / {name}: field `{first_difference(result, want)}` differs from the record"


def test_every_counter_a_host_test_relies_on_is_reached(results):
    seen = {}
    for r in (r for g in results.values() for r in g.values()):
        if dataclasses.is_dataclass(r):
            for f in dataclasses.fields(r):
                v = getattr(r, f.name)
                if isinstance(v, (int, np.integer)) and v:
                    seen.setdefault(type(r).__name__, set()).add(f.name)
    missing = {cls: [n for n in names if n not in seen.get(cls, ())] for cls, names in COUNTERS.items()}
    assert not any(missing.values()), missing
    zrl = [r.zrl for g in results.values() for r in g.values() if isinstance(r, pm.Progressive)]
    assert all(any(z[(1, chroma)] for z in zrl) for chroma in (False, True)), "the band 6 .. 63 never codes a ZRL"      # (1 .. 5 cannot)


if __name__ == "__main__" and "--record" in sys.argv:
    from oracle import oracle
    doc = {g: {name: digest(r) for name, r in fn().items()} for g, fn in groups(oracle).items()}
    JSON_PATH.write_text(json.dumps(doc, indent=0, sort_keys=False) + "\n")
    print(sum(len(v) for v in doc.values()), "cases in", len(doc), "groups")
