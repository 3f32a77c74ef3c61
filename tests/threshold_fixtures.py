"""Pictures that sit exactly on the item and string thresholds of k_tile_encode, k_segment_merge and k_stitch -- TEST
INFRASTRUCTURE ONLY.

A picture is a grid of 8 x 8 blocks.  Block (row, bx) is pattern (bx + 11 row) % 64 of a fixed bank of noise patterns, scaled by a
per-block amplitude 0 .. 255 (0: flat 128), or an override: a single cosine basis function (one coefficient behind a long run of
zeros: ZRLs), a flat value, or 64 pixel values (the tile of more bits than any noise gives).  Blocks transform independently, so the items and bits of every (pattern, amplitude) pair at a
quality are known from ONE run of the oracle's stage functions; the search (python -m tests.threshold_fixtures --search) tunes the
amplitudes against those numbers until the path model (tests/path_model.py) says the picture meets its target, and writes the
parameters and the model's numbers to tests/golden/thresholds.json.  Tests only rebuild pictures from that file and re-derive where
they sit (tests/test_thresholds_host.py); nothing here is read by the library."""
from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
for _p in (str(HERE), str(HERE.parent)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import color_fixtures as cf   # noqa: E402
import color_model as cm      # noqa: E402
import path_model as pm       # noqa: E402
import scan_model as sm       # noqa: E402

JSON_PATH = HERE / "golden" / "thresholds.json"
NPAT, BANK_SEED = 64, 20240917
_BANK = np.random.default_rng(BANK_SEED).integers(-128, 128, (NPAT, 8, 8))
_BASIS = cf.basis()
K = pm.K


def _oracle():
    from oracle import oracle
    return oracle


# ---- pictures -------------------------------------------------------------------------------------------------------------
def pattern_of(row, bx):
    return (bx + 11 * row) % NPAT


def noise_block(pat: int, amp: int) -> np.ndarray:
    return np.clip(128 + (_BANK[pat] * amp) // 128, 0, 255)


def basis_block(z: int, a: int) -> np.ndarray:
    """128 + a x the basis function of zigzag position z: one coefficient of about a / step at z"""
    return np.clip(np.rint(128.0 + a * _BASIS[cm.ZIGZAG[z]]), 0, 255).astype(np.int64)


def expand_rows(spec: dict) -> np.ndarray:
    """int [block rows, blocks per row]: amplitudes.  spec["rows"]: per block row a list of [count, amplitude] runs; fewer rows than
    the picture has are repeated cyclically."""
    bw, bh = spec["w"] // 8, spec["h"] // 8
    out = np.zeros((bh, bw), np.int64)
    for r in range(bh):
        runs = spec["rows"][r % len(spec["rows"])]
        row = np.concatenate([np.full(c, a, np.int64) for c, a in runs]) if runs else np.zeros(0, np.int64)
        assert len(row) == bw, (spec["name"], r, len(row), bw)
        out[r] = row
    return out


def plane_of(spec: dict) -> np.ndarray:
    """uint8 [h, w]: the picture's one-byte plane (the luma itself, or the Cb plane of a chroma fixture)."""
    amps = expand_rows(spec)
    bh, bw = amps.shape
    pats = pattern_of(np.arange(bh)[:, None], np.arange(bw)[None, :])
    blocks = np.clip(128 + (_BANK[pats] * amps[:, :, None, None]) // 128, 0, 255)              # [bh, bw, 8, 8]
    for (r, bx, kind, p1, p2) in spec.get("over", []):
        blocks[r, bx] = basis_block(p1, p2) if kind == "basis" else (np.array(p1).reshape(8, 8) if kind == "pix" else np.full((8, 8), p1))
    return np.ascontiguousarray(blocks.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8)).astype(np.uint8)


def rle(row) -> list:
    out = []
    for a in row:
        if out and out[-1][1] == int(a):
            out[-1][0] += 1
        else:
            out.append([1, int(a)])
    return out


def gray_bmp(y: np.ndarray, top_down: bool = False) -> bytes:
    """24-bit BMP with R = G = B = y: the luma weights sum to 256, so Y == y exactly."""
    h, w = y.shape
    stride = (3 * w + 3) & ~3
    rows = np.zeros((h, stride), np.uint8)
    rows[:, :3 * w] = np.repeat(y if top_down else y[::-1], 3, axis=1)
    head = b"BM" + (54 + stride * h).to_bytes(4, "little") + bytes(4) + (54).to_bytes(4, "little")
    info = ((40).to_bytes(4, "little") + w.to_bytes(4, "little") + (-h if top_down else h).to_bytes(4, "little", signed=True)
            + (1).to_bytes(2, "little") + (24).to_bytes(2, "little") + bytes(24))
    return head + info + rows.tobytes()


def quant_of(spec_or_q, chroma: bool) -> np.ndarray:
    q = spec_or_q if isinstance(spec_or_q, int) else spec_or_q["quality"]
    return cm.scaled_table(cm.CHROMA_Q, q) if chroma else _oracle().quant_table(q)


def zigzag_of(spec: dict) -> np.ndarray:
    """The oracle's zigzag coefficients of the picture's plane: oracle.stages of the BMP (luma), color_model's plane_zigzag (Cb)."""
    chroma = spec["plane"] == "cb"
    if chroma:
        return cm.plane_zigzag(_oracle(), plane_of(spec), quant_of(spec, True))
    return _oracle().stages(gray_bmp(plane_of(spec)), spec["quality"])["zigzag"]


def scan_of(spec: dict, zz: np.ndarray) -> bytes:
    return sm.pack_scan(_oracle(), zz, True) if spec["plane"] == "cb" else _oracle().entropy(zz)


def report_of(spec: dict, with_scan: bool = True):
    zz = zigzag_of(spec)
    tab = pm.CHROMA if spec["plane"] == "cb" else pm.LUMA
    scan = scan_of(spec, zz) if with_scan else None
    return pm.picture_report(zz, spec["w"] // 8, spec["h"] // 8, tab, scan), zz, scan


# ---- targets: name -> (fixture, test over the model's report) -----------------------------------------------------------------
def _kinds(t, part=0):
    return [p["kind"] for p in t["parts"][part]["passes"]]


def _zrl_in(t, kind, count):
    """a pass of `kind` holds a symbol with `count` ZRLs in front"""
    return any(p["kind"] == kind and p["zrl"][count - 1] > 0 for pt in t["parts"] for p in pt["passes"])


def _zrl_after_fell(t, count):
    return any(a["kind"] == "fell" and a["zrl"][count - 1] > 0 for pt in t["parts"] for a in pt["passes"])


T0 = lambda r: r["tiles"][0]                                                             # noqa: E731
S8 = lambda r, i=0: r["seg"][K["kSegTiles"]]["segs"][i]                                  # noqa: E731
S16 = lambda r, i=0: r["seg"][K["kSegTilesBatch"]]["segs"][i]                            # noqa: E731
R8 = lambda r: r["seg"][K["kSegTiles"]]                                                  # noqa: E731
R16 = lambda r: r["seg"][K["kSegTilesBatch"]]                                            # noqa: E731
LADDER = {"head-1": (0, -1), "head": (0, 0), "head+1": (0, 1), "head+piece-1": (1, -1), "head+piece": (1, 0), "head+piece+1": (1, 1),
          "head+2piece-1": (2, -1), "head+2piece": (2, 0), "head+2piece+1": (2, 1)}     # target name -> (pieces, words) beyond the head
CAP, HEAD, PASS, QMIN = K["kStageItemCap"], K["kTileHeadStr"], K["kPassItems"], K["kQuadMinItems"]
F8, F16 = K["merge_fast_bits"][K["kSegTiles"]], K["merge_fast_bits"][K["kSegTilesBatch"]]
P16 = K["stitch_part_bits"][K["kSegTilesBatch"]]
LIGHT = 700                                                                              # "the other half stays light"

TARGETS = {
    # tile coder: item counts
    "tile.items_at_cap": ("items928", lambda r: T0(r)["items"] == CAP and T0(r)["nparts"] == 1),
    "tile.items_over_cap": ("items929", lambda r: T0(r)["items"] == CAP + 1 and T0(r)["nparts"] > 1),
    "tile.first_half_at_cap": ("h0_928", lambda r: T0(r)["items_h0"] == CAP and T0(r)["items"] - CAP <= LIGHT and T0(r)["nparts"] == 2),
    "tile.first_half_over_cap": ("h0_929", lambda r: T0(r)["items_h0"] == CAP + 1 and T0(r)["items"] - CAP - 1 <= LIGHT and T0(r)["nparts"] == 4),
    "tile.second_half_at_cap": ("h1_928", lambda r: T0(r)["items"] - T0(r)["items_h0"] == CAP and T0(r)["items_h0"] <= LIGHT and T0(r)["nparts"] == 2),
    "tile.second_half_over_cap": ("h1_929", lambda r: T0(r)["items"] - T0(r)["items_h0"] == CAP + 1 and T0(r)["items_h0"] <= LIGHT and T0(r)["nparts"] == 4),
    # tile coder: part lengths
    "tile.part_mod128_0": ("items256", lambda r: T0(r)["items"] == 2 * PASS and _kinds(T0(r)) == ["pair", "pair"]),
    "tile.part_mod128_1": ("items257", lambda r: T0(r)["items"] == 2 * PASS + 1 and _kinds(T0(r)) == ["pair", "pair", "tail"]),
    "tile.part_mod128_64": ("items320", lambda r: T0(r)["items"] == 2 * PASS + 64 and _kinds(T0(r)) == ["pair", "pair", "tail"]),
    "tile.part_mod128_65": ("items321", lambda r: T0(r)["items"] == 2 * PASS + 65 and _kinds(T0(r)) == ["pair", "pair", "pair"]),
    "tile.part_mod128_127": ("items383", lambda r: T0(r)["items"] == 2 * PASS + 127 and _kinds(T0(r)) == ["pair", "pair", "pair"]),
    "tile.at_most_64_items": ("flat_tile", lambda r: T0(r)["items"] <= K["tail_items"] and _kinds(T0(r)) == ["tail"]),
    "tile.one_block_ragged": ("ragged1", lambda r: r["tiles_per_row"] == K["kSegTiles"] + 1 and r["tiles"][K["kSegTiles"]]["items"] <= 65 and r["blocks_w"] % K["kTileBlocks"] == 1),
    # tile coder: the quad pass
    "tile.quad_below_min": ("items383", lambda r: T0(r)["items"] == QMIN - 1 and "quad" not in _kinds(T0(r)) and "fell" not in _kinds(T0(r))),
    "tile.quad_at_min": ("items384", lambda r: T0(r)["items"] == QMIN and _kinds(T0(r)) == ["quad", "pair"]),
    "tile.quad_128_left": ("items640", lambda r: T0(r)["items"] == 5 * PASS and _kinds(T0(r)) == ["quad", "quad", "pair"]),
    "tile.quad_129_left": ("items641", lambda r: T0(r)["items"] == 5 * PASS + 1 and _kinds(T0(r)) == ["quad", "quad", "quad"]),
    "tile.quad_with_run16": ("zrl_fell", lambda r: "fell" in _kinds(T0(r))),
    # tile coder: ZRLs
    **{f"tile.zrl{c}_tail": ("zrl_tail", (lambda c: lambda r: _zrl_in(T0(r), "tail", c))(c)) for c in (1, 2, 3)},
    **{f"tile.zrl{c}_pair": ("zrl_pair", (lambda c: lambda r: _zrl_in(T0(r), "pair", c))(c)) for c in (1, 2, 3)},
    **{f"tile.zrl{c}_after_fall_through": ("zrl_fell", (lambda c: lambda r: _zrl_after_fell(T0(r), c))(c)) for c in (1, 2, 3)},
    "tile.run_spans_pass": ("carry", lambda r: any(p["carry_run"] for p in T0(r)["parts"][0]["passes"])),
    # tile coder: string length
    "tile.words_56": ("words56", lambda r: T0(r)["str_words"] == K["tile_rezero_words"] - K["kTileRecWords"] and not T0(r)["rezero"]),
    "tile.words_57": ("words57", lambda r: T0(r)["str_words"] == K["tile_rezero_words"] - K["kTileRecWords"] + 1 and T0(r)["rezero"]),
    "tile.words_at_head": ("words120", lambda r: T0(r)["str_words"] == HEAD and T0(r)["whole"]),
    "tile.words_over_head": ("words121", lambda r: T0(r)["str_words"] == HEAD + 1 and not T0(r)["whole"]),
    "tile.writeouts_0": ("words121", lambda r: T0(r)["writeouts"] == 0 and not T0(r)["whole"]),
    "tile.writeouts_1": ("writeout1", lambda r: T0(r)["writeouts"] == 1),
    "tile.writeouts_2plus": ("dense_q100", lambda r: T0(r)["writeouts"] >= 2),
    "tile.stale_window": ("stale", lambda r: all(r["tiles"][i]["writeouts"] >= 2 and r["tiles"][i + 8]["items"] <= 64 for i in (0, 16))),
    # merge
    "merge8.bits_at_bound": ("seg8_at", lambda r: S8(r)["seg_bits"] == F8 and S8(r)["merge_fast"]),
    "merge8.bits_over_bound": ("seg8_over", lambda r: S8(r)["seg_bits"] == F8 + 1 and not S8(r)["merge_fast"] and S8(r)["max_words"] <= HEAD),
    "merge16.bits_at_bound": ("seg16_at", lambda r: S16(r)["seg_bits"] == F16 and S16(r)["merge_fast"] and S16(r)["tiles"] == 16),
    "merge16.bits_over_bound": ("seg16_over", lambda r: S16(r)["seg_bits"] == F16 + 1 and not S16(r)["merge_fast"] and S16(r)["max_words"] <= HEAD),
    "merge.slow_for_head_alone": ("words121", lambda r: S8(r)["seg_bits"] < F8 // 2 and S8(r)["max_words"] == HEAD + 1 and not S8(r)["merge_fast"]
                                  and S8(r)["merge_writeouts"] == 0),
    **{f"merge.tile_words_{name}": ("ladder", (lambda n: lambda r: any(t["str_words"] == n for t in r["tiles"]))(HEAD + K["kPieceWords"] * k + d))
       for name, (k, d) in LADDER.items()},
    "merge.slow_writeouts_0": ("words121", lambda r: not S8(r)["merge_fast"] and S8(r)["merge_writeouts"] == 0),
    "merge.slow_writeouts_1": ("seg8_w1", lambda r: not S8(r)["merge_fast"] and S8(r)["merge_writeouts"] == 1),
    "merge.slow_writeouts_3plus": ("dense_q100", lambda r: S8(r)["merge_writeouts"] >= 3 and S16(r)["merge_writeouts"] >= 3),
    "merge.ragged_1_tile": ("ragged1", lambda r: R8(r)["segs"][1]["tiles"] == 1),
    "merge.ragged_7_tiles": ("ragged7", lambda r: R8(r)["segs"][1]["tiles"] == 7),
    **{f"merge.segments_mod4_{n % 4}": (f"segs{n}", (lambda n: lambda r: R8(r)["num_segs"] == n)(n)) for n in (4, 5, 6, 7)},
    "merge.segments_16": ("segs16", lambda r: R8(r)["num_segs"] == K["kFinWaves"]),
    "merge.segments_17": ("segs17", lambda r: R8(r)["num_segs"] == K["kFinWaves"] + 1),
    # 0xFF placement
    "ff.tile_string": ("ff_tall", lambda r: r["ff_at"]["tile_string"] >= 1),
    "ff.first_dc": ("ff_tall", lambda r: r["ff_at"]["first_dc"] >= 1),
    "ff.merge_writeout": ("ff_dense", lambda r: R8(r)["ff_at"]["writeout"] >= 1 and R16(r)["ff_at"]["writeout"] >= 1),
    "ff.segment_in_group": ("ff_tall", lambda r: R8(r)["ff_at"]["segment_in_group"] >= 1),
    "ff.group": ("ff_tall", lambda r: R8(r)["ff_at"]["group"] >= 1),
    "ff.chunk": ("ff_tall", lambda r: R8(r)["ff_at"]["chunk"] >= 1),
    "ff.stitch_part": ("ff_dense", lambda r: R16(r)["ff_at"]["stitch_part"] >= 1),
    "ff.stitch_workgroup": ("ff_tall", lambda r: R16(r)["ff_at"]["stitch_workgroup"] >= 1),
    # stitch
    "stitch.parts_1": ("seg16_at", lambda r: S16(r)["stitch_parts"] == 1 and S16(r)["stitch_single"] and S16(r)["seg_bits"] == P16),
    "stitch.parts_2": ("seg16_over", lambda r: S16(r)["stitch_parts"] == 2 and S16(r)["seg_bits"] == P16 + 1),
    "stitch.parts_4plus": ("dense_q100", lambda r: S16(r)["stitch_parts"] >= 4),
    "stitch.tile_longer_than_part": ("long_tile", lambda r: S16(r)["stitch_piece_parts"] >= 2 and r["tiles"][0]["dc_bits"] + r["tiles"][0]["str_bits"] > P16),
    "stitch.wg_ff_at_most_255": ("ff_tall", lambda r: 0 < max(max(w) for w in R16(r)["wg_ff"]) <= 255),
    "stitch.wg_ff_256plus": ("dense_q100", lambda r: max(max(w) for w in R16(r)["wg_ff"]) >= 256),
    **{f"stitch.workgroups_{g}": (f"flat{n}", (lambda g: lambda r: -(-R16(r)["num_segs"] // K["kStWaves"]) == g and all(t["items"] == 2 for t in r["tiles"]))(g))
       for g, n in ((1, 8), (2, 9), (4, 32), (5, 33), (256, 2048), (257, 2049))},
    # chroma tables
    "chroma.parts_1": ("c_items928", lambda r: T0(r)["items"] == CAP and T0(r)["nparts"] == 1),
    "chroma.parts_2": ("c_h0_928", lambda r: T0(r)["items_h0"] == CAP and T0(r)["nparts"] == 2),
    "chroma.parts_4": ("c_h0_929", lambda r: T0(r)["items_h0"] == CAP + 1 and T0(r)["nparts"] == 4),
    "chroma.words_at_head": ("c_words120", lambda r: T0(r)["str_words"] == HEAD and T0(r)["whole"]),
    "chroma.words_over_head": ("c_words121", lambda r: T0(r)["str_words"] == HEAD + 1 and not T0(r)["whole"]),
    "chroma.zrl_tail": ("c_zrl_tail", lambda r: all(_zrl_in(T0(r), "tail", c) for c in (1, 2, 3))),
    "chroma.zrl_pair": ("c_zrl_pair", lambda r: all(_zrl_in(T0(r), "pair", c) for c in (1, 2, 3))),
    "chroma.zrl_after_fall_through": ("c_zrl_fell", lambda r: all(_zrl_after_fell(T0(r), c) for c in (1, 2, 3))),
    "chroma.slow_merge": ("c_words121", lambda r: not S8(r)["merge_fast"]),
    "chroma.stitch_parts": ("c_dense", lambda r: S16(r)["stitch_parts"] >= 2),
}
EXACT_PAIRS = [("tile.items_at_cap", "tile.items_over_cap"), ("tile.first_half_at_cap", "tile.first_half_over_cap"),
               ("tile.second_half_at_cap", "tile.second_half_over_cap"), ("tile.quad_below_min", "tile.quad_at_min"),
               ("tile.quad_128_left", "tile.quad_129_left"), ("tile.words_56", "tile.words_57"), ("tile.words_at_head", "tile.words_over_head"),
               ("merge8.bits_at_bound", "merge8.bits_over_bound"), ("merge16.bits_at_bound", "merge16.bits_over_bound"),
               ("stitch.parts_1", "stitch.parts_2"), ("chroma.words_at_head", "chroma.words_over_head")]


def model_numbers(rep: dict) -> dict:
    """What the JSON records next to the parameters: for a reader, and as a second opinion in the host test."""
    t, s8, s16 = rep["tiles"][0], S8(rep), S16(rep)
    return dict(total_bits=rep["total_bits"], symbols=rep["symbols"], ff=rep.get("ff_total"),
                tile0=dict(items=t["items"], items_h0=t["items_h0"], nparts=t["nparts"], str_bits=t["str_bits"], str_words=t["str_words"],
                           writeouts=t["writeouts"], whole=t["whole"], passes=[_kinds(t, i) for i in range(t["nparts"])]),
                seg8=dict(seg_bits=s8["seg_bits"], fast=s8["merge_fast"], writeouts=s8["merge_writeouts"], n=R8(rep)["num_segs"]),
                seg16=dict(seg_bits=s16["seg_bits"], fast=s16["merge_fast"], writeouts=s16["merge_writeouts"], parts=s16["stitch_parts"],
                           n=R16(rep)["num_segs"]))


def load() -> dict:
    return json.loads(JSON_PATH.read_text())


def fixtures() -> list:
    return load()["fixtures"]


def targets_met(spec: dict, rep: dict) -> list:
    """the fixture's recorded targets that it meets (a name this module no longer knows counts as not met)"""
    return [t for t in spec["targets"] if t in TARGETS and TARGETS[t][1](rep)]


# ---- the search -----------------------------------------------------------------------------------------------------------
class Pool:
    """Items, bits and DC of every (pattern, amplitude) block at one quality and table, from one run of the oracle's stages."""

    def __init__(self, quality: int, chroma: bool):
        self.tab = pm.CHROMA if chroma else pm.LUMA
        pats, amps = np.meshgrid(np.arange(NPAT), np.arange(256), indexing="ij")
        blocks = np.clip(128 + (_BANK[pats] * amps[:, :, None, None]) // 128, 0, 255)
        plane = np.ascontiguousarray(blocks.transpose(0, 2, 1, 3).reshape(NPAT * 8, 256 * 8)).astype(np.uint8)
        zz = cm.plane_zigzag(_oracle(), plane, quant_of(quality, chroma))
        it = pm.item_lists(zz, self.tab)
        blk_bits = np.bincount(it["block"], weights=it["bits"], minlength=len(zz)).astype(np.int64)
        self.items = it["items"].reshape(NPAT, 256)
        self.ac_bits = (blk_bits - it["dc_bits"]).reshape(NPAT, 256)
        self.dc = zz[:, 0].astype(np.int64).reshape(NPAT, 256)
        self.zrls = np.bincount(it["block"], weights=it["zrl"], minlength=len(zz)).astype(np.int64).reshape(NPAT, 256)

    def row(self, amps: np.ndarray, row: int = 0):
        """-> per block of one block row (the picture's first: DC predictor 0): items, bits with the DC symbol, ZRLs, DC bits"""
        p = pattern_of(row, np.arange(len(amps)))
        dc = self.dc[p, amps]
        dcb = pm.dc_symbol_bits(dc - np.r_[0, dc[:-1]], self.tab)
        return self.items[p, amps], self.ac_bits[p, amps] + dcb, self.zrls[p, amps], dcb


def climb(pool: Pool, amps: np.ndarray, err, free: np.ndarray, seed: int, iters: int = 8000, allowed=None) -> np.ndarray:
    """Hill climb over the amplitudes of the blocks `free` until err(items, bits, zrls, dc bits) is 0: random steps, and -- close
    to the target -- every amplitude of one block.  `allowed` (bool [pattern, amplitude]): the blocks `free` take only those."""
    last = None
    for attempt in range(4):
        try:
            return _climb(pool, amps, err, free, seed + 1000 * attempt, iters, allowed)
        except RuntimeError as e:
            last = e
    raise last


def _climb(pool, amps, err, free, seed, iters, allowed):
    rng = np.random.default_rng(seed)
    amps = amps.copy()
    pats = pattern_of(0, np.arange(len(amps)))
    ok = (lambda i, a: True) if allowed is None else (lambda i, a: bool(allowed[pats[i], a]))
    for i in free:                                                       # start from allowed amplitudes
        while not ok(i, amps[i]):
            amps[i] = (amps[i] + 1) % 256
    best = err(*pool.row(amps))
    for _ in range(iters):
        if best == 0:
            return amps
        i = int(rng.choice(free))
        old = amps[i]
        if best <= 40 and rng.random() < 0.3:
            cands = rng.permutation(256)
        else:
            cands = [int(np.clip(old + rng.integers(-8, 9), 0, 255))]
        for a in cands:
            if not ok(i, a):
                continue
            amps[i] = a
            e = err(*pool.row(amps))
            if e <= best:
                best, old = e, a
                if e == 0:
                    return amps
        amps[i] = old
    raise RuntimeError(f"search stopped {best} away")


def _dist(x, lo, hi):
    return max(lo - x, 0) + max(x - hi, 0)


def _tile_str_bits(bits, dcb, t=0):
    return int(bits[32 * t:32 * t + 32].sum() - dcb[32 * t])


def _spec(name, w, h, q, rows, over=(), plane="luma"):
    return dict(name=name, w=w, h=h, quality=q, plane=plane, rows=[rle(r) for r in rows], over=[list(o) for o in over])


def _tile0_row(pool, err, a0, seed, nblocks=256, rest=0, allowed=None):
    amps = np.full(nblocks, rest, np.int64)
    amps[:32] = a0
    return climb(pool, amps, err, np.arange(32), seed, allowed=allowed)


def _long_tile(target_bits: int):
    """32 blocks whose symbols take more than `target_bits` bits at quality 100 (the noise bank ends near 880 bits per block, a stitch
    part holds 1016 per block).  Pixel-wise hill climb from 0 / 255 noise with the oracle's stages as the evaluator: blocks of even
    and odd index in turn (a block's DC changes its right neighbour's DC symbol too); a first stage that also tries a pixel's
    complement, then a second with a fresh generator.  About 100 000 steps: the search keeps a tile it found before."""
    qt = quant_of(100, False)
    lanes = np.arange(32)

    def bits(B):
        plane = np.ascontiguousarray(B.transpose(1, 0, 2).reshape(8, 256)).astype(np.uint8)
        it = pm.item_lists(cm.plane_zigzag(_oracle(), plane, qt), pm.LUMA)
        return np.bincount(it["block"], weights=it["bits"], minlength=32)

    B = np.random.default_rng(7).integers(0, 2, (32, 8, 8)) * 255
    best = bits(B)
    for seed, steps, complement in ((7, 12000, True), (8, 150000, False)):
        rng = np.random.default_rng(seed)
        if complement:
            rng.integers(0, 2, (32, 8, 8))                               # (the generator that drew the start goes on)
        for k in range(steps):
            if best.sum() > target_bits:
                return B
            C = B.copy()
            for _ in range(int(rng.integers(1, 4))):
                idx = rng.integers(0, 8, (32, 2))
                opts = [0, 255] + ([255 - C[lanes, idx[:, 0], idx[:, 1]][0]] if complement else []) + [int(rng.integers(0, 256))]
                C[lanes, idx[:, 0], idx[:, 1]] = rng.choice(opts)
            mine = lanes % 2 == k % 2
            g = bits(np.where(mine[:, None, None], C, B)) - best
            up = (g + np.r_[g[1:], 0] > 0) & mine
            if up.any():
                B[up] = C[up]
                best = bits(B)
    raise RuntimeError(f"the densest tile found has {int(best.sum())} bits")


def search() -> dict:
    out, unreachable = [], {}
    pools = {}

    def pool(q, chroma=False):
        if (q, chroma) not in pools:
            pools[(q, chroma)] = Pool(q, chroma)
        return pools[(q, chroma)]

    failed = {}

    def add(make, name=None):
        try:
            spec = make() if callable(make) else make
        except RuntimeError as e:                                         # the target then shows up as unreachable
            print("FAILED", name, e, flush=True)
            failed[name] = str(e)
            return
        out.append(spec)
        print("built", spec["name"], flush=True)

    def items_total(n, no_zrl=False):
        return lambda it, b, z, d: abs(int(it[:32].sum()) - n) + (int(z[:32].sum()) if no_zrl else 0)

    for chroma in (False, True):
        pre, plane, q = ("c_", "cb", 90) if chroma else ("", "luma", 75)
        P = pool(q, chroma)
        add(lambda: _spec(pre + "items928", 2048, 8, q, [_tile0_row(P, items_total(CAP), 120, 1)], plane=plane))
        half = lambda h, n: (lambda it, b, z, d: abs(int(it[16 * h:16 * h + 16].sum()) - n) + _dist(int(it[16 - 16 * h:32 - 16 * h].sum()), 200, LIGHT - 100))   # noqa: E731
        for h, n in ((0, CAP), (0, CAP + 1)) + (() if chroma else ((1, CAP), (1, CAP + 1))):
            a = np.zeros(256, np.int64)
            a[:32] = 10
            a[16 * h:16 * h + 16] = 80
            add(lambda: _spec(f"{pre}h{h}_{n}", 2048, 8, 90, [climb(pool(90, chroma), a, half(h, n), np.arange(32), 2 + h)], plane=plane))
        words = lambda n: (lambda it, b, z, d: _dist(_tile_str_bits(b, d), 32 * n - 31, 32 * n) + max(int(it[:32].sum()) - CAP, 0))   # noqa: E731
        for n in (HEAD, HEAD + 1):
            add(lambda: _spec(f"{pre}words{n}", 2048, 8, q, [_tile0_row(P, words(n), 60, 5)], plane=plane))
        # ZRLs: basis blocks with one coefficient behind 19, 39 and 59 zeros
        step = quant_of(q, chroma)
        over = [[0, i, "basis", z, int(1.6 * step[cm.ZIGZAG[z]]) + 2] for i, z in enumerate((20, 40, 60))]
        add(lambda: _spec(pre + "zrl_tail", 160, 8, q, [np.zeros(20, np.int64)], over, plane))
        add(lambda: _spec(pre + "zrl_pair", 2048, 8, q, [np.zeros(256, np.int64)], over, plane))
        a = np.zeros(256, np.int64)
        a[3:32] = 8 if chroma else 150
        fq = 95 if chroma else q                                         # (the chroma table at 90 leaves noise too few items for a quad attempt)
        fstep = quant_of(fq, chroma)
        fover = [[0, i, "basis", z, int(1.6 * fstep[cm.ZIGZAG[z]]) + 2] for i, z in enumerate((20, 40, 60))]
        add(lambda: _spec(pre + "zrl_fell", 2048, 8, fq, [climb(pool(fq, chroma), a, lambda it, b, z, d: _dist(int(it[3:32].sum()), QMIN + 40, CAP - 40), np.arange(3, 32), 6)],
                          fover, plane))
    P = pool(75)
    add(lambda: _spec("items929", 2048, 8, 75, [_tile0_row(P, items_total(CAP + 1), 120, 1)]))
    for n in (2 * PASS, 2 * PASS + 1, 2 * PASS + 64, 2 * PASS + 65, QMIN - 1):
        add(lambda: _spec(f"items{n}", 2048, 8, 75, [_tile0_row(P, items_total(n), 30, 7)]))
    for n in (QMIN, 5 * PASS, 5 * PASS + 1):
        add(lambda: _spec(f"items{n}", 2048, 8, 75, [_tile0_row(P, items_total(n, True), 60 if n == QMIN else 90, 8, allowed=P.zrls == 0)]))
    add(lambda: _spec("flat_tile", 2048, 8, 75, [np.zeros(256, np.int64)]))
    for name, w in (("ragged1", 2048 + 8), ("ragged7", 2048 + 7 * 256)):
        add(lambda: _spec(name, w, 8, 75, [np.random.default_rng(9).integers(0, 120, w // 8)]))
    # a run that spans a pass boundary: the basis block's AC item is item 128 of the list
    step = quant_of(75, False)
    a = np.zeros(256, np.int64)
    a[:10] = 60
    add(lambda: _spec("carry", 2048, 8, 75, [climb(P, a, lambda it, b, z, d: abs(int(it[:10].sum()) + 1 - PASS) + int(z[:10].sum()), np.arange(10), 3)],
              [[0, 10, "basis", 40, int(1.6 * step[cm.ZIGZAG[40]]) + 2]]))
    for n in (56, 57):
        add(lambda: _spec(f"words{n}", 2048, 8, 75, [_tile0_row(P, lambda it, b, z, d, n=n: _dist(_tile_str_bits(b, d), 32 * n - 31, 32 * n), 30, 5)]))
    P100 = pool(100)
    for amp in range(20, 256, 5):                                      # a tile whose window is written out exactly once
        s = _spec("writeout1", 2048, 8, 100, [np.r_[np.full(32, amp), np.zeros(224, np.int64)]])
        if report_of(s, False)[0]["tiles"][0]["writeouts"] == 1:
            add(s)
            break
    add(lambda: _spec("dense_q100", 4096, 64, 100, [np.full(512, 255, np.int64)]))
    add(lambda: _spec("stale", 2048, 32, 100, [np.full(256, 255, np.int64), np.zeros(256, np.int64)]))
    # merge
    segbits = lambda n, nb: (lambda it, b, z, d: abs(int(b.sum()) - n) + 50 * sum(max(_tile_str_bits(b, d, t) - 32 * HEAD, 0) for t in range(nb // 32)))   # noqa: E731
    for name, nb, n, a0 in (("seg8_at", 256, F8, 48), ("seg8_over", 256, F8 + 1, 48), ("seg16_at", 512, F16, 48), ("seg16_over", 512, F16 + 1, 48)):
        add(lambda: _spec(name, nb * 8, 8, 75, [climb(P, np.full(nb, a0, np.int64), segbits(n, nb), np.arange(nb), 4, iters=60000)]))
    for amp in range(4, 256):                                          # the slow path with exactly one write-out
        s = _spec("seg8_w1", 2048, 8, 75, [np.full(256, amp, np.int64)])
        if S8(report_of(s, False)[0])["merge_writeouts"] == 1:
            add(s)
            break
    P90 = pool(95)
    ladder = [HEAD + K["kPieceWords"] * k + d for k in (0, 1, 2) for d in (-1, 0, 1)]
    a = np.zeros(512, np.int64)
    for t, n in enumerate(ladder):
        a[32 * t:32 * t + 32] = 40 + 35 * (t // 3)
        a = climb(P90, a, lambda it, b, z, d, t=t, n=n: _dist(_tile_str_bits(b, d, t), 32 * n - 31, 32 * n), np.arange(32 * t, 32 * t + 32), 11 + t)
    add(lambda: _spec("ladder", 4096, 8, 95, [a]))
    for n in (4, 5, 6, 7, 16, 17):
        add(lambda: _spec(f"segs{n}", 256, 8 * n, 75, [np.random.default_rng(20 + n + r).integers(0, 200, 32) for r in range(n)]))
    for n in (8, 9, 32, 33, 2048, 2049):
        add(lambda: _spec(f"flat{n}", 8, 8 * n, 75, [np.zeros(1, np.int64)]))
    # 0xFF bytes across boundaries: seeds until the model reports every kind
    for name, w, h, kinds in (("ff_tall", 8, 8 * 1024, [t for t, (f, _) in TARGETS.items() if f == "ff_tall"]),
                              ("ff_dense", 4096, 24, [t for t, (f, _) in TARGETS.items() if f == "ff_dense" and t.startswith("ff.")])):
        for seed in range(40):
            rng = np.random.default_rng(100 + seed)
            s = _spec(name, w, h, 100, [rng.integers(200, 256, w // 8) for _ in range(h // 8)])
            rep = report_of(s)[0]
            if all(TARGETS[t][1](rep) for t in kinds):
                add(s)
                break
        else:
            raise RuntimeError(f"no seed gives {name} every 0xFF placement")
    kept = [f for f in (fixtures() if JSON_PATH.exists() else []) if f["name"] == "long_tile"]          # (the long climb is not repeated)
    if kept and all(TARGETS[t][1](report_of(kept[0])[0]) for t, (f, _) in TARGETS.items() if f == "long_tile"):
        add({k: kept[0][k] for k in ("name", "w", "h", "quality", "plane", "rows", "over")})
    else:
        add(lambda: _spec("long_tile", 4096, 8, 100, [np.zeros(512, np.int64)],
                          [[0, i, "pix", [int(v) for v in b.ravel()], 0] for i, b in enumerate(_long_tile(P16 + 48))]), "long_tile")
    add(lambda: _spec("c_dense", 4096, 8, 100, [np.full(512, 255, np.int64)], plane="cb"))
    names = {s["name"] for s in out}
    for s in out:
        s["targets"] = [t for t, (f, _) in TARGETS.items() if f == s["name"]]
        rep = report_of(s)[0]
        missed = [t for t in s["targets"] if not TARGETS[t][1](rep)]
        for t in missed:
            unreachable[t] = f"the search's fixture {s['name']} does not meet it"
        s["targets"] = [t for t in s["targets"] if t not in missed]
        s["model"] = model_numbers(rep)
    for t, (f, _) in TARGETS.items():
        if f not in names:
            unreachable[t] = f"no fixture {f} was built" + (f": {failed[f]}, a stitch part holds {P16}" if f in failed else "")
    return dict(constants={k: v for k, v in K.items() if isinstance(v, int)}, fixtures=out, unreachable=unreachable)


def dumps(doc: dict) -> str:
    """JSON with one fixture per line group: rows stay on one line each."""
    lines = ['{', ' "constants": ' + json.dumps(doc["constants"]) + ',', ' "unreachable": ' + json.dumps(doc["unreachable"]) + ',', ' "fixtures": [']
    for i, s in enumerate(doc["fixtures"]):
        lines.append("  " + json.dumps(s, separators=(",", ":")) + ("," if i + 1 < len(doc["fixtures"]) else ""))
    return "\n".join(lines + [" ]", "}"]) + "\n"


if __name__ == "__main__":
    if "--search" in sys.argv:
        doc = search()
        JSON_PATH.write_text(dumps(doc))
        print(f"{len(doc['fixtures'])} fixtures, {len(doc['unreachable'])} unreachable: {sorted(doc['unreachable'])}")
    else:
        for s in fixtures():
            rep = report_of(s)[0]
            print(s["name"], targets_met(s, rep) == s["targets"], json.dumps(model_numbers(rep)["tile0"]))
