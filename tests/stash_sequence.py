"""A picture on which one wave of k_tile_encode codes tiles WITH and WITHOUT an exact-order event in turn -- TEST INFRASTRUCTURE ONLY.

The kernel makes the luma stash (the tile's luma in s_pix[wave], what the exact-order path reads) only in a tile that has an event;
after every tile the same words hold that tile's item list.  What can go wrong is a stale stash: a wave codes a tile without an event,
and its next tile, which has one, reads what the tile before left there.  A launch forms min(tiles / 8, JPEGAMD_TILE_MAX_WGS)
workgroups of JPEGAMD_TILE_WG_WAVES waves (both read from the kernel's source here, as tests/path_model.py reads its thresholds), so
only a picture with more tiles than that many waves makes a wave code a second tile; no committed fixture has that many.

The picture is 512 samples wide, two tiles per block row: a picture has at most 65 535 rows (the frame header's 16 bits; describe() and
jpegamd_parse_bmp reject more), so one tile per block row stops at 8 191 tiles, fewer than two per wave.  Tiles of
tests/quant_fixtures.py are laid out in tile order (the order in which the kernel hands them out) in a fixed seeded order, a pattern of
PATTERN tiles repeated until the picture has at least 3 x (waves of a full launch) tiles.  PATTERN is a prime: the pattern does not
line up with the 8 tiles of a chunk or the waves of a launch.  Which tiles have an event is decided by the model (tests/quant_model.py)
at the picture's one quality -- the quality at which the fixture search found the event tiles."""
from __future__ import annotations

import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np

import quant_fixtures as qf
import quant_model as qm

SRC = Path(__file__).resolve().parents[1] / "jpeg-image-compression_amd" / "csrc" / "jpegamd_tile_pipeline.hip"
EVENT_TILES = ("count4", "two_sites_two_groups", "lane63", "tie_luma")
PATTERN = 509                                 # tiles of the seeded pattern (a prime)
SEED = 20264
ROUNDS = 3                                    # the picture has at least this many tiles per wave of a full launch


def launch_waves() -> int:
    """Waves of a full launch of k_tile_encode: JPEGAMD_TILE_MAX_WGS x JPEGAMD_TILE_WG_WAVES, from the kernel's source."""
    text = SRC.read_text()
    vals = []
    for name in ("JPEGAMD_TILE_MAX_WGS", "JPEGAMD_TILE_WG_WAVES"):
        m = re.search(r"#define\s+" + name + r"\s+(\d+)\s*$", text, re.M)
        if not m:
            raise RuntimeError(f"stash_sequence: {name} not found in {SRC.name}")
        vals.append(int(m.group(1)))
    return vals[0] * vals[1]


_made = {}


def picture(jpegamd, oracle):
    """-> namespace: plane uint8 [8 T / 2, 512] (T tiles; tile t in block row t // 2, columns 256 (t % 2) .. 256 (t % 2) + 255), quality,
    has_event bool [T] (by the model), events (the model's total over the picture), names [T] of the tiles, waves (of a full launch)."""
    if "p" in _made:
        return _made["p"]
    s = qf.fixture_set(jpegamd, oracle, "full")
    by_name = {f.name: f for f in s.fixtures}
    ev = [by_name[n] for n in EVENT_TILES]
    quality = ev[0].quality
    if any(f.quality != quality or f.table != "luma" for f in ev):
        raise RuntimeError(f"stash_sequence: the event tiles were found at different qualities: {[(f.name, f.quality) for f in ev]}")
    none = [f for f in s.fixtures if f.name.startswith("dead_")]
    flat = SimpleNamespace(name="flat", tile=np.zeros((32, 64), np.int64))
    kinds = ev + none + [flat]
    # the model, per kind of tile, at the picture's quality (a flag depends on its own block alone)
    flags = {f.name: int(qm.evaluate(jpegamd, oracle, f.tile, "luma", quality).flags.sum()) for f in kinds}
    with_event = [f for f in kinds if flags[f.name] > 0]
    without = [f for f in kinds if flags[f.name] == 0]
    rng = np.random.default_rng(SEED)
    pick_event = rng.integers(0, 2, PATTERN).astype(bool)
    pattern = [with_event[int(rng.integers(0, len(with_event)))] if e else without[int(rng.integers(0, len(without)))] for e in pick_event]
    waves = launch_waves()
    reps = -(-ROUNDS * waves // PATTERN)
    reps += reps & 1                          # whole block rows of two tiles, and whole pairs of patterns
    order = pattern * reps
    rows = {f.name: (f.tile.reshape(32, 8, 8).transpose(1, 0, 2).reshape(8, 256) + 128).astype(np.uint8) for f in kinds}
    plane = np.ascontiguousarray(np.concatenate([np.hstack([rows[a.name], rows[b.name]]) for a, b in zip(order[0::2], order[1::2])], axis=0))
    if plane.shape[0] > 65535:
        raise RuntimeError(f"stash_sequence: {plane.shape[0]} rows do not fit a picture")
    _made["p"] = SimpleNamespace(plane=plane, quality=quality, names=[f.name for f in order], flags=flags, waves=waves,
                                 has_event=np.array([flags[f.name] > 0 for f in order]), events=int(sum(flags[f.name] for f in order)),
                                 event_kinds=[f.name for f in with_event], none_kinds=[f.name for f in without])
    return _made["p"]
