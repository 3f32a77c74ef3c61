"""Pictures whose end-of-band runs lie on the edges of the coder of DESIGN.md 4.6.13 -- TEST INFRASTRUCTURE ONLY, shared by
test_progressive_optimized_host.py (which proves every edge on the model's counters) and test_gpu_progressive_optimized.py."""
from __future__ import annotations

import numpy as np

import color_model as cm
import progressive_runs_model as prm

S444, S420, S422 = cm.SUB_444, cm.SUB_420, 4
FLAT = [(8, 8, 128, S444), (7, 5, 17, S420)]                     # (w, h, value, sub): segments of 1 and 3 bits, one-symbol tables
FLAT_513 = (216, 152, 90, S444)                                  # 27 x 19 = 513 blocks: AC segments of 9 / 9 / 2 bits
EDGE_W, EDGE_H, EDGE_Q = 512, 40, 100                            # 64 x 5 = 320 blocks: segments of 256 + 64


def flat_rgb(w, h, value):
    return np.full((h, w, 3), value, np.uint8)


def _blocks(kinds: dict, seed: int) -> np.ndarray:
    """A 512 x 40 plane of 320 blocks in raster order, flat 128 but for `kinds`: block index -> "N" noise (every coefficient, the last
    of either band too), "G" columns a a a a b b b b (coefficients 1, 6, 15, 28 exactly: non-empty in either band, its last
    coefficient zero), "H" columns a b b a a b b a (coefficient 14 alone: empty in the band 1 .. 5)."""
    rng = np.random.default_rng(seed)
    p = np.full((EDGE_H, EDGE_W), 128, np.uint8)
    for i, kind in kinds.items():
        by, bx = divmod(i, EDGE_W // 8)
        if kind == "N":
            block = rng.integers(0, 256, (8, 8))
        elif kind == "G":
            block = np.tile(np.array([100, 100, 100, 100, 156, 156, 156, 156]), (8, 1))
        else:
            block = np.tile(np.array([150, 106, 106, 150, 150, 106, 106, 150]), (8, 1))
        p[8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = block
    return p


def edge_planes():
    """(Y, Cb, Cr), 4:4:4.
    Y:  segment 0 empty in the band 1 .. 5 -- one run of 256, cut at block 256, which is empty too --, and in the band 6 .. 63 "H" at 59
        and 71: a run of 59, a run of 12 that its non-empty starter 59 begins and that covers 60 .. 70 across the lane round, a run of
        185; segment 1 runs of 1, 1, 2, 3, 4 between noise blocks, then 48.
    Cb: "G" at 0, noise at 127: a run of 127 that includes its non-empty starter, and a run of 128 behind a block whose last coefficient
        is non-zero; segment 1: noise at 256, a run of 63.
    Cr: noise at 0: a run of 255."""
    y = {59: "H", 71: "H", 257: "N", 259: "N", 262: "N", 266: "N", 271: "N"}
    return _blocks(y, 1), _blocks({0: "G", 127: "N", 256: "N"}, 2), _blocks({0: "N"}, 3)


def edge_model(oracle):
    return cm.memo(prm.ycbcr_file, oracle, *edge_planes(), EDGE_Q, S444)


def noise_rgb():
    """56 x 40 noise for quality 90: two block rows over the whole range (dense blocks: tables of many symbols), one of grey noise, two of
    low amplitude (sparse high coefficients: ZRLs)."""
    rng = np.random.default_rng(21)
    rgb = rng.integers(112, 144, (40, 56, 3), np.uint8)
    rgb[:16] = rng.integers(0, 256, (16, 56, 3), np.uint8)
    rgb[16:24] = np.repeat(rng.integers(0, 256, (8, 56, 1), np.uint8), 3, axis=2)
    return rgb


SYNTH = [(333, 250), (325, 243)]                                 # 42 x 32 blocks: whole MCUs at every subsampling; 41 x 31: pad blocks at 4:2:0 and 4:2:2


def synth_batch():
    """Three distinct 333 x 250 pictures: photo-like, noise, gradient."""
    return [cm.synth_rgb(333, 250, 100 + 37 * i, (0, 1, 3)[i], 0) for i in range(3)]
