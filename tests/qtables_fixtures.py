"""Quantisation tables outside the quality family, and the picture that drives them to the coder's limits -- TEST INFRASTRUCTURE ONLY.
Every table is uint8 [64] in raster order, entries 1 .. 255."""
from __future__ import annotations

import numpy as np

import scan_model as sm

_k = np.arange(64)
ONES = np.ones(64, np.uint8)
MAX = np.full(64, 255, np.uint8)
CHECKER_A = np.where(_k % 2 == 0, 1, 255).astype(np.uint8)      # 1 / 255 by raster parity: the DC divides by 1 ...
CHECKER_B = np.where(_k % 2 == 0, 255, 1).astype(np.uint8)      # ... or by 255
FLAT16 = np.full(64, 16, np.uint8)
SPLIT = (sm.scaled_table(sm.LUMA_Q, 90), sm.scaled_table(sm.CHROMA_Q, 10))     # a fine luma table with a coarse chroma table


def RANDOM(seed: int) -> np.ndarray:
    """64 entries drawn uniformly from 1 .. 255."""
    return np.random.default_rng(seed).integers(1, 256, 64).astype(np.uint8)


def sparse_random(seed: int) -> np.ndarray:
    """Mostly 1 and 255 with a few entries in between: the mixtures a perceptual table does not have."""
    rng = np.random.default_rng(seed)
    t = rng.choice(np.array([1, 255], np.uint8), 64)
    at = rng.choice(64, 8, replace=False)
    t[at] = rng.integers(2, 255, 8)
    return t.astype(np.uint8)


# (luma, chroma or None) as Encoder.set_quant_tables takes them; None: the luma table for every component
PAIRS = {
    "ones": (ONES, ONES),
    "max": (MAX, MAX),
    "checker": (CHECKER_A, CHECKER_B),
    "flat16": (FLAT16, FLAT16),
    "random": (RANDOM(1), RANDOM(2)),
    "split": SPLIT,
    "luma_only": (RANDOM(3), None),
}
SINGLES = {"ones": ONES, "max": MAX, "checker_a": CHECKER_A, "checker_b": CHECKER_B, "flat16": FLAT16, "random1": RANDOM(1),
           "split_luma": SPLIT[0], "split_chroma": SPLIT[1]}


def both(pair):
    """(luma, chroma) of a PAIRS entry with the chroma table filled in."""
    return pair[0], (pair[0] if pair[1] is None else pair[1])


def extreme(w: int = 72, h: int = 40) -> np.ndarray:
    """uint8 [h, w]: blocks in turn flat 0, columns alternating 0 / 255 (+-128 about the level shift), flat 255.  Under ONES the
    striped blocks carry an AC coefficient beyond 512 (size 10), and a flat 255 block followed by a flat 0 block is a DC difference of
    -2040 (size 11)."""
    y, x = np.mgrid[0:h, 0:w]
    kind = (x // 8 + y // 8 * ((w + 7) // 8)) % 3
    return np.where(kind == 0, 0, np.where(kind == 2, 255, np.where(x % 2 == 1, 255, 0))).astype(np.uint8)


def extreme_rgb(w: int = 72, h: int = 40) -> np.ndarray:
    """A colour picture made of `extreme`: R carries it, G its mirror image left to right and B its mirror image top to bottom, so
    that the chroma planes are far from flat as well."""
    p = extreme(w, h)
    return np.ascontiguousarray(np.stack([p, p[:, ::-1], p[::-1]], axis=2))
