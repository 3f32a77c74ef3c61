"""The pictures of the grayscale-scan suites (test_gray_scan_host.py proves on the CPU, through gray_scan_model's counters, that each has
the property it is named for; test_gpu_gray_scan.py compares the device's files with the model's) -- TEST INFRASTRUCTURE ONLY.
Everything is seeded and made on the fly; the seeds of the searched pictures were found once through the model and are pinned here."""
from __future__ import annotations

import numpy as np

import color_model as cm
import gray_scan_model as gm
import scan_model as sm

INTERVALS = (0, 1, "row", 255, 256, 257, 65535)
MODES = (False, True)                                          # optimised tables?


def interval(ri, w):
    return -(-w // 8) if ri == "row" else ri


def model(oracle, plane, q, ri=0, optimized=False):
    return gm.gray_file(oracle, plane, q, ri, optimized)


def noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), np.uint8)


def ramp(w, h):
    return np.add.outer(np.arange(h) * 3, np.arange(w) * 2).astype(np.uint8)


def synth_luma(w, h, seed, kind=0):
    return sm.luma_plane(cm.synth_rgb(w, h, seed, kind))


# ---- 1. geometry: (name, plane, quality) ------------------------------------------------------------------------------------------------
# 1 x 1, one block, 2 x 2 blocks with both edges replicated, 9 x 5 blocks; one block row of 255, 256 and 257 blocks -- one below, at and
# one above the coder's segment; 128 x 128 noise at quality 100: 256 blocks in ONE segment of more than 65 536 bits, several rounds of the
# coder's window; 40 x 520: 5 x 65 = 325 blocks in many rows, more than 8 intervals at Ri = row, so RSTn wraps
def shapes():
    return [("1x1", noise(1, 1, 1), 50), ("8x8", noise(8, 8, 2), 90), ("9x9", noise(9, 9, 3), 90), ("72x40", ramp(72, 40), 50),
            ("2040x8", noise(2040, 8, 4), 90), ("2048x8", noise(2048, 8, 5), 50), ("2056x8", noise(2056, 8, 6), 90),
            ("128x128", noise(128, 128, 7), 100), ("40x520", synth_luma(40, 520, 9), 90)]


MULTI_ROUND = "128x128"


# ---- 2. flat pictures: one-symbol tables, the shortest segments ---------------------------------------------------------------------------
def flat(w, h, value=128):
    return np.full((h, w), value, np.uint8)


# (w, h): three blocks (a block is "00" + "1010" = 6 bits with the Annex K tables, 2 bits with the picture's own two one-symbol tables),
# and 257 blocks: the 257th alone in the second segment
FLAT = [(24, 8), (2056, 8)]
FLAT_INTERVALS = (0, 1, 2, 3, 256, 257)


def steps(values, q=50):
    """One block row of flat blocks of the given values: DC symbols alone (and EOB)."""
    return np.repeat(np.repeat(np.array(values, np.uint8)[None, :], 8, 0), 8, 1)


# At quality 50 a flat block of value v has DC round((v - 128) / 2).  With Ri = 1 every difference is taken against 0: a picture's DC table
# has the sizes of its values alone, and a block is (DC code + size) + 1 bits (EOB is the only AC symbol).  Together the three give
# segments of 2, 3, 4 and 5 bits:
#   mostly 130  size 1 '0' + 1 + 1 = 3 bits, size 0 '10' + 1 = 3;      mostly 128  size 0 '0' + 1 = 2, size 1 '10' + 1 + 1 = 4;
#   three sizes size 0 '0': 2 bits, size 2 '10' + 2 + 1 = 5, size 1 '11' -> '110' (no code is all ones) + 1 + 1 = 5
STEPS = [steps([130] * 5 + [128] * 3), steps([128] * 5 + [130] * 3), steps([128] * 5 + [134] * 2 + [130])]
STEP_INTERVALS = (1, 2, 3)


# ---- 3. the writer's edges ----------------------------------------------------------------------------------------------------------
# noise at Ri = 1: many padded bytes that come out 0xFF, many intervals that end on a byte
PAD_FF = [("2056x8", 1), ("128x128", 1)]                        # (shape name, Ri)


def straddle():
    """513 blocks of noise at quality 100 without intervals: an 0xFF byte lies across a 256-block boundary at phase 2 with either tables
    (seed found through the model)."""
    return noise(4104, 8, 1011), 100


def tail_standard():
    """771 blocks: three runs of 255 noise blocks and two flat ones.  At Ri = 257 an interval is a segment of 256 blocks and one of ONE flat
    block (DC difference 0: 6 bits with the Annex K tables); the first segment of one interval ends at bit 1 of a byte (seed found through
    the model), so the padded byte's 7 bits begin in it.  The first 257 blocks alone, without intervals: the same for the flushed byte."""
    p = noise(8 * 771, 8, 2003)
    for i in range(3):
        p[:, 8 * (257 * i + 255):8 * (257 * i + 257)] = 128
    return p, 90


def tail_optimized(blocks=257):
    """Flat blocks, the one at index 10 of every 257 two grey levels up: two DC symbols of size 1 ('10' + 1 bit + EOB: 4 bits each) among
    blocks of 2 bits, so the first segment of every interval is 516 bits and the 2-bit last block shares its byte with 4 of them."""
    p = flat(8 * blocks, 8)
    for i in range(0, blocks, 257):
        p[:, 8 * (i + 10):8 * (i + 11)] = 130
    return p, 50


# ---- 4. the length limit ----------------------------------------------------------------------------------------------------------------
# (w, h, synth kind, seed, quality): the luma of huffman_fixtures.LONG_CODES' pictures -- the AC table's merge gives a length of 17
LONG_CODES = [(384, 288, 1, 1, 97), (384, 288, 0, 2, 97)]


def long_code_plane(w, h, kind, seed):
    return synth_luma(w, h, seed, kind)


# ---- 5. a batch ---------------------------------------------------------------------------------------------------------------------
def batch_of_three():
    """Three different 72 x 40 pictures -- photo-like, noise, gradient: three table pairs, three prefix lengths."""
    return [synth_luma(72, 40, 103 + 37 * i, kind) for i, kind in enumerate((0, 1, 3))]
