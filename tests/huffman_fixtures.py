"""The pictures of the optimised-Huffman suites (test_huffman_host.py proves on the CPU that each sits on its edge, test_gpu_huffman.py
compares the device's files with the model's) -- TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import numpy as np

import color_model as cm
import color_model_422 as m422
import huffman_model as hm
import interleaved_model as im
import restart_model as rm
from color_model import synth_rgb
from interleaved_model import row_interval

S444, S420, S422 = cm.SUB_444, cm.SUB_420, m422.SUB_422
SUBS = (S444, S420, S422)


def interval(ri, w, sub):
    return row_interval(w, sub) if ri == "row" else ri


def model(oracle, rgb, q, sub, ri=0):
    return cm.memo(hm.rgb_file, oracle, rgb, q, sub, ri)


def planes_model(oracle, planes, q, sub, ri=0):
    return cm.memo(hm.ycbcr_file, oracle, *planes, q, sub, ri)


# ---- 1. content x geometry x interval -----------------------------------------------------------------------------------------------
# (w, h, synth kind, quality): photo-like and noise; 200 x 120 is 25 x 15 blocks and 68 x 40 is 9 x 5 -- odd counts, so 4:2:0 has pad
# blocks in the last MCU column and row, 4:2:2 in the last column
CONTENT = [(200, 120, 0, 75), (200, 120, 1, 90), (68, 40, 0, 50), (68, 40, 1, 90)]
INTERVALS = (0, 1, 5, "row")


def content_rgb(w, h, kind):
    return synth_rgb(w, h, 11 + w + kind, kind)


def batch_of_three():
    """Three different 72 x 40 pictures -- photo-like, noise, gradient: three sets of tables, three prefix lengths."""
    return [synth_rgb(72, 40, 103 + 37 * i, kind) for i, kind in enumerate((0, 1, 3))]


# ---- 2. single-symbol tables ----------------------------------------------------------------------------------------------------------
def flat(w, h, value=128):
    return np.full((h, w, 3), value, np.uint8)


FLAT = [(24, 24, sub) for sub in SUBS] + [(688, 8, S444)]      # 688 x 8 at 4:4:4: 86 MCUs, the coder's segments hold 85: the last one is one MCU of 6 bits
FLAT_INTERVALS = (0, 1, 5)


# ---- 3. short tails -------------------------------------------------------------------------------------------------------------------
def disturbed_planes(w, h, sub, edits):
    """Flat planes (128) with 8 x 8 blocks overwritten: edits = [(plane 0 / 1 / 2, block x, block y, 8 x 8 array or a value)]."""
    cw = w if sub == S444 else (w + 1) // 2
    ch = (h + 1) // 2 if sub == S420 else h
    planes = [np.full((h, w), 128, np.uint8), np.full((ch, cw), 128, np.uint8), np.full((ch, cw), 128, np.uint8)]
    for p, bx, by, v in edits:
        planes[p][8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = v
    return tuple(planes)


def basis77(amp: int) -> np.ndarray:
    """An 8 x 8 block whose DCT is (almost) the single coefficient (7, 7) -- zigzag 63 -- of value 4 amp: the block ends without an
    EOB, in the amplitude bits of that coefficient."""
    c = np.cos((2 * np.arange(8) + 1) * 7 * np.pi / 16)
    return np.clip(128 + np.rint(amp * np.outer(c, c)), 0, 255).astype(np.uint8)


def ramp(step: int) -> np.ndarray:
    """An 8 x 8 block that rises by `step` per column around 128: a few AC symbols."""
    return np.clip(128 + np.rint(step * (np.arange(8) - 3.5))[None, :].repeat(8, 0), 0, 255).astype(np.uint8)


# Both short tails exist at 4:4:4 alone: the shortest MCU there is 6 bits, at 4:2:2 it is 8 and at 4:2:0 12 -- never fewer than the
# r <= 7 bits of a padded byte, and a segment that begins inside a byte at phase p completes it with 8 - p <= 7 bits.  And both need an
# interval of two coder segments, the second of one MCU: no restart intervals and S + 1 = 86 MCUs (688 x 8), or the smallest interval
# that has a second segment, Ri = S + 1, over 2 S + 3 = 173 MCUs (1384 x 8): intervals of 85 + 1, 85 + 1 and 1 MCUs.
# The edits were found with the model among flat pictures with a few disturbed blocks (one search per case, pinned here):
#   BORROWED     Y block 1 at 145 (two DC symbols of one size) and a ramp in Cb block 4: the first segment is 537 bits = 1 mod 8, the
#                last MCU 6 bits: the flushed (interval 0) / padded (Ri = 86) byte holds r = 7 bits, one of them the first segment's;
#   AGAINST_FF   quality 97.  Y blocks 1, 3 (130), 5 (132) and 85 (129) make a luma DC table of four symbols in which the last MCU's
#                size 4 has the code 1110; Cr block 84 -- the last block of the first segment -- is basis77(46): it ends in coefficient
#                63 = 31, five 1-bits, no EOB; a ramp in Y block 8 brings the first segment to 589 bits = 5 mod 8.  The byte that
#                straddles the boundary is 11111 + 111: 0xFF, completed by a segment of 13 bits.
SHORT_W = {0: 688, 86: 1384}
BORROWED = dict(quality=90, edits=[(0, 1, 0, 145), (1, 4, 0, ramp(9))])
AGAINST_FF = dict(quality=97, edits=[(0, 1, 0, 130), (0, 3, 0, 130), (0, 5, 0, 132), (0, 85, 0, 129), (2, 84, 0, basis77(46)), (0, 8, 0, ramp(7))])


def short_tail_planes(case, ri):
    return disturbed_planes(SHORT_W[ri], 8, S444, case["edits"])


# ---- 4. the length limit ------------------------------------------------------------------------------------------------------------
# (w, h, synth kind, seed, quality) at 4:2:0: pictures of the project's generator whose merge (step 2) gives lengths beyond 16 -- the
# noise picture in both AC tables, the photo-like one in the luma AC table
LONG_CODES = [(384, 288, 1, 1, 97), (384, 288, 0, 2, 97)]


def fibonacci_counts(depth=40):
    """Counts whose merge is one chain `depth` deep: 1, 2, 4, 7, 12, 20, ... (each the sum of the two before it, plus one, so that no
    merged tree ever ties with a symbol and pairs up elsewhere) on `depth` symbols spread over the table."""
    f = np.zeros(256, np.uint64)
    a, b = 1, 2
    for i in range(depth):
        f[(i * 37) % 256] = a
        a, b = b, a + b + 1
    return f


def count_tables():
    """The count tables of the property tests: Fibonacci-like chains, random tables of several densities and ranges, equal counts, one
    symbol, two symbols, none."""
    rng = np.random.default_rng(5)
    out = [fibonacci_counts(40), fibonacci_counts(60), fibonacci_counts(17)]
    for used, hi in ((256, 2), (256, 1 << 20), (162, 1 << 30), (40, 5), (12, 1 << 16), (3, 9)):
        f = np.zeros(256, np.uint64)
        f[rng.choice(256, used, replace=False)] = rng.integers(1, hi, used, dtype=np.uint64)
        out.append(f)
    f = np.zeros(256, np.uint64)
    f[:200] = np.uint64(2) ** rng.integers(0, 40, 200).astype(np.uint64)       # a wide, skewed range
    out.append(f)
    out.append(np.full(256, 7, np.uint64))
    for used in ((5,), (5, 200), ()):
        f = np.zeros(256, np.uint64)
        f[list(used)] = 3
        out.append(f)
    return out
