"""Pictures for the colour edge tests (tests/test_gpu_color_edges.py) -- TEST INFRASTRUCTURE ONLY.

  * rgb_for_plane: RGB pixels whose Cb (or Cr) plane is exactly a chosen 8-bit plane, at 4:4:4 or 4:2:0.  With R = G = g,
    Cb = (32768 - 128 g + 128 B) >> 8 = 128 + floor((B - g) / 2); with G = B = g, Cr = 128 + floor((R - g) / 2).  At 4:2:0 each
    sample covers a 2 x 2 pixel group of equal values, and (4 v + 2) >> 2 = v.
  * extreme_blocks: the blocks that push the transform's subnormal matrix operand hardest (test_gpu_edges.py).
  * symbol_plane: a chroma plane whose scan holds every DC size, every AC size, every run, ZRLs, EOBs and a block without EOB.
  * tie_plane: a chroma plane with coefficients next to rounding ties (the exact-order fallback).
Checked on the CPU in tests/test_color_host.py."""
from __future__ import annotations

import numpy as np

import color_model as cm
import scan_model as sm

SYMBOL_QUALITY = 96          # chroma steps: 1 at DC, zigzag 1 and 2 (DC size 11, AC size 10), >= 2 elsewhere (rounding noise stays 0)
TIE_QUALITY = 100            # chroma steps 1: the widest guard band


def rgb_for_plane(target: np.ndarray, which: str, sub: int, base: np.ndarray | None = None, shape=None) -> np.ndarray:
    """uint8 [H, W, 3] (R, G, B) whose `which` ('cb' or 'cr') plane is `target` (uint8 [ch, cw]).  `base` (uint8, plane-sized)
    picks the free grey level where it can (clamped to what the target allows); `shape` (H, W) crops a 4:2:0 picture to odd
    sizes whose chroma plane is still `target`."""
    t = target.astype(np.int64)
    d = np.maximum(2 * (t - 128), -255)                              # the other channel minus g: floor(d / 2) = t - 128
    lo, hi = np.maximum(0, -d), np.minimum(255, 255 - d)
    g = np.clip(base.astype(np.int64) if base is not None else 128, lo, hi)
    other = g + d
    rgb = np.zeros(t.shape + (3,), np.int64)
    rgb[..., 1] = g
    if which == "cb":
        rgb[..., 0], rgb[..., 2] = g, other
    elif which == "cr":
        rgb[..., 0], rgb[..., 2] = other, g
    else:
        raise ValueError(which)
    if sub == cm.SUB_420:
        rgb = rgb.repeat(2, axis=0).repeat(2, axis=1)
    if shape is not None:
        rgb = rgb[:shape[0], :shape[1]]
    return rgb.astype(np.uint8)


def layout_blocks(blocks, per_row: int, fill: int = 128) -> np.ndarray:
    """8 x 8 blocks, row-major, `per_row` to a block row (the last row padded with flat `fill` blocks)."""
    rows = (len(blocks) + per_row - 1) // per_row
    p = np.full((rows * 8, per_row * 8), fill, np.uint8)
    for i, b in enumerate(blocks):
        p[(i // per_row) * 8:(i // per_row) * 8 + 8, (i % per_row) * 8:(i % per_row) * 8 + 8] = b
    return p


def extreme_blocks(lut: np.ndarray):
    """For each of the 64 basis functions of `lut` (COS_LUT[x][u]) the block that is 255 where it is positive and 0 elsewhere, its
    complement and two low-contrast companions; all-white, all-black, checkerboards, single bright / dark pixels, random 0 / 255."""
    lut = lut.astype(np.float64)
    blocks = []
    for k in range(64):
        u, v = divmod(k, 8)
        pos = np.outer(lut[:, u], lut[:, v]) > 0
        blocks += [np.where(pos, 255, 0), np.where(pos, 0, 255), np.where(pos, 255, 1), np.where(pos, 128, 127)]
    blocks += [np.full((8, 8), 255), np.zeros((8, 8), int), (np.indices((8, 8)).sum(0) % 2) * 255, (np.indices((8, 8))[0] % 2) * 255]
    for p in ((0, 0), (7, 7), (3, 4)):
        b = np.zeros((8, 8), int); b[p] = 255; blocks.append(b)
        b = np.full((8, 8), 255); b[p] = 0; blocks.append(b)
    rng = np.random.default_rng(4)
    blocks += [rng.choice([0, 255], size=(8, 8)) for _ in range(58)]
    return blocks


def extreme_plane(lut: np.ndarray) -> np.ndarray:
    """extreme_blocks laid out 40 to a block row (320 pixels: a full tile and a ragged one per block row)."""
    return layout_blocks(extreme_blocks(lut), 40)


# ---- chroma symbol coverage ---------------------------------------------------------------------------------------------
def basis() -> np.ndarray:
    """[64 raster k = 8 v + u, 8 y, 8 x]: the orthonormal 2-D DCT basis."""
    c = np.array([np.sqrt(0.5)] + [1.0] * 7)
    x = np.arange(8)
    cos = np.cos((2 * x[None, :] + 1) * np.arange(8)[:, None] * np.pi / 16)       # [freq, pos]
    return np.array([0.25 * c[v] * c[u] * np.outer(cos[v], cos[u]) for v in range(8) for u in range(8)])


def block_symbols(zz_row: np.ndarray):
    """The AC (run, size) symbols of one zigzag block as RLE bytes ((run << 4) | size, 0xF0 ZRL, 0x00 EOB)."""
    out, run = [], 0
    last = int(np.nonzero(zz_row[1:])[0].max()) + 1 if np.any(zz_row[1:]) else 0
    for i in range(1, last + 1):
        v = int(zz_row[i])
        if v == 0:
            run += 1
            continue
        while run > 15:
            out.append(0xF0)
            run -= 16
        out.append((run << 4) | int(abs(v)).bit_length())
        run = 0
    if last < 63:
        out.append(0x00)
    return out


def _dc_blocks():
    """Flat (and nearly flat) blocks whose DC differences, at a DC step of 1, take every size 0 .. 11 (DC = sum(p - 128) / 8)."""
    flat = [np.full((8, 8), v) for v in (128, 128)]                       # predictor 0, then diff 0: size 0
    for rows in (1, 2, 4):                                                # DC 1, 2, 4 and back to 0: sizes 1, 2, 3
        b = np.full((8, 8), 128)
        b[:rows] = 129
        flat += [b, np.full((8, 8), 128)]
    flat += [np.full((8, 8), v) for v in (129, 131, 135, 143, 159, 191, 255, 0, 255)]   # diffs 8 .. 512 (sizes 4 .. 10), -2040 / 2040 (11)
    return flat


def symbol_plane(oracle, seed: int = 7) -> np.ndarray:
    """A chroma plane (uint8, 8 blocks to a row) whose scan at SYMBOL_QUALITY holds every DC size 0..11, every AC size 1..10, every
    run 0..15, the ZRL, EOBs and a block whose zigzag 63 is non-zero.  Blocks are single / paired basis functions with chosen
    quantised amplitudes; each candidate is checked with the oracle's stage functions and kept when it adds a (run, size) code."""
    table = cm.scaled_table(cm.CHROMA_Q, SYMBOL_QUALITY)
    bank = basis()
    rng = np.random.default_rng(seed)
    specs = []                                                            # [(zigzag position, quantised value), ...] per candidate
    for s in range(1, 11):
        lo, hi = 1 << (s - 1), (1 << s) - 1
        for p in range(1, 64):
            for a in (lo, hi, int(rng.integers(lo, hi + 1))):
                specs.append([(p, a if rng.random() < 0.5 else -a)])
                q = p + 1 + int(rng.integers(0, 16))                     # a second symbol behind it: another run for this size
                if q < 64:
                    specs.append([(p, a), (q, -a)])
    specs.append([(63, 1)])
    specs.append([(1, 3), (63, -1)])
    cands = []
    for sp in specs:
        f = np.zeros(64)
        for p, a in sp:
            f[cm.ZIGZAG[p]] = a * int(table[cm.ZIGZAG[p]])
        px = 128.0 + np.tensordot(f, bank, axes=1)
        if px.min() < 0 or px.max() > 255:
            continue
        cands.append(np.rint(px).astype(np.uint8))
    zz = cm.plane_zigzag(oracle, layout_blocks(cands, 64), table)
    have, keep = set(), []
    for i, b in enumerate(cands):
        syms = set(block_symbols(zz[i]))
        if zz[i, 63] != 0 and "no-eob" not in have:
            syms.add("no-eob")
        if syms - have:
            have |= syms
            keep.append(b)
    return layout_blocks(_dc_blocks() + keep, 8)


def chroma_symbol_coverage(oracle, plane: np.ndarray, quality: int = SYMBOL_QUALITY):
    """-> dict: DC sizes, AC (run, size) codes, runs, AC sizes, ZRL / EOB counts and blocks without EOB of the plane's chroma scan,
    from the model's own symbol list (scan_model.symbols)."""
    zz = cm.plane_zigzag(oracle, plane, cm.scaled_table(cm.CHROMA_Q, quality))
    sym, _, _, is_dc, _ = sm.symbols(oracle, zz)
    ac = sym[~is_dc]
    codes = {int(v) for v in ac if v not in (0x00, 0xF0)}
    return dict(dc_sizes={int(v) for v in sym[is_dc]}, codes=codes, runs={c >> 4 for c in codes}, sizes={c & 15 for c in codes},
                zrl=int((ac == 0xF0).sum()), eob=int((ac == 0x00).sum()), no_eob=int((zz[:, 63] != 0).sum()))


# ---- chroma ties ----------------------------------------------------------------------------------------------------------
def tie_plane(w: int = 256, h: int = 128, seed: int = 3) -> np.ndarray:
    """Uniform noise: at TIE_QUALITY (every chroma step 1) hundreds of its coefficients lie within the guard band of a rounding tie.
    (Flat blocks on DC ties do not serve: the kernel's DC is exact and never flagged.)"""
    return np.random.default_rng(seed).integers(0, 256, (h, w), np.uint8)
