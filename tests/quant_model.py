"""CPU model of the tile kernel's quantiser (jpegamd_tile_pipeline.hip, sections 2 to 4) -- TEST INFRASTRUCTURE ONLY, numpy only.

For centred blocks int [n, 64] (raster x * 8 + y, values -128 .. 127) and a table at a quality it evaluates exactly what the kernel
evaluates, site by site:
  * the LUT products cos_lut()[x][u] * cos_lut()[y][v] split into the integer terms hi = round(2^11 K) and lo = round(2^22 (K - hi 2^-11)),
    one accumulator chain per term over the UNCENTRED operand Y = p + 128 scaled by 2^-24 (both chains are exact in float32 in any
    order: integers below 2^24 units, asserted here), ONE float32 add that joins them, dc_off taken off site 0;
  * zc = fma(acc, qmul, qadd) with ONE rounding, fract(zc), the compare fract <= qthr: the flag.  A DC is never flagged (the kernel
    quantises |S| by floor(zc) and puts the sign back);
  * the fast value of an AC site: round-to-nearest-even of acc * qmul (the kernel's fma with 1.5 * 2^23, whose low half is the value).
The fma and the compare are evaluated in float64 and, wherever that could round twice or sits within a float32 step of the threshold,
decided again with exact rational arithmetic.

What comes from the product: the constants its debug entries expose (cos_lut, mfma_consts / chroma_mfma_consts, group_thresholds).
The reference value of a site is the oracle's: oracle.dct_blocks and the oracle's quantiser for the luma table, the chroma pipeline of
tests/color_model.py (plane_zigzag) for the chroma table."""
from __future__ import annotations

from fractions import Fraction
from types import SimpleNamespace

import numpy as np

import color_model as cm

f32, f64 = np.float32, np.float64
ZZ = np.array(cm.ZIGZAG)                      # zigzag position -> raster k
_consts = {}
_split = {}


def _lut_split(jpegamd):
    """(hi, lo) int64 [64 zigzag][64 pixels]: the two integer terms of the LUT-product matrix, rows in zigzag order."""
    if "m" not in _split:
        lut = jpegamd.cos_lut().astype(f64)
        K = np.zeros((64, 64))
        for z in range(64):
            u, v = divmod(int(ZZ[z]), 8)
            K[z] = np.outer(lut[:, u], lut[:, v]).reshape(64)            # exact: 24 x 24 bits
        hi = np.rint(K * 2048.0)
        lo = np.rint((K - hi / 2048.0) * 4194304.0)
        assert np.abs(hi).max() <= 2048 and np.abs(lo).max() <= 1024
        _split["m"] = (hi.astype(np.int64), lo.astype(np.int64))
    return _split["m"]


def table_of(oracle, table: str, quality: int) -> np.ndarray:
    """uint8 [64] raster: the quantisation table as the checker derives it."""
    return oracle.quant_table(quality if quality > 0 else 50) if table == "luma" else cm.scaled_table(cm.CHROMA_Q, quality)


def consts(jpegamd, table: str, quality: int):
    """The kernel's constants for (table, quality), by zigzag position; grp_thr / lo_bound [4][2]; flag_thr [4][2] = the largest qthr
    of the group-half (quant_consts.cpp derives it so, in float32: a maximum is exact)."""
    key = (table, quality)
    if key not in _consts:
        chroma = table == "chroma"
        assert table in ("luma", "chroma")
        c = jpegamd.chroma_mfma_consts(quality) if chroma else jpegamd.mfma_consts(quality)
        thr, lob = jpegamd.group_thresholds(quality, with_lo_bound=True, chroma=chroma)
        qthr = c["qthr"].astype(f32)
        _consts[key] = SimpleNamespace(qmul=c["qmul"].astype(f32), qadd=c["qadd"].astype(f32), qthr=qthr, dc_off=f32(c["dc_off"]),
                                       scale=float(c["scale"]), grp_thr=thr.astype(f32), lo_bound=lob.astype(f32),
                                       flag_thr=qthr.reshape(4, 2, 8).max(axis=2))
    return _consts[key]


def _round_f32(x: Fraction) -> np.float32:
    """Round-to-nearest-even of an exact rational to float32."""
    g = f32(float(x))                                                   # within a step of the answer
    cands = sorted({float(np.nextafter(g, f32(-np.inf))), float(g), float(np.nextafter(g, f32(np.inf)))})
    best = min(cands, key=lambda c: (abs(Fraction(c) - x), int(f32(c).view(np.uint32)) & 1))
    return f32(best)


def fma32(a, b, c, stats=None):
    """fl32(a * b + c) with ONE rounding, elementwise over float32 arrays.  The product is exact in float64 (24 x 24 bits); the float64
    sum may round, and a second rounding to float32 can then land on the wrong side only where the float64 sum sits on a float32
    rounding boundary: within one float64 step of a boundary the element is decided with exact rational arithmetic."""
    a, b, c = (np.asarray(t, f32).astype(f64) for t in np.broadcast_arrays(a, b, c))
    s = a * b + c
    r = s.astype(f32)
    r64 = r.astype(f64)
    up, dn = np.nextafter(r, f32(np.inf)).astype(f64), np.nextafter(r, f32(-np.inf)).astype(f64)
    tol = 2.0 * np.spacing(np.abs(s))
    near = (np.abs(s - 0.5 * (r64 + up)) <= tol) | (np.abs(s - 0.5 * (r64 + dn)) <= tol)
    p = a * b
    t = s - p
    near &= ((p - (s - t)) + (c - t)) != 0.0                           # (an exact float64 sum -- Knuth's two-sum leaves no error -- was rounded once)
    idx = np.argwhere(near)
    for i in map(tuple, idx):
        r[i] = _round_f32(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
    if stats is not None:
        stats["fma_exact"] = stats.get("fma_exact", 0) + len(idx)
    return r


def fract_le(zc, thr, stats=None):
    """fract(zc) <= thr as the kernel compares them (float32 operands).  fract = zc - floor(zc) is exact in float64 whenever it is
    anywhere near a threshold (a fraction that small is a multiple of zc's float32 step); within one float32 step of the threshold the
    compare is made with exact rational arithmetic."""
    zc64, thr64 = np.asarray(zc, f32).astype(f64), np.broadcast_to(np.asarray(thr, f32), np.shape(zc)).astype(f64)
    fr = zc64 - np.floor(zc64)
    le = fr <= thr64
    idx = np.argwhere(np.abs(fr - thr64) <= np.spacing(thr64.astype(f32)).astype(f64))
    for i in map(tuple, idx):
        x = Fraction(float(zc64[i]))
        le[i] = (x - (x.numerator // x.denominator)) <= Fraction(float(thr64[i]))
    if stats is not None:
        stats["cmp_exact"] = stats.get("cmp_exact", 0) + len(idx)
    return le


def accumulate(jpegamd, blocks):
    """-> (acc float32 [n, 64], hi float32 [n, 64]) by zigzag position: the joined accumulator (before dc_off) and the hi chain alone."""
    P = np.asarray(blocks, np.int64).reshape(-1, 64)
    assert P.min(initial=0) >= -128 and P.max(initial=0) <= 127
    hi_i, lo_i = _lut_split(jpegamd)
    Y = P + 128
    Yf = Y.astype(f64)                                                  # (float64 matrix products of integers below 2^35: exact, and fast)
    sh, sl = (Yf @ hi_i.T.astype(f64)).astype(np.int64), (Yf @ lo_i.T.astype(f64)).astype(np.int64)      # the chains, in their units (2^-24 and 2^-35)
    assert np.abs(sh[:, 1:]).max(initial=0) < 1 << 24 and np.abs(sl).max(initial=0) < 1 << 24 and (sh[:, 0] % 2048 == 0).all()
    hi, lo = sh.astype(f64) * 2.0 ** -24, sl.astype(f64) * 2.0 ** -35   # exact float32 values
    assert np.array_equal(hi.astype(f32).astype(f64), hi) and np.array_equal(lo.astype(f32).astype(f64), lo)
    return (hi + lo).astype(f32), hi.astype(f32)                        # (the float64 sum is exact: 36 bits at most) -> one rounding


def reference(oracle, blocks, table: str, quality: int):
    """-> (ref int64 [n, 64] by zigzag position, tie bool [n, 64]): the checker's quantised values, and where |r / q| ends in exactly .5."""
    P = np.asarray(blocks, np.int64).reshape(-1, 64)
    n = len(P)
    qt = np.ascontiguousarray(table_of(oracle, table, quality), np.uint8)
    d = oracle.dct_blocks(P.reshape(n, 8, 8).astype(np.int8))
    if table == "luma":
        zz = oracle.quantise_blocks(d, qt)
    else:
        zz = cm.plane_zigzag(oracle, (P + 128).astype(np.uint8).reshape(n * 8, 8), qt)
    # (the tie marks divide in float32 here, as quantization.c does, rather than asking the oracle's quantiser: they only SELECT
    #  fixtures and label events; every value that a test compares is the oracle's own)
    t = np.abs(d.reshape(n, 64)[:, ZZ] / qt[ZZ].astype(f32)[None, :]).astype(f32)
    return zz.astype(np.int64), (t - np.floor(t)) == f32(0.5)


def evaluate(jpegamd, oracle, blocks, table: str, quality: int, stats=None):
    """The model of n blocks.  Every per-site array is by ZIGZAG position z (lane half h = (z >> 3) & 1, group G = z >> 4, site 8 G + (z & 7)).
      flags   bool [n, 64]     the site takes the exact-order fallback
      mask    uint64 [n]       the same as bits by RASTER k (the layout of jpegamd_debug_stages' exact_mask)
      hi_max  float32 [n,4,2]  the hi chain's largest |acc| per (group, lane half): what group_alive compares with grp_thr
      fract   float64 [n, 64]  fract(zc) (exact wherever it is near a threshold): what the min tree and the flag_thr ballot see
      fast    int64 [n, 64]    the fast path's value
      ref     int64 [n, 64]    the reference's value;  tie: |r / q| ends in exactly .5
      value   int64 [n, 64]    what the kernel must write: ref where flagged, fast elsewhere"""
    c = consts(jpegamd, table, quality)
    acc, hi = accumulate(jpegamd, blocks)
    n = len(acc)
    acc[:, 0] = (acc[:, 0].astype(f64) - f64(c.dc_off)).astype(f32)
    a = acc.copy()
    a[:, 0] = np.abs(acc[:, 0])                                          # the DC lanes quantise |S|
    zc = fma32(a, c.qmul[None, :], c.qadd[None, :], stats)
    flags = fract_le(zc, c.qthr[None, :], stats)
    flags[:, 0] = False
    fract = zc.astype(f64) - np.floor(zc.astype(f64))
    fract[:, 0] = 1.0                                                    # (the kernel sets the DC lanes' fraction to 1.0: never at or below a threshold)
    fast = np.rint(acc.astype(f64) * c.qmul.astype(f64)[None, :]).astype(np.int64)     # exact product, one rounding to the integer grid
    fast[:, 0] = np.floor(zc[:, 0].astype(f64)).astype(np.int64) * np.where(acc[:, 0] < 0, -1, 1)
    fast[:, 8] = np.floor(zc[:, 8].astype(f64)).astype(np.int64)       # site 0 of the lanes h == 1 keeps the floor as well (one code path with the DC)
    ref, tie = reference(oracle, blocks, table, quality)
    mask = np.zeros(n, np.uint64)
    for z in range(1, 64):
        mask |= flags[:, z].astype(np.uint64) << np.uint64(ZZ[z])
    return SimpleNamespace(flags=flags, mask=mask, hi_max=np.abs(hi).reshape(n, 4, 2, 8).max(axis=3), fract=fract, fast=fast, ref=ref, tie=tie,
                           value=np.where(flags, ref, fast), consts=c)


def plane_blocks(plane) -> np.ndarray:
    """uint8 [H, W] -> centred blocks int64 [NB, 64] in raster block order, the plane edge-replicated to multiples of 8 (every block
    of the padded picture is an active block of some tile)."""
    h, w = plane.shape
    ph, pw = (h + 7) & ~7, (w + 7) & ~7
    p = np.pad(plane, ((0, ph - h), (0, pw - w)), mode="edge").astype(np.int64) - 128
    return p.reshape(ph // 8, 8, pw // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)


_planes = {}


def plane_model(jpegamd, oracle, plane, table: str, quality: int):
    """evaluate() over the blocks of a plane, once per distinct (plane, table, quality)."""
    key = (plane.tobytes(), plane.shape, table, quality)
    if key not in _planes:
        _planes[key] = evaluate(jpegamd, oracle, plane_blocks(plane), table, quality)
    return _planes[key]


def dead_groups(m, c=None):
    """bool [n, 4]: every hi sum of the group, in both lane halves, is strictly below grp_thr (a tile of such blocks skips the group)."""
    c = c or m.consts
    return (m.hi_max < c.grp_thr[None]).all(axis=2)

