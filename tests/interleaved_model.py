"""CPU model of the colour file with ONE scan of interleaved MCUs (include/jpeg_compression.h) -- TEST
INFRASTRUCTURE ONLY.

The prefix is the three-scan colour file's up to and including its DHT segments, then one SOS with all three components, one
entropy-coded segment, EOI.  The coefficients are color_model.plane_zigzag's -- the oracle's stage functions over the Y, Cb and Cr
planes -- put in MCU order with libjpeg's pad blocks (DC of the nearest real block, no AC); the symbols are the oracle's
(oracle_rle, run per component so that each keeps its own DC predictor), coded with the Annex K tables."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import color_model as cm
import color_model_422 as m422

SOS3 = bytes([0xFF, 0xDA, 0x00, 0x0C, 0x03, 0x01, 0x00, 0x02, 0x11, 0x03, 0x11, 0x00, 0x3F, 0x00])
SEG_BLOCKS = 256                                                # blocks a segment of the device's coder holds at most


@dataclass(frozen=True)
class Interleaved:
    file: bytes
    pad_blocks: int                 # Y blocks beyond the picture's block grid
    zrl_luma: int                   # ZRL symbols coded with the luma / the chroma AC table
    zrl_chroma: int
    no_eob_blocks: int              # blocks whose zigzag 63 is non-zero
    dc_size_luma: int               # the largest DC size used
    dc_size_chroma: int
    stuffed: int                    # 0x00 bytes behind 0xFF bytes of the scan
    scan_bits: int                  # bits of the entropy-coded segment before stuffing and flush


def sampling(sub: int):
    """(hs, vs) of the Y component."""
    return {cm.SUB_444: (1, 1), cm.SUB_420: (2, 2), m422.SUB_422: (2, 1)}[sub]


def geometry(w: int, h: int, sub: int):
    """-> (hs, vs, bw, bh, mx, my)."""
    hs, vs = sampling(sub)
    bw, bh = (w + 7) // 8, (h + 7) // 8
    return hs, vs, bw, bh, (bw + hs - 1) // hs, (bh + vs - 1) // vs


def segment_count(w: int, h: int, sub: int) -> int:
    """Segments the device's coder cuts the scan into: runs of S = 256 // (hs vs + 2) MCUs."""
    hs, vs, _, _, mx, my = geometry(w, h, sub)
    s = SEG_BLOCKS // (hs * vs + 2)
    return (mx * my + s - 1) // s


def prefix(w: int, h: int, quality: int, sub: int) -> bytes:
    p = m422.prefix_422(w, h, quality) if sub == m422.SUB_422 else cm.color_prefix(w, h, quality, sub)
    assert p.endswith(cm.sos(1))
    return p[:-len(cm.sos(1))] + SOS3


def _mcu_order_luma(zz: np.ndarray, bw: int, bh: int, hs: int, vs: int, mx: int, my: int):
    """The Y blocks in scan order, pad blocks made: int16 [mx my hs vs, 64], and the pad flags."""
    j, i, v, u = np.meshgrid(np.arange(my), np.arange(mx), np.arange(vs), np.arange(hs), indexing="ij")
    bx, by = (i * hs + u).ravel(), (j * vs + v).ravel()
    pad = (bx >= bw) | (by >= bh)
    out = zz[np.minimum(by, bh - 1) * bw + np.minimum(bx, bw - 1)].copy()
    out[pad, 1:] = 0
    return out, pad


def _symbols_by_block(oracle, zz: np.ndarray):
    """color_model._symbols, and the number of symbols of every block."""
    sym, amp, alen, is_dc = cm._symbols(oracle, zz)
    starts = np.nonzero(is_dc)[0]
    counts = np.diff(np.r_[starts, len(sym)])
    assert len(counts) == zz.shape[0]
    return sym, amp, alen, is_dc, counts


def _tables(chroma: bool):
    dc = cm.canonical(cm.DC_CHROMA_BITS if chroma else cm.DC_LUMA_BITS, cm.DC_VALS)
    ac = cm.canonical(cm.AC_CHROMA_BITS if chroma else cm.AC_LUMA_BITS, cm.AC_CHROMA_VALS if chroma else cm.AC_LUMA_VALS)
    t = [np.zeros(256, np.int64) for _ in range(4)]
    for s, (c, ln) in dc.items():
        t[0][s], t[1][s] = c, ln
    for s, (c, ln) in ac.items():
        t[2][s], t[3][s] = c, ln
    return t


def planes_file(oracle, y: np.ndarray, cb: np.ndarray, cr: np.ndarray, quality: int, sub: int) -> Interleaved:
    h, w = y.shape
    hs, vs, bw, bh, mx, my = geometry(w, h, sub)
    ny, bpm = hs * vs, hs * vs + 2
    assert cb.shape == cr.shape == ((h + 1) // 2 if sub == cm.SUB_420 else h, w if sub == cm.SUB_444 else (w + 1) // 2)
    lq, cq = cm.scaled_table(cm.LUMA_Q, quality), cm.scaled_table(cm.CHROMA_Q, quality)
    zy, pad = _mcu_order_luma(cm.plane_zigzag(oracle, y, lq), bw, bh, hs, vs, mx, my)
    zcb, zcr = cm.plane_zigzag(oracle, cb, cq), cm.plane_zigzag(oracle, cr, cq)
    assert zcb.shape[0] == zcr.shape[0] == mx * my
    vals, lens, keys = [], [], []
    zrl = [0, 0]
    dc_size = [0, 0]
    for comp, zz in enumerate((zy, zcb, zcr)):
        chroma = comp > 0
        sym, amp, alen, is_dc, counts = _symbols_by_block(oracle, zz)
        dcc, dcl, acc, acl = _tables(chroma)
        code = np.where(is_dc, dcc[sym], acc[sym])
        clen = np.where(is_dc, dcl[sym], acl[sym])
        vals.append((code << alen) | (amp & ((1 << alen) - 1)))
        lens.append(clen + alen)
        b = np.arange(zz.shape[0])
        key = (b // ny) * bpm + b % ny if comp == 0 else b * bpm + ny + comp - 1      # the block's place in the scan
        keys.append(np.repeat(key, counts))
        zrl[chroma] += int(np.count_nonzero((sym == 0xF0) & ~is_dc))
        dc_size[chroma] = max(dc_size[chroma], int(sym[is_dc].max()))
    val, length, key = np.concatenate(vals), np.concatenate(lens), np.concatenate(keys)
    order = np.argsort(key, kind="stable")                       # the symbols of a block stay in order
    val, length = val[order], length[order]
    total = int(length.sum())
    starts = np.cumsum(length) - length
    idx = np.repeat(np.arange(len(val)), length)
    off = np.arange(total) - starts[idx]
    bits = ((val[idx] >> (length[idx] - 1 - off)) & 1).astype(np.uint8)
    by = np.packbits(bits)                                       # zero-padded to whole bytes
    ff = np.nonzero(by == 0xFF)[0]
    scan = np.insert(by, ff + 1, 0).tobytes()
    no_eob = int(np.count_nonzero(zy[:, 63])) + int(np.count_nonzero(zcb[:, 63])) + int(np.count_nonzero(zcr[:, 63]))
    return Interleaved(prefix(w, h, quality, sub) + scan + b"\xff\xd9", int(pad.sum()), zrl[0], zrl[1], no_eob, dc_size[0], dc_size[1],
                       len(ff), total)


def interleaved_ycbcr_file(oracle, y, cb, cr, quality: int = 0, sub: int = cm.SUB_420) -> Interleaved:
    """The interleaved file of samples that already are Y, Cb and Cr: coded as given."""
    return planes_file(oracle, np.ascontiguousarray(y), np.ascontiguousarray(cb), np.ascontiguousarray(cr), quality, sub)


def interleaved_file(oracle, rgb: np.ndarray, quality: int = 0, sub: int = cm.SUB_420) -> Interleaved:
    """The interleaved file the library must write for these R, G, B pixels: the planes the three-scan path derives, in one scan."""
    y = m422.luma_plane(rgb)
    cb, cr = m422.chroma_planes_422(rgb) if sub == m422.SUB_422 else cm.chroma_planes(rgb, sub)
    return planes_file(oracle, y, cb, cr, quality, sub)


def three_scan_file(oracle, rgb: np.ndarray, quality: int, sub: int) -> bytes:
    """The three-scan model file of the same picture."""
    if sub == m422.SUB_422:
        return cm.memo(m422.color_file_422, oracle, cm.write_bmp(rgb), quality)
    return cm.memo(cm.rgb_file, oracle, rgb, quality, sub)
