"""CPU model of the colour file with ONE scan of interleaved MCUs (include/jpeg_compression.h) -- TEST
INFRASTRUCTURE ONLY.

The prefix is the three-scan colour file's up to and including its DHT segments, then one SOS with all three components, one
entropy-coded segment, EOI.  The coefficients are scan_model.plane_zigzag's -- the oracle's stage functions over the Y, Cb and Cr
planes -- put in MCU order with libjpeg's pad blocks (DC of the nearest real block, no AC); the symbols are the oracle's
(oracle_rle, run per component so that each keeps its own DC predictor), coded with the Annex K tables."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import color_model as cm
import color_model_422 as m422
import scan_model as sm

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


def row_interval(w: int, sub: int) -> int:
    """The restart interval "row": the MCUs of one MCU row."""
    return geometry(w, 1, sub)[4]


def segment_count(w: int, h: int, sub: int) -> int:
    """Segments the device's coder cuts the scan into: runs of S = 256 // (hs vs + 2) MCUs."""
    hs, vs, _, _, mx, my = geometry(w, h, sub)
    s = SEG_BLOCKS // (hs * vs + 2)
    return (mx * my + s - 1) // s


def prefix(w: int, h: int, quality: int, sub: int) -> bytes:
    p = m422.prefix_422(w, h, quality) if sub == m422.SUB_422 else cm.color_prefix(w, h, quality, sub)
    assert p.endswith(cm.sos(1))
    return p[:-len(cm.sos(1))] + SOS3


def scan_blocks(oracle, y: np.ndarray, cb: np.ndarray, cr: np.ndarray, quality: int, sub: int):
    """The coefficients of a one-scan file: -> (Y blocks in MCU order with pad blocks, Cb blocks, Cr blocks, pad block count, Y blocks
    per MCU, MCUs)."""
    h, w = y.shape
    hs, vs, bw, bh, mx, my = geometry(w, h, sub)
    assert cb.shape == cr.shape == ((h + 1) // 2 if sub == cm.SUB_420 else h, w if sub == cm.SUB_444 else (w + 1) // 2)
    lq, cq = sm.scaled_table(sm.LUMA_Q, quality), sm.scaled_table(sm.CHROMA_Q, quality)
    zy, pad = sm.mcu_order_luma(sm.plane_zigzag(oracle, y, lq), bw, bh, hs, vs, mx, my)
    zcb, zcr = sm.plane_zigzag(oracle, cb, cq), sm.plane_zigzag(oracle, cr, cq)
    assert zcb.shape[0] == zcr.shape[0] == mx * my
    return zy, zcb, zcr, int(pad.sum()), hs * vs, mx * my


def planes_file(oracle, y: np.ndarray, cb: np.ndarray, cr: np.ndarray, quality: int, sub: int) -> Interleaved:
    h, w = y.shape
    zy, zcb, zcr, pads, ny, m = scan_blocks(oracle, y, cb, cr, quality, sub)
    (per,) = sm.scan_symbols(oracle, zy, zcb, zcr, ny, m)
    zrl, dc_size = [0, 0], [0, 0]
    for comp, (sym, _, _, is_dc, _) in enumerate(per):
        zrl[comp > 0] += int(np.count_nonzero((sym == 0xF0) & ~is_dc))
        dc_size[comp > 0] = max(dc_size[comp > 0], int(sym[is_dc].max()))
    scan, (whole,) = sm.frame_intervals(*sm.scan_bits([per], sm.std_tables(False), sm.std_tables(True), ny), m, m)
    no_eob = sum(int(np.count_nonzero(zz[:, 63])) for zz in (zy, zcb, zcr))
    return Interleaved(prefix(w, h, quality, sub) + scan + b"\xff\xd9", pads, zrl[0], zrl[1], no_eob, dc_size[0], dc_size[1], whole.ff,
                       whole.bits)


def interleaved_ycbcr_file(oracle, y, cb, cr, quality: int = 0, sub: int = cm.SUB_420) -> Interleaved:
    """The interleaved file of samples that already are Y, Cb and Cr: coded as given."""
    return planes_file(oracle, np.ascontiguousarray(y), np.ascontiguousarray(cb), np.ascontiguousarray(cr), quality, sub)


def interleaved_file(oracle, rgb: np.ndarray, quality: int = 0, sub: int = cm.SUB_420) -> Interleaved:
    """The interleaved file the library must write for these R, G, B pixels: the planes the three-scan path derives, in one scan."""
    return planes_file(oracle, *sm.planes_of(rgb, sub), quality, sub)


def three_scan_file(oracle, rgb: np.ndarray, quality: int, sub: int) -> bytes:
    """The three-scan model file of the same picture."""
    if sub == m422.SUB_422:
        return cm.memo(m422.color_file_422, oracle, cm.write_bmp(rgb), quality)
    return cm.memo(cm.rgb_file, oracle, rgb, quality, sub)
