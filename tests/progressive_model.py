"""CPU model of the progressive colour file (include/jpeg_compression.h) -- TEST INFRASTRUCTURE ONLY.

Seven scans by spectral selection, Ah = Al = 0: the DC scan of the three components in the MCU order of interleaved_model (pad blocks
made, per-component predictors), then the bands 1..5 and 6..63 of Y, Cb and Cr, each over the component's own block grid in raster
order.  The coefficients are scan_model.plane_zigzag's, the tables Annex K's, the packer scan_model's; a band is coded as T.81 G.1.2.2 with end-of-band runs
of exactly one block (symbol 0x00).  Besides the file the model returns the counters the GPU tests claim to exercise."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import color_model as cm
import interleaved_model as im
import scan_model as sm

BANDS = ((1, 5), (6, 63))
SCANS = 7
SEG_BLOCKS = im.SEG_BLOCKS
SOF_OFFSET = 2 + 18 + 134                                       # SOI, APP0, DQT with two tables
SOS_DC = bytes([0xFF, 0xDA, 0x00, 0x0C, 0x03, 0x01, 0x00, 0x02, 0x11, 0x03, 0x11, 0x00, 0x00, 0x00])


def sos(scan: int) -> bytes:
    """The SOS segment of scan 1 .. 7."""
    if scan == 1:
        return SOS_DC
    comp, (ss, se) = (scan - 2) % 3, BANDS[(scan - 2) // 3]
    return bytes([0xFF, 0xDA, 0x00, 0x08, 0x01, comp + 1, 0x00 if comp == 0 else 0x11, ss, se, 0x00])


@dataclass(frozen=True)
class Progressive:
    file: bytes
    scan_bits: tuple                # [7] coded bits of every scan, before stuffing and flush
    seg_bits: tuple                 # [7] the bits of every segment the device's coder cuts the scan into
    zrl: dict                       # (band 0 / 1, chroma False / True) -> ZRL symbols
    no_end: tuple                   # [2] blocks whose coefficient 5 / 63 is non-zero: no end symbol in that band
    eob_only: tuple                 # [2] blocks whose band is all zero: the end symbol alone
    edge_runs: int                  # blocks with coefficients 4 and 5 zero and coefficient 6 non-zero
    dc_size: int                    # the largest DC size
    stuffed: tuple                  # [7] 0x00 bytes behind 0xFF bytes, scan by scan
    pad_blocks: int                 # Y blocks beyond the picture's block grid (the DC scan alone codes them)

    @property
    def bits(self):
        return sum(self.scan_bits)


def prefix(w: int, h: int, quality: int, sub: int) -> bytes:
    """The one-scan file's prefix with SOF2 for SOF0 and the DC scan's SOS."""
    p = bytearray(im.prefix(w, h, quality, sub))
    assert p[SOF_OFFSET:SOF_OFFSET + 2] == b"\xff\xc0" and p.endswith(im.SOS3)
    p[SOF_OFFSET + 1] = 0xC2
    return bytes(p[:-len(im.SOS3)]) + SOS_DC


def _amp(v: int, size: int) -> int:
    return (v if v >= 0 else v - 1) & ((1 << size) - 1)


def _segments(block_bits, per_segment: int):
    return tuple(int(sum(block_bits[i:i + per_segment])) for i in range(0, len(block_bits), per_segment))


def planes_file(oracle, y: np.ndarray, cb: np.ndarray, cr: np.ndarray, quality: int, sub: int) -> Progressive:
    h, w = y.shape
    hs, vs, bw, bh, mx, my = im.geometry(w, h, sub)
    ny, bpm = hs * vs, hs * vs + 2
    lq, cq = sm.scaled_table(sm.LUMA_Q, quality), sm.scaled_table(sm.CHROMA_Q, quality)
    planes = [sm.plane_zigzag(oracle, y, lq), sm.plane_zigzag(oracle, cb, cq), sm.plane_zigzag(oracle, cr, cq)]
    assert planes[0].shape[0] == bw * bh and planes[1].shape[0] == planes[2].shape[0] == mx * my
    zy, pad = sm.mcu_order_luma(planes[0], bw, bh, hs, vs, mx, my)

    scans, scan_bits, seg_bits, stuffed = [], [], [], []
    # ---- scan 1: the DC differences in MCU order, each component against its own predictor ----
    dc_size, per_comp = 0, []
    for comp, zz in enumerate((zy, planes[1], planes[2])):
        (code, ln), _ = sm.std_tables(comp > 0)
        size, amp = sm.dc_symbols(zz[:, 0], len(zz))
        dc_size = max(dc_size, int(size.max()))
        per_comp.append(((code[size] << size) | amp, ln[size] + size, np.ones(len(zz), np.int64)))
    val, length, mcu_bits = sm.mcu_merge(per_comp, ny)
    data, total, ff = sm.pack(val, length)
    scans.append(data); scan_bits.append(total); stuffed.append(ff)
    seg_bits.append(_segments(mcu_bits, SEG_BLOCKS // bpm))

    # ---- scans 2 .. 7: a band of one component's plane, blocks in raster order ----
    zrl = {(b, c): 0 for b in range(2) for c in (False, True)}
    no_end, eob_only = [0, 0], [0, 0]
    for band, (ss, se) in enumerate(BANDS):
        for comp in range(3):
            code, ln = (t.tolist() for t in sm.std_tables(comp > 0)[1])
            zz = planes[comp].astype(np.int64)
            symbols, block_bits = [], []
            for blk in zz.tolist():
                run, n0 = 0, len(symbols)
                for k in range(ss, se + 1):
                    c = blk[k]
                    if c == 0:
                        run += 1
                        continue
                    while run >= 16:
                        symbols.append((code[0xF0], ln[0xF0]))
                        zrl[(band, comp > 0)] += 1
                        run -= 16
                    size = abs(c).bit_length()
                    rs = (run << 4) | size
                    symbols.append(((code[rs] << size) | _amp(c, size), ln[rs] + size))
                    run = 0
                if blk[se] == 0:
                    symbols.append((code[0x00], ln[0x00]))       # EOB0: an end-of-band run of exactly one block
                else:
                    no_end[band] += 1
                if not any(blk[ss:se + 1]):
                    eob_only[band] += 1
                block_bits.append(sum(s[1] for s in symbols[n0:]))
            data, total, ff = sm.pack(*np.array(symbols, np.int64).T)
            scans.append(data); scan_bits.append(total); stuffed.append(ff)
            seg_bits.append(_segments(block_bits, SEG_BLOCKS))
    every = np.concatenate(planes)
    edge_runs = int(np.count_nonzero((every[:, 4] == 0) & (every[:, 5] == 0) & (every[:, 6] != 0)))
    body = b"".join((sos(k + 1) if k else b"") + scans[k] for k in range(SCANS))      # (bands outer, components inner: the file's order)
    return Progressive(prefix(w, h, quality, sub) + body + b"\xff\xd9", tuple(scan_bits), tuple(seg_bits), zrl, tuple(no_end),
                       tuple(eob_only), edge_runs, dc_size, tuple(stuffed), int(pad.sum()))


def progressive_ycbcr_file(oracle, y, cb, cr, quality: int = 0, sub: int = cm.SUB_420) -> Progressive:
    """The progressive file of samples that already are Y, Cb and Cr: coded as given."""
    return planes_file(oracle, np.ascontiguousarray(y), np.ascontiguousarray(cb), np.ascontiguousarray(cr), quality, sub)


def progressive_file(oracle, rgb: np.ndarray, quality: int = 0, sub: int = cm.SUB_420) -> Progressive:
    """The progressive file the library must write for these R, G, B pixels: the planes the other colour paths derive."""
    return planes_file(oracle, *sm.planes_of(rgb, sub), quality, sub)
