"""CPU model of the progressive colour file WITH END-OF-BAND RUNS AND PER-SCAN OPTIMISED TABLES (include/jpeg_compression.h, DESIGN.md
4.6.13) -- TEST INFRASTRUCTURE ONLY.

progressive_model's coefficients, scan script, SOS segments, MCU order, pad blocks and predictors; huffman_model's table construction;
scan_model's packer.  Two passes: every symbol a scan codes is counted into that scan's table (scan 1 has two: Y DC, and Cb + Cr DC
counted together), then coded with the tables made of the counts.  An AC scan codes end-of-band runs (T.81 G.1.2.2) that never cross a
multiple of SEG_BLOCKS blocks of the component's raster block order.  Besides the file the model returns the counters the GPU tests
claim to exercise."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import color_model as cm
import huffman_model as hm
import interleaved_model as im
import progressive_model as pm
import scan_model as sm

SCANS, TABLES = pm.SCANS, 8
SEG_BLOCKS = pm.SEG_BLOCKS
STD_HEADERS = hm.STD_DHT_BYTES                                   # what the standard progressive file spends on DHT segments


def table_id(table: int) -> int:
    """The Tc/Th byte of table 0 .. 7 in the file's order: Y DC, chroma DC, then the AC tables of scans 2 .. 7."""
    if table < 2:
        return table
    return 0x10 if (table - 2) % 3 == 0 else 0x11


@dataclass(frozen=True)
class Run:
    scan: int                       # 2 .. 7
    start: int                      # the block that codes the run's symbol (the component's raster block order)
    length: int                     # blocks it covers, its starter included
    starter_empty: bool             # the starter has no non-zero coefficient in the band: the run includes its starter
    behind_nonzero_se: bool         # started by an empty block only because the block in front ends with a non-zero coefficient Se
    cut: bool                       # ended by a multiple of SEG_BLOCKS with an empty block behind it


@dataclass(frozen=True)
class ProgressiveRuns:
    file: bytes
    counts: np.ndarray              # int64 [8][256] in the file's table order
    tables: tuple                   # 8 x (BITS, HUFFVAL, largest step-2 size)
    header_len: tuple               # [7] bytes in front of every scan's entropy-coded segment (scan 1: the whole head of the file)
    scan_bits: tuple                # [7] coded bits of every scan, before stuffing and flush
    seg_bits: tuple                 # [7] the bits of every segment the device's coder cuts the scan into
    stuffed: tuple                  # [7]
    runs: tuple                     # every Run of the scans 2 .. 7
    zrl: int                        # ZRL symbols
    pad_blocks: int

    @property
    def bits(self):
        return sum(self.scan_bits)

    @property
    def run_hist(self) -> dict:
        out = {}
        for r in self.runs:
            out[r.length] = out.get(r.length, 0) + 1
        return out

    @property
    def cut_runs(self) -> int:
        return sum(r.cut for r in self.runs)

    @property
    def starters(self) -> tuple:
        """(runs started by a block with non-zero coefficients in the band, runs started by an empty one)."""
        return sum(not r.starter_empty for r in self.runs), sum(r.starter_empty for r in self.runs)


def band_symbols(zz: np.ndarray, ss: int, se: int, scan: int):
    """One AC scan's symbols as (symbol, amplitude bits, amplitude length), the symbols of every block, and its runs."""
    blocks = zz.astype(np.int64).tolist()
    nb = len(blocks)
    e = [blk[se] == 0 for blk in blocks]
    z = [not any(blk[ss:se + 1]) for blk in blocks]
    syms, per_block, runs, zrl = [], [], [], 0
    for i, blk in enumerate(blocks):
        n0, run = len(syms), 0
        for k in range(ss, se + 1):
            c = blk[k]
            if c == 0:
                run += 1
                continue
            while run >= 16:
                syms.append((0xF0, 0, 0))
                zrl += 1
                run -= 16
            size = abs(c).bit_length()
            syms.append(((run << 4) | size, (c if c >= 0 else c - 1) & ((1 << size) - 1), size))
            run = 0
        if e[i] and not (z[i] and i % SEG_BLOCKS != 0 and e[i - 1]):
            r, j = 1, i + 1
            while j < nb and z[j] and j % SEG_BLOCKS != 0:
                r, j = r + 1, j + 1
            n = r.bit_length() - 1
            syms.append((n << 4, r - (1 << n), n))
            runs.append(Run(scan, i, r, z[i], bool(z[i] and i % SEG_BLOCKS != 0 and not e[i - 1]), bool(j < nb and j % SEG_BLOCKS == 0 and z[j])))
        per_block.append(len(syms) - n0)
    return np.array(syms, np.int64).reshape(-1, 3), np.array(per_block, np.int64), runs, zrl


def head(w: int, h: int, quality: int, sub: int) -> bytes:
    """SOI, APP0, DQT, SOF2: the standard progressive prefix without its DHT segments and its SOS."""
    p = pm.prefix(w, h, quality, sub)
    n = len(p) - len(pm.SOS_DC) - STD_HEADERS
    assert p[n:n + 2] == b"\xff\xc4" and p[n - 19:n - 17] == b"\xff\xc2"
    return p[:n]


def planes_file(oracle, y: np.ndarray, cb: np.ndarray, cr: np.ndarray, quality: int, sub: int) -> ProgressiveRuns:
    h, w = y.shape
    hs, vs, bw, bh, mx, my = im.geometry(w, h, sub)
    ny, bpm = hs * vs, hs * vs + 2
    lq, cq = sm.scaled_table(sm.LUMA_Q, quality), sm.scaled_table(sm.CHROMA_Q, quality)
    planes = [sm.plane_zigzag(oracle, y, lq), sm.plane_zigzag(oracle, cb, cq), sm.plane_zigzag(oracle, cr, cq)]
    zy, pad = sm.mcu_order_luma(planes[0], bw, bh, hs, vs, mx, my)

    counts = np.zeros((TABLES, 256), np.int64)
    # ---- pass 1: the symbols of every scan, counted ----
    dc = [sm.dc_symbols(zz[:, 0], len(zz)) for zz in (zy, planes[1], planes[2])]
    for comp, (size, _) in enumerate(dc):
        counts[min(comp, 1)] += np.bincount(size, minlength=256)
    bands, runs, zrl = [], [], 0
    for band, (ss, se) in enumerate(pm.BANDS):
        for comp in range(3):
            scan = 2 + 3 * band + comp
            syms, per_block, rs, z = band_symbols(planes[comp], ss, se, scan)
            counts[scan] += np.bincount(syms[:, 0], minlength=256)
            bands.append((syms, per_block))
            runs += rs
            zrl += z
    tables = tuple(hm.optimal_table(c) for c in counts)
    arrays = [sm.code_arrays(b, v) for b, v, _ in tables]
    assert all(length[c > 0].all() for (_, length), c in zip(arrays, counts))

    # ---- pass 2: coded with the scans' own tables ----
    scans, scan_bits, seg_bits, stuffed, header_len = [], [], [], [], []
    per_comp = []
    for comp, (size, amp) in enumerate(dc):
        code, ln = arrays[min(comp, 1)]
        per_comp.append(((code[size] << size) | amp, ln[size] + size, np.ones(len(size), np.int64)))
    val, length, mcu_bits = sm.mcu_merge(per_comp, ny)
    hdr = head(w, h, quality, sub) + hm.dht(*tables[0][:2], table_id(0)) + hm.dht(*tables[1][:2], table_id(1)) + pm.sos(1)
    data, total, ff = sm.pack(val, length)
    scans.append(hdr + data); scan_bits.append(total); stuffed.append(ff); header_len.append(len(hdr))
    seg_bits.append(pm._segments(mcu_bits, SEG_BLOCKS // bpm))
    for k, (syms, per_block) in enumerate(bands):
        code, ln = arrays[2 + k]
        sym, amp, alen = syms.T
        length = ln[sym] + alen
        data, total, ff = sm.pack((code[sym] << alen) | amp, length)
        hdr = hm.dht(*tables[2 + k][:2], table_id(2 + k)) + pm.sos(2 + k)
        scans.append(hdr + data); scan_bits.append(total); stuffed.append(ff); header_len.append(len(hdr))
        ends = np.r_[0, np.cumsum(per_block)]
        csum = np.r_[0, np.cumsum(length)]
        block_bits = csum[ends[1:]] - csum[ends[:-1]]
        seg_bits.append(pm._segments(block_bits, SEG_BLOCKS))
    return ProgressiveRuns(b"".join(scans) + b"\xff\xd9", counts, tables, tuple(header_len), tuple(scan_bits), tuple(seg_bits),
                           tuple(stuffed), tuple(runs), zrl, int(pad.sum()))


def ycbcr_file(oracle, y, cb, cr, quality: int = 0, sub: int = cm.SUB_420) -> ProgressiveRuns:
    """The file of samples that already are Y, Cb and Cr: coded as given."""
    return planes_file(oracle, np.ascontiguousarray(y), np.ascontiguousarray(cb), np.ascontiguousarray(cr), quality, sub)


def rgb_file(oracle, rgb: np.ndarray, quality: int = 0, sub: int = cm.SUB_420) -> ProgressiveRuns:
    """The file the library must write for these R, G, B pixels: the planes the other colour paths derive."""
    return planes_file(oracle, *sm.planes_of(rgb, sub), quality, sub)


def parse_tables(data: bytes):
    """The DHT tables of a file in the order they appear: [(Tc/Th, BITS, HUFFVAL)]."""
    out, at = [], 2
    while data[at + 1] != 0xD9:
        assert data[at] == 0xFF, at
        n = (data[at + 2] << 8) | data[at + 3]
        if data[at + 1] == 0xC4:
            bits = list(data[at + 5:at + 21])
            assert n == 19 + sum(bits)
            out.append((data[at + 4], bits, list(data[at + 21:at + 21 + sum(bits)])))
        at += 2 + n
        if data[at - 2 - n + 1] == 0xDA:                         # behind SOS: the entropy-coded segment up to the next marker
            while not (data[at] == 0xFF and data[at + 1] != 0x00):
                at += 1
    return out
