"""CPU model of the progressive colour file WITH SUCCESSIVE APPROXIMATION (include/jpeg_compression.h) -- TEST
INFRASTRUCTURE ONLY.

The ten scans of libjpeg's jpeg_simple_progression for YCbCr over progressive_model's coefficients, MCU order, pad blocks and predictors;
progressive_runs_model's run rule (a run never crosses a multiple of SEG_BLOCKS blocks) and first-scan walk, over point-transformed
values; huffman_model's table construction, a table per scan; scan_model's packer.  A scan is the concatenation of per-block strings in
block order: a block's head, the symbol of the run it starts, its tail.  Besides the file the model returns the counters the GPU tests
claim to exercise."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import color_model as cm
import huffman_model as hm
import interleaved_model as im
import progressive_model as pm
import progressive_runs_model as prm
import scan_model as sm

# (components, Ss, Se, Ah, Al, tables in the file's order)
SCRIPT = (((0, 1, 2), 0, 0, 0, 1, (0, 1)), ((0,), 1, 5, 0, 2, (2,)), ((2,), 1, 63, 0, 1, (3,)), ((1,), 1, 63, 0, 1, (4,)),
          ((0,), 6, 63, 0, 2, (5,)), ((0,), 1, 63, 2, 1, (6,)), ((0, 1, 2), 0, 0, 1, 0, ()), ((2,), 1, 63, 1, 0, (7,)),
          ((1,), 1, 63, 1, 0, (8,)), ((0,), 1, 63, 1, 0, (9,)))
SCANS, TABLES = len(SCRIPT), 10
SEG_BLOCKS = pm.SEG_BLOCKS
RAW = -1                                                          # the `symbol` of bits that no table codes


def table_id(table: int) -> int:
    """The Tc/Th byte of table 0 .. 9 in the file's order."""
    if table < 2:
        return table
    comps = next(s[0] for s in SCRIPT if table in s[5])
    return 0x10 if comps == (0,) else 0x11


def sos(scan: int) -> bytes:
    """The SOS segment of scan 1 .. 10."""
    comps, ss, se, ah, al, _ = SCRIPT[scan - 1]
    sel = b"".join(bytes([c + 1, 0x00 if c == 0 else 0x11]) for c in comps)
    return bytes([0xFF, 0xDA, 0x00, 6 + 2 * len(comps), len(comps)]) + sel + bytes([ss, se, (ah << 4) | al])


def sos_parameters(data: bytes):
    """[(component ids, Ss, Se, Ah, Al)] of every SOS of a file, found by a walk over its marker segments."""
    out, at = [], 2
    while data[at + 1] != 0xD9:
        assert data[at] == 0xFF, at
        n = (data[at + 2] << 8) | data[at + 3]
        if data[at + 1] == 0xDA:
            ns = data[at + 4]
            p = at + 5 + 2 * ns
            out.append((tuple(data[at + 5 + 2 * i] for i in range(ns)), data[p], data[p + 1], data[p + 2] >> 4, data[p + 2] & 15))
            at += 2 + n
            while not (data[at] == 0xFF and data[at + 1] != 0x00 and not 0xD0 <= data[at + 1] <= 0xD7):
                at += 1
        else:
            at += 2 + n
    return out


@dataclass(frozen=True)
class Run:
    scan: int                       # 2 .. 10
    start: int                      # the block that codes the run's symbol (the component's raster block order)
    length: int                     # blocks it covers, its starter included
    starter_empty: bool             # the starter is a Z block: the symbol is the first thing of its string
    behind_new_se: bool             # started by a Z block only because the block in front has a new (non-zero) coefficient Se
    cut: bool                       # ended by a multiple of SEG_BLOCKS with a Z block behind it
    covered_bits: int               # correction bits of the blocks it covers behind its starter


@dataclass(frozen=True)
class Successive:
    file: bytes
    counts: np.ndarray              # int64 [10][256] in the file's table order
    tables: tuple                   # 10 x (BITS, HUFFVAL, largest step-2 size)
    header_len: tuple               # [10] bytes in front of every scan's entropy-coded segment (scan 1: the whole head of the file)
    scan_bits: tuple                # [10] coded bits of every scan, before stuffing and flush
    seg_bits: tuple                 # [10] the bits of every segment the device's coder cuts the scan into
    stuffed: tuple                  # [10]
    runs: tuple                     # every Run of the AC scans
    zrl: tuple                      # [10] ZRL symbols
    zrl_with_bits: int              # ZRLs of refinement scans coded with a non-empty B behind them
    multi_zrl_blocks: int           # blocks of refinement scans with two or more ZRLs
    longest_b: int                  # the most correction bits behind one symbol
    longest_tail: int               # the most correction bits behind a block's last new coefficient
    pad_blocks: int

    @property
    def bits(self):
        return sum(self.scan_bits)

    @property
    def cut_runs(self) -> int:
        return sum(r.cut for r in self.runs)

    @property
    def empty_starters(self) -> int:
        return sum(r.starter_empty for r in self.runs)

    @property
    def runs_with_covered_bits(self) -> int:
        return sum(r.covered_bits > 0 for r in self.runs)


def point(zz: np.ndarray, al: int) -> np.ndarray:
    """sign(c) (|c| >> Al): what a first AC scan codes."""
    z = zz.astype(np.int64)
    return np.sign(z) * (np.abs(z) >> al)


def _raw(bits):
    """Correction bits as items of at most 32 bits."""
    out = []
    for i in range(0, len(bits), 32):
        piece = bits[i:i + 32]
        out.append((RAW, int("".join(map(str, piece)), 2), len(piece)))
    return out


def refine_symbols(zz: np.ndarray, ss: int, se: int, al: int, scan: int):
    """One AC refinement scan (T.81 G.1.2.3) -> items (symbol or RAW, bits behind it, their number), the items of every block, the
    runs, and (ZRLs, ZRLs with bits, blocks with two or more ZRLs, longest B, longest tail)."""
    blocks = zz.astype(np.int64).tolist()
    nb = len(blocks)
    heads, tails, z, e = [], [], [], []
    zrl = zrl_bits = multi = longest_b = longest_tail = 0
    for blk in blocks:
        a = [abs(c) >> al for c in blk]
        new = [k for k in range(ss, se + 1) if a[k] == 1]
        last = new[-1] if new else ss - 1
        head, r, b, nz = [], 0, [], 0
        for k in range(ss, last + 1):
            if a[k] == 0:
                r += 1
                continue
            while r > 15:
                head.append((0xF0, 0, 0))
                head += _raw(b)
                zrl, nz, zrl_bits, longest_b = zrl + 1, nz + 1, zrl_bits + bool(b), max(longest_b, len(b))
                b, r = [], r - 16
            if a[k] > 1:
                b.append(a[k] & 1)
                continue
            head.append(((r << 4) | 1, 1 if blk[k] > 0 else 0, 1))
            head += _raw(b)
            longest_b = max(longest_b, len(b))
            b, r = [], 0
        assert not b
        multi += nz >= 2
        tail = [a[k] & 1 for k in range(last + 1, se + 1) if a[k] > 1]
        longest_tail = max(longest_tail, len(tail))
        heads.append(head); tails.append(tail); z.append(not new); e.append(a[se] != 1)
    items, per_block, runs = [], [], []
    for i in range(nb):
        n0 = len(items)
        items += heads[i]
        if e[i] and not (z[i] and i % SEG_BLOCKS != 0 and e[i - 1]):
            r, j = 1, i + 1
            while j < nb and z[j] and j % SEG_BLOCKS != 0:
                r, j = r + 1, j + 1
            n = r.bit_length() - 1
            items.append((n << 4, r - (1 << n), n))
            runs.append(Run(scan, i, r, z[i], bool(z[i] and i % SEG_BLOCKS != 0 and not e[i - 1]), bool(j < nb and j % SEG_BLOCKS == 0 and z[j]),
                            sum(len(t) for t in tails[i + 1:j])))
        items += _raw(tails[i])
        per_block.append(len(items) - n0)
    return np.array(items, np.int64).reshape(-1, 3), np.array(per_block, np.int64), runs, (zrl, zrl_bits, multi, longest_b, longest_tail)


def first_symbols(zz: np.ndarray, ss: int, se: int, al: int, scan: int):
    """A first AC scan: progressive_runs_model's walk over the point-transformed values."""
    syms, per_block, runs, zrl = prm.band_symbols(point(zz, al), ss, se, scan)
    return syms, per_block, [Run(r.scan, r.start, r.length, r.starter_empty, r.behind_nonzero_se, r.cut, 0) for r in runs], (zrl, 0, 0, 0, 0)


def planes_file(oracle, y: np.ndarray, cb: np.ndarray, cr: np.ndarray, quality: int, sub: int) -> Successive:
    h, w = y.shape
    hs, vs, bw, bh, mx, my = im.geometry(w, h, sub)
    ny, bpm = hs * vs, hs * vs + 2
    lq, cq = sm.scaled_table(sm.LUMA_Q, quality), sm.scaled_table(sm.CHROMA_Q, quality)
    planes = [sm.plane_zigzag(oracle, y, lq), sm.plane_zigzag(oracle, cb, cq), sm.plane_zigzag(oracle, cr, cq)]
    zy, pad = sm.mcu_order_luma(planes[0], bw, bh, hs, vs, mx, my)
    dcs = [zz[:, 0].astype(np.int64) for zz in (zy, planes[1], planes[2])]        # in MCU order, pad blocks made

    # ---- pass 1: what every scan codes, its symbols counted ----
    counts = np.zeros((TABLES, 256), np.int64)
    coded, runs, zrl = [], [], []
    zrl_bits = multi = longest_b = longest_tail = 0
    for k, (comps, ss, se, ah, al, tabs) in enumerate(SCRIPT):
        if se == 0 and ah == 0:                                  # the first DC scan: the differences of DC >> Al
            dc = [sm.dc_symbols(d >> al, len(d)) for d in dcs]
            for comp, (size, _) in enumerate(dc):
                counts[tabs[min(comp, 1)]] += np.bincount(size, minlength=256)
            coded.append(dc); zrl.append(0)
        elif se == 0:                                            # the DC refinement scan: bit Al of every DC, no table
            coded.append([(d >> al) & 1 for d in dcs]); zrl.append(0)
        else:
            walk = refine_symbols if ah else first_symbols
            items, per_block, rs, (z, zb, mu, lb, lt) = walk(planes[comps[0]], ss, se, al, k + 1)
            sym = items[:, 0]
            counts[tabs[0]] += np.bincount(sym[sym != RAW], minlength=256)
            coded.append((items, per_block)); runs += rs; zrl.append(z)
            zrl_bits, multi, longest_b, longest_tail = zrl_bits + zb, multi + mu, max(longest_b, lb), max(longest_tail, lt)
    tables = tuple(hm.optimal_table(c) for c in counts)
    arrays = [sm.code_arrays(b, v) for b, v, _ in tables]
    assert all(length[c > 0].all() for (_, length), c in zip(arrays, counts))

    # ---- pass 2: coded with the scans' own tables ----
    scans, scan_bits, seg_bits, stuffed, header_len = [], [], [], [], []
    for k, (comps, ss, se, ah, al, tabs) in enumerate(SCRIPT):
        hdr = (prm.head(w, h, quality, sub) if k == 0 else b"") + b"".join(hm.dht(*tables[t][:2], table_id(t)) for t in tabs) + sos(k + 1)
        if se == 0:
            per_comp = []
            for comp, part in enumerate(coded[k]):
                if ah == 0:
                    (size, amp), (code, ln) = part, arrays[tabs[min(comp, 1)]]
                    per_comp.append(((code[size] << size) | amp, ln[size] + size, np.ones(len(size), np.int64)))
                else:
                    per_comp.append((part, np.ones(len(part), np.int64), np.ones(len(part), np.int64)))
            val, length, mcu_bits = sm.mcu_merge(per_comp, ny)
            segs = pm._segments(mcu_bits, SEG_BLOCKS // bpm)
        else:
            (items, per_block), (code, ln) = coded[k], arrays[tabs[0]]
            sym, extra, elen = items.T
            tabbed = sym != RAW
            s = np.where(tabbed, sym, 0)
            length = np.where(tabbed, ln[s], 0) + elen
            val = (np.where(tabbed, code[s], 0) << elen) | extra
            ends = np.r_[0, np.cumsum(per_block)]
            csum = np.r_[0, np.cumsum(length)]
            segs = pm._segments(csum[ends[1:]] - csum[ends[:-1]], SEG_BLOCKS)
        data, total, ff = sm.pack(val, length)
        scans.append(hdr + data); scan_bits.append(total); stuffed.append(ff); header_len.append(len(hdr)); seg_bits.append(segs)
    return Successive(b"".join(scans) + b"\xff\xd9", counts, tables, tuple(header_len), tuple(scan_bits), tuple(seg_bits), tuple(stuffed),
                      tuple(runs), tuple(zrl), zrl_bits, multi, longest_b, longest_tail, int(pad.sum()))


def ycbcr_file(oracle, y, cb, cr, quality: int = 0, sub: int = cm.SUB_420) -> Successive:
    """The file of samples that already are Y, Cb and Cr: coded as given."""
    return planes_file(oracle, np.ascontiguousarray(y), np.ascontiguousarray(cb), np.ascontiguousarray(cr), quality, sub)


def rgb_file(oracle, rgb: np.ndarray, quality: int = 0, sub: int = cm.SUB_420) -> Successive:
    """The file the library must write for these R, G, B pixels: the planes the other colour paths derive."""
    return planes_file(oracle, *sm.planes_of(rgb, sub), quality, sub)
