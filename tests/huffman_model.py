"""CPU model of the one-scan colour file WITH PER-PICTURE OPTIMISED HUFFMAN TABLES (include/jpeg_compression.h) --
TEST INFRASTRUCTURE ONLY.

optimal_table is T.81 K.2 as libjpeg carries it out, with code sizes up to 256 (no error path for long codes).  The file is built from
interleaved_model's and restart_model's parts -- geometry, prefix, DRI, coefficients -- and scan_model's coder in two passes: every
symbol the scan codes with the call's restart interval is counted into four tables (luma DC, luma AC, chroma DC, chroma AC), then coded
with the tables made of the counts.  Besides the file the model keeps what the device's coder and writer have to get right: the counts,
the tables, the bit count of every coder segment, and the short tails of DESIGN.md 4.6.10."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import color_model as cm
import interleaved_model as im
import restart_model as rm
import scan_model as sm

STD_DHT_BYTES = 2 * (33 + 183)                                  # the four Annex K DHT segments
TABLE_IDS = (0x00, 0x10, 0x01, 0x11)                            # luma DC, luma AC, chroma DC, chroma AC


def code_sizes(freq):
    """Steps 1 and 2: size[0..256] of the merge, 0 for unused symbols (index 256: the reserved point)."""
    f = [int(x) for x in freq] + [1]
    assert len(f) == 257 and min(f) >= 0
    size = [0] * 257
    members = {i: [i] for i in range(257) if f[i]}              # tree root -> its symbols
    while True:
        c1 = c2 = -1
        for i in range(257):                                    # least f > 0, the highest index among equals
            if f[i] and (c1 < 0 or f[i] <= f[c1]):
                c1 = i
        for i in range(257):
            if f[i] and i != c1 and (c2 < 0 or f[i] <= f[c2]):
                c2 = i
        if c2 < 0:
            return size
        f[c1] += f[c2]
        f[c2] = 0
        members[c1] += members.pop(c2)
        for s in members[c1]:
            size[s] += 1


def optimal_table(freq):
    """counts f[0..255] -> (BITS[16], HUFFVAL, the largest step-2 size).  All counts zero: an empty table."""
    freq = [int(x) for x in freq]
    size = code_sizes(freq)
    n = [0] * 258
    for s in range(257):
        if size[s]:
            n[size[s]] += 1
    top = max((l for l in range(257) if n[l]), default=0)
    for l in range(top, 16, -1):
        while n[l] > 0:
            j = l - 2
            while n[j] == 0:
                j -= 1
            n[l] -= 2
            n[l - 1] += 1
            n[j + 1] += 2
            n[j] -= 1
    l = max((k for k in range(257) if n[k]), default=0)
    if l:
        n[l] -= 1                                               # the reserved point leaves
    vals = sorted((s for s in range(256) if freq[s]), key=lambda s: (size[s], s))
    assert sum(n[1:17]) == len(vals) and not any(n[17:])
    return n[1:17], vals, top


def dht(bits, vals, tc_th: int) -> bytes:
    n = 19 + len(vals)
    return bytes([0xFF, 0xC4, n >> 8, n & 0xFF, tc_th]) + bytes(bits) + bytes(vals)


def prefix(w: int, h: int, quality: int, sub: int, ri: int, tables) -> bytes:
    """The standard one-scan prefix (with DRI for ri > 0) with its four DHT segments replaced by those of `tables`."""
    std = rm.prefix(w, h, quality, sub, ri) if ri else im.prefix(w, h, quality, sub)
    tail = len(im.SOS3) + (len(rm.dri(ri)) if ri else 0)
    head = len(std) - tail - STD_DHT_BYTES
    assert std[head:head + 5] == b"\xff\xc4\x00\x1f\x00" and std[-tail:] == (rm.dri(ri) if ri else b"") + im.SOS3
    return std[:head] + b"".join(dht(b, v, t) for (b, v, _), t in zip(tables, TABLE_IDS)) + std[-tail:]


@dataclass(frozen=True)
class Optimized:
    file: bytes
    counts: np.ndarray              # int64 [4][256]: luma DC, luma AC, chroma DC, chroma AC
    tables: tuple                   # 4 x (BITS, HUFFVAL, largest step-2 size)
    prefix_len: int
    scan_bits: int                  # coded bits: no pad bits, no flush bits
    stuffed: int                    # 0x00 stuffing bytes, those behind padded bytes included
    intervals: int
    pad_blocks: int
    segment_bits: tuple             # per interval: the bit counts of its coder segments
    borrowed_tails: int             # intervals whose last coder segment has fewer bits than (b0 + bits) & 7: the padded / flushed byte
                                    # begins with bits of the segment in front
    borrowed_pad_ff: int            # ... of which the padded byte came out 0xFF (and was stuffed)
    short_against_ff: int           # coder segments shorter than 14 bits that begin with a 1-bit inside a 0xFF byte begun by the segment in front
    min_segment_bits: int


def planes_file(oracle, y: np.ndarray, cb: np.ndarray, cr: np.ndarray, quality: int, sub: int, ri: int = 0) -> Optimized:
    assert 0 <= ri <= 65535
    h, w = y.shape
    zy, zcb, zcr, pads, ny, m = im.scan_blocks(oracle, y, cb, cr, quality, sub)
    # pass 1: the symbols of every interval (predictors 0 at its start), counted
    intervals = sm.scan_symbols(oracle, zy, zcb, zcr, ny, ri if ri else m)
    counts = np.zeros((4, 256), np.int64)
    for per in intervals:
        for comp, (sym, _, _, is_dc, _) in enumerate(per):
            counts[2 * (comp > 0)] += np.bincount(sym[is_dc], minlength=256)
            counts[2 * (comp > 0) + 1] += np.bincount(sym[~is_dc], minlength=256)
    tables = tuple(optimal_table(c) for c in counts)
    arrays = [sm.code_arrays(b, v) for b, v, _ in tables]
    assert all(length[c > 0].all() for (_, length), c in zip(arrays, counts))      # every symbol of the scan has a code
    # pass 2: coded with the picture's tables
    body, ivs = sm.frame_intervals(*sm.scan_bits(intervals, arrays[:2], arrays[2:], ny), ri if ri else m, rm.seg_mcus(sub))
    assert all(x >= 14 for v in ivs for x in v.seg_bits[:-1])   # only an interval's last segment may be short: what the device's readers of `edge` rely on
    borrowed = [v for v in ivs if v.seg_bits[-1] < v.r]
    against = 0
    for v in ivs:
        b0 = v.bits - v.seg_bits[-1]                            # where the interval's last coder segment begins
        against += bool(len(v.seg_bits) > 1 and v.seg_bits[-1] < 14 and b0 % 8 and v.padded[b0 // 8] == 0xFF)
    pre = prefix(w, h, quality, sub, ri, tables)
    return Optimized(pre + body + b"\xff\xd9", counts, tables, len(pre), sum(v.bits for v in ivs), sum(v.ff for v in ivs), len(ivs), pads,
                     tuple(v.seg_bits for v in ivs), len(borrowed), sum(v.pad_ff for v in borrowed), against,
                     min(min(v.seg_bits) for v in ivs))


def ycbcr_file(oracle, y, cb, cr, quality: int = 0, sub: int = cm.SUB_420, ri: int = 0) -> Optimized:
    """The optimised file of samples that already are Y, Cb and Cr."""
    return planes_file(oracle, np.ascontiguousarray(y), np.ascontiguousarray(cb), np.ascontiguousarray(cr), quality, sub, ri)


def rgb_file(oracle, rgb: np.ndarray, quality: int = 0, sub: int = cm.SUB_420, ri: int = 0) -> Optimized:
    """The optimised file the library must write for these R, G, B pixels: the planes of interleaved_model.interleaved_file."""
    return planes_file(oracle, *sm.planes_of(rgb, sub), quality, sub, ri)


def standard_file(oracle, rgb: np.ndarray, quality: int, sub: int, ri: int = 0) -> bytes:
    """The Annex K file of the same picture and interval."""
    return (cm.memo(rm.restart_file, oracle, rgb, quality, sub, ri) if ri else cm.memo(im.interleaved_file, oracle, rgb, quality, sub)).file


# ---- PIL's files read back: the counts its tables were made of ------------------------------------------------------------------------
def parse_dht(data: bytes):
    """-> {Tc/Th byte: (BITS, HUFFVAL)} of a file's DHT segments in front of its first SOS."""
    out, at = {}, 2
    while data[at + 1] != 0xDA:
        assert data[at] == 0xFF
        n = (data[at + 2] << 8) | data[at + 3]
        if data[at + 1] == 0xC4:
            p = at + 4
            while p < at + 2 + n:
                bits = list(data[p + 1:p + 17])
                out[data[p]] = (bits, list(data[p + 17:p + 17 + sum(bits)]))
                p += 17 + sum(bits)
        at += 2 + n
    return out


def scan_symbol_counts(data: bytes) -> np.ndarray:
    """The symbols of a baseline file's single interleaved scan (three components, Y: tables 0 / 0, chroma: 1 / 1, no restart
    intervals), decoded with the file's own tables and counted: int64 [4][256] in TABLE_IDS' order."""
    tabs = parse_dht(data)
    at = 2
    sof = None
    while data[at + 1] != 0xDA:
        if data[at + 1] == 0xC0:
            sof = data[at + 4:at + 2 + ((data[at + 2] << 8) | data[at + 3])]
        assert data[at + 1] != 0xDD
        at += 2 + ((data[at + 2] << 8) | data[at + 3])
    h, w, ncomp = (sof[1] << 8) | sof[2], (sof[3] << 8) | sof[4], sof[5]
    assert ncomp == 3 and data[at + 4] == 3
    hs, vs = sof[7] >> 4, sof[7] & 15
    assert sof[10] == 0x11 and sof[13] == 0x11
    at += 2 + ((data[at + 2] << 8) | data[at + 3])
    scan = data[at:-2].replace(b"\xff\x00", b"\xff")
    bits = np.unpackbits(np.frombuffer(scan, np.uint8)).tolist()
    lookup = []
    for t in TABLE_IDS:
        lookup.append({(ln, c): s for s, (c, ln) in cm.canonical(*tabs[t]).items()})
    counts = np.zeros((4, 256), np.int64)
    pos = 0

    def symbol(table):
        nonlocal pos
        code = 0
        for ln in range(1, 17):
            code = (code << 1) | bits[pos]
            pos += 1
            s = lookup[table].get((ln, code))
            if s is not None:
                counts[table][s] += 1
                return s
        raise AssertionError("no code word")

    mcus = -(-w // (8 * hs)) * -(-h // (8 * vs))
    for _ in range(mcus):
        for cls in [0] * (hs * vs) + [2, 2]:
            size = symbol(cls)                                   # (symbol moves pos: read it afterwards)
            pos += size
            k = 1
            while k < 64:
                rs = symbol(cls + 1)
                if rs == 0:
                    break
                k += (rs >> 4) + 1
                pos += rs & 15
            assert k <= 64
    assert len(bits) - pos < 8
    return counts
