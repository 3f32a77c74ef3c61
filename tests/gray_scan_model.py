"""CPU model of the GRAYSCALE file written as a scan of one component, with restart intervals and per-picture optimised Huffman tables
(include/jpeg_compression.h) -- TEST INFRASTRUCTURE ONLY.

Built from the parts the colour models use: color_model.plane_zigzag (the oracle's stage functions over the plane),
interleaved_model._symbols_by_block (the oracle's run/size symbols) and _tables (Annex K), huffman_model.optimal_table / dht (K.2 as libjpeg
carries it out), restart_model.dri.  The MCU is one block; the blocks are coded in raster order; a DC difference is taken against the
block in front, or against 0 at the first block of an interval.  Besides the file the model returns what the device's coder and writer
have to get right: intervals and markers, padded bytes that came out 0xFF, intervals that needed no padding, 0xFF bytes across a
boundary of two coder segments (runs of 256 blocks of one interval), short last segments whose tail borrows from the segment in front,
the extreme segment lengths, stuffed bytes, coded bits, the tables and the counts."""
from __future__ import annotations

import struct
from dataclasses import dataclass

import numpy as np

import color_model as cm
import huffman_model as hm
import interleaved_model as im
import restart_model as rm

SEG_BLOCKS = im.SEG_BLOCKS                                     # blocks of a coder segment
SOS1 = cm.sos(1)
STD_DHT_BYTES = 33 + 183                                       # K.3 and K.5
TABLE_IDS = (0x00, 0x10)


def std_prefix(w: int, h: int, quality: int) -> bytes:
    """The 328-byte prefix of the grayscale entries: SOI, APP0, DQT, SOF0 (one component), DHT 0/0, DHT 1/0, SOS."""
    lq = cm.scaled_table(cm.LUMA_Q, quality)
    out = bytearray(b"\xff\xd8\xff\xe0\x00\x10JFIF\x00\x01\x01\x01\x00\x60\x00\x60\x00\x00")
    out += b"\xff\xdb" + struct.pack(">H", 67) + b"\x00" + bytes(lq[cm.ZIGZAG])
    out += b"\xff\xc0" + struct.pack(">HBHHB", 11, 8, h, w, 1) + bytes([1, 0x11, 0])
    out += hm.dht(cm.DC_LUMA_BITS, cm.DC_VALS, 0x00) + hm.dht(cm.AC_LUMA_BITS, cm.AC_LUMA_VALS, 0x10)
    assert len(out) + len(SOS1) == 328
    return bytes(out) + SOS1


def prefix(w: int, h: int, quality: int, ri: int, tables=None) -> bytes:
    """std_prefix with the DRI segment in front of the SOS for ri > 0 and -- `tables`: 2 x (BITS, HUFFVAL, ...) -- the picture's own DHTs."""
    std = std_prefix(w, h, quality)
    head = len(std) - len(SOS1) - STD_DHT_BYTES
    dhts = std[head:-len(SOS1)] if tables is None else b"".join(hm.dht(t[0], t[1], i) for t, i in zip(tables, TABLE_IDS))
    return std[:head] + dhts + (rm.dri(ri) if ri else b"") + SOS1


def with_dri(plain: bytes, ri: int) -> bytes:
    """The file `plain` with the DRI segment inserted in front of its SOS."""
    at = plain.index(SOS1)
    return plain[:at] + rm.dri(ri) + plain[at:]


def block_count(w: int, h: int) -> int:
    return ((w + 7) // 8) * ((h + 7) // 8)


def segment_entries(w: int, h: int, ri: int) -> int:
    """Entries of the coder's segment arrays per picture: intervals x segments per interval."""
    m = block_count(w, h)
    step = min(ri, m) if ri else m
    return -(-m // step) * -(-step // SEG_BLOCKS)


@dataclass(frozen=True)
class GrayScan:
    file: bytes
    blocks: int
    intervals: int
    markers: int                    # RSTn markers written
    pad_ff: int                     # padded bytes that came out 0xFF (and were stuffed)
    aligned: int                    # intervals, the last excluded, that ended on a byte and got no padding
    straddle_ff: int                # 0xFF bytes across a boundary of two coder segments of one interval at a non-zero phase
    straddle_phases: tuple
    borrowed_tails: int             # last coder segments with fewer bits than the interval's last partial byte: it begins in the segment in front
    min_segment_bits: int
    max_segment_bits: int
    segment_bits: tuple             # per interval: the bit counts of its coder segments
    stuffed: int                    # 0x00 stuffing bytes, those behind padded bytes included
    scan_bits: int                  # coded bits: no pad bits, no flush bits
    counts: np.ndarray              # int64 [2][256]: DC sizes, AC run/size symbols
    tables: tuple                   # 2 x (BITS, HUFFVAL, largest length before limiting); the Annex K tables when not optimised
    prefix_len: int


def _dc_symbols(dc: np.ndarray, step: int):
    """DC values in scan order, predictor 0 at every `step`-th block -> (size, amplitude bits) per block (T.81 F.1.2.1)."""
    prev = np.r_[0, dc[:-1]]
    prev[::step] = 0
    diff = dc - prev
    size = np.zeros(len(dc), np.int64)
    mag = np.abs(diff)
    while mag.any():
        size += mag > 0
        mag >>= 1
    amp = np.where(diff < 0, diff - 1, diff) & ((1 << size) - 1)
    return size, amp


def plane_file(oracle, plane: np.ndarray, quality: int = 0, ri: int = 0, optimized: bool = False) -> GrayScan:
    assert 0 <= ri <= 65535 and plane.ndim == 2 and plane.dtype == np.uint8
    h, w = plane.shape
    zz = cm.plane_zigzag(oracle, np.ascontiguousarray(plane), cm.scaled_table(cm.LUMA_Q, quality))
    m = zz.shape[0]
    assert m == block_count(w, h)
    step = min(ri, m) if ri else m
    sym, amp, alen, is_dc, nsym = im._symbols_by_block(oracle, zz)
    sym, amp, alen = sym.copy(), amp.copy(), alen.copy()
    size, dc_amp = _dc_symbols(zz[:, 0].astype(np.int64), m)
    assert np.array_equal(sym[is_dc], size) and np.array_equal(amp[is_dc] & ((1 << size) - 1), dc_amp)   # one interval: the oracle's own DC symbols
    size, dc_amp = _dc_symbols(zz[:, 0].astype(np.int64), step)
    sym[is_dc], alen[is_dc], amp[is_dc] = size, size, dc_amp
    counts = np.stack([np.bincount(sym[is_dc], minlength=256), np.bincount(sym[~is_dc], minlength=256)]).astype(np.int64)
    if optimized:
        tables = tuple(hm.optimal_table(c) for c in counts)
        (dcc, dcl), (acc, acl) = (hm.code_arrays(b, v) for b, v, _ in tables)
    else:
        tables = ((cm.DC_LUMA_BITS, cm.DC_VALS, 9), (cm.AC_LUMA_BITS, list(cm.AC_LUMA_VALS), 16))
        dcc, dcl, acc, acl = im._tables(False)
    clen = np.where(is_dc, dcl[sym], acl[sym])
    assert clen.min() >= 1
    val = (np.where(is_dc, dcc[sym], acc[sym]) << alen) | (amp & ((1 << alen) - 1))
    length = clen + alen
    total = int(length.sum())
    starts = np.cumsum(length) - length
    idx = np.repeat(np.arange(len(val)), length)
    off = np.arange(total) - starts[idx]
    allbits = ((val[idx] >> (length[idx] - 1 - off)) & 1).astype(np.uint8)
    block_bits = np.bincount(np.repeat(np.arange(m), nsym), weights=length, minlength=m).astype(np.int64)
    block_end = np.cumsum(block_bits)

    n = -(-m // step)
    body = bytearray()
    markers = pad_ff = aligned = stuffed = borrowed = 0
    phases, seg_all = [], []
    for i in range(n):
        a, b = i * step, min((i + 1) * step, m)
        lo = int(block_end[a - 1]) if a else 0
        bits = allbits[lo:int(block_end[b - 1])]
        last = i == n - 1
        r = len(bits) % 8
        if r:
            bits = np.r_[bits, np.full(8 - r, 0 if last else 1, np.uint8)]
        elif not last:
            aligned += 1
        by = np.packbits(bits)
        if r and not last and by[-1] == 0xFF:
            pad_ff += 1
        ends = block_end[a:b] - lo
        cuts = np.r_[ends[SEG_BLOCKS - 1::SEG_BLOCKS], ends[-1]] if (b - a) % SEG_BLOCKS else ends[SEG_BLOCKS - 1::SEG_BLOCKS]
        seg_bits = np.diff(np.r_[0, cuts])
        assert seg_bits.sum() == ends[-1] and len(seg_bits) == -(-(b - a) // SEG_BLOCKS)
        assert all(int(x) >= 512 for x in seg_bits[:-1])         # only an interval's last segment may be short
        seg_all.append(tuple(int(x) for x in seg_bits))
        if len(seg_bits) > 1 and int(seg_bits[-1]) < r:
            borrowed += 1
        for p in np.cumsum(seg_bits)[:-1]:
            if p % 8 and by[p // 8] == 0xFF:
                phases.append(int(p % 8))
        ff = np.nonzero(by == 0xFF)[0]
        stuffed += len(ff)
        body += np.insert(by, ff + 1, 0).tobytes()
        if not last:
            body += bytes([0xFF, 0xD0 + i % 8])
            markers += 1
    pre = prefix(w, h, quality, ri, tables if optimized else None)
    flat = [x for s in seg_all for x in s]
    return GrayScan(pre + bytes(body) + b"\xff\xd9", m, n, markers, pad_ff, aligned, len(phases), tuple(phases), borrowed, min(flat), max(flat),
                    tuple(seg_all), stuffed, total, counts, tables, len(pre))


def gray_file(oracle, plane: np.ndarray, quality: int = 0, ri: int = 0, optimized: bool = False) -> GrayScan:
    """plane_file through color_model.memo: one computation per distinct picture and setting in a session."""
    return cm.memo(plane_file, oracle, np.ascontiguousarray(plane), quality, ri, optimized)


def luma(rgb: np.ndarray) -> np.ndarray:
    """The luma plane every entry derives from R, G, B pixels."""
    return cm.model_planes(rgb, cm.SUB_444)[0]


def walk_scan(data: bytes):
    """restart_model.walk_scan for a file with the one-component SOS: -> (markers in order, stuffed 0x00 bytes)."""
    at = data.index(SOS1) + len(SOS1)
    markers, stuffed = [], 0
    while True:
        j = data.find(b"\xff", at)
        assert j >= 0 and j + 1 < len(data), "the scan ends without EOI"
        nxt = data[j + 1]
        if nxt == 0x00:
            stuffed += 1
        elif 0xD0 <= nxt <= 0xD7:
            markers.append(nxt - 0xD0)
        else:
            assert nxt == 0xD9 and j + 2 == len(data), (hex(nxt), j, len(data))
            return markers, stuffed
        at = j + 2
