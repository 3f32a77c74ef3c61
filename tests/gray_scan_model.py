"""CPU model of the GRAYSCALE file written as a scan of one component, with restart intervals and per-picture optimised Huffman tables
(include/jpeg_compression.h) -- TEST INFRASTRUCTURE ONLY.

Built from the parts the colour models use: scan_model's plane_zigzag (the oracle's stage functions over the plane), symbols (the
oracle's run/size symbols), tables, coder and interval framing, huffman_model.optimal_table / dht (K.2 as libjpeg carries it out),
restart_model.dri.  The MCU is one block; the blocks are coded in raster order; a DC difference is taken against the block in front, or
against 0 at the first block of an interval.  Besides the file the model returns what the device's coder and writer
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
import scan_model as sm

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


def plane_file(oracle, plane: np.ndarray, quality: int = 0, ri: int = 0, optimized: bool = False) -> GrayScan:
    assert 0 <= ri <= 65535 and plane.ndim == 2 and plane.dtype == np.uint8
    h, w = plane.shape
    zz = sm.plane_zigzag(oracle, np.ascontiguousarray(plane), sm.scaled_table(sm.LUMA_Q, quality))
    m = zz.shape[0]
    assert m == block_count(w, h)
    step = min(ri, m) if ri else m
    sym, amp, alen, is_dc, nsym = sm.symbols(oracle, zz)
    size, dc_amp = sm.dc_symbols(zz[:, 0], m)
    assert np.array_equal(sym[is_dc], size) and np.array_equal(amp[is_dc] & ((1 << size) - 1), dc_amp)   # one interval: the oracle's own DC symbols
    size, dc_amp = sm.dc_symbols(zz[:, 0], step)                # ... and against 0 at the first block of every interval
    sym[is_dc], alen[is_dc], amp[is_dc] = size, size, dc_amp
    counts = np.stack([np.bincount(sym[is_dc], minlength=256), np.bincount(sym[~is_dc], minlength=256)]).astype(np.int64)
    if optimized:
        tables = tuple(hm.optimal_table(c) for c in counts)
        dc, ac = (sm.code_arrays(b, v) for b, v, _ in tables)
    else:
        tables = ((sm.DC_LUMA_BITS, sm.DC_VALS, 9), (sm.AC_LUMA_BITS, list(sm.AC_LUMA_VALS), 16))
        dc, ac = sm.std_tables(False)
    assert dc[1][counts[0] > 0].all() and ac[1][counts[1] > 0].all()                # every symbol of the scan has a code
    val, length = sm.coded((sym, amp, alen, is_dc), dc, ac)
    block_bits = np.bincount(np.repeat(np.arange(m), nsym), weights=length, minlength=m).astype(np.int64)
    body, ivs = sm.frame_intervals(sm.bit_array(val, length), block_bits, step, SEG_BLOCKS)
    assert all(x >= 512 for v in ivs for x in v.seg_bits[:-1])  # only an interval's last segment may be short
    phases = tuple(p for v in ivs for p in v.straddle_phases)
    pre = prefix(w, h, quality, ri, tables if optimized else None)
    flat = [x for v in ivs for x in v.seg_bits]
    return GrayScan(pre + body + b"\xff\xd9", m, len(ivs), len(ivs) - 1, sum(v.pad_ff for v in ivs), sum(v.aligned for v in ivs), len(phases),
                    phases, sum(len(v.seg_bits) > 1 and v.seg_bits[-1] < v.r for v in ivs), min(flat), max(flat),
                    tuple(v.seg_bits for v in ivs), sum(v.ff for v in ivs), int(length.sum()), counts, tables, len(pre))


def gray_file(oracle, plane: np.ndarray, quality: int = 0, ri: int = 0, optimized: bool = False) -> GrayScan:
    """plane_file through color_model.memo: one computation per distinct picture and setting in a session."""
    return cm.memo(plane_file, oracle, np.ascontiguousarray(plane), quality, ri, optimized)
