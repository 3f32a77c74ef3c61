"""CPU model of the one-scan colour file WITH RESTART INTERVALS (include/jpeg_compression.h) -- TEST INFRASTRUCTURE
ONLY.

Built from interleaved_model's parts: its geometry, prefix, MCU order with pad blocks, symbols and tables.  The oracle's RLE runs per
interval and per component, so every interval starts with all three DC predictors at 0.  An interval's bit string is padded with
1-bits to a byte, stuffed, and followed by RSTn; the last one is flushed with 0-bits and followed by EOI.  Besides the file the model
counts what the device's writer has to get right: padded bytes that came out 0xFF, intervals that needed no padding, 0xFF bytes that
straddle two of the coder's segments inside an interval."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import color_model as cm
import interleaved_model as im


@dataclass(frozen=True)
class Restart:
    file: bytes
    intervals: int
    markers: int                    # RSTn markers written
    pad_ff: int                     # padded bytes that came out 0xFF (and were stuffed)
    aligned: int                    # intervals, the last excluded, that ended on a byte and got no padding
    straddle_ff: int                # 0xFF bytes of an interval that span the boundary of two coder segments at a non-zero phase
    straddle_phases: tuple          # the phases (bit offset of the boundary mod 8) of those
    stuffed: int                    # 0x00 stuffing bytes, those behind padded bytes included
    scan_bits: int                  # coded bits: no pad bits, no flush bits
    segments: int                   # entries of the coder's segment arrays per picture: intervals x segments per interval
    two_segment_intervals: int      # intervals with at least two non-empty coder segments
    max_segment_bits: int           # the longest coder segment


def dri(ri: int) -> bytes:
    return bytes([0xFF, 0xDD, 0x00, 0x04, ri >> 8, ri & 0xFF])


def prefix(w: int, h: int, quality: int, sub: int, ri: int) -> bytes:
    """The one-scan prefix with the DRI segment directly in front of the SOS."""
    p = im.prefix(w, h, quality, sub)
    assert p.endswith(im.SOS3)
    return p[:-len(im.SOS3)] + dri(ri) + im.SOS3


def seg_mcus(sub: int) -> int:
    hs, vs = im.sampling(sub)
    return im.SEG_BLOCKS // (hs * vs + 2)


def interval_count(w: int, h: int, sub: int, ri: int) -> int:
    _, _, _, _, mx, my = im.geometry(w, h, sub)
    return -(-(mx * my) // ri)


def segment_entries(w: int, h: int, sub: int, ri: int) -> int:
    """n x spi: the entries of the coder's segment arrays per picture (before they are rounded up to a multiple of 4)."""
    _, _, _, _, mx, my = im.geometry(w, h, sub)
    m = mx * my
    return -(-m // ri) * -(-min(ri, m) // seg_mcus(sub))


def _coded(oracle, zz: np.ndarray, chroma: bool):
    """The blocks' symbols coded with the component's tables, DC predictor 0 in front of the first block: value and length per
    symbol, symbols per block."""
    sym, amp, alen, is_dc, counts = im._symbols_by_block(oracle, zz)
    dcc, dcl, acc, acl = im._tables(chroma)
    code = np.where(is_dc, dcc[sym], acc[sym])
    clen = np.where(is_dc, dcl[sym], acl[sym])
    return (code << alen) | (amp & ((1 << alen) - 1)), clen + alen, counts


def _interval_bits(oracle, zy, zcb, zcr, a: int, b: int, ny: int):
    """MCUs [a, b) as one interval: its bits (uint8 0 / 1) and the bit count of each of its MCUs."""
    bpm = ny + 2
    vals, lens, keys = [], [], []
    for comp, zz in enumerate((zy[a * ny:b * ny], zcb[a:b], zcr[a:b])):
        val, length, counts = _coded(oracle, zz, comp > 0)
        blk = np.arange(zz.shape[0])
        key = (blk // ny) * bpm + blk % ny if comp == 0 else blk * bpm + ny + comp - 1
        vals.append(val)
        lens.append(length)
        keys.append(np.repeat(key, counts))
    val, length, key = np.concatenate(vals), np.concatenate(lens), np.concatenate(keys)
    order = np.argsort(key, kind="stable")
    val, length, key = val[order], length[order], key[order]
    total = int(length.sum())
    starts = np.cumsum(length) - length
    idx = np.repeat(np.arange(len(val)), length)
    off = np.arange(total) - starts[idx]
    bits = ((val[idx] >> (length[idx] - 1 - off)) & 1).astype(np.uint8)
    mcu_bits = np.bincount(key // bpm, weights=length, minlength=b - a).astype(np.int64)
    return bits, mcu_bits


def planes_file(oracle, y: np.ndarray, cb: np.ndarray, cr: np.ndarray, quality: int, sub: int, ri: int) -> Restart:
    assert 1 <= ri <= 65535
    h, w = y.shape
    hs, vs, bw, bh, mx, my = im.geometry(w, h, sub)
    ny, m, s = hs * vs, mx * my, seg_mcus(sub)
    lq, cq = cm.scaled_table(cm.LUMA_Q, quality), cm.scaled_table(cm.CHROMA_Q, quality)
    zy, _ = im._mcu_order_luma(cm.plane_zigzag(oracle, y, lq), bw, bh, hs, vs, mx, my)
    zcb, zcr = cm.plane_zigzag(oracle, cb, cq), cm.plane_zigzag(oracle, cr, cq)
    n = -(-m // ri)
    body = bytearray()
    markers = pad_ff = aligned = stuffed = scan_bits = two = longest = 0
    phases = []
    for i in range(n):
        a, b = i * ri, min((i + 1) * ri, m)
        bits, mcu_bits = _interval_bits(oracle, zy, zcb, zcr, a, b, ny)
        scan_bits += len(bits)
        last = i == n - 1
        r = len(bits) % 8
        if r:
            bits = np.r_[bits, np.full(8 - r, 0 if last else 1, np.uint8)]
        elif not last:
            aligned += 1
        by = np.packbits(bits)
        if r and not last and by[-1] == 0xFF:
            pad_ff += 1
        ends = np.cumsum(mcu_bits)                               # the coder's segments: runs of s MCUs from the interval's first
        seg_bits = np.diff(np.r_[0, ends[s - 1::s], ends[-1]]) if (b - a) % s else np.diff(np.r_[0, ends[s - 1::s]])
        assert seg_bits.sum() == ends[-1] and len(seg_bits) == -(-(b - a) // s) and seg_bits.min() >= 14
        two += len(seg_bits) >= 2
        longest = max(longest, int(seg_bits.max()))
        for p in np.cumsum(seg_bits)[:-1]:
            if p % 8 and by[p // 8] == 0xFF:
                phases.append(int(p % 8))
        ff = np.nonzero(by == 0xFF)[0]
        stuffed += len(ff)
        body += np.insert(by, ff + 1, 0).tobytes()
        if not last:
            body += bytes([0xFF, 0xD0 + i % 8])
            markers += 1
    return Restart(prefix(w, h, quality, sub, ri) + bytes(body) + b"\xff\xd9", n, markers, pad_ff, aligned, len(phases), tuple(phases),
                   stuffed, scan_bits, segment_entries(w, h, sub, ri), int(two), longest)


def restart_ycbcr_file(oracle, y, cb, cr, quality: int = 0, sub: int = cm.SUB_420, ri: int = 1) -> Restart:
    """The file of samples that already are Y, Cb and Cr."""
    return planes_file(oracle, np.ascontiguousarray(y), np.ascontiguousarray(cb), np.ascontiguousarray(cr), quality, sub, ri)


def restart_file(oracle, rgb: np.ndarray, quality: int = 0, sub: int = cm.SUB_420, ri: int = 1) -> Restart:
    """The file the library must write for these R, G, B pixels: the planes of interleaved_model.interleaved_file."""
    y = im.m422.luma_plane(rgb)
    cb, cr = im.m422.chroma_planes_422(rgb) if sub == im.m422.SUB_422 else cm.chroma_planes(rgb, sub)
    return planes_file(oracle, y, cb, cr, quality, sub, ri)


def with_dri(plain: bytes, ri: int) -> bytes:
    """Rule 5: the one-scan file `plain` with the DRI segment inserted in front of its SOS."""
    at = plain.index(im.SOS3)
    return plain[:at] + dri(ri) + plain[at:]


def walk_scan(data: bytes):
    """A structural walk of a file's scan that knows nothing of how it was written: -> (markers in order, stuffed 0x00 bytes).  Every
    0xFF of the scan must be followed by 0x00, by an RSTn marker or -- as the file's last two bytes -- by EOI."""
    at = data.index(im.SOS3) + len(im.SOS3)
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
