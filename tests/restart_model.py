"""CPU model of the one-scan colour file WITH RESTART INTERVALS (include/jpeg_compression.h) -- TEST INFRASTRUCTURE
ONLY.

Built from interleaved_model's geometry, prefix and coefficients and scan_model's coder.  The oracle's RLE runs per interval and per
component, so every interval starts with all three DC predictors at 0.  An interval's bit string is padded with 1-bits to a byte,
stuffed, and followed by RSTn; the last one is flushed with 0-bits and followed by EOI (scan_model.frame_intervals).  Besides the file
the model counts what the device's writer has to get right: padded bytes that came out 0xFF, intervals that needed no padding, 0xFF
bytes that straddle two of the coder's segments inside an interval."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import color_model as cm
import interleaved_model as im
import scan_model as sm


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


def planes_file(oracle, y: np.ndarray, cb: np.ndarray, cr: np.ndarray, quality: int, sub: int, ri: int) -> Restart:
    assert 1 <= ri <= 65535
    h, w = y.shape
    zy, zcb, zcr, _, ny, _ = im.scan_blocks(oracle, y, cb, cr, quality, sub)
    bits, mcu_bits = sm.scan_bits(sm.scan_symbols(oracle, zy, zcb, zcr, ny, ri), sm.std_tables(False), sm.std_tables(True), ny)
    body, ivs = sm.frame_intervals(bits, mcu_bits, ri, seg_mcus(sub))
    assert min(min(v.seg_bits) for v in ivs) >= 14
    phases = tuple(p for v in ivs for p in v.straddle_phases)
    return Restart(prefix(w, h, quality, sub, ri) + body + b"\xff\xd9", len(ivs), len(ivs) - 1, sum(v.pad_ff for v in ivs),
                   sum(v.aligned for v in ivs), len(phases), phases, sum(v.ff for v in ivs), sum(v.bits for v in ivs),
                   segment_entries(w, h, sub, ri), sum(len(v.seg_bits) >= 2 for v in ivs), max(max(v.seg_bits) for v in ivs))


def restart_ycbcr_file(oracle, y, cb, cr, quality: int = 0, sub: int = cm.SUB_420, ri: int = 1) -> Restart:
    """The file of samples that already are Y, Cb and Cr."""
    return planes_file(oracle, np.ascontiguousarray(y), np.ascontiguousarray(cb), np.ascontiguousarray(cr), quality, sub, ri)


def restart_file(oracle, rgb: np.ndarray, quality: int = 0, sub: int = cm.SUB_420, ri: int = 1) -> Restart:
    """The file the library must write for these R, G, B pixels: the planes of interleaved_model.interleaved_file."""
    return planes_file(oracle, *sm.planes_of(rgb, sub), quality, sub, ri)


def with_dri(plain: bytes, ri: int) -> bytes:
    """Rule 5: the one-scan file `plain` with the DRI segment inserted in front of its SOS."""
    at = plain.index(im.SOS3)
    return plain[:at] + dri(ri) + plain[at:]
