"""CPU model of the progressive file of ANY valid scan script, colour or grayscale (include/jpeg_compression.h) --
TEST INFRASTRUCTURE ONLY.

Built from the pieces the other models share: scan_model's coefficients, DC symbols and packer, progressive_runs_model's first-scan walk
and head, progressive_successive_model's refinement walk, huffman_model's table construction, interleaved_model's geometry,
gray_scan_model's one-component prefix.  A script is a sequence of (components, Ss, Se, Ah, Al) with `components` a tuple of indices
(0 Y, 1 Cb, 2 Cr).  Every scan with symbols has tables of its own, numbered in the file's order: a first DC scan one per table class
among its components (Y; Cb and Cr together), an AC scan one, a DC refinement scan none.  New here: the MCU order of a DC scan of two
components, and a DC scan of one component over its own block grid.  Besides the file the model returns the counters the GPU tests
claim to exercise."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import color_model as cm
import gray_scan_model as gsm
import huffman_model as hm
import interleaved_model as im
import progressive_runs_model as prm
import progressive_successive_model as psm
import scan_model as sm

SEG_BLOCKS = im.SEG_BLOCKS
RAW = psm.RAW
GRAY = 0                                                          # `sub` of a grayscale file
GRAY_SOF_OFFSET = 2 + 18 + 69                                     # SOI, APP0, DQT with one table


def scan_tables(scan) -> int:
    """The tables a scan owns."""
    comps, ss, se, ah, al = scan
    if ss:
        return 1
    return 0 if ah else (0 in comps) + any(c in comps for c in (1, 2))


def table_ids(script) -> list:
    """The Tc/Th byte of every table in the file's order."""
    out = []
    for comps, ss, se, ah, al in script:
        n = scan_tables((comps, ss, se, ah, al))
        if ss:
            out.append(0x10 if comps == (0,) else 0x11)
        elif n == 2:
            out += [0x00, 0x01]
        elif n == 1:
            out.append(0x00 if 0 in comps else 0x01)
    return out


def sos(scan) -> bytes:
    comps, ss, se, ah, al = scan
    sel = b"".join(bytes([c + 1, 0x00 if c == 0 else 0x11]) for c in sorted(comps))
    return bytes([0xFF, 0xDA, 0x00, 6 + 2 * len(comps), len(comps)]) + sel + bytes([ss, se, (ah << 4) | al])


def gray_head(w: int, h: int, quality: int) -> bytes:
    """SOI, APP0, DQT, SOF2 of one component."""
    std = gsm.std_prefix(w, h, quality)
    n = len(std) - len(gsm.SOS1) - gsm.STD_DHT_BYTES
    assert std[GRAY_SOF_OFFSET:GRAY_SOF_OFFSET + 2] == b"\xff\xc0" and std[n:n + 2] == b"\xff\xc4"
    return std[:GRAY_SOF_OFFSET + 1] + b"\xc2" + std[GRAY_SOF_OFFSET + 2:n]


@dataclass(frozen=True)
class Scripted:
    file: bytes
    counts: np.ndarray              # int64 [tables][256] in the file's table order
    tables: tuple                   # (BITS, HUFFVAL, largest step-2 size) of every table
    ids: tuple                      # their Tc/Th bytes
    header_len: tuple               # bytes in front of every scan's entropy-coded segment (scan 1: the whole head of the file)
    scan_bits: tuple                # coded bits of every scan, before stuffing and flush
    seg_bits: tuple                 # the bits of every segment the device's coder cuts the scan into
    stuffed: tuple
    runs: tuple                     # every Run (progressive_successive_model.Run) of the AC scans
    zrl: tuple                      # ZRL symbols of every scan
    zrl_with_bits: int              # ZRLs of refinement scans coded with a non-empty B behind them
    pad_blocks: tuple               # pad blocks every scan codes (interleaved scans with Y alone)

    @property
    def bits(self):
        return sum(self.scan_bits)


def _dc_scan(dcs, comps, ny, al, ah):
    """The blocks of a DC scan in scan order -> per component of the scan (in ascending order) its values per block, and the place of
    every one of its blocks in the scan.  dcs[c]: the component's DC values -- Y in MCU order with pad blocks when the scan is
    interleaved, raster otherwise."""
    comps = sorted(comps)
    per = [ny if c == 0 else 1 for c in comps] if len(comps) > 1 else [1]
    bpm, off, keys = sum(per), 0, []
    for c, n in zip(comps, per):
        blk = np.arange(len(dcs[c]))
        keys.append((blk // n) * bpm + off + blk % n)            # T.81 A.2.3: the components of an MCU in ascending order, each its n blocks
        off += n
    return comps, bpm, keys


def planes_file(oracle, planes_px, quality: int, sub: int, script) -> Scripted:
    script = tuple((tuple(c), ss, se, ah, al) for c, ss, se, ah, al in script)
    gray = sub == GRAY
    h, w = planes_px[0].shape
    lq, cq = sm.scaled_table(sm.LUMA_Q, quality), sm.scaled_table(sm.CHROMA_Q, quality)
    planes = [sm.plane_zigzag(oracle, np.ascontiguousarray(p), cq if i else lq) for i, p in enumerate(planes_px)]
    if gray:
        assert len(planes) == 1 and all(c == (0,) for c, *_ in script)
        ny, pad, zy, head = 1, np.zeros(1, bool), planes[0], gray_head(w, h, quality)
    else:
        hs, vs, bw, bh, mx, my = im.geometry(w, h, sub)
        ny = hs * vs
        zy, pad = sm.mcu_order_luma(planes[0], bw, bh, hs, vs, mx, my)
        head = prm.head(w, h, quality, sub)
    ids = table_ids(script)
    first, at = [], 0
    for s in script:
        first.append(at)
        at += scan_tables(s)
    counts = np.zeros((len(ids), 256), np.int64)

    def dc_values(comps):
        """DC values per component index: Y in MCU order with its pad blocks where the scan is interleaved."""
        inter = len(comps) > 1
        return {c: (zy if c == 0 and inter else planes[c])[:, 0].astype(np.int64) for c in comps}

    def dc_table(k, comps, c):
        return first[k] + (1 if c and 0 in comps else 0)

    # ---- pass 1: what every scan codes, its symbols counted ----
    coded, runs, zrl, zrl_bits, pads = [], [], [], 0, []
    for k, (comps, ss, se, ah, al) in enumerate(script):
        if se == 0:
            dcs = dc_values(comps)
            pads.append(int(pad.sum()) if len(comps) > 1 and 0 in comps else 0)
            if ah == 0:
                part = {c: sm.dc_symbols(d >> al, len(d)) for c, d in dcs.items()}
                for c, (size, _) in part.items():
                    counts[dc_table(k, comps, c)] += np.bincount(size, minlength=256)
            else:
                part = {c: (d >> al) & 1 for c, d in dcs.items()}
            coded.append(part); zrl.append(0)
        else:
            walk = psm.refine_symbols if ah else psm.first_symbols
            items, per_block, rs, (z, zb, *_) = walk(planes[comps[0]], ss, se, al, k + 1)
            sym = items[:, 0]
            counts[first[k]] += np.bincount(sym[sym != RAW], minlength=256)
            coded.append((items, per_block)); runs += rs; zrl.append(z); zrl_bits += zb; pads.append(0)
    tables = tuple(hm.optimal_table(c) for c in counts)
    arrays = [sm.code_arrays(b, v) for b, v, _ in tables]
    assert all(length[c > 0].all() for (_, length), c in zip(arrays, counts))

    # ---- pass 2: coded with the scans' own tables ----
    scans, scan_bits, seg_bits, stuffed, header_len = [], [], [], [], []
    for k, (comps, ss, se, ah, al) in enumerate(script):
        nt = scan_tables(script[k])
        hdr = (head if k == 0 else b"") + b"".join(hm.dht(*tables[t][:2], ids[t]) for t in range(first[k], first[k] + nt)) + sos(script[k])
        if se == 0:
            dcs = dc_values(comps)
            order, bpm, keys = _dc_scan(dcs, comps, ny, al, ah)
            vals, lens = [], []
            for c in order:
                if ah == 0:
                    (size, amp), (code, ln) = coded[k][c], arrays[dc_table(k, comps, c)]
                    vals.append((code[size] << size) | amp); lens.append(ln[size] + size)
                else:
                    vals.append(coded[k][c]); lens.append(np.ones(len(coded[k][c]), np.int64))
            val, length, key = (np.concatenate(x) for x in (vals, lens, keys))
            o = np.argsort(key, kind="stable")
            assert np.array_equal(key[o], np.arange(len(key)))   # every place of the scan has its block
            val, length = val[o], length[o]
            per_seg = SEG_BLOCKS // bpm * bpm                    # a segment: floor(256 / blocks per MCU) MCUs
            segs = tuple(int(length[i:i + per_seg].sum()) for i in range(0, len(length), per_seg))
        else:
            (items, per_block), (code, ln) = coded[k], arrays[first[k]]
            sym, extra, elen = items.T
            tabbed = sym != RAW
            s = np.where(tabbed, sym, 0)
            length = np.where(tabbed, ln[s], 0) + elen
            val = (np.where(tabbed, code[s], 0) << elen) | extra
            ends = np.r_[0, np.cumsum(per_block)]
            csum = np.r_[0, np.cumsum(length)]
            bb = csum[ends[1:]] - csum[ends[:-1]]
            segs = tuple(int(bb[i:i + SEG_BLOCKS].sum()) for i in range(0, len(bb), SEG_BLOCKS))
        data, total, ff = sm.pack(val, length)
        scans.append(hdr + data); scan_bits.append(total); stuffed.append(ff); header_len.append(len(hdr)); seg_bits.append(segs)
    return Scripted(b"".join(scans) + b"\xff\xd9", counts, tables, tuple(ids), tuple(header_len), tuple(scan_bits), tuple(seg_bits),
                    tuple(stuffed), tuple(runs), tuple(zrl), zrl_bits, tuple(pads))


def _key(script):
    return tuple((tuple(c), ss, se, ah, al) for c, ss, se, ah, al in script)


def ycbcr_file(oracle, y, cb, cr, quality: int, sub: int, script) -> Scripted:
    """The file of samples that already are Y, Cb and Cr: coded as given."""
    return planes_file(oracle, (np.ascontiguousarray(y), np.ascontiguousarray(cb), np.ascontiguousarray(cr)), quality, sub, _key(script))


def rgb_file(oracle, rgb: np.ndarray, quality: int, sub: int, script) -> Scripted:
    """The file the library must write for these R, G, B pixels: the planes the other colour paths derive."""
    return planes_file(oracle, sm.planes_of(rgb, sub), quality, sub, _key(script))


def gray_file(oracle, plane: np.ndarray, quality: int, script) -> Scripted:
    """The grayscale file of a luma plane."""
    return planes_file(oracle, (np.ascontiguousarray(plane),), quality, GRAY, _key(script))
