"""What every CPU model of a file shares (color_model.py, color_model_422.py, interleaved_model.py, restart_model.py, huffman_model.py,
gray_scan_model.py, progressive_model.py) -- TEST INFRASTRUCTURE ONLY.  One copy of each step between pixels and the bytes of a scan:
the planes an RGB picture gives, the oracle's stage functions over a plane, its run/size symbols, the Annex K tables, the coder, the MCU
merge, the bit packer with 0xFF stuffing, the framing of restart intervals, and a structural walk of a finished scan.  The file models
keep geometry, prefixes and the counters they report; this module imports none of them."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

# T.81 Annex K: K.1 / K.2 (quantisation, raster order), K.3-K.6 as BITS / HUFFVAL
LUMA_Q = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
          18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
          103, 99]
CHROMA_Q = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99,
            99, 99] + [99] * 32
DC_LUMA_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHROMA_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUMA_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D]
AC_LUMA_VALS = bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748"
    "494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3"
    "c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
AC_CHROMA_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHROMA_VALS = bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a4344454647"
    "48494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2"
    "c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")
SUB_444, SUB_420, SUB_422 = 1, 2, 4                             # JPEGAMD_SUBSAMPLE_*


# ---- pixels to planes ---------------------------------------------------------------------------------------------------------------
def luma_plane(rgb: np.ndarray) -> np.ndarray:
    r, g, b = (rgb[:, :, i].astype(np.int64) for i in range(3))
    return ((77 * r + 150 * g + 29 * b) >> 8).astype(np.uint8)


def chroma_planes(rgb: np.ndarray, sub: int):
    """The spec's integer Cb / Cr planes, uint8 [ch, cw] each.  4:2:0: the rounded mean of a 2 x 2 group, the last row and column
    replicated; 4:2:2: (a + b + 1) >> 1 over the two pixels 2x, 2x + 1 of one row, the last column replicated, no vertical filter."""
    r, g, b = (rgb[:, :, i].astype(np.int64) for i in range(3))
    cb = (32768 - 43 * r - 85 * g + 128 * b) >> 8
    cr = (32768 + 128 * r - 107 * g - 21 * b) >> 8
    h, w = cb.shape
    xs = np.arange(0, w, 2)
    x1 = np.minimum(xs + 1, w - 1)
    if sub == SUB_420:
        ys = np.arange(0, h, 2)
        y1 = np.minimum(ys + 1, h - 1)
        cb, cr = ((p[ys][:, xs] + p[ys][:, x1] + p[y1][:, xs] + p[y1][:, x1] + 2) >> 2 for p in (cb, cr))
    elif sub == SUB_422:
        cb, cr = ((p[:, xs] + p[:, x1] + 1) >> 1 for p in (cb, cr))
    return cb.astype(np.uint8), cr.astype(np.uint8)


def planes_of(rgb: np.ndarray, sub: int):
    """(Y, Cb, Cr) as every RGB entry derives them at `sub`."""
    return (luma_plane(rgb),) + chroma_planes(rgb, sub)


# ---- planes to coefficients -----------------------------------------------------------------------------------------------------------
def scaled_table(base, quality: int) -> np.ndarray:
    """quant_table_for_quality's rule (0 -> 50; libjpeg scaling; clamp 1..255) applied to `base`."""
    q = 50 if quality <= 0 else min(quality, 100)
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.array([min(max((b * s + 50) // 100, 1), 255) for b in base], np.uint8)


def plane_zigzag(oracle, plane: np.ndarray, qt: np.ndarray) -> np.ndarray:
    """The oracle's stage functions over an 8-bit plane (edge-replicated to multiples of 8): int16 [NB, 64] zigzag, raster block order."""
    h, w = plane.shape
    ph, pw = (h + 7) & ~7, (w + 7) & ~7
    padded = np.pad(plane, ((0, ph - h), (0, pw - w)), mode="edge")
    y = np.ascontiguousarray((padded.astype(np.int16) - 128).astype(np.int8))
    lib = oracle._lib
    d = np.zeros((ph, pw), np.float32)
    lib.oracle_dct_image(y.ctypes.data, pw, ph, d.ctypes.data)
    q = np.zeros((ph, pw), np.int16)
    qt = np.ascontiguousarray(qt, np.uint8)
    lib.oracle_quant_image(d.ctypes.data, pw, ph, qt.ctypes.data, q.ctypes.data)
    zz = np.zeros(((pw // 8) * (ph // 8), 64), np.int16)
    lib.oracle_zigzag_image(q.ctypes.data, pw, ph, zz.ctypes.data)
    return zz


def mcu_order_luma(zz: np.ndarray, bw: int, bh: int, hs: int, vs: int, mx: int, my: int):
    """The Y blocks in scan order, libjpeg's pad blocks made (DC of the nearest real block, no AC): int16 [mx my hs vs, 64], and the
    pad flags."""
    j, i, v, u = np.meshgrid(np.arange(my), np.arange(mx), np.arange(vs), np.arange(hs), indexing="ij")
    bx, by = (i * hs + u).ravel(), (j * vs + v).ravel()
    pad = (bx >= bw) | (by >= bh)
    out = zz[np.minimum(by, bh - 1) * bw + np.minimum(bx, bw - 1)].copy()
    out[pad, 1:] = 0
    return out, pad


# ---- coefficients to symbols ----------------------------------------------------------------------------------------------------------
def symbols(oracle, zz: np.ndarray):
    """oracle_rle over the blocks, DC predictor 0 in front of the first -> (symbol, amplitude bits, amplitude length, DC flag) per symbol
    and the symbols of every block."""
    zz = np.ascontiguousarray(zz, np.int16)
    nb = zz.shape[0]
    cap = nb * 70 + 16
    buf = np.zeros(cap * 4, np.uint8)
    n = oracle._lib.oracle_rle(zz.ctypes.data, nb, C.c_void_p(buf.ctypes.data), cap)
    assert n >= 0, n
    rec = buf[:4 * n].reshape(n, 4)
    sym, alen, amp = rec[:, 0].astype(np.int64), rec[:, 1].astype(np.int64), rec[:, 2].astype(np.int64) | (rec[:, 3].astype(np.int64) << 8)
    # symbols per block: DC, (ZRLs + symbol) per non-zero AC, EOB unless zigzag 63 is non-zero (rle.c)
    rows, cols = np.nonzero(zz[:, 1:])
    pos = cols + 1
    same = np.r_[False, rows[1:] == rows[:-1]]
    prev = np.where(same, np.r_[0, pos[:-1]], 0)
    per_ac = 1 + (pos - prev - 1) // 16
    counts = 1 + np.bincount(rows, weights=per_ac, minlength=nb).astype(np.int64) + (zz[:, 63] == 0)
    assert counts.sum() == n, (counts.sum(), n)
    is_dc = np.zeros(n, bool)
    is_dc[np.r_[0, np.cumsum(counts)[:-1]]] = True
    return sym, amp, alen, is_dc, counts


def dc_symbols(dc: np.ndarray, step: int):
    """DC values in scan order, predictor 0 at every `step`-th block -> (size, amplitude bits) per block (T.81 F.1.2.1)."""
    dc = dc.astype(np.int64)
    prev = np.r_[0, dc[:-1]]
    prev[::step] = 0
    diff = dc - prev
    size = np.zeros(len(dc), np.int64)
    mag = np.abs(diff)
    while mag.any():
        size += mag > 0
        mag >>= 1
    return size, np.where(diff < 0, diff - 1, diff) & ((1 << size) - 1)


# ---- symbols to bits ----------------------------------------------------------------------------------------------------------------
def canonical(bits, vals):
    """symbol -> (code, length); symbols the table does not list are absent (length 0: no code bits, as the reference)."""
    out, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            out[vals[k]] = (code, ln)
            code += 1
            k += 1
        code <<= 1
    return out


def code_arrays(bits, vals):
    """-> (code[256], length[256]) of the canonical code, 0 / 0 for symbols without one."""
    code, length = np.zeros(256, np.int64), np.zeros(256, np.int64)
    for s, (c, ln) in canonical(bits, vals).items():
        code[s], length[s] = c, ln
    return code, length


def std_tables(chroma: bool):
    """The Annex K tables of a component: (DC code_arrays, AC code_arrays)."""
    if chroma:
        return code_arrays(DC_CHROMA_BITS, DC_VALS), code_arrays(AC_CHROMA_BITS, AC_CHROMA_VALS)
    return code_arrays(DC_LUMA_BITS, DC_VALS), code_arrays(AC_LUMA_BITS, AC_LUMA_VALS)


def coded(syms, dc_table, ac_table):
    """symbols() with a table pair -> (value, length) per symbol: the code word and the amplitude bits behind it."""
    sym, amp, alen, is_dc = syms[:4]
    code = np.where(is_dc, dc_table[0][sym], ac_table[0][sym])
    return (code << alen) | (amp & ((1 << alen) - 1)), np.where(is_dc, dc_table[1][sym], ac_table[1][sym]) + alen


def bit_array(val: np.ndarray, length: np.ndarray) -> np.ndarray:
    """The `length` low bits of every value, first value and high bit first: uint8 0 / 1."""
    total = int(length.sum())
    starts = np.cumsum(length) - length
    idx = np.repeat(np.arange(len(val)), length)
    off = np.arange(total) - starts[idx]
    return ((val[idx] >> (length[idx] - 1 - off)) & 1).astype(np.uint8)


def stuff(by: np.ndarray):
    """0x00 behind every 0xFF -> (the bytes, the 0xFF count)."""
    ff = np.nonzero(by == 0xFF)[0]
    return np.insert(by, ff + 1, 0).tobytes(), len(ff)


def pack(val: np.ndarray, length: np.ndarray):
    """One entropy-coded segment, flushed with 0-bits and stuffed -> (its bytes, coded bits, stuffed bytes)."""
    data, ff = stuff(np.packbits(bit_array(val, length)))
    return data, int(length.sum()), ff


def pack_scan(oracle, zz: np.ndarray, chroma: bool) -> bytes:
    """Entropy-coded segment of zigzag blocks with the luma or chroma tables: DC predictor 0 at the start, 0xFF stuffing, zero-bit flush."""
    return pack(*coded(symbols(oracle, zz), *std_tables(chroma)))[0]


# ---- three components in one scan -------------------------------------------------------------------------------------------------------
def mcu_merge(components, ny: int):
    """components: (value, length, symbols per block) of Y -- blocks in MCU order, `ny` to an MCU --, Cb and Cr -> the symbols in scan
    order (value, length) and the bits of every MCU."""
    bpm = ny + 2
    keys = []
    for comp, (_, _, counts) in enumerate(components):
        blk = np.arange(len(counts))
        keys.append(np.repeat((blk // ny) * bpm + blk % ny if comp == 0 else blk * bpm + ny + comp - 1, counts))     # the block's place in the scan
    val, length, key = (np.concatenate(x) for x in ([c[0] for c in components], [c[1] for c in components], keys))
    order = np.argsort(key, kind="stable")                       # the symbols of a block stay in order
    val, length, key = val[order], length[order], key[order]
    return val, length, np.bincount(key // bpm, weights=length, minlength=len(components[1][2])).astype(np.int64)


def scan_symbols(oracle, zy, zcb, zcr, ny: int, step: int):
    """Per interval of `step` MCUs the symbols() of its Y, Cb and Cr blocks: the oracle's RLE runs per interval and per component, so
    every interval starts with all three DC predictors at 0."""
    return [[symbols(oracle, zz) for zz in (zy[a * ny:(a + step) * ny], zcb[a:a + step], zcr[a:a + step])] for a in range(0, zcb.shape[0], step)]


def scan_bits(intervals, luma, chroma, ny: int):
    """scan_symbols coded with the (DC, AC) table pairs of Y and of the chroma components, merged -> (every bit, the bits of every MCU)."""
    bits, mcu_bits = [], []
    for per in intervals:
        val, length, per_mcu = mcu_merge([coded(s, *(chroma if comp else luma)) + (s[4],) for comp, s in enumerate(per)], ny)
        bits.append(bit_array(val, length))
        mcu_bits.append(per_mcu)
    return np.concatenate(bits), np.concatenate(mcu_bits)


# ---- bits to the bytes of a scan --------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Interval:
    """One restart interval as frame_intervals wrote it, and what the device's writer has to get right about it."""
    padded: np.ndarray              # its bytes before stuffing, pad or flush bits included
    r: int                          # coded bits in its last byte (0: it ended on a byte)
    last: bool                      # flushed with 0-bits and followed by EOI, not padded with 1-bits and followed by RSTn
    seg_bits: tuple                 # the coded bits of each coder segment
    ff: int                         # 0xFF bytes: as many 0x00 were stuffed

    @property
    def bits(self) -> int:
        return sum(self.seg_bits)

    @property
    def aligned(self) -> bool:
        """It ended on a byte and got no padding (the last interval does not count)."""
        return not self.r and not self.last

    @property
    def pad_ff(self) -> bool:
        """Its padded byte came out 0xFF (and was stuffed)."""
        return bool(self.r and not self.last and self.padded[-1] == 0xFF)

    @property
    def straddle_phases(self) -> list:
        """The phases (bit offset mod 8) of the boundaries of two coder segments that lie inside an 0xFF byte."""
        return [int(p % 8) for p in np.cumsum(self.seg_bits)[:-1] if p % 8 and self.padded[p // 8] == 0xFF]


def frame_intervals(bits: np.ndarray, unit_bits: np.ndarray, step: int, seg_units: int):
    """The body of a scan -- `bits` (uint8 0 / 1) are its units (MCUs) one after the other, unit i `unit_bits[i]` long -- in restart
    intervals of `step` units: each padded with 1-bits to a byte, stuffed and followed by RSTn, the last one flushed with 0-bits.  The
    device's coder cuts an interval into segments of `seg_units` units from its first.  -> (the bytes up to EOI, one Interval each)."""
    end = np.r_[0, np.cumsum(unit_bits)]
    m = len(unit_bits)
    body, out = bytearray(), []
    for i, a in enumerate(range(0, m, step)):
        b = min(a + step, m)
        last = b == m
        chunk = bits[end[a]:end[b]]
        r = len(chunk) % 8
        if r:
            chunk = np.r_[chunk, np.full(8 - r, 0 if last else 1, np.uint8)]
        padded = np.packbits(chunk)
        data, ff = stuff(padded)
        body += data if last else data + bytes([0xFF, 0xD0 + i % 8])
        seg_bits = np.diff(end[np.r_[np.arange(a, b, seg_units), b]])
        out.append(Interval(padded, r, last, tuple(int(x) for x in seg_bits), ff))
    return bytes(body), out


def walk_scan(data: bytes, sos: bytes):
    """A structural walk of the scan behind `sos` that knows nothing of how it was written: -> (markers in order, stuffed 0x00 bytes).
    Every 0xFF of the scan must be followed by 0x00, by an RSTn marker or -- as the file's last two bytes -- by EOI."""
    at = data.index(sos) + len(sos)
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


# ---- three scans, one component each ------------------------------------------------------------------------------------------------
def sos(component: int) -> bytes:
    return bytes([0xFF, 0xDA, 0x00, 0x08, 0x01, component, 0x00 if component == 1 else 0x11, 0, 63, 0])


def three_scans(oracle, prefix: bytes, y_scan: bytes, cb: np.ndarray, cr: np.ndarray, quality: int) -> bytes:
    """A three-scan file: the prefix (it ends with the Y scan's SOS), the Y scan as given, the chroma pipeline over the Cb and Cr planes
    as given, EOI."""
    cq = scaled_table(CHROMA_Q, quality)
    parts = [prefix, y_scan]
    for comp, plane in ((2, cb), (3, cr)):
        parts += [sos(comp), pack_scan(oracle, plane_zigzag(oracle, plane, cq), True)]
    return b"".join(parts) + b"\xff\xd9"
