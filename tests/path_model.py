"""Which path does each tile, segment and workgroup take -- TEST INFRASTRUCTURE ONLY (CPU, numpy).

k_tile_encode, k_segment_merge and k_stitch each hold a rarely taken second path, chosen by integer comparisons against buffer
sizes.  This module restates those comparisons over the zigzag coefficients of a picture (oracle.stages(...)["zigzag"], or a chroma
plane's color_model.plane_zigzag) and reports, per tile / segment / stitch workgroup, where the picture sits relative to them.
Every constant is read from the kernel sources when the module is imported; one that cannot be found is an error, so a changed
buffer size shows up as fixtures that left their edge (tests/test_thresholds_host.py), never as an edge that is quietly no longer
covered.  The model is checked against the oracle (bits, symbols, 0xFF bytes), never against the product."""
from __future__ import annotations

import re
from pathlib import Path

import numpy as np

import color_model as cm

CSRC = Path(__file__).resolve().parents[1] / "jpeg-image-compression_amd" / "csrc"


# ---- constants, from the kernel sources -----------------------------------------------------------------------------------
def _const_exprs(text: str) -> dict:
    out = {}
    for m in re.finditer(r"constexpr\s+(?:unsigned\s+|uint32_t\s+|int\s+)(\w+)\s*=\s*([^;]+);", text):
        out.setdefault(m.group(1), m.group(2))
    for m in re.finditer(r"#define\s+(JPEGAMD_\w+)\s+(\d+)\s*$", text, re.M):
        out.setdefault(m.group(1), m.group(2))
    return out


def _evaluate(expr: str, env: dict) -> int:
    expr = re.sub(r"\((?:uint32_t|int|unsigned)\)", "", expr)
    expr = re.sub(r"(\d+)[uU]\b", r"\1", expr).replace("/", "//")
    names = set(re.findall(r"[A-Za-z_]\w*", expr))
    missing = names - set(env)
    if missing:
        raise KeyError(f"{sorted(missing)} in '{expr}'")
    return int(eval(expr, {"__builtins__": {}}, dict(env)))          # arithmetic over names already resolved from the sources


def read_constants(csrc: Path = CSRC) -> dict:
    """The thresholds of the three kernels, by the names the sources give them.  The merge window and the stitch part are
    templates over the tiles of a segment: 'merge_fast_bits' / 'stitch_part_bits' map tiles per segment -> bits."""
    files = {n: (Path(csrc) / n).read_text() for n in ("jpegamd_internal.h", "jpegamd_tile_pipeline.hip", "jpegamd_entropy.hip",
                                                      "jpegamd_stitch.hip", "jpegamd_finalize.hip")}
    want = {"jpegamd_internal.h": ["kTileBlocks", "JPEGAMD_SEG_TILES", "kSegTiles", "kSegTilesBatch", "kSegGroup", "kTileRecWords", "kStageWords",
                                   "kStageItemCap", "kTileHeadWords", "kTileHeadStr", "kMaxBlockBits"],
            "jpegamd_tile_pipeline.hip": ["kWinWords", "kWinStr", "kPassItems", "kQuadMinItems"],
            "jpegamd_entropy.hip": ["kSegBufWords", "kPieceWords"],
            "jpegamd_finalize.hip": ["kFinWaves"],
            "jpegamd_stitch.hip": ["JPEGAMD_ST_WAVES"]}
    env = {}
    for fname, names in want.items():
        exprs = _const_exprs(files[fname])
        for n in names:
            if n not in exprs:
                raise RuntimeError(f"path_model: constant {n} not found in {fname}: the threshold fixtures need regenerating against the new sources")
            try:
                env[n] = _evaluate(exprs[n], env)
            except KeyError as e:
                raise RuntimeError(f"path_model: cannot evaluate {n} of {fname}: {e}")
    # the templated expressions
    m = re.search(r"constexpr int kBuf\s*=\s*([^;]+);", files["jpegamd_entropy.hip"])
    f = re.search(r"seg_bits\s*<=\s*\(uint32_t\)\(\((kBuf\s*-\s*\d+)\)\s*\*\s*32\)\s*&&\s*max_words\s*<=\s*\(uint32_t\)kTileHeadStr", files["jpegamd_entropy.hip"])
    r = re.search(r"\(need_end >> 5\) - wbase \+ (\d+)u > \(uint32_t\)kBuf", files["jpegamd_entropy.hip"])
    if not (m and f and r):
        raise RuntimeError("path_model: k_segment_merge's window expressions (kBuf, the fast-path bound, make_room) not found in jpegamd_entropy.hip")
    sb = re.search(r"constexpr int kBuf\s*=\s*([^;]+);", files["jpegamd_stitch.hip"])
    sp = re.search(r"constexpr uint32_t kPartBits\s*=\s*([^;]+);", files["jpegamd_stitch.hip"])
    sw = re.search(r"constexpr uint32_t kPieceWords\s*=\s*(\d+);", files["jpegamd_stitch.hip"])
    sr = re.search(r"const uint32_t room\s*=\s*([^;]+);", files["jpegamd_stitch.hip"])
    if not (sb and sp and sw and sr):
        raise RuntimeError("path_model: k_stitch's window expressions (kBuf, kPartBits, kPieceWords, room) not found in jpegamd_stitch.hip")
    t = re.search(r"\(\(cur_bits \+ add_bits\) >> 5\) - wbase \+ (\d+)u > \(uint32_t\)kWinStr", files["jpegamd_tile_pipeline.hip"])
    z = re.search(r"wbase == 0u && nw \+ \(uint32_t\)kTileRecWords <= (\d+)u", files["jpegamd_tile_pipeline.hip"])
    tl = re.search(r"if \(nitems - base <= (\d+)u\)", files["jpegamd_tile_pipeline.hip"])
    if not (t and z and tl):
        raise RuntimeError("path_model: k_tile_encode's window expressions (make_room, the re-zeroing test, the tail pass) not found in jpegamd_tile_pipeline.hip")
    env["tile_room_margin"], env["tile_rezero_words"], env["tail_items"] = int(t.group(1)), int(z.group(1)), int(tl.group(1))
    env["merge_room_margin"] = int(r.group(1))
    env["merge_buf"], env["merge_fast_bits"], env["stitch_buf"], env["stitch_part_bits"], env["stitch_room_words"] = {}, {}, {}, {}, {}
    for tiles in (env["kSegTiles"], env["kSegTilesBatch"]):
        e = dict(env, kTiles=tiles)
        e = {k: v for k, v in e.items() if isinstance(v, int)}
        e["kBuf"] = _evaluate(m.group(1), e)
        env["merge_buf"][tiles] = e["kBuf"]
        env["merge_fast_bits"][tiles] = _evaluate(f.group(1), e) * 32
        e["kBuf"] = _evaluate(sb.group(1), e)
        e["kPartBits"] = _evaluate(sp.group(1), e)
        e["kPieceWords"] = int(sw.group(1))
        env["stitch_buf"][tiles] = e["kBuf"]
        env["stitch_part_bits"][tiles] = e["kPartBits"]
        env["stitch_room_words"][tiles] = _evaluate(sr.group(1), e)
    env["stitch_piece_words"] = int(sw.group(1))
    env["kStWaves"] = env["JPEGAMD_ST_WAVES"]
    return env


K = read_constants()


# ---- tables ---------------------------------------------------------------------------------------------------------------
class Table:
    """Code lengths of a scan's Huffman tables: dc_len[size], ac_len[(run << 4) | size] (0: no code, as the reference)."""

    def __init__(self, chroma: bool):
        self.chroma = chroma
        dc = cm.canonical(cm.DC_CHROMA_BITS if chroma else cm.DC_LUMA_BITS, cm.DC_VALS)
        ac = cm.canonical(cm.AC_CHROMA_BITS if chroma else cm.AC_LUMA_BITS, cm.AC_CHROMA_VALS if chroma else cm.AC_LUMA_VALS)
        self.dc_len, self.ac_len = np.zeros(16, np.int64), np.zeros(256, np.int64)
        for s, (_, ln) in dc.items():
            self.dc_len[s] = ln
        for s, (_, ln) in ac.items():
            self.ac_len[s] = ln
        self.zrl_bits = int(self.ac_len[0xF0])


LUMA, CHROMA = Table(False), Table(True)


def _size(v: np.ndarray) -> np.ndarray:
    """bits of |v| (rle.c's size category)"""
    a = np.abs(v.astype(np.int64))
    return np.where(a > 0, np.floor(np.log2(np.maximum(a, 1))).astype(np.int64) + 1, 0)


def dc_symbol_bits(diff: np.ndarray, tab: Table) -> np.ndarray:
    s = _size(np.asarray(diff))
    return tab.dc_len[s] + s


# ---- items ----------------------------------------------------------------------------------------------------------------
def item_lists(zz: np.ndarray, tab: Table):
    """The item list k_tile_encode builds, for all blocks at once.  -> dict of arrays over items, in list order:
    block, pos (0: DC and EOB), run (AC items: zeros in front), zrl (0..3), bits (code + amplitude + ZRLs; the DC items' bits are
    those of the difference to the block before, the picture's first block against 0), and per block: items, first (index of its
    DC item)."""
    zz = np.asarray(zz, np.int64)
    nb = zz.shape[0]
    rows, cols = np.nonzero(zz[:, 1:])
    pos = cols + 1
    same = np.r_[False, rows[1:] == rows[:-1]]
    prev = np.where(same, np.r_[0, pos[:-1]], 0)
    run = pos - prev - 1
    size = _size(zz[rows, pos])
    zrl = run >> 4
    ac_bits = tab.ac_len[((run & 15) << 4) | size] + size + zrl * tab.zrl_bits
    eob = zz[:, 63] == 0
    dcdiff = zz[:, 0] - np.r_[0, zz[:-1, 0]]
    dc_bits = dc_symbol_bits(dcdiff, tab)
    eb = np.nonzero(eob)[0]
    blk = np.r_[np.arange(nb), rows, eb]
    key = np.r_[np.zeros(nb, np.int64), pos, np.full(len(eb), 64)]
    order = np.lexsort((key, blk))
    n_ac, n_e = len(rows), len(eb)
    it = dict(block=blk[order],
              pos=np.r_[np.zeros(nb, np.int64), pos, np.zeros(n_e, np.int64)][order],
              run=np.r_[np.zeros(nb, np.int64), run, np.zeros(n_e, np.int64)][order],
              zrl=np.r_[np.zeros(nb, np.int64), zrl, np.zeros(n_e, np.int64)][order],
              bits=np.r_[dc_bits, ac_bits, np.full(n_e, tab.ac_len[0])][order])
    items = 1 + np.bincount(rows, minlength=nb) + eob
    it["items"] = items
    it["first"] = np.cumsum(items) - items
    it["dc_bits"] = dc_bits
    return it


# ---- k_tile_encode --------------------------------------------------------------------------------------------------------
def tile_report(it: dict, b0: int, b1: int) -> dict:
    """Blocks [b0, b1) form one tile."""
    cap, pass_items, quad_min, tail_items = K["kStageItemCap"], K["kPassItems"], K["kQuadMinItems"], K["tail_items"]
    items = it["items"][b0:b1]
    incl = np.cumsum(items)
    t_all = int(incl[-1])
    half = K["kTileBlocks"] // 2
    h0 = int(incl[min(half, len(items)) - 1])
    nparts = 1 if t_all <= cap else (2 if max(h0, t_all - h0) <= cap else 4)
    per_part = K["kTileBlocks"] // nparts
    i0 = int(it["first"][b0])
    bits = it["bits"][i0:i0 + t_all].copy()
    bits[0] = 0                                                          # the padding item: the first DC symbol is the merge's
    zrl, run = it["zrl"][i0:i0 + t_all], it["run"][i0:i0 + t_all]
    cur_bits = wbase = nzrl = writeouts = 0
    parts = []

    def make_room(add):
        nonlocal wbase, writeouts
        if ((cur_bits + add) >> 5) - wbase + K["tile_room_margin"] > K["kWinStr"]:
            done = (cur_bits >> 5) - wbase
            if done:
                wbase += done
                writeouts += 1

    for part in range(nparts):
        lb = int(incl[min(part * per_part, len(items)) - 1]) if part else 0
        le = t_all if part == nparts - 1 else int(incl[min((part + 1) * per_part, len(items)) - 1])
        n = le - lb
        passes, base = [], 0
        while base < n:
            left = n - base
            kind, span = None, pass_items
            if left <= tail_items:
                kind, span = "tail", left
            elif n >= quad_min and left > pass_items:
                if np.any(run[lb + base:lb + min(base + 2 * pass_items, n)] >= 16):
                    kind = "fell"                                            # the attempt, then the pair pass over the first 128
                else:
                    kind, span = "quad", 2 * pass_items
            else:
                kind = "pair"
            lo, hi = lb + base, lb + min(base + span, n)
            z = zrl[lo:hi]
            add = int(bits[lo:hi].sum())
            make_room(add)
            cur_bits += add
            nzrl += int(z.sum())
            passes.append(dict(kind=kind, items=hi - lo, zrl=[int((z == k).sum()) for k in (1, 2, 3)],
                               carry_run=bool(base > 0 and run[lo] >= 16)))
            if kind == "tail":
                break
            base += span
        parts.append(dict(items=n, passes=passes))
    nw = ((cur_bits + 31) >> 5) - wbase
    whole = wbase == 0 and nw <= K["kTileHeadStr"]
    return dict(items=t_all, items_h0=h0, nparts=nparts, parts=parts, str_bits=cur_bits, str_words=(cur_bits + 31) >> 5,
                writeouts=writeouts, whole=whole, rezero=not (wbase == 0 and nw + K["kTileRecWords"] <= K["tile_rezero_words"]),
                symbols=t_all + nzrl, dc_bits=int(it["dc_bits"][b0]))


# ---- the stream -----------------------------------------------------------------------------------------------------------
def unstuff(scan: bytes) -> np.ndarray:
    """entropy-coded bytes -> the bytes in front of stuffing (every 00 behind an FF removed)"""
    by = np.frombuffer(scan, np.uint8)
    ff = np.nonzero(by[:-1] == 0xFF)[0]
    assert np.all(by[ff + 1] == 0), "a marker inside the scan"
    return np.delete(by, ff + 1)


def ones8(stream_bytes: np.ndarray) -> np.ndarray:
    """bool per bit offset i: the 8 stream bits from i on are all ones"""
    bits = np.unpackbits(stream_bytes).astype(np.int64)
    c = np.r_[0, np.cumsum(bits)]
    o = np.zeros(len(bits), bool)
    if len(bits) >= 8:
        o[:len(bits) - 7] = (c[8:] - c[:-8]) == 8
    return o


# ---- the picture ----------------------------------------------------------------------------------------------------------
def picture_report(zz: np.ndarray, blocks_w: int, blocks_h: int, tab: Table = LUMA, scan: bytes | None = None) -> dict:
    """zz: int16 [blocks_h * blocks_w, 64] in raster block order; scan: the oracle's entropy-coded bytes of it (for the 0xFF
    placement; optional).  -> tiles (raster order), and for segments of 8 and 16 tiles: merge and stitch reports."""
    it = item_lists(zz, tab)
    tb = K["kTileBlocks"]
    tpr = (blocks_w + tb - 1) // tb
    tiles = []
    for by in range(blocks_h):
        for tx in range(tpr):
            tiles.append(tile_report(it, by * blocks_w + tx * tb, by * blocks_w + min((tx + 1) * tb, blocks_w)))
    tbits = np.array([t["dc_bits"] + t["str_bits"] for t in tiles], np.int64)
    toff = np.cumsum(tbits) - tbits
    rep = dict(tiles=tiles, tile_off=toff, total_bits=int(tbits.sum()), symbols=sum(t["symbols"] for t in tiles),
               blocks_w=blocks_w, blocks_h=blocks_h, tiles_per_row=tpr, seg={})
    o8 = ffpos = None
    if scan is not None:
        o8 = ones8(unstuff(scan))
        ffpos = np.nonzero(o8[::8])[0] * 8                              # bit offsets of the stream's 0xFF bytes
        rep["ff_total"] = len(ffpos)

    def straddled(bounds):
        """how many of the bit offsets `bounds` lie strictly inside an 0xFF byte"""
        if ffpos is None or len(ffpos) == 0:
            return 0
        b = np.asarray(sorted(bounds), np.int64)
        b = b[b % 8 != 0]
        return int(np.isin(b // 8 * 8, ffpos).sum()) if len(b) else 0

    if scan is not None:
        rep["ff_at"] = dict(tile_string=straddled(toff[1:]),
                            first_dc=straddled([toff[i] + tiles[i]["dc_bits"] for i in range(len(tiles)) if tiles[i]["dc_bits"]]))
    for T in (K["kSegTiles"], K["kSegTilesBatch"]):
        spr = (tpr + T - 1) // T
        segs = []
        for by in range(blocks_h):
            for sx in range(spr):
                t0 = by * tpr + sx * T
                t1 = by * tpr + min((sx + 1) * T, tpr)
                segs.append(segment_report(tiles[t0:t1], int(toff[t0]), T))
        seg_off = np.array([s["offset"] for s in segs], np.int64)
        r = dict(segs=segs, segs_per_row=spr, num_segs=len(segs))
        if scan is not None:
            idx = np.arange(1, len(segs))
            r["ff_at"] = dict(
                writeout=straddled([s["offset"] + w for s in segs for w in s["merge_writeout_bits"]]),
                segment_in_group=straddled(seg_off[idx[idx % K["kSegGroup"] != 0]]),
                group=straddled(seg_off[idx[(idx % K["kSegGroup"] == 0) & (idx % K["kFinWaves"] != 0)]]),
                chunk=straddled(seg_off[idx[idx % K["kFinWaves"] == 0]]),
                stitch_part=straddled([s["offset"] + b for s in segs for b in s["stitch_part_ends"][:-1]]),
                stitch_workgroup=straddled(seg_off[idx[idx % K["kStWaves"] == 0]]))
            wgs = []
            for g in range(0, len(segs), K["kStWaves"]):
                a = int(seg_off[g])
                b = int(seg_off[g + K["kStWaves"]]) if g + K["kStWaves"] < len(segs) else rep["total_bits"]
                wgs.append([int(o8[a + (-p) % 8:max(b - 7, 0):8].sum()) if b - a >= 8 else 0 for p in range(8)])
            r["wg_ff"] = wgs
        rep["seg"][T] = r
    return rep


# ---- k_segment_merge and k_stitch -----------------------------------------------------------------------------------------
def segment_report(tiles: list, offset: int, T: int) -> dict:
    head, piece = K["kTileHeadStr"], K["kPieceWords"]
    tbits = [t["dc_bits"] + t["str_bits"] for t in tiles]
    seg_bits = sum(tbits)
    max_words = max(t["str_words"] for t in tiles)
    fast = seg_bits <= K["merge_fast_bits"][T] and max_words <= head
    wbase, outs = 0, []
    if not fast:
        kbuf = K["merge_buf"][T]

        def make_room(upto, need_end):
            nonlocal wbase
            if (need_end >> 5) - wbase + K["merge_room_margin"] > kbuf:
                done = (upto >> 5) - wbase
                if done:
                    wbase += done
                    outs.append(wbase * 32)

        off = 0
        for t in tiles:
            dl, sb = t["dc_bits"], t["str_bits"]
            make_room(off, off + dl + min(sb, piece * 32))
            w0 = 0
            while w0 < t["str_words"]:
                start = off + dl + w0 * 32
                if w0:
                    make_room(start, start + min(sb - w0 * 32, piece * 32))
                w0 += piece if w0 else head
            off += dl + sb
    # k_stitch: the segment as parts
    part_bits, room = K["stitch_part_bits"][T], K["stitch_room_words"][T]
    single = seg_bits <= part_bits and max_words <= head
    ends, piece_parts, pos, pt, pw = [], 0, 0, 0, 0
    if single:
        ends = [seg_bits]
    else:
        while pt < len(tiles):
            if pw == 0 and tbits[pt] <= part_bits:
                b, t1 = tbits[pt], pt + 1
                while t1 < len(tiles) and b + tbits[t1] <= part_bits:
                    b += tbits[t1]
                    t1 += 1
                pt = t1
            else:
                nwords, sb = tiles[pt]["str_words"], tiles[pt]["str_bits"]
                w1 = min(nwords, pw + room)
                b = (tiles[pt]["dc_bits"] if pw == 0 else 0) + (sb - 32 * pw if w1 == nwords else 32 * (w1 - pw))
                piece_parts += 1
                if w1 >= nwords:
                    pt, pw = pt + 1, 0
                else:
                    pw = w1
            pos += b
            ends.append(pos)
    return dict(offset=offset, tiles=len(tiles), seg_bits=seg_bits, max_words=max_words, merge_fast=fast, merge_writeouts=len(outs),
                merge_writeout_bits=outs, stitch_single=single, stitch_parts=len(ends), stitch_piece_parts=piece_parts, stitch_part_ends=ends)
