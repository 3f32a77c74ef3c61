"""CPU model of the files written with CALLER-SUPPLIED quantisation tables (include/jpeg_compression.h) -- TEST
INFRASTRUCTURE ONLY.

A file with tables of the caller's is the file of the same entry with those two tables in its DQT segment and in its quantiser, and
nothing else changed.  So this module takes explicit tables (uint8 [64], raster order) and puts the steps of scan_model.py and the
oracle together the way the quality-driven models do: the grayscale file, the three-scan colour file, the one-scan colour file with
or without restart intervals.  For the tables of a quality the three are the files of color_model / interleaved_model / restart_model
(tests/test_qtables_host.py pins that).  It also gives the quantiser's decisions for a table -- quant_model's arithmetic with the
constants of jpegamd.table_consts -- and reads the tables back out of a file."""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace

import numpy as np

import color_model as cm
import color_model_422 as m422
import interleaved_model as im
import quant_model as qm
import restart_model as rm
import scan_model as sm

ZZ = np.array(cm.ZIGZAG)                      # zigzag position -> raster k
_DQT_AT = 2 + 18                              # SOI, APP0


def _table(t) -> np.ndarray:
    t = np.ascontiguousarray(t, np.uint8).reshape(64)
    assert t.min() >= 1
    return t


# ---- prefixes -------------------------------------------------------------------------------------------------------------------------
def gray_prefix(oracle, w: int, h: int, qt) -> bytes:
    """The oracle's 328-byte grayscale prefix with this table."""
    qt = _table(qt)
    out = (C.c_uint8 * 400)()
    n = oracle._lib.oracle_jfif_prefix(w, h, qt.ctypes.data, out)
    return bytes(out[:n])


def with_tables(prefix: bytes, lq, cq) -> bytes:
    """A colour prefix of the quality-driven models with these two tables in its DQT segment (ids 0 and 1, zigzag order)."""
    assert prefix[_DQT_AT:_DQT_AT + 5] == b"\xff\xdb\x00\x84\x00" and prefix[_DQT_AT + 69] == 1
    dqt = b"\xff\xdb\x00\x84\x00" + bytes(_table(lq)[ZZ]) + b"\x01" + bytes(_table(cq)[ZZ])
    return prefix[:_DQT_AT] + dqt + prefix[_DQT_AT + len(dqt):]


def color_prefix(w: int, h: int, lq, cq, sub: int) -> bytes:
    """The three-scan prefix: it ends with the Y scan's SOS."""
    return with_tables(m422.prefix_422(w, h, 50) if sub == sm.SUB_422 else cm.color_prefix(w, h, 50, sub), lq, cq)


def one_scan_prefix(w: int, h: int, lq, cq, sub: int, ri: int = 0) -> bytes:
    return with_tables(rm.prefix(w, h, 50, sub, ri) if ri else im.prefix(w, h, 50, sub), lq, cq)


# ---- files ------------------------------------------------------------------------------------------------------------------------------
def gray_file(oracle, plane: np.ndarray, qt) -> bytes:
    """The grayscale file of a plane of luma: prefix, the oracle's entropy-coded segment of its coefficients, EOI."""
    h, w = plane.shape
    return gray_prefix(oracle, w, h, qt) + oracle.entropy(sm.plane_zigzag(oracle, plane, _table(qt))) + b"\xff\xd9"


def color_file(oracle, y, cb, cr, lq, cq, sub: int) -> bytes:
    """The three-scan file of samples that are Y, Cb and Cr at `sub` (4:4:4, 4:2:0 or 4:2:2)."""
    h, w = y.shape
    parts = [color_prefix(w, h, lq, cq, sub), sm.pack_scan(oracle, sm.plane_zigzag(oracle, y, _table(lq)), False)]
    for comp, plane in ((2, cb), (3, cr)):
        parts += [sm.sos(comp), sm.pack_scan(oracle, sm.plane_zigzag(oracle, plane, _table(cq)), True)]
    return b"".join(parts) + b"\xff\xd9"


def one_scan_file(oracle, y, cb, cr, lq, cq, sub: int, ri: int = 0) -> bytes:
    """The one-scan file of the same samples, with restart intervals of `ri` MCUs (0: none) and the Annex K Huffman tables."""
    h, w = y.shape
    hs, vs, bw, bh, mx, my = im.geometry(w, h, sub)
    ny, m = hs * vs, mx * my
    zy, _ = sm.mcu_order_luma(sm.plane_zigzag(oracle, y, _table(lq)), bw, bh, hs, vs, mx, my)
    zcb, zcr = sm.plane_zigzag(oracle, cb, _table(cq)), sm.plane_zigzag(oracle, cr, _table(cq))
    assert zcb.shape[0] == zcr.shape[0] == m
    step = ri or m
    bits, mcu_bits = sm.scan_bits(sm.scan_symbols(oracle, zy, zcb, zcr, ny, step), sm.std_tables(False), sm.std_tables(True), ny)
    body, _ = sm.frame_intervals(bits, mcu_bits, step, rm.seg_mcus(sub))
    return one_scan_prefix(w, h, lq, cq, sub, ri) + body + b"\xff\xd9"


def rgb_color_file(oracle, rgb, lq, cq, sub: int) -> bytes:
    return color_file(oracle, *sm.planes_of(rgb, sub), lq, cq, sub)


def rgb_one_scan_file(oracle, rgb, lq, cq, sub: int, ri: int = 0) -> bytes:
    return one_scan_file(oracle, *sm.planes_of(rgb, sub), lq, cq, sub, ri)


def array(fn, oracle, *args):
    """color_model.memo for calls that pass tables: one cache for the host and the GPU suite."""
    return cm.memo(fn, oracle, *[np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a for a in args])


# ---- what a file carries ----------------------------------------------------------------------------------------------------------------
def dqt_tables(data: bytes) -> dict:
    """A marker walk up to the first SOS: {table id: uint8 [64] in RASTER order} of every 8-bit table of every DQT segment."""
    assert data[:2] == b"\xff\xd8"
    at, out = 2, {}
    while True:
        assert data[at] == 0xFF, at
        marker, n = data[at + 1], int.from_bytes(data[at + 2:at + 4], "big")
        if marker == 0xDA:
            return out
        if marker == 0xDB:
            body = data[at + 4:at + 2 + n]
            assert len(body) % 65 == 0
            for k in range(0, len(body), 65):
                assert body[k] >> 4 == 0 and body[k] not in out, "one 8-bit table per id"
                raster = np.zeros(64, np.uint8)
                raster[ZZ] = np.frombuffer(body[k + 1:k + 65], np.uint8)
                out[body[k]] = raster
        at += 2 + n


def decode(data: bytes) -> np.ndarray:
    """PIL's fully loaded pixels of a file."""
    import io

    from PIL import Image
    img = Image.open(io.BytesIO(data))
    img.load()
    return np.asarray(img)


# ---- the quantiser's decisions ----------------------------------------------------------------------------------------------------------
def decisions(jpegamd, blocks, table):
    """quant_model.evaluate's flags for an arbitrary table: centred blocks int [n, 64] -> flags bool [n, 64] by zigzag position (the
    site takes the exact-order fallback) and mask uint64 [n], the same as bits by raster k (jpegamd_debug_stages' exact_mask)."""
    c = jpegamd.table_consts(table)
    dc_off = qm.f64(qm.f32(jpegamd.mfma_consts(50)["dc_off"]))           # (table-independent)
    acc, _ = qm.accumulate(jpegamd, blocks)
    acc[:, 0] = (acc[:, 0].astype(qm.f64) - dc_off).astype(qm.f32)
    acc[:, 0] = np.abs(acc[:, 0])                                         # the DC lanes quantise |S|
    zc = qm.fma32(acc, c["qmul"].astype(qm.f32)[None, :], c["qadd"].astype(qm.f32)[None, :])
    flags = qm.fract_le(zc, c["qthr"].astype(qm.f32)[None, :])
    flags[:, 0] = False                                                   # a DC is never flagged
    mask = np.zeros(len(flags), np.uint64)
    for z in range(1, 64):
        mask |= flags[:, z].astype(np.uint64) << np.uint64(ZZ[z])
    return SimpleNamespace(flags=flags, mask=mask)
