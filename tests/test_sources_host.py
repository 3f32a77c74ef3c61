"""What the launches of a YCbCr batch read, on the CPU: jpegamd_debug_ycbcr_sources over every chroma layout, sample format, range
and first plane of a chroma launch, against the table written out here -- the loader's layout, the luma or the chroma tables, the
range expansion, and the select word wherever the loader reads it -- and the kinds of input the encode entry refuses.  No device."""
from __future__ import annotations

import ctypes as C
import itertools

import pytest

ERR_ARG = -1
# TileSource::layout (jpegamd_internal.h)
SRC_PLANE, SRC_PAIR, SRC_QUAD, SRC_PLANE16, SRC_PAIR16 = 1, 4, 5, 6, 7
PLANES, CBCR, CRCB, YUYV, UYVY = 0, 1, 2, 4, 5            # JPEGAMD_CHROMA_*
S8, S10_MSB, S10_LSB = 0, 1, 2                             # JPEGAMD_SAMPLES_*
FULL, LIMITED = 0, 1                                       # JPEGAMD_RANGE_*
LAYOUTS, FORMATS, RANGES, FIRSTS = (PLANES, CBCR, CRCB, YUYV, UYVY), (S8, S10_MSB, S10_LSB), (FULL, LIMITED), (0, 1, 2, 3)
SHIFT = {S10_MSB: 6, S10_LSB: 0}
NOT_READ = None


def expected_y(layout, fmt):
    """-> (layout, select word or NOT_READ) of the Y launch; always the luma tables."""
    if fmt != S8:
        return SRC_PLANE16, SHIFT[fmt] << 16
    if layout == YUYV:
        return SRC_PAIR, 0
    if layout == UYVY:
        return SRC_PAIR, 1
    return SRC_PLANE, NOT_READ


def expected_chroma(layout, fmt, first):
    """-> (layout, select word or NOT_READ) of a chroma launch whose first plane is `first`; always the chroma tables."""
    crcb = 1 if layout == CRCB else 0
    if layout in (YUYV, UYVY):
        return SRC_QUAD, (first & 1) | (0x100 if layout == YUYV else 0)
    if layout == PLANES:
        return (SRC_PLANE, NOT_READ) if fmt == S8 else (SRC_PLANE16, SHIFT[fmt] << 16)
    if fmt == S8:
        return SRC_PAIR, (first & 1) ^ crcb
    return SRC_PAIR16, ((first & 1) ^ crcb) | (SHIFT[fmt] << 16)


def sources(jpegamd, layout, fmt, rng, first):
    out = (C.c_uint32 * 8)(*([0xDEADBEEF] * 8))
    rc = jpegamd.lib.jpegamd_debug_ycbcr_sources(layout, fmt, rng, first, out)
    return rc, list(out)


def test_the_entry_is_internal(jpegamd):
    assert hasattr(C.CDLL(str(jpegamd.LIB_PATH)), "jpegamd_debug_ycbcr_sources")
    assert "jpegamd_debug_ycbcr_sources" not in jpegamd.HEADER_PATH.read_text()
    assert "jpegamd_debug_ycbcr_sources" not in jpegamd.EXPORTED


def test_every_kind_of_ycbcr_input_maps_to_its_sources(jpegamd):
    seen = 0
    for layout, fmt, rng, first in itertools.product(LAYOUTS, FORMATS, RANGES, FIRSTS):
        rc, out = sources(jpegamd, layout, fmt, rng, first)
        if layout in (YUYV, UYVY) and fmt != S8:           # a packed plane of 16-bit words is not taken
            assert rc == ERR_ARG and out == [0xDEADBEEF] * 8, (layout, fmt, rng, first)
            continue
        assert rc == 0, (layout, fmt, rng, first)
        for got, (want_layout, want_select), chroma in ((out[:4], expected_y(layout, fmt), 0),
                                                        (out[4:], expected_chroma(layout, fmt, first), 1)):
            assert got[0] == want_layout, (layout, fmt, rng, first, chroma, got)
            assert got[1] == chroma, (layout, fmt, rng, first, chroma, got)           # luma / chroma tables
            assert got[2] == (1 if rng == LIMITED else 0), (layout, fmt, rng, first, chroma, got)
            if want_select is not NOT_READ:
                assert got[3] == want_select, (layout, fmt, rng, first, chroma, hex(got[3]))
        seen += 1
    assert seen == (3 * 3 + 2 * 1) * 2 * 4


def test_the_table_rows_spelled_out(jpegamd):
    """A few rows by hand, so that a slip in the helpers above cannot hide one in the library."""
    nv12 = sources(jpegamd, CBCR, S8, FULL, 0)[1]
    assert nv12[:3] == [SRC_PLANE, 0, 0] and nv12[4:] == [SRC_PAIR, 1, 0, 0]               # (a plane's loader does not read the word)
    assert sources(jpegamd, CRCB, S8, LIMITED, 2)[1][4:] == [SRC_PAIR, 1, 1, 1]
    assert sources(jpegamd, CRCB, S8, FULL, 3)[1][4:] == [SRC_PAIR, 1, 0, 0]
    assert sources(jpegamd, YUYV, S8, FULL, 1)[1] == [SRC_PAIR, 0, 0, 0, SRC_QUAD, 1, 0, 0x101]
    assert sources(jpegamd, UYVY, S8, LIMITED, 2)[1] == [SRC_PAIR, 0, 1, 1, SRC_QUAD, 1, 1, 0]
    assert sources(jpegamd, PLANES, S10_MSB, FULL, 1)[1] == [SRC_PLANE16, 0, 0, 6 << 16, SRC_PLANE16, 1, 0, 6 << 16]
    assert sources(jpegamd, PLANES, S10_LSB, LIMITED, 0)[1] == [SRC_PLANE16, 0, 1, 0, SRC_PLANE16, 1, 1, 0]
    assert sources(jpegamd, CBCR, S10_MSB, LIMITED, 3)[1] == [SRC_PLANE16, 0, 1, 6 << 16, SRC_PAIR16, 1, 1, 1 | (6 << 16)]
    assert sources(jpegamd, CRCB, S10_LSB, FULL, 3)[1] == [SRC_PLANE16, 0, 0, 0, SRC_PAIR16, 1, 0, 0]
    assert sources(jpegamd, CRCB, S10_MSB, FULL, 0)[1][4:] == [SRC_PAIR16, 1, 0, 1 | (6 << 16)]


@pytest.mark.parametrize("layout,fmt,rng", [(3, S8, FULL), (6, S8, FULL), (-1, S8, FULL), (PLANES, 3, FULL), (PLANES, -1, FULL),
                                            (CBCR, S8, 2), (CBCR, S8, -1), (YUYV, S10_MSB, FULL), (UYVY, S10_LSB, LIMITED)])
def test_what_the_encode_entry_refuses_is_refused(jpegamd, layout, fmt, rng):
    for first in FIRSTS:
        rc, out = sources(jpegamd, layout, fmt, rng, first)
        assert rc == ERR_ARG and out == [0xDEADBEEF] * 8
    assert jpegamd.lib.jpegamd_debug_ycbcr_sources(PLANES, S8, FULL, 0, None) == ERR_ARG
