"""k_tile_encode's luma stash, made on demand: a wave that codes a tile without an exact-order event and then one with an event must read
THAT tile's luma, not the item list the tile before left in the same words.  The picture of tests/stash_sequence.py has three tiles per
wave of a full launch, about half of them with an event, in a seeded order (its premise: tests/test_stash_sequence_host.py).  Every
file is the oracle's for the same pixels, every fallback count the model's.  Never product against product.  Needs an MI355X."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import stash_sequence as ss
from gpu_support import block_rows_reversed, dev, device_encode, upload_pixels     # noqa: F401
from gpu_support import encode_gray_planes as encode_gray
from gpu_support import gray_bmp_sized as gray_bmp

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pic(jpegamd, oracle):
    """The picture, its 24-bit BMP (R = G = B: the luma is the sample itself) and the oracle's file: made once, never changed."""
    p = ss.picture(jpegamd, oracle)
    bmp = gray_bmp(p.plane)
    p.bmp, p.file = bmp, oracle.encode_bmp(bmp, p.quality)
    return p


def test_bgr_bottom_up(jpegamd, dev, pic):
    """The bench's source: 3 bytes per pixel, BGR, bottom-up, through jpegamd_encode_async."""
    h, w = pic.plane.shape
    enc = jpegamd.Encoder(w, h)
    got, st = device_encode(jpegamd, enc, pic.bmp, dev, quality=pic.quality)
    assert st.exact_fallbacks == pic.events, (st.exact_fallbacks, pic.events)
    assert got == pic.file


def test_gray(jpegamd, dev, pic):
    """One byte per sample (the plane loader)."""
    h, w = pic.plane.shape
    enc = jpegamd.Encoder(w, h)
    files, st = encode_gray(jpegamd, enc, [pic.plane], dev, pic.quality)
    assert st.exact_fallbacks == pic.events, (st.exact_fallbacks, pic.events)
    assert files == [pic.file]


def test_second_picture_of_a_batch(jpegamd, oracle, dev, pic):
    """One launch over two pictures: the tile range crosses the image boundary, and the waves that start in the first picture (the same
    tiles in the opposite order) go on in the second."""
    h, w = pic.plane.shape
    first = block_rows_reversed(pic.plane)
    enc = jpegamd.Encoder(w, 2 * h)
    files, st = encode_gray(jpegamd, enc, [first, pic.plane], dev, pic.quality)
    assert st.exact_fallbacks == 2 * pic.events, (st.exact_fallbacks, pic.events)       # (the first picture holds the same tiles)
    assert files[1] == pic.file
    assert files[0] == oracle.encode_bmp(gray_bmp(first), pic.quality)


def test_stamped_variant_through_the_dto(jpegamd, dev, pic):
    """convertToJpeg runs the stamped compilation of the kernel: the reference's bytes, and the five stage counters that exist as
    instructions are non-zero (the stash's own bucket is one of four that make up cycles_color_conversion), as
    tests/test_gpu_parity.py::test_dto_boundary asks."""
    lib = jpegamd.lib
    h, w = pic.plane.shape
    assert lib.JpegCompression_Init() == 0
    try:
        img, px = upload_pixels(pic.bmp, jpegamd, dev)
        cap = w * h
        huff = torch.zeros(cap, dtype=torch.uint8, device=dev)
        y, dct = (ctypes.c_int8 * 64)(), (ctypes.c_float * 64)()
        quant, zz = (ctypes.c_int16 * 64)(), (ctypes.c_int16 * 64)()
        dto = jpegamd.DTO(width=w, height=h, r_phy_ptr=px.data_ptr(), huff_phy_ptr=huff.data_ptr(), huff_size=cap,
                          y_phy_ptr=ctypes.addressof(y), dct_phy_ptr=ctypes.addressof(dct), quant_phy_ptr=ctypes.addressof(quant),
                          zigzag_phy_ptr=ctypes.addressof(zz), row_stride=img.row_stride, bottom_up=img.bottom_up,
                          channel_order=jpegamd.ORDER_BGR, quality=pic.quality)
        assert lib.convertToJpeg(ctypes.byref(dto)) == 0
        assert bytes(huff[:dto.huff_size].cpu().numpy()) == pic.file[328:-2]
        stages = [dto.cycles_color_conversion, dto.cycles_dct, dto.cycles_quantization, dto.cycles_rle, dto.cycles_huffman]
        assert all(c > 0 for c in stages) and dto.cycles_zigzag == 0 and dto.cycles_total > 0, stages
        assert sum(stages) <= dto.cycles_total
    finally:
        assert lib.JpegCompression_DeInit() == 0
