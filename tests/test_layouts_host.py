"""Planar (channels-first) and 4-byte-pixel input on the CPU: the exported symbol and the ctypes mirror of the header, the argument
checks of jpegamd_encode_planar_batch_async that return before the context is touched, which entries take the 4-byte orders, and
the layout checks of encode_tensor / encode_tensor_batch.  Nothing here needs a device."""
from __future__ import annotations

import ctypes as C

import pytest

ERR_ARG = -1
CAP = 1 << 20


def test_planar_symbol_and_constants(jpegamd):
    assert "jpegamd_encode_planar_batch_async" in jpegamd.EXPORTED
    assert hasattr(C.CDLL(str(jpegamd.LIB_PATH)), "jpegamd_encode_planar_batch_async")
    assert "jpegamd_encode_planar_batch_async" in jpegamd.HEADER_PATH.read_text()
    assert (jpegamd.ORDER_RGBA, jpegamd.ORDER_BGRA) == (3, 4)
    assert hasattr(jpegamd.Encoder, "planar_image") and hasattr(jpegamd.Encoder, "encode_planar_batch_async")
    # JpegAmdPlanarImage: three pointers, five int32, padded to the pointers' alignment
    assert C.sizeof(jpegamd.PlanarImage) == 3 * 8 + 5 * 4 + 4
    assert jpegamd.PlanarImage.width.offset == 24 and jpegamd.PlanarImage.quality.offset == 40
    img = jpegamd.Encoder.planar_image((0x100, 0x200, 0x300), 5, 4, 8, True, 90)
    assert list(img.plane) == [0x100, 0x200, 0x300]
    assert (img.width, img.height, img.row_stride, img.bottom_up, img.quality) == (5, 4, 8, 1, 90)


def _fake_context():
    """A block of zeros where the context would be: a check that came too late would read it."""
    fake = (C.c_uint8 * (1 << 16))()
    return fake, C.cast(fake, C.c_void_p)


def _planar(jpegamd, ctx, imgs, count, sub, outs=True, sizes=True, null_out=None, null_size=None):
    n = max(len(imgs), 1)
    arr = (jpegamd.PlanarImage * n)(*imgs) if imgs else None
    out_arr = (C.c_void_p * 40)(*([C.c_void_p(0x1000)] * 40)) if outs else None
    size_arr = (C.c_void_p * 40)(*([C.c_void_p(0x2000)] * 40)) if sizes else None
    if null_out is not None:
        out_arr[null_out] = None
    if null_size is not None:
        size_arr[null_size] = None
    return jpegamd.lib.jpegamd_encode_planar_batch_async(ctx, arr, count, sub, out_arr, CAP, size_arr, None)


def test_planar_argument_checks_come_before_the_context(jpegamd):
    keep, ctx = _fake_context()

    def img(base=0x100000, w=64, h=32, stride=64, bottom_up=0, q=0, planes=None):
        return jpegamd.Encoder.planar_image(planes or (base, base + 0x10000, base + 0x20000), w, h, stride, bottom_up, q)

    good = [img(0x100000 * (i + 1)) for i in range(40)]
    s420, s444 = jpegamd.SUBSAMPLE_420, jpegamd.SUBSAMPLE_444
    for sub in (0, s444, s420):
        assert _planar(jpegamd, None, good[:2], 2, sub) == ERR_ARG                       # null context
        assert _planar(jpegamd, ctx, good[:1], 0, sub) == ERR_ARG                        # count 0
        assert _planar(jpegamd, ctx, good[:33], 33, sub) == ERR_ARG                      # count 33
        assert _planar(jpegamd, ctx, [], 1, sub) == ERR_ARG                              # no images
        assert _planar(jpegamd, ctx, good[:2], 2, sub, outs=False) == ERR_ARG
        assert _planar(jpegamd, ctx, good[:2], 2, sub, sizes=False) == ERR_ARG
        assert _planar(jpegamd, ctx, good[:3], 3, sub, null_out=2) == ERR_ARG
        assert _planar(jpegamd, ctx, good[:3], 3, sub, null_size=1) == ERR_ARG
        for k in range(3):                                                               # a null plane, first or later picture
            planes = [0x5000, 0x6000, 0x7000]
            planes[k] = None
            assert _planar(jpegamd, ctx, [img(planes=tuple(planes))], 1, sub) == ERR_ARG
            assert _planar(jpegamd, ctx, [good[0], img(planes=tuple(planes)), good[2]], 3, sub) == ERR_ARG
        assert _planar(jpegamd, ctx, [img(stride=63)], 1, sub) == ERR_ARG                # row_stride < width
        for bad in (img(w=0), img(w=-3), img(h=0), img(h=-1)):
            assert _planar(jpegamd, ctx, [bad], 1, sub) == ERR_ARG
        for odd in (img(w=65, stride=65), img(h=31), img(stride=68), img(bottom_up=1), img(q=90)):
            assert _planar(jpegamd, ctx, [good[0], odd, good[2]], 3, sub) == ERR_ARG
    for sub in (3, -1):
        assert _planar(jpegamd, ctx, good[:2], 2, sub) == ERR_ARG, sub


def _packed_calls(jpegamd, ctx, im):
    """The four entries that take the 4-byte orders, each on one image -> their return codes."""
    lib = jpegamd.lib
    one_out, one_size = (C.c_void_p * 1)(0x1000), (C.c_void_p * 1)(0x2000)
    arr = (jpegamd.Image * 1)(im)
    return [
        lib.jpegamd_encode_async(ctx, C.byref(im), 0x1000, CAP, 0x2000, 1, None),
        lib.jpegamd_encode_batch_async(ctx, arr, 1, one_out, CAP, one_size, 1, None),
        lib.jpegamd_encode_color_async(ctx, C.byref(im), jpegamd.SUBSAMPLE_420, 0x1000, CAP, 0x2000, None),
        lib.jpegamd_encode_color_batch_async(ctx, arr, 1, jpegamd.SUBSAMPLE_444, one_out, CAP, one_size, None),
    ]


def test_four_byte_orders_stride_and_unknown_orders(jpegamd):
    keep, ctx = _fake_context()
    for order in (jpegamd.ORDER_RGBA, jpegamd.ORDER_BGRA):
        for stride in (4 * 64 - 1, 3 * 64, 64):                                           # row_stride < 4 * width
            assert _packed_calls(jpegamd, ctx, jpegamd.Image(0x10000, 64, 32, stride, 0, order, 0)) == [ERR_ARG] * 4, (order, stride)
    for order in (5, 7):
        assert _packed_calls(jpegamd, ctx, jpegamd.Image(0x10000, 64, 32, 4 * 64, 0, order, 0)) == [ERR_ARG] * 4, order


def test_four_byte_orders_are_refused_by_every_other_entry(jpegamd):
    keep, ctx = _fake_context()
    lib = jpegamd.lib
    for order in (jpegamd.ORDER_RGBA, jpegamd.ORDER_BGRA):
        im = jpegamd.Image(0x10000, 64, 32, 4 * 64, 0, order, 0)
        assert lib.jpegamd_encode_rows_async(ctx, C.byref(im), 0, 4, None) == ERR_ARG
        assert lib.jpegamd_export_segments(ctx, C.byref(im), 0, 4, 0x1000, 1 << 10, 0x2000, 0x3000, None) == ERR_ARG
        assert lib.jpegamd_import_segments(ctx, C.byref(im), 0, 4, 0x1000, 0x2000, None) == ERR_ARG
        assert lib.jpegamd_finalize_async(ctx, C.byref(im), 0x1000, CAP, 0x2000, 1, None) == ERR_ARG
        assert lib.jpegamd_debug_stages(ctx, C.byref(im), None, None, None) == ERR_ARG
        dto = jpegamd.DTO()
        dto.width, dto.height, dto.row_stride, dto.channel_order = 64, 32, 4 * 64, order
        dto.r_phy_ptr, dto.huff_phy_ptr, dto.huff_size = 0x10000, 0x1000, CAP
        assert lib.convertToJpeg(C.byref(dto)) == ERR_ARG


def test_named_layouts_reject_bad_tensors(jpegamd):
    torch = pytest.importorskip("torch")
    u8 = torch.uint8
    bad = [
        (torch.zeros(2, 3, 8, 8, dtype=torch.float32), "chw"),                           # dtype
        (torch.zeros(2, 8, 8, 4, dtype=torch.int16), "rgba"),
        (torch.zeros(2, 8, 8, 3, dtype=torch.float32), "hwc"),
        (torch.zeros(2, 4, 8, 8, dtype=u8), "chw"),                                      # channel count
        (torch.zeros(2, 8, 8, 3, dtype=u8), "chw"),
        (torch.zeros(2, 8, 8, 3, dtype=u8), "rgba"),
        (torch.zeros(2, 8, 8, 3, dtype=u8), "bgra"),
        (torch.zeros(2, 8, 8, 4, dtype=u8), "hwc"),
        (torch.zeros(3, 8, 8, dtype=u8), "chw"),                                         # one picture, not a batch
        (torch.zeros(2, 3, 8, 16, dtype=u8)[:, :, :, ::2], "chw"),                       # strided pixels
        (torch.zeros(2, 8, 16, 4, dtype=u8)[:, :, ::2], "rgba"),
        (torch.zeros(2, 8, 8, 8, dtype=u8)[:, :, :, ::2], "bgra"),
        (torch.zeros(2, 8, 8, 3, dtype=u8).permute(0, 3, 1, 2), "chw"),                  # channels-last memory seen as [N, 3, H, W]
        ([torch.zeros(2, 8, 8, dtype=u8), torch.zeros(2, 8, 12, dtype=u8)[:, :, :8], torch.zeros(2, 8, 8, dtype=u8)], "chw"),   # row strides 8, 12, 8
        ([torch.zeros(2, 8, 8, dtype=u8)] * 2, "chw"),                                   # two planes
        ([torch.zeros(2, 8, 8, dtype=u8)] * 3, "rgba"),
        (torch.zeros(2, 3, 8, 8, dtype=u8), "nchw"),                                     # unknown names
        (torch.zeros(2, 3, 8, 8, dtype=u8), "CHW"),
        (torch.zeros(2, 3, 8, 8, dtype=u8), 3),
        (torch.zeros(0, 3, 8, 8, dtype=u8), "chw"),                                      # no picture
        (torch.zeros(0, 8, 8, 4, dtype=u8), "rgba"),
    ]
    for t, layout in bad:
        with pytest.raises(ValueError) as err:
            jpegamd.encode_tensor_batch(t, layout=layout)
        assert "device tensor" not in str(err.value), (layout, str(err.value))


def test_well_formed_host_tensors_only_lack_a_device(jpegamd):
    torch = pytest.importorskip("torch")
    u8 = torch.uint8
    big = torch.zeros(4, 3, 20, 24, dtype=u8)
    good = [
        (torch.zeros(2, 3, 8, 8, dtype=u8), "chw"),
        (big[::2, :, 2:18, 4:20], "chw"),                                                # a crop: strided rows, planes and pictures
        ([torch.zeros(2, 8, 8, dtype=u8) for _ in range(3)], "chw"),                     # three separate tensors
        (torch.zeros(2, 8, 8, 4, dtype=u8), "rgba"),
        (torch.zeros(2, 8, 16, 4, dtype=u8)[:, :, :8], "bgra"),                          # strided rows
        (torch.zeros(2, 8, 8, 3, dtype=u8), "hwc"),
    ]
    for t, layout in good:
        with pytest.raises(ValueError, match="device tensor"):
            jpegamd.encode_tensor_batch(t, layout=layout)
    for t, layout in [(torch.zeros(3, 8, 8, dtype=u8), "chw"), (torch.zeros(8, 8, 4, dtype=u8), "bgra"), (torch.zeros(8, 8, 3, dtype=u8), "hwc")]:
        with pytest.raises(ValueError, match="device tensor"):
            jpegamd.encode_tensor(t, layout=layout)
    with pytest.raises(ValueError):
        jpegamd.encode_tensor(torch.zeros(2, 3, 8, 8, dtype=u8), layout="chw")           # a batch is not one picture
