"""Colour batches (jpegamd_encode_color_batch_async) on the CPU: the exported symbol, the argument checks that return before the
context is touched, encode_tensor_batch's layout checks, and the host function that groups the chroma planes of a batch into
launches on a context's limits.  Nothing here needs a device."""
from __future__ import annotations

import ctypes as C

import pytest

ERR_ARG, ERR_TOO_LARGE = -1, -5


def test_color_batch_symbol_is_exported(jpegamd):
    assert "jpegamd_encode_color_batch_async" in jpegamd.EXPORTED
    assert hasattr(C.CDLL(str(jpegamd.LIB_PATH)), "jpegamd_encode_color_batch_async")
    assert hasattr(jpegamd.Encoder, "encode_color_batch_async") and callable(jpegamd.encode_tensor_batch)


def _call(jpegamd, ctx, imgs, count, sub, outs=True, sizes=True, null_out=None):
    n = max(len(imgs), 1)
    arr = (jpegamd.Image * n)(*imgs) if imgs else None
    out_arr = (C.c_void_p * 40)(*([C.c_void_p(0x1000)] * 40)) if outs else None
    size_arr = (C.c_void_p * 40)(*([C.c_void_p(0x2000)] * 40)) if sizes else None
    if null_out is not None:
        out_arr[null_out] = None
    return jpegamd.lib.jpegamd_encode_color_batch_async(ctx, arr, count, sub, out_arr, 1 << 20, size_arr, None)


def test_argument_checks_come_before_the_context(jpegamd):
    """Every bad argument is refused with JPEGAMD_ERR_ARG before the context is read: the calls below pass a block of zeros
    where the context would be, and a check that came too late would read it."""
    fake = (C.c_uint8 * (1 << 16))()
    ctx = C.cast(fake, C.c_void_p)

    def img(ptr=0x10000, w=64, h=32, stride=192, bottom_up=0, order=jpegamd.ORDER_RGB, q=0):
        return jpegamd.Image(ptr, w, h, stride, bottom_up, order, q)

    good = [img(0x10000 + 0x10000 * i) for i in range(40)]
    s420, s444 = jpegamd.SUBSAMPLE_420, jpegamd.SUBSAMPLE_444
    assert _call(jpegamd, None, good[:2], 2, s420) == ERR_ARG                         # null context
    assert _call(jpegamd, ctx, good[:1], 0, s420) == ERR_ARG                          # count 0
    assert _call(jpegamd, ctx, good[:33], 33, s420) == ERR_ARG                        # count 33
    assert _call(jpegamd, ctx, [], 1, s420) == ERR_ARG                                # no images
    assert _call(jpegamd, ctx, good[:2], 2, s420, outs=False) == ERR_ARG
    assert _call(jpegamd, ctx, good[:2], 2, s420, sizes=False) == ERR_ARG
    assert _call(jpegamd, ctx, good[:3], 3, s420, null_out=2) == ERR_ARG
    for sub in (0, 3, -1):
        assert _call(jpegamd, ctx, good[:2], 2, sub) == ERR_ARG, sub
    gray = [img(0x10000 * (i + 1), stride=64, order=jpegamd.ORDER_GRAY) for i in range(2)]
    assert _call(jpegamd, ctx, gray, 2, s444) == ERR_ARG
    assert _call(jpegamd, ctx, [img(order=7)], 1, s420) == ERR_ARG
    for odd in (img(w=65), img(h=31), img(stride=196), img(bottom_up=1), img(order=jpegamd.ORDER_BGR), img(q=90), img(ptr=0)):
        assert _call(jpegamd, ctx, [good[0], odd, good[2]], 3, s420) == ERR_ARG


def test_encode_tensor_batch_rejects_bad_layouts(jpegamd):
    torch = pytest.importorskip("torch")
    bad = [
        torch.zeros(2, 8, 8, 3, dtype=torch.float32),                  # dtype
        torch.zeros(2, 8, 8, 3, dtype=torch.int16),
        torch.zeros(8, 8, dtype=torch.uint8),                          # one picture, not a batch
        torch.zeros(2, 8, 8, 4, dtype=torch.uint8),                    # four channels
        torch.zeros(2, 2, 8, 8, 3, dtype=torch.uint8),                 # five dimensions
        torch.zeros(2, 8, 8, 3, dtype=torch.uint8).permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1),   # planar channels
        torch.zeros(2, 8, 16, 3, dtype=torch.uint8)[:, :, ::2],        # strided pixels
        torch.zeros(2, 8, 16, dtype=torch.uint8)[:, :, ::2],
        torch.zeros(2, 16, 8, dtype=torch.uint8).transpose(1, 2),      # columns as rows
        torch.zeros(0, 8, 8, 3, dtype=torch.uint8),                    # no picture
        torch.zeros(2, 8, 8, 3, dtype=torch.uint8),                    # a host tensor
    ]
    for t in bad:
        with pytest.raises(ValueError):
            jpegamd.encode_tensor_batch(t)


def _tiles(w, h):
    return ((h + 7) // 8) * (((w + 7) // 8 + 31) // 32)


def _segs(w, h, seg_tiles):
    return ((h + 7) // 8) * (((w + 7) // 8 + 32 * seg_tiles - 1) // (32 * seg_tiles))


def _check_plan(jpegamd, mw, mh, w, h, count, sub, pipeline=0):
    group, launches, seg_tiles, stitch = jpegamd._chroma_groups(mw, mh, w, h, count, sub, pipeline)
    cw, ch = ((w + 1) // 2, (h + 1) // 2) if sub == jpegamd.SUBSAMPLE_420 else (w, h)
    planes = 2 * count
    assert 1 <= group <= jpegamd.MAX_BATCH and seg_tiles in (8, 16)
    assert launches == -(-planes // group) and (launches - 1) * group < planes, (group, launches)
    assert group * _tiles(cw, ch) <= _tiles(mw, mh), (mw, mh, w, h, count, group)
    assert group * _segs(cw, ch, seg_tiles) <= _segs(mw, mh, 8), (mw, mh, w, h, count, group)
    return group, launches, seg_tiles, stitch


def test_chroma_groups_444_on_a_batch_context_takes_several_launches(jpegamd):
    for (w, h, count) in [(1024, 1024, 8), (257, 129, 3), (64, 64, 8), (8192, 8192, 2), (33, 17, 32), (1, 1, 1)]:
        group, launches, _, _ = _check_plan(jpegamd, w, count * h, w, h, count, jpegamd.SUBSAMPLE_444)
        assert launches > 1, (w, h, count, group)


def test_chroma_groups_420_up_to_16_pictures_is_one_launch(jpegamd):
    for (w, h) in [(16, 16), (640, 480), (1024, 1024), (4096, 4096), (8192, 8192), (2048, 16), (65520, 16), (16, 65520)]:
        for count in (1, 2, 3, 4, 8, 15, 16):
            group, launches, _, _ = _check_plan(jpegamd, w, count * h, w, h, count, jpegamd.SUBSAMPLE_420)
            assert launches == 1 and group == 2 * count, (w, h, count, group)
    # 17 pictures and more: 34 planes need two launches (kMaxBatch = 32)
    assert _check_plan(jpegamd, 64, 17 * 64, 64, 64, 17, jpegamd.SUBSAMPLE_420)[1] == 2


def test_chroma_groups_fit_at_tiny_heights_and_every_pipeline(jpegamd):
    """At H = 8 a plane is one block row, like the picture, and the per-row rounding of tiles can make two chroma planes need
    more tiles than one luma picture (8 x 8: one tile each): the groups must still fit the context."""
    assert _check_plan(jpegamd, 8, 8, 8, 8, 1, jpegamd.SUBSAMPLE_420)[:2] == (1, 2)
    for pipeline in (jpegamd.PIPELINE_AUTO, jpegamd.PIPELINE_PAIR, jpegamd.PIPELINE_STITCH):
        for sub in (jpegamd.SUBSAMPLE_420, jpegamd.SUBSAMPLE_444):
            for (w, h) in [(8, 8), (9, 8), (264, 8), (65535, 8), (8, 65535), (4097, 9), (2056, 65535), (1, 1), (33, 17)]:
                for count in (1, 2, 3, 7, 16, 17, 32):
                    if count * h > 65535 * 32:
                        continue
                    _check_plan(jpegamd, w, count * h, w, h, count, sub, pipeline)


def test_chroma_groups_pipeline_choice(jpegamd):
    # AUTO at 2056 x 65535: Y takes k_stitch (16 384 segments), the 4:2:0 planes (4 096 segments) the pair
    assert _check_plan(jpegamd, 2056, 2 * 65535, 2056, 65535, 2, jpegamd.SUBSAMPLE_420)[3] is False
    assert _check_plan(jpegamd, 2056, 2 * 65535, 2056, 65535, 2, jpegamd.SUBSAMPLE_444)[3] is True
    assert _check_plan(jpegamd, 64, 64, 64, 64, 1, jpegamd.SUBSAMPLE_420, jpegamd.PIPELINE_STITCH)[2:] == (16, True)
    # a context that cannot hold one plane: refused
    with pytest.raises(jpegamd.JpegAmdError):
        jpegamd._chroma_groups(8, 8, 64, 64, 1, jpegamd.SUBSAMPLE_444)
