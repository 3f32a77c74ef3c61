"""Which entry of libjpegamd.so a binding call reaches, with what arguments in what order.  `jpegamd.lib` is replaced by a stand-in
that records every call and returns a set code: nothing is loaded and no device is touched.  The GPU suite cannot see this where
two entries write the same bytes."""
from __future__ import annotations

import ctypes as C
import re

import pytest

from conftest import PKG

HANDLE = 0x5150
SUB, RANGE, FORMAT, MATRIX, RESTART, CAP, STREAM = 101, 102, 103, 104, 105, 106, 107    # one value per scalar: a swap of two shows
OUTS, SIZES = [0x2010, 0x2020], [0x3010, 0x3020]
OUT, SIZE = 0x2030, 0x3030
ROW_BEGIN, ROW_END, DENSE, DENSE_CAP, META, TOTAL = 108, 109, 0x4010, 110, 0x4020, 0x4030


class Recorder:
    """Every attribute is an entry that appends (name, args) to `calls` and returns `code`."""

    def __init__(self, code: int = 0):
        self.calls, self.code = [], code

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return self.code
        return entry


def plain(x):
    """A ctypes argument as plain Python values: arrays as lists, structs as dicts, byref(x) as x, pointers as integers (None: null)."""
    if isinstance(x, C.Array):
        return [plain(e) for e in x]
    if isinstance(x, C.Structure):
        return {f[0]: plain(getattr(x, f[0])) for f in x._fields_}
    if isinstance(x, C._SimpleCData):
        return x.value
    if hasattr(x, "_obj"):
        return plain(x._obj)
    return x


@pytest.fixture
def rec(jpegamd, monkeypatch):
    r = Recorder()
    monkeypatch.setattr(jpegamd, "lib", r)
    return r


@pytest.fixture
def enc(jpegamd, rec):
    """A context whose handle is HANDLE; the handle is taken away again before the real library could be asked to destroy it."""
    e = jpegamd.Encoder(640, 480)
    assert [c[0] for c in rec.calls] == ["jpegamd_encoder_create"]
    (_, (ref, mw, mh)), = rec.calls
    assert ref._obj is e._h and (mw, mh) == (640, 480)
    del rec.calls[:]
    e._h = C.c_void_p(HANDLE)
    yield e
    e._h = C.c_void_p()


def pictures(jpegamd, kind, order: int = 3):
    """Two pictures of one geometry that differ in their pointers: Image (of channel order `order`), PlanarImage or YCbCrImage."""
    E = jpegamd.Encoder
    if kind is jpegamd.Image:
        return [E.image(0x1000 * (i + 1), 64, 32, 200, bottom_up=False, channel_order=order, quality=77) for i in range(2)]
    if kind is jpegamd.PlanarImage:
        return [E.planar_image((0x1000 * (i + 1), 0x1100 * (i + 1), 0x1200 * (i + 1)), 64, 32, 72, quality=77) for i in range(2)]
    return [E.ycbcr_image(0x1000 * (i + 1), 0x1100 * (i + 1), 0x1200 * (i + 1), 64, 32, 72, 40, jpegamd.CHROMA_PLANES, 77) for i in range(2)]


def batch_cases(jpegamd):
    """(method, its arguments between imgs and out_ptrs, keywords, entry, struct, the entry's integers between count and outs,
    ... between sizes and stream) for every *_batch_async method; encode_ycbcr_batch_async once per branch."""
    I, P, Y = jpegamd.Image, jpegamd.PlanarImage, jpegamd.YCbCrImage
    return [
        ("encode_batch_async", (), dict(with_container=True), "jpegamd_encode_batch_async", I, [], [1]),
        ("encode_batch_async", (), dict(with_container=False), "jpegamd_encode_batch_async", I, [], [0]),
        ("encode_color_batch_async", (SUB,), {}, "jpegamd_encode_color_batch_async", I, [SUB], []),
        ("encode_planar_batch_async", (SUB,), {}, "jpegamd_encode_planar_batch_async", P, [SUB], []),
        ("encode_color_interleaved_batch_async", (SUB,), {}, "jpegamd_encode_color_interleaved_batch_async", I, [SUB], []),
        ("encode_ycbcr_interleaved_batch_async", (SUB,), {}, "jpegamd_encode_ycbcr_interleaved_batch_async", Y, [SUB], []),
        ("encode_color_interleaved_restart_batch_async", (SUB, RESTART), {}, "jpegamd_encode_color_interleaved_restart_batch_async", I,
         [SUB, RESTART], []),
        ("encode_ycbcr_interleaved_restart_batch_async", (SUB, RESTART), {}, "jpegamd_encode_ycbcr_interleaved_restart_batch_async", Y,
         [SUB, RESTART], []),
        ("encode_ycbcr_interleaved_matrix_batch_async", (SUB, RANGE, FORMAT, MATRIX, RESTART), {},
         "jpegamd_encode_ycbcr_interleaved_matrix_batch_async", Y, [SUB, RANGE, FORMAT, MATRIX, RESTART], []),
        ("encode_color_interleaved_pixels_batch_async", (SUB, RESTART), {}, "jpegamd_encode_color_interleaved_pixels_batch_async", I,
         [SUB, RESTART], []),
        ("encode_planar_interleaved_batch_async", (SUB, RESTART), {}, "jpegamd_encode_planar_interleaved_batch_async", P, [SUB, RESTART], []),
        ("encode_gray_scan_batch_async", (RESTART,), {}, "jpegamd_encode_gray_scan_batch_async", I, [RESTART], []),
        # the fall-through of encode_ycbcr_batch_async: the newest entry that the call needs, the older ones otherwise
        ("encode_ycbcr_batch_async", (SUB,), dict(sample_range=RANGE, sample_format=FORMAT, matrix=MATRIX),
         "jpegamd_encode_ycbcr_matrix_batch_async", Y, [SUB, RANGE, FORMAT, MATRIX], []),
        ("encode_ycbcr_batch_async", (SUB,), dict(sample_range=0, sample_format=0, matrix=MATRIX),
         "jpegamd_encode_ycbcr_matrix_batch_async", Y, [SUB, 0, 0, MATRIX], []),
        ("encode_ycbcr_batch_async", (SUB,), dict(sample_range=RANGE, sample_format=FORMAT),
         "jpegamd_encode_ycbcr_samples_batch_async", Y, [SUB, RANGE, FORMAT], []),
        ("encode_ycbcr_batch_async", (SUB,), dict(sample_range=0, sample_format=FORMAT),
         "jpegamd_encode_ycbcr_samples_batch_async", Y, [SUB, 0, FORMAT], []),
        ("encode_ycbcr_batch_async", (SUB,), dict(sample_range=RANGE), "jpegamd_encode_ycbcr_range_batch_async", Y, [SUB, RANGE], []),
        ("encode_ycbcr_batch_async", (SUB,), {}, "jpegamd_encode_ycbcr_batch_async", Y, [SUB], []),
    ]


def check_batch_call(call, entry, struct, imgs, before, after):
    """One recorded call of a batch entry: (handle, images[], count, before..., outs[], cap, sizes[], after..., stream)."""
    name, args = call
    assert name == entry
    assert len(args) == 7 + len(before) + len(after), (name, args)
    arr, outs, sizes = args[1], args[3 + len(before)], args[5 + len(before)]
    assert isinstance(arr, C.Array) and arr._type_ is struct and len(arr) == len(imgs)
    assert plain(arr[0]) == plain(imgs[0]) and plain(arr[len(imgs) - 1]) == plain(imgs[-1]) and plain(arr[0]) != plain(arr[1])
    for ptrs in (outs, sizes):
        assert isinstance(ptrs, C.Array) and ptrs._type_ is C.c_void_p and len(ptrs) == len(imgs)
    got = [plain(a) for a in args]
    assert got[:1] + got[2:] == [HANDLE, len(imgs)] + before + [OUTS, CAP, SIZES] + after + [STREAM], name


def test_batch_methods_reach_their_entries(jpegamd, rec, enc):
    cases = batch_cases(jpegamd)
    assert {c[0] for c in cases} == {m for m in vars(jpegamd.Encoder) if m.endswith("_batch_async")}
    for method, args, kwargs, entry, struct, before, after in cases:
        imgs = pictures(jpegamd, struct)
        kwargs = dict(kwargs)
        if method == "encode_batch_async":
            got = enc.encode_batch_async(imgs, OUTS, CAP, SIZES, kwargs.pop("with_container"), STREAM)
        else:
            got = getattr(enc, method)(imgs, *args, OUTS, CAP, SIZES, STREAM, **kwargs)
        assert got is None
        (call,) = rec.calls
        check_batch_call(call, entry, struct, imgs, before, after)
        del rec.calls[:]


def single_calls(jpegamd, enc):
    """(what to call, entry, the arguments the entry must get, as plain values) for every other method of a context."""
    img = pictures(jpegamd, jpegamd.Image)[1]
    pimg = plain(img)
    return img, [
        (lambda: enc.set_pipeline(jpegamd.PIPELINE_STITCH), "jpegamd_encoder_set_pipeline", [HANDLE, 2]),
        (lambda: enc.set_huffman(jpegamd.HUFFMAN_OPTIMIZED), "jpegamd_encoder_set_huffman", [HANDLE, 1]),
        (lambda: enc.set_profiling(5), "jpegamd_encoder_set_profiling", [HANDLE, 5]),
        (lambda: enc.profile(3), "jpegamd_encoder_profile", [HANDLE, 3, plain(jpegamd.Stats())]),
        (lambda: enc.color_profile(4), "jpegamd_debug_color_profile", [HANDLE, 4, [0] * 11]),
        (lambda: enc.finish(), "jpegamd_encoder_finish", [HANDLE, plain(jpegamd.Stats())]),
        (lambda: enc.encode_async(img, OUT, CAP, SIZE, True, STREAM), "jpegamd_encode_async", [HANDLE, pimg, OUT, CAP, SIZE, 1, STREAM]),
        (lambda: enc.encode_async(img, OUT, CAP, SIZE, False, STREAM), "jpegamd_encode_async", [HANDLE, pimg, OUT, CAP, SIZE, 0, STREAM]),
        (lambda: enc.encode_color_async(img, SUB, OUT, CAP, SIZE, STREAM), "jpegamd_encode_color_async",
         [HANDLE, pimg, SUB, OUT, CAP, SIZE, STREAM]),
        (lambda: enc.encode_rows_async(img, ROW_BEGIN, ROW_END, STREAM), "jpegamd_encode_rows_async", [HANDLE, pimg, ROW_BEGIN, ROW_END, STREAM]),
        (lambda: enc.export_segments(img, ROW_BEGIN, ROW_END, DENSE, DENSE_CAP, META, TOTAL, STREAM), "jpegamd_export_segments",
         [HANDLE, pimg, ROW_BEGIN, ROW_END, DENSE, DENSE_CAP, META, TOTAL, STREAM]),
        (lambda: enc.import_segments(img, ROW_BEGIN, ROW_END, DENSE, META, STREAM), "jpegamd_import_segments",
         [HANDLE, pimg, ROW_BEGIN, ROW_END, DENSE, META, STREAM]),
        (lambda: enc.finalize_async(img, OUT, CAP, SIZE, True, STREAM), "jpegamd_finalize_async", [HANDLE, pimg, OUT, CAP, SIZE, 1, STREAM]),
        (lambda: enc.finalize_async(img, OUT, CAP, SIZE, False, STREAM), "jpegamd_finalize_async", [HANDLE, pimg, OUT, CAP, SIZE, 0, STREAM]),
        (lambda: enc.debug_stages(img, OUT, SIZE, META), "jpegamd_debug_stages", [HANDLE, pimg, OUT, SIZE, META]),
        (lambda: enc.debug_dct_exact(DENSE, META, ROW_END), "jpegamd_debug_dct_exact", [HANDLE, DENSE, META, ROW_END]),
    ]


def test_single_methods_reach_their_entries(jpegamd, rec, enc):
    img, calls = single_calls(jpegamd, enc)
    for run, entry, want in calls:
        got = run()
        (call,) = rec.calls
        name, args = call
        assert name == entry and [plain(a) for a in args] == want, name
        if want[1:2] == [plain(img)]:
            assert args[1]._obj is img, name                                    # the caller's struct itself, by reference
        if entry in ("jpegamd_encoder_profile", "jpegamd_encoder_finish"):
            assert isinstance(got, jpegamd.Stats) and args[-1]._obj is got, name
        elif entry == "jpegamd_debug_color_profile":
            assert got == [0] * 11 and args[-1]._type_ is C.c_uint64, name
        else:
            assert got is None, name
        del rec.calls[:]


def test_a_refusal_is_a_jpegamd_error_that_names_the_entry(jpegamd, rec, enc):
    rec.code = -3

    def refused(run, entry):
        with pytest.raises(jpegamd.JpegAmdError) as ei:
            run()
        assert ei.value.code == -3 and entry in str(ei.value) and "ERR_HIP" in str(ei.value), entry
        assert [c[0] for c in rec.calls] == [entry]
        del rec.calls[:]

    refused(lambda: jpegamd.Encoder(8, 8), "jpegamd_encoder_create")
    for method, args, kwargs, entry, struct, _, _ in batch_cases(jpegamd):
        imgs = pictures(jpegamd, struct)
        kwargs = dict(kwargs)
        if method == "encode_batch_async":
            refused(lambda: enc.encode_batch_async(imgs, OUTS, CAP, SIZES, kwargs["with_container"], STREAM), entry)
        else:
            refused(lambda: getattr(enc, method)(imgs, *args, OUTS, CAP, SIZES, STREAM, **kwargs), entry)
    for run, entry, _ in single_calls(jpegamd, enc)[1]:
        refused(run, entry)


def c_parameters(text: str, name: str):
    """The number of parameters of `name` as `text` (C, comments taken out) declares or defines it; None where it does not."""
    m = re.search(rf"\b{name}\s*\(([^()]*)\)\s*[;{{]", text)
    if m is None:
        return None
    params = m.group(1).strip()
    return 0 if params in ("", "void") else len(params.split(","))


def test_the_tables(jpegamd):
    assert len(jpegamd.EXPORTED) == len(set(jpegamd.EXPORTED))
    strip = lambda s: re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", s, flags=re.S))
    header = strip(jpegamd.HEADER_PATH.read_text())
    api = strip((PKG / "csrc" / "jpegamd_api.cpp").read_text())
    checked = []
    for name in jpegamd.EXPORTED:
        fn = getattr(jpegamd.lib, name)
        want = c_parameters(header, name)
        assert want is not None, name
        if fn.argtypes is not None:
            assert len(fn.argtypes) == want, name
            checked.append(name)
    assert len(checked) >= len(jpegamd.EXPORTED) - 1
    # the debug entries that the header leaves out: counted where they are defined
    for name in ("jpegamd_debug_tile_variant", "jpegamd_debug_matrix_coeffs", "jpegamd_debug_ycbcr_matrix_planes",
                 "jpegamd_debug_chroma_groups", "jpegamd_debug_ycbcr_sources"):
        assert name not in jpegamd.EXPORTED
        assert len(getattr(jpegamd.lib, name).argtypes) == c_parameters(api, name), name


# ---- the choice of entry for one call of the tensor functions, and the tables every prototype comes from ----

def test_every_declared_entry_has_its_prototype_at_import(jpegamd):
    assert all(getattr(jpegamd.lib, name).argtypes is not None for name in jpegamd.EXPORTED)      # jpegamd_encode_files too
    assert set(jpegamd._HIDDEN) == {"jpegamd_debug_tile_variant", "jpegamd_debug_matrix_coeffs", "jpegamd_debug_ycbcr_matrix_planes",
                                    "jpegamd_debug_chroma_groups", "jpegamd_debug_ycbcr_sources"}
    assert not set(jpegamd._BASE) & set(jpegamd._LATER) and not set(jpegamd.EXPORTED) & set(jpegamd._HIDDEN)
    assert len(jpegamd._LATER) + len(jpegamd._HIDDEN) == 28       # what a JPEGAMD_LIB variant build may lack: no more than before


def test_pixel_routes(jpegamd, rec, enc):
    """_queue_pixels: every row of encode_tensor_batch's routes, with and without a Huffman mode."""
    I, P = jpegamd.Image, jpegamd.PlanarImage
    RGB, GRAY, RGBA, BGRA = jpegamd.ORDER_RGB, jpegamd.ORDER_GRAY, jpegamd.ORDER_RGBA, jpegamd.ORDER_BGRA
    one_scan = dict(interleaved=True)
    rows = [   # (struct, channel order, flags, entry, integers between count and outs, ... between sizes and stream)
        (P, None, {}, "jpegamd_encode_planar_batch_async", [SUB], []),
        (I, GRAY, {}, "jpegamd_encode_batch_async", [], [1]),
    ]
    for order in (RGB, RGBA, BGRA):
        rows.append((I, order, {}, "jpegamd_encode_color_batch_async", [SUB], []))
    for huffman in (0, 1):                                              # a Huffman mode takes the same rows ...
        for ri in (RESTART, 0):
            flags = dict(one_scan, any_layout=True, restart=ri, huffman=huffman)
            rows.append((P, None, flags, "jpegamd_encode_planar_interleaved_batch_async", [SUB, ri], []))
            for order in (RGB, RGBA, BGRA):
                rows.append((I, order, flags, "jpegamd_encode_color_interleaved_pixels_batch_async", [SUB, ri], []))
    rows += [
        (I, RGB, dict(one_scan, restart=RESTART), "jpegamd_encode_color_interleaved_restart_batch_async", [SUB, RESTART], []),
        (I, RGB, dict(one_scan, restart=0), "jpegamd_encode_color_interleaved_batch_async", [SUB], []),
        # ... but without any_layout it goes to the restart entry, an interval of 0 included (no public function comes here)
        (I, RGB, dict(one_scan, restart=RESTART, huffman=1), "jpegamd_encode_color_interleaved_restart_batch_async", [SUB, RESTART], []),
        (I, RGB, dict(one_scan, restart=0, huffman=1), "jpegamd_encode_color_interleaved_restart_batch_async", [SUB, 0], []),
    ]
    for struct, order, flags, entry, before, after in rows:
        imgs = pictures(jpegamd, struct, order)
        assert jpegamd._queue_pixels(enc, imgs, SUB, OUTS, CAP, SIZES, STREAM, **flags) is None
        (call,) = rec.calls
        check_batch_call(call, entry, struct, imgs, before, after)
        del rec.calls[:]


def test_ycbcr_routes(jpegamd, rec, enc):
    """_queue_ycbcr: the first match of (any_kind, restart, interleaved) wins; behind them the four three-scan entries."""
    Y = jpegamd.YCbCrImage
    kind = (RANGE, FORMAT, MATRIX)
    rows = [   # (range, format, matrix), flags, entry, integers between count and outs
        (kind, dict(any_kind=True, interleaved=True, restart=RESTART), "jpegamd_encode_ycbcr_interleaved_matrix_batch_async",
         [SUB, RANGE, FORMAT, MATRIX, RESTART]),
        (kind, dict(any_kind=True, interleaved=True), "jpegamd_encode_ycbcr_interleaved_matrix_batch_async", [SUB, RANGE, FORMAT, MATRIX, 0]),
        ((0, 0, 0), dict(any_kind=True, interleaved=True), "jpegamd_encode_ycbcr_interleaved_matrix_batch_async", [SUB, 0, 0, 0, 0]),
        ((0, 0, 0), dict(interleaved=True, restart=RESTART), "jpegamd_encode_ycbcr_interleaved_restart_batch_async", [SUB, RESTART]),
        ((0, 0, 0), dict(interleaved=True), "jpegamd_encode_ycbcr_interleaved_batch_async", [SUB]),
        (kind, {}, "jpegamd_encode_ycbcr_matrix_batch_async", [SUB, RANGE, FORMAT, MATRIX]),
        ((RANGE, FORMAT, 0), {}, "jpegamd_encode_ycbcr_samples_batch_async", [SUB, RANGE, FORMAT]),
        ((RANGE, 0, 0), {}, "jpegamd_encode_ycbcr_range_batch_async", [SUB, RANGE]),
        ((0, 0, 0), {}, "jpegamd_encode_ycbcr_batch_async", [SUB]),
    ]
    for (rng, fmt, mat), flags, entry, before in rows:
        imgs = pictures(jpegamd, Y)
        assert jpegamd._queue_ycbcr(enc, imgs, SUB, OUTS, CAP, SIZES, STREAM, rng, fmt, mat, **flags) is None
        (call,) = rec.calls
        check_batch_call(call, entry, Y, imgs, before, [])
        del rec.calls[:]
    with pytest.raises(ValueError, match="go through jpegamd.mjpeg"):   # a Huffman mode without any_kind: refused before any work
        jpegamd._encode_ycbcr_images(None, 2, 32, 64, SUB, None, huffman=1)
    assert not rec.calls
