"""Metadata in front of the tables on the GPU (jpegamd_encoder_set_metadata, k_metadata_place).  The oracle throughout:
the same call on the same context WITHOUT metadata -- those files are pinned against the models by the suites of each entry -- spliced
with the head and the blob by tests/metadata_model.py.  Required: byte equality with that splice, every size = size + M, the guard bytes
in front of and behind every output intact, and Stats equal field by field except jfif_bytes.  Every test needs an MI355X."""
from __future__ import annotations

import io

import numpy as np
import pytest

import color_model as cm
import gpu_support as gs
import metadata_model as mm
import mjpeg_support as ms
import progressive_script_fixtures as fx
import scan_model as sm
from gpu_support import CBCR, PLANES, S420, S422, S444, YUYV, dev  # noqa: F401

torch = gs.torch
pytestmark = pytest.mark.gpu
ERR_ARG, ERR_CAPACITY = -1, -8
W, H = 72, 40                                                   # 9 x 5 blocks: a partial MCU at 4:2:0
FRONT = 64                                                      # guard bytes in front of every output (a multiple of 16)
OFFSETS = (0, 1, 2, 3, 8)
COUNTERS = ("entropy_bits", "stuffed_bytes", "exact_fallbacks")
ROW = ms.row_interval(W, S420)
ALL = dict(density=(2, 118, 118), exif=bytes.fromhex("49492a0008000000010012010300010000000600000000000000"), icc_profile=mm.icc_like(3144),
           comment=b"seen \xff\xd9 through", segments=((0xE1, b"http://ns.adobe.com/xap/1.0/\0<x/>"),))


def spliced(keywords):
    """(head, blob) by the model for the keywords of set_metadata."""
    kw = dict(keywords)
    density = kw.pop("density", None)
    if "dpi" in kw:
        density = (1, kw["dpi"], kw.pop("dpi"))
    comment = kw.pop("comment", None)
    return mm.head(density), mm.blob(exif=kw.pop("exif", None), segments=kw.pop("segments", ()), icc=kw.pop("icc_profile", None),
                                     comment=comment.encode() if isinstance(comment, str) else comment)


@pytest.fixture(scope="module")
def enc(jpegamd, dev):
    e = jpegamd.Encoder(2056, gs.rows_for(3, H))
    yield e
    e.set_metadata(None)
    e.close()


@pytest.fixture(scope="module")
def pics():
    rgb = {"photo": cm.synth_rgb(W, H, 11, 0), "noise": cm.synth_rgb(W, H, 12, 1), "photo2": cm.synth_rgb(W, H, 13, 0), "small": cm.synth_rgb(9, 9, 14, 1)}
    return rgb, {k: np.ascontiguousarray(sm.luma_plane(v)) for k, v in rgb.items()}


# ---- guarded outputs at chosen offsets ---------------------------------------------------------------------------------------------------
class Guarded(gs.Outputs):
    """gpu_support.Outputs with FRONT + offsets[i] guard bytes in front of picture i's buffer (a different 16-byte residue per picture)."""

    def __init__(self, dev, n, cap, offsets=None):
        self.cap, self.offs = cap, [FRONT + o for o in (offsets or [0] * n)]
        self.outs = [torch.full((off + cap + gs.GUARD,), gs.FILL, dtype=torch.uint8, device=dev) for off in self.offs]
        self.sizes = torch.full((n,), -1, dtype=torch.int64, device=dev)
        self.out_ptrs = [o.data_ptr() + off for o, off in zip(self.outs, self.offs)]
        self.size_ptrs = [self.sizes.data_ptr() + 8 * i for i in range(n)]
        assert all(o.data_ptr() % 16 == 0 for o in self.outs)

    def results(self):
        res = []
        for o, off, n in zip(self.outs, self.offs, self.sizes.cpu().tolist()):
            host = o.cpu().numpy()
            intact = bool(np.all(host[off + self.cap:] == gs.FILL) and np.all(host[:off] == gs.FILL))
            res.append((bytes(host[off:off + (min(n, self.cap) if n >= 0 else self.cap)]), intact))
        return res


class Call:
    """One entry with its pictures on the device: queue(out_ptrs, cap, size_ptrs, stream) queues it; `bound` is its jpegamd_max_jfif_bytes*."""

    def __init__(self, n, bound, queue, keep=None, huffman=None, pipeline=None):
        self.n, self.bound, self.queue, self.keep, self.huffman, self.pipeline = n, bound, queue, keep, huffman, pipeline

    def start(self, jpegamd, enc, dev, cap=None, offsets=None):
        out = Guarded(dev, self.n, self.bound if cap is None else cap, offsets)
        enc.set_huffman(jpegamd.HUFFMAN_STANDARD if self.huffman is None else self.huffman)
        enc.set_pipeline(jpegamd.PIPELINE_AUTO if self.pipeline is None else self.pipeline)
        try:
            self.queue(out.out_ptrs, out.cap, out.size_ptrs, gs.stream())
        finally:
            enc.set_huffman(jpegamd.HUFFMAN_STANDARD)
            enc.set_pipeline(jpegamd.PIPELINE_AUTO)
        return out

    def run(self, jpegamd, enc, dev, cap=None, offsets=None):
        return gs.finish_files(enc, self.start(jpegamd, enc, dev, cap, offsets))


def check(jpegamd, enc, dev, call, keywords, offsets=None, plain=None):
    """The call without and with the metadata of `keywords` -> the plain (files, Stats), for the next check of the same call."""
    enc.set_metadata(None)
    assert enc.metadata_bytes() == 0
    plain = plain or call.run(jpegamd, enc, dev)
    head, blob = spliced(keywords)
    enc.set_metadata(**keywords)
    try:
        assert enc.metadata_bytes() == len(blob)
        files, st = call.run(jpegamd, enc, dev, call.bound + len(blob), offsets)
    finally:
        enc.set_metadata(None)
    for k, (got, base) in enumerate(zip(files, plain[0])):
        assert len(got) == len(base) + len(blob), (k, len(got), len(base), len(blob))
        assert got == mm.splice(base, head, blob), k
    for name in COUNTERS:
        assert getattr(st, name) == getattr(plain[1], name), name
    assert st.jfif_bytes == plain[1].jfif_bytes + len(blob)
    return plain


# ---- the entry families ------------------------------------------------------------------------------------------------------------------
def rgb_images(j, rgbs, dev):
    h, w, _ = rgbs[0].shape
    keep = [gs.upload(gs.stored_rows(r, False), dev, 3 * w) for r in rgbs]
    return keep, [j.Encoder.image(ptr, w, h, 3 * w, False, j.ORDER_RGB, 0) for _, ptr in keep]


def gray_images(j, planes, dev):
    h, w = planes[0].shape
    keep = [gs.upload(p, dev, w) for p in planes]
    return keep, [j.Encoder.image(ptr, w, h, w, False, j.ORDER_GRAY, 0) for _, ptr in keep]


def gray_fused(j, e, d, planes, pipeline=None):
    h, w = planes[0].shape
    keep, imgs = gray_images(j, planes, d)
    if len(planes) == 1:
        return Call(1, j.max_jfif_bytes(w, h), lambda o, cap, s, st: e.encode_async(imgs[0], o[0], cap, s[0], True, st), keep, pipeline=pipeline)
    return Call(len(planes), j.max_jfif_bytes(w, h), lambda o, cap, s, st: e.encode_batch_async(imgs, o, cap, s, True, st), keep, pipeline=pipeline)


def color_single(j, e, d, rgb, sub):
    h, w, _ = rgb.shape
    keep, imgs = rgb_images(j, [rgb], d)
    return Call(1, j.max_jfif_bytes_color(w, h, sub), lambda o, cap, s, st: e.encode_color_async(imgs[0], sub, o[0], cap, s[0], st), keep)


def color_batch(j, e, d, rgbs, sub):
    h, w, _ = rgbs[0].shape
    keep, imgs = rgb_images(j, rgbs, d)
    return Call(len(rgbs), j.max_jfif_bytes_color(w, h, sub), lambda o, cap, s, st: e.encode_color_batch_async(imgs, sub, o, cap, s, st), keep)


def planar(j, e, d, rgb):
    keep = [gs.upload(np.ascontiguousarray(rgb[:, :, k]), d, W) for k in range(3)]
    imgs = [j.Encoder.planar_image(tuple(p for _, p in keep), W, H, W, False, 0)]
    return Call(1, j.max_jfif_bytes_color(W, H, S420), lambda o, cap, s, st: e.encode_planar_batch_async(imgs, S420, o, cap, s, st), keep)


class Recorder:
    """An Encoder as gpu_support.YccBatch sees it: the pictures it built are kept, nothing is queued."""

    def encode_ycbcr_batch_async(self, imgs, subsampling, out_ptrs, out_cap, size_ptrs, stream=0, sample_range=0, sample_format=0):
        self.imgs = imgs


def ycc(j, e, d, sub, layout, kind=ms.FULL8, one_scan=False):
    """Stored planes of a mjpeg_support.Kind through the three-scan YCbCr entry, or the one-scan entry of every kind."""
    rng, fmt, matrix = kind.args(j)
    rec = Recorder()
    keep = gs.YccBatch(j, rec, [ms.stored_planes(kind, W, H, sub, 21)], d, sub, layout, sample_range=rng, sample_format=fmt)
    if one_scan:
        return Call(1, j.max_jfif_bytes_interleaved(W, H, sub),
                    lambda o, cap, s, st: e.encode_ycbcr_interleaved_matrix_batch_async(rec.imgs, sub, rng, fmt, matrix, 0, o, cap, s, st), keep)
    return Call(1, j.max_jfif_bytes_color(W, H, sub), lambda o, cap, s, st: e.encode_ycbcr_batch_async(rec.imgs, sub, o, cap, s, st, rng, fmt, matrix), keep)


def one_scan(j, e, d, rgbs, sub, ri=0, optimized=False):
    h, w, _ = rgbs[0].shape
    keep, imgs = rgb_images(j, rgbs, d)
    return Call(len(rgbs), j.max_jfif_bytes_interleaved_restart(w, h, sub, ri),
                lambda o, cap, s, st: e.encode_color_interleaved_restart_batch_async(imgs, sub, ri, o, cap, s, st), keep,
                huffman=j.HUFFMAN_OPTIMIZED if optimized else None)


def gray_scan(j, e, d, planes, ri, optimized):
    h, w = planes[0].shape
    keep, imgs = gray_images(j, planes, d)
    return Call(len(planes), j.max_jfif_bytes_gray_scan(w, h, ri), lambda o, cap, s, st: e.encode_gray_scan_batch_async(imgs, ri, o, cap, s, st), keep,
                huffman=j.HUFFMAN_OPTIMIZED if optimized else None)


PROGRESSIVE = {"spectral": ("encode_color_progressive_batch_async", "max_jfif_bytes_progressive"),
               "optimized": ("encode_color_progressive_optimized_batch_async", "max_jfif_bytes_progressive_optimized"),
               "successive": ("encode_color_progressive_successive_batch_async", "max_jfif_bytes_progressive_successive")}


def progressive(j, e, d, rgbs, sub, kind):
    h, w, _ = rgbs[0].shape
    keep, imgs = rgb_images(j, rgbs, d)
    method, bound = PROGRESSIVE[kind]
    return Call(len(rgbs), getattr(j, bound)(w, h, sub), lambda o, cap, s, st: getattr(e, method)(imgs, sub, o, cap, s, st), keep)


def scripted(j, e, d, rgbs, sub, script):
    h, w, _ = rgbs[0].shape
    keep, imgs = rgb_images(j, rgbs, d)
    return Call(len(rgbs), j.max_jfif_bytes_progressive_script(w, h, sub, script),
                lambda o, cap, s, st: e.encode_color_progressive_script_batch_async(imgs, sub, script, o, cap, s, st), keep)


def scripted_gray(j, e, d, planes, script):
    h, w = planes[0].shape
    keep, imgs = gray_images(j, planes, d)
    return Call(len(planes), j.max_jfif_bytes_progressive_script(w, h, 0, script),
                lambda o, cap, s, st: e.encode_gray_progressive_script_batch_async(imgs, script, o, cap, s, st), keep)


FAMILIES = {
    "gray_single": lambda j, e, d, rgb, gray: gray_fused(j, e, d, [gray["photo"]]),
    "gray_small": lambda j, e, d, rgb, gray: gray_fused(j, e, d, [gray["small"]]),
    "gray_batch3": lambda j, e, d, rgb, gray: gray_fused(j, e, d, [gray["photo"], gray["noise"], gray["photo2"]]),
    "color_420": lambda j, e, d, rgb, gray: color_single(j, e, d, rgb["photo"], S420),
    "color_422": lambda j, e, d, rgb, gray: color_single(j, e, d, rgb["photo"], S422),
    "color_444": lambda j, e, d, rgb, gray: color_single(j, e, d, rgb["photo"], S444),
    "color_small": lambda j, e, d, rgb, gray: color_single(j, e, d, rgb["small"], S420),
    "color_batch3": lambda j, e, d, rgb, gray: color_batch(j, e, d, [rgb["photo"], rgb["noise"], rgb["photo2"]], S420),
    "planar": lambda j, e, d, rgb, gray: planar(j, e, d, rgb["photo"]),
    "nv12": lambda j, e, d, rgb, gray: ycc(j, e, d, S420, CBCR),
    "yuy2": lambda j, e, d, rgb, gray: ycc(j, e, d, S422, YUYV),
    "limited_range": lambda j, e, d, rgb, gray: ycc(j, e, d, S420, PLANES, ms.LIMITED8),
    "bt709": lambda j, e, d, rgb, gray: ycc(j, e, d, S420, PLANES, ms.FULL8_709),
    "msb10": lambda j, e, d, rgb, gray: ycc(j, e, d, S420, CBCR, ms.MSB10),
    "one_scan": lambda j, e, d, rgb, gray: one_scan(j, e, d, [rgb["photo"]], S420),
    "one_scan_small": lambda j, e, d, rgb, gray: one_scan(j, e, d, [rgb["small"]], S420),
    "one_scan_row": lambda j, e, d, rgb, gray: one_scan(j, e, d, [rgb["photo"]], S420, ROW),
    "one_scan_optimized": lambda j, e, d, rgb, gray: one_scan(j, e, d, [rgb["photo"]], S420, optimized=True),
    "one_scan_ycbcr_709": lambda j, e, d, rgb, gray: ycc(j, e, d, S420, PLANES, ms.LIMITED8_709, one_scan=True),
    "gray_scan_interval": lambda j, e, d, rgb, gray: gray_scan(j, e, d, [gray["photo"]], 9, False),
    "gray_scan_optimized": lambda j, e, d, rgb, gray: gray_scan(j, e, d, [gray["photo"]], 0, True),
    "progressive": lambda j, e, d, rgb, gray: progressive(j, e, d, [rgb["photo"]], S420, "spectral"),
    "progressive_optimized": lambda j, e, d, rgb, gray: progressive(j, e, d, [rgb["photo"]], S420, "optimized"),
    "progressive_successive": lambda j, e, d, rgb, gray: progressive(j, e, d, [rgb["photo"]], S420, "successive"),
    "script_colour": lambda j, e, d, rgb, gray: scripted(j, e, d, [rgb["photo"]], S420, fx.SPLIT),
    "script_gray": lambda j, e, d, rgb, gray: scripted_gray(j, e, d, [gray["photo"]], None),
}


# ---- 1. one case per entry family --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_every_entry_writes_the_splice(jpegamd, dev, enc, pics, family):
    call = FAMILIES[family](jpegamd, enc, dev, *pics)
    plain = check(jpegamd, enc, dev, call, ALL, offsets=[OFFSETS[(3 + i) % 5] for i in range(call.n)])
    check(jpegamd, enc, dev, call, dict(dpi=300), plain=plain)       # a density alone: M = 0, the 20 leading bytes differ


# ---- 2. alignment: every residue of M and of the output pointer, for each kind of writer ------------------------------------------------------
WRITERS = {
    "k_finalize": lambda j, e, d, rgb, gray: gray_fused(j, e, d, [gray["photo"], gray["noise"], gray["photo2"]], j.PIPELINE_PAIR),
    "k_stitch": lambda j, e, d, rgb, gray: gray_fused(j, e, d, [gray["photo"], gray["noise"], gray["photo2"]], j.PIPELINE_STITCH),
    "restart_writer": lambda j, e, d, rgb, gray: one_scan(j, e, d, [rgb["photo"], rgb["noise"], rgb["photo2"]], S420, ROW),
    "k_scans_concat": lambda j, e, d, rgb, gray: progressive(j, e, d, [rgb["photo"], rgb["noise"], rgb["photo2"]], S420, "spectral"),
}


@pytest.mark.parametrize("writer", sorted(WRITERS))
def test_every_residue_of_m_and_of_the_pointer(jpegamd, dev, enc, pics, writer):
    """Comments of 0 .. 15 bytes: M = 4 .. 19 takes every residue mod 16, all of them with M < 20 (the shifted head and the placed one
    overlap); three pictures per call at three different pointer residues out of 0, 1, 2, 3 and 8, rotating with the length."""
    call = WRITERS[writer](jpegamd, enc, dev, *pics)
    plain = None
    for length in range(16):
        offsets = [OFFSETS[(length + i) % 5] for i in range(3)]
        plain = check(jpegamd, enc, dev, call, dict(comment=bytes(range(0x41, 0x41 + length))), offsets, plain)


# ---- 3. size -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("icc_bytes", [65519, 65520])
def test_profiles_at_the_chunk_boundary(jpegamd, dev, enc, pics, icc_bytes):
    check(jpegamd, enc, dev, color_single(jpegamd, enc, dev, pics[0]["photo"], S420), dict(icc_profile=mm.icc_like(icc_bytes)), [1])


def test_a_large_profile_in_a_batch_of_three(jpegamd, dev, enc, pics):
    rgb, _ = pics
    call = one_scan(jpegamd, enc, dev, [rgb["photo"], rgb["noise"], rgb["photo2"]], S420)
    check(jpegamd, enc, dev, call, dict(icc_profile=mm.icc_like(200000), comment="three"), [3, 8, 0])


def test_a_blob_full_of_ff(jpegamd, dev, enc, pics):
    ff = lambda n: b"\xff" * n
    keywords = dict(exif=ff(1000), icc_profile=ff(70000), comment=ff(65533), segments=((0xEF, ff(300)),))
    check(jpegamd, enc, dev, gray_fused(jpegamd, enc, dev, [pics[1]["photo"]]), keywords, [2])


def test_pil_reads_a_device_written_file(jpegamd, dev, enc, pics):
    from PIL import Image
    call = color_single(jpegamd, enc, dev, pics[0]["photo"], S420)
    profile, comment = mm.icc_like(76800), b"seen \xff\xd9 through"
    enc.set_metadata(None)
    (plain,), _ = call.run(jpegamd, enc, dev)
    enc.set_metadata(icc_profile=profile, exif=jpegamd.exif_orientation(6), comment=comment, dpi=(300, 150))
    try:
        (file,), _ = call.run(jpegamd, enc, dev, call.bound + enc.metadata_bytes())
    finally:
        enc.set_metadata(None)
    a, b = Image.open(io.BytesIO(plain)), Image.open(io.BytesIO(file))
    assert b.info["icc_profile"] == profile and b.getexif()[0x0112] == 6 and b.info["comment"] == comment
    assert b.info["jfif_unit"] == 1 and b.info["jfif_density"] == (300, 150) and tuple(b.info["dpi"]) == (300, 150)
    assert a.size == b.size == (W, H) and a.mode == b.mode == "RGB" and a.tobytes() == b.tobytes()


# ---- 4. capacity ---------------------------------------------------------------------------------------------------------------------------
def size_words(jpegamd, enc, dev, call, cap, want_rc):
    """The call at this capacity, finished -> its size words; the status, the guards and Stats.jfif_bytes are checked."""
    out = call.start(jpegamd, enc, dev, cap, [1] * call.n)
    if want_rc:
        with pytest.raises(jpegamd.JpegAmdError) as err:
            enc.finish()
        assert err.value.code == want_rc
    else:
        enc.finish()
    assert all(ok for _, ok in out.results()), "guard bytes around an output were overwritten"
    return out.sizes.cpu().tolist()


@pytest.mark.parametrize("family", ["gray_single", "one_scan"])
def test_capacity_counts_the_metadata(jpegamd, dev, enc, pics, family):
    """With M bytes set an entry behaves towards out_capacity as without metadata towards out_capacity - M: a size word it leaves
    non-zero gets + M, a zero stays zero, and -8 is raised exactly when it would be."""
    call = FAMILIES[family](jpegamd, enc, dev, *pics)
    keywords = dict(icc_profile=mm.icc_like(777), comment="cap")
    head, blob = spliced(keywords)
    m = len(blob)
    enc.set_metadata(None)
    (plain,), _ = call.run(jpegamd, enc, dev)
    size = len(plain)
    short = size_words(jpegamd, enc, dev, call, size - 1, ERR_CAPACITY)       # what today's entry leaves, one byte short ...
    ten = size_words(jpegamd, enc, dev, call, 10, ERR_CAPACITY)              # ... with room for half the leading bytes ...
    none = size_words(jpegamd, enc, dev, call, 0, ERR_CAPACITY)              # ... and with no room at all
    plus = lambda words: [w + m if w else 0 for w in words]
    enc.set_metadata(**keywords)
    try:
        exact = call.run(jpegamd, enc, dev, size + m, [1])[0]
        assert exact == [mm.splice(plain, head, blob)]
        assert size_words(jpegamd, enc, dev, call, size + m - 1, ERR_CAPACITY) == plus(short)
        assert size_words(jpegamd, enc, dev, call, m + 10, ERR_CAPACITY) == plus(ten)    # (no room for the 20 leading bytes: nothing placed)
        assert size_words(jpegamd, enc, dev, call, m, ERR_CAPACITY) == plus(none)
        assert size_words(jpegamd, enc, dev, call, m - 1, ERR_CAPACITY) == plus(none)
        assert size_words(jpegamd, enc, dev, call, 0, ERR_CAPACITY) == plus(none)
        assert call.run(jpegamd, enc, dev, size + m, [2])[0] == exact          # and the context goes on
    finally:
        enc.set_metadata(None)


# ---- 5. stickiness, clearing, a switch behind queued work -----------------------------------------------------------------------------------
def test_sticky_until_cleared(jpegamd, dev, enc, pics):
    rgb, gray = pics
    big, small = gray_fused(jpegamd, enc, dev, [gray["photo"]]), color_single(jpegamd, enc, dev, rgb["small"], S444)
    enc.set_metadata(None)
    (plain_big,), _ = big.run(jpegamd, enc, dev)
    (plain_small,), _ = small.run(jpegamd, enc, dev)
    head, blob = spliced(ALL)
    enc.set_metadata(**ALL)
    try:
        assert big.run(jpegamd, enc, dev, big.bound + len(blob))[0] == [mm.splice(plain_big, head, blob)]
        assert small.run(jpegamd, enc, dev, small.bound + len(blob))[0] == [mm.splice(plain_small, head, blob)]
        with pytest.raises(ValueError):
            enc.set_metadata(density=(3, 1, 1))                               # refused: the context keeps what it had
        assert enc.metadata_bytes() == len(blob)
        assert big.run(jpegamd, enc, dev, big.bound + len(blob))[0] == [mm.splice(plain_big, head, blob)]
    finally:
        enc.set_metadata(None)
    assert enc.metadata_bytes() == 0
    assert big.run(jpegamd, enc, dev)[0] == [plain_big]
    enc.set_metadata()                                                        # no keyword: nothing set
    assert enc.metadata_bytes() == 0 and big.run(jpegamd, enc, dev)[0] == [plain_big]


def test_a_switch_with_work_queued(jpegamd, dev, enc, pics):
    """Two blobs of different length, the second set while the first call is still queued: the upload of the second waits for the first
    call, whose kernel reads the context's copy."""
    call = gray_fused(jpegamd, enc, dev, [pics[1]["photo"], pics[1]["noise"]])
    enc.set_metadata(None)
    plain, _ = call.run(jpegamd, enc, dev)
    first, second = dict(icc_profile=mm.icc_like(5000, 3)), dict(icc_profile=mm.icc_like(90000, 4), comment="longer")
    try:
        enc.set_metadata(**first)
        a = call.start(jpegamd, enc, dev, call.bound + enc.metadata_bytes(), [1, 2])
        enc.set_metadata(**second)
        b = call.start(jpegamd, enc, dev, call.bound + enc.metadata_bytes(), [3, 8])
        enc.set_metadata(**first)
        c = call.start(jpegamd, enc, dev, call.bound + enc.metadata_bytes(), [0, 1])
        enc.finish()
    finally:
        enc.set_metadata(None)
    for out, keywords in ((a, first), (b, second), (c, first)):
        assert gs.intact_files(out) == [mm.splice(f, *spliced(keywords)) for f in plain]


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_entries_that_write_no_metadata_refuse(jpegamd, dev, enc, pics):
    plane = pics[1]["photo"]
    keep, (img,) = gray_images(jpegamd, [plane], dev)
    rows = (H + 7) // 8
    words = rows * ((256 * 1721 + 31) // 32 + 1)
    dense = torch.empty(words, dtype=torch.int32, device=dev)
    meta = torch.zeros(rows * jpegamd.SEG_META_WORDS, dtype=torch.int32, device=dev)
    total = torch.zeros(1, dtype=torch.int32, device=dev)
    stages = torch.zeros(rows * 9 * 64, dtype=torch.int8, device=dev)
    out = Guarded(dev, 1, jpegamd.max_jfif_bytes(W, H))
    calls = [lambda: enc.encode_rows_async(img, 0, rows, gs.stream()),
             lambda: enc.export_segments(img, 0, rows, dense.data_ptr(), words, meta.data_ptr(), total.data_ptr(), gs.stream()),
             lambda: enc.import_segments(img, 0, rows, dense.data_ptr(), meta.data_ptr(), gs.stream()),
             lambda: enc.finalize_async(img, out.out_ptrs[0], out.cap, out.size_ptrs[0], True, gs.stream()),
             lambda: enc.debug_stages(img, stages.data_ptr(), 0, 0),
             lambda: enc.encode_async(img, out.out_ptrs[0], out.cap, out.size_ptrs[0], False, gs.stream())]      # a bare scan is no file
    enc.set_metadata(None)
    (plain,), _ = gray_fused(jpegamd, enc, dev, [plane]).run(jpegamd, enc, dev)
    enc.set_metadata(comment="refused")
    try:
        for k, call in enumerate(calls):
            with pytest.raises(jpegamd.JpegAmdError) as err:
                call()
            assert err.value.code == ERR_ARG, k
    finally:
        enc.set_metadata(None)
    assert gs.intact_files(out) == [b"\xa5" * out.cap]                       # nothing was written, no size either
    for call in calls[:4]:
        call()
    files, _ = gs.finish_files(enc, out)
    assert files == [plain]
    calls[4]()


# ---- 7. the Python surface -----------------------------------------------------------------------------------------------------------------
def test_the_metadata_block(jpegamd, dev, pics):
    from jpegamd import mjpeg, progressive_script
    rgb, gray = pics
    t = torch.from_numpy(np.stack([rgb["photo"], rgb["noise"]])).to(dev)
    planes = [gs.smooth_planes(W, H, S420, 31 + k) for k in range(2)]
    y, cb, cr = (torch.from_numpy(np.ascontiguousarray(np.stack([p[k] for p in planes]))).to(dev) for k in range(3))
    g = torch.from_numpy(gray["photo"]).to(dev)
    calls = [lambda: jpegamd.encode_tensor_batch(t), lambda: mjpeg.encode_ycbcr_batch(y, cb, cr), lambda: [progressive_script.encode_gray(g)],
             lambda: [jpegamd.encode_tensor(t[0])], lambda: [jpegamd.encode_tensor(g)]]
    plain = [call() for call in calls]
    keywords = dict(icc_profile=mm.icc_like(3144), exif=jpegamd.exif_orientation(3), comment="block", dpi=150)
    head, blob = spliced(keywords)
    assert jpegamd.build_metadata(**keywords) == (head, blob)
    with jpegamd.metadata(**keywords):
        inside = [call() for call in calls]
        with jpegamd.metadata(comment="inner"):
            inner = calls[0]()
        again = calls[0]()
    for got, base in zip(inside, plain):
        assert got == [mm.splice(f, head, blob) for f in base]
    assert inner == [mm.splice(f, *spliced(dict(comment="inner"))) for f in plain[0]] and again == inside[0]
    assert [call() for call in calls] == plain                               # outside the block the cached context writes plain files
