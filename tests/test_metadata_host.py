"""Metadata in front of the tables on the CPU: jpegamd_build_metadata against the model of tests/metadata_model.py byte
for byte, its refusals one by one, the spliced golden files read back through PIL (which shares no code with the library), and the
Python helpers.  No compute calls are made here."""
from __future__ import annotations

import ctypes as C
import io
import threading

import pytest

import metadata_model as mm
from conftest import GOLDEN

NEW = ("jpegamd_build_metadata", "jpegamd_encoder_set_metadata", "jpegamd_encoder_metadata_bytes")
FF = lambda n: b"\xff" * n
ORIENT6 = bytes.fromhex("49492a00080000000100120103000100000006000000" "00000000")
SIXTEEN = tuple((0xE1 + i if i < 15 else 0xFE, bytes([i]) * (i * 37)) for i in range(16))

# name -> (keywords of jpegamd.build_metadata, the model's (blob keywords, density))
CASES = {
    "nothing": ({}, ({}, None)),
    "dpi": (dict(dpi=(300, 72)), ({}, (1, 300, 72))),
    "dpi_number": (dict(dpi=600), ({}, (1, 600, 600))),
    "density_cm": (dict(density=(2, 118, 118)), ({}, (2, 118, 118))),
    "density_aspect_extremes": (dict(density=(0, 1, 65535)), ({}, (0, 1, 65535))),
    "exif": (dict(exif=ORIENT6), (dict(exif=ORIENT6), None)),
    "exif_with_identifier": (dict(exif=b"Exif\0\0" + ORIENT6), (dict(exif=ORIENT6), None)),
    "exif_largest": (dict(exif=FF(65527)), (dict(exif=FF(65527)), None)),
    "comment": (dict(comment="café ✓"), (dict(comment="café ✓".encode()), None)),
    "comment_empty": (dict(comment=b""), (dict(comment=b""), None)),
    "comment_largest_all_ff": (dict(comment=FF(65533)), (dict(comment=FF(65533)), None)),
    "comment_with_eoi": (dict(comment=b"a\xff\xd9b"), (dict(comment=b"a\xff\xd9b"), None)),
    "icc_1": (dict(icc_profile=b"\x07"), (dict(icc=b"\x07"), None)),
    "icc_65519": (dict(icc_profile=mm.icc_like(65519)), (dict(icc=mm.icc_like(65519)), None)),
    "icc_65520": (dict(icc_profile=mm.icc_like(65520)), (dict(icc=mm.icc_like(65520)), None)),
    "icc_131038_all_ff": (dict(icc_profile=FF(131038)), (dict(icc=FF(131038)), None)),
    "sixteen_segments": (dict(segments=SIXTEEN), (dict(segments=SIXTEEN), None)),
    "segment_largest_and_empty": (dict(segments=((0xE1, FF(65533)), (0xFE, b""))), (dict(segments=((0xE1, FF(65533)), (0xFE, b""))), None)),
    "all": (dict(density=(2, 118, 118), exif=ORIENT6, icc_profile=mm.icc_like(76800), comment=b"x\xff\xd9y", segments=((0xE1, b"http://ns.adobe.com/xap/1.0/\0<x/>"), (0xFE, b"first"))),
            (dict(exif=ORIENT6, icc=mm.icc_like(76800), comment=b"x\xff\xd9y", segments=((0xE1, b"http://ns.adobe.com/xap/1.0/\0<x/>"), (0xFE, b"first"))), (2, 118, 118))),
}
CHUNKS = {"icc_1": 1, "icc_65519": 1, "icc_65520": 2, "icc_131038_all_ff": 2}


def raw_metadata(jpegamd, **fields):
    """A JpegAmdMetadata filled field by field (the C names), with what its pointers refer to."""
    m, keep = jpegamd.Metadata(), []
    m.density_units = -1
    for name, value in fields.items():
        if isinstance(value, bytes):
            buf = C.create_string_buffer(value, max(len(value), 1))
            keep.append(buf)
            value = C.cast(buf, C.c_void_p)
        setattr(m, name, value)
    return m, keep


def build(jpegamd, m, capacity=None):
    """jpegamd_build_metadata -> (result, blob bytes or None, head)."""
    head = C.create_string_buffer(20)
    n = jpegamd.lib.jpegamd_build_metadata(C.byref(m), None, 0, head)
    if n < 0 or capacity is None:
        return n, None, head.raw
    blob = C.create_string_buffer(b"\xa5" * (capacity + 1), capacity + 1)
    assert jpegamd.lib.jpegamd_build_metadata(C.byref(m), blob, capacity, head) == n
    assert blob.raw[capacity:] == b"\xa5"                          # never beyond the capacity
    return n, blob.raw[:capacity], head.raw


# ---- 1. the surface ---------------------------------------------------------------------------------------------------------------------
def test_symbols(jpegamd):
    header = jpegamd.HEADER_PATH.read_text()
    raw = C.CDLL(str(jpegamd.LIB_PATH))
    for name in NEW:
        assert name in jpegamd.EXPORTED and name in jpegamd._BASE and hasattr(raw, name) and name in header, name
    for word in ("JpegAmdSegment", "JpegAmdMetadata", "jpegamd_encoder_metadata_bytes()"):
        assert word in header, word
    assert header.count("jpegamd_encoder_metadata_bytes() more than this bound") == header.count("\nuint64_t jpegamd_max_jfif_bytes")


def test_a_context_is_needed(jpegamd):
    m, _ = raw_metadata(jpegamd)
    assert jpegamd.lib.jpegamd_encoder_set_metadata(None, C.byref(m)) == -1
    assert jpegamd.lib.jpegamd_encoder_set_metadata(None, None) == -1
    assert jpegamd.lib.jpegamd_encoder_metadata_bytes(None) == -1


# ---- 2. the blob and the head against the model -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_build_metadata_is_the_model(jpegamd, name):
    keywords, (blob_kw, density) = CASES[name]
    head, blob = jpegamd.build_metadata(**keywords)
    want = mm.blob(**blob_kw)
    assert head == mm.head(density) and len(head) == 20
    assert blob == want, (len(blob), len(want))
    if name == "nothing":
        assert blob == b"" and head == mm.PLAIN_HEAD
    if name in CHUNKS:
        assert blob.count(b"ICC_PROFILE\0") >= CHUNKS[name] and blob[17] == CHUNKS[name]     # (the count byte of the first chunk)


def test_pil_exif_objects_and_orientation(jpegamd):
    from PIL import Image
    for n in range(1, 9):
        block = jpegamd.exif_orientation(n)
        assert len(block) == 26 and block[:4] == b"II*\0"
        ex = Image.Exif()
        ex.load(b"Exif\0\0" + block)
        assert ex[0x0112] == n
        file = mm.splice((GOLDEN / "one_block.jpg").read_bytes(), *jpegamd.build_metadata(exif=block))
        assert Image.open(io.BytesIO(file)).getexif()[0x0112] == n
    for bad in (0, 9):
        with pytest.raises(ValueError):
            jpegamd.exif_orientation(bad)
    ex = Image.Exif()
    ex[0x0112] = 6
    head, blob = jpegamd.build_metadata(exif=ex)                   # an object with .tobytes()
    assert blob == mm.blob(exif=ex.tobytes()[6:]) and ex.tobytes()[:6] == b"Exif\0\0"


# ---- 3. refusals, one by one ------------------------------------------------------------------------------------------------------------
def segments_of(jpegamd, pairs):
    arr, keep = (jpegamd.Segment * max(len(pairs), 1))(), []
    for seg, (marker, payload) in zip(arr, pairs):
        buf = C.create_string_buffer(payload, max(len(payload), 1))
        keep.append(buf)
        seg.marker, seg.data, seg.len = marker, C.cast(buf, C.c_void_p), len(payload)
    return arr, keep


@pytest.mark.parametrize("marker", [0xE0, 0xDB, 0xD9, 0xC0, 0xFF, 0xF0, -1, 0x1E1])
def test_refused_marker(jpegamd, marker):
    arr, keep = segments_of(jpegamd, [(0xE1, b"ok"), (marker, b"x")])
    m, _ = raw_metadata(jpegamd, segments=arr, segment_count=2)
    assert build(jpegamd, m)[0] == -1
    with pytest.raises(ValueError):
        jpegamd.build_metadata(segments=[(0xE1, b"ok"), (marker, b"x")])
    m.segment_count = 1
    assert build(jpegamd, m)[0] == 6


def test_refused_counts_and_lengths(jpegamd):
    arr, keep = segments_of(jpegamd, [(0xE1 + i % 15, b"") for i in range(17)])
    m, _ = raw_metadata(jpegamd, segments=arr, segment_count=17)
    assert build(jpegamd, m)[0] == -1
    m.segment_count = 16
    assert build(jpegamd, m)[0] == 64
    m.segment_count = -1
    assert build(jpegamd, m)[0] == -1
    arr, keep = segments_of(jpegamd, [(0xE1, FF(65534))])
    m, _ = raw_metadata(jpegamd, segments=arr, segment_count=1)
    assert build(jpegamd, m)[0] == -1
    for field, most, extra in (("exif", 65527, 4 + 6), ("comment", 65533, 4)):
        m, keep = raw_metadata(jpegamd, **{field: FF(most + 1), field + "_len": most + 1})
        assert build(jpegamd, m)[0] == -1, field
        setattr(m, field + "_len", most)
        assert build(jpegamd, m)[0] == most + extra, field
    big = bytes(mm.ICC_MAX + 1)
    m, keep = raw_metadata(jpegamd, icc=big, icc_len=len(big))
    assert build(jpegamd, m)[0] == -1
    m.icc_len = mm.ICC_MAX
    assert build(jpegamd, m)[0] == mm.ICC_MAX + 255 * 18
    for kw in (dict(exif=FF(65528)), dict(comment=FF(65534)), dict(segments=[(0xFE, b"")] * 17)):
        with pytest.raises(ValueError):
            jpegamd.build_metadata(**kw)


@pytest.mark.parametrize("density", [(3, 72, 72), (-2, 72, 72), (1, 0, 72), (1, 72, 0), (1, 65536, 72), (2, 72, 65536), (0, -1, 1)])
def test_refused_density(jpegamd, density):
    m, _ = raw_metadata(jpegamd, density_units=density[0], x_density=density[1], y_density=density[2])
    assert build(jpegamd, m)[0] == -1
    with pytest.raises(ValueError):
        jpegamd.build_metadata(density=density)


def test_null_with_a_length_and_null_arguments(jpegamd):
    for field in ("exif", "icc", "comment"):
        m, _ = raw_metadata(jpegamd, **{field + "_len": 1})
        assert build(jpegamd, m)[0] == -1, field
    m, _ = raw_metadata(jpegamd, segment_count=1)
    assert build(jpegamd, m)[0] == -1
    arr, keep = segments_of(jpegamd, [(0xE1, b"")])
    arr[0].data, arr[0].len = None, 1
    m, _ = raw_metadata(jpegamd, segments=arr, segment_count=1)
    assert build(jpegamd, m)[0] == -1
    arr[0].len = 0                                                   # NULL with length 0: an empty segment
    assert build(jpegamd, m, 4)[:2] == (4, b"\xff\xe1\x00\x02")
    assert jpegamd.lib.jpegamd_build_metadata(None, None, 0, None) == -1
    m, _ = raw_metadata(jpegamd, comment=b"hi", comment_len=2)
    assert jpegamd.lib.jpegamd_build_metadata(C.byref(m), None, 6, None) == -1     # a NULL blob with a capacity
    assert jpegamd.lib.jpegamd_build_metadata(C.byref(m), None, 0, None) == 6      # the head may be left out
    m, _ = raw_metadata(jpegamd, exif=b"", exif_len=0, icc=b"", icc_len=0)          # pointers with length 0: no such segment
    assert build(jpegamd, m, 0)[:2] == (0, b"")


# ---- 4. length-only calls and a capacity that is too small --------------------------------------------------------------------------------
def test_length_only_and_short_capacity(jpegamd):
    m, keep = raw_metadata(jpegamd, comment=b"hello", comment_len=5, density_units=1, x_density=300, y_density=300)
    want = mm.blob(comment=b"hello")
    n, none, head = build(jpegamd, m)
    assert (n, none, head) == (len(want), None, mm.head((1, 300, 300)))
    assert build(jpegamd, m, len(want))[1] == want
    assert build(jpegamd, m, len(want) + 7)[1] == want + b"\xa5" * 7                # (more room: the rest is untouched)
    for cap in (0, 1, len(want) - 1):
        n, got, head = build(jpegamd, m, cap)
        assert n == len(want) and got == b"\xa5" * cap and head == mm.head((1, 300, 300)), cap


# ---- 5. PIL reads the spliced golden files ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["photo_512x512.jpg", "colour"])
def test_pil_reads_a_spliced_file(jpegamd, oracle, name):
    from PIL import Image
    if name == "colour":                                             # (tests/golden holds grayscale files only: the colour model's file)
        import color_model as cm
        plain = cm.rgb_file(oracle, cm.synth_rgb(72, 40, 11, 0), 50, cm.SUB_420)
    else:
        plain = (GOLDEN / name).read_bytes()
    profile, comment = mm.icc_like(76800), b"seen \xff\xd9 through"
    keywords = dict(density=(2, 118, 118), exif=jpegamd.exif_orientation(6), icc_profile=profile, comment=comment)
    head, blob = jpegamd.build_metadata(**keywords)
    assert blob == mm.blob(exif=jpegamd.exif_orientation(6), icc=profile, comment=comment) and blob.count(b"ICC_PROFILE\0") == 2
    file = mm.splice(plain, head, blob)
    assert len(file) == len(plain) + len(blob) and file[20 + len(blob):] == plain[20:]
    a, b = Image.open(io.BytesIO(plain)), Image.open(io.BytesIO(file))
    assert b.info["jfif_unit"] == 2 and b.info["jfif_density"] == (118, 118)
    assert tuple(round(float(v), 1) for v in b.info["dpi"]) == (299.7, 299.7)       # 118 dots per cm
    assert b.info["icc_profile"] == profile
    assert b.getexif()[0x0112] == 6
    assert b.info["comment"] == comment
    assert a.mode == b.mode and a.size == b.size and a.tobytes() == b.tobytes()
    assert a.info["jfif_density"] == (96, 96) and "icc_profile" not in a.info


# ---- 6. the Python helpers ----------------------------------------------------------------------------------------------------------------
def test_build_metadata_keywords(jpegamd):
    assert jpegamd.build_metadata() == (mm.PLAIN_HEAD, b"")
    assert jpegamd.build_metadata(comment="") == (mm.PLAIN_HEAD, b"\xff\xfe\x00\x02")
    assert jpegamd.build_metadata(dpi=72)[0] == mm.head((1, 72, 72))
    assert jpegamd.build_metadata(exif=bytearray(ORIENT6))[1] == mm.blob(exif=ORIENT6)
    for bad in (dict(dpi=72, density=(1, 72, 72)), dict(comment=5), dict(icc_profile="text"), dict(dpi=(72.5, 72)),
                dict(segments=[(0xE1, "text")])):
        with pytest.raises(ValueError):
            jpegamd.build_metadata(**bad)


def test_the_block_is_thread_local_and_restores(jpegamd):
    """jpegamd.metadata without a device: the keywords are this thread's, nest, and are gone behind the block, also by exception; a
    refused description is refused before anything is set."""
    state = lambda: getattr(jpegamd._block_metadata, "keywords", None)
    assert state() is None
    seen = []
    with jpegamd.metadata(comment="outer", dpi=300):
        assert state()["comment"] == "outer" and state()["dpi"] == 300
        th = threading.Thread(target=lambda: seen.append(state()))
        th.start()
        th.join()
        with jpegamd.metadata(icc_profile=b"p"):
            assert state()["icc_profile"] == b"p" and state()["comment"] is None
        assert state()["comment"] == "outer"
    assert state() is None and seen == [None]
    with pytest.raises(KeyError):
        with jpegamd.metadata(comment="x"):
            raise KeyError("x")
    assert state() is None
    with pytest.raises(ValueError):
        with jpegamd.metadata(density=(3, 1, 1)):
            pass
    assert state() is None
