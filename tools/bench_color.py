#!/usr/bin/env python3
"""Colour-file throughput: single 8192^2 encodes (jpegamd_encode_color_async) at 4:2:0 and 4:4:4, timed through the profiling
ring (every kernel's own begin / end events), with the per-kernel durations.  Prints one JSON line per subsampling.

  python tools/bench_color.py [--size 8192] [--steps 50] [--warmup 10] [--quality 50] [--kind 0]

With --batch N the same timed loop goes through jpegamd_encode_color_batch_async: N distinct pictures (seeds 1 .. N) per call,
reported as the whole call's time (ns_total) per picture, and Gpixels/s.

With --source (and --batch N, default 8) the batch loop reads another source, 4:2:0 only: `i420` the Y, Cb and Cr planes and `nv12` the
Y plane and one plane of Cb Cr pairs that the colour path itself derives from the same pictures (computed once, outside the timed
loop), through jpegamd_encode_ycbcr_batch_async -- the files are those of `rgb`, so "bytes" must agree.  Several sources separated
by commas (--source rgb,i420,nv12) run one after the other in ONE process: one session, one set of pictures.
`i422` (three planes) and `yuyv` (one packed YUY2 plane per picture) are the 4:2:2 sources, derived the same way.
--subsampling {420,444,422} picks ONE subsampling for the rgb loops (default: 4:2:0 and 4:4:4 in turn, as before).
--range limited (i420, nv12, i422, yuyv) takes the same samples as limited ("video") range: the calls go through
jpegamd_encode_ycbcr_range_batch_async with JPEGAMD_RANGE_LIMITED, which expands them on read; the line then carries "range".  With
--convert it also times what that replaces, in the same run: the range map as a pass of its own over the planes (a torch table
lookup, lut[plane.long()], into preallocated planes: "convert_us_per_picture") and the full-range encode of the planes it wrote
("mapped_full_us_per_picture", whose files must be the limited ones: "mapped_bytes_equal").
`p010` and `i010` are the 10-bit 4:2:0 sources: the samples of `nv12` / `i420` as 16-bit words -- s << 8 (MSB-aligned: one plane of Y words
and one of Cb Cr pairs of words per picture) and s << 2 (LSB-aligned: three planes) -- through jpegamd_encode_ycbcr_samples_batch_async,
which narrows them on read: at full range the files are those of `nv12`, so "bytes" must agree.  With --narrow they also time what
that replaces, in the same run: the narrowing as a pass of its own over the planes (16-bit words in, bytes out, into preallocated
planes: "narrow_us_per_picture") and the 8-bit encode of the planes it wrote at the same --range ("narrowed_8bit_us_per_picture").

--matrix bt709 (the YCbCr sources) takes the same samples as BT.709 YCbCr: the calls go through jpegamd_encode_ycbcr_matrix_batch_async
with JPEGAMD_MATRIX_BT709, whose one pass (k_ycbcr_matrix_batch) converts them to BT.601 planes in context scratch; the line then carries
"matrix", and "pass_bytes_per_picture": what that pass reads and writes, from the shapes.  With --convert (i420, nv12, p010, i010) it also
times the route a caller has without the entry, in the same run: the same conversion written with torch ops into preallocated 8-bit
planes ("convert_us_per_picture"; the range / depth map first where the source has one), then the plain encode of the planes it wrote
("converted_plain_us_per_picture", whose files must be the BT.709 call's: "converted_bytes_equal").

With --layout {hwc,chw,rgba} (and --batch N, default 8) the pictures are device tensors stored that way -- [N, H, W, 3], [N, 3, H, W],
[N, H, W, 4] -- and go through the entry that reads them where they lie, 4:2:0 only.  Every call is timed as a whole between two
events on the stream; --rounds R medians of --steps calls each are reported, with their spread (max - min).  --repack (chw only)
also times the route without the planar entry, in the same run and alternating with the direct one: permute(0, 2, 3, 1) into a
preallocated [N, H, W, 3] tensor, then the packed batch entry.

--scan interleaved (with --batch N, default 8) sends the batch loop through the one-scan entries; the line then carries "scan".  The
whole call is timed (ns_total); the per-kernel split comes from a kernel trace of the same command.  Sources rgb, i420, nv12, i422 at
--range full --matrix bt601 keep to jpegamd_encode_color_interleaved_batch_async / jpegamd_encode_ycbcr_interleaved_batch_async (a
library from before the entries below still serves them); yuyv, p010, i010, --range limited and --matrix bt709 go through
jpegamd_encode_ycbcr_interleaved_matrix_batch_async, and --layout chw / rgba through jpegamd_encode_planar_interleaved_batch_async /
jpegamd_encode_color_interleaved_pixels_batch_async.  --mapped (with --range limited; i420, nv12, i422) applies the range map to the
frames once, outside the timed loop, and codes the mapped frames at full range: what the older entries code for the same input.
--restart N|row (with --scan interleaved alone): restart intervals of N MCUs, or of one MCU row, through the _restart entries
(jpegamd_encode_color_interleaved_restart_batch_async / jpegamd_encode_ycbcr_interleaved_restart_batch_async); the line then carries
"restart_interval" in MCUs.  --restart 0 goes through those entries with interval 0 (the file without restart intervals).
--huffman standard|optimized (with --scan interleaved alone): the Annex K tables, or per-picture optimised tables
(jpegamd_encoder_set_huffman on the context); the line then carries "huffman".  `standard` sets nothing on the
context, so a library from before the mode serves it.

--scan progressive (with --batch N, default 8) sends the batch loop through the progressive entries:
jpegamd_encode_color_progressive_batch_async for rgb, jpegamd_encode_ycbcr_progressive_batch_async for every YCbCr source, --range and
--matrix; the whole call is timed (ns_total), the line carries "scan": "progressive".  No --restart, --layout, --convert, --narrow.
With --huffman optimized the loop goes through jpegamd_encode_*_progressive_optimized_batch_async (end-of-band runs and
per-scan optimised tables; nothing is set on the context); --huffman standard is the plain progressive loop.  With --successive as
well it goes through jpegamd_encode_*_progressive_successive_batch_async (the ten scans of successive approximation);
the line then carries "successive": true.
--scans NAME|FILE (with --scan progressive; rgb pictures) goes through the entries that take a scan script: NAME is
spectral, successive (the built-in scripts, passed explicitly) or gray (the default script of a grayscale file); FILE holds a script in
the text form of libjpeg's -scans files (jpegamd.progressive_script.parse_scan_script).  A script in which component 0 alone appears
writes grayscale files (the luma of the pictures) through jpegamd_encode_gray_progressive_script_batch_async.  The line carries "scans".

--qtables FILE (every mode): the context encodes with the one or two quantisation tables of FILE -- the text form of cjpeg -qtables,
64 decimal values a table in raster order, `#` comments (jpegamd.parse_qtables; examples in tools/qtables/) -- set through
jpegamd_encoder_set_quant_tables; --quality then selects nothing, and every line carries "qtables".

--icc BYTES, --comment TEXT, --dpi N (every mode, any of them): the context writes metadata into every file -- a synthetic ICC profile of
BYTES bytes, a comment, a pixel density -- set through jpegamd_encoder_set_metadata; every buffer is sized as the
bound + Encoder.metadata_bytes(), and every line carries "metadata_bytes".  The batch loop and --scan gray also time the same call with
the metadata taken off, in the same run: "no_metadata_ns_total_median" and "metadata_ratio".  The time of a call includes
k_metadata_place.

--source float32|float16|bfloat16 (with --batch N, default 8; --layout chw, the default, or hwc; every --scan mode) times FLOAT pictures
in [0, 1] through the float entries (jpegamd_encode_float_batch_async, _interleaved_, _progressive_script_; --scan gray:
the luma through the one-scan entry with subsampling 0).  Routes `float`, `convert` (the four torch ops of a caller without the entry,
then the uint8 entry of the same layout), `uint8` (that entry alone on the bytes) and `copy` (a device copy of as many bytes as the front
pass moves) alternate in one run, --rounds medians of --steps calls each, timed between events on the stream; one line per route.

--reduce F (1 .. 8; with --batch N, default 8; --layout chw, the default, or hwc; every --scan mode) times uint8 pictures of --size pixels
each way encoded REDUCED by F both ways through the reduced entries (jpegamd_encode_reduced_batch_async, _interleaved_,
_progressive_script_; --scan gray: the luma through the one-scan entry with subsampling 0).  Routes `reduced`, `resize` (what a caller
does without the entry: a float copy, avg_pool2d with ceil_mode and divisor_override=1, the division by the box counts, +0.5, floor,
clamp, the cast and the planar uint8 entry, as one unit), `uint8` (the uint8 entry of the same layout alone on bytes reduced beforehand:
the floor) and `copy` (a device copy of as many bytes as the source holds) alternate in one run, --rounds medians of --steps calls
each, timed between events on the stream; one line per route.

--resize WxH (beside --reduce, with the same options) times uint8 pictures of --size pixels each way encoded RESIZED to W x H through the
resized entries (jpegamd_encode_resized_batch_async, _interleaved_, _progressive_script_), in every --scan mode.  Routes
`resized`, `resize` (what a caller does without the entry: a float copy, F.interpolate(mode="area"), +0.5, floor, clamp, the cast and the
planar uint8 entry, as one unit; torch's area mode gives whole samples to a bin, so its bytes are close to the entry's and not equal),
`uint8` (the uint8 entry alone on bytes resized beforehand: the floor) and `copy`, as for --reduce.

--scan gray (with --batch N, default 8) times GRAYSCALE files through jpegamd_encode_gray_scan_batch_async: the luma
of the same --size pictures, --restart N|row in blocks (`row`: ceil(W / 8)), --huffman standard|optimized; the whole call is timed
(ns_total).  Without --restart (or with 0) and with the standard tables the entry is jpegamd_encode_batch_async, so that line is the
fused grayscale path's time; "plain_us_per_picture" is jpegamd_encode_batch_async itself, timed in the same run.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "jpeg-image-compression_amd" / "python"))

KERNELS = ["k_chroma_planes", "Y k_tile_encode", "Y k_segment_merge", "Y k_finalize", "Cb k_tile_encode", "Cb k_segment_merge",
           "Cb k_finalize", "Cr k_tile_encode", "Cr k_segment_merge", "Cr k_finalize", "k_append_scans"]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--quality", type=int, default=50)
    ap.add_argument("--kind", type=int, default=0)
    ap.add_argument("--batch", type=int, default=None, help="pictures per call through the colour batch entry (1 .. 32)")
    ap.add_argument("--source", default="rgb", help="rgb (default), i420, nv12, i422, yuyv, p010, i010, or several separated by commas: what the batch loop reads")
    ap.add_argument("--subsampling", choices=("420", "444", "422"), default=None, help="rgb: this subsampling alone (default: 420, then 444)")
    ap.add_argument("--range", choices=("full", "limited"), default="full", dest="sample_range",
                    help="i420 / nv12 / i422 / yuyv: the samples are full range (default) or limited range, expanded on read")
    ap.add_argument("--matrix", choices=("bt601", "bt709"), default="bt601",
                    help="the YCbCr sources: the samples are BT.601 (default) or BT.709 YCbCr, converted by one pass in front of the tile kernel")
    ap.add_argument("--convert", action="store_true", help="--range limited: also time the map as a separate pass + the full-range encode; "
                    "--matrix bt709: the conversion with torch ops + the plain encode")
    ap.add_argument("--narrow", action="store_true", help="p010 / i010: also time the narrowing as a separate pass + the 8-bit encode")
    ap.add_argument("--layout", choices=("hwc", "chw", "rgba"), default=None, help="device tensors stored this way, read where they lie")
    ap.add_argument("--rounds", type=int, default=5, help="--layout: medians taken (each of --steps calls)")
    ap.add_argument("--repack", action="store_true", help="--layout chw: also time permute + packed encode")
    ap.add_argument("--scan", choices=("separate", "interleaved", "gray", "progressive"), default="separate",
                    help="interleaved: the batch loop goes through the one-scan entries (every --source, --range, --matrix; --layout chw / rgba); "
                    "gray: grayscale files through jpegamd_encode_gray_scan_batch_async (--batch, --restart, --huffman); "
                    "progressive: the batch loop goes through the progressive entries (every --source, --range, --matrix)")
    ap.add_argument("--mapped", action="store_true",
                    help="--range limited (i420, nv12, i422): map the frames once outside the timed loop and code them at full range")
    ap.add_argument("--huffman", choices=("standard", "optimized"), default=None,
                    help="--scan interleaved: the Annex K tables, or per-picture optimised tables")
    ap.add_argument("--restart", default=None, metavar="N|row",
                    help="--scan interleaved: restart intervals of N MCUs (0 .. 65535), or `row` for one MCU row")
    ap.add_argument("--successive", action="store_true",
                    help="--scan progressive --huffman optimized: the ten scans of successive approximation (DESIGN.md 4.6.14)")
    ap.add_argument("--scans", default=None, metavar="NAME|FILE",
                    help="--scan progressive: a scan script -- spectral, successive, gray, or a file in libjpeg's -scans text form (DESIGN.md 4.6.15)")
    ap.add_argument("--qtables", default=None, metavar="FILE",
                    help="every --scan mode: quantisation tables of the caller's, one or two in the text form of cjpeg -qtables (tools/qtables/)")
    ap.add_argument("--icc", type=int, default=None, metavar="BYTES", help="every --scan mode: a synthetic ICC profile of this length in every file")
    ap.add_argument("--comment", default=None, metavar="TEXT", help="every --scan mode: a comment in every file")
    ap.add_argument("--dpi", type=int, default=None, metavar="N", help="every --scan mode: this pixel density in every file")
    ap.add_argument("--reduce", type=int, default=None, metavar="F",
                    help="every --scan mode: uint8 pictures encoded reduced by F (1 .. 8) both ways through the reduced entries (DESIGN.md 4.6.19)")
    ap.add_argument("--resize", default=None, metavar="WxH",
                    help="every --scan mode: uint8 pictures encoded resized to W x H through the resized entries (DESIGN.md 4.6.20)")
    a = ap.parse_args()
    if a.scans is not None and (a.scan != "progressive" or a.successive or a.huffman is not None or a.source != "rgb"):
        sys.exit("--scans needs --scan progressive and takes --size, --batch, --subsampling, --quality, --kind alone")
    if a.successive and (a.scan != "progressive" or a.huffman != "optimized"):
        sys.exit("--successive needs --scan progressive --huffman optimized")
    import torch                          # (the device runtime comes up through torch first, as in bench.py)
    if not torch.cuda.is_available():
        sys.exit("bench_color.py: no GPU")
    torch.cuda.set_device(0)
    import jpegamd

    dev = torch.device("cuda:0")
    w = h = a.size
    sources = a.source.split(",")
    if a.resize is not None:
        if a.reduce is not None:
            sys.exit("--resize and --reduce are two runs")
        try:
            a.resize = tuple(int(v) for v in a.resize.lower().split("x"))
            jpegamd.resize_check(w, h, *a.resize)
        except (ValueError, TypeError) as e:
            sys.exit(f"--resize takes WxH: {e}")
    if a.reduce is not None or a.resize is not None:
        if a.reduce is not None and not 1 <= a.reduce <= jpegamd.MAX_REDUCE:
            sys.exit(f"--reduce takes 1 .. {jpegamd.MAX_REDUCE}")
        if a.source != "rgb" or a.sample_range != "full" or a.matrix != "bt601" or a.convert or a.narrow or a.mapped or a.repack or a.scans or a.successive:
            sys.exit("--reduce and --resize take --size, --batch, --layout chw|hwc, --scan, --subsampling, --restart, --huffman, --rounds, --quality, --kind, "
                     "--qtables and the metadata options alone")
        if a.scan in ("separate", "progressive") and (a.restart is not None or a.huffman is not None):
            sys.exit("--restart and --huffman need --scan interleaved or gray")
        if a.scan == "gray" and a.subsampling:
            sys.exit("--scan gray has no --subsampling")
        run_reduce(a, jpegamd, torch, dev)
        return
    if any(s in FLOAT_SOURCES for s in sources):
        if any(s not in FLOAT_SOURCES for s in sources):
            sys.exit("--source float32, float16 and bfloat16 do not mix with the byte sources")
        if a.sample_range != "full" or a.matrix != "bt601" or a.convert or a.narrow or a.mapped or a.repack or a.scans or a.successive:
            sys.exit("--source float32|float16|bfloat16 takes --size, --batch, --layout chw|hwc, --scan, --subsampling, --restart, --huffman, "
                     "--rounds, --quality, --kind, --qtables and the metadata options alone")
        if a.scan in ("separate", "progressive") and (a.restart is not None or a.huffman is not None):
            sys.exit("--restart and --huffman need --scan interleaved or gray")
        if a.scan == "gray" and a.subsampling:
            sys.exit("--scan gray has no --subsampling")
        for s in sources:
            run_float(a, jpegamd, torch, dev, s)
        return
    if any(s not in ("rgb", "i420", "nv12", "i422", "yuyv", "p010", "i010") for s in sources):
        sys.exit("--source takes rgb, i420, nv12, i422, yuyv, p010, i010 or a comma-separated list of them")
    if a.sample_range != "full" and "rgb" in sources:
        sys.exit("--range limited is for the YCbCr sources (i420, nv12, i422, yuyv, p010, i010)")
    if a.matrix != "bt601" and "rgb" in sources:
        sys.exit("--matrix bt709 is for the YCbCr sources (i420, nv12, i422, yuyv, p010, i010)")
    if a.convert and a.sample_range != "limited" and a.matrix != "bt709":
        sys.exit("--convert needs --range limited or --matrix bt709")
    if a.convert and a.matrix == "bt709" and any(s in ("i422", "yuyv") for s in sources):
        sys.exit("--matrix bt709 --convert takes the 4:2:0 sources (i420, nv12, p010, i010)")
    if a.convert and a.matrix == "bt709" and a.sample_range == "limited" and any(s in ("p010", "i010") for s in sources):
        sys.exit("--matrix bt709 --convert with p010 / i010 is written for --range full (the torch route narrows by a shift)")
    if a.narrow and not any(s in ("p010", "i010") for s in sources):
        sys.exit("--narrow needs --source p010 or i010")
    if a.scan == "interleaved" and (a.convert or a.narrow):
        sys.exit("--convert and --narrow time routes of the three-scan path: not with --scan interleaved")
    if a.scan == "progressive" and (a.convert or a.narrow or a.layout is not None or a.restart is not None):
        sys.exit("--scan progressive takes --size, --batch, --source, --subsampling, --range, --matrix, --mapped, --quality, --kind, --huffman alone")
    if a.mapped and (a.sample_range != "limited" or any(s not in ("i420", "nv12", "i422") for s in sources)):
        sys.exit("--mapped needs --range limited and takes --source i420, nv12, i422")
    if a.huffman is not None and a.scan == "separate":
        sys.exit("--huffman needs --scan interleaved or gray")
    if a.restart is not None:
        if a.scan == "separate":
            sys.exit("--restart needs --scan interleaved or gray")
        if a.restart != "row" and not (a.restart.isdigit() and int(a.restart) <= 65535):
            sys.exit("--restart takes a number of MCUs, 0 .. 65535, or `row`")
    if a.scans is not None:
        if a.convert or a.narrow or a.mapped or a.layout is not None or a.restart is not None:
            sys.exit("--scans takes --size, --batch, --subsampling, --quality, --kind alone")
        run_scans(a, jpegamd, torch, dev)
        return
    if a.scan == "gray":
        if sources != ["rgb"] or a.layout is not None or a.convert or a.narrow or a.mapped or a.subsampling:
            sys.exit("--scan gray takes --size, --batch, --restart, --huffman, --quality, --kind alone")
        run_gray(a, jpegamd, torch, dev)
        return
    if a.layout is not None:
        run_layout(a, jpegamd, torch, dev)
        return
    if a.batch is not None or sources != ["rgb"] or a.scan in ("interleaved", "progressive"):
        run_batch(a, jpegamd, torch, dev, sources)
        return
    bmp = jpegamd.synth_bmp(w, h, 1, a.kind, 0)
    img, off = jpegamd.parse_bmp(bmp)
    px = torch.frombuffer(bytearray(bmp[off:off + img.row_stride * h]), dtype=torch.uint8).to(dev)
    desc = jpegamd.Encoder.image(px.data_ptr(), w, h, img.row_stride, True, jpegamd.ORDER_BGR, a.quality)
    enc = new_encoder(a, jpegamd, w, h)
    stream = torch.cuda.current_stream().cuda_stream
    for sub, name in rgb_subsamplings(a, jpegamd):
        cap = jpegamd.max_jfif_bytes_color(w, h, sub) + a.metadata_bytes
        out = torch.empty(cap, dtype=torch.uint8, device=dev)
        size = torch.zeros(1, dtype=torch.int64, device=dev)
        for _ in range(a.warmup):
            enc.encode_color_async(desc, sub, out.data_ptr(), cap, size.data_ptr(), stream)
        enc.finish()
        enc.set_profiling(a.steps)
        for _ in range(a.steps):
            enc.encode_color_async(desc, sub, out.data_ptr(), cap, size.data_ptr(), stream)
        st = enc.finish()
        per = [enc.color_profile(i) for i in range(a.steps)]
        totals = [enc.profile(i).ns_total for i in range(a.steps)]
        enc.set_profiling(0)
        med = {k: int(statistics.median(p[i] for p in per)) for i, k in enumerate(KERNELS)}
        t = statistics.median(totals)
        report(a, {"subsampling": name, "width": w, "height": h, "quality": a.quality, "kind": a.kind, "steps": a.steps,
                    "bytes": int(size.item()), "entropy_bits": st.entropy_bits, "ns_total_median": int(t),
                    "gpixels_per_s": round(w * h / t, 2), "kernel_ns_median": med,
                    "kernel_ns_sum": sum(med.values())})


def new_encoder(a, jpegamd, w, rows):
    """The context of a run, with the tables of --qtables set on it."""
    enc = jpegamd.Encoder(w, rows)
    if a.qtables is not None:
        with open(a.qtables, encoding="utf-8") as f:
            enc.set_quant_tables(*jpegamd.parse_qtables(f.read()))
    a.metadata = {}
    if a.icc is not None:
        a.metadata["icc_profile"] = bytes((i * 197 + 31) & 0xFF for i in range(a.icc))
    if a.comment is not None:
        a.metadata["comment"] = a.comment
    if a.dpi is not None:
        a.metadata["dpi"] = a.dpi
    if a.metadata:
        enc.set_metadata(**a.metadata)
    a.metadata_bytes = enc.metadata_bytes()
    return enc


def without_metadata(a, enc, timed):
    """{}, or -- with metadata on the context -- the same timed call with the metadata taken off: its median and the ratio to `t`."""
    if not a.metadata:
        return lambda t: {}
    enc.set_metadata(None)
    try:
        plain = timed()
    finally:
        enc.set_metadata(**a.metadata)
    return lambda t: {"no_metadata_ns_total_median": int(plain), "metadata_ratio": round(t / plain, 4)}


def report(a, line) -> None:
    """One JSON result line; with --qtables it names the file whose tables wrote the files ("quality" then selected nothing)."""
    if getattr(a, "metadata", None):
        line = dict(line, metadata_bytes=a.metadata_bytes)
    print(json.dumps(dict(line, qtables=a.qtables) if a.qtables is not None else line))


def rgb_subsamplings(a, jpegamd):
    subs = {"420": jpegamd.SUBSAMPLE_420, "444": jpegamd.SUBSAMPLE_444, "422": jpegamd.SUBSAMPLE_422}
    return [(subs[a.subsampling], a.subsampling)] if a.subsampling else [(subs["420"], "420"), (subs["444"], "444")]


def ycbcr_422(torch, px, w, h, stride):
    """... at 4:2:2: Y [H, W], Cb and Cr [H, W / 2], (a + b + 1) >> 1 over the pixel pairs of a row."""
    bgr = px.view(h, stride)[:, :3 * w].reshape(h, w, 3).flip(0)
    b, g, r = (bgr[:, :, k].to(torch.int32) for k in range(3))
    y = ((77 * r + 150 * g + 29 * b) >> 8).to(torch.uint8)

    def pair(p):
        return ((p[:, 0::2] + p[:, 1::2] + 1) >> 1).to(torch.uint8)
    return y, pair((32768 - 43 * r - 85 * g + 128 * b) >> 8), pair((32768 + 128 * r - 107 * g - 21 * b) >> 8)


def ycbcr_420(torch, px, w, h, stride):
    """The planes the colour path derives from one stored picture (bottom-up B, G, R rows): Y [H, W], Cb and Cr [H / 2, W / 2]."""
    bgr = px.view(h, stride)[:, :3 * w].reshape(h, w, 3).flip(0)
    b, g, r = (bgr[:, :, k].to(torch.int32) for k in range(3))
    y = ((77 * r + 150 * g + 29 * b) >> 8).to(torch.uint8)

    def box(p):
        return ((p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2) >> 2).to(torch.uint8)
    cb = box((32768 - 43 * r - 85 * g + 128 * b) >> 8)
    cr = box((32768 + 128 * r - 107 * g - 21 * b) >> 8)
    return y, cb, cr


def run_gray(a, jpegamd, torch, dev) -> None:
    """--scan gray: N pictures per call through jpegamd_encode_gray_scan_batch_async, and through jpegamd_encode_batch_async."""
    w = h = a.size
    n = a.batch or 8
    pxs, descs = [], []
    for i in range(n):
        bmp = jpegamd.synth_bmp(w, h, 1 + i, a.kind, 0)
        img, off = jpegamd.parse_bmp(bmp)
        pxs.append(torch.frombuffer(bytearray(bmp[off:off + img.row_stride * h]), dtype=torch.uint8).to(dev))
        descs.append(jpegamd.Encoder.image(pxs[-1].data_ptr(), w, h, img.row_stride, True, jpegamd.ORDER_BGR, a.quality))
        del bmp
    enc = new_encoder(a, jpegamd, w, n * h)
    restart = 0 if a.restart is None else (-(-w // 8) if a.restart == "row" else int(a.restart))
    cap = max(jpegamd.max_jfif_bytes_gray_scan(w, h, restart), jpegamd.max_jfif_bytes(w, h)) + a.metadata_bytes
    outs = [torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(n)]
    sizes = torch.zeros(n, dtype=torch.int64, device=dev)
    out_ptrs = [o.data_ptr() for o in outs]
    size_ptrs = [sizes.data_ptr() + 8 * i for i in range(n)]
    stream = torch.cuda.current_stream().cuda_stream

    def timed(call):
        for _ in range(a.warmup):
            call()
        enc.finish()
        enc.set_profiling(a.steps)
        for _ in range(a.steps):
            call()
        st = enc.finish()
        totals = [enc.profile(i).ns_total for i in range(a.steps)]
        enc.set_profiling(0)
        return statistics.median(totals), st, sizes.cpu().tolist()

    plain, _, plain_bytes = timed(lambda: enc.encode_batch_async(descs, out_ptrs, cap, size_ptrs, True, stream))
    if a.huffman == "optimized":
        enc.set_huffman(jpegamd.HUFFMAN_OPTIMIZED)
    t, st, got = timed(lambda: enc.encode_gray_scan_batch_async(descs, restart, out_ptrs, cap, size_ptrs, stream))
    report(a, {"scan": "gray", "width": w, "height": h, "batch": n, "quality": a.quality, "kind": a.kind, "steps": a.steps,
                "restart_interval": restart, "huffman": a.huffman or "standard", "bytes": got, "entropy_bits": st.entropy_bits,
                "ns_total_median": int(t), "us_per_picture": round(t / n / 1000, 1), "gpixels_per_s": round(n * w * h / t, 2),
                "plain_bytes": plain_bytes, "plain_us_per_picture": round(plain / n / 1000, 1), "ratio_to_plain": round(t / plain, 2),
                **without_metadata(a, enc, lambda: timed(lambda: enc.encode_gray_scan_batch_async(descs, restart, out_ptrs, cap, size_ptrs, stream))[0])(t)})


def run_scans(a, jpegamd, torch, dev) -> None:
    """--scan progressive --scans: N pictures per call through the entries that take a scan script."""
    import jpegamd.progressive_script as ps
    named = {"spectral": ps.SPECTRAL, "successive": ps.SUCCESSIVE, "gray": ps.GRAY_SUCCESSIVE}
    if a.scans in named:
        script = named[a.scans]
    else:
        with open(a.scans, encoding="utf-8") as f:
            script = ps.parse_scan_script(f.read())
    gray = all(comps == (0,) for comps, *_ in script)
    jpegamd.validate_scan_script(script, 1 if gray else 3)
    w = h = a.size
    n = a.batch or 8
    pxs, descs = [], []
    for i in range(n):
        bmp = jpegamd.synth_bmp(w, h, 1 + i, a.kind, 0)
        img, off = jpegamd.parse_bmp(bmp)
        pxs.append(torch.frombuffer(bytearray(bmp[off:off + img.row_stride * h]), dtype=torch.uint8).to(dev))
        descs.append(jpegamd.Encoder.image(pxs[-1].data_ptr(), w, h, img.row_stride, True, jpegamd.ORDER_BGR, a.quality))
        del bmp
    enc = new_encoder(a, jpegamd, w, n * h)
    stream = torch.cuda.current_stream().cuda_stream
    for sub, name in ([(0, "gray")] if gray else rgb_subsamplings(a, jpegamd)):
        cap = jpegamd.max_jfif_bytes_progressive_script(w, h, sub, script) + a.metadata_bytes
        outs = [torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(n)]
        sizes = torch.zeros(n, dtype=torch.int64, device=dev)
        out_ptrs = [o.data_ptr() for o in outs]
        size_ptrs = [sizes.data_ptr() + 8 * i for i in range(n)]
        if gray:
            call = lambda: enc.encode_gray_progressive_script_batch_async(descs, script, out_ptrs, cap, size_ptrs, stream)
        else:
            call = lambda: enc.encode_color_progressive_script_batch_async(descs, sub, script, out_ptrs, cap, size_ptrs, stream)
        for _ in range(a.warmup):
            call()
        enc.finish()
        enc.set_profiling(a.steps)
        for _ in range(a.steps):
            call()
        st = enc.finish()
        totals = [enc.profile(i).ns_total for i in range(a.steps)]
        enc.set_profiling(0)
        t = statistics.median(totals)
        report(a, {"source": "rgb", "subsampling": name, "width": w, "height": h, "batch": n, "quality": a.quality, "kind": a.kind,
                    "steps": a.steps, "bytes": sizes.cpu().tolist(), "entropy_bits": st.entropy_bits, "ns_total_median": int(t),
                    "us_per_picture": round(t / n / 1000, 1), "gpixels_per_s": round(n * w * h / t, 2), "scan": "progressive",
                    "scans": a.scans, "scan_count": len(script)})
        del outs


def run_batch(a, jpegamd, torch, dev, sources=("rgb",)) -> None:
    w = h = a.size
    n = a.batch or 8
    if any(s != "rgb" for s in sources) and (w % 2 or h % 2):
        sys.exit("--source i420 / nv12 / i422 / yuyv / p010 / i010 needs an even --size")
    pxs, descs = [], []
    for i in range(n):
        bmp = jpegamd.synth_bmp(w, h, 1 + i, a.kind, 0)
        img, off = jpegamd.parse_bmp(bmp)
        pxs.append(torch.frombuffer(bytearray(bmp[off:off + img.row_stride * h]), dtype=torch.uint8).to(dev))
        descs.append(jpegamd.Encoder.image(pxs[-1].data_ptr(), w, h, img.row_stride, True, jpegamd.ORDER_BGR, a.quality))
        del bmp
    enc = new_encoder(a, jpegamd, w, n * h)
    if a.huffman == "optimized" and a.scan != "progressive":      # (the optimised progressive entries do not read the context's mode)
        enc.set_huffman(jpegamd.HUFFMAN_OPTIMIZED)
    stream = torch.cuda.current_stream().cuda_stream
    frames = None
    if any(s in ("i420", "nv12", "p010", "i010") for s in sources):   # NV12 frames [N, 3 H / 2, W], and the chroma as two planes
        frames = torch.empty((n, 3 * h // 2, w), dtype=torch.uint8, device=dev)
        cbs, crs = (torch.empty((n, h // 2, w // 2), dtype=torch.uint8, device=dev) for _ in range(2))
        for i in range(n):
            y, cbs[i], crs[i] = ycbcr_420(torch, pxs[i], w, h, img.row_stride)
            frames[i, :h] = y
            frames[i, h:].view(h // 2, w // 2, 2)[:, :, 0] = cbs[i]
            frames[i, h:].view(h // 2, w // 2, 2)[:, :, 1] = crs[i]
            del y
    runs = []
    packed = None
    if "p010" in sources:                                        # the same frames as 16-bit words, the sample in the high byte
        frames16 = frames.to(torch.int16) << 8
    if "i010" in sources:                                        # ... and as three planes of words with the value in the low ten bits
        ys16, cbs16, crs16 = (t.to(torch.int16) << 2 for t in (frames[:, :h], cbs, crs))
    if any(s in ("i422", "yuyv") for s in sources):              # YUY2 frames [N, H, W, 2], and the same samples as three planes
        packed = torch.empty((n, h, w, 2), dtype=torch.uint8, device=dev)
        cbs2, crs2 = (torch.empty((n, h, w // 2), dtype=torch.uint8, device=dev) for _ in range(2))
        for i in range(n):
            y, cbs2[i], crs2[i] = ycbcr_422(torch, pxs[i], w, h, img.row_stride)
            packed[i, :, :, 0] = y
            packed[i, :, 0::2, 1] = cbs2[i]
            packed[i, :, 1::2, 1] = crs2[i]
            del y
        ys2 = packed[:, :, :, 0].contiguous()
    for source in sources:
        # a YCbCr source: its tensors, and the descriptors of pictures stored in tensors of those shapes (--convert writes a second set)
        if source == "rgb":
            runs += [(source, sub, name, None, None) for sub, name in rgb_subsamplings(a, jpegamd)]
        elif source == "p010":                                   # strides in bytes: 2 W for the Y words and for the W / 2 pairs of words
            runs.append((source, jpegamd.SUBSAMPLE_420, "420", (frames16,), lambda t: [
                jpegamd.Encoder.ycbcr_image(t[0][i].data_ptr(), t[0][i, h:].data_ptr(), 0, w, h, 2 * w, 2 * w,
                                            jpegamd.CHROMA_CBCR, a.quality) for i in range(n)]))
        elif source == "i010":
            runs.append((source, jpegamd.SUBSAMPLE_420, "420", (ys16, cbs16, crs16), lambda t: [
                jpegamd.Encoder.ycbcr_image(t[0][i].data_ptr(), t[1][i].data_ptr(), t[2][i].data_ptr(), w, h, 2 * w, w,
                                            jpegamd.CHROMA_PLANES, a.quality) for i in range(n)]))
        elif source == "i422":
            runs.append((source, jpegamd.SUBSAMPLE_422, "422", (ys2, cbs2, crs2), lambda t: [
                jpegamd.Encoder.ycbcr_image(t[0][i].data_ptr(), t[1][i].data_ptr(), t[2][i].data_ptr(), w, h, w, w // 2,
                                            jpegamd.CHROMA_PLANES, a.quality) for i in range(n)]))
        elif source == "yuyv":
            runs.append((source, jpegamd.SUBSAMPLE_422, "422", (packed,), lambda t: [
                jpegamd.Encoder.ycbcr_image(t[0][i].data_ptr(), 0, 0, w, h, 2 * w, 0, jpegamd.CHROMA_YUYV, a.quality) for i in range(n)]))
        elif source == "i420":
            runs.append((source, jpegamd.SUBSAMPLE_420, "420", (frames, cbs, crs), lambda t: [
                jpegamd.Encoder.ycbcr_image(t[0][i].data_ptr(), t[1][i].data_ptr(), t[2][i].data_ptr(), w, h, w, w // 2,
                                            jpegamd.CHROMA_PLANES, a.quality) for i in range(n)]))
        else:
            runs.append((source, jpegamd.SUBSAMPLE_420, "420", (frames,), lambda t: [
                jpegamd.Encoder.ycbcr_image(t[0][i].data_ptr(), t[0][i, h:].data_ptr(), 0, w, h, w, w,
                                            jpegamd.CHROMA_CBCR, a.quality) for i in range(n)]))
    limited = a.sample_range == "limited"
    bt709 = a.matrix == "bt709"
    lut_y = lut_c = None
    if (a.convert or a.mapped) and limited:
        lut_y = torch.tensor([(255 * (min(max(v, 16), 235) - 16) + 109) // 219 for v in range(256)], dtype=torch.uint8, device=dev)
        lut_c = torch.tensor([(255 * (min(max(v, 16), 240) - 16) + 112) // 224 for v in range(256)], dtype=torch.uint8, device=dev)
    if a.mapped:                                                 # the frames as the range map leaves them, coded at full range from here on
        if frames is not None:
            for i in range(n):                                   # (picture by picture: the index tensors of a lookup are eight times the plane)
                frames[i, :h] = lut_y[frames[i, :h].long()]
                frames[i, h:] = lut_c[frames[i, h:].long()]
                cbs[i], crs[i] = lut_c[cbs[i].long()], lut_c[crs[i].long()]
        if packed is not None:
            for i in range(n):
                ys2[i], cbs2[i], crs2[i] = lut_y[ys2[i].long()], lut_c[cbs2[i].long()], lut_c[crs2[i].long()]
        limited = False
    for source, sub, name, tensors, describe in runs:
        ycc = describe(tensors) if describe else None
        one_scan, progressive = a.scan == "interleaved", a.scan == "progressive"
        cap = jpegamd.max_jfif_bytes_interleaved(w, h, sub) if one_scan else jpegamd.max_jfif_bytes_color(w, h, sub)
        own = progressive and a.huffman == "optimized"
        # the three progressive files: (bound, entry of packed pixels, entry of YCbCr pictures)
        bound, color_entry, ycbcr_entry = (jpegamd.max_jfif_bytes_progressive, enc.encode_color_progressive_batch_async,
                                           enc.encode_ycbcr_progressive_batch_async)
        if own and a.successive:
            bound, color_entry, ycbcr_entry = (jpegamd.max_jfif_bytes_progressive_successive, enc.encode_color_progressive_successive_batch_async,
                                               enc.encode_ycbcr_progressive_successive_batch_async)
        elif own:
            bound, color_entry, ycbcr_entry = (jpegamd.max_jfif_bytes_progressive_optimized, enc.encode_color_progressive_optimized_batch_async,
                                               enc.encode_ycbcr_progressive_optimized_batch_async)
        if progressive:
            cap = bound(w, h, sub)
        restart = None
        if a.restart is not None:                                # `row`: ceil(W / 8) MCUs at 4:4:4, ceil(W / 16) otherwise
            restart = -(-w // (8 if sub == jpegamd.SUBSAMPLE_444 else 16)) if a.restart == "row" else int(a.restart)
            cap = jpegamd.max_jfif_bytes_interleaved_restart(w, h, sub, restart)
        cap += a.metadata_bytes
        outs = [torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(n)]
        sizes = torch.zeros(n, dtype=torch.int64, device=dev)
        out_ptrs = [o.data_ptr() for o in outs]
        size_ptrs = [sizes.data_ptr() + 8 * i for i in range(n)]
        if progressive and ycc is None:
            entry = color_entry
            call = lambda: entry(descs, sub, out_ptrs, cap, size_ptrs, stream)
        elif progressive:
            fmt = {"p010": jpegamd.SAMPLES_10_MSB, "i010": jpegamd.SAMPLES_10_LSB}.get(source, jpegamd.SAMPLES_8)
            entry = ycbcr_entry
            call = lambda: entry(
                ycc, sub, jpegamd.RANGE_LIMITED if limited else jpegamd.RANGE_FULL, fmt, jpegamd.MATRIX_BT709 if bt709 else jpegamd.MATRIX_BT601,
                out_ptrs, cap, size_ptrs, stream)
        elif one_scan and ycc is not None and (limited or bt709 or source in ("yuyv", "p010", "i010")):     # a kind the older one-scan entries refuse
            fmt = {"p010": jpegamd.SAMPLES_10_MSB, "i010": jpegamd.SAMPLES_10_LSB}.get(source, jpegamd.SAMPLES_8)
            call = lambda: enc.encode_ycbcr_interleaved_matrix_batch_async(
                ycc, sub, jpegamd.RANGE_LIMITED if limited else jpegamd.RANGE_FULL, fmt, jpegamd.MATRIX_BT709 if bt709 else jpegamd.MATRIX_BT601,
                restart or 0, out_ptrs, cap, size_ptrs, stream)
        elif restart is not None and ycc is None:
            call = lambda: enc.encode_color_interleaved_restart_batch_async(descs, sub, restart, out_ptrs, cap, size_ptrs, stream)
        elif restart is not None:
            call = lambda: enc.encode_ycbcr_interleaved_restart_batch_async(ycc, sub, restart, out_ptrs, cap, size_ptrs, stream)
        elif one_scan and ycc is None:
            call = lambda: enc.encode_color_interleaved_batch_async(descs, sub, out_ptrs, cap, size_ptrs, stream)
        elif one_scan:
            call = lambda: enc.encode_ycbcr_interleaved_batch_async(ycc, sub, out_ptrs, cap, size_ptrs, stream)
        elif ycc is None:
            call = lambda: enc.encode_color_batch_async(descs, sub, out_ptrs, cap, size_ptrs, stream)
        else:
            kw = {"sample_range": jpegamd.RANGE_LIMITED} if limited else {}
            if source in ("p010", "i010"):
                kw["sample_format"] = jpegamd.SAMPLES_10_MSB if source == "p010" else jpegamd.SAMPLES_10_LSB
            if bt709:
                kw["matrix"] = jpegamd.MATRIX_BT709
            call = lambda: enc.encode_ycbcr_batch_async(ycc, sub, out_ptrs, cap, size_ptrs, stream, **kw)
        def timed():
            for _ in range(a.warmup):
                call()
            enc.finish()
            enc.set_profiling(a.steps)
            for _ in range(a.steps):
                call()
            st = enc.finish()
            totals = [enc.profile(i).ns_total for i in range(a.steps)]
            enc.set_profiling(0)
            return statistics.median(totals), st

        t, st = timed()
        line = {"source": source, "subsampling": name, "width": w, "height": h, "batch": n, "quality": a.quality, "kind": a.kind,
                "steps": a.steps, "bytes": sizes.cpu().tolist(), "entropy_bits": st.entropy_bits,
                "ns_total_median": int(t), "us_per_picture": round(t / n / 1000, 1),
                "gpixels_per_s": round(n * w * h / t, 2)}
        line.update(without_metadata(a, enc, lambda: timed()[0])(t))
        if one_scan or progressive:
            line["scan"] = a.scan
        if a.huffman is not None:
            line["huffman"] = a.huffman
        if a.successive:
            line["successive"] = True
        if restart is not None:
            line["restart_interval"] = restart
        if limited:
            line["range"] = "limited"
        if a.mapped:
            line["range"] = "limited, mapped outside the timed loop"
        if bt709 and ycc is not None:
            line["matrix"] = "bt709"
            line["pass_bytes_per_picture"] = pass_bytes(w, h, sub, jpegamd, 2 if source in ("p010", "i010") else 1)
            if a.convert:
                line.update(time_matrix_convert(a, jpegamd, torch, enc, source, tensors, (lut_y, lut_c), h, sub, out_ptrs, cap, size_ptrs,
                                                sizes, stream, n))
            report(a, line)
            del outs
            continue
        if a.narrow and source in ("p010", "i010"):
            line.update(time_narrow(a, jpegamd, torch, enc, source, tensors, h, sub, out_ptrs, cap, size_ptrs, sizes, stream, n))
        if a.convert and source not in ("p010", "i010"):
            line.update(time_convert(a, jpegamd, torch, enc, source, tensors, describe, (lut_y, lut_c), h, sub, out_ptrs, cap, size_ptrs,
                                     sizes, stream, n))
        report(a, line)
        del outs


def time_convert(a, jpegamd, torch, enc, source, tensors, describe, luts, h, sub, out_ptrs, cap, size_ptrs, sizes, stream, n):
    """What expanding on read replaces: the range map as a pass over the source's planes into planes of the same shape (one call's
    worth, between two events on the stream), then the full-range encode of those."""
    lut_y, lut_c = luts
    limited_bytes = sizes.cpu().tolist()
    mapped = tuple(torch.empty_like(t) for t in tensors)

    def convert():
        if source == "yuyv":                                     # [N, H, W, 2]: Y in byte 0 of a pixel, Cb / Cr in byte 1
            mapped[0][..., 0] = lut_y[tensors[0][..., 0].long()]
            mapped[0][..., 1] = lut_c[tensors[0][..., 1].long()]
        elif source == "nv12":                                   # [N, 3 H / 2, W]: H rows of Y, then the Cb Cr pairs
            mapped[0][:, :h] = lut_y[tensors[0][:, :h].long()]
            mapped[0][:, h:] = lut_c[tensors[0][:, h:].long()]
        else:                                                    # three planes (i420: the Y rows of the frames)
            rows = h if source == "i420" else tensors[0].shape[1]
            mapped[0][:, :rows] = lut_y[tensors[0][:, :rows].long()]
            mapped[1][:] = lut_c[tensors[1].long()]
            mapped[2][:] = lut_c[tensors[2].long()]

    for _ in range(2):
        convert()
    torch.cuda.synchronize()
    times = []
    for _ in range(max(3, a.steps // 5)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        convert()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1000.0 / n)
    ycc = describe(mapped)
    call = lambda: enc.encode_ycbcr_batch_async(ycc, sub, out_ptrs, cap, size_ptrs, stream)
    for _ in range(a.warmup):
        call()
    enc.finish()
    enc.set_profiling(a.steps)
    for _ in range(a.steps):
        call()
    enc.finish()
    t = statistics.median(enc.profile(i).ns_total for i in range(a.steps))
    enc.set_profiling(0)
    return {"convert_us_per_picture": round(statistics.median(times), 1), "mapped_full_us_per_picture": round(t / n / 1000, 1),
            "mapped_bytes_equal": sizes.cpu().tolist() == limited_bytes}


def pass_bytes(w, h, sub, jpegamd, sample_bytes):
    """What k_ycbcr_matrix_batch moves for one picture: every stored sample read once, every 8-bit sample of the three planes written once."""
    cw = w if sub == jpegamd.SUBSAMPLE_444 else (w + 1) // 2
    ch = (h + 1) // 2 if sub == jpegamd.SUBSAMPLE_420 else h
    samples = w * h + 2 * cw * ch
    return samples * sample_bytes + samples


def time_matrix_convert(a, jpegamd, torch, enc, source, tensors, luts, h, sub, out_ptrs, cap, size_ptrs, sizes, stream, n):
    """What the BT.709 entry replaces at 4:2:0: the definition of include/jpeg_compression.h in torch integer ops over the source's planes
    (the depth / range map first) into preallocated 8-bit planes, one call's worth between two events on the stream, then the plain
    encode of those planes."""
    w = a.size
    lut_y, lut_c = luts if a.sample_range == "limited" else (None, None)
    direct_bytes = sizes.cpu().tolist()
    out_y = torch.empty((n, h, w), dtype=torch.uint8, device=tensors[0].device)
    out_cb, out_cr = (torch.empty((n, h // 2, w // 2), dtype=torch.uint8, device=tensors[0].device) for _ in range(2))
    c = (1664, 3213, 16218, -1813, -1187, 16112)

    def to8(t, lut, shift):
        """Stored samples -> int32 full-range 8-bit values (the bench's words hold s << 8 or s << 2: at full range the shift is exact)."""
        v = (t.to(torch.int32) >> shift) & 0xFF if shift else t.to(torch.int32)
        return lut[v.long()].to(torch.int32) if lut is not None else v

    def convert():
        if source in ("nv12", "p010"):                           # [N, 3 H / 2, W]: H rows of Y, then the Cb Cr pairs
            shift = 8 if source == "p010" else 0
            y = to8(tensors[0][:, :h], lut_y, shift)
            pairs = to8(tensors[0][:, h:], lut_c, shift).view(n, h // 2, w // 2, 2)
            b, r = pairs[..., 0] - 128, pairs[..., 1] - 128
        else:                                                    # three planes (i420: the Y rows of the frames)
            shift = 2 if source == "i010" else 0
            y = to8(tensors[0][:, :h], lut_y, shift)
            b, r = to8(tensors[1], lut_c, shift) - 128, to8(tensors[2], lut_c, shift) - 128
        ty = (c[0] * b + c[1] * r + 8192) >> 14
        out_y.copy_((y + ty.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)).clamp_(0, 255))
        out_cb.copy_((128 + ((c[2] * b + c[3] * r + 8192) >> 14)).clamp_(0, 255))
        out_cr.copy_((128 + ((c[4] * b + c[5] * r + 8192) >> 14)).clamp_(0, 255))

    for _ in range(2):
        convert()
    torch.cuda.synchronize()
    times = []
    for _ in range(max(3, a.steps // 5)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        convert()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1000.0 / n)
    ycc = [jpegamd.Encoder.ycbcr_image(out_y[i].data_ptr(), out_cb[i].data_ptr(), out_cr[i].data_ptr(), w, h, w, w // 2,
                                       jpegamd.CHROMA_PLANES, a.quality) for i in range(n)]
    call = lambda: enc.encode_ycbcr_batch_async(ycc, sub, out_ptrs, cap, size_ptrs, stream)
    for _ in range(a.warmup):
        call()
    enc.finish()
    enc.set_profiling(a.steps)
    for _ in range(a.steps):
        call()
    enc.finish()
    t = statistics.median(enc.profile(i).ns_total for i in range(a.steps))
    enc.set_profiling(0)
    return {"convert_us_per_picture": round(statistics.median(times), 1), "converted_plain_us_per_picture": round(t / n / 1000, 1),
            "converted_bytes_equal": sizes.cpu().tolist() == direct_bytes}


def time_narrow(a, jpegamd, torch, enc, source, tensors, h, sub, out_ptrs, cap, size_ptrs, sizes, stream, n):
    """What narrowing on read replaces: a pass over the source's planes that reads the 16-bit words and writes bytes into planes of
    the same shape (one call's worth, between two events on the stream), then the 8-bit encode of those at the same range."""
    w = a.size
    direct_bytes = sizes.cpu().tolist()
    narrowed = tuple(torch.empty(t.shape, dtype=torch.uint8, device=t.device) for t in tensors)

    def narrow():
        if source == "p010":                                     # the high byte of every word: ONE strided copy
            narrowed[0].copy_(tensors[0].view(torch.uint8).view(*tensors[0].shape, 2)[..., 1])
        else:                                                    # the value in the low ten bits: v >> 2
            for dst, src in zip(narrowed, tensors):
                dst.copy_(src >> 2)

    for _ in range(2):
        narrow()
    torch.cuda.synchronize()
    times = []
    for _ in range(max(3, a.steps // 5)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        narrow()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1000.0 / n)
    if source == "p010":
        ycc = [jpegamd.Encoder.ycbcr_image(narrowed[0][i].data_ptr(), narrowed[0][i, h:].data_ptr(), 0, w, h, w, w, jpegamd.CHROMA_CBCR,
                                           a.quality) for i in range(n)]
    else:
        ycc = [jpegamd.Encoder.ycbcr_image(narrowed[0][i].data_ptr(), narrowed[1][i].data_ptr(), narrowed[2][i].data_ptr(), w, h, w, w // 2,
                                           jpegamd.CHROMA_PLANES, a.quality) for i in range(n)]
    kw = {"sample_range": jpegamd.RANGE_LIMITED} if a.sample_range == "limited" else {}
    call = lambda: enc.encode_ycbcr_batch_async(ycc, sub, out_ptrs, cap, size_ptrs, stream, **kw)
    for _ in range(a.warmup):
        call()
    enc.finish()
    enc.set_profiling(a.steps)
    for _ in range(a.steps):
        call()
    enc.finish()
    t = statistics.median(enc.profile(i).ns_total for i in range(a.steps))
    enc.set_profiling(0)
    return {"narrow_us_per_picture": round(statistics.median(times), 1), "narrowed_8bit_us_per_picture": round(t / n / 1000, 1),
            "narrowed_bytes_equal": sizes.cpu().tolist() == direct_bytes}


def run_layout(a, jpegamd, torch, dev) -> None:
    w = h = a.size
    n = a.batch or 8
    sub = jpegamd.SUBSAMPLE_420
    pics = []
    for i in range(n):
        bmp = jpegamd.synth_bmp(w, h, 1 + i, a.kind, 0)
        img, off = jpegamd.parse_bmp(bmp)
        rows = torch.frombuffer(bytearray(bmp[off:off + img.row_stride * h]), dtype=torch.uint8).to(dev).view(h, img.row_stride)
        pics.append(rows[:, :3 * w].reshape(h, w, 3).flip(0).flip(2))       # bottom-up B, G, R -> top-down R, G, B
        del bmp, rows
    hwc = torch.stack(pics)
    del pics
    if a.layout == "chw":
        src = hwc.permute(0, 3, 1, 2).contiguous()
    elif a.layout == "rgba":
        src = torch.cat([hwc, torch.full_like(hwc[..., :1], 255)], dim=3)
    else:
        src = hwc
    if a.layout != "hwc" and not a.repack:
        del hwc
    enc = new_encoder(a, jpegamd, w, n * h)
    if a.huffman == "optimized":
        enc.set_huffman(jpegamd.HUFFMAN_OPTIMIZED)
    stream = torch.cuda.current_stream().cuda_stream
    one_scan = a.scan == "interleaved"
    restart = 0
    if a.restart is not None:
        restart = -(-w // 16) if a.restart == "row" else int(a.restart)
    cap = (jpegamd.max_jfif_bytes_interleaved_restart(w, h, sub, restart) if one_scan else jpegamd.max_jfif_bytes_color(w, h, sub)) + a.metadata_bytes
    outs = [torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(n)]
    sizes = torch.zeros(n, dtype=torch.int64, device=dev)
    out_ptrs = [o.data_ptr() for o in outs]
    size_ptrs = [sizes.data_ptr() + 8 * i for i in range(n)]

    def packed_descs(t, order, bpp):
        return [jpegamd.Encoder.image(t[i].data_ptr(), w, h, bpp * w, False, order, a.quality) for i in range(n)]

    if a.layout == "chw":
        planar = [jpegamd.Encoder.planar_image(tuple(src[i, k].data_ptr() for k in range(3)), w, h, w, False, a.quality) for i in range(n)]
        if one_scan:
            direct = lambda: enc.encode_planar_interleaved_batch_async(planar, sub, restart, out_ptrs, cap, size_ptrs, stream)
        else:
            direct = lambda: enc.encode_planar_batch_async(planar, sub, out_ptrs, cap, size_ptrs, stream)
    else:
        descs = packed_descs(src, jpegamd.ORDER_RGBA if a.layout == "rgba" else jpegamd.ORDER_RGB, 4 if a.layout == "rgba" else 3)
        if one_scan:
            direct = lambda: enc.encode_color_interleaved_pixels_batch_async(descs, sub, restart, out_ptrs, cap, size_ptrs, stream)
        else:
            direct = lambda: enc.encode_color_batch_async(descs, sub, out_ptrs, cap, size_ptrs, stream)
    routes = {"direct": direct}
    if a.repack and one_scan:
        sys.exit("--repack times a route of the three-scan path: not with --scan interleaved")
    if a.repack:
        if a.layout != "chw":
            sys.exit("--repack needs --layout chw")
        tmp = torch.empty_like(hwc)
        del hwc
        tmp_descs = packed_descs(tmp, jpegamd.ORDER_RGB, 3)

        def repack():
            tmp.copy_(src.permute(0, 2, 3, 1))
            enc.encode_color_batch_async(tmp_descs, sub, out_ptrs, cap, size_ptrs, stream)
        routes["repack"] = repack
    medians = {k: [] for k in routes}
    got = {}
    for k, call in routes.items():
        for _ in range(a.warmup):
            call()
        enc.finish()
        got[k] = sizes.cpu().tolist()
    for _ in range(a.rounds):
        for k, call in routes.items():                                      # the routes alternate: one thermal history
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
            for e0, e1 in evs:
                e0.record()
                call()
                e1.record()
            enc.finish()
            medians[k].append(statistics.median(e0.elapsed_time(e1) for e0, e1 in evs) * 1000.0 / n)
    for k in routes:
        m = medians[k]
        report(a, {"layout": a.layout, "route": k, "width": w, "height": h, "batch": n, "quality": a.quality, "kind": a.kind,
                    "steps": a.steps, "rounds": a.rounds, "bytes": got[k], "us_per_picture_medians": [round(v, 1) for v in m],
                    "us_per_picture": round(statistics.median(m), 1), "spread_us": round(max(m) - min(m), 1),
                    "gpixels_per_s": round(w * h / statistics.median(m) / 1000, 2),
                    **({"scan": "interleaved", "restart_interval": restart} if one_scan else {}),
                    **({"huffman": a.huffman} if a.huffman is not None else {})})


FLOAT_SOURCES = ("float32", "float16", "bfloat16")


def run_float(a, jpegamd, torch, dev, source) -> None:
    """--source float32|float16|bfloat16: N float pictures in [0, 1] per call, stored as --layout chw (default) or hwc, through the float
    entries.  Three routes alternate in one run, each call timed as a whole between two events on the stream:
    `float` the float entry; `convert` what a caller does without it -- x.mul(255).round().clamp(0, 255).to(uint8), then the uint8 entry
    of the same layout, as one unit --; `uint8` that entry alone on bytes quantised beforehand, the floor the float call approaches
    from above; and `copy`, a device-to-device copy that moves as many bytes as k_float_planes_batch reads and writes, the yardstick
    for that kernel's own time in a kernel trace of the same command."""
    w = h = a.size
    n = a.batch or 8
    layout = a.layout or "chw"
    if layout not in ("chw", "hwc"):
        sys.exit("--source float32|float16|bfloat16 takes --layout chw or hwc")
    dtype = getattr(torch, source)
    sample_type = {"float32": jpegamd.FLOAT_F32, "float16": jpegamd.FLOAT_F16, "bfloat16": jpegamd.FLOAT_BF16}[source]
    size = 4 if source == "float32" else 2
    gray = a.scan == "gray"
    subs = [(0, "gray")] if gray else [s for s in rgb_subsamplings(a, jpegamd)]
    pics = []
    for i in range(n):
        bmp = jpegamd.synth_bmp(w, h, 1 + i, a.kind, 0)
        img, off = jpegamd.parse_bmp(bmp)
        rows = torch.frombuffer(bytearray(bmp[off:off + img.row_stride * h]), dtype=torch.uint8).to(dev).view(h, img.row_stride)
        pics.append(rows[:, :3 * w].reshape(h, w, 3).flip(0).flip(2))       # bottom-up B, G, R -> top-down R, G, B
        del bmp, rows
    hwc8 = torch.stack(pics)
    del pics
    src8 = hwc8.permute(0, 3, 1, 2).contiguous() if layout == "chw" else hwc8
    del hwc8
    src = src8.to(torch.float32).div(255.0).to(dtype)                       # the float pictures
    q8 = src.mul(255).round().clamp(0, 255).to(torch.uint8)                 # their bytes (bfloat16 does not hold every k / 255)
    del src8
    enc = new_encoder(a, jpegamd, w, n * h)
    if a.huffman == "optimized":
        enc.set_huffman(jpegamd.HUFFMAN_OPTIMIZED)
    stream = torch.cuda.current_stream().cuda_stream
    restart = 0
    if a.restart is not None:
        restart = -(-w // (8 if gray else 16)) if a.restart == "row" else int(a.restart)
    if layout == "chw":
        images = lambda t, sz: [jpegamd.Encoder.float_image(tuple(t[i, k].data_ptr() for k in range(3)), w, h, sz * w, sz, a.quality) for i in range(n)]
    else:
        images = lambda t, sz: [jpegamd.Encoder.float_image(tuple(t[i].data_ptr() + sz * k for k in range(3)), w, h, 3 * sz * w, 3 * sz, a.quality)
                                for i in range(n)]
    fimgs = images(src, size)
    for sub, name in subs:
        if a.scan == "progressive":
            cap = jpegamd.max_jfif_bytes_progressive_script(w, h, sub, None)
        elif gray:
            cap = max(jpegamd.max_jfif_bytes_gray_scan(w, h, restart), jpegamd.max_jfif_bytes(w, h))
        elif a.scan == "interleaved":
            cap = jpegamd.max_jfif_bytes_interleaved_restart(w, h, sub, restart)
        else:
            cap = jpegamd.max_jfif_bytes_color(w, h, sub)
        cap += a.metadata_bytes
        outs = [torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(n)]
        sizes = torch.zeros(n, dtype=torch.int64, device=dev)
        tail = ([o.data_ptr() for o in outs], cap, [sizes.data_ptr() + 8 * i for i in range(n)], stream)

        def float_call():
            if a.scan == "progressive":
                enc.encode_float_progressive_script_batch_async(fimgs, sub, sample_type, 255.0, 0.0, None, *tail)
            elif a.scan in ("interleaved", "gray"):
                enc.encode_float_interleaved_batch_async(fimgs, sub, sample_type, 255.0, 0.0, restart, *tail)
            else:
                enc.encode_float_batch_async(fimgs, sub, sample_type, 255.0, 0.0, *tail)

        def uint8_entry(t):
            """The uint8 entry of the same layout and file on the bytes `t`, or None where no entry reads that layout."""
            if layout == "chw":
                planar = [jpegamd.Encoder.planar_image(tuple(t[i, k].data_ptr() for k in range(3)), w, h, w, False, a.quality) for i in range(n)]
                if a.scan == "separate":
                    return lambda: enc.encode_planar_batch_async(planar, sub, *tail)
                if a.scan == "interleaved":
                    return lambda: enc.encode_planar_interleaved_batch_async(planar, sub, restart, *tail)
                if gray and restart == 0 and a.huffman != "optimized":
                    return lambda: enc.encode_planar_batch_async(planar, 0, *tail)
                return None
            descs = [jpegamd.Encoder.image(t[i].data_ptr(), w, h, 3 * w, False, jpegamd.ORDER_RGB, a.quality) for i in range(n)]
            if a.scan == "separate":
                return lambda: enc.encode_color_batch_async(descs, sub, *tail)
            if a.scan == "interleaved":
                return lambda: enc.encode_color_interleaved_pixels_batch_async(descs, sub, restart, *tail)
            if gray:
                return lambda: enc.encode_gray_scan_batch_async(descs, restart, *tail)
            return lambda: enc.encode_color_progressive_script_batch_async(descs, sub, None, *tail)

        routes = {"float": float_call}
        plain = uint8_entry(q8)
        if plain is not None:
            routes["uint8"] = plain

            def convert():
                t = src.mul(255).round().clamp(0, 255).to(torch.uint8)
                uint8_entry(t)()
                return t                                                    # (alive until the next call has been queued)
            routes["convert"] = convert
        # what the front pass moves: every sample in, the planes out
        cw, ch = (w if sub == jpegamd.SUBSAMPLE_444 else (w + 1) // 2), ((h + 1) // 2 if sub == jpegamd.SUBSAMPLE_420 else h)
        pass_bytes = n * (3 * w * h * size + w * h + (2 * cw * ch if sub else 0))
        half = torch.empty(pass_bytes // 2, dtype=torch.uint8, device=dev)
        other = torch.empty_like(half)
        routes["copy"] = lambda: other.copy_(half)
        medians = {k: [] for k in routes}
        got = {}
        for k, call in routes.items():
            for _ in range(a.warmup):
                call()
            wait = torch.cuda.synchronize if k == "copy" else enc.finish    # (a context with nothing queued has nothing to finish)
            wait()
            got[k] = sizes.cpu().tolist()
        for _ in range(a.rounds):
            for k, call in routes.items():                                  # the routes alternate: one thermal history
                evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
                keep = None
                for e0, e1 in evs:
                    e0.record()
                    keep = call()
                    e1.record()
                if k != "copy":
                    enc.finish()
                torch.cuda.synchronize()
                del keep
                medians[k].append(statistics.median(e0.elapsed_time(e1) for e0, e1 in evs) * 1000.0 / n)
        for k in routes:
            m = medians[k]
            line = {"source": source, "layout": layout, "scan": a.scan, "subsampling": name, "route": k, "width": w, "height": h, "batch": n,
                    "quality": a.quality, "kind": a.kind, "steps": a.steps, "rounds": a.rounds,
                    "us_per_picture_medians": [round(v, 1) for v in m], "us_per_picture": round(statistics.median(m), 1),
                    "spread_us": round(max(m) - min(m), 1)}
            if k == "copy":
                line.update(pass_bytes_per_picture=pass_bytes // n, copy_gb_per_s=round(pass_bytes / n / statistics.median(m) / 1000, 1))
            else:
                line.update(bytes=got[k], gpixels_per_s=round(w * h / statistics.median(m) / 1000, 2),
                            ratio_to_float=round(statistics.median(m) / statistics.median(medians["float"]), 3))
            if a.scan in ("interleaved", "gray"):
                line.update(restart_interval=restart, huffman=a.huffman or "standard")
            report(a, line)
        del outs, half, other


def run_reduce(a, jpegamd, torch, dev) -> None:
    """--reduce F: N uint8 pictures per call, stored as --layout chw (default) or hwc, each encoded reduced by F both ways through the
    reduced entries.  Four routes alternate in one run, each call timed as a whole between two events on the stream:
    `reduced` the reduced entry; `resize` what a caller does without it -- a float copy, avg_pool2d(ceil_mode=True, divisor_override=1),
    the division by the box counts, + 0.5, floor, clamp and the cast, then the planar uint8 entry, as one unit --; `uint8` the uint8 entry
    of the same layout alone on bytes reduced beforehand, the floor the reduced call approaches from above; and `copy`, a device-to-device
    copy of as many bytes as the source holds, the yardstick for k_reduce_planes_batch's own time in a kernel trace of the same command.
    --resize WxH: the same four routes around the resized entries; the front route is named `resized`, and the
    caller's route is F.interpolate(mode="area") in place of the pooling."""
    import torch.nn.functional as F
    w = h = a.size
    f = a.reduce
    ow, oh = a.resize if a.resize else jpegamd.reduced_size(w, h, f)
    front = "resized" if a.resize else "reduced"
    n = a.batch or 8
    layout = a.layout or "chw"
    if layout not in ("chw", "hwc"):
        sys.exit("--reduce takes --layout chw or hwc")
    gray = a.scan == "gray"
    subs = [(0, "gray")] if gray else [s for s in rgb_subsamplings(a, jpegamd)]
    pics = []
    for i in range(n):
        bmp = jpegamd.synth_bmp(w, h, 1 + i, a.kind, 0)
        img, off = jpegamd.parse_bmp(bmp)
        rows = torch.frombuffer(bytearray(bmp[off:off + img.row_stride * h]), dtype=torch.uint8).to(dev).view(h, img.row_stride)
        pics.append(rows[:, :3 * w].reshape(h, w, 3).flip(0).flip(2))       # bottom-up B, G, R -> top-down R, G, B
        del bmp, rows
    hwc8 = torch.stack(pics)
    del pics
    src = hwc8.permute(0, 3, 1, 2).contiguous() if layout == "chw" else hwc8
    del hwc8
    # the box counts of the map, and the caller's route with them
    if not a.resize:
        nx = torch.clamp(w - f * torch.arange(ow, device=dev), max=f)
        ny = torch.clamp(h - f * torch.arange(oh, device=dev), max=f)
        inv = 1.0 / (ny[:, None] * nx[None, :]).to(torch.float32)

    def resized():
        x = (src if layout == "chw" else src.permute(0, 3, 1, 2)).to(torch.float32, memory_format=torch.contiguous_format)
        if a.resize:
            return F.interpolate(x, size=(oh, ow), mode="area").add(0.5).floor().clamp(0, 255).to(torch.uint8)
        return F.avg_pool2d(x, f, ceil_mode=True, divisor_override=1).mul(inv).add(0.5).floor().clamp(0, 255).to(torch.uint8)

    small_chw = resized()                                                  # [N, 3, oh, ow]
    small = small_chw if layout == "chw" else small_chw.permute(0, 2, 3, 1).contiguous()
    enc = new_encoder(a, jpegamd, ow, n * ((oh + 7) // 8 * 8))
    if a.huffman == "optimized":
        enc.set_huffman(jpegamd.HUFFMAN_OPTIMIZED)
    stream = torch.cuda.current_stream().cuda_stream
    restart = 0
    if a.restart is not None:
        restart = -(-ow // (8 if gray else 16)) if a.restart == "row" else int(a.restart)
    if layout == "chw":
        rimgs = [jpegamd.Encoder.strided_image(tuple(src[i, k].data_ptr() for k in range(3)), w, h, w, 1, a.quality) for i in range(n)]
    else:
        rimgs = [jpegamd.Encoder.strided_image(tuple(src[i].data_ptr() + k for k in range(3)), w, h, 3 * w, 3, a.quality) for i in range(n)]
    for sub, name in subs:
        if a.scan == "progressive":
            cap = jpegamd.max_jfif_bytes_progressive_script(ow, oh, sub, None)
        elif gray:
            cap = max(jpegamd.max_jfif_bytes_gray_scan(ow, oh, restart), jpegamd.max_jfif_bytes(ow, oh))
        elif a.scan == "interleaved":
            cap = jpegamd.max_jfif_bytes_interleaved_restart(ow, oh, sub, restart)
        else:
            cap = jpegamd.max_jfif_bytes_color(ow, oh, sub)
        cap += a.metadata_bytes
        outs = [torch.empty(cap, dtype=torch.uint8, device=dev) for _ in range(n)]
        sizes = torch.zeros(n, dtype=torch.int64, device=dev)
        tail = ([o.data_ptr() for o in outs], cap, [sizes.data_ptr() + 8 * i for i in range(n)], stream)

        def reduced_call():
            if a.resize:
                if a.scan == "progressive":
                    enc.encode_resized_progressive_script_batch_async(rimgs, sub, ow, oh, None, *tail)
                elif a.scan in ("interleaved", "gray"):
                    enc.encode_resized_interleaved_batch_async(rimgs, sub, ow, oh, restart, *tail)
                else:
                    enc.encode_resized_batch_async(rimgs, sub, ow, oh, *tail)
            elif a.scan == "progressive":
                enc.encode_reduced_progressive_script_batch_async(rimgs, sub, f, None, *tail)
            elif a.scan in ("interleaved", "gray"):
                enc.encode_reduced_interleaved_batch_async(rimgs, sub, f, restart, *tail)
            else:
                enc.encode_reduced_batch_async(rimgs, sub, f, *tail)

        def uint8_entry(t, lay):
            """The uint8 entry of the same file on the reduced bytes `t` stored as `lay`, or None where no entry reads that layout."""
            if lay == "chw":
                planar = [jpegamd.Encoder.planar_image(tuple(t[i, k].data_ptr() for k in range(3)), ow, oh, ow, False, a.quality) for i in range(n)]
                if a.scan == "separate":
                    return lambda: enc.encode_planar_batch_async(planar, sub, *tail)
                if a.scan == "interleaved":
                    return lambda: enc.encode_planar_interleaved_batch_async(planar, sub, restart, *tail)
                if gray and restart == 0 and a.huffman != "optimized":
                    return lambda: enc.encode_planar_batch_async(planar, 0, *tail)
                return None
            descs = [jpegamd.Encoder.image(t[i].data_ptr(), ow, oh, 3 * ow, False, jpegamd.ORDER_RGB, a.quality) for i in range(n)]
            if a.scan == "separate":
                return lambda: enc.encode_color_batch_async(descs, sub, *tail)
            if a.scan == "interleaved":
                return lambda: enc.encode_color_interleaved_pixels_batch_async(descs, sub, restart, *tail)
            if gray:
                return lambda: enc.encode_gray_scan_batch_async(descs, restart, *tail)
            return lambda: enc.encode_color_progressive_script_batch_async(descs, sub, None, *tail)

        routes = {front: reduced_call}
        plain = uint8_entry(small, layout)
        if plain is not None:
            routes["uint8"] = plain
        if uint8_entry(small_chw, "chw") is not None:
            def resize():
                t = resized()
                uint8_entry(t, "chw")()
                return t                                                    # (alive until the next call has been queued)
            routes["resize"] = resize
        other = torch.empty_like(src)
        routes["copy"] = lambda: other.copy_(src)
        medians = {k: [] for k in routes}
        got = {}
        for k, call in routes.items():
            for _ in range(a.warmup):
                call()
            wait = torch.cuda.synchronize if k == "copy" else enc.finish    # (a context with nothing queued has nothing to finish)
            wait()
            got[k] = sizes.cpu().tolist()
        for _ in range(a.rounds):
            for k, call in routes.items():                                  # the routes alternate: one thermal history
                evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.steps)]
                keep = None
                for e0, e1 in evs:
                    e0.record()
                    keep = call()
                    e1.record()
                if k != "copy":
                    enc.finish()
                torch.cuda.synchronize()
                del keep
                medians[k].append(statistics.median(e0.elapsed_time(e1) for e0, e1 in evs) * 1000.0 / n)
        for k in routes:
            m = medians[k]
            line = {"source": "uint8", **({"resize": f"{ow}x{oh}"} if a.resize else {"reduce": f}), "layout": layout, "scan": a.scan, "subsampling": name, "route": k, "width": w, "height": h,
                    "reduced_width": ow, "reduced_height": oh, "batch": n, "quality": a.quality, "kind": a.kind, "steps": a.steps,
                    "rounds": a.rounds, "us_per_picture_medians": [round(v, 1) for v in m], "us_per_picture": round(statistics.median(m), 1),
                    "spread_us": round(max(m) - min(m), 1)}
            if k == "copy":
                line.update(source_bytes_per_picture=src.numel() // n, copy_gb_per_s=round(2 * src.numel() / n / statistics.median(m) / 1000, 1))
            else:
                line.update(bytes=got[k], source_gpixels_per_s=round(w * h / statistics.median(m) / 1000, 2),
                            **{f"ratio_to_{front}": round(statistics.median(m) / statistics.median(medians[front]), 3),
                               f"same_sizes_as_{front}": got[k] == got[front]})     # (torch divides in float32: exact where n is a power of 2)
            if a.scan in ("interleaved", "gray"):
                line.update(restart_interval=restart, huffman=a.huffman or "standard")
            report(a, line)
        del outs, other


if __name__ == "__main__":
    main()
