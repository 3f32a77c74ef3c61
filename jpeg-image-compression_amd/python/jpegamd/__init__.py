"""ctypes binding of libjpegamd.so (include/jpeg_compression.h).

This is plumbing for tests, bench.py and __graft_entry__: every compute call goes through
the C-ABI into the HIP kernels.  There is no Python or CPU implementation of the codec
here; if the shared library is missing the import fails loudly.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
import threading
from pathlib import Path

_PKG_ROOT = Path(__file__).resolve().parents[2]          # .../jpeg-image-compression_amd
# JPEGAMD_LIB: A/B tooling only (tools/gpu_*.sh point it at a variant build of the same library)
LIB_PATH = Path(os.environ.get("JPEGAMD_LIB") or (_PKG_ROOT / "libjpegamd.so"))
HEADER_PATH = _PKG_ROOT.parent / "include" / "jpeg_compression.h"

ORDER_BGR, ORDER_RGB, ORDER_GRAY = 0, 1, 2                  # JPEGAMD_ORDER_* (GRAY: one byte per pixel, the luma itself)
ORDER_RGBA, ORDER_BGRA = 3, 4                                # four bytes per pixel, the fourth ignored
SUBSAMPLE_444, SUBSAMPLE_420, SUBSAMPLE_422 = 1, 2, 4        # JPEGAMD_SUBSAMPLE_* (colour files; 3 stays an invalid value)
JFIF_PREFIX_BYTES = 328

ERR_NAMES = {0: "OK", -1: "ERR_ARG", -2: "ERR_NO_DEVICE", -3: "ERR_HIP", -4: "ERR_NOT_INIT", -5: "ERR_TOO_LARGE",
             -6: "ERR_RLE_CAPACITY", -7: "ERR_BMP", -8: "ERR_HUFF_CAPACITY"}


class JpegAmdError(RuntimeError):
    def __init__(self, code: int, what: str):
        super().__init__(f"{what}: {ERR_NAMES.get(code, code)} ({code})")
        self.code = code


class Image(C.Structure):
    _fields_ = [("pixels", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("row_stride", C.c_int32),
                ("bottom_up", C.c_int32), ("channel_order", C.c_int32), ("quality", C.c_int32)]


class PlanarImage(C.Structure):
    """JpegAmdPlanarImage: the R, G and B planes of one picture (device pointers), one byte per sample."""
    _fields_ = [("plane", C.c_void_p * 3), ("width", C.c_int32), ("height", C.c_int32), ("row_stride", C.c_int32),
                ("bottom_up", C.c_int32), ("quality", C.c_int32)]


CHROMA_PLANES, CHROMA_CBCR, CHROMA_CRCB = 0, 1, 2           # JPEGAMD_CHROMA_*
CHROMA_YUYV, CHROMA_UYVY = 4, 5                             # packed 4:2:2: the picture's y is the packed plane (3 stays invalid)
RANGE_FULL, RANGE_LIMITED = 0, 1                            # JPEGAMD_RANGE_*: JFIF full range / video range (Y 16..235, Cb Cr 16..240), expanded on read
MATRIX_BT601, MATRIX_BT709 = 0, 1                           # JPEGAMD_MATRIX_*: the samples' YCbCr matrix: JFIF's own / BT.709 (HD, UHD video), converted by one pass
SAMPLES_8, SAMPLES_10_MSB, SAMPLES_10_LSB = 0, 1, 2         # JPEGAMD_SAMPLES_*: one byte per sample / 10 bits in 16-bit words, high bits (P010) or low bits (I010), narrowed on read


class YCbCrImage(C.Structure):
    """JpegAmdYCbCrImage: the Y plane and the chroma of one picture (device pointers), JFIF full-range samples."""
    _fields_ = [("y", C.c_void_p), ("cb", C.c_void_p), ("cr", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32),
                ("y_stride", C.c_int32), ("c_stride", C.c_int32), ("chroma_layout", C.c_int32), ("quality", C.c_int32)]


FLOAT_F32, FLOAT_F16, FLOAT_BF16 = 0, 1, 2                   # JPEGAMD_FLOAT_*: the sample type of a float picture


class FloatImage(C.Structure):
    """JpegAmdFloatImage: the R, G and B samples of one float picture (device pointers to the first sample of each; plane[1] and
    plane[2] null: one channel, the luma), strides in bytes."""
    _fields_ = [("plane", C.c_void_p * 3), ("width", C.c_int32), ("height", C.c_int32), ("row_stride", C.c_int32),
                ("pixel_stride", C.c_int32), ("quality", C.c_int32)]


MAX_REDUCE = 8                                               # JPEGAMD_MAX_REDUCE: the largest factor of a reduced picture


class StridedImage(C.Structure):
    """JpegAmdStridedImage: the R, G and B BYTES of one picture to be reduced (device pointers to the first byte of each; plane[1] and
    plane[2] null: one channel, the luma), width and height of the SOURCE, strides in bytes."""
    _fields_ = FloatImage._fields_


class Stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("jfif_bytes", "entropy_bits", "stuffed_bytes", "exact_fallbacks",
                                          "ns_transform", "ns_entropy", "ns_pack", "ns_total")]


class DTO(C.Structure):
    """JPEG_COMPRESSION_DTO (dsp_port/jpeg_compression/include/jpeg_compression.h:32-64 + MI355X fields)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("r_phy_ptr", C.c_uint64), ("gb_phy_ptr", C.c_uint64),
                ("y_phy_ptr", C.c_uint64), ("dct_phy_ptr", C.c_uint64), ("quant_phy_ptr", C.c_uint64),
                ("zigzag_phy_ptr", C.c_uint64), ("rle_phy_ptr", C.c_uint64), ("rle_count", C.c_uint32),
                ("huff_phy_ptr", C.c_uint64), ("huff_size", C.c_uint32),
                ("cycles_color_conversion", C.c_uint64), ("cycles_dct", C.c_uint64),
                ("cycles_quantization", C.c_uint64), ("cycles_zigzag", C.c_uint64), ("cycles_rle", C.c_uint64),
                ("cycles_huffman", C.c_uint64), ("cycles_total", C.c_uint64),
                ("row_stride", C.c_int32), ("bottom_up", C.c_int32), ("channel_order", C.c_int32),
                ("quality", C.c_int32)]


class BMPImage(C.Structure):
    """natural_c/include/bmp_handler.h:37-41"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("data", C.POINTER(C.c_uint8))]


class BatchStats(C.Structure):
    _fields_ = [("files_ok", C.c_int32), ("files_failed", C.c_int32), ("bytes_in", C.c_uint64), ("bytes_out", C.c_uint64),
                ("seconds_total", C.c_double), ("seconds_read", C.c_double), ("seconds_write", C.c_double)]


class Segment(C.Structure):
    """JpegAmdSegment: a marker segment of the caller's (0xE1 .. 0xEF, 0xFE) and its payload."""
    _fields_ = [("marker", C.c_int32), ("data", C.c_void_p), ("len", C.c_uint32)]


class Metadata(C.Structure):
    """JpegAmdMetadata: pixel density, Exif, ICC profile, comment, segments."""
    _fields_ = [("density_units", C.c_int32), ("x_density", C.c_int32), ("y_density", C.c_int32),
                ("exif", C.c_void_p), ("exif_len", C.c_uint32), ("icc", C.c_void_p), ("icc_len", C.c_uint64),
                ("comment", C.c_void_p), ("comment_len", C.c_uint32), ("segments", C.POINTER(Segment)), ("segment_count", C.c_int32)]


def _prototypes():
    """Every entry of libjpegamd.so that the binding calls, written ONCE: name -> (result type, argument types), in four groups.
    `base`: declared in include/jpeg_compression.h, in every build.  `later`: declared there as well, but a variant build of an
    older round (JPEGAMD_LIB) may lack them.  `hidden`: debug entries that the header deliberately leaves out; a variant build may
    lack them too.  `tests`: debug entries the header leaves out that every build has."""
    u64, i32, i64, vp, f32 = C.c_uint64, C.c_int32, C.c_int64, C.c_void_p, C.c_float
    vpp, image = C.POINTER(vp), C.POINTER(Image)

    def batch(struct, before: int, after: int = 0):
        """(context, pictures[], count, `before` ints, outs[], capacity, sizes[], `after` ints, stream)"""
        return i32, [vp, C.POINTER(struct), i32] + [i32] * before + [vpp, u64, vpp] + [i32] * after + [vp]

    base = {
        "jpegamd_encoder_create": (i32, [vpp, i32, i32]),
        "jpegamd_encoder_destroy": (i32, [vp]),
        "jpegamd_max_jfif_bytes": (u64, [i32, i32]),
        "jpegamd_encode_async": (i32, [vp, image, vp, u64, vp, i32, vp]),
        "jpegamd_encode_batch_async": batch(Image, 0, 1),
        "jpegamd_encoder_finish": (i32, [vp, C.POINTER(Stats)]),
        "jpegamd_encoder_set_profiling": (i32, [vp, i32]),
        "jpegamd_encoder_profile": (i32, [vp, i32, C.POINTER(Stats)]),
        "jpegamd_debug_stages": (i32, [vp, image, vp, vp, vp]),
        "jpegamd_debug_dct_exact": (i32, [vp, vp, vp, i64]),
        "jpegamd_synth_bmp": (u64, [i32, i32, C.c_uint32, i32, C.c_uint32, vp, u64]),
        "jpegamd_version": (C.c_char_p, []),
        "jpegamd_debug_quant_table": (i32, [i32, vp]),
        "jpegamd_segment_meta_words": (i32, []),
        "jpegamd_debug_mfma_consts": (i32, [i32, vp, vp, vp, vp]),
        "jpegamd_debug_group_thresholds": (i32, [i32, vp, vp]),
        "jpegamd_debug_cos_lut": (i32, [vp]),
        "JpegCompression_Init": (i32, []),
        "JpegCompression_DeInit": (i32, []),
        "JpegCompression_Reserve": (i32, [i32, i32]),
        "convertToJpeg": (i32, [C.POINTER(DTO)]),
        "JpegCompression_RemoteServiceHandler": (i32, [C.c_char_p, C.c_uint32, vp, C.c_uint32, C.c_uint32]),
        "loadBMPImage": (C.POINTER(BMPImage), [C.c_char_p]),
        "freeBMPImage": (None, [C.POINTER(BMPImage)]),
        "saveJPEGGrayscale": (C.c_bool, [C.c_char_p, C.POINTER(BMPImage)]),
        "jpegamd_encode_bmp_memory": (i64, [vp, u64, i32, vp, u64]),
        "jpegamd_encode_bmp_memory_color": (i64, [vp, u64, i32, i32, vp, u64]),
        "jpegamd_parse_bmp": (i32, [vp, u64, image, C.POINTER(u64)]),
        "jpegamd_encode_files": (i32, [C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), i32, i32, C.POINTER(i32), C.POINTER(BatchStats)]),
        "jpegamd_max_jfif_bytes_color": (u64, [i32, i32, i32]),
        "jpegamd_encode_color_async": (i32, [vp, image, i32, vp, u64, vp, vp]),
        "jpegamd_debug_chroma_quant_table": (i32, [i32, vp]),
        "jpegamd_debug_chroma_mfma_consts": (i32, [i32, vp, vp, vp, vp, vp, vp]),
        "jpegamd_debug_chroma_group_thresholds": (i32, [i32, vp, vp]),
        "jpegamd_debug_color_profile": (i32, [vp, i32, vp]),
        "jpegamd_encode_rows_async": (i32, [vp, image, i32, i32, vp]),
        "jpegamd_export_segments": (i32, [vp, image, i32, i32, vp, u64, vp, vp, vp]),
        "jpegamd_import_segments": (i32, [vp, image, i32, i32, vp, vp, vp]),
        "jpegamd_finalize_async": (i32, [vp, image, vp, u64, vp, i32, vp]),
        # progressive files: no variant build is kept from before them
        "jpegamd_encode_color_progressive_batch_async": batch(Image, 1),
        "jpegamd_encode_ycbcr_progressive_batch_async": batch(YCbCrImage, 4),               # (subsampling, range, format, matrix)
        "jpegamd_max_jfif_bytes_progressive": (u64, [i32, i32, i32]),
        # ... with end-of-band runs and per-scan optimised tables
        "jpegamd_encode_color_progressive_optimized_batch_async": batch(Image, 1),
        "jpegamd_encode_ycbcr_progressive_optimized_batch_async": batch(YCbCrImage, 4),
        "jpegamd_max_jfif_bytes_progressive_optimized": (u64, [i32, i32, i32]),
        "jpegamd_debug_progressive_counts": (i32, [vp, vp]),
        # ... with successive approximation: ten scans
        "jpegamd_encode_color_progressive_successive_batch_async": batch(Image, 1),
        "jpegamd_encode_ycbcr_progressive_successive_batch_async": batch(YCbCrImage, 4),
        "jpegamd_max_jfif_bytes_progressive_successive": (u64, [i32, i32, i32]),
        "jpegamd_debug_progressive_successive_counts": (i32, [vp, vp]),
        # ... with a scan script of the caller's, and grayscale progressive files: (.., scans[], scan count, outs[], ..)
        "jpegamd_validate_scan_script": (i32, [vp, i32, i32, C.POINTER(i32)]),
        "jpegamd_encode_color_progressive_script_batch_async": (i32, [vp, C.POINTER(Image), i32, i32, vp, i32, vpp, u64, vpp, vp]),
        "jpegamd_encode_ycbcr_progressive_script_batch_async": (i32, [vp, C.POINTER(YCbCrImage), i32, i32, i32, i32, i32, vp, i32, vpp, u64, vpp, vp]),
        "jpegamd_encode_gray_progressive_script_batch_async": (i32, [vp, C.POINTER(Image), i32, vp, i32, vpp, u64, vpp, vp]),
        "jpegamd_max_jfif_bytes_progressive_script": (u64, [i32, i32, i32, vp, i32]),
        "jpegamd_debug_progressive_script_counts": (i32, [vp, vp, i32]),
        # caller-supplied quantisation tables
        "jpegamd_quant_tables_for_quality": (i32, [i32, vp, vp]),
        "jpegamd_encoder_set_quant_tables": (i32, [vp, vp, vp]),
        "jpegamd_encoder_get_quant_tables": (i32, [vp, vp, vp, C.POINTER(i32)]),
        "jpegamd_debug_table_consts": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        # metadata in front of the tables
        "jpegamd_build_metadata": (i64, [C.POINTER(Metadata), vp, u64, vp]),
        "jpegamd_encoder_set_metadata": (i32, [vp, C.POINTER(Metadata)]),
        "jpegamd_encoder_metadata_bytes": (i64, [vp]),
        # float pictures: (context, pictures[], count, subsampling, sample type, scale, offset, ..., outs[], ..)
        "jpegamd_encode_float_batch_async": (i32, [vp, C.POINTER(FloatImage), i32, i32, i32, f32, f32, vpp, u64, vpp, vp]),
        "jpegamd_encode_float_interleaved_batch_async": (i32, [vp, C.POINTER(FloatImage), i32, i32, i32, f32, f32, i32, vpp, u64, vpp, vp]),
        "jpegamd_encode_float_progressive_script_batch_async": (i32, [vp, C.POINTER(FloatImage), i32, i32, i32, f32, f32, vp, i32, vpp, u64,
                                                                      vpp, vp]),
        # reduced pictures: (context, pictures[], count, subsampling, factor, ..., outs[], out_cap, sizes[], stream)
        "jpegamd_reduced_size": (i32, [i32, i32, i32, C.POINTER(i32), C.POINTER(i32)]),
        "jpegamd_encode_reduced_batch_async": (i32, [vp, C.POINTER(StridedImage), i32, i32, i32, vpp, u64, vpp, vp]),
        "jpegamd_encode_reduced_interleaved_batch_async": (i32, [vp, C.POINTER(StridedImage), i32, i32, i32, i32, vpp, u64, vpp, vp]),
        "jpegamd_encode_reduced_progressive_script_batch_async": (i32, [vp, C.POINTER(StridedImage), i32, i32, i32, vp, i32, vpp, u64, vpp, vp]),
        # resized pictures: (context, pictures[], count, subsampling, out_width, out_height, ..., outs[], out_cap,
        # sizes[], stream)
        "jpegamd_resize_check": (i32, [i32, i32, i32, i32]),
        "jpegamd_encode_resized_batch_async": (i32, [vp, C.POINTER(StridedImage), i32, i32, i32, i32, vpp, u64, vpp, vp]),
        "jpegamd_encode_resized_interleaved_batch_async": (i32, [vp, C.POINTER(StridedImage), i32, i32, i32, i32, i32, vpp, u64, vpp, vp]),
        "jpegamd_encode_resized_progressive_script_batch_async": (i32, [vp, C.POINTER(StridedImage), i32, i32, i32, i32, vp, i32, vpp, u64,
                                                                        vpp, vp]),
    }
    later = {
        "jpegamd_encoder_set_pipeline": (i32, [vp, i32]),
        "jpegamd_gather_streams": (i32, [vp, i32, i32, i32, vp, u64, i32, vp, vp, u64, vp]),
        "jpegamd_debug_mfma_offsets": (i32, [i32, vp, vp, vp, vp]),
        "jpegamd_encode_color_batch_async": batch(Image, 1),                                # (subsampling)
        "jpegamd_encode_planar_batch_async": batch(PlanarImage, 1),
        "jpegamd_encode_ycbcr_batch_async": batch(YCbCrImage, 1),
        "jpegamd_encode_ycbcr_range_batch_async": batch(YCbCrImage, 2),                     # (subsampling, range)
        "jpegamd_encode_ycbcr_samples_batch_async": batch(YCbCrImage, 3),                   # (subsampling, range, format)
        "jpegamd_encode_ycbcr_matrix_batch_async": batch(YCbCrImage, 4),                    # (subsampling, range, format, matrix)
        "jpegamd_encode_color_interleaved_batch_async": batch(Image, 1),
        "jpegamd_encode_ycbcr_interleaved_batch_async": batch(YCbCrImage, 1),
        "jpegamd_max_jfif_bytes_interleaved": (u64, [i32, i32, i32]),
        "jpegamd_encode_color_interleaved_restart_batch_async": batch(Image, 2),            # (subsampling, restart interval)
        "jpegamd_encode_ycbcr_interleaved_restart_batch_async": batch(YCbCrImage, 2),
        "jpegamd_max_jfif_bytes_interleaved_restart": (u64, [i32, i32, i32, i32]),
        "jpegamd_encode_ycbcr_interleaved_matrix_batch_async": batch(YCbCrImage, 5),        # (subsampling, range, format, matrix, restart interval)
        "jpegamd_encode_color_interleaved_pixels_batch_async": batch(Image, 2),
        "jpegamd_encode_planar_interleaved_batch_async": batch(PlanarImage, 2),
        "jpegamd_encoder_set_huffman": (i32, [vp, i32]),
        "jpegamd_debug_optimal_huffman": (i32, [vp, vp, i32, vp, vp, vp]),
        "jpegamd_debug_huffman_counts": (i32, [vp, vp]),
        "jpegamd_encode_gray_scan_batch_async": batch(Image, 1),                            # (restart interval)
        "jpegamd_max_jfif_bytes_gray_scan": (u64, [i32, i32, i32]),
    }
    hidden = {
        "jpegamd_debug_tile_variant": (i32, [i32, i32, i32, i32]),
        "jpegamd_debug_matrix_coeffs": (i32, [i32, vp]),
        "jpegamd_debug_ycbcr_matrix_planes": (i32, [vp, C.POINTER(YCbCrImage), i32, i32, i32, i32, i32, vp, vp, vp, vp]),
        "jpegamd_debug_chroma_groups": (i32, [i32, i32, i32, i32, i32, i32, i32, vp]),
        "jpegamd_debug_ycbcr_sources": (i32, [i32, i32, i32, i32, vp]),
    }
    tests = {
        "jpegamd_debug_float_planes": (i32, [vp, C.POINTER(FloatImage), i32, i32, i32, f32, f32, vp, vp, vp, vp]),
        "jpegamd_debug_reduced_planes": (i32, [vp, C.POINTER(StridedImage), i32, i32, i32, vp, vp, vp, vp]),
        "jpegamd_debug_reduce_reciprocal": (i32, [i32, C.POINTER(C.c_uint32), C.POINTER(i32)]),
        "jpegamd_debug_resized_planes": (i32, [vp, C.POINTER(StridedImage), i32, i32, i32, i32, vp, vp, vp, vp]),
        "jpegamd_debug_resize_divide": (i32, [C.c_uint32, u64, C.POINTER(C.c_uint32)]),
    }
    return base, later, hidden, tests


def _load() -> C.CDLL:
    if not LIB_PATH.exists():
        raise ImportError(f"{LIB_PATH} is missing: build it with `make -C {_PKG_ROOT}` "
                          "(or __graft_entry__.build()); there is no fallback implementation")
    lib = C.CDLL(str(LIB_PATH), mode=getattr(os, "RTLD_NOW", 2))
    for name, (res, args) in {**_BASE, **_LATER, **_HIDDEN, **_TESTS}.items():
        if name not in _BASE and name not in _TESTS and os.environ.get("JPEGAMD_LIB") and not hasattr(lib, name):
            continue                                              # (A/B tooling: a variant build of an older round)
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


_BASE, _LATER, _HIDDEN, _TESTS = _prototypes()
EXPORTED = [*_BASE, *_LATER]                                     # what include/jpeg_compression.h declares
lib = _load()


def _checked(name: str, *args):
    """lib.<name>(*args); a non-zero result is a JpegAmdError that names the entry.  `lib` is looked up at call time: tests and
    tools put their own in its place."""
    rc = getattr(lib, name)(*args)
    if rc:
        raise JpegAmdError(rc, name)


def quant_table(quality: int = 50):
    """uint8[64], raster order: the reference's table (quality 50) or its libjpeg scaling."""
    import numpy as np
    table = np.zeros(64, np.uint8)
    lib.jpegamd_debug_quant_table(quality, table.ctypes.data)
    return table


def chroma_quant_table(quality: int = 50):
    """uint8[64], raster order: the colour files' chroma table (T.81 Annex K, K.2), scaled for `quality` like quant_table."""
    import numpy as np
    table = np.zeros(64, np.uint8)
    lib.jpegamd_debug_chroma_quant_table(quality, table.ctypes.data)
    return table


def chroma_mfma_consts(quality: int = 50):
    """mfma_consts() for the chroma table: qmul/qthr/bias/zoff/qadd float32[64] by zigzag position, delta float64[64] by raster k,
    dc_off and scale (table-independent: the luma set's)."""
    import numpy as np
    out = {k: np.zeros(64, np.float32) for k in ("qmul", "qthr", "bias", "zoff", "qadd")}
    delta = np.zeros(64, np.float64)
    lib.jpegamd_debug_chroma_mfma_consts(quality, out["qmul"].ctypes.data, out["qthr"].ctypes.data, out["bias"].ctypes.data,
                                         delta.ctypes.data, out["zoff"].ctypes.data, out["qadd"].ctypes.data)
    luma = mfma_consts(quality)
    return dict(out, delta=delta, dc_off=luma["dc_off"], scale=luma["scale"])


PIPELINE_AUTO, PIPELINE_PAIR, PIPELINE_STITCH = 0, 1, 2                    # JPEGAMD_PIPELINE_*
MAX_BATCH = 32                                               # JPEGAMD_MAX_BATCH
SEG_META_WORDS = int(lib.jpegamd_segment_meta_words())      # metadata words per segment in the sharded-image exchange


def mfma_consts(quality: int = 50):
    """Constants of the matrix-pipe kernel: qmul/qthr/bias/zoff/qadd float32[64] by zigzag position, delta float64[64] by raster k,
    dc_off and scale (accumulator units)."""
    import numpy as np
    qmul, qthr = np.zeros(64, np.float32), np.zeros(64, np.float32)
    bias, delta = np.zeros(64, np.float32), np.zeros(64, np.float64)
    lib.jpegamd_debug_mfma_consts(quality, qmul.ctypes.data, qthr.ctypes.data, bias.ctypes.data, delta.ctypes.data)
    zoff, qadd = np.zeros(64, np.float32), np.zeros(64, np.float32)
    dc_off, scale = np.zeros(1, np.float32), np.zeros(1, np.float32)
    lib.jpegamd_debug_mfma_offsets(quality, zoff.ctypes.data, qadd.ctypes.data, dc_off.ctypes.data, scale.ctypes.data)
    return dict(qmul=qmul, qthr=qthr, bias=bias, delta=delta, zoff=zoff, qadd=qadd, dc_off=float(dc_off[0]), scale=float(scale[0]))


def group_thresholds(quality: int = 50, with_lo_bound: bool = False, chroma: bool = False):
    """float32 [4][2]: zero threshold of coefficient group G for lane half h, on the hi chain (with_lo_bound: and the lo chain's bound);
    chroma: for the colour files' chroma table."""
    import numpy as np
    t, lo = np.zeros(8, np.float32), np.zeros(8, np.float32)
    (lib.jpegamd_debug_chroma_group_thresholds if chroma else lib.jpegamd_debug_group_thresholds)(quality, t.ctypes.data, lo.ctypes.data)
    return (t.reshape(4, 2), lo.reshape(4, 2)) if with_lo_bound else t.reshape(4, 2)


def quant_tables_for_quality(quality: int = 50):
    """(luma, chroma), uint8[64] each in raster order: Annex K scaled for `quality` (0 -> 50) as the encoder derives them
    (jpegamd_quant_tables_for_quality)."""
    import numpy as np
    luma, chroma = np.zeros(64, np.uint8), np.zeros(64, np.uint8)
    _checked("jpegamd_quant_tables_for_quality", int(quality), luma.ctypes.data, chroma.ctypes.data)
    return luma, chroma


def as_quant_table(t):
    """A quantisation table given as 64 values or as 8 x 8 values (a list or an array; raster order) -> uint8[64] in raster order.
    A wrong shape, a value that is no integer or one outside 1 .. 255 is a ValueError."""
    import numpy as np
    try:
        a = np.asarray(t)
    except Exception:
        raise ValueError("a quantisation table is 64 values or 8 x 8 values") from None
    if a.shape not in ((64,), (8, 8)):
        raise ValueError(f"a quantisation table is 64 values or 8 x 8 values, not an array of shape {a.shape}")
    if a.dtype.kind not in "iu":
        if a.dtype.kind != "f" or not np.all(a == np.floor(a)):
            raise ValueError("the entries of a quantisation table are integers 1 .. 255")
    a = a.reshape(64)
    if np.any(a < 1) or np.any(a > 255):
        raise ValueError(f"the entries of a quantisation table are 1 .. 255, not {int(a.min())} .. {int(a.max())}")
    return np.ascontiguousarray(a.astype(np.uint8))


def table_consts(table):
    """Constants of the matrix-pipe quantiser for an arbitrary table (jpegamd_debug_table_consts): what mfma_consts and
    group_thresholds give for a quality -- qmul/qthr/bias/zoff/qadd float32[64] by zigzag position, delta float64[64] by raster k,
    grp_thr and lo_bound float32 [4][2]."""
    import numpy as np
    t = as_quant_table(table)
    out = {k: np.zeros(64, np.float32) for k in ("qmul", "qthr", "bias", "zoff", "qadd")}
    delta, grp, lo = np.zeros(64, np.float64), np.zeros(8, np.float32), np.zeros(8, np.float32)
    _checked("jpegamd_debug_table_consts", t.ctypes.data, out["qmul"].ctypes.data, out["qthr"].ctypes.data, out["bias"].ctypes.data,
             delta.ctypes.data, out["zoff"].ctypes.data, out["qadd"].ctypes.data, grp.ctypes.data, lo.ctypes.data)
    return dict(out, delta=delta, grp_thr=grp.reshape(4, 2), lo_bound=lo.reshape(4, 2))


def parse_qtables(text: str):
    """The text format of cjpeg -qtables -> (luma, chroma), uint8[64] each in raster order; chroma is None for a text of one table.
    Decimal integers separated by whitespace, `#` starts a comment that runs to the end of the line, 64 values a table in raster
    order, one or two tables; anything else is a ValueError that names the count found."""
    words = " ".join(line.split("#", 1)[0] for line in text.splitlines()).split()
    bad = [w for w in words if not (w.isascii() and w.isdigit())]
    if bad:
        raise ValueError(f"quantisation tables are written as decimal integers, not {bad[0]!r}")
    if len(words) not in (64, 128):
        raise ValueError(f"expected 64 or 128 values (one or two tables of 64), found {len(words)}")
    values = [int(w) for w in words]
    return as_quant_table(values[:64]), (as_quant_table(values[64:]) if len(values) == 128 else None)


_EXIF_ID = b"Exif\0\0"


def _bytes_of(value, what: str) -> bytes:
    if isinstance(value, (bytes, bytearray, memoryview)):
        return bytes(value)
    raise ValueError(f"{what} is given as bytes, not as {type(value).__name__}")


def _metadata_struct(icc_profile=None, exif=None, comment=None, dpi=None, density=None, segments=()):
    """The keywords of build_metadata -> (Metadata, the objects its pointers refer to: keep them while the struct is in use)."""
    m, keep = Metadata(), []
    m.density_units = -1

    def buffer(data: bytes):
        buf = C.create_string_buffer(data, len(data)) if data else C.create_string_buffer(1)
        keep.append(buf)
        return C.cast(buf, C.c_void_p)

    if dpi is not None and density is not None:
        raise ValueError("give dpi or density, not both")
    if dpi is not None:
        x, y = dpi if isinstance(dpi, (tuple, list)) else (dpi, dpi)
        density = (1, x, y)
    if density is not None:
        units, x, y = density
        if any(v != int(v) for v in (units, x, y)):
            raise ValueError("a pixel density is made of whole numbers: units 0 .. 2, X and Y 1 .. 65535")
        m.density_units, m.x_density, m.y_density = int(units), int(x), int(y)
        if m.density_units < 0:
            raise ValueError("density units are 0 (aspect ratio), 1 (dots per inch) or 2 (dots per cm)")
    if exif is not None:
        data = exif.tobytes() if hasattr(exif, "tobytes") and not isinstance(exif, memoryview) else _bytes_of(exif, "exif")
        if data.startswith(_EXIF_ID):
            data = data[len(_EXIF_ID):]
        m.exif, m.exif_len = buffer(data), len(data)
    if icc_profile is not None:
        data = _bytes_of(icc_profile, "icc_profile")
        m.icc, m.icc_len = buffer(data), len(data)
    if comment is not None:
        data = comment.encode("utf-8") if isinstance(comment, str) else _bytes_of(comment, "comment")
        m.comment, m.comment_len = buffer(data), len(data)
    segments = list(segments)
    if segments:
        arr = (Segment * len(segments))()
        for seg, (marker, payload) in zip(arr, segments):
            data = _bytes_of(payload, "a segment's payload")
            seg.marker, seg.data, seg.len = int(marker), buffer(data), len(data)
        keep.append(arr)
        m.segments, m.segment_count = arr, len(segments)
    return m, keep


def build_metadata(icc_profile=None, exif=None, comment=None, dpi=None, density=None, segments=()):
    """(head, blob), both bytes: the 20 leading bytes of every file and the marker segments that follow them, as a context with this
    metadata writes them (jpegamd_build_metadata; host only).  dpi=(x, y) or a number: dots per inch; density=(units, x, y) with
    units 0 / 1 / 2.  exif: the TIFF block as bytes, with or without the "Exif\\0\\0" identifier, or an object with .tobytes()
    (PIL's Image.Exif).  comment: str (written as UTF-8) or bytes; "" writes an empty comment.  segments: (marker, payload) pairs of
    the caller's own, 0xE1 .. 0xEF and 0xFE, written between Exif and the ICC profile.  What the library refuses is a ValueError."""
    m, keep = _metadata_struct(icc_profile, exif, comment, dpi, density, segments)
    head = C.create_string_buffer(20)
    n = lib.jpegamd_build_metadata(C.byref(m), None, 0, head)
    if n < 0:
        raise ValueError("metadata refused: a density outside units 0 .. 2 / 1 .. 65535, Exif above 65527 bytes, a comment or segment "
                         "above 65533, a marker other than 0xE1 .. 0xEF / 0xFE, more than 16 segments or an ICC profile above 16707345 bytes")
    blob = C.create_string_buffer(max(int(n), 1))
    if lib.jpegamd_build_metadata(C.byref(m), blob, int(n), head) != n:
        raise JpegAmdError(-1, "jpegamd_build_metadata")
    del keep
    return head.raw, blob.raw[:int(n)]


def exif_orientation(n: int) -> bytes:
    """The TIFF block that holds the orientation tag (0x0112) alone, value n = 1 .. 8: 26 bytes, little-endian.  For exif=."""
    import struct
    if not 1 <= int(n) <= 8:
        raise ValueError("an Exif orientation is 1 .. 8")
    return b"II*\0" + struct.pack("<IHHHIHHI", 8, 1, 0x0112, 3, 1, int(n), 0, 0)


def cos_lut():
    """float32 [8][8]: COS_LUT[x][u] as compiled into the kernels."""
    import numpy as np
    t = np.zeros(64, np.float32)
    lib.jpegamd_debug_cos_lut(t.ctypes.data)
    return t.reshape(8, 8)


def version() -> str:
    return lib.jpegamd_version().decode()


def synth_bmp(width: int, height: int, seed: int = 1, kind: int = 0, flags: int = 0) -> bytes:
    """Deterministic synthetic 24-bit BMP file (host code in the library; no device needed)."""
    n = lib.jpegamd_synth_bmp(width, height, seed, kind, flags, None, 0)
    if n == 0:
        raise ValueError("bad synth_bmp arguments")
    buf = (C.c_uint8 * n)()
    got = lib.jpegamd_synth_bmp(width, height, seed, kind, flags, buf, n)
    assert got == n
    return bytes(buf)


def synth_bmp_into(ptr: int, cap: int, width: int, height: int, seed: int = 1, kind: int = 0, flags: int = 0) -> int:
    """Generate straight into caller memory (e.g. a pinned torch tensor); returns file size."""
    return int(lib.jpegamd_synth_bmp(width, height, seed, kind, flags, C.c_void_p(ptr), cap))


def parse_bmp(data: bytes):
    """-> (Image view with pixels=offset, pixel_offset) using loadBMPImage's header rules."""
    img, off = Image(), C.c_uint64(0)
    _checked("jpegamd_parse_bmp", data, len(data), C.byref(img), C.byref(off))
    return img, off.value


def max_jfif_bytes(width: int, height: int) -> int:
    return int(lib.jpegamd_max_jfif_bytes(width, height))


def encode_bmp_bytes(bmp: bytes, quality: int = 0) -> bytes:
    """BMP file bytes -> JFIF file bytes through the device (upload, encode, download)."""
    img, _ = parse_bmp(bmp)
    cap = 4096 + img.width * img.height * 2
    for _ in range(2):
        out = (C.c_uint8 * cap)()
        n = lib.jpegamd_encode_bmp_memory(bmp, len(bmp), quality, out, cap)
        if n == -8:
            cap = max_jfif_bytes(img.width, img.height)
            continue
        if n < 0:
            raise JpegAmdError(int(n), "jpegamd_encode_bmp_memory")
        return bytes(out[:n])
    raise JpegAmdError(-8, "jpegamd_encode_bmp_memory")


def max_jfif_bytes_color(width: int, height: int, subsampling: int = SUBSAMPLE_420) -> int:
    return int(lib.jpegamd_max_jfif_bytes_color(width, height, subsampling))


def max_jfif_bytes_interleaved(width: int, height: int, subsampling: int = SUBSAMPLE_420) -> int:
    """Upper bound on the bytes of a colour file with ONE scan of interleaved MCUs (pad blocks counted); 0 for bad arguments."""
    return int(lib.jpegamd_max_jfif_bytes_interleaved(width, height, subsampling))


def max_jfif_bytes_interleaved_restart(width: int, height: int, subsampling: int = SUBSAMPLE_420, restart_interval: int = 0) -> int:
    """Upper bound on the bytes of the one-scan file with restart intervals of `restart_interval` MCUs (0: none); 0 for bad arguments."""
    return int(lib.jpegamd_max_jfif_bytes_interleaved_restart(width, height, subsampling, restart_interval))


def max_jfif_bytes_gray_scan(width: int, height: int, restart_interval: int = 0) -> int:
    """Upper bound on the bytes of a grayscale file of jpegamd_encode_gray_scan_batch_async, in either Huffman mode; 0 for bad arguments."""
    return int(lib.jpegamd_max_jfif_bytes_gray_scan(width, height, restart_interval))


def max_jfif_bytes_progressive(width: int, height: int, subsampling: int = SUBSAMPLE_420) -> int:
    """Upper bound on the bytes of a progressive colour file (seven scans); 0 for bad arguments."""
    return int(lib.jpegamd_max_jfif_bytes_progressive(width, height, subsampling))


def max_jfif_bytes_progressive_optimized(width: int, height: int, subsampling: int = SUBSAMPLE_420) -> int:
    """Upper bound on the bytes of a progressive colour file with end-of-band runs and per-scan optimised tables (DESIGN.md
    4.6.13): max_jfif_bytes_progressive + 780; 0 for bad arguments."""
    return int(lib.jpegamd_max_jfif_bytes_progressive_optimized(width, height, subsampling))


def max_jfif_bytes_progressive_successive(width: int, height: int, subsampling: int = SUBSAMPLE_420) -> int:
    """Upper bound on the bytes of a progressive colour file with successive approximation (ten scans); 0 for bad
    arguments."""
    return int(lib.jpegamd_max_jfif_bytes_progressive_successive(width, height, subsampling))


MAX_SCANS = 16                                                   # JPEGAMD_MAX_SCANS


class Scan(C.Structure):
    """JpegAmdScan: the component set as a bit mask (bit 0 Y, bit 1 Cb, bit 2 Cr), Ss, Se, Ah, Al."""
    _fields_ = [("components", C.c_uint8), ("ss", C.c_uint8), ("se", C.c_uint8), ("ah", C.c_uint8), ("al", C.c_uint8)]


def _scan_array(scans):
    """scans: None (the default script) or a sequence of (components, Ss, Se, Ah, Al), components a tuple of component indices 0 .. 2
    -> (the JpegAmdScan array or None, its length).  Values that no JpegAmdScan holds are a ValueError; the rules of a script are
    the library's to check."""
    if scans is None:
        return None, 0
    out = []
    for k, scan in enumerate(scans):
        try:
            comps, ss, se, ah, al = scan
            comps = tuple(int(c) for c in comps)
            rest = tuple(int(v) for v in (ss, se, ah, al))
        except (TypeError, ValueError):
            raise ValueError(f"scan {k}: expected (components, ss, se, ah, al) with components a tuple of indices, not {scan!r}") from None
        if any(c < 0 or c > 2 for c in comps) or len(set(comps)) != len(comps) or any(v < 0 or v > 255 for v in rest):
            raise ValueError(f"scan {k}: component indices are distinct and 0 .. 2, the other values 0 .. 255, not {scan!r}")
        out.append(Scan(sum(1 << c for c in comps), *rest))
    return (Scan * len(out))(*out), len(out)


def validate_scan_script(scans, components: int = 3) -> None:
    """Check a scan script -- a sequence of (components, Ss, Se, Ah, Al) -- for a file of `components` components (3, or 1 for a
    grayscale file) with jpegamd_validate_scan_script; a script that breaks a rule is a ValueError that names the offending scan."""
    arr, n = _scan_array(scans if scans is not None else ())
    bad = C.c_int32(-1)
    if lib.jpegamd_validate_scan_script(arr, n, int(components), C.byref(bad)):
        where = f"scan {bad.value}" if bad.value >= 0 else "the script as a whole"
        raise ValueError(f"invalid scan script for {components} component(s): {where} breaks a rule of T.81 G.1.1.1")


def max_jfif_bytes_progressive_script(width: int, height: int, subsampling: int = SUBSAMPLE_420, scans=None) -> int:
    """Upper bound on the bytes of a progressive file with the scan script `scans` (None: the default script);
    subsampling 0: a grayscale file.  0 for bad arguments or an invalid script."""
    arr, n = _scan_array(scans)
    return int(lib.jpegamd_max_jfif_bytes_progressive_script(width, height, subsampling, arr, n))


class ProgressiveScript:
    """A `progressive` argument inside this package: the entries of DESIGN.md 4.6.15 with this script (None: the default one)."""

    def __init__(self, scans):
        self.scans = None if scans is None else [(tuple(c), ss, se, ah, al) for c, ss, se, ah, al in scans]


SCANS = ("separate", "interleaved")
HUFFMAN_STANDARD, HUFFMAN_OPTIMIZED = 0, 1       # jpegamd_encoder_set_huffman
PROGRESSIVE_OPTIMIZED = "optimized"              # a `progressive` argument inside this package: the entries of DESIGN.md 4.6.13 (True: 4.6.12's)
PROGRESSIVE_SUCCESSIVE = "successive"            # ... of DESIGN.md 4.6.14


def _progressive_entry(enc, progressive, ycbcr: bool):
    """The Encoder method a `progressive` argument names, as a callable with the arguments of the entries without a script: a
    ProgressiveScript's scans go in front of the output pointers."""
    fn = getattr(enc, _progressive_mode(progressive)[2 if ycbcr else 1])
    if isinstance(progressive, ProgressiveScript):
        return lambda *a: fn(*a[:-4], progressive.scans, *a[-4:])
    return fn


def _progressive_mode(progressive):
    """A `progressive` argument -> (the bound, the Encoder method of packed pixels, the one of YCbCr pictures, whether the entries
    make their own tables and leave the context's Huffman mode alone)."""
    if isinstance(progressive, ProgressiveScript):
        return (lambda w, h, sub: max_jfif_bytes_progressive_script(w, h, sub, progressive.scans), "encode_color_progressive_script_batch_async",
                "encode_ycbcr_progressive_script_batch_async", True)
    if progressive == PROGRESSIVE_SUCCESSIVE:
        return (max_jfif_bytes_progressive_successive, "encode_color_progressive_successive_batch_async",
                "encode_ycbcr_progressive_successive_batch_async", True)
    if progressive == PROGRESSIVE_OPTIMIZED:
        return (max_jfif_bytes_progressive_optimized, "encode_color_progressive_optimized_batch_async",
                "encode_ycbcr_progressive_optimized_batch_async", True)
    return max_jfif_bytes_progressive, "encode_color_progressive_batch_async", "encode_ycbcr_progressive_batch_async", False



HUFFMANS = ("standard", "optimized")


def _huffman(huffman) -> int:
    """huffman= of jpegamd.mjpeg's functions -> HUFFMAN_STANDARD / HUFFMAN_OPTIMIZED; anything else is a ValueError."""
    if not isinstance(huffman, str) or huffman not in HUFFMANS:
        raise ValueError(f'huffman must be "standard" or "optimized", not {huffman!r}')
    return HUFFMANS.index(huffman)


def _restart(restart_interval, interleaved: bool, w: int, subsampling: int) -> int:
    """restart_interval= of the tensor functions -> the interval in MCUs: None / 0 none, an int 1 .. 65535, or "row" for one MCU row
    (ceil(W / 8) MCUs at SUBSAMPLE_444, ceil(W / 16) otherwise).  Restart intervals exist in scan="interleaved" files alone."""
    if restart_interval is None or (isinstance(restart_interval, int) and not isinstance(restart_interval, bool) and restart_interval == 0):
        return 0
    if restart_interval == "row":
        ri = -(-w // (8 if subsampling == SUBSAMPLE_444 else 16))
    elif isinstance(restart_interval, int) and not isinstance(restart_interval, bool) and 1 <= restart_interval <= 65535:
        ri = restart_interval
    else:
        raise ValueError(f'restart_interval must be 0 / None, an int in 1..65535 (MCUs) or "row", not {restart_interval!r}')
    if not interleaved:
        raise ValueError('restart_interval needs scan="interleaved"')
    return ri


def _scan(scan) -> bool:
    """"separate" / "interleaved" -> is it the interleaved file; anything else is a ValueError."""
    if not isinstance(scan, str) or scan not in SCANS:
        raise ValueError(f"scan must be one of {SCANS}, not {scan!r}")
    return scan == "interleaved"


def encode_bmp_bytes_color(bmp: bytes, quality: int = 0, subsampling: int = SUBSAMPLE_420) -> bytes:
    """BMP file bytes -> colour JFIF file bytes (YCbCr, three scans) through the device."""
    img, _ = parse_bmp(bmp)
    cap = max_jfif_bytes_color(img.width, img.height, subsampling) or 1
    out = (C.c_uint8 * cap)()
    n = lib.jpegamd_encode_bmp_memory_color(bmp, len(bmp), quality, subsampling, out, cap)
    if n < 0:
        raise JpegAmdError(int(n), "jpegamd_encode_bmp_memory_color")
    return bytes(out[:n])


_tensor_encoders = {}


def _tensor_encoder(dev: int, w: int, rows: int):
    """The per-device context of the tensor functions, grown (a new one made) when a call needs more than w x rows."""
    enc, mw, mh = _tensor_encoders.get(dev, (None, 0, 0))
    if enc is None or w > mw or rows > mh:
        mw, mh = max(w, mw), max(rows, mh)
        if enc is not None:
            enc.close()
        enc = Encoder(mw, mh)
        _tensor_encoders[dev] = (enc, mw, mh)
    return enc


_block_tables = threading.local()            # .tables: the (luma, chroma) of the innermost quant_tables block of this thread


@contextlib.contextmanager
def quant_tables(luma, chroma=None):
    """with jpegamd.quant_tables(luma, chroma): every module-level encode of this thread -- jpegamd's, jpegamd.mjpeg's and the
    progressive modules' -- writes its files with these quantisation tables (as_quant_table takes each; chroma None: the luma table
    for every component) and ignores `quality`.  The tables are set on the shared per-device context for each call and taken off
    behind it, so that outside the block, also when an exception leaves it, the cached contexts encode by quality.  Blocks nest:
    the inner tables hold until the inner block ends."""
    tables = (as_quant_table(luma), None if chroma is None else as_quant_table(chroma))
    before = getattr(_block_tables, "tables", None)
    _block_tables.tables = tables
    try:
        yield
    finally:
        _block_tables.tables = before


_block_metadata = threading.local()          # .keywords: those of the innermost metadata block of this thread


@contextlib.contextmanager
def metadata(icc_profile=None, exif=None, comment=None, dpi=None, density=None, segments=()):
    """with jpegamd.metadata(icc_profile=, exif=, comment=, dpi=, density=, segments=): every module-level encode of this thread --
    jpegamd's, jpegamd.mjpeg's and the progressive modules' -- writes this metadata into its files (build_metadata names the
    keywords).  It is set on the shared per-device context for each call and taken off behind it, so that outside the block, also
    when an exception leaves it, the cached contexts write plain files.  Blocks nest: the inner metadata holds until the inner block
    ends (it replaces the outer one, it is not merged with it)."""
    keywords = dict(icc_profile=icc_profile, exif=exif, comment=comment, dpi=dpi, density=density, segments=tuple(segments))
    build_metadata(**keywords)                   # (refused here, not at the first encode)
    before = getattr(_block_metadata, "keywords", None)
    _block_metadata.keywords = keywords
    try:
        yield
    finally:
        _block_metadata.keywords = before


@contextlib.contextmanager
def _borrowed_encoder(dev: int, w: int, rows: int):
    """The per-device context for the calls of one tensor function: with the tables of the thread's quant_tables block and the
    metadata of its metadata block set on it, and back on quality and plain files when the function is done with it, whatever
    happens."""
    enc = _tensor_encoder(dev, w, rows)
    tables = getattr(_block_tables, "tables", None)
    keywords = getattr(_block_metadata, "keywords", None)
    if tables is None and keywords is None:
        yield enc
        return
    try:
        if tables is not None:
            enc.set_quant_tables(*tables)
        if keywords is not None:
            enc.set_metadata(**keywords)
        yield enc
    finally:
        if tables is not None:
            enc.set_quant_tables(None)
        if keywords is not None:
            enc.set_metadata(None)


def _files(out, sizes, k: int) -> list:
    """The first k files of a finished call: row i of `out`, sizes[i] bytes of it."""
    got = sizes[:k].cpu().tolist()
    return [bytes(out[i, :got[i]].cpu().numpy().tobytes()) for i in range(k)]


def _encode_pictures(device, n: int, h: int, w: int, cap: int, queue, huffman=None) -> list:
    """`n` pictures of one geometry through the per-device context, in calls of at most MAX_BATCH -> their files of at most `cap`
    bytes.  queue(enc, b0, k, outs, cap, size_ptrs, stream) queues pictures b0 .. b0 + k - 1 on `enc`.  `huffman`: None leaves the
    context's tables alone; a mode is set on the shared context around every call, which is finished inside, and HUFFMAN_STANDARD
    is put back whatever happens."""
    import torch
    dev = device.index if device.index is not None else torch.cuda.current_device()
    files = []
    per = min(n, MAX_BATCH)
    # (a batch needs `per` x the block rows of one picture; inside a quant_tables block the context carries its tables meanwhile)
    with torch.cuda.device(dev), _borrowed_encoder(dev, w, per * ((h + 7) // 8 * 8)) as enc:
        cap += enc.metadata_bytes()                                  # (no bound counts the metadata of a metadata block)
        out = torch.empty((per, cap), dtype=torch.uint8, device=device)
        sizes = torch.zeros(per, dtype=torch.int64, device=device)
        stream = torch.cuda.current_stream(device).cuda_stream
        for b0 in range(0, n, MAX_BATCH):
            k = min(MAX_BATCH, n - b0)
            outs = [out[i].data_ptr() for i in range(k)]
            size_ptrs = [sizes.data_ptr() + 8 * i for i in range(k)]
            if huffman is not None:
                enc.set_huffman(huffman)
            try:
                queue(enc, b0, k, outs, cap, size_ptrs, stream)
                enc.finish()
            finally:
                if huffman is not None:
                    enc.set_huffman(HUFFMAN_STANDARD)
            files += _files(out, sizes, k)
    return files


def encode_tensor(t, quality: int = 0, subsampling: int = SUBSAMPLE_420, layout=None, scan: str = "separate", restart_interval=None) -> bytes:
    """A uint8 DEVICE tensor -> JFIF file bytes: [H, W] a grayscale file (the tensor is the luma), [H, W, 3] (R, G, B) a colour file.
    Rows may be strided (t.stride(0) bytes apart); pixels within a row must be packed.  Runs on the tensor's device and the
    current stream; one encoder context per device is kept and grown as needed.
    `layout` names how the picture is stored, as for encode_tensor_batch: "chw" [3, H, W], "rgba" / "bgra" [H, W, 4], "hwc" [H, W, 3].
    scan="interleaved": the colour file with ONE scan of interleaved MCUs, as for encode_tensor_batch ([H, W, 3] alone), and with
    restart_interval= its restart intervals (jpegamd.mjpeg.encode_tensor: the one-scan file of every colour layout)."""
    import torch
    if _scan(scan):
        return encode_tensor_batch(t, quality, subsampling, "hwc" if layout is None else layout, _single=True, scan=scan,
                                   restart_interval=restart_interval)[0]
    _restart(restart_interval, False, 1, subsampling)
    if layout is not None:
        return encode_tensor_batch(t, quality, subsampling, layout, _single=True)[0]
    if t.dtype != torch.uint8 or not t.is_cuda:
        raise ValueError("encode_tensor needs a uint8 device tensor")
    if t.dim() == 2:
        h, w = t.shape
        if t.stride(1) != 1:
            raise ValueError("pixels of a row must be packed (stride(1) == 1)")
        order = ORDER_GRAY
    elif t.dim() == 3 and t.shape[2] == 3:
        h, w = t.shape[0], t.shape[1]
        if t.stride(2) != 1 or t.stride(1) != 3:
            raise ValueError("pixels of a row must be packed RGB (stride(1) == 3, stride(2) == 1)")
        order = ORDER_RGB
    else:
        raise ValueError("encode_tensor takes [H, W] or [H, W, 3]")
    dev = t.device.index if t.device.index is not None else torch.cuda.current_device()
    with torch.cuda.device(dev), _borrowed_encoder(dev, w, h) as enc:
        cap = (max_jfif_bytes(w, h) if order == ORDER_GRAY else max_jfif_bytes_color(w, h, subsampling)) + enc.metadata_bytes()
        out = torch.empty((1, cap), dtype=torch.uint8, device=t.device)
        size = torch.zeros(1, dtype=torch.int64, device=t.device)
        stream = torch.cuda.current_stream(t.device).cuda_stream
        img = Encoder.image(t.data_ptr(), w, h, t.stride(0), bottom_up=False, channel_order=order, quality=quality)
        if order == ORDER_GRAY:
            enc.encode_async(img, out.data_ptr(), cap, size.data_ptr(), True, stream)
        else:
            enc.encode_color_async(img, subsampling, out.data_ptr(), cap, size.data_ptr(), stream)
        enc.finish()
        return _files(out, size, 1)[0]


def _chroma_groups(max_width: int, max_height: int, width: int, height: int, count: int, subsampling: int = SUBSAMPLE_420,
                   pipeline: int = 0):
    """Test hook, not part of the API (jpegamd_debug_chroma_groups is not in the public header).  Host-only: how a colour batch of `count` width x height pictures on a context created for max_width x max_height groups its
    2 x count chroma planes into launches -> (planes per launch, launches, tiles per segment, k_stitch)."""
    out = (C.c_int32 * 4)()
    _checked("jpegamd_debug_chroma_groups", max_width, max_height, pipeline, width, height, count, subsampling, out)
    return out[0], out[1], out[2], bool(out[3])


def _batch_tensor_layout(t):
    """-> (count, height, width, row stride, channel order) of a [N, H, W, 3] (R, G, B) or [N, H, W] uint8 tensor whose pixels
    are packed within each row; pictures and rows may be strided."""
    import torch
    if t.dtype != torch.uint8:
        raise ValueError("encode_tensor_batch needs a uint8 tensor")
    if t.dim() == 3:
        n, h, w = t.shape
        if t.stride(2) != 1:
            raise ValueError("pixels of a row must be packed (stride(2) == 1)")
        order = ORDER_GRAY
        row_bytes = w
    elif t.dim() == 4 and t.shape[3] == 3:
        n, h, w = t.shape[0], t.shape[1], t.shape[2]
        if t.stride(3) != 1 or t.stride(2) != 3:
            raise ValueError("pixels of a row must be packed RGB (stride(2) == 3, stride(3) == 1)")
        order = ORDER_RGB
        row_bytes = 3 * w
    else:
        raise ValueError("encode_tensor_batch takes [N, H, W] or [N, H, W, 3]")
    if n < 1 or h < 1 or w < 1:
        raise ValueError("encode_tensor_batch needs at least one picture of at least one pixel")
    if h > 1 and t.stride(1) < row_bytes:
        raise ValueError("rows overlap (stride(1) is less than a row)")
    return n, h, w, (t.stride(1) if h > 1 else row_bytes), order


LAYOUTS = ("hwc", "chw", "rgba", "bgra")


def _named_layout(t, layout, single: bool):
    """The pictures of `t` stored as `layout` says -> (count, height, width, row stride, channel order -- None for planes --,
    picture index -> device pointer or (R, G, B) plane pointers, the tensors).  Shapes and strides only: host tensors pass."""
    import torch
    if layout not in LAYOUTS:
        raise ValueError(f"layout must be one of {LAYOUTS} or None, not {layout!r}")
    planes = list(t) if isinstance(t, (tuple, list)) else None
    if planes is not None and (layout != "chw" or len(planes) != 3):
        raise ValueError('a sequence of tensors is the R, G and B planes of layout="chw"')
    tensors = planes if planes is not None else [t]
    if any(not isinstance(x, torch.Tensor) or x.dtype != torch.uint8 for x in tensors):
        raise ValueError("the encoder needs uint8 tensors")
    lead = 0 if single else 1                                  # dimensions in front of a picture
    if layout == "chw":
        if planes is None:
            if t.dim() != lead + 3 or t.shape[lead] != 3:
                raise ValueError('layout="chw" takes [3, H, W] or [N, 3, H, W]')
            planes = [t.select(lead, k) for k in range(3)]
        if any(p.dim() != lead + 2 or p.shape != planes[0].shape for p in planes):
            raise ValueError("the three planes must be [H, W] or [N, H, W] tensors of one shape")
        if single:
            planes = [p.unsqueeze(0) for p in planes]
        n, h, w = planes[0].shape
        if n < 1 or h < 1 or w < 1:
            raise ValueError("the encoder needs at least one picture of at least one pixel")
        if any(p.stride(2) != 1 for p in planes):
            raise ValueError("samples of a row must be packed (last stride 1)")
        strides = {(p.stride(1) if h > 1 else w) for p in planes}
        if len(strides) != 1:
            raise ValueError("the three planes of a picture must share one row stride")
        stride = strides.pop()
        if stride < w:
            raise ValueError("rows overlap (the row stride is less than a row)")
        return n, h, w, stride, None, (lambda i: tuple(p[i].data_ptr() for p in planes)), planes
    c = 3 if layout == "hwc" else 4
    if t.dim() != lead + 3 or t.shape[-1] != c:
        raise ValueError(f'layout="{layout}" takes [H, W, {c}] or [N, H, W, {c}]')
    if single:
        t = t.unsqueeze(0)
    n, h, w = t.shape[0], t.shape[1], t.shape[2]
    if n < 1 or h < 1 or w < 1:
        raise ValueError("the encoder needs at least one picture of at least one pixel")
    if t.stride(3) != 1 or t.stride(2) != c:
        raise ValueError(f"pixels of a row must be packed (pixel stride {c}, last stride 1)")
    if h > 1 and t.stride(1) < c * w:
        raise ValueError("rows overlap (the row stride is less than a row)")
    order = {"hwc": ORDER_RGB, "rgba": ORDER_RGBA, "bgra": ORDER_BGRA}[layout]
    return n, h, w, (t.stride(1) if h > 1 else c * w), order, (lambda i: t[i].data_ptr()), [t]


def encode_tensor_batch(t, quality: int = 0, subsampling: int = SUBSAMPLE_420, layout=None, _single: bool = False,
                        scan: str = "separate", restart_interval=None, _any_layout: bool = False, _huffman: int = 0,
                        _progressive: bool = False) -> list:
    """A uint8 DEVICE tensor of N pictures -> N JFIF files: [N, H, W, 3] (R, G, B) colour files through
    jpegamd_encode_color_batch_async, [N, H, W] grayscale files through jpegamd_encode_batch_async.  Pictures may be strided
    (t[::2]), pixels within a row must be packed.  Batches of more than MAX_BATCH pictures go as several calls of at most
    MAX_BATCH.  Runs on the tensor's device and the current stream, with the per-device context of encode_tensor (grown to
    hold a batch).
    `layout` names another storage, read where it lies (no repacking): "chw" [N, 3, H, W] -- or a sequence of three [N, H, W]
    tensors, the R, G and B planes -- through jpegamd_encode_planar_batch_async (rows may be strided, the planes of a picture
    share one row stride, any plane stride; subsampling 0 gives grayscale files); "rgba" / "bgra" [N, H, W, 4], the fourth byte
    ignored; "hwc" the explicit name of [N, H, W, 3].  The files are those of the same R, G, B values as [N, H, W, 3].
    scan="interleaved": colour files with ONE scan of interleaved MCUs (jpegamd_encode_color_interleaved_batch_async) -- what
    Motion-JPEG containers and hardware decoders take -- for [N, H, W, 3] (layout None or "hwc") and the three colour subsamplings;
    every other combination is a ValueError here: jpegamd.mjpeg.encode_tensor_batch gives the one-scan files of every layout.  They
    decode to the same pixels as the scan="separate" files.
    restart_interval= (scan="interleaved" alone): restart intervals of that many MCUs, 1 .. 65535, or "row" for one MCU row (DRI /
    RSTn, jpegamd_encode_color_interleaved_restart_batch_async); 0 / None: none.
    (`_any_layout`: jpegamd.mjpeg's call -- scan="interleaved" with every colour layout, through the entries that read them;
    `_huffman`: its tables, set on the per-device context for this call and put back to HUFFMAN_STANDARD behind it;
    `_progressive`: jpegamd.progressive's call -- jpegamd.mjpeg's, with the progressive file of every packed layout written instead.)"""
    interleaved = _scan(scan)
    if _progressive and getattr(getattr(t, "dtype", None), "is_floating_point", False):
        raise ValueError("the progressive encoder needs a uint8 tensor: float pictures go through "
                         "jpegamd.progressive_script.encode_float_batch")
    if _progressive and layout == "chw":
        raise ValueError('progressive files take packed pixels: layout "hwc", "rgba" or "bgra", not "chw"')
    if _huffman and not interleaved:
        raise ValueError('optimised Huffman tables need scan="interleaved"')
    if not interleaved:
        _restart(restart_interval, False, 1, subsampling)
    if interleaved and not _any_layout and layout not in (None, "hwc"):
        raise ValueError(f'scan="interleaved" takes layout="hwc" (or None) alone, not {layout!r}')
    if interleaved and subsampling not in (SUBSAMPLE_444, SUBSAMPLE_420, SUBSAMPLE_422):
        raise ValueError('scan="interleaved" needs SUBSAMPLE_444, SUBSAMPLE_420 or SUBSAMPLE_422')
    if layout is None:
        n, h, w, stride, order = _batch_tensor_layout(t)
        ptr, tensors = (lambda i: t[i].data_ptr()), [t]
    else:
        n, h, w, stride, order, ptr, tensors = _named_layout(t, layout, _single)
    if interleaved and _any_layout and order == ORDER_GRAY:
        raise ValueError("a one-scan file is a colour file: [N, H, W] grayscale pictures are not taken")
    if interleaved and not _any_layout and order != ORDER_RGB:
        raise ValueError('scan="interleaved" takes colour pictures [N, H, W, 3] alone')
    ri = _restart(restart_interval, interleaved, w, subsampling)
    if any(not x.is_cuda or x.device != tensors[0].device for x in tensors):
        raise ValueError("encode_tensor_batch needs a device tensor")
    if _progressive:
        cap = _progressive_mode(_progressive)[0](w, h, subsampling)
    elif interleaved:
        cap = max_jfif_bytes_interleaved_restart(w, h, subsampling, ri) if ri else max_jfif_bytes_interleaved(w, h, subsampling)
    elif order == ORDER_GRAY or (order is None and subsampling == 0):
        cap = max_jfif_bytes(w, h)
    else:
        cap = max_jfif_bytes_color(w, h, subsampling)

    def queue(enc, b0, k, outs, cap, size_ptrs, stream):
        if order is None:
            imgs = [Encoder.planar_image(ptr(b0 + i), w, h, stride, bottom_up=False, quality=quality) for i in range(k)]
        else:
            imgs = [Encoder.image(ptr(b0 + i), w, h, stride, bottom_up=False, channel_order=order, quality=quality) for i in range(k)]
        _queue_pixels(enc, imgs, subsampling, outs, cap, size_ptrs, stream, interleaved, ri, _any_layout, _huffman, _progressive)

    # (a progressive call sets the standard tables on the shared context: the entry refuses any other mode; the progressive
    # entries that make their own tables do not read the mode)
    return _encode_pictures(tensors[0].device, n, h, w, cap, queue,
                            HUFFMAN_STANDARD if _progressive and not _progressive_mode(_progressive)[3] else (_huffman or None))


def _queue_pixels(enc, imgs, subsampling, outs, cap, size_ptrs, stream, interleaved: bool = False, restart: int = 0,
                  any_layout: bool = False, huffman: int = 0, progressive: bool = False):
    """One call of encode_tensor_batch queued on `enc`: which entry takes `imgs` (Image or PlanarImage structs of one geometry).
    Three scans: the planar, the grayscale (ORDER_GRAY) or the colour batch entry.  One scan: the planar entry; for packed pixels
    the entry of every pixel order with `any_layout` (jpegamd.mjpeg), otherwise the RGB entries of encode_tensor_batch's own
    scan="interleaved" -- the restart entry when there are intervals, and for `huffman` (whatever the interval)."""
    planar = isinstance(imgs[0], PlanarImage)
    if progressive:                                               # (jpegamd.progressive: packed pixels, no intervals, the standard tables;
        # jpegamd.progressive_optimized, jpegamd.progressive_successive: the tables of every scan its own)
        _progressive_entry(enc, progressive, False)(imgs, subsampling, outs, cap, size_ptrs, stream)
    elif not interleaved:
        if planar:
            enc.encode_planar_batch_async(imgs, subsampling, outs, cap, size_ptrs, stream)
        elif imgs[0].channel_order == ORDER_GRAY:
            enc.encode_batch_async(imgs, outs, cap, size_ptrs, True, stream)
        else:
            enc.encode_color_batch_async(imgs, subsampling, outs, cap, size_ptrs, stream)
    elif planar:
        enc.encode_planar_interleaved_batch_async(imgs, subsampling, restart, outs, cap, size_ptrs, stream)
    elif any_layout:
        enc.encode_color_interleaved_pixels_batch_async(imgs, subsampling, restart, outs, cap, size_ptrs, stream)
    elif restart or huffman:
        enc.encode_color_interleaved_restart_batch_async(imgs, subsampling, restart, outs, cap, size_ptrs, stream)
    else:
        enc.encode_color_interleaved_batch_async(imgs, subsampling, outs, cap, size_ptrs, stream)


def _encode_gray_scan_batch(t, quality, restart_interval, huffman, name: str) -> list:
    """jpegamd.mjpeg.encode_gray_batch: [N, H, W] uint8 on a device -> N grayscale files through jpegamd_encode_gray_scan_batch_async.
    Every argument is checked on the CPU before any device work."""
    import torch
    huff = _huffman(huffman)
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 3 or min(t.shape) < 1:
        raise ValueError(f"{name} needs a uint8 tensor [N, H, W]")
    n, h, w = (int(x) for x in t.shape)
    if w > 65535 or h > 65535:
        raise ValueError(f"{name}: a picture is at most 65535 x 65535")
    if t.stride(2) != 1 or t.stride(1) < w:
        raise ValueError(f"{name} needs pictures packed within a row (a row stride is fine)")
    ri = _restart(restart_interval, True, w, SUBSAMPLE_444)            # ("row": ceil(W / 8) -- the MCU is one block)
    if not t.is_cuda:
        raise ValueError(f"{name} needs a device tensor")

    def queue(enc, b0, k, outs, cap, size_ptrs, stream):
        imgs = [Encoder.image(t[b0 + i].data_ptr(), w, h, t.stride(1), bottom_up=False, channel_order=ORDER_GRAY, quality=quality)
                for i in range(k)]
        enc.encode_gray_scan_batch_async(imgs, ri, outs, cap, size_ptrs, stream)

    return _encode_pictures(t.device, n, h, w, max_jfif_bytes_gray_scan(w, h, ri), queue, huff)   # (the mode is set even for "standard")


def _ycbcr_layout_of(y, cb, cr, subsampling, order, dtypes, sample_bytes, pairs):
    """The pictures of a YCbCr batch -> (count, height, width, y stride, chroma stride, JPEGAMD_CHROMA_* layout), strides in BYTES.
    Shapes, dtypes and strides only: host tensors pass.  `dtypes`: the names of the torch dtypes taken; `sample_bytes`: 1 or 2;
    `pairs`: what the messages call the interleaved samples."""
    import torch
    if subsampling not in (SUBSAMPLE_444, SUBSAMPLE_420, SUBSAMPLE_422):
        raise ValueError("subsampling must be SUBSAMPLE_444, SUBSAMPLE_420 or SUBSAMPLE_422")
    if order not in ("cbcr", "crcb"):
        raise ValueError(f'order must be "cbcr" or "crcb", not {order!r}')
    tensors = [y, cb] + ([cr] if cr is not None else [])
    if any(not isinstance(x, torch.Tensor) or x.dtype not in [getattr(torch, d) for d in dtypes] for x in tensors):
        raise ValueError(f"the encoder needs {' or '.join(dtypes)} tensors" + (f" ({8 * sample_bytes}-bit sample words)" if sample_bytes > 1 else ""))
    if y.dim() != 3:
        raise ValueError("y must be [N, H, W]")
    n, h, w = y.shape
    if n < 1 or h < 1 or w < 1 or h > 65535 or w > 65535:
        raise ValueError("the encoder needs at least one picture of 1..65535 pixels each way")
    cw = w if subsampling == SUBSAMPLE_444 else (w + 1) // 2
    ch = (h + 1) // 2 if subsampling == SUBSAMPLE_420 else h
    if cr is None:
        if cb.dim() != 4 or tuple(cb.shape) != (n, ch, cw, 2):
            raise ValueError(f"with cr=None, cb holds the {pairs}: [N, {ch}, {cw}, 2] for this y and subsampling, not {tuple(cb.shape)}")
        if cb.stride(3) != 1 or cb.stride(2) != 2:
            raise ValueError("the pairs of a row must be packed (pair stride 2, last stride 1)")
        layout, c_row = (CHROMA_CBCR if order == "cbcr" else CHROMA_CRCB), 2 * cw
    else:
        if order != "cbcr":
            raise ValueError('order="crcb" names the interleaved layout (cr=None); swap the tensors for planes')
        for name, p in (("cb", cb), ("cr", cr)):
            if p.dim() != 3 or tuple(p.shape) != (n, ch, cw):
                raise ValueError(f"{name} must be [N, {ch}, {cw}] for this y and subsampling, not {tuple(p.shape)}")
            if p.stride(2) != 1:
                raise ValueError("samples of a row must be packed (last stride 1)")
        if ch > 1 and cb.stride(1) != cr.stride(1):
            raise ValueError("cb and cr must share one row stride")
        layout, c_row = CHROMA_PLANES, cw
    if y.stride(2) != 1:
        raise ValueError("samples of a row must be packed (last stride 1)")
    y_stride = y.stride(1) if h > 1 else w            # (in samples up to here)
    c_stride = cb.stride(1) if ch > 1 else c_row
    if y_stride < w or c_stride < c_row:
        raise ValueError("rows overlap (a row stride is less than a row)")
    if sample_bytes > 1 and (sample_bytes * y_stride >= 1 << 31 or sample_bytes * c_stride >= 1 << 31):
        raise ValueError("a row stride must stay below 2^31 bytes")
    return n, h, w, sample_bytes * y_stride, sample_bytes * c_stride, layout


def _ycbcr_layout(y, cb, cr, subsampling, order):
    """_ycbcr_layout_of for encode_ycbcr_batch: one byte per sample."""
    return _ycbcr_layout_of(y, cb, cr, subsampling, order, ("uint8",), 1, "byte pairs")


def _ycbcr16_layout(y, cb, cr, subsampling, order):
    """_ycbcr_layout_of for encode_ycbcr16_batch: 16-bit sample words."""
    return _ycbcr_layout_of(y, cb, cr, subsampling, order, ("int16", "uint16"), 2, "pairs of words")


def _sample_range(sample_range) -> int:
    """"full" / "limited" -> JPEGAMD_RANGE_*; anything else is a ValueError."""
    if not isinstance(sample_range, str) or sample_range not in ("full", "limited"):
        raise ValueError(f'sample_range must be "full" or "limited", not {sample_range!r}')
    return RANGE_LIMITED if sample_range == "limited" else RANGE_FULL


def _matrix(matrix) -> int:
    """"bt601" / "bt709" -> JPEGAMD_MATRIX_*; anything else is a ValueError."""
    if not isinstance(matrix, str) or matrix not in ("bt601", "bt709"):
        raise ValueError(f'matrix must be "bt601" or "bt709", not {matrix!r}')
    return MATRIX_BT709 if matrix == "bt709" else MATRIX_BT601


def encode_ycbcr_batch(y, cb, cr=None, quality: int = 0, subsampling: int = SUBSAMPLE_420, order: str = "cbcr",
                       sample_range: str = "full", matrix: str = "bt601", scan: str = "separate", restart_interval=None) -> list:
    """N pictures whose samples already ARE Y, Cb and Cr (JFIF full range; no range or matrix conversion is done) -> N colour JFIF
    files through jpegamd_encode_ycbcr_batch_async, read where they lie: no RGB detour, no chroma-plane pass.
    sample_range="limited": the samples are video range (Y 16..235, Cb / Cr 16..240, as decoders deliver them) and are expanded to
    full range as the kernel reads them (jpegamd_encode_ycbcr_range_batch_async: no pass over the planes); the matrix stays BT.601.
    matrix="bt709": the samples are BT.709 YCbCr (HD and UHD video) and are converted to JFIF's BT.601 by one pass in front of the tile
    kernel (jpegamd_encode_ycbcr_matrix_batch_async: the integer map of include/jpeg_compression.h, after the range map).
    `y` is a uint8 DEVICE tensor [N, H, W]; `cb` and `cr` are [N, ch, cw] with (ch, cw) = (H, W) at SUBSAMPLE_444,
    (ceil(H / 2), ceil(W / 2)) at SUBSAMPLE_420 (I420; YV12 by swapping them) and (H, ceil(W / 2)) at SUBSAMPLE_422 (I422).  With
    cr=None, `cb` is [N, ch, cw, 2]: byte pairs Cb Cr (NV12; NV16 at 4:2:2; NV24 at 4:4:4), or Cr Cb with order="crcb" (NV21 / NV61 /
    NV42).  Packed 4:2:2 frames (YUY2 / UYVY) go through encode_yuyv_batch.  Rows and pictures may be strided, samples within a row
    are packed.  Batches of more than MAX_BATCH pictures go as several calls; the per-device context of encode_tensor is used.
    An NV12 frame tensor `f` of shape [3 * H // 2, W] (H and W even: H rows of Y, then H / 2 rows of Cb Cr pairs) is

        y    = f[:H].unsqueeze(0)                                   # [1, H, W]
        cbcr = f[H:].view(H // 2, W // 2, 2).unsqueeze(0)           # [1, H / 2, W / 2, 2]
        jpegamd.encode_ycbcr_batch(y, cbcr)

    and a stack of frames [N, 3 * H // 2, W] slices the same way: f[:, :H] and f[:, H:].unflatten(2, (W // 2, 2)).
    scan="interleaved": the files with ONE scan of interleaved MCUs (jpegamd_encode_ycbcr_interleaved_batch_async), for
    sample_range="full" and matrix="bt601" alone; anything else is a ValueError here (jpegamd.mjpeg.encode_ycbcr_batch, _ycbcr16_batch
    and _yuyv_batch give the one-scan files of every kind).  restart_interval= (scan="interleaved" alone): restart
    intervals of that many MCUs, or "row", as for encode_tensor_batch (jpegamd_encode_ycbcr_interleaved_restart_batch_async)."""
    rng, mat = _sample_range(sample_range), _matrix(matrix)
    interleaved = _scan(scan)
    if interleaved and (rng != RANGE_FULL or mat != MATRIX_BT601):
        raise ValueError('scan="interleaved" takes sample_range="full" and matrix="bt601" alone')
    return _encode_ycbcr_planes("encode_ycbcr_batch", _ycbcr_layout, y, cb, cr, quality, subsampling, order, restart_interval,
                                rng, matrix=mat, interleaved=interleaved)


def _encode_ycbcr_planes(name: str, layout_of, y, cb, cr, quality, subsampling, order, restart_interval, sample_range: int,
                         sample_format: int = SAMPLES_8, matrix: int = MATRIX_BT601, interleaved: bool = False, **one_scan):
    """What the four planes-or-pairs functions (encode_ycbcr_batch, encode_ycbcr16_batch and their jpegamd.mjpeg twins) share behind
    their own checks: the layout (layout_of: _ycbcr_layout or _ycbcr16_layout), the restart interval, the device, the encode."""
    n, h, w, y_stride, c_stride, layout = layout_of(y, cb, cr, subsampling, order)
    ri = _restart(restart_interval, interleaved, w, subsampling)
    tensors = [y, cb] + ([cr] if cr is not None else [])
    if any(not x.is_cuda or x.device != y.device for x in tensors):
        raise ValueError(f"{name} needs device tensors on one device")
    return _encode_ycbcr_images(y.device, n, h, w, subsampling, lambda i: Encoder.ycbcr_image(
        y[i].data_ptr(), cb[i].data_ptr(), cr[i].data_ptr() if cr is not None else 0, w, h, y_stride, c_stride, layout, quality),
        sample_range, sample_format, matrix, interleaved, ri, **one_scan)


def _encode_ycbcr_images(device, n, h, w, subsampling, image, sample_range: int = RANGE_FULL, sample_format: int = SAMPLES_8,
                         matrix: int = MATRIX_BT601, interleaved: bool = False, restart: int = 0, any_kind: bool = False, huffman: int = 0,
                         progressive: bool = False):
    """`n` YCbCr pictures of one geometry, picture i described by image(i), through the per-device context in calls of at most
    MAX_BATCH -> their files.  `any_kind` (jpegamd.mjpeg): the interleaved files of whatever range, format, matrix and layout, through
    jpegamd_encode_ycbcr_interleaved_matrix_batch_async, with the tables `huffman` (set on the context for the call, STANDARD put back)."""
    if huffman and not any_kind:
        raise ValueError("optimised Huffman tables go through jpegamd.mjpeg")
    if progressive:                                               # (jpegamd.progressive: any kind, no intervals, the standard tables set for the call;
        bound, _, _, own = _progressive_mode(progressive)    # jpegamd.progressive_optimized, _successive: the context's mode is left alone)
        cap = bound(w, h, subsampling)

        def queue_progressive(enc, b0, k, outs, cap, size_ptrs, stream):
            _progressive_entry(enc, progressive, True)([image(b0 + i) for i in range(k)], subsampling, sample_range, sample_format, matrix, outs,
                                                       cap, size_ptrs, stream)

        return _encode_pictures(device, n, h, w, cap, queue_progressive, None if own else HUFFMAN_STANDARD)
    if restart:
        cap = max_jfif_bytes_interleaved_restart(w, h, subsampling, restart)
    else:
        cap = max_jfif_bytes_interleaved(w, h, subsampling) if interleaved else max_jfif_bytes_color(w, h, subsampling)

    def queue(enc, b0, k, outs, cap, size_ptrs, stream):
        _queue_ycbcr(enc, [image(b0 + i) for i in range(k)], subsampling, outs, cap, size_ptrs, stream, sample_range, sample_format,
                     matrix, interleaved, restart, any_kind)

    return _encode_pictures(device, n, h, w, cap, queue, huffman or None)


def _queue_ycbcr(enc, imgs, subsampling, outs, cap, size_ptrs, stream, sample_range: int = RANGE_FULL, sample_format: int = SAMPLES_8,
                 matrix: int = MATRIX_BT601, interleaved: bool = False, restart: int = 0, any_kind: bool = False):
    """One call of _encode_ycbcr_images queued on `enc`: which entry takes `imgs` (YCbCrImage structs of one geometry).  `any_kind`:
    the one-scan entry of every range, format and matrix; otherwise the one-scan entries of full-range 8-bit BT.601 samples, with
    or without restart intervals; otherwise the three-scan entries (encode_ycbcr_batch_async picks among them)."""
    if any_kind:
        enc.encode_ycbcr_interleaved_matrix_batch_async(imgs, subsampling, sample_range, sample_format, matrix, restart, outs, cap,
                                                        size_ptrs, stream)
    elif restart:
        enc.encode_ycbcr_interleaved_restart_batch_async(imgs, subsampling, restart, outs, cap, size_ptrs, stream)
    elif interleaved:
        enc.encode_ycbcr_interleaved_batch_async(imgs, subsampling, outs, cap, size_ptrs, stream)
    else:
        enc.encode_ycbcr_batch_async(imgs, subsampling, outs, cap, size_ptrs, stream, sample_range, sample_format=sample_format,
                                     matrix=matrix)


def encode_ycbcr16_batch(y, cb, cr=None, quality: int = 0, subsampling: int = SUBSAMPLE_420, order: str = "cbcr",
                         sample_range: str = "full", align: str = "msb", matrix: str = "bt601") -> list:
    """N pictures of 10-bit Y, Cb and Cr samples in 16-bit words (a Main10 / AV1 10-bit decoder's frames) -> N colour JFIF files through
    jpegamd_encode_ycbcr_samples_batch_async, read where they lie: every sample is narrowed to 8 bits as the kernel reads it (no pass
    over the planes), with ONE rounding from ten bits for either sample_range ("full" / "limited": Y 64..940, Cb / Cr 64..960).
    align="msb": the value sits in the high ten bits of the word and the low six are ignored (P010 / P210 / P410); align="lsb": in the
    low ten bits, larger words clamp to 1023 (I010 / yuv420p10le).  The tensors are torch.int16 or torch.uint16 DEVICE tensors -- the
    bit pattern is what counts -- shaped as encode_ycbcr_batch's: `y` [N, H, W], `cb` and `cr` [N, ch, cw], or with cr=None `cb` as
    [N, ch, cw, 2] pairs of words Cb Cr (Cr Cb with order="crcb").  Rows and pictures may be strided, samples within a row are packed.
    Batches of more than MAX_BATCH pictures go as several calls; the per-device context of encode_tensor is used.
    matrix="bt709": BT.709 samples, converted to BT.601 by one pass as in encode_ycbcr_batch; the pass narrows each sample by the same
    map first and applies the matrix to the 8-bit results."""
    rng, mat = _sample_range(sample_range), _matrix(matrix)
    if not isinstance(align, str) or align not in ("msb", "lsb"):
        raise ValueError(f'align must be "msb" or "lsb", not {align!r}')
    return _encode_ycbcr_planes("encode_ycbcr16_batch", _ycbcr16_layout, y, cb, cr, quality, subsampling, order, None, rng,
                                SAMPLES_10_MSB if align == "msb" else SAMPLES_10_LSB, mat)


def _yuyv_layout(frames, order):
    """The pictures of encode_yuyv_batch -> (count, height, width, row stride, JPEGAMD_CHROMA_* layout).  Shapes, dtypes and strides
    only: host tensors pass."""
    import torch
    if order not in ("yuyv", "uyvy"):
        raise ValueError(f'order must be "yuyv" or "uyvy", not {order!r}')
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8:
        raise ValueError("the encoder needs a uint8 tensor")
    if frames.dim() != 4 or frames.shape[3] != 2:
        raise ValueError("frames must be [N, H, W, 2]: two bytes per pixel")
    n, h, w = frames.shape[0], frames.shape[1], frames.shape[2]
    if n < 1 or h < 1 or w < 1 or h > 65535 or w > 65535:
        raise ValueError("the encoder needs at least one picture of 1..65535 pixels each way")
    if w % 2:
        raise ValueError("a [N, H, W, 2] frame holds whole 4-byte groups of two pixels: W must be even")
    if frames.stride(3) != 1 or frames.stride(2) != 2:
        raise ValueError("the pixels of a row must be packed (pixel stride 2, last stride 1)")
    stride = frames.stride(1) if h > 1 else 2 * w
    if stride < 2 * w:
        raise ValueError("rows overlap (the row stride is less than a row)")
    return n, h, w, stride, (CHROMA_YUYV if order == "yuyv" else CHROMA_UYVY)


def encode_yuyv_batch(frames, quality: int = 0, order: str = "yuyv", sample_range: str = "full", matrix: str = "bt601") -> list:
    """N packed 4:2:2 frames -> N colour JFIF files at SUBSAMPLE_422 through jpegamd_encode_ycbcr_batch_async, read where they
    lie: the samples are coded as given (JFIF full range; no range or matrix conversion, no filter).
    `frames` is a uint8 DEVICE tensor [N, H, W, 2], W even: groups of four bytes Y0 Cb Y1 Cr for two pixels (YUY2), or Cb Y0 Cr Y1
    with order="uyvy".  Rows and pictures may be strided; the two bytes of a pixel and the pixels of a row are packed.  Batches of
    more than MAX_BATCH frames go as several calls; the per-device context of encode_tensor is used.  sample_range="limited": video-range
    samples, expanded to full range on read as in encode_ycbcr_batch.  matrix="bt709": BT.709 samples, converted to BT.601 by one pass as
    in encode_ycbcr_batch."""
    rng, mat = _sample_range(sample_range), _matrix(matrix)
    return _encode_yuyv_frames(frames, quality, order, None, rng, mat)


def _encode_yuyv_frames(frames, quality, order, restart_interval, sample_range: int, matrix: int, interleaved: bool = False, **one_scan):
    """What encode_yuyv_batch and its jpegamd.mjpeg twin share behind their own checks, as _encode_ycbcr_planes."""
    n, h, w, stride, layout = _yuyv_layout(frames, order)
    ri = _restart(restart_interval, interleaved, w, SUBSAMPLE_422)
    if not frames.is_cuda:
        raise ValueError("encode_yuyv_batch needs a device tensor")
    return _encode_ycbcr_images(frames.device, n, h, w, SUBSAMPLE_422, lambda i: Encoder.ycbcr_image(
        frames[i].data_ptr(), 0, 0, w, h, stride, 0, layout, quality), sample_range, matrix=matrix, interleaved=interleaved, restart=ri,
        **one_scan)


FLOAT_LAYOUTS = ("chw", "hwc", "rgba", "bgra", "gray")
FLOAT_SCALE_MAX = 16777216.0                                     # |scale| of a float call is at most this (include/jpeg_compression.h)


def _value_range(value_range):
    """value_range=(lo, hi) of the float functions -> (scale, offset) of the C entries: float32(255 / (hi - lo)) and
    float32(-lo * 255 / (hi - lo)), computed in double and rounded once.  (0, 1) -> (255, 0); (-1, 1) -> (127.5, 127.5);
    (0, 255) -> (1, 0).  hi < lo inverts the picture.  Anything that is no pair of distinct finite numbers, or a range so narrow that
    |scale| passes FLOAT_SCALE_MAX, is a ValueError."""
    import math
    try:
        lo, hi = value_range
        lo, hi = float(lo), float(hi)
    except (TypeError, ValueError):
        raise ValueError(f"value_range must be a pair of numbers (lo, hi), not {value_range!r}") from None
    if not (math.isfinite(lo) and math.isfinite(hi)) or lo == hi:
        raise ValueError(f"value_range must be two distinct finite numbers, not {value_range!r}")
    scale = 255.0 / (hi - lo)
    scale32, offset32 = C.c_float(scale).value, C.c_float(-lo * scale + 0.0).value
    if not (math.isfinite(scale32) and math.isfinite(offset32)) or abs(scale32) > FLOAT_SCALE_MAX:
        raise ValueError(f"value_range {value_range!r} gives a scale or offset outside what the encoder takes (|scale| <= {FLOAT_SCALE_MAX:.0f})")
    return scale32, offset32


def _float_layout(t, layout, single: bool, byte: bool = False):
    """The float pictures (`byte`: the uint8 pictures, sample type 0, of the reduced functions) of `t` stored as `layout` says -> (count, height, width, row stride, pixel stride -- both in BYTES --,
    FLOAT_* sample type, channels, picture index -> the (R, G, B) pointers of JpegAmdFloatImage, the channel views).
    layout: "chw" [N, 3, H, W], "hwc" [N, H, W, 3], "rgba" / "bgra" [N, H, W, 4] (the fourth sample ignored), "gray" [N, H, W] (one
    channel: the luma itself), or `t` a sequence of three [N, H, W] tensors, the R, G and B planes; `single`: without the N.  Every
    stride that one row stride and one pixel stride describe is taken as it is -- channels_last, crops, t[::2], strided rows -- and
    nothing is copied.  Shapes, dtypes and strides only: host tensors pass."""
    import torch
    types = {torch.uint8: 0} if byte else {torch.float32: FLOAT_F32, torch.float16: FLOAT_F16, torch.bfloat16: FLOAT_BF16}
    planes = list(t) if isinstance(t, (tuple, list)) else None
    if planes is None and (not isinstance(layout, str) or layout not in FLOAT_LAYOUTS):
        raise ValueError(f"layout must be one of {FLOAT_LAYOUTS}, or the pictures a sequence of three plane tensors, not {layout!r}")
    if planes is not None and len(planes) != 3:
        raise ValueError("a sequence of tensors is the R, G and B planes: three of them")
    tensors = planes if planes is not None else [t]
    if any(not isinstance(x, torch.Tensor) or x.dtype not in types for x in tensors) or len({x.dtype for x in tensors}) != 1:
        raise ValueError("the reduced encoder needs uint8 tensors" if byte else
                         "the float encoder needs float32, float16 or bfloat16 tensors of one dtype")
    lead = 0 if single else 1                                  # dimensions in front of a picture
    if planes is not None:
        if any(p.dim() != lead + 2 or p.shape != planes[0].shape for p in planes):
            raise ValueError("the three planes must be [H, W] or [N, H, W] tensors of one shape")
    elif layout == "gray":
        if t.dim() != lead + 2:
            raise ValueError('layout="gray" takes [H, W] or [N, H, W]')
        planes = [t]
    elif layout == "chw":
        if t.dim() != lead + 3 or t.shape[lead] != 3:
            raise ValueError('layout="chw" takes [3, H, W] or [N, 3, H, W]')
        planes = [t.select(lead, k) for k in range(3)]
    else:
        c = 3 if layout == "hwc" else 4
        if t.dim() != lead + 3 or t.shape[-1] != c:
            raise ValueError(f'layout="{layout}" takes [H, W, {c}] or [N, H, W, {c}]')
        planes = [t.select(lead + 2, k) for k in ((2, 1, 0) if layout == "bgra" else (0, 1, 2))]
    if single:
        planes = [p.unsqueeze(0) for p in planes]
    n, h, w = (int(v) for v in planes[0].shape)
    if n < 1 or h < 1 or w < 1 or h > 65535 or w > 65535:
        raise ValueError("the encoder needs at least one picture of 1..65535 pixels each way")
    size = planes[0].element_size()
    pixel = {p.stride(2) if w > 1 else 1 for p in planes}
    if len(pixel) != 1:
        raise ValueError("the planes of a picture must share one pixel stride")
    pixel = pixel.pop()
    if pixel < 1:
        raise ValueError(f"the samples of a row must lie at a positive stride, not {pixel} (expanded or flipped views are not taken)")
    rows = {p.stride(1) if h > 1 else pixel * w for p in planes}
    if len(rows) != 1:
        raise ValueError("the planes of a picture must share one row stride")
    row = rows.pop()
    if row < pixel * w:
        raise ValueError(f"rows overlap or run backwards (the row stride {row} is less than a row of {pixel * w} samples)")
    if row * size >= 1 << 31:
        raise ValueError("a row stride must stay below 2^31 bytes")
    return n, h, w, row * size, pixel * size, types[planes[0].dtype], len(planes), (lambda i: tuple(p[i].data_ptr() for p in planes)), planes


def _encode_float(name: str, t, quality, subsampling, layout, value_range, single: bool, interleaved: bool = False, restart_interval=None,
                  huffman=None, progressive: bool = False, scans=None) -> list:
    """What the float functions of jpegamd, jpegamd.mjpeg and jpegamd.progressive_script share: every argument checked on the CPU,
    then the pictures through the per-device context in calls of at most MAX_BATCH.  One channel (layout="gray") is a grayscale file
    whatever `subsampling` says."""
    scale, offset = _value_range(value_range)
    huff = None if huffman is None else _huffman(huffman)
    n, h, w, row, pixel, sample_type, channels, ptr, planes = _float_layout(t, layout, single)
    sub = 0 if channels == 1 else subsampling
    if sub not in (0, SUBSAMPLE_444, SUBSAMPLE_420, SUBSAMPLE_422):
        raise ValueError("subsampling must be SUBSAMPLE_444, SUBSAMPLE_420, SUBSAMPLE_422 or 0 (a grayscale file)")
    ri = _restart(restart_interval, interleaved, w, sub or SUBSAMPLE_444)      # (a grayscale scan: "row" is ceil(W / 8))
    if progressive:
        cap = max_jfif_bytes_progressive_script(w, h, sub, scans)
        if not cap:
            if scans is not None:
                validate_scan_script(scans, 1 if sub == 0 else 3)
            raise ValueError("bad dimensions")
    elif interleaved:
        cap = max_jfif_bytes_gray_scan(w, h, ri) if sub == 0 else max_jfif_bytes_interleaved_restart(w, h, sub, ri)
    else:
        cap = max_jfif_bytes(w, h) if sub == 0 else max_jfif_bytes_color(w, h, sub)
    if any(not p.is_cuda or p.device != planes[0].device for p in planes):
        raise ValueError(f"{name} needs device tensors on one device")

    def queue(enc, b0, k, outs, cap, size_ptrs, stream):
        imgs = [Encoder.float_image(ptr(b0 + i), w, h, row, pixel, quality) for i in range(k)]
        if progressive:
            enc.encode_float_progressive_script_batch_async(imgs, sub, sample_type, scale, offset, scans, outs, cap, size_ptrs, stream)
        elif interleaved:
            enc.encode_float_interleaved_batch_async(imgs, sub, sample_type, scale, offset, ri, outs, cap, size_ptrs, stream)
        else:
            enc.encode_float_batch_async(imgs, sub, sample_type, scale, offset, outs, cap, size_ptrs, stream)

    return _encode_pictures(planes[0].device, n, h, w, cap, queue, huff)


def encode_float_batch(t, quality: int = 0, subsampling: int = SUBSAMPLE_420, layout="chw", value_range=(0.0, 1.0)) -> list:
    """A float32, float16 or bfloat16 DEVICE tensor of N pictures -> N JFIF files through jpegamd_encode_float_batch_async: one kernel
    reads every sample once, where it lies, and makes the byte x.float().mul(scale).add(offset).round().clamp(0, 255) of it (NaN -> 0;
    include/jpeg_compression.h has the definition), with (scale, offset) = (255 / (hi - lo), -lo * scale) of value_range=(lo, hi):
    (0, 1), (-1, 1), (0, 255).  The files are byte for byte those of encode_tensor_batch for the uint8 tensor of these bytes: no
    conversion pass of the caller's, no byte tensor.
    layout: "chw" [N, 3, H, W] (also in torch.channels_last memory), "hwc" [N, H, W, 3], "rgba" / "bgra" [N, H, W, 4], "gray"
    [N, H, W] -- one channel, the luma itself: a grayscale file --, or `t` a sequence of three [N, H, W] plane tensors.  subsampling 0:
    the grayscale file of the pictures' luma.  Crops, strided rows and t[::2] are read as they are; what one row stride and one pixel
    stride cannot describe is a ValueError.  Batches of more than MAX_BATCH pictures go as several calls; the per-device context of
    encode_tensor is used, with the tables and metadata of a quant_tables / metadata block."""
    return _encode_float("encode_float_batch", t, quality, subsampling, layout, value_range, False)


def encode_float(t, quality: int = 0, subsampling: int = SUBSAMPLE_420, layout="chw", value_range=(0.0, 1.0)) -> bytes:
    """One float picture -> its file, as encode_float_batch: [3, H, W], [H, W, 3], [H, W, 4], [H, W] or three [H, W] planes."""
    return _encode_float("encode_float", t, quality, subsampling, layout, value_range, True)[0]


def reduced_size(width: int, height: int, factor: int) -> tuple:
    """(ow, oh) = (ceil(width / factor), ceil(height / factor)) of a reduced picture (jpegamd_reduced_size): what the files of the
    reduced functions measure and what their buffers are sized for.  A ValueError outside 1..65535 and 1..MAX_REDUCE."""
    ow, oh = C.c_int32(0), C.c_int32(0)
    try:
        rc = lib.jpegamd_reduced_size(width, height, factor, C.byref(ow), C.byref(oh))
    except (C.ArgumentError, TypeError):
        rc = -1
    if rc:
        raise ValueError(f"reduced_size takes a width and height of 1..65535 and a factor of 1..{MAX_REDUCE}, not {(width, height, factor)!r}")
    return ow.value, oh.value


def _encode_reduced(name: str, t, quality, subsampling, factor, layout, single: bool, interleaved: bool = False, restart_interval=None,
                    huffman=None, progressive: bool = False, scans=None) -> list:
    """What the reduced functions of jpegamd, jpegamd.mjpeg and jpegamd.progressive_script share, as _encode_float: every argument
    checked on the CPU, then the pictures through the per-device context -- sized for the REDUCED pictures -- in calls of at most
    MAX_BATCH.  One channel (layout="gray") is a grayscale file whatever `subsampling` says."""
    huff = None if huffman is None else _huffman(huffman)
    if isinstance(factor, bool) or not isinstance(factor, int) or not 1 <= factor <= MAX_REDUCE:
        raise ValueError(f"factor must be an integer of 1..{MAX_REDUCE}, not {factor!r}")
    n, h, w, row, pixel, _, channels, ptr, planes = _float_layout(t, layout, single, byte=True)
    ow, oh = reduced_size(w, h, factor)
    sub = 0 if channels == 1 else subsampling
    if sub not in (0, SUBSAMPLE_444, SUBSAMPLE_420, SUBSAMPLE_422):
        raise ValueError("subsampling must be SUBSAMPLE_444, SUBSAMPLE_420, SUBSAMPLE_422 or 0 (a grayscale file)")
    ri = _restart(restart_interval, interleaved, ow, sub or SUBSAMPLE_444)     # ("row": an MCU row of the REDUCED picture)
    if progressive:
        cap = max_jfif_bytes_progressive_script(ow, oh, sub, scans)
        if not cap:
            if scans is not None:
                validate_scan_script(scans, 1 if sub == 0 else 3)
            raise ValueError("bad dimensions")
    elif interleaved:
        cap = max_jfif_bytes_gray_scan(ow, oh, ri) if sub == 0 else max_jfif_bytes_interleaved_restart(ow, oh, sub, ri)
    else:
        cap = max_jfif_bytes(ow, oh) if sub == 0 else max_jfif_bytes_color(ow, oh, sub)
    if any(not p.is_cuda or p.device != planes[0].device for p in planes):
        raise ValueError(f"{name} needs device tensors on one device")

    def queue(enc, b0, k, outs, cap, size_ptrs, stream):
        imgs = [Encoder.strided_image(ptr(b0 + i), w, h, row, pixel, quality) for i in range(k)]
        if progressive:
            enc.encode_reduced_progressive_script_batch_async(imgs, sub, factor, scans, outs, cap, size_ptrs, stream)
        elif interleaved:
            enc.encode_reduced_interleaved_batch_async(imgs, sub, factor, ri, outs, cap, size_ptrs, stream)
        else:
            enc.encode_reduced_batch_async(imgs, sub, factor, outs, cap, size_ptrs, stream)

    return _encode_pictures(planes[0].device, n, oh, ow, cap, queue, huff)


def encode_reduced_batch(t, quality: int = 0, subsampling: int = SUBSAMPLE_420, factor: int = 2, layout="chw") -> list:
    """A uint8 DEVICE tensor of N pictures -> N JFIF files of ceil(W / factor) x ceil(H / factor) pixels through
    jpegamd_encode_reduced_batch_async: one kernel reads every byte once, where it lies, and makes every reduced sample the rounded mean
    (S + (n >> 1)) // n of its factor x factor box -- of what of the box lies inside the picture; include/jpeg_compression.h has the
    definition.  The files are byte for byte those of encode_tensor_batch for the uint8 tensor of those means: no resize of the
    caller's, no float copy, no reduced tensor.  The mean is of the stored (gamma-encoded) bytes.
    factor: 1..MAX_REDUCE; 1 reduces nothing and encodes a uint8 tensor at any row and pixel stride.  layout, the three-plane form,
    subsampling 0, crops, strided rows, t[::2] and channels_last memory as for encode_float_batch; the per-device context of
    encode_tensor is used, with the tables and metadata of a quant_tables / metadata block."""
    return _encode_reduced("encode_reduced_batch", t, quality, subsampling, factor, layout, False)


def encode_reduced(t, quality: int = 0, subsampling: int = SUBSAMPLE_420, factor: int = 2, layout="chw") -> bytes:
    """One picture of bytes -> its reduced file, as encode_reduced_batch: [3, H, W], [H, W, 3], [H, W, 4], [H, W] or three [H, W] planes."""
    return _encode_reduced("encode_reduced", t, quality, subsampling, factor, layout, True)[0]


MAX_RESIZE_RATIO = 64                                        # JPEGAMD_MAX_RESIZE_RATIO: source over target, each way


def resize_check(width: int, height: int, out_width: int, out_height: int) -> None:
    """What the resized functions take (jpegamd_resize_check): a source of 1..65535 each way and a target that is no larger than it
    and no smaller than 1/MAX_RESIZE_RATIO of it, each way.  A ValueError otherwise."""
    try:
        rc = lib.jpegamd_resize_check(width, height, out_width, out_height)
    except (C.ArgumentError, TypeError):
        rc = -1
    if rc:
        raise ValueError(f"a resized picture needs a source of 1..65535 each way and a target of 1 <= out_width <= width <= "
                         f"{MAX_RESIZE_RATIO} * out_width (the same for the heights), not {(width, height)!r} -> {(out_width, out_height)!r}")


def fit_size(w: int, h: int, max_w: int, max_h: int) -> tuple:
    """The largest size of the picture's shape inside max_w x max_h, in integers: (w, h) itself where it fits; else the side that
    binds becomes the bound and the other is rounded half up, at least 1.  Python only; resize_check still judges the result."""
    if any(isinstance(v, bool) or not isinstance(v, int) or v < 1 for v in (w, h, max_w, max_h)):
        raise ValueError(f"fit_size takes four positive integers, not {(w, h, max_w, max_h)!r}")
    if w <= max_w and h <= max_h:
        return w, h
    if w * max_h >= h * max_w:
        return max_w, max(1, (h * max_w + w // 2) // w)
    return max(1, (w * max_h + h // 2) // h), max_h


def _encode_resized(name: str, t, quality, subsampling, size, layout, single: bool, interleaved: bool = False, restart_interval=None,
                    huffman=None, progressive: bool = False, scans=None) -> list:
    """What the resized functions of jpegamd, jpegamd.mjpeg and jpegamd.progressive_script share, as _encode_reduced: every argument
    checked on the CPU, then the pictures through the per-device context -- sized for the RESIZED pictures -- in calls of at most
    MAX_BATCH.  One channel (layout="gray") is a grayscale file whatever `subsampling` says."""
    huff = None if huffman is None else _huffman(huffman)
    if (not isinstance(size, (tuple, list)) or len(size) != 2 or
            any(isinstance(v, bool) or not isinstance(v, int) for v in size)):
        raise ValueError(f"size must be (out_width, out_height), two integers, not {size!r}")
    ow, oh = size
    n, h, w, row, pixel, _, channels, ptr, planes = _float_layout(t, layout, single, byte=True)
    resize_check(w, h, ow, oh)
    sub = 0 if channels == 1 else subsampling
    if sub not in (0, SUBSAMPLE_444, SUBSAMPLE_420, SUBSAMPLE_422):
        raise ValueError("subsampling must be SUBSAMPLE_444, SUBSAMPLE_420, SUBSAMPLE_422 or 0 (a grayscale file)")
    ri = _restart(restart_interval, interleaved, ow, sub or SUBSAMPLE_444)     # ("row": an MCU row of the RESIZED picture)
    if progressive:
        cap = max_jfif_bytes_progressive_script(ow, oh, sub, scans)
        if not cap:
            if scans is not None:
                validate_scan_script(scans, 1 if sub == 0 else 3)
            raise ValueError("bad dimensions")
    elif interleaved:
        cap = max_jfif_bytes_gray_scan(ow, oh, ri) if sub == 0 else max_jfif_bytes_interleaved_restart(ow, oh, sub, ri)
    else:
        cap = max_jfif_bytes(ow, oh) if sub == 0 else max_jfif_bytes_color(ow, oh, sub)
    if any(not p.is_cuda or p.device != planes[0].device for p in planes):
        raise ValueError(f"{name} needs device tensors on one device")

    def queue(enc, b0, k, outs, cap, size_ptrs, stream):
        imgs = [Encoder.strided_image(ptr(b0 + i), w, h, row, pixel, quality) for i in range(k)]
        if progressive:
            enc.encode_resized_progressive_script_batch_async(imgs, sub, ow, oh, scans, outs, cap, size_ptrs, stream)
        elif interleaved:
            enc.encode_resized_interleaved_batch_async(imgs, sub, ow, oh, ri, outs, cap, size_ptrs, stream)
        else:
            enc.encode_resized_batch_async(imgs, sub, ow, oh, outs, cap, size_ptrs, stream)

    return _encode_pictures(planes[0].device, n, oh, ow, cap, queue, huff)


def encode_resized_batch(t, quality: int = 0, subsampling: int = SUBSAMPLE_420, size=None, layout="chw") -> list:
    """A uint8 DEVICE tensor of N pictures -> N JFIF files of size = (out_width, out_height) pixels through
    jpegamd_encode_resized_batch_async: one kernel makes every sample of the target the exact area mean of the source -- every source
    byte weighted by the share of it inside the target sample's footprint, rounded half up; include/jpeg_compression.h has the
    definition.  The files are byte for byte those of encode_tensor_batch for the uint8 tensor of those means: no resize of the
    caller's, no float copy, no resized tensor.  The mean is of the stored (gamma-encoded) bytes.
    size: no larger than the source and no smaller than 1/MAX_RESIZE_RATIO of it, each way (resize_check); fit_size gives the size
    that fits a box.  layout, the three-plane form, subsampling 0, crops, strided rows, t[::2] and channels_last memory as for
    encode_reduced_batch; the per-device context of encode_tensor is used, with the tables and metadata of a quant_tables / metadata
    block."""
    return _encode_resized("encode_resized_batch", t, quality, subsampling, size, layout, False)


def encode_resized(t, quality: int = 0, subsampling: int = SUBSAMPLE_420, size=None, layout="chw") -> bytes:
    """One picture of bytes -> its resized file, as encode_resized_batch: [3, H, W], [H, W, 3], [H, W, 4], [H, W] or three [H, W] planes."""
    return _encode_resized("encode_resized", t, quality, subsampling, size, layout, True)[0]


def encode_files(in_paths, out_paths, quality: int = 0):
    """File-to-file batch with overlapped I/O and transfers (jpegamd_encode_files) -> (return code, [status per file], BatchStats)."""
    n = len(in_paths)
    if len(out_paths) != n:
        raise ValueError("in_paths and out_paths differ in length")
    ins = (C.c_char_p * n)(*[str(p).encode() for p in in_paths])
    outs = (C.c_char_p * n)(*[str(p).encode() for p in out_paths])
    status = (C.c_int32 * n)()
    st = BatchStats()
    rc = lib.jpegamd_encode_files(ins, outs, n, quality, status, C.byref(st))
    return int(rc), list(status), st


class _ProgressiveEntries:
    """The progressive entries of a context, a base of Encoder: they take the context's handle and its batch
    marshaller as every other batch method does."""

    def encode_color_progressive_batch_async(self, imgs, subsampling: int, out_ptrs, out_cap: int, size_ptrs, stream: int = 0):
        """The progressive files (SOF2, seven scans by spectral selection) of RGB / BGR / RGBA / BGRA pictures
        (jpegamd_encode_color_progressive_batch_async); out_cap from max_jfif_bytes_progressive.  The context's Huffman mode must be
        HUFFMAN_STANDARD."""
        self._batch("jpegamd_encode_color_progressive_batch_async", Image, imgs, (subsampling,), out_ptrs, out_cap, size_ptrs, stream)

    def encode_ycbcr_progressive_batch_async(self, imgs, subsampling: int, sample_range: int, sample_format: int, matrix: int,
                                             out_ptrs, out_cap: int, size_ptrs, stream: int = 0):
        """The progressive files of YCbCr pictures of any kind encode_ycbcr_interleaved_matrix_batch_async takes
        (jpegamd_encode_ycbcr_progressive_batch_async)."""
        self._batch("jpegamd_encode_ycbcr_progressive_batch_async", YCbCrImage, imgs, (subsampling, sample_range, sample_format, matrix),
                    out_ptrs, out_cap, size_ptrs, stream)

    def encode_color_progressive_optimized_batch_async(self, imgs, subsampling: int, out_ptrs, out_cap: int, size_ptrs, stream: int = 0):
        """The progressive files with end-of-band runs and per-scan optimised tables of the same pictures
        (jpegamd_encode_color_progressive_optimized_batch_async); out_cap from max_jfif_bytes_progressive_optimized.  The context's
        Huffman mode is neither read nor changed."""
        self._batch("jpegamd_encode_color_progressive_optimized_batch_async", Image, imgs, (subsampling,), out_ptrs, out_cap, size_ptrs, stream)

    def encode_ycbcr_progressive_optimized_batch_async(self, imgs, subsampling: int, sample_range: int, sample_format: int, matrix: int,
                                                       out_ptrs, out_cap: int, size_ptrs, stream: int = 0):
        """... of YCbCr pictures of any kind (jpegamd_encode_ycbcr_progressive_optimized_batch_async)."""
        self._batch("jpegamd_encode_ycbcr_progressive_optimized_batch_async", YCbCrImage, imgs,
                    (subsampling, sample_range, sample_format, matrix), out_ptrs, out_cap, size_ptrs, stream)

    def encode_color_progressive_successive_batch_async(self, imgs, subsampling: int, out_ptrs, out_cap: int, size_ptrs, stream: int = 0):
        """The progressive files with successive approximation -- the ten scans of libjpeg's default script, a table per scan
         -- of the same pictures (jpegamd_encode_color_progressive_successive_batch_async); out_cap from
        max_jfif_bytes_progressive_successive.  The context's Huffman mode is neither read nor changed."""
        self._batch("jpegamd_encode_color_progressive_successive_batch_async", Image, imgs, (subsampling,), out_ptrs, out_cap, size_ptrs, stream)

    def encode_ycbcr_progressive_successive_batch_async(self, imgs, subsampling: int, sample_range: int, sample_format: int, matrix: int,
                                                        out_ptrs, out_cap: int, size_ptrs, stream: int = 0):
        """... of YCbCr pictures of any kind (jpegamd_encode_ycbcr_progressive_successive_batch_async)."""
        self._batch("jpegamd_encode_ycbcr_progressive_successive_batch_async", YCbCrImage, imgs,
                    (subsampling, sample_range, sample_format, matrix), out_ptrs, out_cap, size_ptrs, stream)


class _ProgressiveScriptEntries(_ProgressiveEntries):
    """... and those that take a scan script.  `scans`: None for the default script, or a sequence of (components,
    Ss, Se, Ah, Al) with components a tuple of component indices; out_cap from max_jfif_bytes_progressive_script."""

    def _script_batch(self, name: str, struct, imgs, ints, scans, out_ptrs, out_cap: int, size_ptrs, stream: int):
        n = len(imgs)
        arr, pointers = (struct * n)(*imgs), C.c_void_p * n
        sc, ns = _scan_array(scans)
        rc = getattr(lib, name)(self._h, arr, n, *[int(v) for v in ints], sc, ns, pointers(*out_ptrs), out_cap, pointers(*size_ptrs),
                                C.c_void_p(stream))
        if rc:
            raise JpegAmdError(rc, name)

    def encode_color_progressive_script_batch_async(self, imgs, subsampling: int, scans, out_ptrs, out_cap: int, size_ptrs, stream: int = 0):
        """The progressive files of RGB / BGR / RGBA / BGRA pictures with the caller's scan script
        (jpegamd_encode_color_progressive_script_batch_async).  The context's Huffman mode is neither read nor changed."""
        self._script_batch("jpegamd_encode_color_progressive_script_batch_async", Image, imgs, (subsampling,), scans, out_ptrs, out_cap, size_ptrs, stream)

    def encode_ycbcr_progressive_script_batch_async(self, imgs, subsampling: int, sample_range: int, sample_format: int, matrix: int, scans,
                                                    out_ptrs, out_cap: int, size_ptrs, stream: int = 0):
        """... of YCbCr pictures of any kind (jpegamd_encode_ycbcr_progressive_script_batch_async)."""
        self._script_batch("jpegamd_encode_ycbcr_progressive_script_batch_async", YCbCrImage, imgs,
                           (subsampling, sample_range, sample_format, matrix), scans, out_ptrs, out_cap, size_ptrs, stream)

    def encode_gray_progressive_script_batch_async(self, imgs, scans, out_ptrs, out_cap: int, size_ptrs, stream: int = 0):
        """The grayscale progressive files (SOF2, one component) of pictures in any of the five channel orders: their luma
        (jpegamd_encode_gray_progressive_script_batch_async); out_cap from max_jfif_bytes_progressive_script with subsampling 0."""
        self._script_batch("jpegamd_encode_gray_progressive_script_batch_async", Image, imgs, (), scans, out_ptrs, out_cap, size_ptrs, stream)


class _FloatEntries(_ProgressiveScriptEntries):
    """... and the entries of float pictures: float32 / float16 / bfloat16 samples, each made a byte by
    x * scale + offset, rounded half to even and clamped, by one kernel in front of the tile encoder."""

    @staticmethod
    def float_image(planes, width: int, height: int, row_stride: int, pixel_stride: int, quality: int = 0) -> FloatImage:
        """`planes`: the device pointers of the first R, G and B sample -- (p, 0, 0) or (p,): one channel, the luma -- with rows
        `row_stride` and the samples of a row `pixel_stride` BYTES apart."""
        r, g, b = (tuple(planes) + (0, 0))[:3]
        return FloatImage((C.c_void_p * 3)(r or None, g or None, b or None), width, height, row_stride, pixel_stride, quality)

    def _float_batch(self, name: str, imgs, subsampling: int, sample_type: int, scale: float, offset: float, middle, out_ptrs, out_cap: int,
                     size_ptrs, stream: int):
        """A float entry: name(context, pictures[], count, subsampling, sample type, scale, offset, middle..., outs[], out_cap,
        sizes[], stream)."""
        n = len(imgs)
        arr, pointers = (FloatImage * n)(*imgs), C.c_void_p * n
        rc = getattr(lib, name)(self._h, arr, n, int(subsampling), int(sample_type), C.c_float(scale), C.c_float(offset), *middle,
                                pointers(*out_ptrs), out_cap, pointers(*size_ptrs), C.c_void_p(stream))
        if rc:
            raise JpegAmdError(rc, name)

    def encode_float_batch_async(self, imgs, subsampling: int, sample_type: int, scale: float, offset: float, out_ptrs, out_cap: int,
                                 size_ptrs, stream: int = 0):
        """The files of `len(imgs)` float pictures of one geometry (float_image; FLOAT_F32 / FLOAT_F16 / FLOAT_BF16 samples, each made a
        byte by x * scale + offset, rounded half to even and clamped) in three scans, or for subsampling 0 the grayscale file
        (jpegamd_encode_float_batch_async); the context, out_cap and the files as for encode_planar_batch_async on those bytes."""
        self._float_batch("jpegamd_encode_float_batch_async", imgs, subsampling, sample_type, scale, offset, (), out_ptrs, out_cap, size_ptrs, stream)

    def encode_float_interleaved_batch_async(self, imgs, subsampling: int, sample_type: int, scale: float, offset: float, restart_interval: int,
                                             out_ptrs, out_cap: int, size_ptrs, stream: int = 0):
        """... in ONE scan, with restart intervals of `restart_interval` MCUs (0: none) and the context's Huffman tables; subsampling
        0: the grayscale file of encode_gray_scan_batch_async (jpegamd_encode_float_interleaved_batch_async)."""
        self._float_batch("jpegamd_encode_float_interleaved_batch_async", imgs, subsampling, sample_type, scale, offset, (int(restart_interval),),
                          out_ptrs, out_cap, size_ptrs, stream)

    def encode_float_progressive_script_batch_async(self, imgs, subsampling: int, sample_type: int, scale: float, offset: float, scans,
                                                    out_ptrs, out_cap: int, size_ptrs, stream: int = 0):
        """... as progressive files with the scan script `scans` (None: the default one); subsampling 0: the grayscale progressive
        file (jpegamd_encode_float_progressive_script_batch_async)."""
        sc, ns = _scan_array(scans)
        self._float_batch("jpegamd_encode_float_progressive_script_batch_async", imgs, subsampling, sample_type, scale, offset, (sc, ns),
                          out_ptrs, out_cap, size_ptrs, stream)


class _ReducedEntries(_FloatEntries):
    """... and the entries of reduced pictures: bytes at any row and pixel stride, averaged in factor x factor
    boxes by one kernel in front of the tile encoder; the files measure reduced_size(width, height, factor)."""

    @staticmethod
    def strided_image(planes, width: int, height: int, row_stride: int, pixel_stride: int, quality: int = 0) -> StridedImage:
        """`planes`: the device pointers of the first R, G and B byte -- (p, 0, 0) or (p,): one channel, the luma -- of a SOURCE of
        width x height pixels with rows `row_stride` and the bytes of a row `pixel_stride` bytes apart."""
        r, g, b = (tuple(planes) + (0, 0))[:3]
        return StridedImage((C.c_void_p * 3)(r or None, g or None, b or None), width, height, row_stride, pixel_stride, quality)

    def _reduced_batch(self, name: str, imgs, subsampling: int, factor: int, middle, out_ptrs, out_cap: int, size_ptrs, stream: int):
        """A reduced entry: name(context, pictures[], count, subsampling, factor, middle..., outs[], out_cap, sizes[], stream)."""
        n = len(imgs)
        arr, pointers = (StridedImage * n)(*imgs), C.c_void_p * n
        rc = getattr(lib, name)(self._h, arr, n, int(subsampling), int(factor), *middle, pointers(*out_ptrs), out_cap, pointers(*size_ptrs),
                                C.c_void_p(stream))
        if rc:
            raise JpegAmdError(rc, name)

    def encode_reduced_batch_async(self, imgs, subsampling: int, factor: int, out_ptrs, out_cap: int, size_ptrs, stream: int = 0):
        """The files of `len(imgs)` pictures of bytes of one geometry (strided_image), each reduced by `factor` both ways, in three
        scans, or for subsampling 0 the grayscale file (jpegamd_encode_reduced_batch_async); the context, out_cap and the files as for
        encode_planar_batch_async on the reduced bytes."""
        self._reduced_batch("jpegamd_encode_reduced_batch_async", imgs, subsampling, factor, (), out_ptrs, out_cap, size_ptrs, stream)

    def encode_reduced_interleaved_batch_async(self, imgs, subsampling: int, factor: int, restart_interval: int, out_ptrs, out_cap: int,
                                               size_ptrs, stream: int = 0):
        """... in ONE scan, with restart intervals of `restart_interval` MCUs of the reduced picture (0: none) and the context's Huffman
        tables; subsampling 0: the grayscale file of encode_gray_scan_batch_async (jpegamd_encode_reduced_interleaved_batch_async)."""
        self._reduced_batch("jpegamd_encode_reduced_interleaved_batch_async", imgs, subsampling, factor, (int(restart_interval),), out_ptrs,
                            out_cap, size_ptrs, stream)

    def encode_reduced_progressive_script_batch_async(self, imgs, subsampling: int, factor: int, scans, out_ptrs, out_cap: int, size_ptrs,
                                                      stream: int = 0):
        """... as progressive files with the scan script `scans` (None: the default one); subsampling 0: the grayscale progressive
        file (jpegamd_encode_reduced_progressive_script_batch_async)."""
        sc, ns = _scan_array(scans)
        self._reduced_batch("jpegamd_encode_reduced_progressive_script_batch_async", imgs, subsampling, factor, (sc, ns), out_ptrs, out_cap,
                            size_ptrs, stream)


class _ResizedEntries(_ReducedEntries):
    """... and the entries of resized pictures: bytes at any row and pixel stride (strided_image), resampled to
    out_width x out_height by exact area means by one kernel in front of the tile encoder."""

    def _resized_batch(self, name: str, imgs, subsampling: int, out_width: int, out_height: int, middle, out_ptrs, out_cap: int, size_ptrs,
                       stream: int):
        """A resized entry: name(context, pictures[], count, subsampling, out_width, out_height, middle..., outs[], out_cap, sizes[],
        stream)."""
        n = len(imgs)
        arr, pointers = (StridedImage * n)(*imgs), C.c_void_p * n
        rc = getattr(lib, name)(self._h, arr, n, int(subsampling), int(out_width), int(out_height), *middle, pointers(*out_ptrs), out_cap,
                                pointers(*size_ptrs), C.c_void_p(stream))
        if rc:
            raise JpegAmdError(rc, name)

    def encode_resized_batch_async(self, imgs, subsampling: int, out_width: int, out_height: int, out_ptrs, out_cap: int, size_ptrs,
                                   stream: int = 0):
        """The files of `len(imgs)` pictures of bytes of one geometry (strided_image), each resized to out_width x out_height, in three
        scans, or for subsampling 0 the grayscale file (jpegamd_encode_resized_batch_async); the context, out_cap and the files as for
        encode_planar_batch_async on the resized bytes."""
        self._resized_batch("jpegamd_encode_resized_batch_async", imgs, subsampling, out_width, out_height, (), out_ptrs, out_cap, size_ptrs,
                            stream)

    def encode_resized_interleaved_batch_async(self, imgs, subsampling: int, out_width: int, out_height: int, restart_interval: int,
                                               out_ptrs, out_cap: int, size_ptrs, stream: int = 0):
        """... in ONE scan, with restart intervals of `restart_interval` MCUs of the resized picture (0: none) and the context's Huffman
        tables; subsampling 0: the grayscale file of encode_gray_scan_batch_async (jpegamd_encode_resized_interleaved_batch_async)."""
        self._resized_batch("jpegamd_encode_resized_interleaved_batch_async", imgs, subsampling, out_width, out_height,
                            (int(restart_interval),), out_ptrs, out_cap, size_ptrs, stream)

    def encode_resized_progressive_script_batch_async(self, imgs, subsampling: int, out_width: int, out_height: int, scans, out_ptrs,
                                                      out_cap: int, size_ptrs, stream: int = 0):
        """... as progressive files with the scan script `scans` (None: the default one); subsampling 0: the grayscale progressive
        file (jpegamd_encode_resized_progressive_script_batch_async)."""
        sc, ns = _scan_array(scans)
        self._resized_batch("jpegamd_encode_resized_progressive_script_batch_async", imgs, subsampling, out_width, out_height, (sc, ns),
                            out_ptrs, out_cap, size_ptrs, stream)


class Encoder(_ResizedEntries):
    """Level-1 context: device pointers in, device pointers out, stream-ordered."""

    def __init__(self, max_width: int, max_height: int):
        self._h = C.c_void_p()
        _checked("jpegamd_encoder_create", C.byref(self._h), max_width, max_height)

    def close(self):
        if self._h:
            lib.jpegamd_encoder_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_pipeline(self, pipeline: int):
        """PIPELINE_AUTO / PIPELINE_PAIR (k_segment_merge + k_finalize) / PIPELINE_STITCH (k_stitch): which kernels follow k_tile_encode."""
        _checked("jpegamd_encoder_set_pipeline", self._h, int(pipeline))

    def set_huffman(self, huffman: int):
        """HUFFMAN_STANDARD (the Annex K tables, default) or HUFFMAN_OPTIMIZED (per-picture tables) for the one-scan entries
        (jpegamd_encoder_set_huffman); takes effect with the next encode."""
        _checked("jpegamd_encoder_set_huffman", self._h, int(huffman))

    def set_quant_tables(self, luma, chroma=None):
        """Quantisation tables of the caller's for every later encode on this context (jpegamd_encoder_set_quant_tables): each as
        as_quant_table takes it; chroma None: the luma table for every component.  set_quant_tables(None): back to the tables of each
        picture's quality.  Takes effect with the next encode; a refused table leaves the context as it was."""
        if luma is None:
            if chroma is not None:
                raise ValueError("a chroma table needs a luma table")
            _checked("jpegamd_encoder_set_quant_tables", self._h, None, None)
            return
        lt = as_quant_table(luma)
        ct = None if chroma is None else as_quant_table(chroma)
        _checked("jpegamd_encoder_set_quant_tables", self._h, lt.ctypes.data, None if ct is None else ct.ctypes.data)

    def quant_tables(self):
        """None while the context encodes by quality, else the (luma, chroma) it holds: uint8[64] each, raster order."""
        import numpy as np
        luma, chroma, custom = np.zeros(64, np.uint8), np.zeros(64, np.uint8), C.c_int32(0)
        _checked("jpegamd_encoder_get_quant_tables", self._h, luma.ctypes.data, chroma.ctypes.data, C.byref(custom))
        return (luma, chroma) if custom.value else None

    def set_metadata(self, *none, icc_profile=None, exif=None, comment=None, dpi=None, density=None, segments=()):
        """Metadata for every later encode on this context (jpegamd_encoder_set_metadata): the keywords of build_metadata.
        set_metadata(None), or no keyword at all: plain files again.  Everything is copied; takes effect with the next encode, whose
        buffers need metadata_bytes() more than the bound; a refused description is a ValueError and leaves the context as it was."""
        if none not in ((), (None,)):
            raise TypeError("set_metadata takes keywords, or None alone to clear")
        m, keep = _metadata_struct(icc_profile, exif, comment, dpi, density, segments)
        rc = lib.jpegamd_encoder_set_metadata(self._h, C.byref(m))
        del keep
        if rc == -1:
            raise ValueError("metadata refused (see build_metadata)")
        if rc:
            raise JpegAmdError(rc, "jpegamd_encoder_set_metadata")

    def metadata_bytes(self) -> int:
        """M: the bytes the context's metadata adds to every file (jpegamd_encoder_metadata_bytes)."""
        return int(lib.jpegamd_encoder_metadata_bytes(self._h))

    def set_profiling(self, slots: int):
        _checked("jpegamd_encoder_set_profiling", self._h, int(slots))

    def profile(self, slot: int) -> Stats:
        st = Stats()
        _checked("jpegamd_encoder_profile", self._h, slot, C.byref(st))
        return st

    @staticmethod
    def image(pixels_ptr: int, width: int, height: int, row_stride: int, bottom_up: bool = True,
              channel_order: int = ORDER_BGR, quality: int = 0) -> Image:
        return Image(pixels_ptr, width, height, row_stride, 1 if bottom_up else 0, channel_order, quality)

    @staticmethod
    def planar_image(planes, width: int, height: int, row_stride: int, bottom_up: bool = False, quality: int = 0) -> PlanarImage:
        """`planes`: the device pointers of the R, G and B planes, each `row_stride` bytes per stored row."""
        r, g, b = planes
        return PlanarImage((C.c_void_p * 3)(r, g, b), width, height, row_stride, 1 if bottom_up else 0, quality)

    @staticmethod
    def ycbcr_image(y_ptr: int, cb_ptr: int, cr_ptr: int, width: int, height: int, y_stride: int, c_stride: int,
                    chroma_layout: int = CHROMA_PLANES, quality: int = 0) -> YCbCrImage:
        """Device pointers of the Y plane and the chroma: two planes (CHROMA_PLANES), or one plane of byte pairs in `cb_ptr`
        (CHROMA_CBCR / CHROMA_CRCB; `cr_ptr` is then ignored and may be 0), or one packed 4:2:2 plane in `y_ptr` (CHROMA_YUYV /
        CHROMA_UYVY: `y_stride` is its row stride, the chroma arguments are ignored)."""
        return YCbCrImage(y_ptr or None, cb_ptr or None, cr_ptr or None, width, height, y_stride, c_stride, chroma_layout, quality)

    def _batch(self, name: str, struct, imgs, ints, out_ptrs, out_cap: int, size_ptrs, stream: int, tail=()):
        """A batch entry: name(context, pictures[], count, ints..., outs[], out_cap, sizes[], tail..., stream) with the pictures as
        one array of `struct` and the two lists of device pointers as arrays.  encode_batch_async is on bench.py's timed path: this
        raises like _checked, itself, so that the path is one call deeper than it was and no more, and the pointer arrays are made
        from the integers as they are (no c_void_p object each), which pays that call back."""
        n = len(imgs)
        arr, pointers = (struct * n)(*imgs), C.c_void_p * n
        rc = getattr(lib, name)(self._h, arr, n, *[int(v) for v in ints], pointers(*out_ptrs), out_cap, pointers(*size_ptrs), *tail,
                                C.c_void_p(stream))
        if rc:
            raise JpegAmdError(rc, name)

    def encode_planar_batch_async(self, imgs, subsampling: int, out_ptrs, out_cap: int, size_ptrs, stream: int = 0):
        """The files of `len(imgs)` planar pictures of one geometry (jpegamd_encode_planar_batch_async): subsampling 0 grayscale
        files, SUBSAMPLE_444 / SUBSAMPLE_420 / SUBSAMPLE_422 colour files; the context as for the packed batch entries."""
        self._batch("jpegamd_encode_planar_batch_async", PlanarImage, imgs, (subsampling,), out_ptrs, out_cap, size_ptrs, stream)

    def encode_ycbcr_batch_async(self, imgs, subsampling: int, out_ptrs, out_cap: int, size_ptrs, stream: int = 0,
                                 sample_range: int = RANGE_FULL, sample_format: int = SAMPLES_8, matrix: int = MATRIX_BT601):
        """The colour files of `len(imgs)` YCbCr pictures of one geometry (jpegamd_encode_ycbcr_batch_async); the context as for
        encode_color_batch_async.  sample_range: RANGE_FULL, or RANGE_LIMITED for video-range samples, which go through
        jpegamd_encode_ycbcr_range_batch_async and are expanded on read.  sample_format: SAMPLES_8, or SAMPLES_10_MSB / SAMPLES_10_LSB
        for 10-bit samples in 16-bit words (strides in bytes), which go through jpegamd_encode_ycbcr_samples_batch_async and are
        narrowed on read.  matrix: MATRIX_BT601, or MATRIX_BT709 for BT.709 samples, which go through
        jpegamd_encode_ycbcr_matrix_batch_async: one pass converts them to BT.601 planes in context scratch."""
        # The newest entry that the call needs: a call that an older entry can serve keeps to it, so that a variant library
        # without the newer ones still serves it.
        if int(matrix) != MATRIX_BT601:
            name, ints = "jpegamd_encode_ycbcr_matrix_batch_async", (subsampling, sample_range, sample_format, matrix)
        elif int(sample_format) != SAMPLES_8:
            name, ints = "jpegamd_encode_ycbcr_samples_batch_async", (subsampling, sample_range, sample_format)
        elif int(sample_range) != RANGE_FULL:
            name, ints = "jpegamd_encode_ycbcr_range_batch_async", (subsampling, sample_range)
        else:
            name, ints = "jpegamd_encode_ycbcr_batch_async", (subsampling,)
        self._batch(name, YCbCrImage, imgs, ints, out_ptrs, out_cap, size_ptrs, stream)

    def encode_async(self, img: Image, out_ptr: int, out_cap: int, size_ptr: int, with_container: bool = True,
                     stream: int = 0):
        _checked("jpegamd_encode_async", self._h, C.byref(img), C.c_void_p(out_ptr), out_cap, C.c_void_p(size_ptr),
                 1 if with_container else 0, C.c_void_p(stream))

    def encode_color_async(self, img: Image, subsampling: int, out_ptr: int, out_cap: int, size_ptr: int, stream: int = 0):
        """The colour file of an RGB / BGR image (jpegamd_encode_color_async): SUBSAMPLE_444, SUBSAMPLE_420 or SUBSAMPLE_422."""
        _checked("jpegamd_encode_color_async", self._h, C.byref(img), int(subsampling), C.c_void_p(out_ptr), out_cap, C.c_void_p(size_ptr),
                 C.c_void_p(stream))

    def encode_color_batch_async(self, imgs, subsampling: int, out_ptrs, out_cap: int, size_ptrs, stream: int = 0):
        """The colour files of `len(imgs)` RGB / BGR pictures of one geometry (<= MAX_BATCH) with one launch of each kernel
        (jpegamd_encode_color_batch_async); the context must hold len(imgs) x the tiles and segments of one picture."""
        self._batch("jpegamd_encode_color_batch_async", Image, imgs, (subsampling,), out_ptrs, out_cap, size_ptrs, stream)

    def encode_color_interleaved_batch_async(self, imgs, subsampling: int, out_ptrs, out_cap: int, size_ptrs, stream: int = 0):
        """The colour files of `len(imgs)` RGB / BGR pictures of one geometry (<= MAX_BATCH) with ONE scan of interleaved MCUs each
        (jpegamd_encode_color_interleaved_batch_async); the context as for encode_color_batch_async."""
        self._batch("jpegamd_encode_color_interleaved_batch_async", Image, imgs, (subsampling,), out_ptrs, out_cap, size_ptrs, stream)

    def encode_ycbcr_interleaved_batch_async(self, imgs, subsampling: int, out_ptrs, out_cap: int, size_ptrs, stream: int = 0):
        """The same files from 8-bit full-range BT.601 YCbCr pictures in planes or byte pairs
        (jpegamd_encode_ycbcr_interleaved_batch_async)."""
        self._batch("jpegamd_encode_ycbcr_interleaved_batch_async", YCbCrImage, imgs, (subsampling,), out_ptrs, out_cap, size_ptrs, stream)

    def encode_color_interleaved_restart_batch_async(self, imgs, subsampling: int, restart_interval: int, out_ptrs, out_cap: int, size_ptrs,
                                                     stream: int = 0):
        """encode_color_interleaved_batch_async with restart intervals of `restart_interval` MCUs (DRI / RSTn; 0: the file without)
        (jpegamd_encode_color_interleaved_restart_batch_async)."""
        self._batch("jpegamd_encode_color_interleaved_restart_batch_async", Image, imgs, (subsampling, restart_interval), out_ptrs, out_cap,
                    size_ptrs, stream)

    def encode_ycbcr_interleaved_restart_batch_async(self, imgs, subsampling: int, restart_interval: int, out_ptrs, out_cap: int, size_ptrs,
                                                     stream: int = 0):
        """encode_ycbcr_interleaved_batch_async with restart intervals (jpegamd_encode_ycbcr_interleaved_restart_batch_async)."""
        self._batch("jpegamd_encode_ycbcr_interleaved_restart_batch_async", YCbCrImage, imgs, (subsampling, restart_interval), out_ptrs,
                    out_cap, size_ptrs, stream)

    def encode_ycbcr_interleaved_matrix_batch_async(self, imgs, subsampling: int, sample_range: int, sample_format: int, matrix: int,
                                                    restart_interval: int, out_ptrs, out_cap: int, size_ptrs, stream: int = 0):
        """The one-scan files of YCbCr pictures of ANY kind encode_ycbcr_batch_async takes -- limited range, 10-bit words, BT.709, a
        packed 4:2:2 plane -- with restart intervals of `restart_interval` MCUs (0: none)
        (jpegamd_encode_ycbcr_interleaved_matrix_batch_async)."""
        self._batch("jpegamd_encode_ycbcr_interleaved_matrix_batch_async", YCbCrImage, imgs,
                    (subsampling, sample_range, sample_format, matrix, restart_interval), out_ptrs, out_cap, size_ptrs, stream)

    def encode_color_interleaved_pixels_batch_async(self, imgs, subsampling: int, restart_interval: int, out_ptrs, out_cap: int, size_ptrs,
                                                    stream: int = 0):
        """The one-scan files of RGB / BGR / RGBA / BGRA pictures, with restart intervals of `restart_interval` MCUs (0: none)
        (jpegamd_encode_color_interleaved_pixels_batch_async)."""
        self._batch("jpegamd_encode_color_interleaved_pixels_batch_async", Image, imgs, (subsampling, restart_interval), out_ptrs, out_cap,
                    size_ptrs, stream)

    def encode_planar_interleaved_batch_async(self, imgs, subsampling: int, restart_interval: int, out_ptrs, out_cap: int, size_ptrs,
                                              stream: int = 0):
        """The one-scan files of planar pictures (planar_image), with restart intervals of `restart_interval` MCUs (0: none)
        (jpegamd_encode_planar_interleaved_batch_async); no grayscale files: subsampling 0 is refused."""
        self._batch("jpegamd_encode_planar_interleaved_batch_async", PlanarImage, imgs, (subsampling, restart_interval), out_ptrs, out_cap,
                    size_ptrs, stream)

    def color_profile(self, slot: int):
        """Per-kernel ns of a profiled colour encode: planes, (tile, merge, finalize) x Y / Cb / Cr, append."""
        ns = (C.c_uint64 * 11)()
        _checked("jpegamd_debug_color_profile", self._h, slot, ns)
        return list(ns)

    def encode_batch_async(self, imgs, out_ptrs, out_cap: int, size_ptrs, with_container: bool = True, stream: int = 0):
        """`len(imgs)` images of one geometry (<= MAX_BATCH) through ONE launch of each kernel; the context must hold
        len(imgs) x the tiles and segments of one image (e.g. Encoder(W, len(imgs) * H))."""
        self._batch("jpegamd_encode_batch_async", Image, imgs, (), out_ptrs, out_cap, size_ptrs, stream, (1 if with_container else 0,))

    def encode_gray_scan_batch_async(self, imgs, restart_interval: int, out_ptrs, out_cap: int, size_ptrs, stream: int = 0):
        """The grayscale files of `len(imgs)` pictures of one geometry (<= MAX_BATCH; any channel order: the luma) with restart
        intervals of `restart_interval` blocks (0: none) and the context's Huffman tables (set_huffman)
        (jpegamd_encode_gray_scan_batch_async); out_cap from max_jfif_bytes_gray_scan."""
        self._batch("jpegamd_encode_gray_scan_batch_async", Image, imgs, (restart_interval,), out_ptrs, out_cap, size_ptrs, stream)

    # ---- one image sharded over GPUs by block rows (include/jpeg_compression.h) ----
    def encode_rows_async(self, img: Image, row_begin: int, row_end: int, stream: int = 0):
        _checked("jpegamd_encode_rows_async", self._h, C.byref(img), C.c_int32(row_begin), C.c_int32(row_end), C.c_void_p(stream))

    def export_segments(self, img: Image, row_begin: int, row_end: int, dense_ptr: int, dense_cap_words: int, meta_ptr: int,
                        total_ptr: int, stream: int = 0):
        _checked("jpegamd_export_segments", self._h, C.byref(img), C.c_int32(row_begin), C.c_int32(row_end), C.c_void_p(dense_ptr),
                 C.c_uint64(dense_cap_words), C.c_void_p(meta_ptr), C.c_void_p(total_ptr), C.c_void_p(stream))

    def import_segments(self, img: Image, row_begin: int, row_end: int, dense_ptr: int, meta_ptr: int, stream: int = 0):
        _checked("jpegamd_import_segments", self._h, C.byref(img), C.c_int32(row_begin), C.c_int32(row_end), C.c_void_p(dense_ptr),
                 C.c_void_p(meta_ptr), C.c_void_p(stream))

    def finalize_async(self, img: Image, out_ptr: int, out_cap: int, size_ptr: int, with_container: bool = True, stream: int = 0):
        _checked("jpegamd_finalize_async", self._h, C.byref(img), C.c_void_p(out_ptr), C.c_uint64(out_cap), C.c_void_p(size_ptr),
                 1 if with_container else 0, C.c_void_p(stream))

    def finish(self) -> Stats:
        st = Stats()
        _checked("jpegamd_encoder_finish", self._h, C.byref(st))
        return st

    def debug_stages(self, img: Image, y_ptr: int = 0, zz_ptr: int = 0, mask_ptr: int = 0):
        _checked("jpegamd_debug_stages", self._h, C.byref(img), C.c_void_p(y_ptr), C.c_void_p(zz_ptr), C.c_void_p(mask_ptr))

    def debug_dct_exact(self, blocks_ptr: int, coeffs_ptr: int, nblocks: int):
        _checked("jpegamd_debug_dct_exact", self._h, C.c_void_p(blocks_ptr), C.c_void_p(coeffs_ptr), nblocks)
