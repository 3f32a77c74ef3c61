/*
 * jpeg_compression.h -- C-ABI of the MI355X-native BMP -> baseline-JPEG encoder: grayscale (the reference's output) and
 * colour (YCbCr 4:4:4 / 4:2:0 in three non-interleaved scans, jpegamd_encode_color_async).
 *
 * This is the drop-in boundary for the reference's encode path
 * (strbac-damjan/jpeg-image-compression).  Every entry point cites the reference interface
 * it replaces; file:line are relative to the reference root.  Plain C types only: a
 * maintainer binds these from C (natural_c/src/main.c links unchanged), from ctypes, or
 * from any FFI.  See INTEGRATION.md for the reference-side stubs.
 *
 * Three levels, lowest first:
 *   1. jpegamd_*            device-resident, stream-ordered hot path (what bench.py times)
 *   2. JpegCompression_Init / convertToJpeg(JPEG_COMPRESSION_DTO*)
 *                           the reference's accelerator boundary
 *                           (dsp_port/jpeg_compression/include/jpeg_compression.h:32-77,111)
 *   3. loadBMPImage / saveJPEGGrayscale / stage functions
 *                           the natural_c library surface
 *                           (natural_c/include/bmp_handler.h:37-47, jpeg_handler.h:100-109)
 *
 * There is NO CPU fallback anywhere behind this header: without a HIP device every
 * compute entry point fails with JPEGAMD_ERR_NO_DEVICE (and the natural_c-shaped ones
 * return NULL / false after printing the reason).
 *
 * Threading: one in-flight call per encoder context; JpegCompression_Init once per
 * process (the reference is single-threaded and non-re-entrant as well:
 * natural_c/src/core/huffman.c:9-11,106-117).
 */
#ifndef JPEGAMD_JPEG_COMPRESSION_H
#define JPEGAMD_JPEG_COMPRESSION_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------
 * Status codes.  0 / -6 / -8 keep the reference's meaning
 * (dsp_port/jpeg_compression/src/jpeg_compression.c:181,206,214).
 * ---------------------------------------------------------------------------------- */
#define JPEGAMD_OK                0
#define JPEGAMD_ERR_ARG          (-1)  /* NULL / non-positive dims / bad stride */
#define JPEGAMD_ERR_NO_DEVICE    (-2)  /* no HIP device or kernel image not loadable */
#define JPEGAMD_ERR_HIP          (-3)  /* a HIP runtime call failed */
#define JPEGAMD_ERR_NOT_INIT     (-4)  /* JpegCompression_Init() not called */
#define JPEGAMD_ERR_TOO_LARGE    (-5)  /* image exceeds the context's max dims */
#define JPEGAMD_ERR_RLE_CAPACITY (-6)  /* reference: RLE capacity exhausted */
#define JPEGAMD_ERR_BMP          (-7)  /* malformed BMP (magic / bit count / compression / short) */
#define JPEGAMD_ERR_HUFF_CAPACITY (-8) /* reference: Huffman buffer too small */

#define JPEGAMD_JFIF_PREFIX_BYTES 328  /* APP0+DQT+SOF0+DHT+DHT+SOS, natural_c/src/io/jpeg_handler.c:220-233 */

/* ------------------------------------------------------------------------------------
 * Level 1: device-resident hot path
 * ---------------------------------------------------------------------------------- */

/* Pixel source description.  Covers both things the reference feeds its codec:
 *  - BMP file rows as they lie in the file: BGR, bottom-up, stride (3W+3)&~3
 *    (natural_c/src/io/bmp_handler.c:68-75,109-122)      -> JPEGAMD_ORDER_BGR, bottom_up=1
 *  - a loaded BMPImage: RGB, top-down, tightly packed
 *    (natural_c/include/bmp_handler.h:37-41)              -> JPEGAMD_ORDER_RGB, bottom_up=0
 */
#define JPEGAMD_ORDER_BGR 0
#define JPEGAMD_ORDER_RGB 1
/* One byte per pixel: `pixels` holds the luma itself (row_stride >= width); the output is a grayscale file.  Accepted by
 * jpegamd_encode_async, jpegamd_encode_batch_async and jpegamd_debug_stages (not by the colour entry points). */
#define JPEGAMD_ORDER_GRAY 2
/* Four bytes per pixel (row_stride >= 4 * width): R, G, B, x or B, G, R, x.  The fourth byte is ignored: the output is byte for
 * byte that of the same R, G, B values stored as JPEGAMD_ORDER_RGB.  Accepted by jpegamd_encode_async, jpegamd_encode_batch_async
 * (the grayscale file), jpegamd_encode_color_async and jpegamd_encode_color_batch_async (the colour file); every other entry that
 * takes an image or a DTO -- the row-sharded entries, convertToJpeg, jpegamd_debug_stages, the BMP and file entries -- answers
 * JPEGAMD_ERR_ARG. */
#define JPEGAMD_ORDER_RGBA 3
#define JPEGAMD_ORDER_BGRA 4

typedef struct JpegAmdImage {
    const void *pixels;    /* DEVICE pointer to the first stored row */
    int32_t width;         /* original (unpadded) width,  1..65535 */
    int32_t height;        /* original (unpadded) height, 1..65535 */
    int32_t row_stride;    /* bytes between stored rows (>= 3*width; GRAY: >= width; RGBA / BGRA: >= 4*width) */
    int32_t bottom_up;     /* 1: stored row 0 is the LAST image row (BMP default) */
    int32_t channel_order; /* JPEGAMD_ORDER_BGR, _RGB, _GRAY, _RGBA or _BGRA */
    int32_t quality;       /* 0 or 50: the reference's only table
                              (natural_c/src/core/jpeg_tables.c:3-12); 1..100 otherwise =
                              libjpeg scaling of that table (extension) */
} JpegAmdImage;

/* Per-call statistics, filled on request (host memory).  The *_ns fields are hipEvent
 * times of the device phases; they play the role of the reference DTO's cycles_* fields
 * (dsp_port/jpeg_compression/include/jpeg_compression.h:55-62). */
typedef struct JpegAmdStats {
    uint64_t jfif_bytes;        /* total bytes written (prefix + segment + EOI) */
    uint64_t entropy_bits;      /* unstuffed entropy-coded bits */
    uint64_t stuffed_bytes;     /* number of 0x00 bytes inserted after 0xFF */
    uint64_t exact_fallbacks;   /* coefficients recomputed in the reference's float order */
    /* With profiling on (jpegamd_encoder_set_profiling) every kernel is launched with its own begin / end events
       (hipExtLaunchKernelGGL): the three figures are the kernels' OWN durations, what a kernel trace shows. */
    uint64_t ns_transform;      /* k_tile_encode: luma + DCT + quantisation + zigzag + run/size symbols + Huffman coding, per tile */
    uint64_t ns_entropy;        /* k_segment_merge: the tiles' bit strings -> one per segment (the field keeps its round-1 name) */
    uint64_t ns_pack;           /* k_finalize: bit / stuffing offsets, stitch, 0xFF stuffing, container */
    uint64_t ns_total;          /* begin of the first kernel .. end of the last: the three durations plus the launch gaps between them */
} JpegAmdStats;

typedef struct JpegAmdEncoder JpegAmdEncoder;   /* opaque; owns device scratch */

/* Create a context able to encode images up to max_width x max_height on the current
 * HIP device.  Scratch is allocated once here (nothing is allocated per call). */
int32_t jpegamd_encoder_create(JpegAmdEncoder **enc, int32_t max_width, int32_t max_height);
int32_t jpegamd_encoder_destroy(JpegAmdEncoder *enc);

/* Upper bound on the JFIF bytes an image of this size can produce (every block at the
 * 1658-bit worst case and every byte stuffed): size `out` with this. */
/* (With metadata set on the context -- jpegamd_encoder_set_metadata -- a buffer needs jpegamd_encoder_metadata_bytes() more than this bound.) */
uint64_t jpegamd_max_jfif_bytes(int32_t width, int32_t height);

/* Enqueue one encode on `stream` (a hipStream_t, or NULL for the default stream).
 *   out_dev        DEVICE buffer receiving the JFIF file bytes
 *   out_capacity   its size in bytes (>= jpegamd_max_jfif_bytes for a guaranteed fit;
 *                  smaller is allowed, overflow is reported through out_size_dev = 0 and
 *                  JPEGAMD_ERR_HUFF_CAPACITY from jpegamd_encoder_finish)
 *   out_size_dev   DEVICE uint64_t receiving the byte count
 *   with_container 1: JFIF prefix + entropy segment + EOI (what saveJPEGGrayscale writes,
 *                  natural_c/src/io/jpeg_handler.c:220-262); 0: entropy segment only
 *                  (what the reference's accelerator hands back,
 *                  dsp_port/jpeg_compression/src/jpeg_compression.c:198-203)
 * Asynchronous: returns once the kernels are enqueued. */
int32_t jpegamd_encode_async(JpegAmdEncoder *enc, const JpegAmdImage *img, void *out_dev,
                             uint64_t out_capacity, uint64_t *out_size_dev,
                             int32_t with_container, void *stream);

/* Enqueue the encode of `count` images (1 .. JPEGAMD_MAX_BATCH) of ONE geometry -- same width, height, row_stride,
 * bottom_up, channel_order and quality, different pixels -- as ONE launch of each kernel: the reference codes one file per
 * process (natural_c/src/main.c:21-24), a server codes many, and small images leave a launch per image mostly idle (a 4096^2
 * image gives every wave of the transform two tiles).  outs_dev[i] / out_sizes_dev[i] receive image i's bytes and byte
 * count; every output has out_capacity bytes.  The context must have been created for at least count x the tiles and
 * segments of one image (e.g. jpegamd_encoder_create(W, count * H) for count W x H images -- max_height may go up to
 * JPEGAMD_MAX_BATCH x 65535 for that purpose); JPEGAMD_ERR_TOO_LARGE otherwise.
 * jpegamd_encoder_finish then reports the LAST image's size and the batch's summed counters. */
#define JPEGAMD_MAX_BATCH 32
int32_t jpegamd_encode_batch_async(JpegAmdEncoder *enc, const JpegAmdImage *imgs, int32_t count, void *const *outs_dev,
                                   uint64_t out_capacity, uint64_t *const *out_sizes_dev, int32_t with_container,
                                   void *stream);

/* ---- Colour (no reference counterpart: the reference writes grayscale only) ------------------------------------------
 * A baseline JFIF file with three components in three NON-interleaved scans, Y, Cb, Cr (colour scans):
 *   Y  = (77 R + 150 G + 29 B) >> 8              (the grayscale path's luma; its scan is byte for byte the grayscale file's)
 *   Cb = (32768 - 43 R - 85 G + 128 B) >> 8      Cr = (32768 + 128 R - 107 G - 21 B) >> 8
 *   4:2:0: chroma planes of ceil(W/2) x ceil(H/2), sample = (a + b + c + d + 2) >> 2 over 2 x 2 pixels (last column / row
 *   replicated); 4:2:2: ceil(W/2) x H, sample = (a + b + 1) >> 1 over the two pixels 2x, 2x + 1 of one row (last column replicated,
 *   no vertical filter; SOF0 gives component 1 the sampling factors 2 x 1); 4:4:4: W x H.  Chroma: T.81 Annex K tables K.2 (quantisation, scaled for `quality` like the luma table),
 *   K.4 / K.6 (Huffman).  No restart markers.
 * jpegamd_encode_color_async always writes the whole file (prefix, three scans, EOI) into out_dev, stream-ordered, with no host
 * synchronisation inside the call.  A GRAY image or another subsampling value: JPEGAMD_ERR_ARG.  An RGBA / BGRA image runs as a
 * colour batch of one (jpegamd_encode_color_batch_async: with profiling on it records ns_total only).  If the file does not fit
 * out_capacity, jpegamd_encoder_finish returns JPEGAMD_ERR_HUFF_CAPACITY, *out_size_dev is 0 and nothing is written past
 * out_capacity.  Its statistics are sums over the three scans; ns_total spans the whole call.
 * The context allocates its colour scratch (chroma constants, the two planes, the chroma scans) on its first colour call, sized
 * for that picture at 4:4:4 and grown when a later colour call needs more; a context that never encodes colour allocates
 * nothing for it. */
#define JPEGAMD_SUBSAMPLE_444 1
#define JPEGAMD_SUBSAMPLE_420 2
/* (3 is skipped, here and among the chroma layouts below: every entry has always answered 3 with JPEGAMD_ERR_ARG, callers and the
 *  test suite rely on it as a known-bad value, and a new meaning for it would change what existing code gets.) */
#define JPEGAMD_SUBSAMPLE_422 4
/* Upper bound on the colour file's bytes (every block at the 1723-bit chroma worst case, every byte stuffed); 0 for bad args. */
/* (With metadata set on the context -- jpegamd_encoder_set_metadata -- a buffer needs jpegamd_encoder_metadata_bytes() more than this bound.) */
uint64_t jpegamd_max_jfif_bytes_color(int32_t width, int32_t height, int32_t subsampling);
int32_t jpegamd_encode_color_async(JpegAmdEncoder *enc, const JpegAmdImage *img, int32_t subsampling, void *out_dev,
                                   uint64_t out_capacity, uint64_t *out_size_dev, void *stream);
/* The colour files of `count` pictures (1 .. JPEGAMD_MAX_BATCH) of ONE geometry -- the rules of jpegamd_encode_batch_async, BGR or
 * RGB (or RGBA / BGRA) only -- with one launch of each kernel: the chroma planes of all pictures, the Y scans as one batch, and the Cb and Cr planes
 * of all pictures as batches of planes (one launch for count <= 16 at 4:2:0 on a context created for count x H with H a multiple
 * of 16; more where the context's scratch holds fewer planes).  outs_dev[i] / *out_sizes_dev[i] receive exactly what
 * jpegamd_encode_color_async writes for imgs[i]; a picture whose file does not fit out_capacity gets size 0 and nothing past
 * out_capacity, the others are unaffected, and jpegamd_encoder_finish returns JPEGAMD_ERR_HUFF_CAPACITY.  The context must hold
 * count x the tiles and segments of one picture, i.e. count x its block rows: jpegamd_encoder_create(W, count * H8) with H8 = H
 * rounded up to a multiple of 8 (count * H is too small when H is not a multiple of 8); JPEGAMD_ERR_TOO_LARGE otherwise.  No host
 * synchronisation inside the call.  jpegamd_encoder_finish then reports the last picture's size; entropy_bits, stuffed_bytes and
 * exact_fallbacks are sums over every picture and scan.  With profiling on, a batch records ns_total only (the whole call).  The
 * colour batch scratch (2 x count planes and chroma scans) is sized for the call's real plane geometry and grown when a later
 * batch needs more. */
int32_t jpegamd_encode_color_batch_async(JpegAmdEncoder *enc, const JpegAmdImage *imgs, int32_t count, int32_t subsampling,
                                         void *const *outs_dev, uint64_t out_capacity, uint64_t *const *out_sizes_dev,
                                         void *stream);

/* ---- Planar (channels-first) pictures: the R, G and B planes of one byte per sample, as a [3, H, W] tensor stores them ------------
 * Three pointers, not a base and a plane stride: a crop of a [3, H, W] tensor and three separate allocations both fit. */
typedef struct JpegAmdPlanarImage {
    const void *plane[3];   /* DEVICE pointers: the R, G and B planes, one byte per sample */
    int32_t width, height;  /* 1..65535 */
    int32_t row_stride;     /* bytes between stored rows, the same for the three planes, >= width */
    int32_t bottom_up;
    int32_t quality;
} JpegAmdPlanarImage;
/* The files of `count` (1 .. JPEGAMD_MAX_BATCH) planar pictures of ONE geometry (width, height, row_stride, bottom_up, quality), read
 * where they lie -- no repacking pass.  subsampling 0: grayscale files with container, as jpegamd_encode_batch_async writes them;
 * JPEGAMD_SUBSAMPLE_444 / _420 / _422: colour files, as jpegamd_encode_color_batch_async writes them.  Each file is byte for byte the one
 * those entries produce for the same R, G, B values stored as packed JPEGAMD_ORDER_RGB.  Context sizing, capacity, status and
 * statistics are those of the entry it stands for.  out_sizes_dev[i] is a DEVICE uint64_t.  Bad arguments -- a null array or element,
 * a null plane, count out of range, row_stride < width, another subsampling value, pictures of different geometry -- are refused
 * with JPEGAMD_ERR_ARG before the context is read. */
int32_t jpegamd_encode_planar_batch_async(JpegAmdEncoder *enc, const JpegAmdPlanarImage *imgs, int32_t count, int32_t subsampling,
                                          void *const *outs_dev, uint64_t out_capacity, void *const *out_sizes_dev, void *stream);

/* ---- YCbCr pictures: samples that already ARE Y, Cb and Cr (a video decoder's NV12 / I420 frame, a resizer's output) ----------------
 * The planes are coded as they are given: the samples are taken as JFIF full-range values (Y 0..255, Cb / Cr centred on 128), and
 * NO range or matrix conversion, no subsampling and no filtering is done -- limited-range (16..235) material goes through
 * jpegamd_encode_ycbcr_range_batch_async below, BT.709 material through jpegamd_encode_ycbcr_matrix_batch_async.  The Y plane is width x height; the chroma planes are cw x ch: width x height at JPEGAMD_SUBSAMPLE_444,
 * ceil(width / 2) x ceil(height / 2) at JPEGAMD_SUBSAMPLE_420, ceil(width / 2) x height at JPEGAMD_SUBSAMPLE_422 (I422; NV16 / NV61
 * as byte pairs).  Odd sizes are allowed.
 * 4:2:2 also comes packed, as capture hardware delivers it: ONE plane of 4-byte groups, two pixels each, that holds all three
 * components (YUY2 / UYVY).  Then y points at the packed plane, y_stride is its row stride (>= 4 * ceil(width / 2)), cb, cr and
 * c_stride are not looked at (cb and cr may be null), and JPEGAMD_SUBSAMPLE_422 is the only subsampling accepted.  Odd widths are
 * allowed: the second Y byte of a row's last group is never read. */
#define JPEGAMD_CHROMA_PLANES 0   /* cb and cr: two planes of one byte per sample (I420; YV12 by swapping the pointers; planar 4:4:4) */
#define JPEGAMD_CHROMA_CBCR   1   /* cb: ONE plane of byte pairs Cb0 Cr0 Cb1 Cr1 ... (NV12; NV24 at 4:4:4); cr is ignored and may be null */
#define JPEGAMD_CHROMA_CRCB   2   /* the same with Cr first (NV21 / NV42) */
#define JPEGAMD_CHROMA_YUYV   4   /* y: ONE plane of 4-byte groups Y0 Cb Y1 Cr (YUY2); cb, cr, c_stride ignored (3: see JPEGAMD_SUBSAMPLE_422) */
#define JPEGAMD_CHROMA_UYVY   5   /* the same as Cb Y0 Cr Y1 */
typedef struct JpegAmdYCbCrImage {
    const void *y, *cb, *cr;      /* DEVICE pointers, top row first */
    int32_t width, height;        /* of the Y plane, 1..65535 */
    int32_t y_stride, c_stride;   /* bytes between rows; y_stride >= width; c_stride >= cw (PLANES) or >= 2*cw (CBCR / CRCB); YUYV / UYVY: y_stride >= 4*cw
                                   * (16-bit samples, jpegamd_encode_ycbcr_samples_batch_async: twice these) */
    int32_t chroma_layout;        /* JPEGAMD_CHROMA_* */
    int32_t quality;
} JpegAmdYCbCrImage;
/* The colour files of `count` (1 .. JPEGAMD_MAX_BATCH) YCbCr pictures of ONE geometry (width, height, both strides, layout, quality),
 * read where they lie.  The file is the colour file of jpegamd_encode_color_batch_async for (width, height, quality, subsampling)
 * with these samples in its three scans: the Y scan is the entropy-coded segment of the grayscale file of the Y plane, the Cb and
 * Cr scans are the chroma pipeline (tables K.2, K.4 / K.6) over the chroma planes.  Fed the Y, Cb and Cr that the colour entry derives
 * from an RGB picture it writes that entry's file byte for byte, and every chroma layout of the same samples gives the same file.
 * No chroma-plane pass runs and no plane scratch is allocated.  Any pointer alignment and stride is taken (planes on dword
 * boundaries with strides that are multiples of 4 below 2^24 take the fast loader).  Context sizing, capacity behaviour (size 0 and
 * JPEGAMD_ERR_HUFF_CAPACITY at jpegamd_encoder_finish), status, statistics and profiling are those of
 * jpegamd_encode_color_batch_async.  out_sizes_dev[i] is a DEVICE uint64_t.  Bad arguments -- a null array or element, a null y or
 * cb, a null cr with JPEGAMD_CHROMA_PLANES, an unknown layout or subsampling, a packed layout with another subsampling than 4:2:2,
 * count out of range, a stride too short, pictures of different geometry or layout -- are refused with JPEGAMD_ERR_ARG before the context is read. */
int32_t jpegamd_encode_ycbcr_batch_async(JpegAmdEncoder *enc, const JpegAmdYCbCrImage *imgs, int32_t count, int32_t subsampling,
                                         void *const *outs_dev, uint64_t out_capacity, void *const *out_sizes_dev, void *stream);

/* The same entry for samples of either range.  Video decoders and capture hardware deliver LIMITED ("video", "studio") range: Y in
 * 16..235, Cb / Cr in 16..240.  With JPEGAMD_RANGE_LIMITED every sample is expanded to JFIF full range as the tile kernel reads it --
 * no pass over the planes, no scratch, no extra launch -- by this map (integers, `/` is floor division: clamp, then rescale with
 * round-half-up):
 *     Y' = (255 * (clamp(Y, 16, 235) - 16) + 109) / 219        0..255
 *     C' = (255 * (clamp(C, 16, 240) - 16) + 112) / 224        0..255   (Cb and Cr alike)
 * so Y 16 -> 0 and 235 -> 255, Cb / Cr 16 -> 0, 128 -> 128 (neutral chroma stays neutral) and 240 -> 255; both maps are monotone and
 * everything outside the nominal range clamps.  The file is byte for byte the file jpegamd_encode_ycbcr_batch_async writes for the
 * mapped samples.  Only the RANGE is expanded: the matrix stays BT.601 as JFIF defines it (BT.709 -> BT.601 matrix conversion is
 * jpegamd_encode_ycbcr_matrix_batch_async's).  With JPEGAMD_RANGE_FULL this IS jpegamd_encode_ycbcr_batch_async: same code path, same files.  Layouts,
 * subsamplings, context sizing, capacity behaviour, status, statistics and profiling are those of that entry, and so are its argument
 * checks; any other sample_range is refused with JPEGAMD_ERR_ARG, like them before the context is read. */
#define JPEGAMD_RANGE_FULL    0   /* samples are JFIF full range: coded as given */
#define JPEGAMD_RANGE_LIMITED 1   /* Y 16..235, Cb / Cr 16..240: expanded on read by the map above */
int32_t jpegamd_encode_ycbcr_range_batch_async(JpegAmdEncoder *enc, const JpegAmdYCbCrImage *imgs, int32_t count, int32_t subsampling,
                                               int32_t sample_range, void *const *outs_dev, uint64_t out_capacity, void *const *out_sizes_dev,
                                               void *stream);

/* The same entry for 10-bit samples in 16-bit words: what a Main10 / AV1 10-bit / VP9 profile 2 decoder delivers -- P010 from hardware
 * decoders, yuv420p10le (I010) from software ones.  Every sample is a little-endian 16-bit word w, narrowed to the 8-bit sample that is
 * coded as the tile kernel reads it -- no pass over the planes, no scratch, no extra launch.  Its 10-bit value v follows from
 * sample_format:
 *     JPEGAMD_SAMPLES_8       one byte per sample: this entry IS jpegamd_encode_ycbcr_range_batch_async, same code path, same files
 *     JPEGAMD_SAMPLES_10_MSB  v = w >> 6, the low six bits ignored   (P010 / P210 / P410 and their planar twins; P012 / P016 read at 10 bits)
 *     JPEGAMD_SAMPLES_10_LSB  v = min(w, 1023)                       (I010 / I210 / I410, yuv4xxp10le)
 * and the coded sample from v (integers, `/` is floor division):
 *     JPEGAMD_RANGE_FULL      s  = min(255, (v + 2) >> 2)                             Y, Cb, Cr alike; 512 -> 128
 *     JPEGAMD_RANGE_LIMITED   Y' = (255 * (clamp(v, 64, 940) - 64) + 438) / 876       64 -> 0, 940 -> 255
 *                             C' = (255 * (clamp(v, 64, 960) - 64) + 448) / 896       64 -> 0, 512 -> 128, 960 -> 255
 * One rounding from ten bits, not two through an 8-bit limited-range sample: every one of the 256 output levels is reached.  The
 * file is byte for byte the file jpegamd_encode_ycbcr_batch_async writes for the mapped 8-bit planes.
 * The JpegAmdYCbCrImage is the same and strides stay in BYTES: with a 16-bit format y_stride >= 2 * width, c_stride >= 2 * cw
 * (JPEGAMD_CHROMA_PLANES: I010 / I210 / I410) or >= 4 * cw (JPEGAMD_CHROMA_CBCR / _CRCB: P010 / P210 / P410 and their Cr-first twins:
 * one plane of 16-bit pairs).  All three subsamplings and both ranges are taken.  The packed layouts (JPEGAMD_CHROMA_YUYV / _UYVY)
 * with a 16-bit format -- Y210 -- are NOT taken: JPEGAMD_ERR_ARG.  Any pointer alignment and any stride is taken, odd addresses
 * included (planes on dword boundaries with strides that are multiples of 4 below 2^24 take the fast loader; everything else is read
 * byte by byte).  An unknown sample_format is refused with JPEGAMD_ERR_ARG like every other bad argument of that entry, before the
 * context is read; context sizing, capacity behaviour, status, statistics and profiling are those of jpegamd_encode_color_batch_async. */
#define JPEGAMD_SAMPLES_8      0   /* one byte per sample */
#define JPEGAMD_SAMPLES_10_MSB 1   /* 16-bit words, the 10-bit value in the HIGH bits (P010): v = w >> 6 */
#define JPEGAMD_SAMPLES_10_LSB 2   /* 16-bit words, the 10-bit value in the LOW bits (I010): v = min(w, 1023) */
int32_t jpegamd_encode_ycbcr_samples_batch_async(JpegAmdEncoder *enc, const JpegAmdYCbCrImage *imgs, int32_t count, int32_t subsampling,
                                                 int32_t sample_range, int32_t sample_format, void *const *outs_dev, uint64_t out_capacity,
                                                 void *const *out_sizes_dev, void *stream);

/* The same entry for samples of either matrix.  JFIF fixes the matrix at BT.601; every HD and UHD stream a decoder delivers is BT.709,
 * and coded as given its colours come out shifted.  With JPEGAMD_MATRIX_BT709 ONE pass over the batch (k_ycbcr_matrix_batch, one launch
 * for every picture) reads each picture once, in whatever layout, depth and range it has, and writes 8-bit full-range BT.601 Y, Cb and
 * Cr planes into context scratch (the plane scratch of jpegamd_encode_color_batch_async, and one Y plane more per picture); the
 * full-range plane launches then code those.  Let Y, Cb, Cr be the 8-bit full-range samples the entries above would code: the stored
 * bytes, or the bytes after the JPEGAMD_RANGE_LIMITED map, or after the JPEGAMD_SAMPLES_10_* maps for either alignment and range.
 * Those maps come first and stay as they are; the matrix works on their 8-bit results (so 10-bit BT.709 input is rounded twice, once
 * by its map and once here).  With cb = Cb - 128, cr = Cr - 128 and >> an arithmetic (floor) shift of a signed 32-bit value:
 *     Y'  = clamp(Y   + ((  1664 * cb +  3213 * cr + 8192) >> 14), 0, 255)
 *     Cb' = clamp(128 + (( 16218 * cb -  1813 * cr + 8192) >> 14), 0, 255)
 *     Cr' = clamp(128 + (( -1187 * cb + 16112 * cr + 8192) >> 14), 0, 255)
 * Luma sample (x, y) takes the chroma sample at the same indices as the file's subsampling -- (x, y) at 4:4:4, (x >> 1, y) at 4:2:2,
 * (x >> 1, y >> 1) at 4:2:0 -- without interpolation.  The six integers are round(c * 2^14) of the real matrix that composes BT.709
 * YCbCr -> R'G'B' (Kr = 0.2126, Kb = 0.0722) with R'G'B' -> BT.601 YCbCr (Kr = 0.299, Kb = 0.114):
 *      0.101579   0.196076
 *      0.989854  -0.110653
 *     -0.072453   0.983398
 * Each of the three terms is within 0.51 of the real-valued one over all 65 536 (cb, cr); Cb = Cr = 128 is the identity, so grey stays
 * grey.  The file is byte for byte the file jpegamd_encode_ycbcr_batch_async writes for the planes (Y', Cb', Cr').
 * With JPEGAMD_MATRIX_BT601 this IS jpegamd_encode_ycbcr_samples_batch_async: no pass, no scratch, the same launches, the same files.
 * Layouts, subsamplings, formats, ranges, context sizing, capacity behaviour, status, statistics and profiling are those of that entry
 * (in a profiled call the pass opens ns_total), and so are its argument checks; any other matrix is refused with JPEGAMD_ERR_ARG, like
 * them before the context is read. */
#define JPEGAMD_MATRIX_BT601 0   /* the samples are BT.601 YCbCr, as JFIF defines it: coded as given */
#define JPEGAMD_MATRIX_BT709 1   /* the samples are BT.709 YCbCr: converted to BT.601 by the map above, in one pass in front of the tile kernel */
int32_t jpegamd_encode_ycbcr_matrix_batch_async(JpegAmdEncoder *enc, const JpegAmdYCbCrImage *imgs, int32_t count, int32_t subsampling,
                                                int32_t sample_range, int32_t sample_format, int32_t matrix, void *const *outs_dev,
                                                uint64_t out_capacity, void *const *out_sizes_dev, void *stream);

/* Colour files with ONE scan of interleaved MCUs -- what Motion-JPEG containers, RTP/JPEG, hardware and most embedded decoders
 * need, and what a decoder can take in a streaming fashion.  The file: the colour prefix of the entries above unchanged up to and
 * including its four DHT segments, then ONE SOS (FF DA 00 0C 03 01 00 02 11 03 11 00 3F 00), one entropy-coded segment, EOI; no
 * restart markers.  With (hs, vs) = (1,1) at 4:4:4, (2,2) at 4:2:0, (2,1) at 4:2:2 the MCU grid is ceil(W / 8hs) x ceil(H / 8vs),
 * coded in raster order; inside an MCU the Y blocks (v outer, u inner), then the Cb block, then the Cr block.  A real block's 64
 * quantised coefficients are exactly those the three-scan entries code for the same picture.  A Y block beyond the picture's last
 * block column or row (the MCU grid overhangs it) is a pad block: its 63 AC coefficients are zero and its DC is that of the nearest
 * real block (clamped block coordinates) -- libjpeg's choice; a decoder discards it.  Coding is T.81 F.1.2 with the Annex K tables of
 * the prefix, one DC predictor per component running through that component's blocks in scan order, pad blocks included.  The file
 * decodes to the same pixels as the three-scan file of the same picture.
 * jpegamd_encode_color_interleaved_batch_async follows jpegamd_encode_color_batch_async (JPEGAMD_ORDER_BGR / _RGB, either row order,
 * all three subsamplings; GRAY, RGBA and BGRA: JPEGAMD_ERR_ARG), jpegamd_encode_ycbcr_interleaved_batch_async follows
 * jpegamd_encode_ycbcr_batch_async (8-bit, full-range, BT.601 samples in JPEGAMD_CHROMA_PLANES, _CBCR, _CRCB; out_sizes_dev[i] a
 * DEVICE uint64_t; _YUYV / _UYVY: JPEGAMD_ERR_ARG): count 1 .. JPEGAMD_MAX_BATCH of one geometry, the context created as for those
 * entries, no host synchronisation inside the call, bad arguments refused with JPEGAMD_ERR_ARG before the context is read.  A picture
 * that does not fit out_capacity gets size 0, nothing is written past out_capacity, the other pictures are unaffected and
 * jpegamd_encoder_finish returns JPEGAMD_ERR_HUFF_CAPACITY.  finish reports the last picture's size; entropy_bits, stuffed_bytes and
 * exact_fallbacks are sums over the batch (exact_fallbacks equals the three-scan entry's figure: pad blocks add none).  With
 * profiling on, a call records ns_total only.  jpegamd_encoder_set_pipeline has no effect on these entries.
 * This is a first version: the coefficients make a round trip through device memory (the stage-tap build of the tile kernel stores
 * them, one launch per picture and component; k_mcu_segments codes them in MCU order; the unchanged k_finalize writes the file), so
 * it is slower per picture than the three-scan entries.  Its scratch -- the coefficient planes and the path's own segment arrays
 * -- is allocated on the context's first interleaved call, sized for that call and grown when a later one needs more; a large batch
 * goes through in groups of pictures that bound it.  Limited range, 16-bit samples, BT.709, packed 4:2:2, planar RGB and 4-byte
 * pixels in one scan: the three entries further down (jpegamd_encode_ycbcr_interleaved_matrix_batch_async and its neighbours).
 * Y210 and a single-picture or row-sharded one-scan entry are follow-ups. */
int32_t jpegamd_encode_color_interleaved_batch_async(JpegAmdEncoder *enc, const JpegAmdImage *imgs, int32_t count, int32_t subsampling,
                                                     void *const *outs_dev, uint64_t out_capacity, uint64_t *const *out_sizes_dev,
                                                     void *stream);
int32_t jpegamd_encode_ycbcr_interleaved_batch_async(JpegAmdEncoder *enc, const JpegAmdYCbCrImage *imgs, int32_t count, int32_t subsampling,
                                                     void *const *outs_dev, uint64_t out_capacity, void *const *out_sizes_dev, void *stream);
/* Upper bound on the interleaved file's bytes: 640 (the prefix) + 2 * (ceil(nb * 1723 / 8) + 1) + 2 + 16 with
 * nb = mx * my * (hs * vs + 2) blocks, pad blocks included (jpegamd_max_jfif_bytes_color does not count those); 0 for bad args. */
/* (With metadata set on the context -- jpegamd_encoder_set_metadata -- a buffer needs jpegamd_encoder_metadata_bytes() more than this bound.) */
uint64_t jpegamd_max_jfif_bytes_interleaved(int32_t width, int32_t height, int32_t subsampling);

/* The one-scan files with RESTART INTERVALS (DRI / RSTn, T.81 B.2.4.4, E.1.4) -- what an RTP/JPEG sender puts into
 * its restart header (RFC 2435) so that a lost packet costs one interval, what a decoder uses to decode a scan in parallel, and what
 * libjpeg's -restart writes.  restart_interval = Ri is in MCUs, 1 .. 65535; with M = mx * my MCUs the scan has n = ceil(M / Ri)
 * intervals.  The file:
 *   1. the prefix of the one-scan file with one DRI segment FF DD 00 04 hi(Ri) lo(Ri) directly in front of the SOS, behind the last
 *      DHT: 6 bytes longer, nothing else changed;
 *   2. interval i codes the MCUs [i Ri, min((i + 1) Ri, M)) of the raster MCU order -- block order, tables, ZRL / EOB and the pad-block
 *      rule (no AC, the DC VALUE of the nearest real block) as above.  At the start of every interval the DC predictors of all three
 *      components are 0; a pad block's difference is taken against the predictor like any other block's;
 *   3. every interval but the last: its bit string is padded with 1-bits to a whole byte (nothing when it ends on one), every 0xFF
 *      byte of it, the padded one included, is followed by a stuffed 0x00, then comes the marker FF D0+(i mod 8), unstuffed;
 *   4. the last interval ends with the zero-bit flush of the other scans, then EOI; it has no RST marker;
 *   5. Ri >= M (one interval): the one-scan file of the same picture with the DRI segment inserted, byte for byte.
 * restart_interval 0: the entry IS the entry without _restart -- same launches, same file, no DRI.  Any other value outside
 * 1 .. 65535: JPEGAMD_ERR_ARG, refused like every other bad argument before the context is read.  Sources, layouts, subsamplings,
 * context sizing, refusals, capacity behaviour (size 0, nothing past out_capacity, the other pictures unaffected,
 * JPEGAMD_ERR_HUFF_CAPACITY from finish, the context usable afterwards), profiling (ns_total only) and set_pipeline are those of the
 * entries above.  entropy_bits is the sum of the coded bits (pad and flush bits are not counted), stuffed_bytes counts the 0x00
 * stuffing bytes, those behind padded bytes included, markers not; exact_fallbacks is the three-scan figure.
 * A segment of the coder never crosses an interval's boundary, so a short interval means many short segments: the path's scratch per
 * picture is the coefficient planes plus, per segment, a string reserved for min(Ri, S) MCUs (S = 256 / (hs vs + 2)) and 56 bytes of
 * numbers.  When that exceeds the path's 4 GiB group budget for ONE picture (Ri = 1: from about 15000 x 15000 at 4:4:4, 21500 x 21500 at 4:2:0) the call
 * answers JPEGAMD_ERR_TOO_LARGE before anything is allocated or launched. */
int32_t jpegamd_encode_color_interleaved_restart_batch_async(JpegAmdEncoder *enc, const JpegAmdImage *imgs, int32_t count, int32_t subsampling,
                                                             int32_t restart_interval, void *const *outs_dev, uint64_t out_capacity,
                                                             uint64_t *const *out_sizes_dev, void *stream);
int32_t jpegamd_encode_ycbcr_interleaved_restart_batch_async(JpegAmdEncoder *enc, const JpegAmdYCbCrImage *imgs, int32_t count, int32_t subsampling,
                                                             int32_t restart_interval, void *const *outs_dev, uint64_t out_capacity,
                                                             void *const *out_sizes_dev, void *stream);
/* Upper bound on the bytes of the file with restart intervals: jpegamd_max_jfif_bytes_interleaved + 6 + 4 * (n - 1).  That bound holds
 * the scan's bits rounded up to a byte once with every byte stuffed; the DRI segment adds 6 bytes, and every interval but the last
 * rounds up on its own -- at most one more byte --, may have that byte stuffed, and ends with two marker bytes.  With
 * restart_interval 0 it equals jpegamd_max_jfif_bytes_interleaved; 0 for bad arguments (restart_interval outside 0 .. 65535 too). */
/* (With metadata set on the context -- jpegamd_encoder_set_metadata -- a buffer needs jpegamd_encoder_metadata_bytes() more than this bound.) */
uint64_t jpegamd_max_jfif_bytes_interleaved_restart(int32_t width, int32_t height, int32_t subsampling, int32_t restart_interval);

/* The one-scan files from EVERY source the three-scan entries read.  No new file: the one-scan file above -- with
 * restart_interval 1 .. 65535 the file with restart intervals, with 0 the file without; anything else JPEGAMD_ERR_ARG -- built from
 * the 8-bit full-range BT.601 Y, Cb and Cr samples that the three-scan entry of the same input codes.  Prefix, DRI, SOS, MCU order,
 * pad rule, DC predictors, stuffing, RSTn, flush, the two bounds above, capacity behaviour, statistics (exact_fallbacks: the
 * three-scan entry's figure for the same input), profiling and context sizing are those of the entries above; arguments are checked
 * before the context is read.
 *   jpegamd_encode_ycbcr_interleaved_matrix_batch_async takes exactly what jpegamd_encode_ycbcr_matrix_batch_async takes and refuses
 *     what it refuses: any chroma layout (packed _YUYV / _UYVY at JPEGAMD_SUBSAMPLE_422 alone), sample_range FULL / LIMITED,
 *     sample_format 8 / 10_MSB / 10_LSB (packed with 16-bit samples, Y210: JPEGAMD_ERR_ARG), matrix BT601 / BT709.  The samples are
 *     the caller's after the depth map, the range map and -- BT.709 -- the matrix map, in that order, sample for sample.  Every kind
 *     but BT.709 is read where it lies by the tile kernel; a BT.709 batch runs the one pass of the three-scan entry first.  With
 *     8-bit full-range BT.601 samples in planes or pairs the file is jpegamd_encode_ycbcr_interleaved_restart_batch_async's, byte for
 *     byte.
 *   jpegamd_encode_color_interleaved_pixels_batch_async takes JPEGAMD_ORDER_BGR, _RGB, _RGBA and _BGRA (GRAY and unknown orders:
 *     JPEGAMD_ERR_ARG); the file is that of the same R, G, B values stored as packed RGB.
 *   jpegamd_encode_planar_interleaved_batch_async takes three planes per picture, as jpegamd_encode_planar_batch_async; subsampling 0
 *     (no grayscale one-scan file) is JPEGAMD_ERR_ARG. */
int32_t jpegamd_encode_ycbcr_interleaved_matrix_batch_async(JpegAmdEncoder *enc, const JpegAmdYCbCrImage *imgs, int32_t count,
                                                            int32_t subsampling, int32_t sample_range, int32_t sample_format, int32_t matrix,
                                                            int32_t restart_interval, void *const *outs_dev, uint64_t out_capacity,
                                                            void *const *out_sizes_dev, void *stream);
int32_t jpegamd_encode_color_interleaved_pixels_batch_async(JpegAmdEncoder *enc, const JpegAmdImage *imgs, int32_t count, int32_t subsampling,
                                                            int32_t restart_interval, void *const *outs_dev, uint64_t out_capacity,
                                                            uint64_t *const *out_sizes_dev, void *stream);
int32_t jpegamd_encode_planar_interleaved_batch_async(JpegAmdEncoder *enc, const JpegAmdPlanarImage *imgs, int32_t count, int32_t subsampling,
                                                      int32_t restart_interval, void *const *outs_dev, uint64_t out_capacity,
                                                      void *const *out_sizes_dev, void *stream);

/* Which kernels follow k_tile_encode for whole pictures (no reference counterpart: a tuning knob, results are byte-identical).
 *   PAIR    k_segment_merge + k_finalize: the tiles' bit strings joined per segment, then stitched behind a kernel boundary;
 *   STITCH  k_stitch: one pass, the offsets handed from workgroup to workgroup inside the launch (decoupled look-back);
 *   AUTO    (default) PAIR, and STITCH for pictures of 16 384 segments and more (16384^2 and up), where k_finalize's scan over
 *           every predecessor of every workgroup would grow quadratically.
 * Takes effect with the next encode on the context. */
#define JPEGAMD_PIPELINE_AUTO   0
#define JPEGAMD_PIPELINE_PAIR   1
#define JPEGAMD_PIPELINE_STITCH 2
int32_t jpegamd_encoder_set_pipeline(JpegAmdEncoder *enc, int32_t pipeline);

/* The Huffman tables of the ONE-SCAN colour files: the entries named *_interleaved_* above and below.
 *   STANDARD   (default) the Annex K tables: every entry launches what it launched and writes the bytes it wrote;
 *   OPTIMIZED  four tables made for each picture from its own symbol counts, as libjpeg -optimize / PIL optimize=True make them.
 * Takes effect with the next encode on the context; any other value, or a null context: JPEGAMD_ERR_ARG.
 * The OPTIMIZED file equals the STANDARD one-scan file of the same input and restart interval except for the four DHT segments and
 * the code words of the scan: coefficients, MCU order, pad blocks, DC predictors and their reset per interval, 1-bit padding,
 * stuffing, RSTn, flush, EOI, every byte in front of the first DHT, the DRI segment and the SOS are unchanged.
 *   Counts.  Four tables per picture: luma DC (Tc/Th 0/0) from the DC size symbols of the Y blocks, luma AC (1/0) from their AC
 *     run/size symbols, chroma DC (0/1) and chroma AC (1/1) from those of the Cb and Cr blocks together.  Every symbol the scan codes
 *     with the call's restart interval counts: a pad block's DC symbol and its EOB, every ZRL, every EOB, and the DC differences
 *     taken against a predictor of 0 at each interval's start -- the counts depend on the interval.
 *   Tables.  T.81 K.2 as libjpeg carries it out, for counts f[0..255]:
 *     1. f[256] = 1 (a reserved point: no code word is all ones); every index with f > 0 is a tree of one symbol, size[s] = 0;
 *     2. repeat: c1 = the tree root with the least f > 0, the highest index among equals; c2 = the same among the other roots; stop
 *        when there is none; f[c1] += f[c2], f[c2] = 0, size[s] += 1 for every symbol of both trees, whose root becomes c1;
 *     3. n[l] = the symbols with size == l, the reserved one included (l may reach 256);
 *     4. for l from the largest used length down to 17, while n[l] > 0: j = l - 2; while n[j] == 0, j -= 1;
 *        n[l] -= 2, n[l-1] += 1, n[j+1] += 2, n[j] -= 1;
 *     5. l = the largest length with n[l] > 0: n[l] -= 1 (the reserved point leaves);
 *     6. BITS[l] = n[l], l = 1 .. 16; HUFFVAL = the real symbols with f > 0 ordered by (size of step 2, symbol value); the code words
 *        are the canonical ones of T.81 Annex C -- a symbol's final length follows from its place in HUFFVAL against BITS.
 *     A table with one used symbol gives it the 1-bit code 0.
 *   DHT.  Four segments where the standard four stand, in their order (Tc/Th 00, 10, 01, 11): FF C4, length 19 + nvals, the Tc/Th
 *     byte, 16 BITS bytes, HUFFVAL.  The prefix's length differs from picture to picture of a batch and never exceeds the standard one's.
 * Capacity behaviour, status, profiling (ns_total only) and context sizing are those of the STANDARD call; entropy_bits is the sum of
 * the bits actually coded, stuffed_bytes and exact_fallbacks keep their meaning.  jpegamd_max_jfif_bytes_interleaved and
 * jpegamd_max_jfif_bytes_interleaved_restart remain upper bounds: an optimised DC symbol is at most 16 + 11 bits and an AC symbol
 * 16 + 10 (an AC coefficient of 8-bit samples is below 1024 in magnitude for this quantiser as for T.81), 27 + 63 x 26 bits a block --
 * below the 22 + 63 x 27 the bounds and the path's reservations are made of.  The scratch of the mode -- per picture 4.3 KB of
 * counters, 2.2 KB of coder tables, one prefix slot -- is allocated with the path's scratch on the context's first OPTIMIZED call.
 * It governs jpegamd_encode_gray_scan_batch_async (further down) as well, with two tables per picture.  No effect on the other
 * grayscale entries and the three-scan, row-sharded, DTO and file entries, whose coder is inside the tile kernel: optimised tables
 * for those are a follow-up. */
#define JPEGAMD_HUFFMAN_STANDARD  0
#define JPEGAMD_HUFFMAN_OPTIMIZED 1
int32_t jpegamd_encoder_set_huffman(JpegAmdEncoder *enc, int32_t huffman);
/* Tests.  Both synchronous, host pointers; bad arguments are refused with JPEGAMD_ERR_ARG before the device is touched.
 * jpegamd_debug_optimal_huffman: the device's table builder on `n` (1 .. 4096) arbitrary tables of 256 counts, each table's counts
 * summing to less than 2^54 -> BITS [n][16], HUFFVAL [n][256] (zeros behind the used ones), the number of HUFFVAL bytes [n].
 * jpegamd_debug_huffman_counts: the symbol counts of the context's last OPTIMIZED call, [pictures of that call][4][256] in the table
 * order above (a DC table's at 0 .. 15); JPEGAMD_ERR_ARG when the context made no such call. */
int32_t jpegamd_debug_optimal_huffman(JpegAmdEncoder *enc, const uint64_t *freq, int32_t n, uint8_t *bits, uint8_t *vals, int32_t *nvals);
int32_t jpegamd_debug_huffman_counts(JpegAmdEncoder *enc, uint64_t *counts);

/* CALLER-SUPPLIED QUANTISATION TABLES.
 * Annex K scaled for `quality` (0 -> 50), raster order, as the encoder derives them; either pointer may be NULL. */
int32_t jpegamd_quant_tables_for_quality(int32_t quality, uint8_t *luma, uint8_t *chroma);
/* Tables of the caller's for every later encode on this context.  uint8[64], RASTER order (the order of
 * jpegamd_debug_quant_table and of cjpeg -qtables), entries 1..255.
 *   luma, chroma   : component 1 uses luma, components 2 and 3 use chroma
 *   luma, NULL     : one table for all components (a colour file still carries DQT ids 0 and 1, identical: no prefix changes length)
 *   NULL, NULL     : back to the tables of each picture's `quality`
 *   NULL, chroma   : JPEGAMD_ERR_ARG
 * An entry of 0: JPEGAMD_ERR_ARG, and the context keeps what it had.  The tables are copied.
 * The setting is sticky on the context, like jpegamd_encoder_set_huffman.  While tables are set a picture's `quality` selects
 * nothing (the batch entries still want it uniform).  The file is the one the same entry writes for a quality, with these two
 * tables in its DQT segment (zigzag order there) and in its quantiser and nothing else changed; for the tables of
 * jpegamd_quant_tables_for_quality(q) it is byte for byte the file of quality q.
 * The call itself touches no device memory and does not disturb queued work.  The NEXT encode uploads the quantiser's constants
 * and the file headers by the route a change of `quality` takes -- which waits for the work queued on this context before it
 * rewrites them, so a table switch costs a stream wait exactly as a quality switch does.
 * Every jpegamd_max_jfif_bytes* bound holds unchanged: each is made of per-block worst cases that already cover the all-ones
 * table (quality 100), the finest an 8-bit table can be.
 * The tables govern every encode entry that takes a context: jpegamd_encode_async / _batch_async, the three-scan, one-scan,
 * gray-scan and progressive entries from every source, jpegamd_encode_rows_async / export / import / jpegamd_finalize_async (every
 * rank sets the same tables) and jpegamd_debug_stages.  convertToJpeg, the stage functions and the BMP and file entries own their
 * contexts and stay quality-only. */
int32_t jpegamd_encoder_set_quant_tables(JpegAmdEncoder *enc, const uint8_t *luma, const uint8_t *chroma);
/* What the context holds: *custom = 1 and the two tables, or *custom = 0 (tables untouched). */
int32_t jpegamd_encoder_get_quant_tables(JpegAmdEncoder *enc, uint8_t *luma, uint8_t *chroma, int32_t *custom);

/* METADATA: ICC profile, Exif, comment, pixel density, segments of the caller's.
 * Let F be the file an entry writes for some call.  For a context that holds metadata the file is
 *     F[0, 20) with its density fields replaced  |  B  |  F[20, ..)
 * F[0, 20) is SOI and the JFIF APP0 segment: byte 13 the density units (0 aspect ratio, 1 dots per inch, 2 dots per cm), bytes
 * 14 .. 17 the X and Y density (big-endian, 1 .. 65535 each); with density_units -1 they stay 01 0060 0060 (96 dpi).
 * B, the "blob" of M bytes, is a sequence of complete marker segments -- FF mm, a big-endian length of payload + 2, the payload -- in
 * this order:
 *   1. Exif      FFE1, "Exif\0\0" + the caller's TIFF block (exif / exif_len; at most 65527 bytes)
 *   2. segments  the caller's own, in the caller's order: at most 16, markers 0xE1 .. 0xEF and 0xFE only, 0 .. 65533 bytes of payload
 *                each, not interpreted (XMP, MPF, a second comment)
 *   3. ICC       the profile cut into chunks of at most 65519 bytes; each FFE2, "ICC_PROFILE\0" + the chunk's number (from 1) + the
 *                number of chunks + the chunk, as libjpeg's jpeg_write_icc_profile writes it.  More than 255 chunks (a profile above
 *                16707345 bytes): refused
 *   4. comment   FFFE, 0 .. 65533 bytes; a non-NULL pointer with length 0 writes an empty COM segment, NULL writes none
 * A NULL exif / icc pointer writes no such segment; an exif or icc pointer with length 0 writes none either.  The bytes are copied
 * verbatim: an FF inside a payload is not stuffed.  Nothing behind offset 20 of F changes, for any entry, source, subsampling,
 * scan kind, restart interval, Huffman mode, scan script or quantisation tables. */
typedef struct {
    int32_t marker;             /* 0xE1 .. 0xEF, 0xFE */
    const uint8_t *data;        /* the payload; NULL only with len 0 */
    uint32_t len;               /* 0 .. 65533 */
} JpegAmdSegment;
typedef struct {
    int32_t density_units;      /* -1: leave 96 dpi (x_density, y_density are not looked at); 0, 1, 2 */
    int32_t x_density, y_density;   /* 1 .. 65535 */
    const uint8_t *exif;        /* the TIFF block, WITHOUT the "Exif\0\0" identifier */
    uint32_t exif_len;
    const uint8_t *icc;
    uint64_t icc_len;
    const uint8_t *comment;
    uint32_t comment_len;
    const JpegAmdSegment *segments;
    int32_t segment_count;      /* 0 .. 16 */
} JpegAmdMetadata;
#define JPEGAMD_METADATA_HEAD_BYTES 20
#define JPEGAMD_METADATA_MAX_SEGMENTS 16
/* THE definition of B and of the 20 leading bytes; everything else goes through it.  Host only: no context, no device.  Validates
 * `m`, returns M (>= 0), fills `blob` when M <= capacity (a NULL blob with capacity 0 asks for the length alone; a capacity that is
 * too small still returns M and writes nothing), and fills `head` (may be NULL) with the 20 leading bytes.  JPEGAMD_ERR_ARG: m NULL,
 * any refusal above, a NULL pointer with a non-zero length, a NULL blob with a capacity. */
int64_t jpegamd_build_metadata(const JpegAmdMetadata *m, uint8_t *blob, uint64_t capacity, uint8_t *head /*[20]*/);
/* Metadata for every later encode on this context; `m` NULL (or a description that sets nothing) clears it.  Everything is copied:
 * the caller may free its buffers at once.  Sticky on the context, like jpegamd_encoder_set_quant_tables.  An invalid description:
 * JPEGAMD_ERR_ARG, and the context keeps what it had.
 * The call itself touches no device memory and does not disturb queued work.  The NEXT encode uploads the 20 + M bytes into context
 * scratch that only grows -- behind the work queued on this context, so a switch costs a stream wait as a switch of quantisation
 * tables does.
 * CAPACITY.  No jpegamd_max_jfif_bytes* changes: a caller sizes its buffers as bound + jpegamd_encoder_metadata_bytes().  With M
 * bytes set an entry behaves towards out_capacity as it does without metadata towards out_capacity - M (a capacity <= M counts
 * as 0): a file that fits has its size + M in the size word; a size word the entry leaves non-zero for a file that did NOT fit (the
 * would-be size) has + M too, a zero stays zero; JPEGAMD_ERR_HUFF_CAPACITY is raised exactly when it would be for out_capacity - M;
 * nothing is written at or beyond out + out_capacity, nor in front of out.  JpegAmdStats.jfif_bytes includes M; every other field is
 * what the call reports without metadata.
 * With nothing set every entry writes the bytes it wrote before, with the launches it made before.  With metadata set each call
 * makes ONE more launch (k_metadata_place) behind its own.
 * The metadata governs every encode entry that takes a context and writes whole files: jpegamd_encode_async / _batch_async (with
 * with_container 0 -- a bare scan, no file -- they return JPEGAMD_ERR_ARG while metadata is set), the three-scan and one-scan colour,
 * planar and YCbCr entries with and without restart intervals, the gray-scan entry and every progressive entry.  One description
 * serves every picture of a batch.  jpegamd_encode_rows_async / export / import / jpegamd_finalize_async and jpegamd_debug_stages
 * return JPEGAMD_ERR_ARG while metadata is set rather than drop it silently.  convertToJpeg, the stage functions and the BMP and
 * file entries own their contexts and write no metadata. */
int32_t jpegamd_encoder_set_metadata(JpegAmdEncoder *enc, const JpegAmdMetadata *m);
/* M of the metadata the context holds (0: none, or a density alone). */
int64_t jpegamd_encoder_metadata_bytes(JpegAmdEncoder *enc);

/* GRAYSCALE files with restart intervals and per-picture optimised Huffman tables: the grayscale file written as
 * a scan of ONE component from coefficient planes, the way the one-scan colour files are.  For a picture of W x H at quality q,
 * restart_interval = Ri (0 .. 65535, in MCUs) and the context's Huffman mode (jpegamd_encoder_set_huffman governs this entry too):
 *   Prefix.  The 328-byte prefix of jpegamd_encode_batch_async(..., with_container = 1): SOI, APP0, DQT, SOF0 with one component,
 *     DHT 0/0 (K.3), DHT 1/0 (K.5), SOS FF DA 00 08 01 01 00 00 3F 00.  Ri > 0: one DRI segment FF DD 00 04 hi lo directly in front
 *     of the SOS, behind the last DHT.  JPEGAMD_HUFFMAN_OPTIMIZED: the picture's own two DHT segments stand where the standard two
 *     stand, in the same order (Tc/Th 00, then 10), each FF C4, length 19 + nvals, the Tc/Th byte, 16 BITS bytes, HUFFVAL.
 *   Scan.  A non-interleaved scan of one component: the MCU is one block.  The bw x bh = ceil(W / 8) x ceil(H / 8) blocks are coded
 *     in raster order, M = bw bh; there are no pad blocks.  A block's 64 coefficients are exactly those the grayscale entries code
 *     for the same picture.  Coding is T.81 F.1.2.
 *   Intervals.  With Ri > 0 interval i codes the blocks [i Ri, min((i + 1) Ri, M)); the DC predictor is 0 at its first block.  Rules
 *     3 - 5 of the colour files' restart section above apply unchanged: every interval but the last is padded with 1-bits, every
 *     0xFF is stuffed (the padded byte too), then FF D0+(i mod 8); the last interval ends with the zero-bit flush, then EOI; Ri >= M
 *     gives the file without intervals with the DRI segment inserted, byte for byte.
 *   Tables in OPTIMIZED mode.  The DC table is built from the DC size symbols of all blocks, differences taken against 0 at every
 *     interval start -- the counts depend on Ri; the AC table from the run/size symbols, every ZRL and EOB included.  The construction
 *     is the one written down for JPEGAMD_HUFFMAN_OPTIMIZED above; a table with one used symbol gets the 1-bit code 0.
 * Pictures, count (1 .. JPEGAMD_MAX_BATCH, one geometry) and context sizing are those of jpegamd_encode_batch_async; all five channel
 * orders are taken (GRAY, and the luma of BGR, RGB, RGBA and BGRA pictures), either row order, any valid stride.  restart_interval
 * outside 0 .. 65535 and every other bad argument: JPEGAMD_ERR_ARG before the context is read.  A picture whose scratch alone exceeds
 * the path's 4 GiB group budget (small Ri on huge pictures): JPEGAMD_ERR_TOO_LARGE before anything is allocated or launched.
 * restart_interval 0 with JPEGAMD_HUFFMAN_STANDARD IS jpegamd_encode_batch_async with with_container = 1: same launches, file,
 * statistics and profiling.  Every other combination takes the coefficient route of the one-scan colour entries -- per picture one
 * stage-tap launch of the tile kernel; per group of pictures the symbol counts and table builder when OPTIMIZED, the coder, the
 * restart writer -- and shares their behaviour: a picture that does not fit out_capacity gets size 0, nothing is written past
 * out_capacity, the other pictures are unaffected, jpegamd_encoder_finish returns JPEGAMD_ERR_HUFF_CAPACITY and the context stays
 * usable; entropy_bits and stuffed_bytes as defined there, exact_fallbacks the grayscale entry's figure; with profiling on a call
 * records ns_total only; jpegamd_encoder_set_pipeline has no effect.  After an OPTIMIZED call jpegamd_debug_huffman_counts keeps its
 * [pictures][4][256] shape with tables 2 and 3 all zero.
 * The bound.  jpegamd_max_jfif_bytes is NOT an upper bound for the OPTIMIZED file: an optimised DC symbol may take 16 + 11 bits where
 * Annex K's takes at most 9 + 11.  jpegamd_max_jfif_bytes_gray_scan = 328 + 2 * (ceil(M * 1723 / 8) + 1) + 2 + 16, and with
 * restart_interval > 0 and n = ceil(M / Ri) intervals + 6 + 4 * (n - 1): a block of either mode is below 22 + 63 x 27 = 1723 bits
 * (optimised: at most 27 + 63 x 26 = 1665; the coder's string of a segment is reserved for 256 blocks of 1723), the scan rounds up
 * to a byte once and every byte may be stuffed, then EOI; the DRI segment adds 6 bytes, and every interval but the last rounds up on
 * its own -- at most one more byte --, may have that byte stuffed, and ends with two marker bytes.  0 for bad arguments (a dimension
 * outside 1 .. 65535, restart_interval outside 0 .. 65535). */
int32_t jpegamd_encode_gray_scan_batch_async(JpegAmdEncoder *enc, const JpegAmdImage *imgs, int32_t count, int32_t restart_interval,
                                             void *const *outs_dev, uint64_t out_capacity, uint64_t *const *out_sizes_dev, void *stream);
/* (With metadata set on the context -- jpegamd_encoder_set_metadata -- a buffer needs jpegamd_encoder_metadata_bytes() more than this bound.) */
uint64_t jpegamd_max_jfif_bytes_gray_scan(int32_t width, int32_t height, int32_t restart_interval);

/* Progressive colour files (SOF2): seven scans by spectral selection, no successive approximation (Ah = Al = 0 in every scan).  The
 * file holds the coefficients of the one-scan file of the same input (jpegamd_encode_color_interleaved_pixels_batch_async,
 * jpegamd_encode_ycbcr_interleaved_matrix_batch_async), so a decoder reconstructs the same pixels.  What this version gives is the
 * progressive rendering; the file is a little LARGER than the one-scan file (six more SOS headers, an end-of-band symbol per block
 * and band, seven flushes), because no end-of-band runs are coded: the entries with per-scan optimised tables further down code them.
 *   Layout.  The one-scan file's prefix up to and including its four Annex K DHT segments, with ONE change: the frame header's
 *     marker is FF C2 where that file has FF C0 (length, contents and the sampling factors 0x11 / 0x22 / 0x21 stay).  Then seven
 *     scans, each an SOS segment and a byte-aligned entropy-coded segment, then EOI:
 *       scan 1      Y, Cb, Cr interleaved, Ss..Se = 0..0     FF DA 00 0C 03 01 00 02 11 03 11 00 00 00
 *       scan 2 3 4  Y, Cb, Cr (one each),  Ss..Se = 1..5     FF DA 00 08 01 cc tt 01 05 00   (tt = 00 for Y, 11 for Cb and Cr)
 *       scan 5 6 7  Y, Cb, Cr (one each),  Ss..Se = 6..63    FF DA 00 08 01 cc tt 06 3F 00
 *   Scan 1, the DC scan.  The MCU order, the pad blocks and the per-component predictors of the one-scan file; a pad block's DC is
 *     the DC of the nearest real block.  Every block codes its DC difference alone, with its component's DC table: no AC symbol, no EOB.
 *   Scans 2 - 7.  The blocks of the component's OWN block grid in raster order: bw x bh for Y -- no pad blocks --, mx x my for Cb
 *     and Cr.  A block codes its coefficients Ss .. Se as T.81 G.1.2.2 defines them, with the component's Annex K AC table: the zero
 *     run is 0 at Ss; sixteen zeros are ZRL (0xF0); the block ends with symbol 0x00 -- EOB0, an end-of-band run of exactly one block --
 *     when coefficient Se is zero, and with no end symbol when it is not.  NO end-of-band run longer than one block is coded: the
 *     Annex K tables hold no EOBn symbol for n >= 1.
 *   Every scan.  A 0x00 behind every 0xFF; the last byte padded with zero bits; no restart intervals.
 * jpegamd_encode_color_progressive_batch_async takes the pictures of jpegamd_encode_color_interleaved_pixels_batch_async (BGR, RGB,
 * RGBA, BGRA), jpegamd_encode_ycbcr_progressive_batch_async everything jpegamd_encode_ycbcr_interleaved_matrix_batch_async reads,
 * with the same sample_range, sample_format and matrix.  Each refuses what its one-scan twin refuses, and JPEGAMD_ORDER_GRAY, and a
 * context set to JPEGAMD_HUFFMAN_OPTIMIZED (per-scan optimised tables are the entries below): JPEGAMD_ERR_ARG with nothing allocated
 * or launched.  Batching, context sizing, capacity handling and profiling are the one-scan entries': a picture that does not fit
 * out_capacity gets size 0, nothing is written past out_capacity (what was written of its first scan stays in the buffer), the other
 * pictures are unaffected, jpegamd_encoder_finish returns JPEGAMD_ERR_HUFF_CAPACITY and the context stays usable.  finish reports
 * the coded bits and stuffed bytes summed over the seven scans of every picture of the call, exact_fallbacks of the three tap
 * launches counted once, and the last picture's file size.  The scans 2 - 7 are staged in context scratch at their worst-case
 * sizes (about 425 bytes per block of every component: 1.3 GiB for an 8192 x 8192 picture at 4:4:4), which counts into the 4 GiB budget that groups the pictures of a call.
 * The bound.  jpegamd_max_jfif_bytes_progressive = jpegamd_max_jfif_bytes_interleaved + 6 * (10 + 2).  That bound takes every block
 * of every MCU, pad blocks too, at 22 + 63 x 27 = 1723 bits, every byte stuffed, one rounding up to a byte, and EOI.  Here a block's
 * DC difference is at most 11 + 11 bits, and a band costs at most 27 bits per coefficient -- every non-zero coefficient is one
 * symbol of at most 16 + 11 bits, a ZRL of at most 11 bits pays for sixteen zero coefficients, the EOB for the zero coefficient
 * Se --, so the bands 1..5 and 6..63 are at most 135 and 1566 bits and the three together 1723: what the seven scans code of a
 * block (pad blocks: the DC alone) costs no more than that bound allows it.  Six more SOS segments add 6 * 10 bytes; seven scans
 * round up to a byte seven times where the one scan rounds once -- at most six more bytes, each of which may be stuffed: 6 * 2.
 * 0 for bad arguments (a dimension outside 1 .. 65535, an invalid subsampling). */
int32_t jpegamd_encode_color_progressive_batch_async(JpegAmdEncoder *enc, const JpegAmdImage *imgs, int32_t count, int32_t subsampling,
                                                     void *const *outs_dev, uint64_t out_capacity, uint64_t *const *out_sizes_dev,
                                                     void *stream);
int32_t jpegamd_encode_ycbcr_progressive_batch_async(JpegAmdEncoder *enc, const JpegAmdYCbCrImage *imgs, int32_t count, int32_t subsampling,
                                                     int32_t sample_range, int32_t sample_format, int32_t matrix,
                                                     void *const *outs_dev, uint64_t out_capacity, void *const *out_sizes_dev,
                                                     void *stream);
/* (With metadata set on the context -- jpegamd_encoder_set_metadata -- a buffer needs jpegamd_encoder_metadata_bytes() more than this bound.) */
uint64_t jpegamd_max_jfif_bytes_progressive(int32_t width, int32_t height, int32_t subsampling);

/* Progressive colour files with END-OF-BAND RUNS and PER-SCAN OPTIMISED TABLES: the file above with three changes.  Unchanged: the
 * coefficients, the scan script, the SOS bytes, the MCU order, pad blocks and predictors of scan 1, stuffing, the zero-bit flush of
 * every scan, EOI.  The file is about the size of the one-scan file with per-picture optimised tables.
 *   1. No Annex K DHT segments.  The head is SOI, APP0, DQT, SOF2.  Scan 1 is preceded by its own DHT 0/0 (Y DC) and DHT 0/1 (Cb and
 *      Cr DC, counted together), in that order, then the DC scan's SOS.  Each of the scans 2 .. 7 is preceded by ONE DHT segment with
 *      Tc/Th 0x10 (Y) or 0x11 (Cb, Cr), then its 10-byte SOS: the table ids 1/0 and 1/1 are redefined from scan to scan.  Every DHT
 *      is FF C4, length 19 + nvals, the Tc/Th byte, 16 BITS bytes, HUFFVAL.  Every table is built from the counts of the symbols ITS
 *      scan codes by the construction of JPEGAMD_HUFFMAN_OPTIMIZED above: steps 1 - 6 with the reserved point, the highest index
 *      winning ties, the 16-bit limit; a table with one used symbol gives it the 1-bit code 0.
 *   2. End-of-band runs in the scans 2 .. 7 (T.81 G.1.2.2).  Blocks are indexed in the component's own raster block order.  Let E[i]
 *      mean "coefficient Se of block i is zero" and Z[i] "the coefficients Ss .. Se of block i are all zero".  A block first codes its
 *      non-zero coefficients as above -- run/size and amplitude, a ZRL per sixteen zeros, nothing for the trailing zeros.  Block i
 *      then STARTS A RUN iff E[i] and not (Z[i] and i mod 256 != 0 and E[i - 1]).  The run's length r is 1 plus the number of
 *      consecutive blocks j = i + 1, i + 2, ... with Z[j] and j mod 256 != 0.  It is coded as symbol n << 4, n = floor(log2 r),
 *      followed by the n low bits of r - 2^n.  A block that neither starts a run nor has non-zero coefficients codes nothing.
 *   3. A run never crosses a multiple of 256 blocks: r <= 256, the symbols are EOB0 .. EOB8 (0x00 .. 0x80).  (256 blocks are what
 *      one wave codes; decoders accept any partition into runs.  The cost is at most one symbol per 256 blocks.)
 *   Scan 1 is the DC scan above coded with the two optimised DC tables; pad blocks count.
 * jpegamd_encode_color_progressive_optimized_batch_async and jpegamd_encode_ycbcr_progressive_optimized_batch_async take the
 * arguments of their twins above: the same pictures, batching, context sizing, capacity behaviour (size 0,
 * JPEGAMD_ERR_HUFF_CAPACITY, nothing written past out_capacity, the other pictures unaffected), refusals and statistics -- bits and
 * stuffed bytes summed over the seven scans, exact_fallbacks counted once.  They do not read the context's Huffman mode and leave it
 * as it was (the twins keep refusing JPEGAMD_HUFFMAN_OPTIMIZED).  The scans also take the scratch of the restart writer.
 * The bound.  jpegamd_max_jfif_bytes_progressive_optimized = jpegamd_max_jfif_bytes_progressive + 780.  The scans: a DC difference
 * is at most 16 + 11 bits; a non-zero AC coefficient 16 + 10; a ZRL 16 bits for sixteen zeros; a run's symbol 16 + 8 bits, paid for
 * by the zero coefficient Se of the block that starts it.  So a block costs at most 27 + 63 x 26 = 1665 bits over all scans, below
 * the 1723 the bound above allows it, with the same roundings, stuffing and SOS segments.  The headers: an AC table has at most
 * 160 run/size symbols, ZRL and EOB0 .. EOB8 = 170 symbols, a DC table 12: the DHT segments are at most 2 x 33 + 6 x 191 = 1212
 * bytes where the four Annex K segments, which the bound above holds, are 432.  0 for bad arguments.
 * jpegamd_debug_progressive_counts (tests; synchronous, `counts` a HOST pointer): the symbol counts of the context's last such call,
 * [pictures of that call][8][256] in the file's table order -- Y DC, chroma DC, then the scans 2 .. 7.  JPEGAMD_ERR_ARG when the
 * context made no such call. */
int32_t jpegamd_encode_color_progressive_optimized_batch_async(JpegAmdEncoder *enc, const JpegAmdImage *imgs, int32_t count, int32_t subsampling,
                                                               void *const *outs_dev, uint64_t out_capacity, uint64_t *const *out_sizes_dev,
                                                               void *stream);
int32_t jpegamd_encode_ycbcr_progressive_optimized_batch_async(JpegAmdEncoder *enc, const JpegAmdYCbCrImage *imgs, int32_t count,
                                                               int32_t subsampling, int32_t sample_range, int32_t sample_format, int32_t matrix,
                                                               void *const *outs_dev, uint64_t out_capacity, void *const *out_sizes_dev,
                                                               void *stream);
/* (With metadata set on the context -- jpegamd_encoder_set_metadata -- a buffer needs jpegamd_encoder_metadata_bytes() more than this bound.) */
uint64_t jpegamd_max_jfif_bytes_progressive_optimized(int32_t width, int32_t height, int32_t subsampling);
int32_t jpegamd_debug_progressive_counts(JpegAmdEncoder *enc, uint64_t *counts);

/* Progressive colour files with SUCCESSIVE APPROXIMATION: SOF2, and the coefficients of the one-scan file of the same input -- the
 * quantiser, the pad blocks and the MCU order of the progressive file above.  The ten scans are those of libjpeg's
 * jpeg_simple_progression for YCbCr (what `cjpeg -progressive` writes), in this order:
 *     scan  components            Ss..Se  Ah Al  tables (the file's order)
 *      1    Y Cb Cr interleaved   0..0    0  1   0: Y DC, 1: Cb + Cr DC
 *      2    Y                     1..5    0  2   2
 *      3    Cr                    1..63   0  1   3
 *      4    Cb                    1..63   0  1   4
 *      5    Y                     6..63   0  2   5
 *      6    Y                     1..63   2  1   6
 *      7    Y Cb Cr interleaved   0..0    1  0   none: raw bits, its SOS alone
 *      8    Cr                    1..63   1  0   7
 *      9    Cb                    1..63   1  0   8
 *     10    Y                     1..63   1  0   9
 * The head is SOI, APP0, DQT, SOF2; there are no Annex K segments.  Every table is made of its own scan's symbol counts by the
 * construction above and written as the scan's own DHT in front of its SOS: Tc/Th 0x00 / 0x01 for the DC tables, 0x10 for Y AC scans
 * and 0x11 for chroma AC scans.  SOS: the segments above with Ss, Se and the byte Ah << 4 | Al.  Every scan is stuffed and flushed
 * with 0-bits; EOI follows the last.
 *   First DC scan (Ah = 0).  The value is DC >> Al, an arithmetic shift; the difference to the previous block's shifted value (0 in
 *     front of a component's first block) is coded as a DC difference always is.  Pad blocks count.
 *   DC refinement scan.  One raw bit per block in MCU order, (DC >> Al) & 1.  Pad blocks count.  No Huffman table.
 *   First AC scans.  The walk of the file above (points 2 and 3) over v = sign(c) (|c| >> Al); E and Z of the run rule are taken on v.
 *   AC refinement scans (T.81 G.1.2.3, what libjpeg's encode_mcu_AC_refine writes).  a[k] = |c[k]| >> Al.  A coefficient of the band
 *     is NEW if a = 1, OLD if a > 1, zero otherwise.  K is the last new k of the band; Z: the band has no new coefficient; E: a[Se] != 1.
 *     The block's string is HEAD, RUN SYMBOL (if the block starts a run), TAIL.
 *       Head: for k = Ss .. K, r counts zeros and B collects the bits a & 1 of old coefficients.  At every non-zero coefficient, while
 *         r > 15: code ZRL, then B; empty B; r -= 16.  An old coefficient then appends its bit to B.  A new coefficient codes symbol
 *         (r << 4) | 1, one sign bit (1 for positive), then B; it empties B and sets r = 0.
 *       Tail: the correction bits a & 1 of the old coefficients behind K -- of a Z block: of all its old coefficients.  No ZRL behind K.
 *       Runs: the rule above, unchanged, with this E and Z.  Block i starts a run iff E[i] and not (Z[i] and i mod 256 != 0 and
 *         E[i - 1]); the run covers the following Z blocks up to the next multiple of 256; the symbol is EOBn and n bits.
 *     Because the symbol stands between its starter's head and tail and a covered block's string is its tail alone, the scan is the
 *     concatenation of the blocks' strings in block order.
 * jpegamd_encode_color_progressive_successive_batch_async and jpegamd_encode_ycbcr_progressive_successive_batch_async take the
 * arguments, refusals, batching, context sizing, capacity behaviour (size 0, JPEGAMD_ERR_HUFF_CAPACITY, nothing written past
 * out_capacity, the other pictures unaffected) and statistics of the _progressive_optimized_ entries: bits and stuffed bytes summed
 * over the ten scans, exact_fallbacks counted once.  They neither read nor change the context's Huffman mode.
 * The bound, jpegamd_max_jfif_bytes_progressive_successive.  Bits per block, summed over the scans that touch it.  A Y block: its DC
 * difference at most 16 + 11 (scan 1); its refinement bit, 1 (scan 7); its 63 coefficients in the first scans 2 and 5 at most
 * 26 each (a non-zero one 16 + 10 -- the point transform only shortens amplitudes --, a ZRL 16 for sixteen zeros, either scan's run
 * symbol 16 + 8 paid by its own zero coefficient Se); in each of the refinement scans 6 and 10 a new coefficient 16 + 1, an old one 1,
 * sixteen zeros a ZRL of at most 16, and the run symbol 16 + 8 only where coefficient Se is not new and costs at most 1:
 * 62 x 17 + 25 = 1079.  Together 27 + 1 + 1638 + 2 x 1079 = 3824 bits; a chroma block has one refinement scan and costs less.  The
 * bound is the one-scan bound's form with 3824 for 1723 -- every block of every MCU, pad blocks too, every byte stuffed, one
 * rounding up to a byte, EOI, 640 bytes for the head with 432 bytes of DHT and a 14-byte SOS -- plus nine more roundings of at most
 * one byte each that may be stuffed (18), eight more SOS of 10 bytes and one of 14, and the DHT segments of ten tables, at most
 * 2 x 33 + 8 x 191 = 1594 bytes against the 432 held: 1162 more.  0 for bad arguments.
 * One block's string in any single scan is at most 1665 bits (a first scan: 27 or 63 x 26; a refinement scan: 1079; the DC
 * refinement scan: 1): the reservation of a coder segment (256 blocks of 1665 bits) holds every scan's segments.
 * jpegamd_debug_progressive_successive_counts (tests; synchronous, `counts` a HOST pointer): the symbol counts of the context's last
 * such call, [pictures of that call][10][256] in the file's table order.  JPEGAMD_ERR_ARG when the context's last call with per-scan
 * tables was not one of these (jpegamd_debug_progressive_counts answers the same way after one of these). */
int32_t jpegamd_encode_color_progressive_successive_batch_async(JpegAmdEncoder *enc, const JpegAmdImage *imgs, int32_t count, int32_t subsampling,
                                                                void *const *outs_dev, uint64_t out_capacity, uint64_t *const *out_sizes_dev,
                                                                void *stream);
int32_t jpegamd_encode_ycbcr_progressive_successive_batch_async(JpegAmdEncoder *enc, const JpegAmdYCbCrImage *imgs, int32_t count,
                                                                int32_t subsampling, int32_t sample_range, int32_t sample_format, int32_t matrix,
                                                                void *const *outs_dev, uint64_t out_capacity, void *const *out_sizes_dev,
                                                                void *stream);
/* (With metadata set on the context -- jpegamd_encoder_set_metadata -- a buffer needs jpegamd_encoder_metadata_bytes() more than this bound.) */
uint64_t jpegamd_max_jfif_bytes_progressive_successive(int32_t width, int32_t height, int32_t subsampling);
int32_t jpegamd_debug_progressive_successive_counts(JpegAmdEncoder *enc, uint64_t *counts);

/* ---- Progressive files with a scan script of the caller's, and grayscale progressive files ----------------------------------------
 * NORMATIVE.  A script is 1 .. JPEGAMD_MAX_SCANS scans in the file's order; a scan is a set of components (bit 0 Y, bit 1 Cb, bit 2
 * Cr; a grayscale file: bit 0 alone) and Ss, Se, Ah, Al.  jpegamd_validate_scan_script (host only, no device) accepts a script that
 * keeps every rule below (T.81 G.1.1.1, libjpeg's validate_script) and answers JPEGAMD_ERR_ARG otherwise; *bad_scan (may be NULL) is
 * then the index of the first scan that breaks a rule, -1 for a rule about the whole script (and -1 on success):
 *   - count is 1 .. JPEGAMD_MAX_SCANS, file_components 1 or 3 (whole script);
 *   - components is a non-empty subset of the file's components;
 *   - Ss = 0 implies Se = 0: a DC scan, of one, two or three components; Ss > 0: exactly one component and Ss <= Se <= 63;
 *   - Al <= 13; Ah = 0 or Ah = Al + 1;
 *   - for every (component, coefficient) the scan covers: Ah = 0 if no earlier scan coded it, otherwise Ah = the Al of the last that did
 *     and Ah = Al + 1 (so a first scan cannot be repeated, and a coefficient coded down to bit 0 is done);
 *   - an AC scan of a component comes after the component's first DC scan;
 *   - the script needs at most 16 Huffman tables (whole script): a first DC scan one per table class among its components (Y is a
 *     class, Cb and Cr share one), an AC scan one, a DC refinement scan none;
 *   - every component of the file has a first DC scan (whole script).  Nothing else has to be complete: a DC-only script is valid.
 * The file.  Head: SOI, APP0, DQT, SOF2 (a grayscale file: the one-component head, one quantisation table).  Every scan with symbols
 * has tables of its own, made of the scan's symbol counts as in the files above, numbered in the file's order and written as DHT
 * segments in front of the scan's SOS -- a first DC scan with Y and chroma: Y's, then the chroma table.  Tc/Th: 0x00 / 0x01 the DC
 * tables of Y / chroma, 0x10 / 0x11 the AC tables; a grayscale file uses 0x00 and 0x10.  SOS: Ns, the scan's components with
 * ascending selectors 1, 2, 3 -- Y with the tables 0 / 0, Cb and Cr 1 / 1 --, Ss, Se, Ah << 4 | Al: 8 + 2 Ns bytes.  The scans are
 * coded as in the file above (first and refinement scans, runs inside segments of 256 blocks); the scan shapes:
 *   three components, DC   the interleaved MCU of the one-scan file, pad blocks included;
 *   two components, DC     {Y, Cb}, {Y, Cr}, {Cb, Cr}: the MCU of T.81 A.2.3 -- Y's hs x vs blocks with the pad blocks of the
 *                          three-component scan, one block of each chroma component --, a component's predictor its previous block
 *                          in this scan's order, over the three-component MCU grid;
 *   one component, DC/AC   the component's own ceil(X / 8) x ceil(Y / 8) blocks in raster order (chroma: of its subsampled plane),
 *                          no pad blocks, the predictor the block in front.
 * scans == NULL with scan_count == 0 is libjpeg's jpeg_simple_progression for the file's component count: the ten scans above for a
 * colour file -- the file is the _successive_ entry's byte for byte --, and for a grayscale file the six scans
 *   DC 0,1; AC 1-5 0,2; AC 6-63 0,2; AC 1-63 2,1; DC 1,0; AC 1-63 1,0   (Ss-Se Ah,Al).
 * The entries take batches of up to 32 pictures with the arguments, grouping, capacity behaviour and statistics of the _successive_
 * entries; the gray entry any of the five channel orders, as jpegamd_encode_gray_scan_batch_async.  The script is validated before
 * anything is allocated or launched: a refused call (JPEGAMD_ERR_ARG) leaves the context as it was.  The context's Huffman mode is
 * neither read nor changed.  Not built: restart intervals, the planar (three-pointer) source, the Annex K tables with a script.
 * The bound, jpegamd_max_jfif_bytes_progressive_script (subsampling 0: grayscale), scan by scan: the scan's DHT segments at most (a
 * DC table 21 + 12 = 33 bytes, an AC table 21 + 170 = 191), its SOS, and its blocks -- every block of every MCU of an interleaved scan,
 * pad blocks too; a component's own blocks otherwise -- at the scan's worst bits per block, every byte stuffed, plus one rounding up
 * to a byte that may be stuffed.  Bits per block: a first DC scan 16 + 11 = 27; a DC refinement scan 1; a first AC scan of n
 * coefficients 26 n + 1 (a coefficient 16 + 10, a ZRL at most a bit per zero, the run symbol 16 + 8 paid by a zero coefficient Se
 * that costs nothing else -- 27 when n = 1); an AC refinement scan 17 (n - 1) + 25 (the derivation of 1079 above for n = 63).  The file
 * adds its head (bounded by the standard prefix: 640 bytes, grayscale 328) and EOI.  0 for an invalid script or bad dimensions.  One
 * block's string in any scan is at most 1665 bits: the reservation of a coder segment holds every scan's segments.
 * jpegamd_debug_progressive_script_counts (tests; synchronous, HOST pointer): the counts of the context's last script call,
 * [pictures][tables][256] with `tables` that script's table count; JPEGAMD_ERR_ARG after any other call (and the two entries above
 * answer JPEGAMD_ERR_ARG after a script call). */
#define JPEGAMD_MAX_SCANS 16
typedef struct JpegAmdScan {
    uint8_t components;                 /* bit 0 Y, bit 1 Cb, bit 2 Cr; a grayscale file: bit 0 alone */
    uint8_t ss, se, ah, al;
} JpegAmdScan;
int32_t jpegamd_validate_scan_script(const JpegAmdScan *scans, int32_t count, int32_t file_components, int32_t *bad_scan);
int32_t jpegamd_encode_color_progressive_script_batch_async(JpegAmdEncoder *enc, const JpegAmdImage *imgs, int32_t count, int32_t subsampling,
                                                            const JpegAmdScan *scans, int32_t scan_count, void *const *outs_dev,
                                                            uint64_t out_capacity, uint64_t *const *out_sizes_dev, void *stream);
int32_t jpegamd_encode_ycbcr_progressive_script_batch_async(JpegAmdEncoder *enc, const JpegAmdYCbCrImage *imgs, int32_t count,
                                                            int32_t subsampling, int32_t sample_range, int32_t sample_format, int32_t matrix,
                                                            const JpegAmdScan *scans, int32_t scan_count, void *const *outs_dev,
                                                            uint64_t out_capacity, void *const *out_sizes_dev, void *stream);
int32_t jpegamd_encode_gray_progressive_script_batch_async(JpegAmdEncoder *enc, const JpegAmdImage *imgs, int32_t count,
                                                           const JpegAmdScan *scans, int32_t scan_count, void *const *outs_dev,
                                                           uint64_t out_capacity, uint64_t *const *out_sizes_dev, void *stream);
/* (With metadata set on the context -- jpegamd_encoder_set_metadata -- a buffer needs jpegamd_encoder_metadata_bytes() more than this bound.) */
uint64_t jpegamd_max_jfif_bytes_progressive_script(int32_t width, int32_t height, int32_t subsampling, const JpegAmdScan *scans,
                                                   int32_t scan_count);
int32_t jpegamd_debug_progressive_script_counts(JpegAmdEncoder *enc, uint64_t *counts, int32_t tables);

/* Float pictures: float32, float16 or bfloat16 samples -- what a renderer, a generative model or an augmentation
 * pipeline leaves on the device -- encoded directly.  One kernel (k_float_planes_batch) in front of the tile encoder reads every sample
 * once, where it lies, makes its byte, applies the RGB -> YCbCr map and the chroma subsampling of this header to those bytes and
 * leaves 8-bit Y, Cb and Cr planes in context scratch, which are then coded as a BT.709 batch's planes are.  Every file is BYTE FOR
 * BYTE the file the uint8 entries write for the bytes of the samples.
 *
 * The byte of a stored sample x, for the call's `scale` and `offset`:
 *     x32 = x converted to float32            (exact for float16 and bfloat16, subnormals included)
 *     p   = x32 * scale                       rounded once to float32
 *     t   = p + offset                        rounded once to float32 (NOT fused with the multiply)
 *     v   = 0                                 if t is NaN
 *           min(max(rint(t), 0), 255)         otherwise; rint = round half to even; +inf -> 255, -inf -> 0
 * v is the byte: torch's x.float().mul(scale).add(offset).round().clamp(0, 255).to(uint8) with NaN -> 0.  Behind it, everything is
 * this header's definition for those bytes: Y = (77 R + 150 G + 29 B) >> 8; Cb and Cr per pixel by the two formulas above; 4:2:0 and
 * 4:2:2 samples by (a + b + c + d + 2) >> 2 and (a + b + 1) >> 1 with the last column / row replicated; the byte of a single-channel
 * picture is its Y sample.  scale and offset must be finite and |scale| <= 16777216: no float32 or bfloat16 subnormal can then
 * reach 0.5, so the result does not depend on the device's float32 denormal mode (float16 subnormals do count: at scale 65536 the
 * largest one maps to 4).  Samples in [0, 1]: (255, 0); in [-1, 1]: (127.5, 127.5), where 0 is a tie and gives 128; in [0, 255]: (1, 0).
 *
 * One description covers every tensor layout.  [3, H, W]: pixel_stride = the sample size.  [H, W, 3], and a channels-last
 * [N, 3, H, W]: the three pointers one sample apart, pixel_stride = 3 samples.  RGBA floats: 4 samples.  BGR: swap the pointers.
 * Crops and strided rows as they come.  plane[1] == plane[2] == NULL: ONE channel, the luma itself, for subsampling 0 alone.
 * Refused with JPEGAMD_ERR_ARG before the context is read: null arrays, elements or plane[0]; exactly one of plane[1] / plane[2]
 * null; a single channel with a colour subsampling; count outside 1 .. JPEGAMD_MAX_BATCH; an unknown sample_type or subsampling; a
 * non-finite scale or offset, |scale| above the bound; a pointer, row_stride or pixel_stride that is no multiple of the sample size;
 * pixel_stride below the sample size; row_stride < pixel_stride * width; pictures of different geometry.  Nothing outside a row's own
 * samples is read.
 *
 *   jpegamd_encode_float_batch_async                     three scans for JPEGAMD_SUBSAMPLE_444 / _420 / _422; subsampling 0: the fused
 *                                                        grayscale file (the luma of three planes, or the single channel)
 *   jpegamd_encode_float_interleaved_batch_async         one scan, restart_interval 0 .. 65535, the context's Huffman mode; subsampling
 *                                                        0 goes where jpegamd_encode_gray_scan_batch_async goes (the plain file is
 *                                                        the fused entry's)
 *   jpegamd_encode_float_progressive_script_batch_async  progressive files; scans NULL (scan_count 0): libjpeg's default script;
 *                                                        subsampling 0: the grayscale progressive file
 * Context sizing, capacity, status, statistics and every jpegamd_max_jfif_bytes* bound are those of the uint8 entry each call stands
 * for (jpegamd_encode_planar_batch_async, jpegamd_encode_planar_interleaved_batch_async / jpegamd_encode_gray_scan_batch_async,
 * jpegamd_encode_color_progressive_script_batch_async / jpegamd_encode_gray_progressive_script_batch_async); quantisation tables and
 * metadata set on the context apply.  With profiling on, ns_total opens at the front pass. */
#define JPEGAMD_FLOAT_F32  0
#define JPEGAMD_FLOAT_F16  1
#define JPEGAMD_FLOAT_BF16 2
typedef struct JpegAmdFloatImage {
    const void *plane[3];   /* DEVICE pointers to the first sample of R, G, B; plane[1] == plane[2] == NULL: one channel (luma) */
    int32_t width, height;  /* 1..65535 */
    int32_t row_stride;     /* bytes between rows, the same for the three planes */
    int32_t pixel_stride;   /* bytes between horizontally adjacent samples of a plane */
    int32_t quality;
} JpegAmdFloatImage;
int32_t jpegamd_encode_float_batch_async(JpegAmdEncoder *enc, const JpegAmdFloatImage *imgs, int32_t count, int32_t subsampling,
                                         int32_t sample_type, float scale, float offset, void *const *outs_dev, uint64_t out_capacity,
                                         void *const *out_sizes_dev, void *stream);
int32_t jpegamd_encode_float_interleaved_batch_async(JpegAmdEncoder *enc, const JpegAmdFloatImage *imgs, int32_t count, int32_t subsampling,
                                                     int32_t sample_type, float scale, float offset, int32_t restart_interval,
                                                     void *const *outs_dev, uint64_t out_capacity, void *const *out_sizes_dev, void *stream);
int32_t jpegamd_encode_float_progressive_script_batch_async(JpegAmdEncoder *enc, const JpegAmdFloatImage *imgs, int32_t count,
                                                            int32_t subsampling, int32_t sample_type, float scale, float offset,
                                                            const JpegAmdScan *scans, int32_t scan_count, void *const *outs_dev,
                                                            uint64_t out_capacity, void *const *out_sizes_dev, void *stream);

/* Reduced pictures: a file SMALLER than the picture it is made from -- a preview beside the full file, the 1/2, 1/4
 * and 1/8 steps of a pyramid, a contact sheet, a low-bandwidth stream -- with the box filter fused in front of the encoder.  One kernel
 * (k_reduce_planes_batch) reads every byte of the source once, where it lies, forms the box means, applies the RGB -> YCbCr map and the
 * chroma subsampling of this header to them and leaves 8-bit Y, Cb and Cr planes of the reduced picture in context scratch, which are
 * then coded as a float batch's planes are.
 *
 * The map, for a factor f in 1 .. JPEGAMD_MAX_REDUCE (the same both ways) and a source of W x H samples per channel:
 *     ow = ceil(W / f), oh = ceil(H / f)
 *     box(X, Y) = the source samples x in [f X, min(f X + f, W)), y in [f Y, min(f Y + f, H))
 *     n = the number of samples in the box   (1 .. f * f: only what lies inside the picture, nothing is replicated)
 *     S = their sum
 *     v(X, Y) = (S + (n >> 1)) / n            integer division rounding down; 0 .. 255
 * applied to R, G and B separately, or to the single channel.  v is a byte.  Behind it, everything is this header's definition for
 * those bytes: Y = (77 R + 150 G + 29 B) >> 8; Cb and Cr per REDUCED pixel by the two formulas above; 4:2:0 and 4:2:2 samples by
 * (a + b + c + d + 2) >> 2 and (a + b + 1) >> 1 with the last reduced column / row replicated; the byte of a single-channel picture
 * is its Y sample.  Every file is BYTE FOR BYTE the file the uint8 entries write for the ow x oh picture of those bytes stored as
 * packed RGB (or as JPEGAMD_ORDER_GRAY).  f = 1 is the identity map: a uint8 source at any row and pixel stride.  The mean is taken of
 * the STORED (gamma-encoded) bytes; averaging in linear light is out of scope.
 *
 * One description covers every tensor layout, as JpegAmdFloatImage does with one byte per sample.  [3, H, W]: pixel_stride = 1.
 * [H, W, 3], and a channels-last [N, 3, H, W]: the three pointers one byte apart, pixel_stride = 3.  RGBA: 4.  BGR: swap the pointers.
 * Crops and strided rows as they come; top-down only.  plane[1] == plane[2] == NULL: ONE channel, the luma itself, for subsampling 0
 * alone.  width and height are the SOURCE's (1 .. 65535 each, whatever the context was made for).  Refused with JPEGAMD_ERR_ARG before
 * the context is read: null arrays, elements or plane[0]; exactly one of plane[1] / plane[2] null; a single channel with a colour
 * subsampling; count outside 1 .. JPEGAMD_MAX_BATCH; factor outside 1 .. JPEGAMD_MAX_REDUCE; an unknown subsampling; pixel_stride
 * below 1; row_stride < pixel_stride * width (in 64 bits); pictures of different geometry; a bad restart interval or script.  Nothing
 * outside a row's own pixel_stride * width bytes is read.
 *
 *   jpegamd_reduced_size                                   (ow, oh) of a source and a factor; host only; JPEGAMD_ERR_ARG for a width or
 *                                                          height outside 1 .. 65535, a factor outside the range, a null result
 *   jpegamd_encode_reduced_batch_async                     three scans for JPEGAMD_SUBSAMPLE_444 / _420 / _422; subsampling 0: the fused
 *                                                          grayscale file (the luma of three planes, or the single channel)
 *   jpegamd_encode_reduced_interleaved_batch_async         one scan, restart_interval 0 .. 65535 in MCUs of the REDUCED picture, the
 *                                                          context's Huffman mode; subsampling 0: the gray scan
 *   jpegamd_encode_reduced_progressive_script_batch_async  progressive files; scans NULL (scan_count 0): libjpeg's default script;
 *                                                          subsampling 0: the grayscale progressive file
 * Context sizing, capacity, status, statistics and profiling are the float entries' rules at the REDUCED geometry: the context holds
 * count x the reduced picture's block rows, and buffers are sized with the jpegamd_max_jfif_bytes* functions at (ow, oh).  Quantisation
 * tables and metadata set on the context apply. */
#define JPEGAMD_MAX_REDUCE 8
typedef struct JpegAmdStridedImage {
    const void *plane[3];   /* DEVICE pointers to the first byte of R, G, B; plane[1] == plane[2] == NULL: one channel (luma) */
    int32_t width, height;  /* of the SOURCE, 1..65535 */
    int32_t row_stride;     /* bytes between rows, the same for the three planes */
    int32_t pixel_stride;   /* bytes between horizontally adjacent samples of a plane */
    int32_t quality;
} JpegAmdStridedImage;
int32_t jpegamd_reduced_size(int32_t width, int32_t height, int32_t factor, int32_t *out_width, int32_t *out_height);
int32_t jpegamd_encode_reduced_batch_async(JpegAmdEncoder *enc, const JpegAmdStridedImage *imgs, int32_t count, int32_t subsampling,
                                           int32_t factor, void *const *outs_dev, uint64_t out_capacity, void *const *out_sizes_dev,
                                           void *stream);
int32_t jpegamd_encode_reduced_interleaved_batch_async(JpegAmdEncoder *enc, const JpegAmdStridedImage *imgs, int32_t count,
                                                       int32_t subsampling, int32_t factor, int32_t restart_interval, void *const *outs_dev,
                                                       uint64_t out_capacity, void *const *out_sizes_dev, void *stream);
int32_t jpegamd_encode_reduced_progressive_script_batch_async(JpegAmdEncoder *enc, const JpegAmdStridedImage *imgs, int32_t count,
                                                              int32_t subsampling, int32_t factor, const JpegAmdScan *scans,
                                                              int32_t scan_count, void *const *outs_dev, uint64_t out_capacity,
                                                              void *const *out_sizes_dev, void *stream);

/* Resized pictures: a file of ANY smaller size -- "320 wide", "fit inside 1024 x 1024", 1920 x 1080 from a
 * 4096 x 2304 frame, a contact-sheet cell -- with exact area resampling fused in front of the encoder.  One kernel
 * (k_resize_planes_batch) reads the source where it lies, weights every source sample by the exact share of it that lies inside a
 * target sample's footprint, applies the RGB -> YCbCr map and the chroma subsampling of this header to the rounded means and leaves
 * 8-bit Y, Cb and Cr planes of the target in context scratch, which are then coded as a float batch's planes are.
 *
 * The map, for a source of W x H samples per channel and a target of ow x oh:
 *     1 <= ow <= W <= R ow  and  1 <= oh <= H <= R oh,  R = JPEGAMD_MAX_RESIZE_RATIO     (no enlargement; one target sample's
 *                                                                                          footprint is at most 65 x 65 samples)
 *     wx(X, x) = max(0, min((X + 1) W, (x + 1) ow) - max(X W, x ow))        sum over x: W
 *     wy(Y, y) = max(0, min((Y + 1) H, (y + 1) oh) - max(Y H, y oh))        sum over y: H
 *     S(X, Y)  = sum over y of wy(Y, y) * sum over x of wx(X, x) * s(x, y)  <= 255 W H < 2^40
 *     D        = W H                                                        < 2^32
 *     v(X, Y)  = (S + (D >> 1)) / D            integer division rounding down; 0 .. 255
 * applied to R, G and B separately, or to the single channel.  This is the area mean: every source sample weighted by the exact share
 * of it inside the footprint [X W / ow, (X + 1) W / ow) x [Y H / oh, (Y + 1) H / oh), rounded half up: v = floor(mean + 1/2).
 * ow = W, oh = H is the identity.  Where W = fx ow and H = fy oh the weights are constant and v is the plain box mean; for
 * fx = fy = f it is sample for sample the reduced map above (whose partial edge boxes, where W is no multiple of f, are its own
 * definition and not this one).  A target sample touches at most ceil(W / ow) + 1 source columns and ceil(H / oh) + 1 rows.  v is a
 * byte.  Behind it, everything is this header's definition for those bytes: Y = (77 R + 150 G + 29 B) >> 8; Cb and Cr per RESIZED
 * pixel by the two formulas above; 4:2:0 and 4:2:2 samples by (a + b + c + d + 2) >> 2 and (a + b + 1) >> 1 with the last resized
 * column / row replicated; the byte of a single-channel picture is its Y sample.  Every file is BYTE FOR BYTE the file the uint8
 * entries write for the ow x oh picture of those bytes stored as packed RGB (or as JPEGAMD_ORDER_GRAY).  The mean is taken of the
 * STORED (gamma-encoded) bytes; averaging in linear light is out of scope.
 *
 * JpegAmdStridedImage describes the source as it does for the reduced entries; width and height are the SOURCE's (1 .. 65535 each,
 * whatever the context was made for).  Refused with JPEGAMD_ERR_ARG before the context is read: everything the reduced entries
 * refuse, with jpegamd_resize_check on (width, height, out_width, out_height) in place of the factor's range.  Nothing outside a row's
 * own pixel_stride * width bytes is read.
 *
 *   jpegamd_resize_check                                   JPEGAMD_OK where the constraints above hold for a source of 1 .. 65535
 *                                                          each way, JPEGAMD_ERR_ARG otherwise; host only
 *   jpegamd_encode_resized_batch_async                     three scans for JPEGAMD_SUBSAMPLE_444 / _420 / _422; subsampling 0: the fused
 *                                                          grayscale file (the luma of three planes, or the single channel)
 *   jpegamd_encode_resized_interleaved_batch_async         one scan, restart_interval 0 .. 65535 in MCUs of the RESIZED picture, the
 *                                                          context's Huffman mode; subsampling 0: the gray scan
 *   jpegamd_encode_resized_progressive_script_batch_async  progressive files; scans NULL (scan_count 0): libjpeg's default script;
 *                                                          subsampling 0: the grayscale progressive file
 * Context sizing, capacity, status, statistics and profiling are the float entries' rules at the TARGET geometry: the context holds
 * count x the resized picture's block rows, and buffers are sized with the jpegamd_max_jfif_bytes* functions at (ow, oh).  Quantisation
 * tables and metadata set on the context apply. */
#define JPEGAMD_MAX_RESIZE_RATIO 64
int32_t jpegamd_resize_check(int32_t width, int32_t height, int32_t out_width, int32_t out_height);
int32_t jpegamd_encode_resized_batch_async(JpegAmdEncoder *enc, const JpegAmdStridedImage *imgs, int32_t count, int32_t subsampling,
                                           int32_t out_width, int32_t out_height, void *const *outs_dev, uint64_t out_capacity,
                                           void *const *out_sizes_dev, void *stream);
int32_t jpegamd_encode_resized_interleaved_batch_async(JpegAmdEncoder *enc, const JpegAmdStridedImage *imgs, int32_t count,
                                                       int32_t subsampling, int32_t out_width, int32_t out_height,
                                                       int32_t restart_interval, void *const *outs_dev, uint64_t out_capacity,
                                                       void *const *out_sizes_dev, void *stream);
int32_t jpegamd_encode_resized_progressive_script_batch_async(JpegAmdEncoder *enc, const JpegAmdStridedImage *imgs, int32_t count,
                                                              int32_t subsampling, int32_t out_width, int32_t out_height,
                                                              const JpegAmdScan *scans, int32_t scan_count, void *const *outs_dev,
                                                              uint64_t out_capacity, void *const *out_sizes_dev, void *stream);

/* Block until the last enqueued encode on this context finished; optionally fetch stats
 * (stats may be NULL).  Returns JPEGAMD_ERR_HUFF_CAPACITY if the output did not fit. */
int32_t jpegamd_encoder_finish(JpegAmdEncoder *enc, JpegAmdStats *stats);

/* Per-phase hipEvent timing.  slots = 0 turns it off (default).  slots = n keeps a ring of n
 * event sets: encode call i records into slot i % n on ITS stream, so a caller can enqueue
 * many encodes, synchronise once, and read every call's kernel times with
 * jpegamd_encoder_profile (only the *_ns fields are filled). */
int32_t jpegamd_encoder_set_profiling(JpegAmdEncoder *enc, int32_t slots);
int32_t jpegamd_encoder_profile(JpegAmdEncoder *enc, int32_t slot, JpegAmdStats *stats);

/* Stage taps for parity tests and the DTO's debug pointers.  Runs the same device code as
 * the hot path over the whole image and writes, for every 8x8 block in raster block order,
 * into DEVICE buffers (any of them may be NULL):
 *   y_centered   int8  [NB][64]  luma - 128, row-major inside the block  (converter.c:51,84-86)
 *   quant_zigzag int16 [NB][64]  quantised coefficients in zigzag order  (quantization.c:34-36, zigzag.c:51-61)
 *   exact_mask   u64   [NB]      bit k set = zigzag-raster coefficient k took the exact path
 * Synchronous. */
int32_t jpegamd_debug_stages(JpegAmdEncoder *enc, const JpegAmdImage *img, int8_t *y_centered,
                             int16_t *quant_zigzag, uint64_t *exact_mask);

/* Exact-order DCT of arbitrary centred blocks on the device (dct.c:63-96), for the float
 * parity test: in int8 [n][64] (row-major), out float [n][64] (out[u*8+v]).  DEVICE ptrs. */
int32_t jpegamd_debug_dct_exact(JpegAmdEncoder *enc, const int8_t *blocks, float *coeffs, int64_t nblocks);

/* Deterministic integer-only synthetic BMP generator (host code, no device needed); the
 * same generator feeds tests, goldens and bench.py on every machine.
 *   kind: 0 photo-like (smooth + textured regions), 1 uniform noise, 2 flat grey (seed&255),
 *         3 horizontal+vertical gradient
 *   flags bit0: top-down (negative biHeight); bit1: 138-byte offset to pixel data (V5-style)
 * Returns the BMP file size, or 0 if cap is too small (call with out=NULL to query). */
uint64_t jpegamd_synth_bmp(int32_t width, int32_t height, uint32_t seed, int32_t kind,
                           uint32_t flags, uint8_t *out, uint64_t cap);

/* Host-only introspection for tests.  The quantisation table for `quality` (raster order; 50 = the reference's,
 * natural_c/src/core/jpeg_tables.c:3-12; other values = its libjpeg scaling, an extension). */
int32_t jpegamd_debug_quant_table(int32_t quality, uint8_t *table);

/* Constants of the fast quantiser: qmul, qthr, bias float[64] by ZIGZAG position; the rigorous guard band delta, double[64], by raster k. */
int32_t jpegamd_debug_mfma_consts(int32_t quality, float *qmul, float *qthr, float *bias, double *delta);
/* The same for the colour files' chroma table: the table (raster order) and its constants (every output pointer may be NULL;
 * zoff / qadd as in jpegamd_debug_mfma_offsets). */
int32_t jpegamd_debug_chroma_quant_table(int32_t quality, uint8_t *table);
int32_t jpegamd_debug_chroma_mfma_consts(int32_t quality, float *qmul, float *qthr, float *bias, double *delta, float *zoff,
                                         float *qadd);
/* Per-kernel durations of a PROFILED colour encode in ring slot `slot` (jpegamd_encoder_set_profiling), ns[11]: k_chroma_planes,
 * then for Y, Cb, Cr the transform / merge / finalize kernels (k_stitch: in the finalize entry, merge 0), then k_append_scans. */
int32_t jpegamd_debug_color_profile(JpegAmdEncoder *enc, int32_t slot, uint64_t *ns);
/* Zero thresholds of the coefficient groups ([group 0..3][lane half 0..1], group G of half h = zigzag 16G+8h .. +7): a tile
 * whose hi-chain LUT sums all stay below grp_thr skips that group's quantiser entirely; lo_bound (may be NULL) is the largest
 * magnitude the lo chain can add to a site of the group -- grp_thr has it taken off. */
int32_t jpegamd_debug_group_thresholds(int32_t quality, float *grp_thr, float *lo_bound);
/* The same for the colour files' chroma table (as jpegamd_debug_chroma_mfma_consts is to jpegamd_debug_mfma_consts). */
int32_t jpegamd_debug_chroma_group_thresholds(int32_t quality, float *grp_thr, float *lo_bound);
/* Host-only, for tests: the fast quantiser's constants for an arbitrary table (raster order, entries 1..255; what
 * jpegamd_debug_mfma_consts, _mfma_offsets and _group_thresholds give for a quality).  Any output pointer may be NULL. */
int32_t jpegamd_debug_table_consts(const uint8_t *table, float *qmul, float *qthr, float *bias, double *delta,
                                   float *zoff, float *qadd, float *grp_thr, float *lo_bound);
/* ... and what the uncentred matrix operand (luma 0 .. 255 as binary16 subnormals) adds: zoff[64] / qadd[64] = bias + zoff by zigzag
 * position, the DC row's surplus in accumulator units, the accumulator scale.  Any pointer may be NULL. */
int32_t jpegamd_debug_mfma_offsets(int32_t quality, float *zoff, float *qadd, float *dc_off, float *scale);
/* The six-decimal cosine table the kernels multiply with, [x][u] (natural_c/src/core/dct.c:9-18), for host-side emulations. */
int32_t jpegamd_debug_cos_lut(float *lut);

const char *jpegamd_version(void);

/* ------------------------------------------------------------------------------------
 * Level 2: the reference's accelerator boundary
 * ---------------------------------------------------------------------------------- */

/* Same role and field order as dsp_port/jpeg_compression/include/jpeg_compression.h:32-64.
 * Differences forced by the hardware: the TI planar r / gb "physical" pointers become ONE
 * interleaved device pointer (r_phy_ptr) plus layout fields appended at the end; the
 * cycle counters count nanoseconds.  As in the reference the CALLER owns every buffer and
 * the callee fills rle_count, huff_size and the counters. */
typedef struct JPEG_COMPRESSION_DTO {
    int32_t width;
    int32_t height;

    uint64_t r_phy_ptr;       /* DEVICE address of the interleaved pixel rows */
    uint64_t gb_phy_ptr;      /* unused (kept for layout compatibility), must be 0 */

    /* First-block debug taps, HOST addresses, each may be 0
     * (dsp_port/jpeg_compression/src/jpeg_compression.c:150-169). */
    uint64_t y_phy_ptr;       /* int8  [64] */
    uint64_t dct_phy_ptr;     /* float [64] exact-order DCT of block 0 */
    uint64_t quant_phy_ptr;   /* int16 [64] raster order */
    uint64_t zigzag_phy_ptr;  /* int16 [64] zigzag order */

    uint64_t rle_phy_ptr;     /* unused: symbols never leave the chip; must be 0 */
    uint32_t rle_count;       /* OUT: number of run/size symbols coded */

    uint64_t huff_phy_ptr;    /* DEVICE address receiving the entropy-coded segment */
    uint32_t huff_size;       /* IN: capacity in bytes; OUT: bytes written */

    uint64_t cycles_color_conversion; /* OUT, ns: colour, DCT, quantisation and zigzag run fused in one  */
    uint64_t cycles_dct;              /*   kernel: cycles_dct carries its time, the other three are 0    */
    uint64_t cycles_quantization;
    uint64_t cycles_zigzag;
    uint64_t cycles_rle;              /* OUT, ns: symbol kernel (run/size + Huffman codes per segment)   */
    uint64_t cycles_huffman;          /* OUT, ns: offsets + stitch + stuffing kernels */
    uint64_t cycles_total;            /* OUT, ns */

    /* MI355X additions */
    int32_t row_stride;
    int32_t bottom_up;
    int32_t channel_order;
    int32_t quality;
} JPEG_COMPRESSION_DTO;

/* dsp_port/jpeg_compression/include/jpeg_compression.h:77 (registration of the remote
 * service becomes: pick the HIP device, load kernels, allocate the shared context).
 * Idempotent; returns 0 on success like the reference. */
int32_t JpegCompression_Init(void);
int32_t JpegCompression_DeInit(void);
/* Optional: pre-size the shared context (Init sizes it for 2048x2048, or JPEGAMD_INIT_DIM;
 * convertToJpeg / saveJPEGGrayscale grow it on demand). */
int32_t JpegCompression_Reserve(int32_t max_width, int32_t max_height);

/* dsp_port/jpeg_compression/include/jpeg_compression.h:111.  Synchronous.
 * Returns 0, or -6 / -8 with the reference's meaning, or a JPEGAMD_ERR_* code. */
int32_t convertToJpeg(JPEG_COMPRESSION_DTO *dto);

/* dsp_port/jpeg_compression/include/jpeg_compression.h:72-73 (handler signature). */
int32_t JpegCompression_RemoteServiceHandler(char *service_name, uint32_t cmd, void *prm,
                                             uint32_t prm_size, uint32_t flags);

/* ------------------------------------------------------------------------------------
 * Level 3: the natural_c library surface (same names and signatures, so
 * natural_c/src/main.c compiles and links against this library unchanged)
 * ---------------------------------------------------------------------------------- */

/* natural_c/include/bmp_handler.h:37-41 */
typedef struct BMPImage {
    int32_t width;
    int32_t height;
    uint8_t *data;   /* RGB, top-down, tightly packed; malloc'd */
} BMPImage;

/* natural_c/include/bmp_handler.h:43-45 (src/io/bmp_handler.c:5-129). Host code. */
BMPImage *loadBMPImage(const char *filename);
void freeBMPImage(BMPImage *image);

/* natural_c/include/jpeg_handler.h:107 (src/io/jpeg_handler.c:119-282): runs the whole
 * pipeline on the GPU and writes the file.  Opens the file first, prints the reference's
 * progress lines, returns false on any failure. */
bool saveJPEGGrayscale(const char *filename, const BMPImage *img);

/* In-memory variants used by tests and the CLI (no reference counterpart; they are what
 * loadBMPImage + saveJPEGGrayscale do without the file system).
 * jpegamd_encode_bmp_memory: BMP file bytes (host) -> JFIF file bytes (host).
 * Returns the JFIF size, or a negative JPEGAMD_ERR_* code. */
int64_t jpegamd_encode_bmp_memory(const uint8_t *bmp, uint64_t bmp_len, int32_t quality,
                                  uint8_t *out, uint64_t out_cap);
/* ... the colour file (jpegamd_encode_color_async) of the same BMP; subsampling JPEGAMD_SUBSAMPLE_444, _420 or _422. */
int64_t jpegamd_encode_bmp_memory_color(const uint8_t *bmp, uint64_t bmp_len, int32_t quality, int32_t subsampling,
                                        uint8_t *out, uint64_t out_cap);

/* ---- One image sharded over several GPUs by block rows (no reference counterpart) --------
 * Blocks are independent up to the entropy stage, which couples them only through the previous
 * block's DC (rle.c:59-70) and the running bit offset (huffman.c:35-62).  Each rank calls
 * jpegamd_encode_rows_async for its block rows [begin, end) of the SAME image description
 * (it needs the pixel rows of its range and of the one block row above); the unstuffed
 * per-segment bit strings stay in its context.  jpegamd_export_segments packs them densely:
 * `dense_words` (used 32-bit words of the range's segments, back to back), `meta`
 * (jpegamd_segment_meta_words() = 12 uint32 per segment: bits, word offset, first 8 / last 7 bits, symbols,
 * exact-path count, 0, 0, 0, and the counts of 0xFF bytes inside the segment for the 8 byte phases) and the word total.
 * After moving both buffers to the root (RCCL), jpegamd_import_segments places them at their
 * global segment indices in the root's context, and jpegamd_finalize_async stitches all
 * segments: bit offsets, 0xFF stuffing and the zero-padded flush happen once, there.
 * All four are stream-ordered; errors as jpegamd_encode_async. */
int32_t jpegamd_segment_meta_words(void);
int32_t jpegamd_encode_rows_async(JpegAmdEncoder *enc, const JpegAmdImage *img, int32_t block_row_begin,
                                  int32_t block_row_end, void *stream);
int32_t jpegamd_export_segments(JpegAmdEncoder *enc, const JpegAmdImage *img, int32_t block_row_begin,
                                int32_t block_row_end, uint32_t *dense_words_dev,
                                uint64_t dense_capacity_words, uint32_t *meta_dev,
                                uint32_t *total_words_dev, void *stream);
int32_t jpegamd_import_segments(JpegAmdEncoder *enc, const JpegAmdImage *img, int32_t block_row_begin,
                                int32_t block_row_end, const uint32_t *dense_words_dev,
                                const uint32_t *meta_dev, void *stream);
int32_t jpegamd_finalize_async(JpegAmdEncoder *enc, const JpegAmdImage *img, void *out_dev,
                               uint64_t out_capacity, uint64_t *out_size_dev, int32_t with_container,
                               void *stream);

/* ---- Independent images sharded over the GPUs of a node: the exchange step as a C entry (no reference counterpart: its
 * accelerator is one DSP core; the role is that of the host loop in dsp_port/jpeg_client/main.c:397-530) ------------------------
 * One process per GPU encodes its own images with jpegamd_encode_async / _batch_async, pointing image k's output at a staging
 * RECORD: `slot_bytes` long, the stream at offset 0 (capacity slot_bytes - 8), its byte count -- out_size_dev -- in the record's
 * last 8 bytes.  jpegamd_gather_streams then moves the `slots` records of every rank to `root` over RCCL as a gather-v: one
 * all-gather of the size tables, one host wait, one grouped launch of exact-size sends / receives (rounded up to 8 bytes) on
 * `stream`; synchronous.  `rccl_comm` is the caller's ncclComm_t (RCCL is dlopen'ed here, the library does not link it).
 *   sizes_host  HOST, [world][slots], filled on every rank.  A count above slot_bytes - 8 marks a stream the encoder had to
 *               cut: it does not travel; its owner encodes it again into a buffer of that size and sends it by itself.
 *   recv        DEVICE, root only: rank r's streams densely from recv + r * recv_stride on, in record order, each rounded up to
 *               8 bytes (the root's own included).  JPEGAMD_ERR_HUFF_CAPACITY when a rank's total exceeds recv_stride. */
int32_t jpegamd_gather_streams(void *rccl_comm, int32_t rank, int32_t world, int32_t root, const void *records_dev,
                               uint64_t slot_bytes, int32_t slots, uint64_t *sizes_host, void *recv_dev, uint64_t recv_stride,
                               void *stream);

/* File-to-file batch encoding with the host I/O and the PCIe transfers overlapped (no
 * reference counterpart: natural_c/src/main.c:21-24 handles one file, synchronously).
 * Files are processed in order with a few in flight: pinned staging buffers, one HIP stream
 * and one encoder context per slot; a file's read/upload overlaps the encode and the
 * download/write of its neighbours.  status[i] (optional) receives 0 or the JPEGAMD_ERR_*
 * code of file i; a failing file does not stop the batch.  Returns 0 when every file was
 * written, JPEGAMD_ERR_BMP when some failed, another code when nothing could run. */
typedef struct JpegAmdBatchStats {
    int32_t files_ok, files_failed;
    uint64_t bytes_in, bytes_out;       /* BMP file bytes read / JFIF bytes written (files_ok only) */
    double seconds_total;               /* wall time of the call */
    double seconds_read, seconds_write; /* host time spent inside fread / fwrite */
} JpegAmdBatchStats;
int32_t jpegamd_encode_files(const char *const *in_paths, const char *const *out_paths,
                             int32_t count, int32_t quality, int32_t *status,
                             JpegAmdBatchStats *stats);

/* Parse a BMP header the way loadBMPImage does (bmp_handler.c:22-88); fills a JpegAmdImage
 * whose `pixels` is an OFFSET into the file (cast to pointer), for callers that upload the
 * file themselves.  Returns 0 or JPEGAMD_ERR_BMP. */
int32_t jpegamd_parse_bmp(const uint8_t *bmp, uint64_t bmp_len, JpegAmdImage *view,
                          uint64_t *pixel_offset);

#ifdef __cplusplus
}
#endif
#endif /* JPEGAMD_JPEG_COMPRESSION_H */
