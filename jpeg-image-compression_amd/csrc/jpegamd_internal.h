// jpegamd_internal.h -- shared between the HIP kernels and the C-ABI host layer.
// Not installed; the public surface is include/jpeg_compression.h.
#pragma once

#include <stddef.h>
#include <stdint.h>

struct JpegAmdEncoder;
struct JpegAmdImage;

namespace jpegamd {

// ---- geometry of the device pipeline ---------------------------------------------------
// block   8x8 pixels
// tile    32 consecutive blocks of one block row: one wave-iteration of k_tile_encode, one 32-column MFMA operand, one bit string
// segment 8 consecutive tiles of one block row (<= 256 blocks): one wave of k_segment_merge, the unit of bitstream ownership
constexpr int kTileBlocks = 32;
#ifndef JPEGAMD_SEG_TILES
#define JPEGAMD_SEG_TILES 8
#endif
constexpr int kSegTiles = JPEGAMD_SEG_TILES;
constexpr int kSegBlocks = kTileBlocks * kSegTiles;                  // 256
// A launch that codes four or more pictures (jpegamd_encode_batch_async) has waves to spare and uses segments of 16 tiles:
// the per-segment costs of k_segment_merge and k_finalize -- both mostly per-segment bookkeeping -- are paid half as often.
// (A single picture keeps 8: with 16 its two small kernels have too few waves: measured +20 % each.)
constexpr int kSegTilesBatch = 16;
constexpr int kSegTilesMax = kSegTilesBatch;
// Worst case bits per block: DC 9+11, 63 x (16+11) AC (quality 100 -> 11-bit amplitudes).
constexpr int kMaxBlockBits = 20 + 63 * 27;                          // 1721
constexpr int seg_cap_words(int seg_tiles) { return ((kTileBlocks * seg_tiles * kMaxBlockBits + 31) / 32 + 1 + 63) / 64 * 64; }   // words reserved per segment
constexpr int kSegCapWords = seg_cap_words(kSegTiles);
// Colour scans (jpegamd_encode_color_async): a chroma DC code is up to 11 bits (T.81 K.4), so a chroma block's bound is
// 22 + 63 x 27 bits.  The reservations sized with kMaxBlockBits hold it as well (they round to the same word counts); the
// attainable worst case is lower still -- neither AC table has a code for size 11, so an AC symbol is at most 16 + 10 bits.
constexpr int kMaxBlockBitsColor = 22 + 63 * 27;                     // 1723
constexpr int seg_cap_words_at(int seg_tiles, int block_bits) { return ((kTileBlocks * seg_tiles * block_bits + 31) / 32 + 1 + 63) / 64 * 64; }
static_assert(seg_cap_words_at(kSegTiles, kMaxBlockBitsColor) == seg_cap_words(kSegTiles) &&
              seg_cap_words_at(kSegTilesBatch, kMaxBlockBitsColor) == seg_cap_words(kSegTilesBatch),
              "a segment of chroma blocks fits the luma reservation");
constexpr int kAFragWords = 2 * 2 * 4 * 64 * 4;                      // [term][chain][kstep][lane] x 8 binary16 = 16 KiB
constexpr float kMfmaScale = 1.0f / 8192.0f;                         // the accumulator chains hold kMfmaScale * LUT sum (hi chain + lo chain): the A terms are 2048 K, the B operand is y 2^-24

// Per-tile symbol lists (private to k_tile_encode: built in LDS, coded by the wave that built them, never written out).
// An item is one symbol-to-be, 4 bytes: bits 15..0 the value (int16), bits 21..16 the zigzag position (the producer writes
// the upper half with one SDWA add of an inline constant, and the coder's run is one 16-bit subtraction).  A block's run is: DC item, non-zero AC items, EOB item unless zigzag 63 is non-zero.  DC, EOB and padding
// items have position 0 ("class D": coded from row 0 of the code table, whatever precedes them); a non-zero AC item always
// has position >= 1.
// The padding item: size 12 -- a size the table has no code for -- with all-zero amplitude bits (value -4095: amplitude code
// -4096 = ...1 0000 0000 0000): it yields no bit.  It stands in for the DC of a tile's FIRST block, whose predictor is the last
// block of the tile before (rle.c:59-70): that one symbol is coded by k_segment_merge, which knows both.
constexpr uint32_t kItPadValue = 0xF001u;
// The EOB item (rle.c:121-123) in the same style: size 13, amplitude bits all zero (value -8191); row 0 of the code table
// holds the EOB code under "size 13".
constexpr uint32_t kItEobValue = 0xE001u;
constexpr int kStageWords = 8 * 132;            // a wave's LDS region: the tile's luma stash (8 rows of 132 words), then -- the stash dead -- its item list
constexpr int kStageItemCap = kStageWords - 128;   // items of one PART of a tile: the list is padded to whole passes of 128 items inside the region (928 >= 8 blocks x 65)

// Code table of k_tile_encode (LDS), built once on the host (quant_consts.cpp: build_code_table), independent of the quality.
// Entry (row r, fb) at word kCodeLead + 33 r + fb (odd row stride: symbols of one size and different runs sit in different LDS banks):
//   r   0: class D (fb selects the DC size, 12 = no code, 13 = EOB); r >= 1: AC symbol with run r - 1 (runs >= 16: the entry
//       is that of run & 15 and carries the number of ZRL symbols in front of it, rle.c:99-103)
//   fb  v_ffbh_i32 of twice the amplitude code: 31 - size, or -1 for a zero value (size 0)
//   entry: bits 31..16 the Huffman code LEFT-ALIGNED, 15..8 code length + size, 6..5 ZRLs, 4..0 code length
constexpr int kCodeLead = 32;
constexpr int kCodeRows = 64;
constexpr int kCodeRowStride = 33;
constexpr int kCodeWords = kCodeLead + kCodeRows * kCodeRowStride;   // 2144
constexpr uint32_t kZrlBits = 11, kZrlCode = 0x7F9u;                  // symbol 0xF0: '11111111001' (jpeg_tables.c:36-48)
constexpr uint32_t kZrlBitsChroma = 10, kZrlCodeChroma = 0x3FAu;      // ... in the chroma AC table (T.81 K.6): '1111111010'

// Per-tile output of k_tile_encode in HBM: an 8-word record and the tile's bit string (MSB-first): every symbol of the tile
// except the DC of its first block.
//   record: {bits of the string, DC of the first block (absolute), DC of the last block, exact-order fallbacks,
//            symbols (run/size symbols incl. ZRLs and the first DC), 0, 0, 0}
// The record and the first 120 words of the string -- all of it for photo-like content -- form the tile's HEAD, 512 bytes in a
// DENSE array (16 MB per 8192^2 picture: it stays in L2 / Infinity Cache between the two kernels); what lies beyond goes to a
// sparse array reserved for the worst case (only touched bytes cost anything).  Round 2 kept everything in worst-case strides
// of 8.7 KB per tile: every tile a DRAM row and a TLB entry of its own for ~100 useful bytes.
constexpr int kTileRecWords = 8;
constexpr int kTileHeadWords = 128;             // record + first string words: ONE 8-byte-per-lane store
constexpr int kTileHeadStr = kTileHeadWords - kTileRecWords;   // 120
constexpr int kTileOverCap = ((kTileBlocks * kMaxBlockBits + 31) / 32 + 2 + 63) / 64 * 64;   // words reserved per tile behind the head (1728)
static_assert(((kTileBlocks * kMaxBlockBitsColor + 31) / 32 + 2 + 63) / 64 * 64 == kTileOverCap, "a tile of chroma blocks fits the luma reservation");
// (A dense array for the segments' strings as well was measured: k_finalize 38 -> 51 us per launch of eight pictures.)

struct MfmaTables {
    uint32_t afrag[kAFragWords];   // 2048 x the LUT-product matrix as two integer-valued binary16 terms (lo 2^-11, hi), MFMA A-operand order (the B operand brings 2^-24)
    float qmul[64];                // by zigzag position z: M_z = K / (q * kMfmaScale)  (the MFMA output is kMfmaScale * LUT sum)
    float qthr[64];                // flag threshold 2 (bias_z - 0.5), exactly (the kernel derives it as fma(2, bias_z, -1))
    float qstep[64];               // (float) q, by zigzag position
    float bias[64];                // by zigzag position: 0.5 + delta_z (with margin) -- a band of delta_z on EITHER side of a rounding tie
    float grp_thr[8];              // [group G][lane half h]: |hi-chain output| below it in every site => zigzag 16G+8h .. +7 all quantise to an unflagged 0
                                   // (the lo chain's largest possible contribution, lo_bound, is taken off: the test runs ahead of the add that joins the chains)
    float lo_bound[8];             // [group G][lane half h]: max over the sites of |lo-chain output|, in accumulator units
    float flag_thr[8];             // [group G][lane half h]: max qthr over zigzag 16G+8h .. +7
    float zoff[64];                // by zigzag position: what the quantiser adds besides the bias -- minus (K/q) x the constant the UNCENTRED B operand leaves in the row (five positions; 0 elsewhere)
    float qadd[64];                // bias + zoff: the additive constant of the quantiser's fma, by zigzag position
    float dc_off;                  // what the DC row's accumulator holds beyond the centred pixel sum: kMfmaScale * 64 * 128 (= 1.0)
    float pad[3];
};

struct ScanStats {                   // device-side per-call record
    uint64_t total_bits;
    uint64_t total_syms;
    uint64_t total_exact;
    uint64_t total_ff;
    uint64_t out_size;               // copy of *out_size
    uint32_t status;                 // bit0 = output capacity overflow (sticky until jpegamd_encoder_finish reads it)
    uint32_t pad;
};

constexpr int kMaxBatch = 32;           // images of one geometry coded by ONE launch of each kernel (jpegamd_encode_batch_async)

// ---- what a launch of k_tile_encode reads -----------------------------------------------------------------------------------
// TileSource says it in three independent facts.  `layout` is the memory walk of the loader, the kernel's template parameter kSrc:
//   kSrcRgb     3 bytes per pixel, luma by the weights in ImageDesc::select (BGR / RGB, either row order)
//   kSrcPlane   1 byte per pixel: the sample itself (a GRAY picture, a Y plane, a chroma plane)
//   kSrcPx4     4 bytes per pixel (RGBA / BGRA): luma by the same weights, the fourth byte meets a zero weight
//   kSrcPlanar  the R, G and B planes of one byte per sample: R in ImageDesc::batch_pixels, G and B in TilePlanes
//   kSrcPair    a plane of byte pairs of which a launch image takes ONE component: a chroma scan of Cb Cr pairs (NV12), or -- with
//               the luma tables -- the Y scan of a packed 4:2:2 plane (Y Cb Y Cr / Cb Y Cr Y)
//   kSrcQuad    a plane of 4-byte groups of which a launch image takes ONE byte: the chroma scans of that packed plane
//   kSrcPlane16 a plane of 16-bit little-endian words holding 10-bit samples; kSrcPair16: a plane of pairs of such words, one
//               component per launch image.  Every sample is narrowed to 8 bits behind the loader.
// width, height and row_stride of the ImageDesc describe the component that is coded (width in samples, pairs or groups; row_stride
// in bytes).  `chroma`: the scan is coded with the chroma MfmaTables, the chroma code and Huffman tables and the chroma ZRL code.
// `expand`: the samples are limited range (JPEGAMD_RANGE_LIMITED) and are mapped to full range behind the loader, Y by the luma map
// and Cb / Cr by the chroma map; with a 16-bit layout it selects the limited-range narrowing.  launch_tile_transform has the list of
// combinations that exist as kernels (the stamped build: luma kSrcRgb / kSrcPlane and chroma kSrcPlane alone; stage taps: luma
// kSrcRgb / kSrcPlane, and -- the coefficient planes of an interleaved-MCU file -- every source a colour batch reads); any other is
// hipErrorInvalidValue.
constexpr int kSrcRgb = 0, kSrcPlane = 1, kSrcPx4 = 2, kSrcPlanar = 3, kSrcPair = 4, kSrcQuad = 5, kSrcPlane16 = 6, kSrcPair16 = 7;
struct TileSource {
    int layout = kSrcRgb;
    bool chroma = false, expand = false;
};

// ImageDesc::select is ONE word that tells the loader which of the stored bytes it wants.  Its three shapes, each with its packer
// here and its readers in jpegamd_device.h:
//   kSrcRgb, kSrcPx4        the luma weights of stored bytes 0, 1, 2 in bytes 0, 1, 2 (byte 3 = 0)       select_luma / luma_of
//   kSrcPair, kSrcQuad      bit 0: the parity p -- launch image i takes component (p + i) & 1 of a pair, so a chroma launch that
//                           starts on plane `first` of the call (Cb even, Cr odd) passes first & 1, flipped when Cr is stored first;
//                           the Y scan of a packed plane takes component p for EVERY image.  Bit 8: kSrcQuad's first byte f -- the
//                           byte taken is f + 2 ((p + i) & 1): 1 / 3 of Y Cb Y Cr, 0 / 2 of Cb Y Cr Y    select_byte / select_component, select_quad_byte
//   kSrcPlane16, kSrcPair16 bit 0: kSrcPair16's parity, as above; bits 16..20: the right shift that leaves the 10-bit value of a
//                           word (6: MSB-aligned, 0: LSB-aligned)                                          select_depth / select_component, select_shift
// kSrcPlane and kSrcPlanar do not read it.
constexpr uint32_t select_luma(bool blue_first) { return blue_first ? (29u | (150u << 8) | (77u << 16)) : (77u | (150u << 8) | (29u << 16)); }   // Y = (77 R + 150 G + 29 B) >> 8 (converter.c:51)
constexpr uint32_t select_byte(uint32_t parity, uint32_t first_byte) { return (parity & 1u) | ((first_byte & 1u) << 8); }
constexpr uint32_t select_depth(uint32_t parity, uint32_t shift) { return (parity & 1u) | ((shift & 31u) << 16); }

struct ImageDesc {
    const uint8_t *pixels;              // image 0 (== batch_pixels[0])
    const uint8_t *batch_pixels[kMaxBatch];
    int32_t batch;                      // images in this launch; tiles / segments of image i are [i * num_tiles, ..) / [i * num_segs, ..)
    uint32_t tpi_magic;                 // min(floor(2^32 / num_tiles), 2^32 - 1): global tile / num_tiles by multiply-high, at most one too small
    int32_t width, height, row_stride, bottom_up;
    uint32_t select;                    // which stored bytes the loader takes (above)
    int32_t blocks_w, blocks_h, segs_per_row, num_segs;
    int32_t seg_tiles;                  // tiles per segment of this launch: kSegTiles, or kSegTilesBatch
    int32_t tiles_per_row, num_tiles;
    int32_t tile_begin, tile_end;       // tiles this launch transforms (whole images: 0, batch * num_tiles; a block-row shard otherwise)
    int32_t seg_begin, seg_end;         // segments this launch codes (whole images: 0, batch * num_segs)
    int32_t fast_ok;           // pixels % 4 == 0 && row_stride % 4 == 0 (planar: every plane)
};
// (a kernel argument: the committed profiles and tools know its layout)
static_assert(sizeof(ImageDesc) == 8 * (1 + kMaxBatch) + 4 * 20 && offsetof(ImageDesc, select) == 8 * (1 + kMaxBatch) + 24 &&
              offsetof(ImageDesc, fast_ok) == 8 * (1 + kMaxBatch) + 72, "ImageDesc keeps its size and member offsets");

// What k_segment_merge leaves per segment (and what one image sharded over GPUs exchanges, besides the bit strings).
struct SegArrays {
    uint32_t *words;            // [num_segs][words_stride] MSB-first bit string, unstuffed
    uint32_t words_stride;      // seg_cap_words(tiles per segment of the launch)
    uint32_t *bits;             // [num_segs] bit count
    uint32_t *syms;             // [num_segs] run/size symbols coded (DTO rle_count)
    uint32_t *exact;            // [num_segs] coefficients recomputed in exact order
    uint32_t *edge;             // [num_segs] (first 8 bits << 8) | last 7 bits: what the byte straddling two segments is made of
    uint16_t *ffin;             // [num_segs][8] 0xFF bytes lying wholly inside the segment when its first bit sits at byte phase p
    // Per GROUP of kSegGroup consecutive segments (one workgroup of k_segment_merge), so that k_finalize's scan over everything in
    // front of a chunk reads a quarter of the entries: the group's bits, and the 0xFF bytes its segments own when the group's
    // first bit sits at byte phase p -- without the byte straddling the group's start (that needs the segment in front).
    uint32_t *grp_bits;         // [ceil(num_segs / kSegGroup)]
    uint32_t *grp_ff;           // [ceil(num_segs / kSegGroup)][8] (32-bit: sixteen worst-case segments hold more than 65535 bytes)
};
constexpr int kSegGroup = 4;      // (16 -- one k_finalize chunk -- was measured: k_segment_merge's 1024-thread workgroups cost it 60 %)

struct TransformOutM {
    const MfmaTables *tables;   // device copy
    uint32_t *tile_head;        // [num_tiles][kTileHeadWords]: record + first string words of every tile
    uint32_t *tile_over;        // [num_tiles][kTileOverCap]: string words from kTileHeadStr on (index w - kTileHeadStr)
    const uint32_t *code_tab;   // [kCodeWords] device copy of the code table
    uint32_t *tile_ctr;         // [64 groups][32 words]: word 0 = ticket counter of the group's tile hand-out; zero at launch
    uint32_t *tile_ctr_next;    // the set the NEXT launch on this context uses: zeroed by this launch
    unsigned long long *stamps; // per-wave phase cycle sums (launch_tile_transform_stamped only)
    int8_t *tap_y;              // stage taps (debug variant only)
    int16_t *tap_zz;
    uint64_t *tap_mask;
};
// `ev` (optional): two hipEvent_t that receive the kernel's OWN begin / end timestamps (hipExtLaunchKernelGGL), i.e. what a
// kernel trace reports as its duration -- an event recorded in front of a launch also sees the dispatch latency.
// `src`: what the launch reads (TileSource, above); a chroma source wants the chroma constants in TransformOutM.
struct TilePlanes {                     // the second and third plane of every picture of a planar launch (its own kernel argument)
    const uint8_t *g[kMaxBatch];
    const uint8_t *b[kMaxBatch];
};
int launch_tile_transform(const ImageDesc &im, const TransformOutM &out, bool taps, void *stream, void *const *ev = nullptr, TileSource src = {},
                          const TilePlanes *planes = nullptr);
// whether launch_tile_transform has a kernel for (taps, src): a lookup in its list, no device needed
bool tile_variant_exists(bool taps, TileSource src);
// the same kernel with its phases stamped (out.stamps must point at 16 words per wave): jpegamd_tile_pipeline.hip, -DJPEGAMD_STAMPED_TU
int launch_tile_transform_stamped(const ImageDesc &im, const TransformOutM &out, bool taps, void *stream, void *const *ev = nullptr, TileSource src = {},
                                  const TilePlanes *planes = nullptr);

struct MergeArgs {              // k_segment_merge: the tile strings of a segment -> ONE bit string per segment + its numbers
    const uint32_t *tile_head, *tile_over;
    const uint32_t *huff;           // [272] (len << 16) | code: AC by run/size symbol, then 16 DC sizes
    int32_t num_segs, segs_per_row, tiles_per_row;     // per image
    int32_t seg_tiles;              // tiles per segment: kSegTiles or kSegTilesBatch
    int32_t seg_begin, seg_end;     // segments this launch codes (whole images: 0, batch * num_segs)
    int32_t tiles_per_image;        // a batch: segment s belongs to image s / num_segs, whose tiles start at image * tiles_per_image
    SegArrays seg;
    uint32_t *status;               // ScanStats::status: bit 1 = a tile record did not fit its reservation (JPEGAMD_ERR_RLE_CAPACITY)
};
int launch_segment_merge(const MergeArgs &a, void *stream, void *const *ev = nullptr);

// Post-processing (jpegamd_finalize.hip): global bit / stuffing offsets, stitch, stuffing, container -- ONE launch.
struct FinalizeArgs {
    SegArrays seg;
    int32_t num_segs;               // per image
    int32_t num_chunks;             // per image: workgroups = batch * ceil(num_segs / 16)
    int32_t batch;
    int32_t use_groups;             // the group aggregates are valid for these segments (whole images merged by k_segment_merge, num_segs % kSegGroup == 0)
    uint8_t *out[kMaxBatch];
    uint64_t out_capacity;          // of every output
    uint64_t *out_size[kMaxBatch];  // device
    ScanStats *stats;               // device
    const uint8_t *prefix;
    int32_t prefix_len;
    int32_t write_eoi;
};
int launch_finalize(const FinalizeArgs &a, void *stream, void *const *ev = nullptr);
int finalize_chunks(int num_segs);

// k_stitch (jpegamd_stitch.hip): whole images -- the tiles' strings -> the finished entropy-coded segment in ONE pass (what
// k_segment_merge + k_finalize do in two for the block-row shards of one image over several GPUs).
// Workgroups hand their numbers on in 16-byte granules tagged with the launch's 14-bit epoch (layout: jpegamd_stitch.hip); the
// array is zeroed when the context is created and whenever the epoch wraps, so a granule of an older launch never matches.
struct StitchArgs {
    const uint32_t *tile_head, *tile_over;
    const uint32_t *huff;           // [272] (len << 16) | code: AC by run/size symbol, then 16 DC sizes
    int32_t num_segs, segs_per_row, tiles_per_row;     // per image
    int32_t seg_tiles;              // tiles per segment: kSegTiles or kSegTilesBatch
    int32_t tiles_per_image;
    int32_t batch, wgs_per_image;   // grid = batch * wgs_per_image
    uint32_t epoch;                 // 1 .. 16383
    uint32_t *desc;                 // [batch * wgs_per_image][4] granules
    uint32_t *desc_ffx;             // [batch * wgs_per_image][8] a workgroup's 0xFF counts by byte phase in full (read when a granule's 8-bit counts saturated)
    uint32_t *seg_syms, *seg_exact; // [batch * num_segs] per-segment counters (summed on request)
    uint8_t *out[kMaxBatch];
    uint64_t out_capacity;          // of every output
    uint64_t *out_size[kMaxBatch];  // device
    ScanStats *stats;               // device
    uint32_t *status;               // &stats->status: bit 0 output capacity, bit 1 corrupt tile record, bit 2 a look-back gave up
    const uint8_t *prefix;
    int32_t prefix_len;
    int32_t write_eoi;
};
int launch_stitch(const StitchArgs &a, void *stream, void *const *ev = nullptr);
int stitch_workgroups(int num_segs);

// Segment exchange for one image sharded over GPUs by block rows (jpegamd_finalize.hip): dense copy of the used words of
// segments [s0, s1) + kSegMetaWords words of metadata per segment, and back.
constexpr int kSegMetaWords = 12;   // {bits, word offset, edge, symbols, exact-path count, 0, 0, 0, ffin[0..7] as 4 words}
struct SegExchange {
    SegArrays seg;
    int32_t s0, s1;
    uint32_t *dense; uint64_t dense_cap_words;
    uint32_t *meta;                 // [s1 - s0][kSegMetaWords]
    uint32_t *total_words;          // [1] (export: written; import: unused)
    uint32_t *status;               // ScanStats::status word: bit 0 set when dense_cap_words was too small
};
int launch_seg_export(const SegExchange &x, void *stream);
int launch_seg_import(const SegExchange &x, void *stream);
int launch_sum_stats(const uint32_t *seg_syms, const uint32_t *seg_exact, int n, ScanStats *stats, void *stream);
int launch_dct_exact(const int8_t *blocks, float *coeffs, int64_t nblocks, void *stream);

// Colour (jpegamd_color.hip).  k_chroma_planes: the picture -> Cb and Cr planes (u8, `pitch` bytes per row, a multiple of 4), full
// resolution (4:4:4), 2 x 2 averaged (4:2:0) or 2 x 1 averaged (4:2:2: cw x ch = ceil(w / 2) x h).  k_append_scans: the chroma scans, coded into context scratch, copied behind the
// Y scan in the caller's buffer at the offsets the device computed; the per-scan statistics summed into one record.
constexpr int kChromaMode444 = 0, kChromaMode420 = 1, kChromaMode422 = 2;
struct ChromaPlanesArgs {
    const uint8_t *pixels;
    int32_t width, height, row_stride, bottom_up;
    int32_t rgb;                        // 1: stored bytes R, G, B; 0: B, G, R
    int32_t mode;                       // kChromaMode*
    int32_t cw, ch, pitch;              // plane geometry
    uint8_t *cb, *cr;
};
int launch_chroma_planes(const ChromaPlanesArgs &a, void *stream, void *const *ev = nullptr);
struct AppendArgs {
    uint8_t *out;
    uint64_t out_capacity;
    uint64_t *out_size;                 // the caller's: the file's size, or 0 when it did not fit
    const uint64_t *scan_size;          // [3] bytes of the Y part (prefix + Y scan) and of the two chroma parts (SOS + scan [+ EOI])
    const uint8_t *src[2];              // the chroma parts (context scratch)
    ScanStats *scan_stats;              // [3] per-scan records (status, bits, 0xFF bytes, symbols, exact-path count)
    ScanStats *stats;                   // the context's record: the sums
};
int launch_append_scans(const AppendArgs &a, void *stream, void *const *ev = nullptr);

// Colour batches (jpegamd_encode_color_batch_async): `batch` pictures of one geometry, ONE launch of each kernel where the context
// allows.  k_chroma_planes_batch writes 2 x batch planes, plane j = picture j / 2, Cb (j even) or Cr (j odd), `plane_bytes` apart.
constexpr int kChromaSrcPx3 = 0, kChromaSrcPx4 = 1, kChromaSrcPlanar = 2;   // 3 / 4 bytes per pixel, or the R, G and B planes
struct ChromaPlanesBatchArgs {
    const uint8_t *pixels[kMaxBatch];   // (planar: the R planes)
    int32_t batch;
    int32_t width, height, row_stride, bottom_up;
    int32_t rgb, mode;                  // mode: kChromaMode*
    int32_t cw, ch, pitch;
    uint64_t plane_bytes;               // a multiple of 16
    uint8_t *planes;
    int32_t layout;                     // kChromaSrc*
    const uint8_t *pixels_g[kMaxBatch], *pixels_b[kMaxBatch];   // kChromaSrcPlanar alone
};
int launch_chroma_planes_batch(const ChromaPlanesBatchArgs &a, void *stream, void *const *ev = nullptr);

// BT.709 YCbCr pictures (jpegamd_encode_ycbcr_matrix_batch_async, jpegamd_matrix.hip).  k_ycbcr_matrix_batch reads every picture of
// the batch once, in whatever layout, depth and range it has, and writes 8-bit full-range BT.601 planes into context scratch: the
// chroma planes where k_chroma_planes_batch puts them (plane j = picture j / 2, Cb or Cr, `plane_bytes` apart, `pitch` bytes per row),
// the Y planes `yplane_bytes` apart at `ypitch` bytes per row (the width rounded up to 4).  With cb = Cb - 128, cr = Cr - 128 of the
// 8-bit full-range samples (after the range and depth maps) and >> an arithmetic shift:
//     Y'  = clamp(Y   + ((c[0] cb + c[1] cr + 8192) >> 14), 0, 255)
//     Cb' = clamp(128 + ((c[2] cb + c[3] cr + 8192) >> 14), 0, 255)
//     Cr' = clamp(128 + ((c[4] cb + c[5] cr + 8192) >> 14), 0, 255)
// c = round(2^14 x) of BT.709 YCbCr -> R'G'B' (Kr 0.2126, Kb 0.0722) followed by R'G'B' -> BT.601 YCbCr (Kr 0.299, Kb 0.114).
constexpr int kMatrixShift = 14;
constexpr int32_t kMatrix709[6] = {1664, 3213, 16218, -1813, -1187, 16112};
constexpr int32_t kMatrix601[6] = {0, 0, 1 << kMatrixShift, 0, 0, 1 << kMatrixShift};     // the identity: what BT.601 input asks for
constexpr int kMatrixWalkPlanes = 0, kMatrixWalkPairs = 1, kMatrixWalkPacked = 2;        // Y, Cb, Cr planes / Y and a pair plane / one packed 4:2:2 plane
struct YccMatrixBatchArgs {
    const uint8_t *y[kMaxBatch];        // the Y planes (packed: the packed planes)
    const uint8_t *cb[kMaxBatch];       // the Cb planes, or the pair planes (packed: not read)
    const uint8_t *cr[kMaxBatch];       // kMatrixWalkPlanes alone
    int32_t batch;
    int32_t width, height, y_stride, c_stride;     // strides in bytes
    int32_t mode, walk, sample_bytes;   // kChromaMode*, kMatrixWalk*, 1 or 2
    int32_t first;                      // pairs: the index of Cb in a pair (0 / 1); packed: of Y in a pixel's two bytes (0 YUYV, 1 UYVY)
    int32_t shift, limited;             // 16-bit words: 6 (MSB-aligned) or 0; limited range: 1
    int32_t cw, ch, pitch, ypitch;
    uint64_t plane_bytes, yplane_bytes; // multiples of 16
    uint8_t *planes, *yplanes;
};
int launch_ycbcr_matrix_batch(const YccMatrixBatchArgs &a, void *stream, void *const *ev = nullptr);

// Float pictures (jpegamd_encode_float_batch_async and its twins, jpegamd_float.hip).  k_float_planes_batch reads every f32 / f16 /
// bf16 sample of the batch once, where it lies, makes the byte of each (jpeg_compression.h: x * scale + offset in two float32
// roundings, round half to even, clamp, NaN -> 0), applies the header's RGB -> YCbCr map and chroma subsampling to those bytes, and
// writes the planes exactly where k_ycbcr_matrix_batch writes its own: what codes a BT.709 batch's planes codes these unchanged.
constexpr int kFloatF32 = 0, kFloatF16 = 1, kFloatBF16 = 2;                 // JPEGAMD_FLOAT_*
// three planes of packed samples / the three channels of a pixel side by side, read from plane[0] / samples pixel_stride apart
constexpr int kFloatWalkPlanar = 0, kFloatWalkPacked3 = 1, kFloatWalkGeneric = 2;
// Y, Cb and Cr planes / the Y plane alone of three channels / the bytes of the single channel as the Y plane
constexpr int kFloatOutColor = 0, kFloatOutLuma = 1, kFloatOutSingle = 2;
struct FloatPlanesBatchArgs {
    const uint8_t *plane[3][kMaxBatch]; // R, G, B of every picture (kFloatOutSingle: plane[0] alone; kFloatWalkPacked3: plane[0] is the
                                        // lowest of the three pointers)
    int32_t batch;
    int32_t width, height, row_stride, pixel_stride;       // strides in bytes, multiples of the sample size
    int32_t mode, walk, type, out;      // kChromaMode* (kFloatOutColor alone), kFloatWalk*, kFloatF32 / F16 / BF16, kFloatOut*
    int32_t reversed;                   // kFloatWalkPacked3: the pixel's samples lie B, G, R
    float scale, offset;
    int32_t cw, ch, pitch, ypitch;      // (kFloatOutLuma, kFloatOutSingle: cw = width, ch = height; pitch, plane_bytes, planes unused)
    uint64_t plane_bytes, yplane_bytes; // multiples of 16
    uint8_t *planes, *yplanes;
};
int launch_float_planes_batch(const FloatPlanesBatchArgs &a, void *stream, void *const *ev = nullptr);

// Reduced pictures (jpegamd_encode_reduced_batch_async and its twins, jpegamd_reduce.hip).  k_reduce_planes_batch reads every byte of
// the batch's sources once, where it lies, forms the mean of every factor x factor box (jpeg_compression.h: (S + (n >> 1)) / n over
// the n samples inside the picture), applies the header's RGB -> YCbCr map and chroma subsampling to those bytes, and writes the planes
// of the REDUCED picture exactly where k_float_planes_batch writes its own.
constexpr int kMaxReduce = 8;                                               // JPEGAMD_MAX_REDUCE
// The division by n = 1 .. kMaxReduce^2 is a multiply by ceil(2^22 / n) and a shift: exact for every numerator up to 255 n + n / 2
// (the error term x e / (n 2^22), e < n, stays below 1 / n; the product below 2^31).  tests/test_reduce_host.py walks all of them.
constexpr int kReduceShift = 22;
constexpr uint32_t reduce_recip(int n) { return (uint32_t)(((1u << kReduceShift) + (uint32_t)n - 1u) / (uint32_t)n); }
// the walks and outputs of the float pass: three planes of bytes / R G B (or B G R) bytes side by side, read from plane[0] / bytes
// pixel_stride apart (and every factor that is not 1, 2, 4 or 8)
constexpr int kReduceWalkPlanar = 0, kReduceWalkPacked3 = 1, kReduceWalkGeneric = 2;
constexpr int kReduceOutColor = 0, kReduceOutLuma = 1, kReduceOutSingle = 2;
struct ReducePlanesBatchArgs {
    const uint8_t *plane[3][kMaxBatch]; // R, G, B of every picture (kReduceOutSingle: plane[0] alone; kReduceWalkPacked3: plane[0] is the
                                        // lowest of the three pointers)
    int32_t batch;
    int32_t src_width, src_height, row_stride, pixel_stride;   // the source: samples, bytes
    int32_t factor;                     // 1 .. kMaxReduce
    int32_t width, height;              // the reduced picture: ceil(src_width / factor), ceil(src_height / factor)
    int32_t mode, walk, out;            // kChromaMode* (kReduceOutColor alone), kReduceWalk*, kReduceOut*
    int32_t reversed;                   // kReduceWalkPacked3: the pixel's bytes lie B, G, R
    int32_t cw, ch, pitch, ypitch;      // (kReduceOutLuma, kReduceOutSingle: cw = width, ch = height; pitch, plane_bytes, planes unused)
    uint64_t plane_bytes, yplane_bytes; // multiples of 16
    uint8_t *planes, *yplanes;
};
int launch_reduce_planes_batch(const ReducePlanesBatchArgs &a, void *stream, void *const *ev = nullptr);

// Resized pictures (jpegamd_encode_resized_batch_async and its twins, jpegamd_resize.hip).  k_resize_planes_batch makes every sample
// of the width x height target the exact area mean of the src_width x src_height source (jpeg_compression.h, "Resized pictures":
// (S + (D >> 1)) / D with D = src_width src_height), applies the header's RGB -> YCbCr map and chroma subsampling to those bytes, and
// writes the planes exactly where k_float_planes_batch writes its own.
constexpr int kMaxResizeRatio = 64;                                         // JPEGAMD_MAX_RESIZE_RATIO
// The division of n = S + (D >> 1) <= 256 D by D < 2^32, whose quotient is at most 256: the bits of n above `shift` times
// mul = floor(2^(31 + shift) / D), >> 31, is the quotient or one less, and one comparison of the remainder corrects it.  With
// shift = max(0, bits(D) - 12): cutting n costs at most 2^shift / D <= 2^-11 of the quotient and cutting mul at most
// n / 2^(31 + shift) <= 2^-11, less than 2^-10 together; at shift == 0 (D < 2^12, n < 2^20) n is not cut at all and the one
// truncation costs n / 2^31 < 2^-11.  The kernel and jpegamd_debug_resize_divide share this text.
struct ResizeDivide { uint32_t d, mul; int32_t shift; };
constexpr ResizeDivide resize_divide_for(uint32_t d) {
    int bits = 0;
    for (uint32_t t = d; t; t >>= 1) ++bits;
    const int shift = bits > 12 ? bits - 12 : 0;
    return ResizeDivide{d, (uint32_t)(((uint64_t)1 << (31 + shift)) / d), shift};
}
constexpr uint32_t resize_divide(uint64_t n, uint32_t d, uint32_t mul, int shift) {
    uint32_t q = (uint32_t)(((uint64_t)(uint32_t)(n >> shift) * mul) >> 31);
    if (n - (uint64_t)q * d >= d) ++q;
    return q;
}
// the walks: three planes of bytes one apart (16-byte loads) / the three channels of a pixel inside its pixel_stride <= kResizePackedMax
// bytes, read as one run from plane[0] (R G B, B G R, RGBA, BGRA) / bytes pixel_stride apart, gathered one by one
constexpr int kResizeWalkPlanar = 0, kResizeWalkPacked = 1, kResizeWalkGeneric = 2;
constexpr int kResizeOutColor = 0, kResizeOutLuma = 1, kResizeOutSingle = 2;
constexpr int kResizePackedMax = 4;
constexpr int kResizeLdsBudget = 32768;                                     // bytes of source rows a workgroup stages at a time
struct ResizePlanesBatchArgs {
    const uint8_t *plane[3][kMaxBatch]; // R, G, B of every picture (kResizeOutSingle: plane[0] alone; kResizeWalkPacked: plane[0] is the
                                        // lowest of the three pointers and offset[] says where each channel lies from it)
    int32_t batch;
    int32_t src_width, src_height, row_stride, pixel_stride;   // the source: samples, bytes
    int32_t width, height;              // the target: width <= src_width <= 64 width, the same for the heights
    int32_t mode, walk, out;            // kChromaMode* (kResizeOutColor alone), kResizeWalk*, kResizeOut*
    int32_t offset[3];                  // kResizeWalkPacked: bytes from plane[0] to R, G, B, each below pixel_stride
    int32_t cw, ch, pitch, ypitch;      // (kResizeOutLuma, kResizeOutSingle: cw = width, ch = height; pitch, plane_bytes, planes unused)
    uint64_t plane_bytes, yplane_bytes; // multiples of 16
    uint8_t *planes, *yplanes;
    // filled by launch_resize_planes_batch
    ResizeDivide div;                   // by D = src_width src_height
    int32_t lds_pitch, lds_rows;        // bytes of one staged source row of one run (a multiple of 16); source rows staged at a time
};
int launch_resize_planes_batch(const ResizePlanesBatchArgs &a, void *stream, void *const *ev = nullptr);
// k_picture_stats: what the tile records of one k_tile_encode launch add up to per picture and scan -- bits (with the first DC
// symbol of every tile, which the record leaves out), run/size symbols, exact-order fallbacks -- summed into
// pic[picture][scan][3].  Launch image i is picture i, scan 0 (luma), or plane first_plane + i (chroma).
constexpr int kPicStatWords = 9;        // [scan 0..2][bits, symbols, exact]
struct PictureStatsArgs {
    const uint32_t *tile_head;
    const uint32_t *huff;               // the scan's table: DC size s at 256 + s
    int32_t tiles_per_image, batch;
    int32_t chroma, first_plane;
    unsigned long long *pic;            // [picture][kPicStatWords]
};
int launch_picture_stats(const PictureStatsArgs &a, void *stream);
// k_append_scans_batch: per picture, behind its Y scan: SOS(2), the Cb scan, SOS(3), the Cr scan, EOI -- only when the whole file
// fits; the picture's size (0 when it did not fit); the context's record (last picture's size, sums over every picture and scan).
struct AppendBatchArgs {
    uint8_t *out[kMaxBatch];
    uint64_t *out_size[kMaxBatch];
    uint64_t out_capacity;
    int32_t batch, hdr_len;
    const uint64_t *y_size;             // [batch] prefix + Y scan
    const uint64_t *c_size;             // [2 batch] bare chroma scans, by plane
    const uint8_t *scans;               // plane j's scan at scans + j * slot_bytes (slot_bytes a multiple of 16)
    uint64_t slot_bytes;
    const uint8_t *sos;                 // SOS(2) at 0, SOS(3) at 16
    const unsigned long long *pic;      // [batch][kPicStatWords]
    const ScanStats *launch_stats;      // [n_launch] the records of the Y launch and of every chroma launch
    int32_t n_launch;
    ScanStats *stats;                   // the context's record
};
int launch_append_scans_batch(const AppendBatchArgs &a, void *stream, void *const *ev = nullptr);

// Metadata in front of the tables (jpegamd_metadata.hip).  The entries of a context that holds metadata of M bytes
// write each file at out + M; k_metadata_place then copies `bytes` = 20 + M bytes -- the file's 20 leading bytes with the caller's
// density, then the marker segments -- to out[0, bytes), over the shifted copy of those 20 bytes, and adds M to every size word that
// is not zero (a file that did not fit keeps its zero) and to the record's out_size.  A picture with out_capacity < bytes is left alone.
constexpr int kJfifHeadBytes = 20;      // SOI and the APP0 segment: what every file begins with
constexpr int kMetaSrcPad = 32;         // zero bytes behind src[bytes): the kernel reads whole 16-byte pieces, one beyond the last
struct MetadataPlaceArgs {
    uint8_t *out[kMaxBatch];
    uint64_t *out_size[kMaxBatch];
    uint64_t out_capacity;
    const uint8_t *src;                 // 16-byte aligned; bytes + kMetaSrcPad readable
    uint64_t bytes;                     // 20 + M
    int32_t batch;
    ScanStats *stats;                   // the context's record
};
// end_event (may be null): takes the kernel's end stamp, as the events of launch_append_scans_batch do.
int launch_metadata_place(const MetadataPlaceArgs &a, void *stream, void *end_event = nullptr);

// Interleaved-MCU colour files (jpegamd_encode_color_interleaved_batch_async, jpegamd_mcu.hip): ONE scan coded from coefficient
// planes.  A picture's planes lie at coef + picture * pic_stride (int16 elements): Y [bh][bw][64] at 0, Cb and Cr [my][mx][64] at
// cb_off / cr_off -- what the stage-tap build of k_tile_encode stores through tap_zz, zigzag order inside a block.  The MCU grid
// is mx x my MCUs of hs x vs Y blocks, one Cb and one Cr block; Y blocks with bx >= bw or by >= bh are pad blocks.  Segment s of a
// picture is the MCUs [s seg_mcus, (s + 1) seg_mcus) of the raster MCU order; every picture has num_segs_pad entries in the segment
// arrays -- num_segs rounded up to kSegGroup with EMPTY segments (no bits), so that k_finalize's four-at-a-time reads of the
// per-segment arrays stay aligned for every picture of a batch.
// A scan of ONE component (comps = 1: the grayscale file of DESIGN.md 4.6.11) is the same with an MCU of one block: the plane at 0
// alone, mx x my = bw x bh, no pad blocks, a segment of kSegBlocks consecutive blocks.
constexpr int mcu_blocks_per_mcu(int hs, int vs, int comps = 3) { return comps == 1 ? 1 : hs * vs + 2; }
constexpr int mcu_seg_mcus(int hs, int vs, int comps = 3) { return kSegBlocks / mcu_blocks_per_mcu(hs, vs, comps); }     // 85 / 42 / 64, one component: 256 -- at most 256 blocks per segment
static_assert(mcu_seg_mcus(1, 1, 1) == kSegBlocks, "a segment of a one-component scan is kSegBlocks blocks");
static_assert(mcu_seg_mcus(1, 1) * 3 <= kSegBlocks && mcu_seg_mcus(2, 2) * 6 <= kSegBlocks && mcu_seg_mcus(2, 1) * 4 <= kSegBlocks &&
              kSegBlocks == kTileBlocks * kSegTiles, "a segment of MCUs fits seg_cap_words(kSegTiles)");
//
// Restart intervals: with restart = Ri > 0 the scan is n = ceil(M / Ri) intervals of Ri MCUs (M = mx my), and a
// segment never crosses an interval's boundary: every interval has segs_per_interval = ceil(min(Ri, M) / seg_mcus) segments, segment
// (i, k) -- entry i segs_per_interval + k of the picture -- holds the MCUs [i Ri + k seg_mcus, min(i Ri + (k + 1) seg_mcus, (i + 1) Ri, M)),
// EMPTY where that range is (only behind the last interval's last MCU).  The DC predictors are 0 at MCU i Ri.  A segment holds at
// most min(Ri, seg_mcus) MCUs, and its string is reserved for that many blocks: mcu_restart_cap_words.
constexpr int mcu_restart_cap_words(int blocks) { return ((blocks * kMaxBlockBitsColor + 31) / 32 + 1 + 63) / 64 * 64; }   // seg_cap_words_at's rounding
static_assert(mcu_restart_cap_words(kSegBlocks) == seg_cap_words_at(kSegTiles, kMaxBlockBitsColor), "a full segment takes the reservation of the plain scan");
struct McuSegArgs {
    const int16_t *coef;
    uint64_t pic_stride, cb_off, cr_off;
    int32_t bw, bh, mx, my, hs, vs;
    int32_t seg_mcus, num_segs, num_segs_pad, batch;
    const uint32_t *huff_y, *huff_c;    // [272] (len << 16) | code: AC by run/size symbol, then 16 DC sizes
    uint32_t huff_stride;               // words from a picture's tables to the next picture's (k_huff_optimal's); 0: every picture codes with the same (Annex K)
    SegArrays seg;                      // the interleaved path's own (words_stride = seg_cap_words(kSegTiles), or mcu_restart_cap_words); no group aggregates
    uint32_t *status;                   // ScanStats::status: bit 1 = a count that did not fit its 16 bits
    int32_t restart, segs_per_interval; // 0, 0: no restart intervals
    int32_t comps;                      // components of the scan: 3, or 1 (hs = vs = 1, mx = bw, my = bh; cb_off, cr_off and huff_c are not read)
    // launch_mcu_band_segments alone (a scan of a progressive file; k_mcu_segments reads none of these):
    int32_t ss, se;                     // the band, uniform over the launch: 0, 0 the DC scan (comps = 3), 1 <= ss <= se <= 63 an AC scan (comps = 1)
    unsigned long long *sums;           // [batch][2]: every segment's bits and symbols are ADDED to its picture's pair (the caller zeroed them)
    int32_t runs;                       // an AC scan with end-of-band runs and the pictures' own tables (huff_stride > 0); the DC scan: its own tables
    // successive approximation (`runs` alone): ah = 0, al > 0 a first scan over the point transform by al; ah = al + 1
    // a refinement scan that codes bit al.  0, 0: the scans of 4.6.12 / 4.6.13.  (They lie in what was the struct's padding.)
    uint8_t ah, al;
    // a caller's scan script: comps = 2, the DC scan of TWO interleaved components -- bit 0 Y, bit 1 Cb, bit 2 Cr,
    // two of them: Y as hs x vs blocks with pad blocks, a chroma component one block; the MCU grid, planes and strides are the
    // three-component scan's.  huff_y: the table of the scan's first component class, huff_c: of its second ({Cb, Cr}: not read).
    // comps = 1 with ss = se = 0: the DC scan of one component over its own block grid.  Not read by the other scans.
    uint8_t mask;
};
// blocks per MCU and MCUs per segment of a two-component DC scan
constexpr int mcu_blocks_per_mcu2(int hs, int vs, int mask) { return (mask & 1 ? hs * vs : 0) + ((mask >> 1) & 1) + ((mask >> 2) & 1); }
int launch_mcu_segments(const McuSegArgs &a, void *stream);

// Progressive colour files: kProgScans scans by spectral selection, Ah = Al = 0 -- the DC scan of the three
// components in MCU order (the segments, pad blocks and predictors of the one-scan file), then the bands 1 .. 5 and 6 .. 63 of Y, Cb
// and Cr, each a scan of ONE component over its plane's blocks in raster order (comps = 1: coef points at the plane, bw x bh is ITS
// block grid, huff_y ITS table class).  launch_mcu_band_segments codes one scan into the segment arrays; the unchanged k_finalize
// writes it -- scan 1 behind the file's prefix into the caller's buffer, the others behind their SOS into slots of context scratch --
// and k_scans_concat puts the slots behind scan 1 when the whole file fits, writes the size word and adds up the call's record.
// A block of a band is at most 27 bits per coefficient of the band (a ZRL pays for sixteen zeros, EOB for a zero coefficient se),
// a DC difference at most 11 + 11 bits: together no more than kMaxBlockBitsColor, the bound of a whole block.
constexpr int kProgScans = 7;
constexpr int kProgScansMax = 16, kProgTablesMax = 16;          // the most scans and tables a scan script has (JPEGAMD_MAX_SCANS); the kernels take the counts at run time
constexpr int kProgBandSs[2] = {1, 6}, kProgBandSe[2] = {5, 63};
constexpr int prog_band_bits(int band) { return (kProgBandSe[band] - kProgBandSs[band] + 1) * 27; }
static_assert(22 + prog_band_bits(0) + prog_band_bits(1) == kMaxBlockBitsColor, "the three bands of a block cost no more than the block's bound");
int launch_mcu_band_segments(const McuSegArgs &a, void *stream);
struct ScansConcatArgs {
    uint8_t *out[kMaxBatch];
    uint64_t *out_size[kMaxBatch];
    uint64_t out_capacity;
    int32_t batch;
    int32_t prefix_len;                 // bytes in front of scan 1's entropy-coded segment: the file's prefix with SOS 1
    int32_t last_of_call;               // the launch's last picture is the call's last: its size is what finish reports
    int32_t scans;                      // the file's scans: 1 .. kProgScansMax (one scan: nothing is appended)
    const uint64_t *size;               // [scans][kMaxBatch] k_finalize's: scan 1 with the prefix, the others with their SOS, the last with EOI
    const uint8_t *slots;               // scan k >= 1 (from 0) of picture q at slots + q pic_bytes + slot_off[k]; multiples of 16
    uint64_t pic_bytes, slot_off[kProgScansMax];
    const unsigned long long *sums;     // [scans][kMaxBatch][2] coded bits and symbols (launch_mcu_band_segments)
    const unsigned long long *pic;      // k_picture_stats' words of THESE pictures
    const ScanStats *scan_stats;        // [2] k_finalize's records: scan 1's, and the one the scans into slots share
    ScanStats *stats;                   // the context's record, whose sums the caller zeroed
    // the scans went through the restart writer: `size` is k_mcu_restart_offsets' -- every scan with ITS header, the
    // last with EOI --, and the stuffed bytes are word 2 of its sums, [scans][kMaxBatch][kMcuPicSums]; null: k_finalize's scans
    const unsigned long long *writer_sums;
};
int launch_scans_concat(const ScansConcatArgs &a, void *stream);
// Progressive files with end-of-band runs and per-scan optimised tables: kProgTables tables per picture in the
// file's order -- Y DC, chroma DC (scan 1), then the AC tables of the scans 2 .. 7.  launch_mcu_band_histogram counts the symbols of
// one scan (the coder's walks, no table read) into counts [pictures][kProgTables][256], which the caller zeroed; k_huff_optimal makes
// BITS / HUFFVAL of all of them in one launch (its `freq` form: the counts ARE kProgTables x pictures jobs of 256 symbols);
// k_prog_tables makes the coder's tables and every scan's header -- DHT segment(s) + SOS, scan 1's behind the file's head -- of them.
// With successive approximation the scans and tables are a script's: `tables` tables per picture in `counts`,
// and the launches below take the script's numbers -- the seven-scan file's are kProgScans and kProgTables.
constexpr int kProgTables = 8;
int launch_mcu_band_histogram(const McuSegArgs &a, unsigned long long *counts, int table, int tables, void *stream);
struct ProgTablesArgs {
    const uint8_t *res;                 // [launch pictures][tables][kHuffResBytes] k_huff_optimal's
    uint32_t *tabs;                     // [launch pictures][tables][272]
    uint8_t *hdr_out;                   // scan k (from 0) of picture p of the CALL at hdr_out + (k pictures + p) kMcuPrefixSlot
    uint32_t *hdr_len;                  // [scans][pictures]
    int32_t pictures, first;            // pictures of the call; the launch's first
    const uint8_t *hdr;                 // the standard progressive prefix: its head (SOI .. SOF2) is the file's
    int32_t head_len;
    const uint8_t *sos;                 // the SOS of scan k (from 0) at sos + 16 k, sos_len[k] bytes
    int32_t scans, tables;              // the script's: 1 .. kProgScansMax, 1 .. kProgTablesMax
    uint32_t bare;                      // bit k: scan k has no table -- its header is its SOS alone
    uint8_t table_scan[kProgTablesMax]; // the scan (from 0) of table t: non-decreasing, table 0 (and 1, when it has two) the DC tables of scan 0; any scan may own two
    uint8_t table_id[kProgTablesMax];   // its Tc/Th byte
    uint8_t sos_len[kProgScansMax];
};
int launch_prog_tables(const ProgTablesArgs &a, int batch, void *stream);
// The writer of a file with restart intervals: two launches in place of k_finalize (which knows neither the 1-bit padding of an
// interval nor markers).  k_mcu_restart_offsets, one workgroup per picture: every segment's bit offset inside its interval (pre is its
// scratch: the bit counts' running sum over the picture), the 0xFF bytes it owns at that phase, and -- an exclusive sum over the
// picture of what every segment writes -- its place in the file; the picture's sums (bits, symbols, stuffed bytes) and its would-be size word.
// k_mcu_restart_write, one wave per segment: the bytes whose last bit the segment holds, stuffed; an interval's last segment adds
// the padded byte, its stuffing byte and RSTn, the picture's last one the zero-bit flush and EOI; the first workgroup the prefix.
constexpr int kMcuPicSums = 4;
struct McuRestartArgs {
    SegArrays seg;
    int32_t num_segs_pad, batch;
    int32_t segs_per_interval, intervals;
    int32_t last_seg;                   // the picture's last segment that is not EMPTY
    uint32_t *pre, *b0, *ff;            // [batch][num_segs_pad]
    uint64_t *pos;                      // [batch][num_segs_pad] bytes of the scan in front of the segment's own
    unsigned long long *pic_sums;       // [batch][kMcuPicSums] the picture's coded bits, symbols and stuffed 0x00 bytes
    uint8_t *out[kMaxBatch];
    uint64_t out_capacity;
    uint64_t *out_size[kMaxBatch];
    const uint8_t *prefix;
    int32_t prefix_len;
    // per-picture prefixes (optimised Huffman tables: k_huff_optimal wrote them): picture q's is pic_prefix + q pic_prefix_stride,
    // pic_prefix_len[q] bytes, read from device memory; null: `prefix` / `prefix_len` for every picture
    const uint8_t *pic_prefix;
    const uint32_t *pic_prefix_len;
    uint32_t pic_prefix_stride;
    int32_t no_eoi;                     // the scan's last segment flushes its byte with 0-bits and writes no EOI: another scan follows
};
int launch_mcu_restart_writer(const McuRestartArgs &a, void *stream);
// k_mcu_totals, behind k_finalize: per picture of the launch the sums of its segments, its stuffed bytes (from its size) and its
// exact-order fallbacks (pic: k_picture_stats' words of THESE pictures) ADDED to the context's record, whose sums the caller zeroed;
// the picture's size word set to 0 when the file did not fit; scan_stats->status (k_finalize's) ORed into the context's.
struct McuTotalsArgs {
    SegArrays seg;
    int32_t num_segs_pad, prefix_len;
    int32_t last_of_call;               // the launch's last picture is the call's last: its size is what finish reports
    const unsigned long long *pic_sums; // k_mcu_restart_offsets' sums of THESE pictures (McuRestartArgs), taken instead of the sums over the segments
                                        // and the stuffed bytes from the size (which holds markers and a padded byte per interval); null without restart intervals
    uint64_t *out_size[kMaxBatch];
    uint64_t out_capacity;
    const unsigned long long *pic;
    const ScanStats *scan_stats;
    ScanStats *stats;
};
int launch_mcu_totals(const McuTotalsArgs &a, int batch, void *stream, void *const *ev = nullptr);

// Per-picture optimised Huffman tables of the one-scan files.  k_mcu_histogram: the coder's grid and block walk
// (McuSegArgs, no tables read) with every symbol counted instead of coded, into counts [batch][2][272] u64 -- a component class's AC
// symbols by run/size at 0, its DC sizes at 256, luma first: the layout of the coder's tables -- which the caller zeroed on the stream.
int launch_mcu_histogram(const McuSegArgs &a, unsigned long long *counts, void *stream);
// k_huff_optimal, one wave per table and four tables (luma DC, luma AC, chroma DC, chroma AC) per workgroup: T.81 K.2 as libjpeg
// carries it out.  A table's counts must sum to less than 2^54 (the merge key holds a count and a slot index in 64 bits).
// Always: res [jobs][kHuffResBytes] -- BITS[16], the number of HUFFVAL bytes (u32 at 16), HUFFVAL at 32.
// With `freq` (jpegamd_debug_optimal_huffman): job j reads freq + 256 j, 256 symbols, and nothing else is written.
// Without: job tables q + t reads picture q's counts, and the workgroup writes the picture's coder tables (tabs + q kMcuTabWords: [2][272],
// unused symbols 0), its prefix (prefix + q kMcuPrefixSlot: hdr[0, head_len), the `tables` DHT segments, hdr[tail_off, tail_off + tail_len))
// and the prefix's length (prefix_len[q]).  The caller cuts the standard DHT segments out of hdr: head_len = tail_off - kStdDhtBytes[Gray].
constexpr int kMcuTabWords = 2 * 272;
constexpr int kMcuPrefixSlot = 704;     // >= kColorPrefixMax + DRI + SOS: an optimised prefix is never longer than the standard one
constexpr int kHuffResBytes = 288;
constexpr int kStdDhtBytes = 432;       // the four Annex K DHT segments: 2 x (33 + 183)
constexpr int kStdDhtBytesGray = 216;   // the two of a one-component file: K.3 and K.5
// A block coded with a picture's own tables is at most 27 + 63 x 26 bits (DC: 16 + 11, AC: 16 + 10): the strings reserved with
// kMaxBlockBitsColor hold 256 of them.
constexpr int kMaxBlockBitsOptimized = 27 + 63 * 26;                 // 1665
static_assert(kMaxBlockBitsOptimized <= kMaxBlockBitsColor && (kSegBlocks * kMaxBlockBitsOptimized + 31) / 32 + 1 <= mcu_restart_cap_words(kSegBlocks),
              "a segment of 256 blocks in either Huffman mode fits its string");
// Successive approximation.  A first scan codes shifted values: the sizes only shrink, so its block is within
// kMaxBlockBitsOptimized.  A block of an AC refinement scan: a new coefficient costs a symbol and its sign, 16 + 1 bits; an old one its
// correction bit; sixteen zeros a ZRL of at most 16 bits -- a bit each; the run's symbol 16 + 8 bits, and only a block whose
// coefficient se is not new (it costs at most 1 bit) starts one: 62 x 17 + max(17, 1 + 24).  A block of the DC refinement scan: 1 bit.
constexpr int kMaxBlockBitsRefine = 62 * 17 + 25;                    // 1079
static_assert(kMaxBlockBitsRefine <= kMaxBlockBitsOptimized, "one block's string in any single scan fits the reservation of a segment");
struct HuffOptimalArgs {
    const unsigned long long *counts;   // [pictures][2][272], or null
    const unsigned long long *freq;     // [jobs][256], or null
    int32_t jobs;
    int32_t tables;                     // with `counts`: tables per picture -- 4, or 2 (one component: luma DC and AC alone); jobs = tables x pictures
    uint8_t *res;
    uint32_t *tabs;
    uint8_t *prefix;
    uint32_t *prefix_len;
    const uint8_t *hdr;
    int32_t head_len, tail_off, tail_len;
};
int launch_huff_optimal(const HuffOptimalArgs &a, void *stream);

// ---- host-side constant derivation (quant_consts.cpp) ----------------------------------
void quant_table_for_quality(int quality, uint8_t table[64]);
// T.81 Annex K K.2 (the chroma table), scaled for `quality` with the rule of quant_table_for_quality
void chroma_quant_table_for_quality(int quality, uint8_t table[64]);
void build_huffman_words_chroma(uint32_t words[272]);
void build_code_table_chroma(uint32_t words[kCodeWords]);
// The colour file's headers up to the Y scan: SOI, APP0, DQT (tables 0 and 1), SOF0 (3 components), DHT x 4, SOS (Y).  Returns
// the byte count (<= kColorPrefixMax).  color_sos: the SOS segment in front of the scan of component 2 or 3 (10 bytes).
constexpr int kColorPrefixMax = 640;
constexpr int kSosBytes = 10;
// mode (kChromaMode*): the sampling factors of component 1 in SOF0 -- 0x11, 0x22 or 0x21.
size_t build_jfif_prefix_color(int width, int height, const uint8_t luma[64], const uint8_t chroma[64], int mode,
                               uint8_t out[kColorPrefixMax]);
void color_sos(int component, uint8_t out[kSosBytes]);
// A-row order of the pipeline: lane half h, site s <-> zigzag 16(s>>3) + 8h + (s&7)
void derive_mfma_tables(const uint8_t table[64], MfmaTables *mt, double delta_out[64] /*by raster k, may be null*/);
void build_huffman_words(uint32_t words[272]);
void build_code_table(uint32_t words[kCodeWords]);
void cos_lut_copy(float out[64]);              // COS_LUT[x][u] as the kernels use it (natural_c/src/core/dct.c:9-18)
size_t build_jfif_prefix(int width, int height, const uint8_t table[64], uint8_t out[328]);

extern const uint8_t kZigzagHost[64];

// Process-wide context behind JpegCompression_Init / convertToJpeg / saveJPEGGrayscale
// (jpegamd_api.cpp); grows to fit w x h.  Returns nullptr without a usable HIP device.
::JpegAmdEncoder *shared_context(int w, int h, uint64_t **size_dev);
// Block (0,0) stage taps (host outputs): centred luma, exact-order DCT, quantised zigzag.
int32_t first_block_taps(::JpegAmdEncoder *e, const struct ::JpegAmdImage *img, int8_t y[64], float dct[64],
                         int16_t zz[64]);

}  // namespace jpegamd
