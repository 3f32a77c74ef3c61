// jpegamd_api.cpp -- C-ABI host layer over the HIP kernels (include/jpeg_compression.h).
//
// Level 1 (jpegamd_*): device-resident, stream-ordered encode: k_tile_encode -> k_segment_merge -> k_finalize, or -- very large
//          pictures, where k_finalize's scan over every predecessor would grow quadratically -- k_tile_encode -> k_stitch.
// Level 2 (JpegCompression_Init / convertToJpeg): the reference's accelerator boundary
//          (dsp_port/jpeg_compression/src/jpeg_compression.c:6-33,35-216).
// There is no CPU fallback: without a HIP device every compute entry fails.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "jpeg_compression.h"
#include "jpegamd_internal.h"

using namespace jpegamd;

#define HIP_TRY(expr)                                                                           \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) {                                                                 \
            std::fprintf(stderr, "jpegamd: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_), \
                         __FILE__, __LINE__);                                                   \
            return JPEGAMD_ERR_HIP;                                                             \
        }                                                                                       \
    } while (0)

// What a context created for max_w x max_h holds: the bounds every launch on it is checked against.
struct CtxLimits {
    int max_segs, max_tiles, max_wgs;
    size_t words_cap;                   // words of seg.words
};

// What a header kept on the device was built for, and its length.  Plain data: all zero means "nothing cached" (no picture is 0 wide).
struct HeaderCache {
    int w, h, q, sub, len;
    int restart;                        // the interval of the DRI segment (files with one: the interleaved path's); 0: none
    int progressive;                    // 1: the prefix of a progressive file (SOF2, the DC scan's SOS: the interleaved path's); 0: baseline
    bool matches(int w_, int h_, int q_, int sub_, int restart_ = 0, int progressive_ = 0) const {
        return w == w_ && h == h_ && q == q_ && sub == sub_ && restart == restart_ && progressive == progressive_;
    }
    void set(int w_, int h_, int q_, int sub_, int len_, int restart_ = 0, int progressive_ = 0) {
        w = w_; h = h_; q = q_; sub = sub_; len = len_; restart = restart_; progressive = progressive_;
    }
};

constexpr int kFirstTableKey = 101;     // (the qualities end at 100)

struct JpegAmdEncoder {
    int device = -1;
    int max_w = 0, max_h = 0;
    CtxLimits lim = {};
    // device scratch, sized once for max_w x max_h
    SegArrays seg = {};
    uint32_t *huff = nullptr;
    uint8_t *prefix = nullptr;
    ScanStats *stats_dev = nullptr;
    ScanStats mirror;            // host copy of stats_dev, fetched by finish()
    MfmaTables *tables_dev = nullptr;
    MfmaTables *tables_host = nullptr;          // this context's own staging copy (contexts may be driven from different threads)
    uint32_t *tile_head = nullptr, *tile_over = nullptr, *tile_ctr = nullptr, *code_tab = nullptr;
    int ctr_set = 0;                    // which half of tile_ctr the next k_tile_encode launch uses
    uint32_t *desc = nullptr;           // k_stitch's hand-off granules: max_wgs x 16 bytes, then max_wgs x 8 counts in full
    uint32_t epoch = 0;                 // 1 .. 16383: tag of the last k_stitch launch's granules
    int pipeline = JPEGAMD_PIPELINE_AUTO;
    int huffman = JPEGAMD_HUFFMAN_STANDARD;     // jpegamd_encoder_set_huffman: the tables of the one-scan entries
    int poison_tile = -1;               // jpegamd_debug_poison_tile_record: the next encode overwrites this tile's record word 0 ...
    uint32_t poison_value = 0;          // ... with this value, between k_tile_encode and k_segment_merge
    unsigned long long *stamps_dev = nullptr;   // per-wave phase cycle sums of the stamped kernel (allocated by the first convertToJpeg, or with JPEGAMD_STAMPS=1)
    bool stamp_next = false;                    // the next k_tile_encode launch is the stamped variant (convertToJpeg)
    // The caller's quantisation tables (jpegamd_encoder_set_quant_tables; raster order) and the key the caches below hold them under:
    // outside 0 .. 100, where the keys of the quality-driven pictures lie, and new with every successful set.
    bool custom_tables = false;
    int table_key = kFirstTableKey - 1;
    uint8_t custom_luma[64], custom_chroma[64];
    // Metadata (jpegamd_encoder_set_metadata): the 20 leading bytes of every file, the blob and kMetaSrcPad zero bytes
    // as ONE host string, empty while nothing is set; its copy in device scratch that only grows, made by the next encode.
    std::vector<uint8_t> meta;
    bool meta_dirty = false;
    uint8_t *meta_dev = nullptr;
    size_t meta_cap = 0;
    // cached constants (cur_quality, color.cur_quality and the q of the three HeaderCaches are table keys: quant_choice)
    int cur_quality = -1;
    uint8_t qtable[64];
    HeaderCache prefix_for = {};        // what `prefix` holds (no subsampling: 0)
    // profiling: a ring of event quadruples so callers can time many async encodes and read
    // the per-kernel durations after ONE synchronisation
    struct EventSet {
        hipEvent_t ev[6]; bool merged;   // begin / end of k_tile_encode, [k_segment_merge,] k_stitch or k_finalize (the kernels' own timestamps)
        // a colour encode (made on the slot's first one): k_chroma_planes, 3 x the six above, k_append_scans
        std::vector<hipEvent_t> cev; bool color = false; bool cmerged[3] = {false, false, false};
        bool cbatch = false;             // a colour batch: only cev[0] (k_chroma_planes_batch begin) and cev[21] (k_append_scans_batch end)
    };
    std::vector<EventSet> ring;
    uint64_t calls = 0;          // encodes enqueued since profiling was (re)enabled
    int last_slot = -1;
    // last call
    int last_segs = 0;
    hipStream_t last_stream = nullptr;
    bool pending = false;
    bool timed = false;
    bool last_color = false;            // the last call was a colour encode: its statistics are summed already (k_append_scans)
    // Colour (jpegamd_encode_color_async): nothing of this is allocated before the context's first colour call.
    struct Color {
        MfmaTables *tables_dev = nullptr;   // the chroma table's constants (a second set: no re-upload between the scans)
        uint32_t *code_tab = nullptr, *huff = nullptr;
        uint8_t *hdr = nullptr;             // [0, kColorPrefixMax) the prefix up to the Y scan; then the SOS of Cb and of Cr
        uint64_t *scan_size = nullptr;      // [3]
        ScanStats *scan_stats = nullptr;    // [3]
        uint8_t *planes = nullptr;          // Cb, then Cr
        uint8_t *scans = nullptr;           // the Cb part, then the Cr part (each scan_cap bytes)
        size_t planes_cap = 0, scan_cap = 0;
        int cur_quality = -1;
        HeaderCache hdr_for = {};           // what the prefix in `hdr` holds
        // colour batches (jpegamd_encode_color_batch_async), sized for the planes and scans of the largest batch so far
        uint8_t *bmeta = nullptr;           // ScanStats [kBatchLaunches], u64 pic [kMaxBatch][kPicStatWords], y_size [kMaxBatch], c_size [2 kMaxBatch]
        uint8_t *bplanes = nullptr, *bscans = nullptr;
        size_t bplanes_cap = 0, bscans_cap = 0;
    } color;
    // Interleaved-MCU colour files (jpegamd_encode_color_interleaved_batch_async): nothing of this is allocated before the context's
    // first such call; sized for that call, grown when a later one needs more.
    struct Mcu {
        int16_t *coef = nullptr;            // the coefficient planes of one group of pictures
        size_t coef_cap = 0;                // int16 elements
        SegArrays seg = {};                 // the path's own segments (an MCU scan has 1.5 x to 3 x the blocks of the Y scan)
        size_t segs_cap = 0, words_cap = 0; // entries of the per-segment arrays, words of the strings
        // restart intervals (jpegamd_encode_*_interleaved_restart_batch_async): what k_mcu_restart_offsets leaves per segment and picture
        uint32_t *rst_words = nullptr;      // pre, b0, ff: 3 x rst_cap
        uint64_t *rst_pos = nullptr;
        unsigned long long *rst_pic_sums = nullptr;   // [kMaxBatch][kMcuPicSums]
        size_t rst_cap = 0;
        uint8_t *hdr = nullptr;             // the prefix with the three-component SOS
        ScanStats *scan_stats = nullptr;    // k_finalize's record of the call
        HeaderCache hdr_for = {};           // what `hdr` holds
        // per-picture optimised Huffman tables (jpegamd_encoder_set_huffman): nothing of this is allocated before the first such call
        unsigned long long *hcounts = nullptr;   // [hcap][2][272] the symbol counts (k_mcu_histogram)
        uint32_t *htabs = nullptr;          // [hcap][2][272] the coder's tables (k_huff_optimal)
        uint8_t *hprefix = nullptr;         // [hcap][kMcuPrefixSlot] the pictures' prefixes
        uint32_t *hprefix_len = nullptr;    // [hcap]
        uint8_t *hres = nullptr;            // [4 hcap][kHuffResBytes] BITS / HUFFVAL as k_huff_optimal leaves them
        int hcap = 0;                       // pictures
        int hlast = 0;                      // pictures of the last optimised call: hcounts[0, hlast) are theirs
        // progressive files (jpegamd_encode_*_progressive_batch_async): nothing of this is allocated before the first such call
        uint8_t *pmeta = nullptr;           // ProgMeta: k_finalize's records, the scans' sizes and sums, the six SOS segments
        uint8_t *pslots = nullptr;          // the scans 2 .. 7 of one group of pictures
        size_t pslots_cap = 0;
        // ... with end-of-band runs and per-scan optimised tables (jpegamd_encode_*_progressive_optimized_batch_async): allocated by the first such call
        unsigned long long *pcounts = nullptr;   // [pcap][kProgTables][256] the symbol counts (k_mcu_band_histogram)
        uint8_t *pres = nullptr;            // [pcap][kProgTables][kHuffResBytes] BITS / HUFFVAL (k_huff_optimal)
        uint32_t *ptabs = nullptr;          // [pcap][kProgTables][272] the coder's tables (k_prog_tables)
        uint8_t *phdr = nullptr;            // [kProgScans][pictures of the call][kMcuPrefixSlot] every scan's DHT segment(s) and SOS
        uint32_t *phdr_len = nullptr;       // [kProgScans][pictures of the call]
        int pcap = 0;                       // pictures
        int plast = 0;                      // pictures of the last such call: pcounts[0, plast) are theirs
        int plast_tables = 0;               // ... and the tables of its script: pcounts is [plast][plast_tables][256]
        int plast_script = 0;               // ... and which script it was: ProgScript::id
        uint8_t psos[16][16] = {};          // a caller's script: the SOS segments that lie in pmeta, the key of that upload
        bool psos_valid = false;
    } mcu;
};

static int segs_for(int w, int h, int *bw, int *bh, int *spr, int seg_tiles = kSegTiles) {
    const int blocks_w = (w + 7) / 8, blocks_h = (h + 7) / 8;
    const int per_row = (blocks_w + kTileBlocks * seg_tiles - 1) / (kTileBlocks * seg_tiles);
    if (bw) *bw = blocks_w;
    if (bh) *bh = blocks_h;
    if (spr) *spr = per_row;
    return blocks_h * per_row;
}

extern "C" const char *jpegamd_version(void) { return "jpegamd 0.4 (gfx950)"; }

extern "C" int32_t jpegamd_segment_meta_words(void) { return kSegMetaWords; }

// Small formulas every entry shares: the tiles of a w x h picture, the quality that is coded, the words of the stamp buffer.
static int tiles_for(int w, int h) { return ((h + 7) / 8) * (((w + 7) / 8 + kTileBlocks - 1) / kTileBlocks); }
static int clamp_quality(int q) { return q <= 0 ? 50 : (q > 100 ? 100 : q); }
static size_t stamp_words(int max_segs) { return (size_t)(max_segs > 4096 ? max_segs : 4096) * 16; }   // 16 per wave

extern "C" int32_t jpegamd_debug_quant_table(int32_t quality, uint8_t *table) {
    if (!table) return JPEGAMD_ERR_ARG;
    quant_table_for_quality(quality, table);
    return JPEGAMD_OK;
}

extern "C" int32_t jpegamd_debug_chroma_quant_table(int32_t quality, uint8_t *table) {
    if (!table) return JPEGAMD_ERR_ARG;
    chroma_quant_table_for_quality(quality, table);
    return JPEGAMD_OK;
}

extern "C" int32_t jpegamd_debug_cos_lut(float *lut /*[8][8]: COS_LUT[x][u]*/) {
    if (!lut) return JPEGAMD_ERR_ARG;
    cos_lut_copy(lut);
    return JPEGAMD_OK;
}

// Behind the constant getters below (host-only, reentrant; tests pin the values against the oracle's arithmetic): the constants of
// the fast path for `quality` with the luma or the chroma table, and the guard bands by raster index, handed to `take`.
template <class Take>
static int32_t with_table_consts(const uint8_t t[64], Take take) {
    double delta[64];
    MfmaTables *mt = new (std::nothrow) MfmaTables;
    if (!mt) return JPEGAMD_ERR_HIP;
    derive_mfma_tables(t, mt, delta);
    take(*mt, delta);
    delete mt;
    return JPEGAMD_OK;
}
template <class Take>
static int32_t with_mfma_consts(int32_t quality, bool chroma, Take take) {
    uint8_t t[64];
    (chroma ? chroma_quant_table_for_quality : quant_table_for_quality)(quality, t);
    return with_table_consts(t, take);
}
template <class T, size_t N>
static void copy_out(void *dst /*may be null*/, const T (&src)[N]) { if (dst) std::memcpy(dst, src, sizeof(src)); }

// qmul, qthr, bias by zigzag position, delta by raster index; the chroma entry adds what jpegamd_debug_mfma_offsets gives.
static int32_t mfma_consts(int32_t quality, bool chroma, float *qmul, float *qthr, float *bias, double *delta, float *zoff, float *qadd) {
    return with_mfma_consts(quality, chroma, [&](const MfmaTables &mt, const double (&d)[64]) {
        copy_out(qmul, mt.qmul); copy_out(qthr, mt.qthr); copy_out(bias, mt.bias); copy_out(delta, d);
        copy_out(zoff, mt.zoff); copy_out(qadd, mt.qadd);
    });
}
extern "C" int32_t jpegamd_debug_mfma_consts(int32_t quality, float *qmul, float *qthr, float *bias, double *delta) {
    return mfma_consts(quality, false, qmul, qthr, bias, delta, nullptr, nullptr);
}
extern "C" int32_t jpegamd_debug_chroma_mfma_consts(int32_t quality, float *qmul, float *qthr, float *bias, double *delta, float *zoff,
                                                    float *qadd) {
    return mfma_consts(quality, true, qmul, qthr, bias, delta, zoff, qadd);
}

// What the UNCENTRED matrix operand adds to the quantiser's constants: qadd = bias + zoff by zigzag position, the DC row's
// surplus in accumulator units, the accumulator scale (kMfmaScale).
extern "C" int32_t jpegamd_debug_mfma_offsets(int32_t quality, float *zoff, float *qadd, float *dc_off, float *scale) {
    return with_mfma_consts(quality, false, [&](const MfmaTables &mt, const double (&)[64]) {
        copy_out(zoff, mt.zoff); copy_out(qadd, mt.qadd);
        if (dc_off) *dc_off = mt.dc_off;
        if (scale) *scale = kMfmaScale;
    });
}

static int32_t group_thresholds(int32_t quality, bool chroma, float *grp_thr /*[4 groups][2 lane halves]*/, float *lo_bound /*same shape, may be NULL*/) {
    if (!grp_thr) return JPEGAMD_ERR_ARG;
    return with_mfma_consts(quality, chroma, [&](const MfmaTables &mt, const double (&)[64]) { copy_out(grp_thr, mt.grp_thr); copy_out(lo_bound, mt.lo_bound); });
}
extern "C" int32_t jpegamd_debug_group_thresholds(int32_t quality, float *grp_thr, float *lo_bound) { return group_thresholds(quality, false, grp_thr, lo_bound); }
extern "C" int32_t jpegamd_debug_chroma_group_thresholds(int32_t quality, float *grp_thr, float *lo_bound) { return group_thresholds(quality, true, grp_thr, lo_bound); }

// The same constants for a table of the caller's (raster order, entries 1 .. 255).
static bool table_valid(const uint8_t *t) { return std::find(t, t + 64, (uint8_t)0) == t + 64; }
extern "C" int32_t jpegamd_debug_table_consts(const uint8_t *table, float *qmul, float *qthr, float *bias, double *delta, float *zoff, float *qadd,
                                              float *grp_thr, float *lo_bound) {
    if (!table || !table_valid(table)) return JPEGAMD_ERR_ARG;
    return with_table_consts(table, [&](const MfmaTables &mt, const double (&d)[64]) {
        copy_out(qmul, mt.qmul); copy_out(qthr, mt.qthr); copy_out(bias, mt.bias); copy_out(delta, d);
        copy_out(zoff, mt.zoff); copy_out(qadd, mt.qadd); copy_out(grp_thr, mt.grp_thr); copy_out(lo_bound, mt.lo_bound);
    });
}

extern "C" int32_t jpegamd_quant_tables_for_quality(int32_t quality, uint8_t *luma, uint8_t *chroma) {
    if (luma) quant_table_for_quality(quality, luma);
    if (chroma) chroma_quant_table_for_quality(quality, chroma);
    return JPEGAMD_OK;
}

// The colour subsamplings: 4:4:4, 4:2:0 (chroma halved both ways) and 4:2:2 (halved along the row alone).
static bool sub_valid(int sub) { return sub == JPEGAMD_SUBSAMPLE_444 || sub == JPEGAMD_SUBSAMPLE_420 || sub == JPEGAMD_SUBSAMPLE_422; }
static int chroma_mode(int sub) { return sub == JPEGAMD_SUBSAMPLE_420 ? kChromaMode420 : (sub == JPEGAMD_SUBSAMPLE_422 ? kChromaMode422 : kChromaMode444); }
static size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
// A chroma plane of a w x h picture: cw x ch samples; in scratch its rows lie `pitch` bytes apart, its planes `plane_bytes`.
struct ChromaGeom {
    int cw, ch, pitch;
    size_t plane_bytes;
};
static ChromaGeom chroma_geom(int w, int h, int sub) {
    ChromaGeom c;
    c.cw = sub == JPEGAMD_SUBSAMPLE_444 ? w : (w + 1) / 2;
    c.ch = sub == JPEGAMD_SUBSAMPLE_420 ? (h + 1) / 2 : h;
    c.pitch = (int)(((int64_t)c.cw + 3) / 4 * 4);      // (64-bit: the size bounds take any positive width)
    c.plane_bytes = round_up((size_t)c.pitch * (size_t)c.ch, 256);
    return c;
}
static bool is_packed422(int layout) { return layout == JPEGAMD_CHROMA_YUYV || layout == JPEGAMD_CHROMA_UYVY; }

// One scan of nb blocks at the worst-case bit count (kMaxBlockBits, or kMaxBlockBitsColor), every byte stuffed, its flush byte.
static uint64_t scan_bound(uint64_t nb, uint64_t block_bits) { return 2 * ((nb * block_bits + 7) / 8 + 1); }
static uint64_t blocks_of(int w, int h) { return (uint64_t)((w + 7) / 8) * (uint64_t)((h + 7) / 8); }

extern "C" uint64_t jpegamd_max_jfif_bytes_color(int32_t width, int32_t height, int32_t subsampling) {
    if (width <= 0 || height <= 0 || !sub_valid(subsampling)) return 0;
    const ChromaGeom cg = chroma_geom(width, height, subsampling);
    return kColorPrefixMax + 2 * kSosBytes + 2 + scan_bound(blocks_of(width, height), kMaxBlockBitsColor) +
           2 * scan_bound(blocks_of(cg.cw, cg.ch), kMaxBlockBitsColor) + 16;
}

extern "C" uint64_t jpegamd_max_jfif_bytes(int32_t width, int32_t height) {
    if (width <= 0 || height <= 0) return 0;
    // every block at the worst-case bit count, every byte stuffed, + container
    return JPEGAMD_JFIF_PREFIX_BYTES + 2 + scan_bound(blocks_of(width, height), kMaxBlockBits) + 16;
}

// Allocation failures free everything allocated so far (jpegamd_encoder_destroy tolerates a half-built context).
#define HIP_TRY_CREATE(expr)                                                                    \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess) {                                                                 \
            std::fprintf(stderr, "jpegamd: %s failed: %s (%s:%d)\n", #expr, hipGetErrorString(e_), \
                         __FILE__, __LINE__);                                                   \
            jpegamd_encoder_destroy(e);                                                         \
            return JPEGAMD_ERR_HIP;                                                             \
        }                                                                                       \
    } while (0)

static CtxLimits context_limits(int max_w, int max_h) {
    CtxLimits l;
    l.max_segs = segs_for(max_w, max_h, nullptr, nullptr, nullptr);
    l.max_tiles = tiles_for(max_w, max_h);
    // (room for either segment length: the same blocks as fewer, longer segments need a little more than as many short ones)
    const size_t w8 = (size_t)l.max_segs * kSegCapWords;
    const size_t w16 = (size_t)segs_for(max_w, max_h, nullptr, nullptr, nullptr, kSegTilesBatch) * seg_cap_words(kSegTilesBatch);
    l.words_cap = (w8 > w16 ? w8 : w16) + seg_cap_words(kSegTilesBatch);
    l.max_wgs = l.max_segs + 2;                                    // (a picture never has more workgroups than segments)
    return l;
}

// The per-segment arrays of `segs` segments whose strings take `words` words in all; `groups`: with the group aggregates
// (k_segment_merge writes them; a path that fills its segments itself has none).
static int32_t alloc_seg_arrays(SegArrays *s, size_t segs, size_t words, bool groups) {
    const size_t n = segs + 16;                                   // k_finalize reads the per-segment arrays four at a time
    HIP_TRY(hipMalloc((void **)&s->words, words * sizeof(uint32_t)));
    s->words_stride = kSegCapWords;
    HIP_TRY(hipMalloc((void **)&s->bits, n * sizeof(uint32_t)));
    HIP_TRY(hipMalloc((void **)&s->syms, n * sizeof(uint32_t)));
    HIP_TRY(hipMalloc((void **)&s->exact, n * sizeof(uint32_t)));
    HIP_TRY(hipMalloc((void **)&s->edge, n * sizeof(uint32_t)));
    HIP_TRY(hipMalloc((void **)&s->ffin, n * 8 * sizeof(uint16_t)));
    if (groups) {
        HIP_TRY(hipMalloc((void **)&s->grp_bits, (n / kSegGroup + 2) * sizeof(uint32_t)));
        HIP_TRY(hipMalloc((void **)&s->grp_ff, (n / kSegGroup + 2) * 8 * sizeof(uint32_t)));
    }
    return JPEGAMD_OK;
}
static void free_seg_arrays(SegArrays *s) {
    hipFree(s->words); hipFree(s->bits); hipFree(s->syms); hipFree(s->exact); hipFree(s->edge); hipFree(s->ffin); hipFree(s->grp_bits); hipFree(s->grp_ff);
    *s = SegArrays{};
}

// Every event of the profiling ring.
static void destroy_ring_events(JpegAmdEncoder *e) {
    for (auto &set : e->ring) { for (auto &ev : set.ev) if (ev) hipEventDestroy(ev); for (auto &ev : set.cev) if (ev) hipEventDestroy(ev); }
}

extern "C" int32_t jpegamd_encoder_create(JpegAmdEncoder **out, int32_t max_width, int32_t max_height) {
    // (an image is at most 65535 rows -- describe() checks that; a context may reserve room for a batch of them)
    if (!out || max_width <= 0 || max_height <= 0 || max_width > 65535 || max_height > 65535 * kMaxBatch) return JPEGAMD_ERR_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        std::fprintf(stderr, "jpegamd: no HIP device available (this library has no CPU path)\n");
        return JPEGAMD_ERR_NO_DEVICE;
    }
    JpegAmdEncoder *e = new (std::nothrow) JpegAmdEncoder();
    if (!e) return JPEGAMD_ERR_HIP;
    std::memset(&e->mirror, 0, sizeof(e->mirror));
    e->tables_host = new (std::nothrow) MfmaTables;
    if (!e->tables_host) { delete e; return JPEGAMD_ERR_HIP; }
    HIP_TRY_CREATE(hipGetDevice(&e->device));
    e->max_w = max_width; e->max_h = max_height;
    e->lim = context_limits(max_width, max_height);
    if (alloc_seg_arrays(&e->seg, (size_t)e->lim.max_segs, e->lim.words_cap, true)) { jpegamd_encoder_destroy(e); return JPEGAMD_ERR_HIP; }
    HIP_TRY_CREATE(hipMalloc((void **)&e->huff, 272 * sizeof(uint32_t)));
    HIP_TRY_CREATE(hipMalloc((void **)&e->prefix, 512));
    HIP_TRY_CREATE(hipMalloc((void **)&e->stats_dev, sizeof(ScanStats)));
    HIP_TRY_CREATE(hipMemset(e->stats_dev, 0, sizeof(ScanStats)));
    HIP_TRY_CREATE(hipMalloc((void **)&e->tables_dev, sizeof(MfmaTables)));
    HIP_TRY_CREATE(hipMalloc((void **)&e->tile_head, ((size_t)e->lim.max_tiles + 1) * kTileHeadWords * sizeof(uint32_t)));
    HIP_TRY_CREATE(hipMalloc((void **)&e->tile_over, (size_t)e->lim.max_tiles * kTileOverCap * sizeof(uint32_t)));
    HIP_TRY_CREATE(hipMalloc((void **)&e->code_tab, kCodeWords * sizeof(uint32_t)));
    HIP_TRY_CREATE(hipMalloc((void **)&e->tile_ctr, 2 * 64 * 128));      // two sets of ticket-group cache lines, used alternately
    HIP_TRY_CREATE(hipMemset(e->tile_ctr, 0, 2 * 64 * 128));
    HIP_TRY_CREATE(hipMalloc((void **)&e->desc, 12 * (size_t)e->lim.max_wgs * sizeof(uint32_t)));
    HIP_TRY_CREATE(hipMemset(e->desc, 0, 12 * (size_t)e->lim.max_wgs * sizeof(uint32_t)));
    if (std::getenv("JPEGAMD_STAMPS")) {
        const size_t n = stamp_words(e->lim.max_segs) * sizeof(unsigned long long);
        HIP_TRY_CREATE(hipMalloc((void **)&e->stamps_dev, n));
        HIP_TRY_CREATE(hipMemset(e->stamps_dev, 0, n));
    }
    uint32_t words[272];
    build_huffman_words(words);
    HIP_TRY_CREATE(hipMemcpy(e->huff, words, sizeof(words), hipMemcpyHostToDevice));
    {
        std::vector<uint32_t> ct(kCodeWords);
        build_code_table(ct.data());
        HIP_TRY_CREATE(hipMemcpy(e->code_tab, ct.data(), kCodeWords * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    *out = e;
    return JPEGAMD_OK;
}

extern "C" int32_t jpegamd_encoder_destroy(JpegAmdEncoder *e) {
    if (!e) return JPEGAMD_OK;
    if (e->pending) hipStreamSynchronize(e->last_stream);
    free_seg_arrays(&e->seg);
    hipFree(e->huff); hipFree(e->prefix); hipFree(e->stats_dev); hipFree(e->tables_dev);
    hipFree(e->tile_head); hipFree(e->tile_over); hipFree(e->code_tab); hipFree(e->tile_ctr); hipFree(e->desc); hipFree(e->stamps_dev);
    hipFree(e->meta_dev);
    hipFree(e->color.tables_dev); hipFree(e->color.code_tab); hipFree(e->color.huff); hipFree(e->color.hdr); hipFree(e->color.scan_size);
    hipFree(e->color.scan_stats); hipFree(e->color.planes); hipFree(e->color.scans);
    hipFree(e->color.bmeta); hipFree(e->color.bplanes); hipFree(e->color.bscans);
    hipFree(e->mcu.coef); hipFree(e->mcu.hdr); hipFree(e->mcu.scan_stats);
    hipFree(e->mcu.rst_words); hipFree(e->mcu.rst_pos); hipFree(e->mcu.rst_pic_sums);
    hipFree(e->mcu.pmeta); hipFree(e->mcu.pslots);
    hipFree(e->mcu.pcounts); hipFree(e->mcu.pres); hipFree(e->mcu.ptabs); hipFree(e->mcu.phdr); hipFree(e->mcu.phdr_len);
    hipFree(e->mcu.hcounts); hipFree(e->mcu.htabs); hipFree(e->mcu.hprefix); hipFree(e->mcu.hprefix_len); hipFree(e->mcu.hres);
    free_seg_arrays(&e->mcu.seg);
    destroy_ring_events(e);
    delete e->tables_host;
    delete e;
    return JPEGAMD_OK;
}

extern "C" int32_t jpegamd_encoder_set_pipeline(JpegAmdEncoder *e, int32_t pipeline) {
    if (!e || pipeline < JPEGAMD_PIPELINE_AUTO || pipeline > JPEGAMD_PIPELINE_STITCH) return JPEGAMD_ERR_ARG;
    e->pipeline = pipeline;
    return JPEGAMD_OK;
}

extern "C" int32_t jpegamd_encoder_set_huffman(JpegAmdEncoder *e, int32_t huffman) {
    if (!e || (huffman != JPEGAMD_HUFFMAN_STANDARD && huffman != JPEGAMD_HUFFMAN_OPTIMIZED)) return JPEGAMD_ERR_ARG;
    e->huffman = huffman;
    return JPEGAMD_OK;
}

// Host state only: the next encode finds a key its caches do not hold and uploads constants and headers behind the queued work.
extern "C" int32_t jpegamd_encoder_set_quant_tables(JpegAmdEncoder *e, const uint8_t *luma, const uint8_t *chroma) {
    if (!e || (!luma && chroma)) return JPEGAMD_ERR_ARG;
    if (!luma) { e->custom_tables = false; return JPEGAMD_OK; }
    if (!chroma) chroma = luma;
    if (!table_valid(luma) || !table_valid(chroma)) return JPEGAMD_ERR_ARG;
    std::memmove(e->custom_luma, luma, 64);
    std::memmove(e->custom_chroma, chroma, 64);
    e->custom_tables = true;
    e->table_key = e->table_key == INT32_MAX ? kFirstTableKey : e->table_key + 1;
    return JPEGAMD_OK;
}

extern "C" int32_t jpegamd_encoder_get_quant_tables(JpegAmdEncoder *e, uint8_t *luma, uint8_t *chroma, int32_t *custom) {
    if (!e || !custom) return JPEGAMD_ERR_ARG;
    *custom = e->custom_tables ? 1 : 0;
    if (!e->custom_tables) return JPEGAMD_OK;
    if (luma) std::memcpy(luma, e->custom_luma, 64);
    if (chroma) std::memcpy(chroma, e->custom_chroma, 64);
    return JPEGAMD_OK;
}

// Host state only, as the tables above: the next encode uploads.  The description is turned into its bytes here, which is the copy.
static uint64_t metadata_bytes(const JpegAmdEncoder *e) { return e->meta.empty() ? 0 : e->meta.size() - kJfifHeadBytes - kMetaSrcPad; }
extern "C" int32_t jpegamd_encoder_set_metadata(JpegAmdEncoder *e, const JpegAmdMetadata *m) {
    if (!e) return JPEGAMD_ERR_ARG;
    if (!m) { e->meta.clear(); return JPEGAMD_OK; }
    const int64_t n = jpegamd_build_metadata(m, nullptr, 0, nullptr);
    if (n < 0) return (int32_t)n;
    std::vector<uint8_t> bytes;
    try { bytes.assign((size_t)kJfifHeadBytes + (size_t)n + kMetaSrcPad, 0); } catch (const std::bad_alloc &) { return JPEGAMD_ERR_HIP; }
    jpegamd_build_metadata(m, bytes.data() + kJfifHeadBytes, (uint64_t)n, bytes.data());
    if (n == 0 && m->density_units < 0) bytes.clear();              // a description that sets nothing: today's files, today's launches
    e->meta.swap(bytes);
    e->meta_dirty = true;
    return JPEGAMD_OK;
}

extern "C" int64_t jpegamd_encoder_metadata_bytes(JpegAmdEncoder *e) { return e ? (int64_t)metadata_bytes(e) : JPEGAMD_ERR_ARG; }

extern "C" int32_t jpegamd_encoder_set_profiling(JpegAmdEncoder *e, int32_t slots) {
    if (!e || slots < 0 || slots > 65536) return JPEGAMD_ERR_ARG;
    if (e->pending) HIP_TRY(hipStreamSynchronize(e->last_stream));
    destroy_ring_events(e);
    e->ring.clear();
    e->ring.resize((size_t)slots);
    for (auto &set : e->ring) { set.merged = false; for (auto &ev : set.ev) HIP_TRY(hipEventCreate(&ev)); }
    e->calls = 0;
    e->last_slot = -1;
    return JPEGAMD_OK;
}

// The time between two recorded events, in nanoseconds.
static int32_t elapsed_ns(hipEvent_t begin, hipEvent_t end, uint64_t *ns) {
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, begin, end));
    *ns = (uint64_t)((double)ms * 1e6);
    return JPEGAMD_OK;
}

static int32_t read_color_slot(JpegAmdEncoder *e, int slot, uint64_t ns[11]) {
    const auto &set = e->ring[(size_t)slot];
    const hipEvent_t *cev = set.cev.data();
    for (int i = 0; i < 11; ++i) ns[i] = 0;
    if (int32_t rc = elapsed_ns(cev[0], cev[1], &ns[0])) return rc;
    for (int c = 0; c < 3; ++c) {
        const int b = 2 + 6 * c;
        if (int32_t rc = elapsed_ns(cev[b], cev[b + 1], &ns[1 + 3 * c])) return rc;
        if (set.cmerged[c]) {
            if (int32_t rc = elapsed_ns(cev[b + 2], cev[b + 3], &ns[2 + 3 * c])) return rc;
        }
        if (int32_t rc = elapsed_ns(cev[b + 4], cev[b + 5], &ns[3 + 3 * c])) return rc;
    }
    return elapsed_ns(cev[20], cev[21], &ns[10]);
}

static int32_t read_slot(JpegAmdEncoder *e, int slot, JpegAmdStats *stats) {
    if (slot < 0 || (size_t)slot >= e->ring.size()) return JPEGAMD_ERR_ARG;
    const auto &set = e->ring[(size_t)slot];
    if (set.color && set.cbatch)                  // a colour batch: the whole call only
        return elapsed_ns(set.cev[0], set.cev[21], &stats->ns_total);
    if (set.color) {                              // sums over the three scans; the planes count as transform, the append as pack
        uint64_t ns[11];
        if (int32_t rc = read_color_slot(e, slot, ns)) return rc;
        stats->ns_transform = ns[0] + ns[1] + ns[4] + ns[7];
        stats->ns_entropy = ns[2] + ns[5] + ns[8];
        stats->ns_pack = ns[3] + ns[6] + ns[9] + ns[10];
        return elapsed_ns(set.cev[0], set.cev[21], &stats->ns_total);
    }
    const hipEvent_t *ev = set.ev;
    if (int32_t rc = elapsed_ns(ev[0], ev[1], &stats->ns_transform)) return rc;
    stats->ns_entropy = 0;                                     // (whole images: there is no separate merge kernel)
    if (set.merged) {
        if (int32_t rc = elapsed_ns(ev[2], ev[3], &stats->ns_entropy)) return rc;
    }
    if (int32_t rc = elapsed_ns(ev[4], ev[5], &stats->ns_pack)) return rc;
    return elapsed_ns(ev[0], ev[5], &stats->ns_total);         // first begin .. last end: includes the launch gaps
}

extern "C" int32_t jpegamd_debug_color_profile(JpegAmdEncoder *e, int32_t slot, uint64_t *ns) {
    if (!e || !ns || slot < 0 || (size_t)slot >= e->ring.size() || !e->ring[(size_t)slot].color || e->ring[(size_t)slot].cbatch)
        return JPEGAMD_ERR_ARG;
    return read_color_slot(e, slot, ns);
}

extern "C" int32_t jpegamd_encoder_profile(JpegAmdEncoder *e, int32_t slot, JpegAmdStats *stats) {
    if (!e || !stats) return JPEGAMD_ERR_ARG;
    std::memset(stats, 0, sizeof(*stats));
    return read_slot(e, slot, stats);
}

// Context memory that queued work may still read is rewritten from the host only behind that work.
static int32_t wait_pending(JpegAmdEncoder *e) {
    if (e->pending) HIP_TRY(hipStreamSynchronize(e->last_stream));
    return JPEGAMD_OK;
}

// The fast path's constants for quantisation table `t` into `dst` (the context's luma or chroma set), staged in tables_host.
static int32_t upload_tables(JpegAmdEncoder *e, const uint8_t t[64], MfmaTables *dst) {
    derive_mfma_tables(t, e->tables_host, nullptr);
    if (int32_t rc = wait_pending(e)) return rc;
    HIP_TRY(hipMemcpy(dst, e->tables_host, sizeof(MfmaTables), hipMemcpyHostToDevice));
    return JPEGAMD_OK;
}

// The quantisation tables of a picture on this context (raster order; either pointer may be null) and the key the caches of
// constants and headers hold them under: the caller's tables while some are set, else those of the picture's quality.
static int quant_choice(const JpegAmdEncoder *e, const JpegAmdImage *img, uint8_t *luma, uint8_t *chroma) {
    if (e->custom_tables) {
        if (luma) std::memcpy(luma, e->custom_luma, 64);
        if (chroma) std::memcpy(chroma, e->custom_chroma, 64);
        return e->table_key;
    }
    const int q = clamp_quality(img->quality);
    if (luma) quant_table_for_quality(q, luma);
    if (chroma) chroma_quant_table_for_quality(q, chroma);
    return q;
}

static int32_t prepare_constants(JpegAmdEncoder *e, const JpegAmdImage *img, bool need_prefix) {
    const int q = quant_choice(e, img, nullptr, nullptr);
    if (q != e->cur_quality) {
        quant_choice(e, img, e->qtable, nullptr);
        if (int32_t rc = upload_tables(e, e->qtable, e->tables_dev)) return rc;
        e->cur_quality = q;
    }
    if (need_prefix && !e->prefix_for.matches(img->width, img->height, q, 0)) {
        uint8_t hdr[JPEGAMD_JFIF_PREFIX_BYTES];
        build_jfif_prefix(img->width, img->height, e->qtable, hdr);
        if (int32_t rc = wait_pending(e)) return rc;
        HIP_TRY(hipMemcpy(e->prefix, hdr, sizeof(hdr), hipMemcpyHostToDevice));
        e->prefix_for.set(img->width, img->height, q, 0, JPEGAMD_JFIF_PREFIX_BYTES);
    }
    return JPEGAMD_OK;
}

// Does a w x h image fit the scratch of `e`?  Every derived count is checked on its own: an image wider than max_w with
// fewer rows can need MORE segments or tiles than max_w x max_h (per-row rounding).
static bool context_fits(const JpegAmdEncoder *e, int w, int h) {
    if (!e || w <= 0 || h <= 0) return false;
    return segs_for(w, h, nullptr, nullptr, nullptr) <= e->lim.max_segs && tiles_for(w, h) <= e->lim.max_tiles;
}

// Layouts beyond the three every entry takes: the 4-byte orders (the four whole-picture encode entries), and the internal order of
// a planar picture (jpegamd_encode_planar_batch_async: `pixels` is its R plane, G and B travel in a PlaneSet).
constexpr int kOrderPlanar = 0x100;
enum Accept { kAcceptBasic = 0, kAcceptPx4 = 1, kAcceptPlanar = 2 };
static bool is_px4(int order) { return order == JPEGAMD_ORDER_RGBA || order == JPEGAMD_ORDER_BGRA; }
static int bytes_per_pixel(int order) {
    return (order == JPEGAMD_ORDER_GRAY || order == kOrderPlanar) ? 1 : (is_px4(order) ? 4 : 3);
}

// ImageDesc::fast_ok, from the OR of every pointer the launch reads and their row stride.  The dword loader wants both on dword
// boundaries; it multiplies the row stride by a 24-bit multiply (and keeps a tile's eight row offsets in 32 bits): wider strides --
// a region of interest inside a huge buffer -- take the clamped byte loader, whose addresses are 64-bit.
static int32_t dword_loader_ok(uintptr_t pointer_bits, int stride) {
    return ((pointer_bits & 3u) == 0 && (stride & 3) == 0 && stride < (1 << 24)) ? 1 : 0;
}

// A launch of ONE picture with d's geometry and stride: its pixels, and whether the dword loader may read them.
static void set_single_picture(ImageDesc *d, const uint8_t *pixels) {
    d->pixels = pixels;
    d->batch = 1;
    for (int i = 0; i < kMaxBatch; ++i) d->batch_pixels[i] = pixels;
    d->fast_ok = dword_loader_ok((uintptr_t)pixels, d->row_stride);
}

static int32_t describe(const JpegAmdEncoder *e, const JpegAmdImage *img, ImageDesc *d, int seg_tiles = kSegTiles, int accept = kAcceptBasic) {
    if (!img || !img->pixels || img->width <= 0 || img->height <= 0 || img->width > 65535 || img->height > 65535)
        return JPEGAMD_ERR_ARG;
    const bool basic = img->channel_order == JPEGAMD_ORDER_BGR || img->channel_order == JPEGAMD_ORDER_RGB || img->channel_order == JPEGAMD_ORDER_GRAY;
    if (!basic && !(accept == kAcceptPx4 && is_px4(img->channel_order)) && !(accept == kAcceptPlanar && img->channel_order == kOrderPlanar))
        return JPEGAMD_ERR_ARG;
    if (img->row_stride < bytes_per_pixel(img->channel_order) * img->width) return JPEGAMD_ERR_ARG;
    d->width = img->width; d->height = img->height; d->row_stride = img->row_stride;
    set_single_picture(d, (const uint8_t *)img->pixels);
    d->bottom_up = img->bottom_up ? 1 : 0;
    d->select = select_luma(img->channel_order == JPEGAMD_ORDER_BGR || img->channel_order == JPEGAMD_ORDER_BGRA);   // the weights follow the STORED byte order
    d->seg_tiles = seg_tiles;
    d->num_segs = segs_for(img->width, img->height, &d->blocks_w, &d->blocks_h, &d->segs_per_row, seg_tiles);
    d->tiles_per_row = (d->blocks_w + kTileBlocks - 1) / kTileBlocks;
    d->num_tiles = d->tiles_per_row * d->blocks_h;
    d->tile_begin = 0; d->tile_end = d->num_tiles;
    d->seg_begin = 0; d->seg_end = d->num_segs;
    const uint64_t tpi = 0x100000000ull / (uint64_t)d->num_tiles;
    d->tpi_magic = tpi > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)tpi;
    if (e && !context_fits(e, img->width, img->height)) return JPEGAMD_ERR_TOO_LARGE;
    return JPEGAMD_OK;
}

// What k_tile_encode reads for this image (a chroma source is set by the colour paths alone).
static TileSource src_of(const JpegAmdImage *img) {
    if (img->channel_order == JPEGAMD_ORDER_GRAY) return {kSrcPlane};
    if (img->channel_order == kOrderPlanar) return {kSrcPlanar};
    return {is_px4(img->channel_order) ? kSrcPx4 : kSrcRgb};
}

// The pictures of a batch as the kernels take them: p[0] the pixels (planar: the R planes), p[1] / p[2] the G / B planes.
struct PlaneSet {
    const uint8_t *p[3][kMaxBatch];
};
// One picture's output buffer and size word, as the arrays the batch functions take.
struct SingleOut {
    void *outs[1];
    uint64_t *sizes[1];
};

// k_tile_encode (+ the fault injection of the tests).
static int launch_transform(JpegAmdEncoder *e, const ImageDesc &im, bool taps, int8_t *ty, int16_t *tzz, uint64_t *tmask,
                            void *stream, hipEvent_t *ev = nullptr /*2: begin/end*/, TileSource src = {}, const PlaneSet *ps = nullptr) {
    TransformOutM to;
    std::memset(&to, 0, sizeof(to));
    to.tables = src.chroma ? e->color.tables_dev : e->tables_dev; to.stamps = e->stamps_dev;
    to.tap_y = ty; to.tap_zz = tzz; to.tap_mask = tmask;
    to.tile_head = e->tile_head; to.tile_over = e->tile_over; to.code_tab = src.chroma ? e->color.code_tab : e->code_tab;
    // Launches on one context are stream-ordered by contract (they share the scratch): launch i draws tickets from set
    // i % 2 and zeroes the other one for launch i + 1.
    to.tile_ctr = e->tile_ctr + (e->ctr_set ? 64 * 32 : 0);
    to.tile_ctr_next = e->tile_ctr + (e->ctr_set ? 0 : 64 * 32);
    const bool stamped = e->stamp_next && e->stamps_dev && !taps;
    e->stamp_next = false;
    TilePlanes tp;
    if (src.layout == kSrcPlanar) {
        if (!ps) return (int)hipErrorInvalidValue;
        std::memcpy(tp.g, ps->p[1], sizeof(tp.g));
        std::memcpy(tp.b, ps->p[2], sizeof(tp.b));
    }
    const TilePlanes *planes = src.layout == kSrcPlanar ? &tp : nullptr;
    if (int err = stamped ? launch_tile_transform_stamped(im, to, taps, stream, ev ? (void *const *)ev : nullptr, src, planes)
                          : launch_tile_transform(im, to, taps, stream, (ev && !taps) ? (void *const *)ev : nullptr, src, planes)) return err;
    if (im.tile_end > im.tile_begin) e->ctr_set ^= 1;      // (an empty range launches nothing)
    if (e->poison_tile >= 0) {                             // fault injection for the tests: a corrupt record must end in a status code
        if (e->poison_tile < e->lim.max_tiles &&
            hipMemsetD32Async((hipDeviceptr_t)(e->tile_head + (size_t)e->poison_tile * kTileHeadWords), (int)e->poison_value, 1, (hipStream_t)stream) != hipSuccess)
            return (int)hipErrorUnknown;
        e->poison_tile = -1;
    }
    return 0;
}

// k_tile_encode, then k_segment_merge (block-row shards, stage taps).
static int launch_transform_and_entropy(JpegAmdEncoder *e, const ImageDesc &im, bool taps, int8_t *ty, int16_t *tzz, uint64_t *tmask,
                                        void *stream, hipEvent_t *ev = nullptr /*4: begin/end of the two kernels*/, TileSource src = {},
                                        const PlaneSet *ps = nullptr) {
    if (int err = launch_transform(e, im, taps, ty, tzz, tmask, stream, ev, src, ps)) return err;
    MergeArgs ea;
    std::memset(&ea, 0, sizeof(ea));
    ea.tile_head = e->tile_head; ea.tile_over = e->tile_over;
    ea.huff = src.chroma ? e->color.huff : e->huff; ea.num_segs = im.num_segs; ea.segs_per_row = im.segs_per_row; ea.tiles_per_row = im.tiles_per_row;
    ea.seg_tiles = im.seg_tiles;
    ea.seg_begin = im.seg_begin; ea.seg_end = im.seg_end;
    ea.tiles_per_image = im.batch > 1 ? im.num_tiles : 0;
    ea.seg = e->seg;
    ea.seg.words_stride = (uint32_t)seg_cap_words(im.seg_tiles);       // (the stride follows the launch's segment length: carried in the arguments, the context keeps none)
    ea.status = &e->stats_dev->status;
    return launch_segment_merge(ea, stream, ev ? (void *const *)(ev + 2) : nullptr);
}

// Where a scan of a colour file goes: its own header bytes in front, EOI or not, its own statistics record.
struct ScanTarget {
    const uint8_t *prefix;
    int32_t prefix_len, write_eoi;
    ScanStats *stats;
    bool chroma;
    const SegArrays *seg = nullptr;     // the segments k_finalize reads when they are not the context's own (an interleaved-MCU scan)
};

// k_finalize over the segments k_segment_merge (or an import) left: `batch` pictures.  `use_groups`: the group aggregates are valid
// -- whole pictures merged on this context whose segments fill whole groups, so that every picture starts on a group boundary;
// segments imported from other ranks have none.
static int run_finalize(JpegAmdEncoder *e, const ImageDesc &im, void *const *outs_dev, uint64_t out_capacity, uint64_t *const *out_sizes_dev,
                        int32_t with_container, hipStream_t stream, hipEvent_t *ev, int batch, bool use_groups, const ScanTarget *tgt = nullptr) {
    FinalizeArgs fa;
    std::memset(&fa, 0, sizeof(fa));
    fa.seg = (tgt && tgt->seg) ? *tgt->seg : e->seg;
    fa.seg.words_stride = (uint32_t)seg_cap_words(im.seg_tiles);
    fa.num_segs = im.num_segs; fa.num_chunks = finalize_chunks(im.num_segs);
    fa.batch = batch;
    fa.use_groups = use_groups ? 1 : 0;
    for (int i = 0; i < batch; ++i) { fa.out[i] = (uint8_t *)outs_dev[i]; fa.out_size[i] = out_sizes_dev[i]; }
    fa.out_capacity = out_capacity; fa.stats = e->stats_dev;
    fa.prefix = e->prefix; fa.prefix_len = with_container ? JPEGAMD_JFIF_PREFIX_BYTES : 0;
    fa.write_eoi = with_container ? 1 : 0;
    if (tgt) { fa.prefix = tgt->prefix; fa.prefix_len = tgt->prefix_len; fa.write_eoi = tgt->write_eoi; fa.stats = tgt->stats; }
    return launch_finalize(fa, stream, (void *const *)ev);
}

// Which pipeline codes a launch of whole pictures (jpegamd_encoder_set_pipeline): the pair k_segment_merge + k_finalize -- faster
// up to 8192^2-class pictures and on dense content (profiles/r04_notes_experiments.txt) -- or the single-pass k_stitch, whose
// look-back reads at most 256 predecessors per round where k_finalize's scan reads every predecessor of every workgroup.
constexpr int kStitchAutoSegs = 16384;      // 8-tile segments of ONE picture from which AUTO takes k_stitch (a 16384^2 picture)
static bool use_stitch_for(int pipeline, int w, int h) {
    if (pipeline == JPEGAMD_PIPELINE_PAIR) return false;
    if (pipeline == JPEGAMD_PIPELINE_STITCH) return true;
    return segs_for(w, h, nullptr, nullptr, nullptr) >= kStitchAutoSegs;
}
static bool use_stitch(const JpegAmdEncoder *e, int w, int h) { return use_stitch_for(e->pipeline, w, h); }

// k_stitch over the tiles k_tile_encode left: whole images, one or a batch.
static int run_stitch(JpegAmdEncoder *e, const ImageDesc &im, void *const *outs_dev, uint64_t out_capacity,
                      uint64_t *const *out_sizes_dev, int32_t with_container, hipStream_t stream, hipEvent_t *ev = nullptr,
                      const ScanTarget *tgt = nullptr) {
    StitchArgs sa;
    std::memset(&sa, 0, sizeof(sa));
    sa.tile_head = e->tile_head; sa.tile_over = e->tile_over; sa.huff = (tgt && tgt->chroma) ? e->color.huff : e->huff;
    sa.num_segs = im.num_segs; sa.segs_per_row = im.segs_per_row; sa.tiles_per_row = im.tiles_per_row;
    sa.seg_tiles = im.seg_tiles; sa.tiles_per_image = im.num_tiles;
    sa.batch = im.batch; sa.wgs_per_image = stitch_workgroups(im.num_segs);
    if ((int64_t)sa.batch * sa.wgs_per_image > e->lim.max_wgs) return (int)hipErrorInvalidValue;
    // a fresh epoch per launch: granules of older launches never match (no zeroing between launches); the arrays are cleared
    // when the 14-bit tag wraps
    if (e->epoch >= 16383u) {
        if (hipMemsetAsync(e->desc, 0, 12 * (size_t)e->lim.max_wgs * sizeof(uint32_t), stream) != hipSuccess) return (int)hipErrorUnknown;
        e->epoch = 0;
    }
    sa.epoch = ++e->epoch;
    sa.desc = e->desc; sa.desc_ffx = e->desc + 4 * (size_t)e->lim.max_wgs;
    sa.seg_syms = e->seg.syms; sa.seg_exact = e->seg.exact;
    for (int i = 0; i < im.batch; ++i) { sa.out[i] = (uint8_t *)outs_dev[i]; sa.out_size[i] = out_sizes_dev[i]; }
    sa.out_capacity = out_capacity; sa.stats = e->stats_dev; sa.status = &e->stats_dev->status;
    sa.prefix = e->prefix; sa.prefix_len = with_container ? JPEGAMD_JFIF_PREFIX_BYTES : 0;
    sa.write_eoi = with_container ? 1 : 0;
    if (tgt) {
        sa.prefix = tgt->prefix; sa.prefix_len = tgt->prefix_len; sa.write_eoi = tgt->write_eoi;
        sa.stats = tgt->stats; sa.status = &tgt->stats->status;
    }
    return launch_stitch(sa, stream, (void *const *)ev);
}

// "Code the tiles of this ImageDesc": k_tile_encode, [k_picture_stats over its records,] then k_stitch, or k_segment_merge +
// k_finalize.  `ev`: begin / end of the first two kernels (4, or null), `ev_out`: of k_stitch or k_finalize (2, or null).
// `tgt` (a scan of a colour file): its own header bytes, EOI and statistics record instead of the grayscale container.
static int code_tiles(JpegAmdEncoder *e, const ImageDesc &im, TileSource src, const PlaneSet *ps, const PictureStatsArgs *pstats,
                      void *const *outs_dev, uint64_t out_capacity, uint64_t *const *out_sizes_dev, int32_t with_container,
                      const ScanTarget *tgt, bool stitch, hipStream_t stream, hipEvent_t *ev, hipEvent_t *ev_out) {
    if (int err = stitch ? launch_transform(e, im, false, nullptr, nullptr, nullptr, stream, ev, src, ps)
                         : launch_transform_and_entropy(e, im, false, nullptr, nullptr, nullptr, stream, ev, src, ps)) return err;
    if (pstats) if (int err = launch_picture_stats(*pstats, stream)) return err;
    return stitch ? run_stitch(e, im, outs_dev, out_capacity, out_sizes_dev, with_container, stream, ev_out, tgt)
                  : run_finalize(e, im, outs_dev, out_capacity, out_sizes_dev, with_container, stream, ev_out, im.batch, im.num_segs % kSegGroup == 0, tgt);
}

// The next slot of the profiling ring for this call: *ev its events -- a gray call's six, or a colour call's 22 (made on the slot's
// first colour call) -- or null when profiling is off.  `flag`: a gray call has a k_segment_merge; a colour call is a batch.
static int32_t claim_slot(JpegAmdEncoder *e, bool color, bool flag, hipEvent_t **ev) {
    *ev = nullptr;
    if (e->ring.empty()) return JPEGAMD_OK;
    e->last_slot = (int)(e->calls % e->ring.size());
    auto &set = e->ring[(size_t)e->last_slot];
    if (color && set.cev.empty()) {
        set.cev.assign(22, nullptr);
        for (auto &v : set.cev) HIP_TRY(hipEventCreate(&v));
    }
    set.color = color;
    (color ? set.cbatch : set.merged) = flag;
    *ev = color ? set.cev.data() : set.ev;
    ++e->calls;
    return JPEGAMD_OK;
}

// The bookkeeping behind every enqueued call: what jpegamd_encoder_finish waits for and reads.  segs < 0: the count stays.
static int32_t enqueued(JpegAmdEncoder *e, hipStream_t stream, int segs, bool timed = false, bool color = false) {
    if (segs >= 0) e->last_segs = segs;
    e->last_stream = stream;
    e->pending = true;
    e->timed = timed;
    e->last_color = color;      // a colour call summed its statistics already (k_append_scans)
    return JPEGAMD_OK;
}

// Grow-only scratch: *p holds *cap units of `unit` bytes; a call that needs more gets a new buffer of exactly `need` units, behind
// whatever queued work may still use the old one.  The contents are not kept.
template <class T>
static int32_t grow_scratch(JpegAmdEncoder *e, T **p, size_t *cap, size_t need, size_t unit = sizeof(T)) {
    if (need <= *cap) return JPEGAMD_OK;
    if (int32_t rc = wait_pending(e)) return rc;
    hipFree(*p); *p = nullptr; *cap = 0;
    HIP_TRY(hipMalloc((void **)p, need * unit));
    *cap = need;
    return JPEGAMD_OK;
}

// Metadata around the launches of one call: `run(outs, capacity)` is an entry's whole launch sequence.  Nothing
// set: exactly that.  Otherwise the sequence runs M bytes further into every buffer with M bytes less capacity -- a capacity of at
// most M counts as 0, and the pointers then stay where they are: nothing is written either way -- and k_metadata_place, once per call
// behind the last launch, puts the 20 leading bytes and the blob in front and adds M to the sizes.  A profiled call's time runs to the end
// of that kernel: the slot's last event takes its end stamp, or -- `end_recorded`: the entry records that event on the stream -- is
// recorded again behind it.
template <class Run>
static int32_t with_metadata(JpegAmdEncoder *e, int32_t count, void *const *outs_dev, uint64_t out_capacity, uint64_t *const *out_sizes_dev,
                             void *stream, bool end_recorded, Run run) {
    if (e->meta.empty()) return run(outs_dev, out_capacity);
    const uint64_t m = metadata_bytes(e);
    if (e->meta_dirty) {                                               // the context's copy, behind whatever queued work still reads the old one
        if (int32_t rc = grow_scratch(e, &e->meta_dev, &e->meta_cap, e->meta.size())) return rc;
        if (int32_t rc = wait_pending(e)) return rc;
        HIP_TRY(hipMemcpy(e->meta_dev, e->meta.data(), e->meta.size(), hipMemcpyHostToDevice));
        e->meta_dirty = false;
    }
    const uint64_t cap = out_capacity > m ? out_capacity - m : 0;
    void *outs[kMaxBatch];
    for (int i = 0; i < count; ++i) outs[i] = cap ? (uint8_t *)outs_dev[i] + m : outs_dev[i];
    if (int32_t rc = run(outs, cap)) return rc;
    MetadataPlaceArgs pa;
    std::memset(&pa, 0, sizeof(pa));
    for (int i = 0; i < count; ++i) { pa.out[i] = (uint8_t *)outs_dev[i]; pa.out_size[i] = out_sizes_dev[i]; }
    pa.out_capacity = out_capacity;
    pa.src = e->meta_dev; pa.bytes = kJfifHeadBytes + m; pa.batch = count; pa.stats = e->stats_dev;
    hipEvent_t end = nullptr;
    if (e->timed && e->last_slot >= 0) {
        const auto &set = e->ring[(size_t)e->last_slot];
        end = set.color ? set.cev[21] : set.ev[5];
    }
    if (launch_metadata_place(pa, stream, end_recorded ? nullptr : end)) return JPEGAMD_ERR_HIP;
    if (end && end_recorded) HIP_TRY(hipEventRecord(end, (hipStream_t)stream));
    return JPEGAMD_OK;
}

// ---------------------------------------------------------------------------------------------------------
// One image sharded over several GPUs by block rows.  Each rank transforms and entropy-codes its rows
// (jpegamd_encode_rows_async: the unstuffed per-segment bit strings stay in its scratch), exports them densely
// (jpegamd_export_segments), the root imports every rank's segments at their global indices
// (jpegamd_import_segments) and runs the ordinary finalize over all of them (jpegamd_finalize_async): bit offsets,
// 0xFF stuffing and the zero-padded flush depend on the global byte phase and so happen once, at the root.
// ---------------------------------------------------------------------------------------------------------
static int32_t shard_desc(JpegAmdEncoder *e, const JpegAmdImage *img, int32_t by0, int32_t by1, ImageDesc *im) {
    if (!e || !e->meta.empty()) return JPEGAMD_ERR_ARG;            // (the sharded entries write no metadata: refused, not dropped)
    int32_t rc = describe(e, img, im);
    if (rc) return rc;
    if (by0 < 0 || by1 < by0 || by1 > im->blocks_h) return JPEGAMD_ERR_ARG;
    return JPEGAMD_OK;
}

extern "C" int32_t jpegamd_encode_rows_async(JpegAmdEncoder *e, const JpegAmdImage *img, int32_t block_row_begin,
                                             int32_t block_row_end, void *stream_) {
    ImageDesc im;
    int32_t rc = shard_desc(e, img, block_row_begin, block_row_end, &im);
    if (rc) return rc;
    rc = prepare_constants(e, img, false);
    if (rc) return rc;
    // the DC predictor of the shard's first block is the last block of the row above (rle.c:59-70 chains across rows):
    // that ONE tile is transformed here too (its quantised DC does not depend on anything before it), not coded
    im.tile_begin = block_row_begin * im.tiles_per_row - (block_row_begin > 0 ? 1 : 0);
    im.tile_end = block_row_end * im.tiles_per_row;
    im.seg_begin = block_row_begin * im.segs_per_row;
    im.seg_end = block_row_end * im.segs_per_row;
    hipStream_t stream = (hipStream_t)stream_;
    if (launch_transform_and_entropy(e, im, false, nullptr, nullptr, nullptr, stream, nullptr, src_of(img))) return JPEGAMD_ERR_HIP;
    return enqueued(e, stream, im.num_segs);
}

static int32_t exchange_args(JpegAmdEncoder *e, const JpegAmdImage *img, int32_t by0, int32_t by1, uint32_t *dense, uint64_t cap,
                             uint32_t *meta, uint32_t *total, SegExchange *x) {
    ImageDesc im;
    int32_t rc = shard_desc(e, img, by0, by1, &im);
    if (rc) return rc;
    if (!dense || !meta) return JPEGAMD_ERR_ARG;
    std::memset(x, 0, sizeof(*x));
    x->seg = e->seg;
    x->seg.words_stride = (uint32_t)kSegCapWords;           // (the sharded path uses the standard segment length)
    x->s0 = by0 * im.segs_per_row; x->s1 = by1 * im.segs_per_row;
    x->dense = dense; x->dense_cap_words = cap; x->meta = meta; x->total_words = total;
    x->status = &e->stats_dev->status;
    return JPEGAMD_OK;
}

extern "C" int32_t jpegamd_export_segments(JpegAmdEncoder *e, const JpegAmdImage *img, int32_t block_row_begin, int32_t block_row_end,
                                           uint32_t *dense_words_dev, uint64_t dense_capacity_words, uint32_t *meta_dev,
                                           uint32_t *total_words_dev, void *stream) {
    SegExchange x;
    if (!total_words_dev) return JPEGAMD_ERR_ARG;
    int32_t rc = exchange_args(e, img, block_row_begin, block_row_end, dense_words_dev, dense_capacity_words, meta_dev, total_words_dev, &x);
    if (rc) return rc;
    if (launch_seg_export(x, stream)) return JPEGAMD_ERR_HIP;
    return enqueued(e, (hipStream_t)stream, -1);
}

extern "C" int32_t jpegamd_import_segments(JpegAmdEncoder *e, const JpegAmdImage *img, int32_t block_row_begin, int32_t block_row_end,
                                           const uint32_t *dense_words_dev, const uint32_t *meta_dev, void *stream) {
    SegExchange x;
    int32_t rc = exchange_args(e, img, block_row_begin, block_row_end, const_cast<uint32_t *>(dense_words_dev), ~0ull,
                               const_cast<uint32_t *>(meta_dev), nullptr, &x);
    if (rc) return rc;
    if (launch_seg_import(x, stream)) return JPEGAMD_ERR_HIP;
    return enqueued(e, (hipStream_t)stream, -1);
}

extern "C" int32_t jpegamd_finalize_async(JpegAmdEncoder *e, const JpegAmdImage *img, void *out_dev, uint64_t out_capacity,
                                          uint64_t *out_size_dev, int32_t with_container, void *stream_) {
    if (!out_dev || !out_size_dev) return JPEGAMD_ERR_ARG;
    ImageDesc im;
    int32_t rc = shard_desc(e, img, 0, 0, &im);
    if (rc) return rc;
    rc = prepare_constants(e, img, with_container != 0);
    if (rc) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const SingleOut one = {{out_dev}, {out_size_dev}};
    if (run_finalize(e, im, one.outs, out_capacity, one.sizes, with_container, stream, nullptr, 1, false)) return JPEGAMD_ERR_HIP;
    return enqueued(e, stream, im.num_segs);
}

// The pictures of a batch of JpegAmdImage: every output, size word and pixel pointer set, every picture like the first (which the
// entry has checked: each takes its own layouts) -> their pixels in ps->p[0].  Reads nothing of a context.
static int32_t uniform_batch_args(const JpegAmdImage *imgs, int32_t count, void *const *outs_dev, uint64_t *const *out_sizes_dev, PlaneSet *ps) {
    const JpegAmdImage &g0 = imgs[0];
    *ps = PlaneSet{};
    for (int i = 0; i < count; ++i) {
        const JpegAmdImage &g = imgs[i];
        if (!outs_dev[i] || !out_sizes_dev[i] || !g.pixels) return JPEGAMD_ERR_ARG;
        if (g.width != g0.width || g.height != g0.height || g.row_stride != g0.row_stride || (g.bottom_up != 0) != (g0.bottom_up != 0) ||
            g.channel_order != g0.channel_order || g.quality != g0.quality)
            return JPEGAMD_ERR_ARG;
        ps->p[0][i] = (const uint8_t *)g.pixels;
    }
    return JPEGAMD_OK;
}

// `count` images of one geometry through ONE launch of each kernel (see the header): image i's tiles are
// [i * num_tiles, (i + 1) * num_tiles), its segments [i * num_segs, ..); DC prediction, bit offsets and stuffing restart per image.
// The launch plan of `count` pictures like g0, pixels in ps, coded as ONE batch (a grayscale batch, the Y scans of a colour batch):
// segments of 16 tiles for k_stitch and from four pictures on (jpegamd_internal.h) -- of 8 after all when the context's words do
// not hold the longer ones (a geometry other than its own) -- then whether the whole batch fits the context.
static int32_t plan_batch(const JpegAmdEncoder *e, const JpegAmdImage &g0, const PlaneSet &ps, int32_t count, ImageDesc *im, bool *stitch) {
    const int accept = g0.channel_order == kOrderPlanar ? kAcceptPlanar : kAcceptPx4;
    *stitch = use_stitch(e, g0.width, g0.height);
    int seg_tiles = (*stitch || count >= 4) ? kSegTilesBatch : kSegTiles;
    const auto words = [&]() { return (size_t)count * im->num_segs * seg_cap_words(seg_tiles); };
    if (int32_t rc = describe(e, &g0, im, seg_tiles, accept)) return rc;
    if (!*stitch && seg_tiles != kSegTiles && words() > e->lim.words_cap) {
        seg_tiles = kSegTiles;
        if (int32_t rc = describe(e, &g0, im, seg_tiles, accept)) return rc;
    }
    if ((int64_t)count * im->num_tiles > e->lim.max_tiles || (int64_t)count * im->num_segs > e->lim.max_segs || (!*stitch && words() > e->lim.words_cap))
        return JPEGAMD_ERR_TOO_LARGE;
    for (int i = 0; i < count; ++i) im->batch_pixels[i] = ps.p[0][i];
    uintptr_t pointer_bits = 0;                                        // every pointer of every picture (planar: of all three planes)
    for (int k = 0; k < (g0.channel_order == kOrderPlanar ? 3 : 1); ++k)
        for (int i = 0; i < count; ++i) pointer_bits |= (uintptr_t)ps.p[k][i];
    im->fast_ok = dword_loader_ok(pointer_bits, g0.row_stride);
    im->batch = count;
    im->tile_end = count * im->num_tiles;
    im->seg_end = count * im->num_segs;
    return JPEGAMD_OK;
}

// A batch of float pictures (jpegamd_encode_float_batch_async and its twins): what k_float_planes_batch reads.  The launches behind
// that pass read the planes it leaves in color.bplanes.
// `reduce` (jpegamd_encode_reduced_batch_async and its twins): BYTES instead, src_width x src_height of them per channel, which
// k_reduce_planes_batch averages in reduce x reduce boxes; the geometry of every launch behind the pass is the reduced picture's.
struct FloatSource {
    const uint8_t *plane[3][kMaxBatch]; // R, G, B; one channel: plane[0] alone
    int32_t channels, type, row_stride, pixel_stride;      // 1 or 3; JPEGAMD_FLOAT_*; bytes
    float scale, offset;
    int32_t reduce, src_width, src_height;                 // 0: float samples
    int32_t resize, out_width, out_height;                 // resize: BYTES again, which k_resize_planes_batch resamples to out_width x
                                                           // out_height by exact area means (jpegamd_encode_resized_batch_async)
};
static int launch_float_luma_pass(JpegAmdEncoder *e, const FloatSource &fl, const JpegAmdImage &gy, int32_t count, hipStream_t stream,
                                  void *const *ev);

// The grayscale files of a batch whose arguments are known to be good: g0 describes every picture, ps holds their pixels.
// `fl` (a float batch): g0 / ps are the Y planes in color.bplanes, which the caller has sized and k_float_planes_batch fills first.
static int32_t gray_batch_run(JpegAmdEncoder *e, const JpegAmdImage &g0, const PlaneSet &ps, int32_t count, void *const *outs_dev,
                              uint64_t out_capacity, uint64_t *const *out_sizes_dev, int32_t with_container, void *stream_,
                              const FloatSource *fl = nullptr) {
    ImageDesc im;
    bool stitch;
    int32_t rc = plan_batch(e, g0, ps, count, &im, &stitch);
    if (rc) return rc;
    rc = prepare_constants(e, &g0, with_container != 0);
    if (rc) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    hipEvent_t *ev;
    rc = claim_slot(e, false, !stitch, &ev);
    if (rc) return rc;
    hipEvent_t ev_tiles[4] = {ev ? ev[0] : nullptr, ev ? ev[1] : nullptr, ev ? ev[2] : nullptr, ev ? ev[3] : nullptr};
    if (fl) {                                                          // the front pass: ITS begin stamp opens ns_transform and ns_total
        hipEvent_t ev_front[2] = {ev_tiles[0], nullptr};
        if (launch_float_luma_pass(e, *fl, g0, count, stream, ev ? (void *const *)ev_front : nullptr)) return JPEGAMD_ERR_HIP;
        ev_tiles[0] = nullptr;
    }
    if (code_tiles(e, im, src_of(&g0), &ps, nullptr, outs_dev, out_capacity, out_sizes_dev, with_container, nullptr, stitch, stream,
                   ev ? ev_tiles : nullptr, ev ? ev + 4 : nullptr)) return JPEGAMD_ERR_HIP;
    return enqueued(e, stream, count * im.num_segs, ev != nullptr);
}

// ... with the context's metadata in front (a bare scan is no file: refused while metadata is set).
static int32_t gray_batch(JpegAmdEncoder *e, const JpegAmdImage &g0, const PlaneSet &ps, int32_t count, void *const *outs_dev,
                          uint64_t out_capacity, uint64_t *const *out_sizes_dev, int32_t with_container, void *stream_,
                          const FloatSource *fl = nullptr) {
    if (!e->meta.empty() && !with_container) return JPEGAMD_ERR_ARG;
    return with_metadata(e, count, outs_dev, out_capacity, out_sizes_dev, stream_, false, [&](void *const *outs, uint64_t cap) {
        return gray_batch_run(e, g0, ps, count, outs, cap, out_sizes_dev, with_container, stream_, fl);
    });
}

// One picture: the argument checks, then a batch of one.
extern "C" int32_t jpegamd_encode_async(JpegAmdEncoder *e, const JpegAmdImage *img, void *out_dev,
                                        uint64_t out_capacity, uint64_t *out_size_dev, int32_t with_container,
                                        void *stream_) {
    if (!e || !out_dev || !out_size_dev) return JPEGAMD_ERR_ARG;
    ImageDesc im;
    int32_t rc = describe(nullptr, img, &im, kSegTiles, kAcceptPx4);      // (the arguments alone: the context is looked at by gray_batch)
    if (rc) return rc;
    PlaneSet ps = {};
    ps.p[0][0] = (const uint8_t *)img->pixels;
    const SingleOut one = {{out_dev}, {out_size_dev}};
    return gray_batch(e, *img, ps, 1, one.outs, out_capacity, one.sizes, with_container, stream_);
}

extern "C" int32_t jpegamd_encode_batch_async(JpegAmdEncoder *e, const JpegAmdImage *imgs, int32_t count, void *const *outs_dev,
                                              uint64_t out_capacity, uint64_t *const *out_sizes_dev, int32_t with_container,
                                              void *stream_) {
    if (!e || !imgs || !outs_dev || !out_sizes_dev || count < 1 || count > kMaxBatch) return JPEGAMD_ERR_ARG;
    ImageDesc im;
    int32_t rc = describe(nullptr, &imgs[0], &im, kSegTiles, kAcceptPx4);      // (the arguments alone: the context is looked at by gray_batch)
    if (rc) return rc;
    PlaneSet ps;
    rc = uniform_batch_args(imgs, count, outs_dev, out_sizes_dev, &ps);
    if (rc) return rc;
    return gray_batch(e, imgs[0], ps, count, outs_dev, out_capacity, out_sizes_dev, with_container, stream_);
}

// ---------------------------------------------------------------------------------------------------------
// Colour: three non-interleaved scans (colour scans).  k_chroma_planes writes the Cb / Cr planes; Y runs through the
// unchanged RGB path straight into `out` behind the colour prefix; Cb and Cr run through k_tile_encode's one-byte mode with the
// chroma constants into context scratch, each behind its SOS (Cr with EOI); k_append_scans copies them behind the Y scan at
// offsets the device knows.  Everything is stream-ordered: the host never waits between the scans.
// ---------------------------------------------------------------------------------------------------------
static int32_t color_alloc_consts(JpegAmdEncoder *e) {
    auto &c = e->color;
    if (!c.tables_dev) {
        HIP_TRY(hipMalloc((void **)&c.tables_dev, sizeof(MfmaTables)));
        HIP_TRY(hipMalloc((void **)&c.code_tab, kCodeWords * sizeof(uint32_t)));
        HIP_TRY(hipMalloc((void **)&c.huff, 272 * sizeof(uint32_t)));
        HIP_TRY(hipMalloc((void **)&c.hdr, 1024));
        HIP_TRY(hipMalloc((void **)&c.scan_size, 4 * sizeof(uint64_t)));
        HIP_TRY(hipMalloc((void **)&c.scan_stats, 3 * sizeof(ScanStats)));
        uint32_t words[272];
        build_huffman_words_chroma(words);
        HIP_TRY(hipMemcpy(c.huff, words, sizeof(words), hipMemcpyHostToDevice));
        std::vector<uint32_t> ct(kCodeWords);
        build_code_table_chroma(ct.data());
        HIP_TRY(hipMemcpy(c.code_tab, ct.data(), kCodeWords * sizeof(uint32_t), hipMemcpyHostToDevice));
        uint8_t sos[2 * 16] = {};
        color_sos(2, sos);
        color_sos(3, sos + 16);
        HIP_TRY(hipMemcpy(c.hdr + kColorPrefixMax, sos, sizeof(sos), hipMemcpyHostToDevice));
    }
    return JPEGAMD_OK;
}

static int32_t color_alloc(JpegAmdEncoder *e, int w, int h) {
    auto &c = e->color;
    if (int32_t rc = color_alloc_consts(e)) return rc;
    // planes and scans sized for this picture at 4:4:4 (the larger case), grown when a later picture needs more
    const size_t planes = 2 * (size_t)((w + 3) / 4 * 4) * (size_t)h + 64;
    const size_t scan = (kSosBytes + 2 + scan_bound(blocks_of(w, h), kMaxBlockBitsColor) + 64 + 255) & ~(size_t)255;     // (k_append_scans reads 16 bytes at a time)
    if (int32_t rc = grow_scratch(e, &c.planes, &c.planes_cap, planes)) return rc;
    return grow_scratch(e, &c.scans, &c.scan_cap, scan, 2);          // (the Cb part, then the Cr part)
}

static int32_t prepare_color_constants(JpegAmdEncoder *e, const JpegAmdImage *img, int sub) {
    auto &c = e->color;
    const int q = quant_choice(e, img, nullptr, nullptr);
    if (q != c.cur_quality) {
        uint8_t t[64];
        quant_choice(e, img, nullptr, t);
        if (int32_t rc = upload_tables(e, t, c.tables_dev)) return rc;
        c.cur_quality = q;
    }
    if (!c.hdr_for.matches(img->width, img->height, q, sub)) {
        uint8_t luma[64], chroma[64], hdr[kColorPrefixMax];
        quant_choice(e, img, luma, chroma);
        const int len = (int)build_jfif_prefix_color(img->width, img->height, luma, chroma, chroma_mode(sub), hdr);
        if (int32_t rc = wait_pending(e)) return rc;
        HIP_TRY(hipMemcpy(c.hdr, hdr, (size_t)len, hipMemcpyHostToDevice));
        c.hdr_for.set(img->width, img->height, q, sub, len);
    }
    return JPEGAMD_OK;
}

// One scan of the colour file: k_tile_encode, then k_segment_merge + k_finalize or k_stitch, then the scan's symbol sums.
static int run_scan(JpegAmdEncoder *e, const ImageDesc &im, TileSource src, void *out, uint64_t cap, uint64_t *size_dev, const ScanTarget &tgt,
                    bool stitch, hipStream_t stream, hipEvent_t *ev) {
    const SingleOut one = {{out}, {size_dev}};
    if (int err = code_tiles(e, im, src, nullptr, nullptr, one.outs, cap, one.sizes, 1, &tgt, stitch, stream, ev, ev ? ev + 4 : nullptr)) return err;
    return launch_sum_stats(e->seg.syms, e->seg.exact, im.num_segs, tgt.stats, stream);
}

static int32_t color_single_run(JpegAmdEncoder *e, const JpegAmdImage *img, int32_t subsampling, void *out_dev, uint64_t out_capacity,
                                uint64_t *out_size_dev, void *stream_);
extern "C" int32_t jpegamd_encode_color_async(JpegAmdEncoder *e, const JpegAmdImage *img, int32_t subsampling, void *out_dev,
                                              uint64_t out_capacity, uint64_t *out_size_dev, void *stream_) {
    if (!e || !img || !out_dev || !out_size_dev) return JPEGAMD_ERR_ARG;
    if (!sub_valid(subsampling)) return JPEGAMD_ERR_ARG;
    if (is_px4(img->channel_order)) {             // a batch of one through the batch kernels (k_chroma_planes reads 3-byte pixels only)
        const SingleOut one = {{out_dev}, {out_size_dev}};
        return jpegamd_encode_color_batch_async(e, img, 1, subsampling, one.outs, out_capacity, one.sizes, stream_);
    }
    if (img->channel_order != JPEGAMD_ORDER_BGR && img->channel_order != JPEGAMD_ORDER_RGB) return JPEGAMD_ERR_ARG;
    const SingleOut one = {{out_dev}, {out_size_dev}};
    return with_metadata(e, 1, one.outs, out_capacity, one.sizes, stream_, false, [&](void *const *outs, uint64_t cap) {
        return color_single_run(e, img, subsampling, outs[0], cap, out_size_dev, stream_);
    });
}

static int32_t color_single_run(JpegAmdEncoder *e, const JpegAmdImage *img, int32_t subsampling, void *out_dev, uint64_t out_capacity,
                                uint64_t *out_size_dev, void *stream_) {
    ImageDesc iy;
    const bool stitch_y = use_stitch(e, img->width, img->height);
    int32_t rc = describe(e, img, &iy, stitch_y ? kSegTilesBatch : kSegTiles);
    if (rc) return rc;
    const ChromaGeom cg = chroma_geom(img->width, img->height, subsampling);
    rc = color_alloc(e, img->width, img->height);
    if (rc) return rc;
    rc = prepare_constants(e, img, false);
    if (rc) return rc;
    rc = prepare_color_constants(e, img, subsampling);
    if (rc) return rc;
    auto &c = e->color;
    hipStream_t stream = (hipStream_t)stream_;

    hipEvent_t *cev;
    rc = claim_slot(e, true, false, &cev);
    if (rc) return rc;
    const bool timed = cev != nullptr;
    HIP_TRY(hipMemsetAsync(c.scan_stats, 0, 3 * sizeof(ScanStats), stream));

    ChromaPlanesArgs pa;
    pa.pixels = (const uint8_t *)img->pixels;
    pa.width = img->width; pa.height = img->height; pa.row_stride = img->row_stride; pa.bottom_up = img->bottom_up ? 1 : 0;
    pa.rgb = img->channel_order == JPEGAMD_ORDER_RGB ? 1 : 0;
    pa.mode = chroma_mode(subsampling);
    pa.cw = cg.cw; pa.ch = cg.ch; pa.pitch = cg.pitch;
    pa.cb = c.planes; pa.cr = c.planes + (size_t)cg.pitch * (size_t)cg.ch;
    if (launch_chroma_planes(pa, stream, cev ? (void *const *)cev : nullptr)) return JPEGAMD_ERR_HIP;

    // Y: the grayscale scan of the same picture, behind the colour prefix, no EOI
    const ScanTarget ty = {c.hdr, c.hdr_for.len, 0, &c.scan_stats[0], false};
    if (timed) e->ring[(size_t)e->last_slot].cmerged[0] = !stitch_y;
    if (run_scan(e, iy, TileSource{kSrcRgb}, out_dev, out_capacity, &c.scan_size[0], ty, stitch_y, stream, cev ? cev + 2 : nullptr))
        return JPEGAMD_ERR_HIP;
    // Cb, Cr: one-byte planes, chroma tables, into scratch
    JpegAmdImage pimg = *img;
    pimg.width = cg.cw; pimg.height = cg.ch; pimg.row_stride = cg.pitch; pimg.bottom_up = 0; pimg.channel_order = JPEGAMD_ORDER_GRAY;
    const bool stitch_c = use_stitch(e, cg.cw, cg.ch);
    for (int k = 0; k < 2; ++k) {
        pimg.pixels = k ? pa.cr : pa.cb;
        ImageDesc ic;
        rc = describe(e, &pimg, &ic, stitch_c ? kSegTilesBatch : kSegTiles);
        if (rc) return rc;
        const ScanTarget tc = {c.hdr + kColorPrefixMax + 16 * k, kSosBytes, k, &c.scan_stats[1 + k], true};
        if (timed) e->ring[(size_t)e->last_slot].cmerged[1 + k] = !stitch_c;
        if (run_scan(e, ic, TileSource{kSrcPlane, true}, c.scans + (size_t)k * c.scan_cap, c.scan_cap, &c.scan_size[1 + k], tc, stitch_c, stream,
                     cev ? cev + 8 + 6 * k : nullptr))
            return JPEGAMD_ERR_HIP;
    }
    AppendArgs aa;
    aa.out = (uint8_t *)out_dev; aa.out_capacity = out_capacity; aa.out_size = out_size_dev;
    aa.scan_size = c.scan_size; aa.src[0] = c.scans; aa.src[1] = c.scans + c.scan_cap;
    aa.scan_stats = c.scan_stats; aa.stats = e->stats_dev;
    if (launch_append_scans(aa, stream, cev ? (void *const *)(cev + 20) : nullptr)) return JPEGAMD_ERR_HIP;
    return enqueued(e, stream, iy.num_segs, timed, true);
}

// ---------------------------------------------------------------------------------------------------------
// Colour batches: `count` pictures of one geometry.  k_chroma_planes_batch writes all 2 x count chroma planes; Y runs as ONE batch of
// the RGB path straight into the callers' buffers behind the colour prefix; every Cb and Cr plane shares one geometry and one set of
// tables, so all of them run through the chroma pipeline as batches of planes -- as few launches as the context's scratch allows --
// bare (no SOS, no EOI) into per-plane scratch slots; k_picture_stats adds up each launch's tile records per picture and scan; and
// k_append_scans_batch finishes every picture.  Nothing waits on the host.
// ---------------------------------------------------------------------------------------------------------
constexpr int kBatchLaunches = 1 + 2 * kMaxBatch;     // the Y launch, and at most one chroma launch per plane

// How the chroma planes of a batch are grouped into launches: the most planes per launch that kMaxBatch and the context's tiles,
// segments, segment words (k_segment_merge + k_finalize) or k_stitch workgroups allow -- a group never holds more than fits, whatever
// the per-row rounding of the plane's geometry -- then spread evenly over the launches that takes.  Returns false only when not
// even one plane fits.
struct ChromaPlan { int group, launches, seg_tiles; bool stitch; };
static int chroma_group_limit(const CtxLimits &l, int cw, int ch, int seg_tiles, bool stitch) {
    const int64_t tiles = tiles_for(cw, ch);
    const int64_t segs = segs_for(cw, ch, nullptr, nullptr, nullptr, seg_tiles);
    int64_t g = kMaxBatch;
    g = std::min(g, (int64_t)l.max_tiles / tiles);
    g = std::min(g, (int64_t)l.max_segs / segs);
    if (stitch) g = std::min(g, (int64_t)l.max_wgs / stitch_workgroups((int)segs));
    else g = std::min(g, (int64_t)(l.words_cap / ((size_t)segs * (size_t)seg_cap_words(seg_tiles))));
    return (int)g;
}
static bool chroma_plan(const CtxLimits &l, int pipeline, int cw, int ch, int planes, ChromaPlan *p) {
    p->stitch = use_stitch_for(pipeline, cw, ch);
    int g;
    if (p->stitch) {
        p->seg_tiles = kSegTilesBatch;                                 // (k_stitch works on segments of 16 tiles)
        g = chroma_group_limit(l, cw, ch, kSegTilesBatch, true);
    } else {                                                           // segments of 16 tiles for four planes or more, as a grayscale batch --
        p->seg_tiles = kSegTiles;                                      // unless that takes more launches
        g = chroma_group_limit(l, cw, ch, kSegTiles, false);
        const int g16 = chroma_group_limit(l, cw, ch, kSegTilesBatch, false);
        if (std::min(g16, planes) >= 4 && g16 >= 1 && (planes + g16 - 1) / g16 <= (planes + g - 1) / std::max(g, 1)) {
            p->seg_tiles = kSegTilesBatch;
            g = g16;
        }
    }
    if (g < 1 || planes < 1) return false;
    p->launches = (planes + g - 1) / g;
    p->group = (planes + p->launches - 1) / p->launches;
    return true;
}

// Host-only (tests): the chroma launches of a colour batch of `count` width x height pictures on a context created for
// max_width x max_height under `pipeline`: out = {planes per launch, launches, tiles per segment, k_stitch}.  Not part of the
// public header.
extern "C" int32_t jpegamd_debug_chroma_groups(int32_t max_width, int32_t max_height, int32_t pipeline, int32_t width, int32_t height,
                                               int32_t count, int32_t subsampling, int32_t *out) {
    if (!out || max_width <= 0 || max_height <= 0 || width <= 0 || height <= 0 || count < 1 || count > kMaxBatch) return JPEGAMD_ERR_ARG;
    if (!sub_valid(subsampling)) return JPEGAMD_ERR_ARG;
    const ChromaGeom cg = chroma_geom(width, height, subsampling);
    ChromaPlan p;
    if (!chroma_plan(context_limits(max_width, max_height), pipeline, cg.cw, cg.ch, 2 * count, &p)) return JPEGAMD_ERR_TOO_LARGE;
    out[0] = p.group; out[1] = p.launches; out[2] = p.seg_tiles; out[3] = p.stitch ? 1 : 0;
    return JPEGAMD_OK;
}

constexpr size_t kBatchMetaStats = kBatchLaunches * sizeof(ScanStats);
constexpr size_t kBatchMetaPic = (size_t)kMaxBatch * kPicStatWords * sizeof(uint64_t);
constexpr size_t kBatchMetaBytes = kBatchMetaStats + kBatchMetaPic + 3 * kMaxBatch * sizeof(uint64_t);

// The batch's scratch: fixed-size records once, planes and scan slots grown when a call needs more than the context holds.
static int32_t color_batch_alloc(JpegAmdEncoder *e, size_t planes, size_t scans) {
    auto &c = e->color;
    if (!c.bmeta) HIP_TRY(hipMalloc((void **)&c.bmeta, kBatchMetaBytes));
    if (int32_t rc = grow_scratch(e, &c.bplanes, &c.bplanes_cap, planes)) return rc;
    return grow_scratch(e, &c.bscans, &c.bscans_cap, scans);
}

// The caller's own chroma (jpegamd_encode_ycbcr_batch_async): cb[i] / cr[i] the planes of picture i (a pair layout: cb[i] alone; a
// packed 4:2:2 layout: cb[i] is the packed plane -- the picture's y -- and c_stride its row stride).  layout, format and range
// (JPEGAMD_CHROMA_*, _SAMPLES_*, _RANGE_*) choose the sources of the launches: ycbcr_y_source, ycbcr_chroma_source.
struct YccSource {
    int32_t layout, c_stride, format, range;
    const uint8_t *cb[kMaxBatch], *cr[kMaxBatch];
    int32_t matrix;                     // JPEGAMD_MATRIX_*: BT709 goes through k_ycbcr_matrix_batch, and the launches read ITS planes
};

// The kinds of YCbCr input that are taken: a known layout, format and range; a packed layout in one byte per sample (Y210: not taken).
static bool ycbcr_kind_valid(int32_t layout, int32_t format, int32_t range) {
    if (range != JPEGAMD_RANGE_FULL && range != JPEGAMD_RANGE_LIMITED) return false;
    if (format != JPEGAMD_SAMPLES_8 && format != JPEGAMD_SAMPLES_10_MSB && format != JPEGAMD_SAMPLES_10_LSB) return false;
    if (layout != JPEGAMD_CHROMA_PLANES && layout != JPEGAMD_CHROMA_CBCR && layout != JPEGAMD_CHROMA_CRCB && !is_packed422(layout)) return false;
    return !(is_packed422(layout) && format != JPEGAMD_SAMPLES_8);
}

// What the launches of a YCbCr batch read: the source, and ImageDesc::select (a source that does not read it keeps describe()'s).
// 16-bit words are narrowed on read whichever the range; the shift that leaves the 10-bit value is 6 (MSB-aligned) or 0.
struct SourceChoice { TileSource src; uint32_t select; };
static uint32_t depth_shift(int32_t format) { return format == JPEGAMD_SAMPLES_10_MSB ? 6u : 0u; }
// The Y launch: a plane of samples; of a packed plane byte 0 (Y Cb Y Cr) or 1 (Cb Y Cr Y) of every pair, for EVERY picture.
static SourceChoice ycbcr_y_source(int32_t layout, int32_t format, int32_t range) {
    const bool expand = range == JPEGAMD_RANGE_LIMITED;
    if (format != JPEGAMD_SAMPLES_8) return {{kSrcPlane16, false, expand}, select_depth(0, depth_shift(format))};
    if (is_packed422(layout)) return {{kSrcPair, false, expand}, select_byte(layout == JPEGAMD_CHROMA_UYVY ? 1 : 0, 0)};
    return {{kSrcPlane, false, expand}, select_luma(false)};
}
// A chroma launch whose first plane has index `first` in the WHOLE call (picture first / 2; Cb even, Cr odd): a group may be odd, a
// launch then starts on a Cr plane.  The parity is flipped when Cr is stored first; a packed plane has Cb in front of Cr, at bytes
// 1 and 3 (Y Cb Y Cr) or 0 and 2 (Cb Y Cr Y).
static SourceChoice ycbcr_chroma_source(int32_t layout, int32_t format, int32_t range, int first) {
    const bool expand = range == JPEGAMD_RANGE_LIMITED, wide = format != JPEGAMD_SAMPLES_8;
    const uint32_t parity = (uint32_t)((first & 1) ^ (layout == JPEGAMD_CHROMA_CRCB ? 1 : 0));
    if (is_packed422(layout)) return {{kSrcQuad, true, expand}, select_byte(parity, layout == JPEGAMD_CHROMA_YUYV ? 1 : 0)};
    if (layout == JPEGAMD_CHROMA_PLANES)
        return wide ? SourceChoice{{kSrcPlane16, true, expand}, select_depth(0, depth_shift(format))} : SourceChoice{{kSrcPlane, true, expand}, select_luma(false)};
    return wide ? SourceChoice{{kSrcPair16, true, expand}, select_depth(parity, depth_shift(format))} : SourceChoice{{kSrcPair, true, expand}, select_byte(parity, 0)};
}

// Host-only (tests): the two functions above for one kind of input: out = {layout, chroma, expand, select} of the Y launch, then of
// a chroma launch that starts on plane `first`.  JPEGAMD_ERR_ARG for a kind the encode entry refuses.  Not part of the public header.
extern "C" int32_t jpegamd_debug_ycbcr_sources(int32_t chroma_layout, int32_t sample_format, int32_t sample_range, int32_t first, uint32_t *out) {
    if (!out || first < 0 || !ycbcr_kind_valid(chroma_layout, sample_format, sample_range)) return JPEGAMD_ERR_ARG;
    const SourceChoice both[2] = {ycbcr_y_source(chroma_layout, sample_format, sample_range),
                                  ycbcr_chroma_source(chroma_layout, sample_format, sample_range, first)};
    for (int k = 0; k < 2; ++k) {
        out[4 * k] = (uint32_t)both[k].src.layout; out[4 * k + 1] = both[k].src.chroma; out[4 * k + 2] = both[k].src.expand;
        out[4 * k + 3] = both[k].select;
    }
    return JPEGAMD_OK;
}

// What a BT.709 batch keeps in color.bplanes: the 2 x count chroma planes where the RGB route has them, then count Y planes.
struct MatrixScratch {
    int ypitch;
    size_t yplane_bytes, y_off, total;
};
static MatrixScratch matrix_scratch(int w, int h, int count, size_t plane_bytes) {
    MatrixScratch m;
    m.ypitch = (w + 3) / 4 * 4;
    m.yplane_bytes = round_up((size_t)m.ypitch * (size_t)h, 256);
    m.y_off = 2 * (size_t)count * plane_bytes;
    m.total = m.y_off + (size_t)count * m.yplane_bytes + 256;
    return m;
}

// k_ycbcr_matrix_batch over the caller's planes (g0 / px: the Y planes, ycc: the chroma) into color.bplanes, which holds m.total bytes.
static int launch_matrix_pass(JpegAmdEncoder *e, const JpegAmdImage &g0, const PlaneSet &px, const YccSource &ycc, int32_t count,
                              int32_t subsampling, const ChromaGeom &cg, const MatrixScratch &m, hipStream_t stream, void *const *ev) {
    YccMatrixBatchArgs ma;
    std::memset(&ma, 0, sizeof(ma));
    for (int i = 0; i < count; ++i) { ma.y[i] = px.p[0][i]; ma.cb[i] = ycc.cb[i]; ma.cr[i] = ycc.cr[i]; }
    ma.batch = count;
    ma.width = g0.width; ma.height = g0.height; ma.y_stride = g0.row_stride; ma.c_stride = ycc.c_stride;
    ma.mode = chroma_mode(subsampling);
    ma.walk = is_packed422(ycc.layout) ? kMatrixWalkPacked : (ycc.layout == JPEGAMD_CHROMA_PLANES ? kMatrixWalkPlanes : kMatrixWalkPairs);
    ma.sample_bytes = ycc.format == JPEGAMD_SAMPLES_8 ? 1 : 2;
    ma.first = (ycc.layout == JPEGAMD_CHROMA_CRCB || ycc.layout == JPEGAMD_CHROMA_UYVY) ? 1 : 0;
    ma.shift = (int32_t)depth_shift(ycc.format);
    ma.limited = ycc.range == JPEGAMD_RANGE_LIMITED ? 1 : 0;
    ma.cw = cg.cw; ma.ch = cg.ch; ma.pitch = cg.pitch; ma.ypitch = m.ypitch;
    ma.plane_bytes = cg.plane_bytes; ma.yplane_bytes = m.yplane_bytes;
    ma.planes = e->color.bplanes; ma.yplanes = e->color.bplanes + m.y_off;
    return launch_ycbcr_matrix_batch(ma, stream, ev);
}

// k_float_planes_batch over the caller's float samples into color.bplanes, laid out as `m` says: `out` kFloatOutColor -- Y, Cb and Cr
// planes of geometry cg, where a BT.709 batch has them -- or the Y planes alone (m.y_off = 0: kFloatOutLuma of three channels, or
// kFloatOutSingle).  The host picks the walk from the pointers and strides: three planes of packed samples; the three channels of a
// pixel side by side in either order; anything else by samples.
static int launch_reduce_pass(JpegAmdEncoder *e, const FloatSource &fl, int w, int h, int32_t count, int out, int32_t subsampling,
                              const ChromaGeom &cg, const MatrixScratch &m, hipStream_t stream, void *const *ev);
static int launch_resize_pass(JpegAmdEncoder *e, const FloatSource &fl, int w, int h, int32_t count, int out, int32_t subsampling,
                              const ChromaGeom &cg, const MatrixScratch &m, hipStream_t stream, void *const *ev);
static int launch_float_pass(JpegAmdEncoder *e, const FloatSource &fl, int w, int h, int32_t count, int out, int32_t subsampling,
                             const ChromaGeom &cg, const MatrixScratch &m, hipStream_t stream, void *const *ev) {
    if (fl.reduce) return launch_reduce_pass(e, fl, w, h, count, out, subsampling, cg, m, stream, ev);
    if (fl.resize) return launch_resize_pass(e, fl, w, h, count, out, subsampling, cg, m, stream, ev);
    FloatPlanesBatchArgs fa;
    std::memset(&fa, 0, sizeof(fa));
    const int kb = fl.type == JPEGAMD_FLOAT_F32 ? 4 : 2;
    // the three samples of a pixel side by side: 0 as R G B, 1 as B G R, -1 otherwise -- one answer for every picture of the call
    const auto side_by_side = [&](int i) {
        const uint8_t *r = fl.plane[0][i], *g = fl.plane[1][i], *b = fl.plane[2][i];
        return (g == r + kb && b == g + kb) ? 0 : ((g == b + kb && r == g + kb) ? 1 : -1);
    };
    int order = fl.channels == 3 && fl.pixel_stride == 3 * kb ? side_by_side(0) : -1;
    for (int i = 1; i < count && order >= 0; ++i) if (side_by_side(i) != order) order = -1;
    fa.walk = order >= 0 ? kFloatWalkPacked3 : (fl.pixel_stride == kb ? kFloatWalkPlanar : kFloatWalkGeneric);
    fa.reversed = order == 1 ? 1 : 0;
    for (int i = 0; i < count; ++i)
        for (int k = 0; k < fl.channels; ++k) fa.plane[k][i] = fl.plane[k][i];
    if (order == 1) for (int i = 0; i < count; ++i) fa.plane[0][i] = fl.plane[2][i];                   // the lowest of the three
    fa.batch = count;
    fa.width = w; fa.height = h; fa.row_stride = fl.row_stride; fa.pixel_stride = fl.pixel_stride;
    fa.type = fl.type; fa.out = out; fa.scale = fl.scale; fa.offset = fl.offset;
    fa.ypitch = m.ypitch; fa.yplane_bytes = m.yplane_bytes; fa.yplanes = e->color.bplanes + m.y_off;
    if (out == kFloatOutColor) {
        fa.mode = chroma_mode(subsampling);
        fa.cw = cg.cw; fa.ch = cg.ch; fa.pitch = cg.pitch; fa.plane_bytes = cg.plane_bytes; fa.planes = e->color.bplanes;
    } else {
        fa.cw = w; fa.ch = h;
    }
    return launch_float_planes_batch(fa, stream, ev);
}
// k_reduce_planes_batch in its place for a batch of bytes to be reduced (fl.reduce): w x h is the REDUCED picture, `out` and the
// scratch layout are the float pass's, and the walk is chosen the same way -- with every factor that is not 1, 2, 4 or 8 on the walk
// that takes bytes one by one.
static int launch_reduce_pass(JpegAmdEncoder *e, const FloatSource &fl, int w, int h, int32_t count, int out, int32_t subsampling,
                              const ChromaGeom &cg, const MatrixScratch &m, hipStream_t stream, void *const *ev) {
    static_assert(kReduceOutColor == kFloatOutColor && kReduceOutLuma == kFloatOutLuma && kReduceOutSingle == kFloatOutSingle, "one `out`");
    ReducePlanesBatchArgs ra;
    std::memset(&ra, 0, sizeof(ra));
    const auto side_by_side = [&](int i) {
        const uint8_t *r = fl.plane[0][i], *g = fl.plane[1][i], *b = fl.plane[2][i];
        return (g == r + 1 && b == g + 1) ? 0 : ((g == b + 1 && r == g + 1) ? 1 : -1);
    };
    const bool pow2 = fl.reduce == 1 || fl.reduce == 2 || fl.reduce == 4 || fl.reduce == 8;
    int order = pow2 && fl.channels == 3 && fl.pixel_stride == 3 ? side_by_side(0) : -1;
    for (int i = 1; i < count && order >= 0; ++i) if (side_by_side(i) != order) order = -1;
    ra.walk = order >= 0 ? kReduceWalkPacked3 : (pow2 && fl.pixel_stride == 1 ? kReduceWalkPlanar : kReduceWalkGeneric);
    ra.reversed = order == 1 ? 1 : 0;
    for (int i = 0; i < count; ++i)
        for (int k = 0; k < fl.channels; ++k) ra.plane[k][i] = fl.plane[k][i];
    if (order == 1) for (int i = 0; i < count; ++i) ra.plane[0][i] = fl.plane[2][i];                   // the lowest of the three
    ra.batch = count;
    ra.src_width = fl.src_width; ra.src_height = fl.src_height; ra.row_stride = fl.row_stride; ra.pixel_stride = fl.pixel_stride;
    ra.factor = fl.reduce; ra.width = w; ra.height = h; ra.out = out;
    ra.ypitch = m.ypitch; ra.yplane_bytes = m.yplane_bytes; ra.yplanes = e->color.bplanes + m.y_off;
    if (out == kReduceOutColor) {
        ra.mode = chroma_mode(subsampling);
        ra.cw = cg.cw; ra.ch = cg.ch; ra.pitch = cg.pitch; ra.plane_bytes = cg.plane_bytes; ra.planes = e->color.bplanes;
    } else {
        ra.cw = w; ra.ch = h;
    }
    return launch_reduce_planes_batch(ra, stream, ev);
}
// k_resize_planes_batch in its place for a batch of bytes to be resized (fl.resize): w x h is the TARGET (fl.out_width x
// fl.out_height), `out` and the scratch layout are the float pass's.  The walk: planes of bytes one apart; the three channels of every
// picture at the same places inside a pixel of at most kResizePackedMax bytes (R G B, B G R, RGBA, BGRA), read as one run from the
// lowest of the three pointers; anything else by bytes.
static int launch_resize_pass(JpegAmdEncoder *e, const FloatSource &fl, int w, int h, int32_t count, int out, int32_t subsampling,
                              const ChromaGeom &cg, const MatrixScratch &m, hipStream_t stream, void *const *ev) {
    static_assert(kResizeOutColor == kFloatOutColor && kResizeOutLuma == kFloatOutLuma && kResizeOutSingle == kFloatOutSingle, "one `out`");
    ResizePlanesBatchArgs ra;
    std::memset(&ra, 0, sizeof(ra));
    bool packed = fl.channels == 3 && fl.pixel_stride > 1 && fl.pixel_stride <= kResizePackedMax;
    for (int i = 0; i < count && packed; ++i) {
        const uint8_t *lowest = std::min(fl.plane[0][i], std::min(fl.plane[1][i], fl.plane[2][i]));
        for (int k = 0; k < 3; ++k) {
            const ptrdiff_t off = fl.plane[k][i] - lowest;
            if (off >= fl.pixel_stride || (i > 0 && off != ra.offset[k])) packed = false;
            if (i == 0) ra.offset[k] = (int32_t)std::min<ptrdiff_t>(off, kResizePackedMax);
        }
    }
    if (!packed) ra.offset[0] = ra.offset[1] = ra.offset[2] = 0;
    ra.walk = packed ? kResizeWalkPacked : (fl.pixel_stride == 1 ? kResizeWalkPlanar : kResizeWalkGeneric);
    for (int i = 0; i < count; ++i)
        for (int k = 0; k < fl.channels; ++k) ra.plane[k][i] = fl.plane[k][i];
    if (packed) for (int i = 0; i < count; ++i) ra.plane[0][i] = fl.plane[0][i] - ra.offset[0];        // the lowest of the three
    ra.batch = count;
    ra.src_width = fl.src_width; ra.src_height = fl.src_height; ra.row_stride = fl.row_stride; ra.pixel_stride = fl.pixel_stride;
    ra.width = w; ra.height = h; ra.out = out;
    ra.ypitch = m.ypitch; ra.yplane_bytes = m.yplane_bytes; ra.yplanes = e->color.bplanes + m.y_off;
    if (out == kResizeOutColor) {
        ra.mode = chroma_mode(subsampling);
        ra.cw = cg.cw; ra.ch = cg.ch; ra.pitch = cg.pitch; ra.plane_bytes = cg.plane_bytes; ra.planes = e->color.bplanes;
    } else {
        ra.cw = w; ra.ch = h;
    }
    return launch_resize_planes_batch(ra, stream, ev);
}
// ... the Y planes alone, for the grayscale routes: gy describes the scratch planes (matrix_scratch with no chroma in front).
static int launch_float_luma_pass(JpegAmdEncoder *e, const FloatSource &fl, const JpegAmdImage &gy, int32_t count, hipStream_t stream,
                                  void *const *ev) {
    const MatrixScratch m = matrix_scratch(gy.width, gy.height, count, 0);
    return launch_float_pass(e, fl, gy.width, gy.height, count, fl.channels == 1 ? kFloatOutSingle : kFloatOutLuma, 0, ChromaGeom{}, m,
                             stream, ev);
}

// k_chroma_planes_batch over the pixels of an RGB batch (g0 / px, any layout the colour entries take): the 2 x count chroma planes of
// geometry cg into color.bplanes, plane j (picture j / 2, Cb even, Cr odd) at j x cg.plane_bytes.
static int launch_plane_pass(JpegAmdEncoder *e, const JpegAmdImage &g0, const PlaneSet &px, int32_t count, int32_t subsampling,
                             const ChromaGeom &cg, hipStream_t stream, void *const *ev) {
    ChromaPlanesBatchArgs pa;
    std::memset(&pa, 0, sizeof(pa));
    for (int i = 0; i < count; ++i) { pa.pixels[i] = px.p[0][i]; pa.pixels_g[i] = px.p[1][i]; pa.pixels_b[i] = px.p[2][i]; }
    pa.layout = g0.channel_order == kOrderPlanar ? kChromaSrcPlanar : (is_px4(g0.channel_order) ? kChromaSrcPx4 : kChromaSrcPx3);
    pa.batch = count;
    pa.width = g0.width; pa.height = g0.height; pa.row_stride = g0.row_stride; pa.bottom_up = g0.bottom_up ? 1 : 0;
    pa.rgb = (g0.channel_order == JPEGAMD_ORDER_BGR || g0.channel_order == JPEGAMD_ORDER_BGRA) ? 0 : 1;
    pa.mode = chroma_mode(subsampling);
    pa.cw = cg.cw; pa.ch = cg.ch; pa.pitch = cg.pitch;
    pa.plane_bytes = cg.plane_bytes; pa.planes = e->color.bplanes;
    return launch_chroma_planes_batch(pa, stream, ev);
}

// What the launches of a colour batch read.  `ycc` null: the call's own pixels for Y, the plane scratch for Cb and Cr (an RGB batch, or
// a BT.709 one behind its pass); otherwise the caller's planes, and the launch's ImageDesc::select with them.
// The Y launch (g: the pictures as the launch sees them).
static TileSource y_source_of(const JpegAmdImage &g, const YccSource *ycc, ImageDesc *im) {
    if (!ycc) return src_of(&g);
    const SourceChoice y = ycbcr_y_source(ycc->layout, ycc->format, ycc->range);
    im->select = y.select;
    return y.src;
}
// A chroma launch whose first plane has index `first` in the whole call.
static TileSource chroma_source_of(const YccSource *ycc, int first, ImageDesc *im) {
    if (!ycc) return {kSrcPlane, true};
    const SourceChoice cs = ycbcr_chroma_source(ycc->layout, ycc->format, ycc->range, first);
    im->select = cs.select;
    return cs.src;
}
// Plane j of the call (picture j / 2, Cb even, Cr odd).  Cb and Cr of a caller's picture may lie in ONE plane: pairs, or a packed plane.
static const uint8_t *chroma_plane_of(const JpegAmdEncoder *e, const YccSource *ycc, const ChromaGeom &cg, int j) {
    if (!ycc) return e->color.bplanes + (size_t)j * cg.plane_bytes;
    if (ycc->layout != JPEGAMD_CHROMA_PLANES) return ycc->cb[j / 2];
    return (j & 1) ? ycc->cr[j / 2] : ycc->cb[j / 2];
}

// The colour files of a batch whose arguments are known to be good: g0 describes every picture, ps holds their pixels.
// `ycc` (a YCbCr batch): g0 / px are the Y planes as a GRAY picture, the chroma scans read the caller's planes -- no
// k_chroma_planes_batch launch, no plane scratch.  A BT.709 YCbCr batch (ycc->matrix) is the RGB route with another kernel in front:
// k_ycbcr_matrix_batch writes BT.601 Y, Cb and Cr planes into the plane scratch, and every launch reads those as full-range planes.
static int32_t color_batch_run(JpegAmdEncoder *e, const JpegAmdImage &g0, const PlaneSet &px, int32_t count, int32_t subsampling,
                               void *const *outs_dev, uint64_t out_capacity, uint64_t *const *out_sizes_dev, void *stream_,
                               const YccSource *ycc_in, const FloatSource *fl) {
    // a front pass fills the scratch planes: k_ycbcr_matrix_batch (a BT.709 batch), or k_float_planes_batch (`fl`, a float batch: g0 is a
    // GRAY picture of the batch's geometry, px is not read)
    const bool front = fl || (ycc_in && ycc_in->matrix == JPEGAMD_MATRIX_BT709);
    const YccSource *const ycc = front ? nullptr : ycc_in;            // what the launches read: the caller's planes, or the scratch
    // Y: the grayscale batch's launch plan
    ImageDesc iy;
    bool stitch_y;
    int32_t rc = plan_batch(e, g0, px, count, &iy, &stitch_y);
    if (rc) return rc;
    // Cb, Cr: 2 count planes at one pitch, in as few launches as the context allows
    const ChromaGeom cg = chroma_geom(g0.width, g0.height, subsampling);
    const int planes = 2 * count;
    ChromaPlan plan;
    if (!chroma_plan(e->lim, e->pipeline, cg.cw, cg.ch, planes, &plan)) return JPEGAMD_ERR_TOO_LARGE;
    const size_t slot_bytes = round_up(scan_bound(blocks_of(cg.cw, cg.ch), kMaxBlockBitsColor) + 64, 256);      // (k_append_scans_batch reads 16 bytes at a time)
    const MatrixScratch ms = matrix_scratch(g0.width, g0.height, count, cg.plane_bytes);
    rc = color_alloc_consts(e);
    if (rc) return rc;
    rc = color_batch_alloc(e, front ? ms.total : (ycc ? 0 : planes * cg.plane_bytes + 256), planes * slot_bytes);
    if (rc) return rc;
    // behind a front pass the Y launch is a GRAY batch over the scratch Y planes
    JpegAmdImage gy = g0;
    PlaneSet py = px;
    if (front) {
        gy.pixels = e->color.bplanes + ms.y_off; gy.row_stride = ms.ypitch;
        for (int i = 0; i < count; ++i) py.p[0][i] = e->color.bplanes + ms.y_off + (size_t)i * ms.yplane_bytes;
        rc = plan_batch(e, gy, py, count, &iy, &stitch_y);
        if (rc) return rc;
    }
    rc = prepare_constants(e, &g0, false);
    if (rc) return rc;
    rc = prepare_color_constants(e, &g0, subsampling);
    if (rc) return rc;
    auto &c = e->color;
    ScanStats *lstats = reinterpret_cast<ScanStats *>(c.bmeta);
    unsigned long long *pic = reinterpret_cast<unsigned long long *>(c.bmeta + kBatchMetaStats);
    uint64_t *y_size = reinterpret_cast<uint64_t *>(c.bmeta + kBatchMetaStats + kBatchMetaPic);
    uint64_t *c_size = y_size + kMaxBatch;
    hipStream_t stream = (hipStream_t)stream_;

    hipEvent_t *cev;
    rc = claim_slot(e, true, true, &cev);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(c.bmeta, 0, kBatchMetaStats + kBatchMetaPic, stream));

    hipEvent_t *const ev_y = ycc ? cev : nullptr;     // a YCbCr batch begins with its Y launch: that kernel's begin stamp opens ns_total
    hipEvent_t ev_planes[2] = {cev ? cev[0] : nullptr, nullptr};      // (a plane pass comes first: ITS begin stamp opens ns_total)
    if (fl) {
        if (launch_float_pass(e, *fl, g0.width, g0.height, count, kFloatOutColor, subsampling, cg, ms, stream, cev ? (void *const *)ev_planes : nullptr))
            return JPEGAMD_ERR_HIP;
    } else if (front) {
        if (launch_matrix_pass(e, g0, px, *ycc_in, count, subsampling, cg, ms, stream, cev ? (void *const *)ev_planes : nullptr))
            return JPEGAMD_ERR_HIP;
    } else if (!ycc) {
        if (launch_plane_pass(e, g0, px, count, subsampling, cg, stream, cev ? (void *const *)ev_planes : nullptr)) return JPEGAMD_ERR_HIP;
    }

    // Y: every picture's scan behind the colour prefix, no EOI; its size into y_size
    {
        uint64_t *sizes[kMaxBatch];
        for (int i = 0; i < count; ++i) sizes[i] = y_size + i;
        const ScanTarget ty = {c.hdr, c.hdr_for.len, 0, &lstats[0], false};
        PictureStatsArgs ps = {e->tile_head, e->huff, iy.num_tiles, count, 0, 0, pic};
        const TileSource ysrc = y_source_of(gy, ycc, &iy);
        if (code_tiles(e, iy, ysrc, &py, &ps, outs_dev, out_capacity, sizes, 1, &ty, stitch_y, stream, ev_y, nullptr)) return JPEGAMD_ERR_HIP;
    }
    // Cb, Cr: plane j (picture j / 2) bare into slot j; its size into c_size[j]
    JpegAmdImage pimg = g0;
    pimg.width = cg.cw; pimg.height = cg.ch; pimg.row_stride = ycc ? ycc->c_stride : cg.pitch; pimg.bottom_up = 0; pimg.channel_order = JPEGAMD_ORDER_GRAY;
    pimg.pixels = chroma_plane_of(e, ycc, cg, 0);
    uintptr_t chroma_bits = 0;                                         // every plane of the call: one answer for all its launches
    for (int j = 0; j < planes; ++j) chroma_bits |= (uintptr_t)chroma_plane_of(e, ycc, cg, j);
    for (int l = 0; l < plan.launches; ++l) {
        const int first = l * plan.group, n = std::min(plan.group, planes - first);
        ImageDesc ic;
        rc = describe(e, &pimg, &ic, plan.seg_tiles);
        if (rc) return rc;
        void *outs[kMaxBatch];
        uint64_t *sizes[kMaxBatch];
        for (int i = 0; i < n; ++i) {
            const int j = first + i;                                   // the plane's index in the whole call: picture j / 2, Cb (even) or Cr (odd)
            ic.batch_pixels[i] = chroma_plane_of(e, ycc, cg, j);
            outs[i] = c.bscans + (size_t)j * slot_bytes;
            sizes[i] = c_size + j;
        }
        ic.pixels = ic.batch_pixels[0];
        ic.batch = n;
        ic.tile_end = n * ic.num_tiles;
        ic.seg_end = n * ic.num_segs;
        ic.fast_ok = dword_loader_ok(chroma_bits, pimg.row_stride);
        const TileSource csrc = chroma_source_of(ycc, first, &ic);
        const ScanTarget tc = {c.hdr, 0, 0, &lstats[1 + l], true};
        PictureStatsArgs ps = {e->tile_head, c.huff, ic.num_tiles, n, 1, first, pic};
        if (code_tiles(e, ic, csrc, nullptr, &ps, outs, slot_bytes, sizes, 1, &tc, plan.stitch, stream, nullptr, nullptr)) return JPEGAMD_ERR_HIP;
    }
    AppendBatchArgs aa;
    std::memset(&aa, 0, sizeof(aa));
    for (int i = 0; i < count; ++i) { aa.out[i] = (uint8_t *)outs_dev[i]; aa.out_size[i] = out_sizes_dev[i]; }
    aa.out_capacity = out_capacity;
    aa.batch = count; aa.hdr_len = c.hdr_for.len;
    aa.y_size = y_size; aa.c_size = c_size;
    aa.scans = c.bscans; aa.slot_bytes = slot_bytes;
    aa.sos = c.hdr + kColorPrefixMax;
    aa.pic = pic;
    aa.launch_stats = lstats; aa.n_launch = 1 + plan.launches;
    aa.stats = e->stats_dev;
    hipEvent_t ev_append[2] = {nullptr, cev ? cev[21] : nullptr};
    if (launch_append_scans_batch(aa, stream, cev ? (void *const *)ev_append : nullptr)) return JPEGAMD_ERR_HIP;
    return enqueued(e, stream, count * iy.num_segs, cev != nullptr, true);
}

// ... with the context's metadata in front.
static int32_t color_batch(JpegAmdEncoder *e, const JpegAmdImage &g0, const PlaneSet &px, int32_t count, int32_t subsampling,
                           void *const *outs_dev, uint64_t out_capacity, uint64_t *const *out_sizes_dev, void *stream_,
                           const YccSource *ycc_in = nullptr, const FloatSource *fl = nullptr) {
    return with_metadata(e, count, outs_dev, out_capacity, out_sizes_dev, stream_, false, [&](void *const *outs, uint64_t cap) {
        return color_batch_run(e, g0, px, count, subsampling, outs, cap, out_sizes_dev, stream_, ycc_in, fl);
    });
}

extern "C" int32_t jpegamd_encode_color_batch_async(JpegAmdEncoder *e, const JpegAmdImage *imgs, int32_t count, int32_t subsampling,
                                                    void *const *outs_dev, uint64_t out_capacity, uint64_t *const *out_sizes_dev,
                                                    void *stream_) {
    // the arguments first: nothing of the context is read before they are known to be good
    if (!e || !imgs || !outs_dev || !out_sizes_dev || count < 1 || count > kMaxBatch) return JPEGAMD_ERR_ARG;
    if (!sub_valid(subsampling)) return JPEGAMD_ERR_ARG;
    const JpegAmdImage &g0 = imgs[0];
    if (g0.channel_order != JPEGAMD_ORDER_BGR && g0.channel_order != JPEGAMD_ORDER_RGB && !is_px4(g0.channel_order)) return JPEGAMD_ERR_ARG;
    if (g0.width <= 0 || g0.row_stride < bytes_per_pixel(g0.channel_order) * (int64_t)g0.width) return JPEGAMD_ERR_ARG;
    PlaneSet ps;
    if (int32_t rc = uniform_batch_args(imgs, count, outs_dev, out_sizes_dev, &ps)) return rc;
    return color_batch(e, g0, ps, count, subsampling, outs_dev, out_capacity, out_sizes_dev, stream_);
}

// The arguments of a planar batch, checked before anything of the context is read (`gray_ok`: subsampling 0 is taken) -> the R planes
// as a picture of the internal planar order, all three planes in ps.
static int32_t planar_args(const JpegAmdEncoder *e, const JpegAmdPlanarImage *imgs, int32_t count, int32_t subsampling, bool gray_ok,
                           void *const *outs_dev, void *const *out_sizes_dev, JpegAmdImage *g0, PlaneSet *ps, uint64_t **sizes) {
    if (!e || !imgs || !outs_dev || !out_sizes_dev || count < 1 || count > kMaxBatch) return JPEGAMD_ERR_ARG;
    if (!(gray_ok && subsampling == 0) && !sub_valid(subsampling)) return JPEGAMD_ERR_ARG;
    const JpegAmdPlanarImage &p0 = imgs[0];
    if (p0.width <= 0 || p0.height <= 0 || p0.width > 65535 || p0.height > 65535 || p0.row_stride < p0.width) return JPEGAMD_ERR_ARG;
    *ps = PlaneSet{};
    for (int i = 0; i < count; ++i) {
        const JpegAmdPlanarImage &g = imgs[i];
        if (!outs_dev[i] || !out_sizes_dev[i] || !g.plane[0] || !g.plane[1] || !g.plane[2]) return JPEGAMD_ERR_ARG;
        if (g.width != p0.width || g.height != p0.height || g.row_stride != p0.row_stride || (g.bottom_up != 0) != (p0.bottom_up != 0) ||
            g.quality != p0.quality)
            return JPEGAMD_ERR_ARG;
        for (int k = 0; k < 3; ++k) ps->p[k][i] = (const uint8_t *)g.plane[k];
        sizes[i] = (uint64_t *)out_sizes_dev[i];
    }
    g0->pixels = p0.plane[0];
    g0->width = p0.width; g0->height = p0.height; g0->row_stride = p0.row_stride; g0->bottom_up = p0.bottom_up;
    g0->channel_order = kOrderPlanar; g0->quality = p0.quality;
    return JPEGAMD_OK;
}

// `count` planar pictures: the argument checks, then the grayscale or the colour batch with the planes as the pixel source.
extern "C" int32_t jpegamd_encode_planar_batch_async(JpegAmdEncoder *e, const JpegAmdPlanarImage *imgs, int32_t count, int32_t subsampling,
                                                     void *const *outs_dev, uint64_t out_capacity, void *const *out_sizes_dev,
                                                     void *stream_) {
    // the arguments first: nothing of the context is read before they are known to be good
    JpegAmdImage g0;
    PlaneSet ps;
    uint64_t *sizes[kMaxBatch];
    if (int32_t rc = planar_args(e, imgs, count, subsampling, true, outs_dev, out_sizes_dev, &g0, &ps, sizes)) return rc;
    if (subsampling == 0) return gray_batch(e, g0, ps, count, outs_dev, out_capacity, sizes, 1, stream_);
    return color_batch(e, g0, ps, count, subsampling, outs_dev, out_capacity, sizes, stream_);
}

// The arguments of a YCbCr batch, checked before anything of the context is read (outs_dev / out_sizes_dev: null for an entry that
// writes no files) -> the Y planes as a GRAY picture and the caller's chroma.
static int32_t ycbcr_args(const JpegAmdEncoder *e, const JpegAmdYCbCrImage *imgs, int32_t count, int32_t subsampling, int32_t sample_range,
                          int32_t sample_format, int32_t matrix, void *const *outs_dev, void *const *out_sizes_dev, bool files,
                          JpegAmdImage *g0, PlaneSet *ps, YccSource *ycc, uint64_t **sizes) {
    if (!e || !imgs || (files && (!outs_dev || !out_sizes_dev)) || count < 1 || count > kMaxBatch) return JPEGAMD_ERR_ARG;
    if (!sub_valid(subsampling)) return JPEGAMD_ERR_ARG;
    if (matrix != JPEGAMD_MATRIX_BT601 && matrix != JPEGAMD_MATRIX_BT709) return JPEGAMD_ERR_ARG;
    const int64_t bps = sample_format == JPEGAMD_SAMPLES_8 ? 1 : 2;   // bytes per sample
    const JpegAmdYCbCrImage &p0 = imgs[0];
    const bool packed = is_packed422(p0.chroma_layout);               // y is the packed plane; cb, cr and c_stride are not looked at
    if (!ycbcr_kind_valid(p0.chroma_layout, sample_format, sample_range)) return JPEGAMD_ERR_ARG;
    if (packed && subsampling != JPEGAMD_SUBSAMPLE_422) return JPEGAMD_ERR_ARG;
    if (p0.width <= 0 || p0.height <= 0 || p0.width > 65535 || p0.height > 65535) return JPEGAMD_ERR_ARG;
    const bool pair = p0.chroma_layout != JPEGAMD_CHROMA_PLANES && !packed;
    const int cw = chroma_geom(p0.width, p0.height, subsampling).cw;
    if (packed ? p0.y_stride < 4 * cw : (p0.y_stride < bps * p0.width || p0.c_stride < bps * (pair ? 2 * cw : cw))) return JPEGAMD_ERR_ARG;
    *ps = PlaneSet{};
    *ycc = YccSource{};
    ycc->layout = p0.chroma_layout; ycc->c_stride = packed ? p0.y_stride : p0.c_stride;
    ycc->format = sample_format; ycc->range = sample_range; ycc->matrix = matrix;
    for (int i = 0; i < count; ++i) {
        const JpegAmdYCbCrImage &g = imgs[i];
        if ((files && (!outs_dev[i] || !out_sizes_dev[i])) || !g.y || (!packed && (!g.cb || (!pair && !g.cr)))) return JPEGAMD_ERR_ARG;
        if (g.width != p0.width || g.height != p0.height || g.y_stride != p0.y_stride || (!packed && g.c_stride != p0.c_stride) ||
            g.chroma_layout != p0.chroma_layout || g.quality != p0.quality)
            return JPEGAMD_ERR_ARG;
        ps->p[0][i] = (const uint8_t *)g.y;
        ycc->cb[i] = (const uint8_t *)(packed ? g.y : g.cb);
        ycc->cr[i] = (pair || packed) ? nullptr : (const uint8_t *)g.cr;
        if (files) sizes[i] = (uint64_t *)out_sizes_dev[i];
    }
    g0->pixels = p0.y;
    g0->width = p0.width; g0->height = p0.height; g0->row_stride = p0.y_stride; g0->bottom_up = 0;
    g0->channel_order = JPEGAMD_ORDER_GRAY; g0->quality = p0.quality;
    return JPEGAMD_OK;
}

// `count` YCbCr pictures: the argument checks, then the colour batch with the Y planes as its one-sample source and the caller's chroma.
// sample_range: JPEGAMD_RANGE_FULL -- the samples are coded as given -- or JPEGAMD_RANGE_LIMITED: every launch expands them on read.
// sample_format: JPEGAMD_SAMPLES_8, or 10-bit samples in 16-bit words (MSB- or LSB-aligned), which every launch narrows on read.
// matrix: JPEGAMD_MATRIX_BT601 -- exactly that -- or JPEGAMD_MATRIX_BT709: one pass (k_ycbcr_matrix_batch) applies the same maps and
// the matrix and leaves full-range BT.601 planes in context scratch, which the launches then read.
extern "C" int32_t jpegamd_encode_ycbcr_matrix_batch_async(JpegAmdEncoder *e, const JpegAmdYCbCrImage *imgs, int32_t count, int32_t subsampling,
                                                           int32_t sample_range, int32_t sample_format, int32_t matrix, void *const *outs_dev,
                                                           uint64_t out_capacity, void *const *out_sizes_dev, void *stream_) {
    // the arguments first: nothing of the context is read before they are known to be good
    JpegAmdImage g0;
    PlaneSet ps;
    YccSource ycc;
    uint64_t *sizes[kMaxBatch];
    if (int32_t rc = ycbcr_args(e, imgs, count, subsampling, sample_range, sample_format, matrix, outs_dev, out_sizes_dev, true, &g0, &ps, &ycc, sizes))
        return rc;
    return color_batch(e, g0, ps, count, subsampling, outs_dev, out_capacity, sizes, stream_, &ycc);
}

// Host-only (tests): the six integers of a matrix and the shift, as k_ycbcr_matrix_batch applies them (BT601: the identity, which no
// kernel applies).  Not part of the public header.
extern "C" int32_t jpegamd_debug_matrix_coeffs(int32_t matrix, int32_t *out /*[7]*/) {
    if (!out || (matrix != JPEGAMD_MATRIX_BT601 && matrix != JPEGAMD_MATRIX_BT709)) return JPEGAMD_ERR_ARG;
    for (int k = 0; k < 6; ++k) out[k] = matrix == JPEGAMD_MATRIX_BT709 ? kMatrix709[k] : kMatrix601[k];
    out[6] = kMatrixShift;
    return JPEGAMD_OK;
}

// Tests: the pass of a BT.709 batch alone, into the same scratch, and its planes copied tightly packed into the caller's DEVICE buffers
// (y_out: count x height x width bytes; cb_out, cr_out: count x ch x cw).  Returns when the copies are done.  Only JPEGAMD_MATRIX_BT709
// has a pass.  Not part of the public header.
extern "C" int32_t jpegamd_debug_ycbcr_matrix_planes(JpegAmdEncoder *e, const JpegAmdYCbCrImage *imgs, int32_t count, int32_t subsampling,
                                                     int32_t sample_range, int32_t sample_format, int32_t matrix, void *y_out, void *cb_out,
                                                     void *cr_out, void *stream_) {
    JpegAmdImage g0;
    PlaneSet ps;
    YccSource ycc;
    if (!y_out || !cb_out || !cr_out) return JPEGAMD_ERR_ARG;
    if (int32_t rc = ycbcr_args(e, imgs, count, subsampling, sample_range, sample_format, matrix, nullptr, nullptr, false, &g0, &ps, &ycc, nullptr))
        return rc;
    if (matrix != JPEGAMD_MATRIX_BT709) return JPEGAMD_ERR_ARG;
    const ChromaGeom cg = chroma_geom(g0.width, g0.height, subsampling);
    const MatrixScratch ms = matrix_scratch(g0.width, g0.height, count, cg.plane_bytes);
    if (int32_t rc = color_batch_alloc(e, ms.total, 0)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    if (launch_matrix_pass(e, g0, ps, ycc, count, subsampling, cg, ms, stream, nullptr)) return JPEGAMD_ERR_HIP;
    const uint8_t *base = e->color.bplanes;
    for (int i = 0; i < count; ++i) {
        HIP_TRY(hipMemcpy2DAsync((uint8_t *)y_out + (size_t)i * g0.width * g0.height, (size_t)g0.width, base + ms.y_off + (size_t)i * ms.yplane_bytes,
                                 (size_t)ms.ypitch, (size_t)g0.width, (size_t)g0.height, hipMemcpyDeviceToDevice, stream));
        for (int k = 0; k < 2; ++k)
            HIP_TRY(hipMemcpy2DAsync((uint8_t *)(k ? cr_out : cb_out) + (size_t)i * cg.cw * cg.ch, (size_t)cg.cw, base + (size_t)(2 * i + k) * cg.plane_bytes,
                                     (size_t)cg.pitch, (size_t)cg.cw, (size_t)cg.ch, hipMemcpyDeviceToDevice, stream));
    }
    HIP_TRY(hipStreamSynchronize(stream));
    return JPEGAMD_OK;
}

// The BT.601 matrix: the entry above with JPEGAMD_MATRIX_BT601 -- no pass, no scratch, the launches read the caller's planes.
extern "C" int32_t jpegamd_encode_ycbcr_samples_batch_async(JpegAmdEncoder *e, const JpegAmdYCbCrImage *imgs, int32_t count, int32_t subsampling,
                                                            int32_t sample_range, int32_t sample_format, void *const *outs_dev,
                                                            uint64_t out_capacity, void *const *out_sizes_dev, void *stream_) {
    return jpegamd_encode_ycbcr_matrix_batch_async(e, imgs, count, subsampling, sample_range, sample_format, JPEGAMD_MATRIX_BT601, outs_dev,
                                                   out_capacity, out_sizes_dev, stream_);
}

// One byte per sample: the entry above with JPEGAMD_SAMPLES_8.
extern "C" int32_t jpegamd_encode_ycbcr_range_batch_async(JpegAmdEncoder *e, const JpegAmdYCbCrImage *imgs, int32_t count, int32_t subsampling,
                                                          int32_t sample_range, void *const *outs_dev, uint64_t out_capacity,
                                                          void *const *out_sizes_dev, void *stream_) {
    return jpegamd_encode_ycbcr_samples_batch_async(e, imgs, count, subsampling, sample_range, JPEGAMD_SAMPLES_8, outs_dev, out_capacity,
                                                    out_sizes_dev, stream_);
}

// Full-range samples: the entry above with JPEGAMD_RANGE_FULL.
extern "C" int32_t jpegamd_encode_ycbcr_batch_async(JpegAmdEncoder *e, const JpegAmdYCbCrImage *imgs, int32_t count, int32_t subsampling,
                                                    void *const *outs_dev, uint64_t out_capacity, void *const *out_sizes_dev,
                                                    void *stream_) {
    return jpegamd_encode_ycbcr_range_batch_async(e, imgs, count, subsampling, JPEGAMD_RANGE_FULL, outs_dev, out_capacity, out_sizes_dev, stream_);
}

// ---------------------------------------------------------------------------------------------------------
// Colour in ONE scan of interleaved MCUs.  Per picture and component the stage-tap build of k_tile_encode stores
// the quantised zigzag coefficients (tap_zz) into context scratch -- one launch per picture and component: the tap's block index has
// no picture term -- and k_picture_stats takes the exact-order fallback counts from the records those launches leave.  k_mcu_segments
// codes the planes in MCU order into the path's OWN segment arrays, the unchanged k_finalize writes prefix, scan and EOI straight
// into the caller's buffers, k_mcu_totals sums the call's record.  A large batch goes through in groups of pictures that bound the
// scratch.  jpegamd_encoder_set_pipeline has no effect here: k_stitch reads tile records.
// With JPEGAMD_HUFFMAN_OPTIMIZED on the context k_mcu_histogram and k_huff_optimal run in front of k_mcu_segments,
// which then codes every picture with its own tables, and the restart writer stands in for k_finalize at every interval: it reads a
// prefix and its length per picture.
// ---------------------------------------------------------------------------------------------------------
constexpr int kSubNone = 0;              // `subsampling` of a scan of ONE component (the grayscale file of DESIGN.md 4.6.11): no entry takes it from a caller
struct McuGeometry {
    int comps;                          // components of the scan: 3, or 1 -- the MCU is then one block, the MCU grid the block grid
    int hs, vs, bw, bh, mx, my, seg_mcus, num_segs, num_segs_pad;
    ChromaGeom chroma;
    size_t coef_per_pic;                // int16 elements
    // restart intervals (restart > 0: 4.6.8): the scan's intervals, the segments of each, the picture's last segment that holds MCUs
    int restart, intervals, segs_per_interval, last_seg;
    int64_t segs64;                     // num_segs before it is narrowed (restart = 1 on the largest pictures: beyond an int's reach once padded and batched)
    size_t cap_words;                   // words reserved per segment string
};
// restart: the interval in MCUs, 0 for none.
static McuGeometry mcu_geometry(int w, int h, int sub, int restart = 0) {
    McuGeometry g;
    g.comps = sub == kSubNone ? 1 : 3;
    g.hs = sub == JPEGAMD_SUBSAMPLE_444 || sub == kSubNone ? 1 : 2;
    g.vs = sub == JPEGAMD_SUBSAMPLE_420 ? 2 : 1;
    g.bw = (w + 7) / 8; g.bh = (h + 7) / 8;
    g.mx = (g.bw + g.hs - 1) / g.hs; g.my = (g.bh + g.vs - 1) / g.vs;
    g.chroma = chroma_geom(w, h, sub);
    g.seg_mcus = mcu_seg_mcus(g.hs, g.vs, g.comps);
    const int bpm = mcu_blocks_per_mcu(g.hs, g.vs, g.comps);
    const int64_t mcus = (int64_t)g.mx * g.my;
    g.restart = restart;
    g.intervals = restart ? (int)((mcus + restart - 1) / restart) : 1;
    g.segs_per_interval = (int)((std::min<int64_t>(restart ? restart : mcus, mcus) + g.seg_mcus - 1) / g.seg_mcus);
    g.segs64 = (int64_t)g.intervals * g.segs_per_interval;          // (no restart: ceil(mcus / seg_mcus), as ever)
    g.num_segs = (int)std::min<int64_t>(g.segs64, INT32_MAX / 2);
    g.num_segs_pad = (g.num_segs + kSegGroup - 1) / kSegGroup * kSegGroup;
    const int64_t in_last = mcus - (int64_t)(g.intervals - 1) * (restart ? restart : 0);     // MCUs of the last interval
    g.last_seg = (int)std::min<int64_t>((int64_t)(g.intervals - 1) * g.segs_per_interval + (in_last + g.seg_mcus - 1) / g.seg_mcus - 1, INT32_MAX / 2);
    g.cap_words = restart ? (size_t)mcu_restart_cap_words(std::min(restart, g.seg_mcus) * bpm) : (size_t)kSegCapWords;
    g.coef_per_pic = ((size_t)g.bw * g.bh + (g.comps == 1 ? 0 : 2 * (size_t)g.mx * g.my)) * 64;
    return g;
}
// Bytes of the path's scratch one picture takes in the group budget: its coefficient planes and its segment strings; with restart
// intervals -- segments may be as short as one MCU -- the per-segment numbers as well, the coder's and the writer's (56 bytes).
// `writer`: the call goes through k_mcu_restart_offsets / k_mcu_restart_write (restart intervals, or a picture's own tables).
static uint64_t mcu_scratch_per_pic(const McuGeometry &g, bool writer) {
    const uint64_t segs = (uint64_t)(g.segs64 + kSegGroup - 1) / kSegGroup * kSegGroup;
    return (uint64_t)g.coef_per_pic * sizeof(int16_t) + segs * (uint64_t)g.cap_words * sizeof(uint32_t) + (writer ? segs * 56u : 0u);
}

extern "C" uint64_t jpegamd_max_jfif_bytes_interleaved(int32_t width, int32_t height, int32_t subsampling) {
    if (width <= 0 || height <= 0 || width > 65535 || height > 65535 || !sub_valid(subsampling)) return 0;
    const McuGeometry g = mcu_geometry(width, height, subsampling);
    // the prefix, every block of every MCU (pad blocks too) at the worst case with every byte stuffed, the flush byte, EOI
    return kColorPrefixMax + scan_bound((uint64_t)g.mx * (uint64_t)g.my * (uint64_t)(g.hs * g.vs + 2), kMaxBlockBitsColor) + 2 + 16;
}

constexpr int kMcuDriBytes = 6;          // FF DD 00 04 hi lo

extern "C" uint64_t jpegamd_max_jfif_bytes_interleaved_restart(int32_t width, int32_t height, int32_t subsampling, int32_t restart_interval) {
    const uint64_t plain = jpegamd_max_jfif_bytes_interleaved(width, height, subsampling);
    if (!plain || restart_interval < 0 || restart_interval > 65535) return 0;
    if (!restart_interval) return plain;
    // The plain bound holds the scan's bits rounded up to a byte ONCE, every byte stuffed.  With n intervals the DRI segment is 6
    // bytes, and every interval but the last rounds up by itself -- at most one more byte --, may have that byte stuffed, and ends
    // with a two-byte marker: 4 (n - 1).
    const McuGeometry g = mcu_geometry(width, height, subsampling, restart_interval);
    return plain + kMcuDriBytes + 4 * (uint64_t)(g.intervals - 1);
}

constexpr int kMcuSosBytes = 14;
constexpr size_t kMcuScratchBudget = (size_t)4 << 30;       // coefficient planes + segment strings of one group of pictures

// ---- progressive files ----
// interleaved_batch's `progressive`: one scan / seven scans, Annex K / seven scans with runs and own tables / the ten scans of successive approximation
constexpr int kProgNone = 0, kProgStandard = 1, kProgRuns = 2, kProgSuccessive = 3, kProgScript = 4;      // kProgScript: a caller's scan script (4.6.15)

// The scan script: what every scan of a progressive file codes, in the file's order.  mask: the scan's
// components (bit 0 Y, bit 1 Cb, bit 2 Cr; 7: the three interleaved); table: the scan's first table in the file's table order (a DC
// scan has one per table class of its components: Y, then Cb + Cr), -1 for a scan of raw bits.  The files of 4.6.12 and 4.6.13 are
// the first script (4.6.12 reads no table numbers), the file of 4.6.14 -- libjpeg's jpeg_simple_progression for YCbCr -- the second;
// id 2 is a caller's (4.6.15: prog_script_from), whose SOS segments are uploaded per call.  comps: the file's components, 3 or 1.
struct ProgScan { uint8_t mask; uint8_t ss, se, ah, al; int8_t table; };
struct ProgScript { int id, scans, tables, comps; ProgScan scan[kProgScansMax]; };
static const ProgScript kScriptSpectral = {0, kProgScans, kProgTables, 3,
    {{7, 0, 0, 0, 0, 0}, {1, 1, 5, 0, 0, 2}, {2, 1, 5, 0, 0, 3}, {4, 1, 5, 0, 0, 4}, {1, 6, 63, 0, 0, 5}, {2, 6, 63, 0, 0, 6}, {4, 6, 63, 0, 0, 7}}};
static const ProgScript kScriptSuccessive = {1, 10, 10, 3,
    {{7, 0, 0, 0, 1, 0}, {1, 1, 5, 0, 2, 2}, {4, 1, 63, 0, 1, 3}, {2, 1, 63, 0, 1, 4}, {1, 6, 63, 0, 2, 5},
     {1, 1, 63, 2, 1, 6}, {7, 0, 0, 1, 0, -1}, {4, 1, 63, 1, 0, 7}, {2, 1, 63, 1, 0, 8}, {1, 1, 63, 1, 0, 9}}};
static_assert(kProgScans <= kProgScansMax && kProgTables <= kProgTablesMax, "the scripts fit the kernels' maxima");
static_assert(JPEGAMD_MAX_SCANS == kProgScansMax && JPEGAMD_MAX_SCANS == kProgTablesMax, "the public limit is the kernels'");
static const ProgScript &prog_script(int progressive) { return progressive == kProgSuccessive ? kScriptSuccessive : kScriptSpectral; }
static int popcount3(int mask) { return (mask & 1) + ((mask >> 1) & 1) + ((mask >> 2) & 1); }
// the tables a scan owns: a first DC scan one per table class among its components, an AC scan one, a DC refinement scan none
static int prog_scan_tables(const ProgScan &s) { return s.ss ? 1 : (s.ah ? 0 : ((s.mask & 1) ? 1 : 0) + ((s.mask & 6) ? 1 : 0)); }
// The SOS segment of a script's scan, 8 + 2 n bytes for n components: the selectors ascending, Y with the tables 0 / 0, Cb and Cr 1 / 1.
static int prog_sos(const ProgScan &s, uint8_t out[16]) {
    const int nc = popcount3(s.mask);
    int n = 0;
    out[n++] = 0xFF; out[n++] = 0xDA; out[n++] = 0x00; out[n++] = (uint8_t)(6 + 2 * nc); out[n++] = (uint8_t)nc;
    for (int c = 0; c < 3; ++c)
        if ((s.mask >> c) & 1) { out[n++] = (uint8_t)(c + 1); out[n++] = c ? 0x11 : 0x00; }
    out[n++] = s.ss; out[n++] = s.se; out[n++] = (uint8_t)((s.ah << 4) | s.al);
    return n;
}

// T.81 G.1.1.1 and libjpeg's validate_script (include/jpeg_compression.h has the rules).
extern "C" int32_t jpegamd_validate_scan_script(const JpegAmdScan *scans, int32_t count, int32_t file_components, int32_t *bad_scan) {
    int32_t bad_local;
    int32_t &bad = bad_scan ? *bad_scan : bad_local;
    bad = -1;
    if (!scans || count < 1 || count > JPEGAMD_MAX_SCANS || (file_components != 1 && file_components != 3)) return JPEGAMD_ERR_ARG;
    int8_t last_al[3][64];                                           // the al of the last scan that coded (component, coefficient); -1: none did
    std::memset(last_al, -1, sizeof(last_al));
    const int full = file_components == 3 ? 7 : 1;
    int tables = 0;
    for (int k = 0; k < count; ++k) {
        const JpegAmdScan &c = scans[k];
        bad = k;
        if (c.components == 0 || (c.components & ~full)) return JPEGAMD_ERR_ARG;
        if (c.ss == 0 ? c.se != 0 : (popcount3(c.components) != 1 || c.se < c.ss || c.se > 63)) return JPEGAMD_ERR_ARG;
        if (c.al > 13 || (c.ah != 0 && c.ah != c.al + 1)) return JPEGAMD_ERR_ARG;
        for (int j = 0; j < 3; ++j) {
            if (!((c.components >> j) & 1)) continue;
            if (c.ss > 0 && last_al[j][0] < 0) return JPEGAMD_ERR_ARG;           // an AC scan in front of the component's first DC scan
            for (int i = c.ss; i <= c.se; ++i) {
                // a first scan of it: Ah = 0; a refinement: of the bit below the last one coded (a coefficient coded down to bit 0 is done)
                if (last_al[j][i] < 0 ? c.ah != 0 : (c.ah != (uint8_t)last_al[j][i] || c.ah != c.al + 1)) return JPEGAMD_ERR_ARG;
                last_al[j][i] = (int8_t)c.al;
            }
        }
        const ProgScan ps = {c.components, c.ss, c.se, c.ah, c.al, 0};
        tables += prog_scan_tables(ps);
    }
    bad = -1;
    if (tables > JPEGAMD_MAX_SCANS) return JPEGAMD_ERR_ARG;
    for (int j = 0; j < file_components; ++j) if (last_al[j][0] < 0) return JPEGAMD_ERR_ARG;
    return JPEGAMD_OK;
}

// libjpeg's jpeg_simple_progression: the ten scans of a YCbCr file (kScriptSuccessive), the six of a grayscale file.
static const JpegAmdScan kDefaultScansColor[10] = {{7, 0, 0, 0, 1}, {1, 1, 5, 0, 2}, {4, 1, 63, 0, 1}, {2, 1, 63, 0, 1}, {1, 6, 63, 0, 2},
                                                   {1, 1, 63, 2, 1}, {7, 0, 0, 1, 0}, {4, 1, 63, 1, 0}, {2, 1, 63, 1, 0}, {1, 1, 63, 1, 0}};
static const JpegAmdScan kDefaultScansGray[6] = {{1, 0, 0, 0, 1}, {1, 1, 5, 0, 2}, {1, 6, 63, 0, 2}, {1, 1, 63, 2, 1}, {1, 0, 0, 1, 0}, {1, 1, 63, 1, 0}};
// A caller's script as the internal one, tables numbered in file order; scans == NULL with count 0: the default script of the
// file's component count.  false: the script breaks a rule.
static bool prog_script_from(const JpegAmdScan *scans, int32_t count, int comps, ProgScript *out) {
    if (!scans && count == 0) { scans = comps == 3 ? kDefaultScansColor : kDefaultScansGray; count = comps == 3 ? 10 : 6; }
    if (jpegamd_validate_scan_script(scans, count, comps, nullptr) != JPEGAMD_OK) return false;
    ProgScript sc = {};
    sc.id = 2; sc.scans = count; sc.comps = comps;
    for (int k = 0; k < count; ++k) {
        ProgScan &c = sc.scan[k];
        c.mask = scans[k].components; c.ss = scans[k].ss; c.se = scans[k].se; c.ah = scans[k].ah; c.al = scans[k].al;
        const int nt = prog_scan_tables(c);
        c.table = nt ? (int8_t)sc.tables : (int8_t)-1;
        sc.tables += nt;
    }
    *out = sc;
    return true;
}

// What a progressive call keeps on the device besides the slots: k_finalize's two records (scan 1's; the scans into slots share the
// other), every scan's size and sums per picture of the group -- [scans][kMaxBatch] arrays one behind the other, so a call clears as
// many bytes as its script has scans for --, and behind the records of the longest script the SOS segments of every script's
// scans, 16 bytes apart.
struct ProgMeta {
    ScanStats *scan_stats;              // [2]
    uint64_t *size;                     // [scans][kMaxBatch]
    unsigned long long *sums;           // [scans][kMaxBatch][2]
    unsigned long long *writer_sums;    // [scans][kMaxBatch][kMcuPicSums] k_mcu_restart_offsets' (4.6.13, 4.6.14)
    size_t record_bytes;                // all of the above
};
static_assert(sizeof(ScanStats) % 8 == 0, "the arrays behind the two records are aligned");
constexpr size_t prog_meta_bytes(int scans) { return 2 * sizeof(ScanStats) + (size_t)scans * kMaxBatch * (8 + 16 + 8 * kMcuPicSums); }
constexpr size_t kProgMetaSos = prog_meta_bytes(kProgScansMax), kProgMetaAlloc = kProgMetaSos + 3 * kProgScansMax * 16;      // (the two built-in scripts', a caller's)
static ProgMeta prog_meta(uint8_t *base, int scans) {
    ProgMeta m;
    m.scan_stats = reinterpret_cast<ScanStats *>(base);
    m.size = reinterpret_cast<uint64_t *>(base + 2 * sizeof(ScanStats));
    m.sums = reinterpret_cast<unsigned long long *>(m.size + (size_t)scans * kMaxBatch);
    m.writer_sums = m.sums + (size_t)scans * kMaxBatch * 2;
    m.record_bytes = prog_meta_bytes(scans);
    return m;
}
static const uint8_t *prog_meta_sos(const uint8_t *base, const ProgScript &sc) { return base + kProgMetaSos + (size_t)sc.id * kProgScansMax * 16; }

// The slots of the scans 2 .. of one picture: each holds the scan's header, the scan at its bound (every block of the component's
// plane at the band's worst case, every byte stuffed, the flush byte), EOI, and what k_scans_concat reads behind them in 16-byte steps.
// own_tables (4.6.13): the scan's DHT segment in front of its SOS; a coefficient of a band then costs at most 16 + 10 bits, a run's
// symbol 16 + 8, paid for by the zero coefficient se of the block that starts it -- below the 27 of prog_band_bits either way.
// Successive approximation: a first scan's coefficient costs no more (shorter amplitudes); a refinement scan's at most 17, its run's
// symbol at a coefficient se that costs 1 (kMaxBlockBitsRefine): below 27 a coefficient again; the DC refinement scan, the one
// three-component scan in a slot, is 1 bit a block of an MCU, pad blocks included.
constexpr int kProgDhtMax = 21 + 170;       // an AC table of a scan: 160 run/size symbols, ZRL, EOB0 .. EOB8
static_assert(kProgDhtMax + kSosBytes <= kMcuPrefixSlot, "a scan's header fits its slot");
static_assert(kMaxBlockBitsRefine <= 63 * 27, "a refinement scan's block is within the slot's 27 bits a coefficient");
struct ProgSlots { uint64_t off[kProgScansMax], cap[kProgScansMax], pic_bytes; };
// the blocks a scan codes: every block of every MCU of an interleaved scan, pad blocks included; a component's own blocks of a scan of one
static uint64_t prog_scan_blocks(const McuGeometry &g, const ProgScan &c) {
    const uint64_t mcus = (uint64_t)g.mx * g.my;
    if (popcount3(c.mask) == 1) return c.mask == 1 ? (uint64_t)g.bw * g.bh : mcus;
    return mcus * (uint64_t)((c.mask & 1 ? g.hs * g.vs : 0) + popcount3(c.mask & 6));
}
// the DHT segments in front of a scan's SOS at most: a DC table 33 bytes, an AC table kProgDhtMax
static uint64_t prog_scan_dht_max(const ProgScan &c) { return c.ss ? kProgDhtMax : 33u * (uint64_t)prog_scan_tables(c); }
static ProgSlots prog_slots(const McuGeometry &g, const ProgScript &sc, bool own_tables = false) {
    ProgSlots s = {};
    for (int k = 1; k < sc.scans; ++k) {
        const ProgScan &c = sc.scan[k];
        const uint64_t nb = prog_scan_blocks(g, c);
        // a DC scan (4.6.15: a first one may live in a slot): 27 bits a block, a refinement 1; (prog_band_bits for the bands of 4.6.12)
        const uint64_t bits = c.ss == 0 ? (c.ah ? 1u : 27u) : (uint64_t)(c.se - c.ss + 1) * 27u;
        s.cap[k] = (own_tables ? prog_scan_dht_max(c) : 0) + (8 + 2 * popcount3(c.mask)) + scan_bound(nb, bits) + 2;
        s.off[k] = s.pic_bytes;
        s.pic_bytes += round_up((size_t)s.cap[k] + 64, 256);
    }
    return s;
}
static_assert(prog_band_bits(0) == 5 * 27 && prog_band_bits(1) == 58 * 27, "the slots of the seven-scan files are what they were");

extern "C" uint64_t jpegamd_max_jfif_bytes_progressive(int32_t width, int32_t height, int32_t subsampling) {
    // The one-scan bound holds every block of every MCU (pad blocks too) at kMaxBlockBitsColor bits -- no less than its DC
    // difference and its two bands cost together (prog_band_bits) --, every byte stuffed, ONE rounding up to a byte, and EOI.
    // Seven scans add six SOS segments of kSosBytes, and six more roundings of at most one byte each, which may be stuffed.
    const uint64_t plain = jpegamd_max_jfif_bytes_interleaved(width, height, subsampling);
    return plain ? plain + (uint64_t)(kProgScans - 1) * (kSosBytes + 2) : 0;
}

extern "C" uint64_t jpegamd_max_jfif_bytes_progressive_optimized(int32_t width, int32_t height, int32_t subsampling) {
    // The scans: a DC difference is at most 16 + 11 bits with a table of the picture's own; a non-zero AC coefficient 16 + 10 (sizes
    // 1 .. 10: the reasoning of jpegamd_max_jfif_bytes_gray_scan's optimised mode); a ZRL at most 16 bits for sixteen zero
    // coefficients; a run's symbol at most 16 + 8 bits (EOB8 and eight more), and only a block whose coefficient se is zero starts one
    // -- so every coefficient of a band pays for at most 26 bits, and a block for 27 + 63 x 26 = kMaxBlockBitsOptimized over all
    // scans, below the kMaxBlockBitsColor per block that jpegamd_max_jfif_bytes_progressive holds -- with its seven roundings, its
    // stuffing, six SOS segments and EOI.
    // The headers: that bound holds kColorPrefixMax for a prefix with the four Annex K DHT segments (kStdDhtBytes).  Here a DC table
    // has at most 12 symbols, DHT 21 + 12 = 33 bytes, and an AC table at most 160 run/size symbols, ZRL and EOB0 .. EOB8 = 170, DHT
    // 21 + 170 = kProgDhtMax: 2 x 33 + 6 x 191 = 1212 bytes against 432 -- 780 more.
    static_assert(2 * 33 + 6 * kProgDhtMax - kStdDhtBytes == 780 && kMaxBlockBitsOptimized <= kMaxBlockBitsColor, "the bound's derivation");
    const uint64_t std_tables = jpegamd_max_jfif_bytes_progressive(width, height, subsampling);
    return std_tables ? std_tables + 780 : 0;
}

// The ten scans of successive approximation.  A Y block over the scans that touch it: its DC difference at most
// 16 + 11 bits (scan 1), its DC refinement bit (scan 7), its 63 coefficients in the first scans 2 and 5 at 26 bits each (the
// reasoning above: a point transform only shortens amplitudes, and either scan's run symbol is paid by its own zero coefficient se),
// and kMaxBlockBitsRefine in each of the refinement scans 6 and 10: 27 + 1 + 63 x 26 + 2 x 1079 = kMaxBlockBitsSuccessive.  A chroma
// block has one refinement scan and costs less.  So: the one-scan bound's form -- every block of every MCU, pad blocks too, at
// that many bits, every byte stuffed, one rounding, EOI, kColorPrefixMax for the head with 432 bytes of DHT and a 14-byte SOS --,
// nine more roundings that may be stuffed, eight SOS of kSosBytes and one of 14, and the DHT segments of ten tables, 2 x 33 + 8 x
// kProgDhtMax = 1594 bytes against 432.
constexpr int kMaxBlockBitsSuccessive = 27 + 1 + 63 * 26 + 2 * kMaxBlockBitsRefine;      // 3824
extern "C" uint64_t jpegamd_max_jfif_bytes_progressive_successive(int32_t width, int32_t height, int32_t subsampling) {
    static_assert(kMaxBlockBitsSuccessive == 3824 && 2 * 33 + 8 * kProgDhtMax - kStdDhtBytes == 1162, "the bound's derivation");
    if (width <= 0 || height <= 0 || width > 65535 || height > 65535 || !sub_valid(subsampling)) return 0;
    const McuGeometry g = mcu_geometry(width, height, subsampling);
    const uint64_t blocks = (uint64_t)g.mx * (uint64_t)g.my * (uint64_t)(g.hs * g.vs + 2);
    return kColorPrefixMax + scan_bound(blocks, kMaxBlockBitsSuccessive) + 2 + 16 + 9 * 2 + 8 * kSosBytes + 14 + 1162;
}

// The path's scratch for `group` pictures of geometry g: allocated on the first call, grown when a call needs more.
// `writer`: the restart writer's arrays as well.  `own_tables`: the scratch of `own_tables` pictures with tables of their own.
static int32_t mcu_alloc(JpegAmdEncoder *e, const McuGeometry &g, int group, bool writer, int own_tables) {
    auto &m = e->mcu;
    if (!m.hdr) {
        HIP_TRY(hipMalloc((void **)&m.hdr, 1024));
        HIP_TRY(hipMalloc((void **)&m.scan_stats, sizeof(ScanStats)));
    }
    const size_t coef = (size_t)group * g.coef_per_pic, segs = (size_t)group * (size_t)g.num_segs_pad;
    const size_t words = (segs + 1) * g.cap_words;                    // (strings of either length share the array: a call sets its own stride)
    if (int32_t rc = grow_scratch(e, &m.coef, &m.coef_cap, coef)) return rc;
    if (segs > m.segs_cap || words > m.words_cap) {                   // (grow_scratch's steps over a set of arrays)
        if (int32_t rc = wait_pending(e)) return rc;
        const size_t new_segs = std::max(segs, m.segs_cap), new_words = std::max(words, m.words_cap);
        free_seg_arrays(&m.seg);
        m.segs_cap = m.words_cap = 0;
        if (int32_t rc = alloc_seg_arrays(&m.seg, new_segs, new_words, false)) return rc;
        m.segs_cap = new_segs; m.words_cap = new_words;
    }
    if (own_tables > m.hcap) {
        if (int32_t rc = wait_pending(e)) return rc;
        hipFree(m.hcounts); hipFree(m.htabs); hipFree(m.hprefix); hipFree(m.hprefix_len); hipFree(m.hres);
        m.hcounts = nullptr; m.htabs = nullptr; m.hprefix = nullptr; m.hprefix_len = nullptr; m.hres = nullptr; m.hcap = 0; m.hlast = 0;
        const size_t n = (size_t)own_tables;
        HIP_TRY(hipMalloc((void **)&m.hcounts, n * kMcuTabWords * sizeof(unsigned long long)));
        HIP_TRY(hipMalloc((void **)&m.htabs, n * kMcuTabWords * sizeof(uint32_t)));
        HIP_TRY(hipMalloc((void **)&m.hprefix, n * kMcuPrefixSlot));
        HIP_TRY(hipMalloc((void **)&m.hprefix_len, n * sizeof(uint32_t)));
        HIP_TRY(hipMalloc((void **)&m.hres, 4 * n * kHuffResBytes));
        m.hcap = own_tables;
    }
    if (writer && segs > m.rst_cap) {
        if (int32_t rc = wait_pending(e)) return rc;
        hipFree(m.rst_words); hipFree(m.rst_pos); m.rst_words = nullptr; m.rst_pos = nullptr; m.rst_cap = 0;
        if (!m.rst_pic_sums) HIP_TRY(hipMalloc((void **)&m.rst_pic_sums, kMaxBatch * kMcuPicSums * sizeof(unsigned long long)));
        HIP_TRY(hipMalloc((void **)&m.rst_words, 3 * segs * sizeof(uint32_t)));
        HIP_TRY(hipMalloc((void **)&m.rst_pos, segs * sizeof(uint64_t)));
        m.rst_cap = segs;
    }
    return JPEGAMD_OK;
}

// The colour prefix up to its DHTs, [DRI with the restart interval,] then the SOS of all three components (Y: tables 0 / 0, Cb and
// Cr: 1 / 1).  One component (kSubNone): the grayscale prefix up to its two DHTs, [DRI,] its SOS.
// progressive (colour, no restart intervals): the frame header's marker is SOF2, and the SOS is the DC scan's (Ss = Se = 0).
constexpr int kColorSofOffset = 2 + 18 + 134;       // SOI, APP0, DQT with two tables
constexpr int kGraySofOffset = 2 + 18 + 69;         // ... with one: the one-component head (a grayscale progressive file)
static int32_t prepare_mcu_prefix(JpegAmdEncoder *e, const JpegAmdImage *img, int sub, int restart, bool progressive = false) {
    auto &m = e->mcu;
    const int q = quant_choice(e, img, nullptr, nullptr);
    if (m.hdr_for.matches(img->width, img->height, q, sub, restart, progressive ? 1 : 0)) return JPEGAMD_OK;
    uint8_t luma[64], chroma[64], hdr[kColorPrefixMax + kMcuDriBytes + kMcuSosBytes];
    quant_choice(e, img, luma, chroma);
    size_t n, nsos;
    uint8_t sos[kMcuSosBytes] = {0xFF, 0xDA, 0x00, 0x0C, 0x03, 0x01, 0x00, 0x02, 0x11, 0x03, 0x11, 0x00, 0x3F, 0x00};
    if (sub == kSubNone) {
        static_assert(JPEGAMD_JFIF_PREFIX_BYTES <= kColorPrefixMax, "the grayscale prefix fits the staging buffer");
        n = build_jfif_prefix(img->width, img->height, luma, hdr) - kSosBytes;
        nsos = kSosBytes;
        std::memcpy(sos, hdr + n, nsos);                                // (behind the DRI segment again)
    } else {
        n = build_jfif_prefix_color(img->width, img->height, luma, chroma, chroma_mode(sub), hdr) - kSosBytes;
        nsos = kMcuSosBytes;
    }
    if (restart) {
        const uint8_t dri[kMcuDriBytes] = {0xFF, 0xDD, 0x00, 0x04, (uint8_t)(restart >> 8), (uint8_t)restart};
        std::memcpy(hdr + n, dri, sizeof(dri));
        n += sizeof(dri);
    }
    if (progressive) {
        const int sof = sub == kSubNone ? kGraySofOffset : kColorSofOffset;
        if (restart || hdr[sof] != 0xFF || hdr[sof + 1] != 0xC0) return JPEGAMD_ERR_ARG;
        hdr[sof + 1] = 0xC2;
        sos[nsos - 2] = 0x00;                                           // Se
    }
    std::memcpy(hdr + n, sos, nsos);
    if (int32_t rc = wait_pending(e)) return rc;
    HIP_TRY(hipMemcpy(m.hdr, hdr, n + nsos, hipMemcpyHostToDevice));
    m.hdr_for.set(img->width, img->height, q, sub, (int)(n + nsos), restart, progressive ? 1 : 0);
    return JPEGAMD_OK;
}

// The scratch of a progressive call: the records (made once, with the SOS segments of the scans 2 .. 7) and `slot_bytes` of slots.
static int32_t prog_alloc(JpegAmdEncoder *e, size_t slot_bytes) {
    auto &m = e->mcu;
    if (!m.pmeta) {
        HIP_TRY(hipMalloc((void **)&m.pmeta, kProgMetaAlloc));
        uint8_t sos[2][kProgScansMax][16] = {};
        for (const ProgScript *sc : {&kScriptSpectral, &kScriptSuccessive})
            for (int k = 0; k < sc->scans; ++k) prog_sos(sc->scan[k], sos[sc->id][k]);
        HIP_TRY(hipMemcpy(m.pmeta + kProgMetaSos, sos, sizeof(sos), hipMemcpyHostToDevice));
    }
    return grow_scratch(e, &m.pslots, &m.pslots_cap, slot_bytes);
}

// The SOS segments of a caller's script behind the built-in scripts': uploaded when they differ from what lies there.
static int32_t prog_upload_sos(JpegAmdEncoder *e, const ProgScript &sc) {
    auto &m = e->mcu;
    uint8_t sos[kProgScansMax][16] = {};
    for (int k = 0; k < sc.scans; ++k) prog_sos(sc.scan[k], sos[k]);
    static_assert(sizeof(sos) == sizeof(m.psos), "the key is the upload");
    if (m.psos_valid && std::memcmp(sos, m.psos, sizeof(sos)) == 0) return JPEGAMD_OK;
    if (int32_t rc = wait_pending(e)) return rc;                    // (a call in flight may still read the segments)
    m.psos_valid = false;
    HIP_TRY(hipMemcpy(m.pmeta + kProgMetaSos + (size_t)sc.id * kProgScansMax * 16, sos, sizeof(sos), hipMemcpyHostToDevice));
    std::memcpy(m.psos, sos, sizeof(sos));
    m.psos_valid = true;
    return JPEGAMD_OK;
}

// ... and of a call that makes its own tables (4.6.13), for `pictures` pictures.
static int32_t prog_tables_alloc(JpegAmdEncoder *e, int pictures) {
    auto &m = e->mcu;
    if (pictures <= m.pcap) return JPEGAMD_OK;
    if (int32_t rc = wait_pending(e)) return rc;
    hipFree(m.pcounts); hipFree(m.pres); hipFree(m.ptabs); hipFree(m.phdr); hipFree(m.phdr_len);
    m.pcounts = nullptr; m.pres = nullptr; m.ptabs = nullptr; m.phdr = nullptr; m.phdr_len = nullptr; m.pcap = 0; m.plast = 0;
    const size_t n = (size_t)pictures;
    // (room for the longest script: a call lays its pictures out with its own script's numbers)
    HIP_TRY(hipMalloc((void **)&m.pcounts, n * kProgTablesMax * 256 * sizeof(unsigned long long)));
    HIP_TRY(hipMalloc((void **)&m.pres, n * kProgTablesMax * kHuffResBytes));
    HIP_TRY(hipMalloc((void **)&m.ptabs, n * kProgTablesMax * 272 * sizeof(uint32_t)));
    HIP_TRY(hipMalloc((void **)&m.phdr, n * kProgScansMax * kMcuPrefixSlot));
    HIP_TRY(hipMalloc((void **)&m.phdr_len, n * kProgScansMax * sizeof(uint32_t)));
    m.pcap = pictures;
    return JPEGAMD_OK;
}

// A script's scan as the one-component (comp >= 0) form of the group's three-component arguments.
// A scan of two components (4.6.15): the group's grid with the scan's own MCU; a grayscale file's scans: the group's arguments are the
// one-component form already.
static bool prog_scan_args(const McuGeometry &g, const McuSegArgs &sa3, const ProgScan &c, McuSegArgs *out) {
    const int comp = g.comps == 3 && popcount3(c.mask) == 1 ? (c.mask == 1 ? 0 : (c.mask == 2 ? 1 : 2)) : -1;
    McuSegArgs sa = sa3;
    sa.ah = c.ah; sa.al = c.al;
    if (g.comps == 1) { sa.ss = c.ss; sa.se = c.se; }
    if (g.comps == 3 && popcount3(c.mask) == 2) {
        sa.comps = 2; sa.mask = c.mask;
        sa.seg_mcus = kSegBlocks / mcu_blocks_per_mcu2(g.hs, g.vs, c.mask);
        sa.num_segs = (int)(((int64_t)g.mx * g.my + sa.seg_mcus - 1) / sa.seg_mcus);
        sa.num_segs_pad = (sa.num_segs + kSegGroup - 1) / kSegGroup * kSegGroup;
        if (sa.num_segs_pad > g.num_segs_pad) return false;         // (a shorter MCU: no more segments than the three-component scan has)
    }
    if (comp >= 0) {                                                 // ONE component: its plane, its block grid, its table class
        sa.coef = sa3.coef + (comp == 0 ? 0 : (comp == 1 ? sa3.cb_off : sa3.cr_off));
        sa.bw = sa.mx = comp ? g.mx : g.bw; sa.bh = sa.my = comp ? g.my : g.bh;
        sa.hs = sa.vs = 1; sa.comps = 1;
        sa.seg_mcus = mcu_seg_mcus(1, 1, 1);
        sa.num_segs = (int)(((int64_t)sa.bw * sa.bh + sa.seg_mcus - 1) / sa.seg_mcus);
        sa.num_segs_pad = (sa.num_segs + kSegGroup - 1) / kSegGroup * kSegGroup;
        if (sa.num_segs_pad > g.num_segs_pad) return false;         // (a plane has fewer segments than the MCU scan: the arrays hold them)
        if (comp) sa.huff_y = sa3.huff_c;
        sa.ss = c.ss; sa.se = c.se;
    }
    *out = sa;
    return true;
}

// The seven scans of one group's files with end-of-band runs and tables of their own: count every scan's symbols,
// make all the tables and headers at once (the counts of a scan with runs do not depend on a table, so nothing of a later scan waits
// for an earlier one), then code scan by scan over the path's one set of segment arrays and let the restart writer -- one interval, a
// header per picture, no EOI but behind the last scan -- place each: scan 1 in the caller's buffers, the others in the slots.
// `sc`: the file's scan script -- the seven scans of 4.6.13, or the ten of successive approximation (4.6.14), whose scan of raw bits
// is not counted and gets a header of its SOS alone.
static int progressive_runs_scans(JpegAmdEncoder *e, const McuGeometry &g, const ProgScript &sc, const ProgSlots &slots, const McuSegArgs &sa3, int first, int n,
                                  int count, bool last_of_call, void *const *outs_dev, uint64_t out_capacity, uint64_t *const *out_sizes_dev,
                                  const unsigned long long *pic, hipStream_t stream) {
    auto &m = e->mcu;
    const ProgMeta meta = prog_meta(m.pmeta, sc.scans);
    const size_t tables = (size_t)sc.tables;
    if (hipMemsetAsync(m.pmeta, 0, meta.record_bytes, stream) != hipSuccess) return (int)hipErrorUnknown;
    unsigned long long *counts = m.pcounts + (size_t)first * tables * 256;
    if (hipMemsetAsync(counts, 0, (size_t)n * tables * 256 * sizeof(unsigned long long), stream) != hipSuccess) return (int)hipErrorUnknown;
    McuSegArgs sa[kProgScansMax];
    for (int k = 0; k < sc.scans; ++k) {
        if (!prog_scan_args(g, sa3, sc.scan[k], &sa[k])) return (int)hipErrorInvalidValue;
        if (sc.scan[k].table < 0) continue;
        if (int err = launch_mcu_band_histogram(sa[k], counts, sc.scan[k].table, sc.tables, stream)) return err;
    }
    HuffOptimalArgs ha;
    std::memset(&ha, 0, sizeof(ha));
    ha.freq = counts; ha.jobs = sc.tables * n;
    ha.res = m.pres + (size_t)first * tables * kHuffResBytes;
    if (int err = launch_huff_optimal(ha, stream)) return err;
    ProgTablesArgs pa;
    std::memset(&pa, 0, sizeof(pa));
    pa.res = ha.res; pa.tabs = m.ptabs + (size_t)first * tables * 272;
    pa.hdr_out = m.phdr; pa.hdr_len = m.phdr_len; pa.pictures = count; pa.first = first;
    pa.hdr = m.hdr; pa.head_len = g.comps == 1 ? m.hdr_for.len - kSosBytes - kStdDhtBytesGray : m.hdr_for.len - kMcuSosBytes - kStdDhtBytes;
    pa.sos = prog_meta_sos(m.pmeta, sc);
    pa.scans = sc.scans; pa.tables = sc.tables;
    for (int k = 0; k < sc.scans; ++k) {
        const ProgScan &c = sc.scan[k];
        pa.sos_len[k] = (uint8_t)(8 + 2 * popcount3(c.mask));
        if (c.table < 0) { pa.bare |= 1u << k; continue; }
        const int nt = prog_scan_tables(c);
        for (int t = c.table; t < c.table + nt; ++t) {              // Tc/Th: 0x00 / 0x01 the DC tables of Y / chroma, 0x10 / 0x11 the AC tables
            pa.table_scan[t] = (uint8_t)k;
            pa.table_id[t] = (uint8_t)((c.ss ? 0x10 : 0x00) | ((nt == 2 ? t > c.table : !(c.mask & 1)) ? 1 : 0));
        }
    }
    if (int err = launch_prog_tables(pa, n, stream)) return err;

    for (int k = 0; k < sc.scans; ++k) {
        McuSegArgs &s = sa[k];
        const int table = sc.scan[k].table < 0 ? 0 : sc.scan[k].table;   // (a scan of raw bits reads no table: any that exists)
        s.huff_y = pa.tabs + (size_t)table * 272; s.huff_c = pa.tabs + (size_t)(table + (prog_scan_tables(sc.scan[k]) == 2 ? 1 : 0)) * 272; s.huff_stride = (uint32_t)(tables * 272);
        s.runs = 1;
        s.sums = meta.sums + (size_t)k * kMaxBatch * 2;
        s.status = &meta.scan_stats[k ? 1 : 0].status;
        if (int err = launch_mcu_band_segments(s, stream)) return err;
        McuRestartArgs ra;
        std::memset(&ra, 0, sizeof(ra));
        ra.seg = s.seg;
        ra.num_segs_pad = s.num_segs_pad; ra.batch = n;
        ra.segs_per_interval = s.num_segs; ra.intervals = 1; ra.last_seg = s.num_segs - 1;       // the scan is its one interval
        ra.pre = m.rst_words; ra.b0 = m.rst_words + m.rst_cap; ra.ff = m.rst_words + 2 * m.rst_cap;
        ra.pos = m.rst_pos; ra.pic_sums = meta.writer_sums + (size_t)k * kMaxBatch * kMcuPicSums;
        for (int i = 0; i < n; ++i) {
            ra.out[i] = k ? m.pslots + (size_t)i * slots.pic_bytes + slots.off[k] : (uint8_t *)outs_dev[first + i];
            ra.out_size[i] = meta.size + (size_t)k * kMaxBatch + i;
        }
        ra.out_capacity = k ? slots.cap[k] : out_capacity;
        ra.pic_prefix = m.phdr + ((size_t)k * count + (size_t)first) * kMcuPrefixSlot; ra.pic_prefix_len = m.phdr_len + (size_t)k * count + first;
        ra.pic_prefix_stride = kMcuPrefixSlot;
        ra.no_eoi = k == sc.scans - 1 ? 0 : 1;
        if (int err = launch_mcu_restart_writer(ra, stream)) return err;
    }
    ScansConcatArgs ca;
    std::memset(&ca, 0, sizeof(ca));
    for (int i = 0; i < n; ++i) { ca.out[i] = (uint8_t *)outs_dev[first + i]; ca.out_size[i] = out_sizes_dev[first + i]; }
    ca.out_capacity = out_capacity;
    ca.batch = n; ca.prefix_len = 0; ca.last_of_call = last_of_call ? 1 : 0;
    ca.scans = sc.scans;
    ca.size = meta.size;
    ca.slots = m.pslots; ca.pic_bytes = slots.pic_bytes;
    for (int k = 0; k < sc.scans; ++k) ca.slot_off[k] = slots.off[k];
    ca.sums = meta.sums;
    ca.writer_sums = meta.writer_sums;
    ca.pic = pic;
    ca.scan_stats = meta.scan_stats; ca.stats = e->stats_dev;
    return launch_scans_concat(ca, stream);
}

// The seven scans of the progressive files of one group of pictures, [first, first + n) of the call, whose coefficient planes the taps
// left in m.coef: one after the other on the stream over the path's one set of segment arrays.  `sa`: the group's arguments of the
// three-component coder (the DC scan's as they are).  Scan 1 goes through k_finalize behind the file's prefix into the caller's
// buffers, the others behind their SOS into the pictures' slots; k_scans_concat joins them.
static int progressive_scans(JpegAmdEncoder *e, const McuGeometry &g, const ProgSlots &slots, const McuSegArgs &sa3, const ImageDesc &iy, int first,
                             int n, bool last_of_call, void *const *outs_dev, uint64_t out_capacity, uint64_t *const *out_sizes_dev,
                             const unsigned long long *pic, hipStream_t stream) {
    auto &m = e->mcu;
    const ProgScript &sc = kScriptSpectral;                          // (k_finalize knows no per-picture header: the script with the Annex K tables alone)
    const ProgMeta meta = prog_meta(m.pmeta, sc.scans);
    const uint8_t *sos = prog_meta_sos(m.pmeta, sc);
    if (hipMemsetAsync(m.pmeta, 0, meta.record_bytes, stream) != hipSuccess) return (int)hipErrorUnknown;
    for (int k = 0; k < sc.scans; ++k) {
        McuSegArgs sa;
        if (!prog_scan_args(g, sa3, sc.scan[k], &sa)) return (int)hipErrorInvalidValue;
        sa.sums = meta.sums + (size_t)k * kMaxBatch * 2;
        sa.status = &meta.scan_stats[k ? 1 : 0].status;
        if (int err = launch_mcu_band_segments(sa, stream)) return err;

        ImageDesc is = iy;                                               // what run_finalize reads of it: the segments per picture and their length
        is.num_segs = sa.num_segs_pad; is.seg_tiles = kSegTiles;
        void *outs[kMaxBatch];
        uint64_t *sizes[kMaxBatch];
        for (int i = 0; i < n; ++i) {
            outs[i] = k ? (void *)(m.pslots + (size_t)i * slots.pic_bytes + slots.off[k]) : outs_dev[first + i];
            sizes[i] = meta.size + (size_t)k * kMaxBatch + i;
        }
        const ScanTarget tgt = {k ? sos + 16 * k : m.hdr, k ? kSosBytes : m.hdr_for.len, k == sc.scans - 1 ? 1 : 0, &meta.scan_stats[k ? 1 : 0], false, &m.seg};
        if (int err = run_finalize(e, is, outs, k ? slots.cap[k] : out_capacity, sizes, 1, stream, nullptr, n, false, &tgt)) return err;
    }
    ScansConcatArgs ca;
    std::memset(&ca, 0, sizeof(ca));
    for (int i = 0; i < n; ++i) { ca.out[i] = (uint8_t *)outs_dev[first + i]; ca.out_size[i] = out_sizes_dev[first + i]; }
    ca.out_capacity = out_capacity;
    ca.batch = n; ca.prefix_len = m.hdr_for.len; ca.last_of_call = last_of_call ? 1 : 0;
    ca.scans = sc.scans;
    ca.size = meta.size;
    ca.slots = m.pslots; ca.pic_bytes = slots.pic_bytes;
    for (int k = 0; k < sc.scans; ++k) ca.slot_off[k] = slots.off[k];
    ca.sums = meta.sums;
    ca.pic = pic;
    ca.scan_stats = meta.scan_stats; ca.stats = e->stats_dev;
    return launch_scans_concat(ca, stream);
}

// The interleaved files of a batch whose arguments are known to be good: g0 describes every picture, px holds their pixels (any
// layout color_batch takes).  `ycc_in` (a YCbCr batch of any kind): g0 / px are the Y planes as a GRAY picture, the chroma comes
// from the caller and every launch reads it where it lies; a BT.709 batch (ycc_in->matrix) is the RGB route with
// k_ycbcr_matrix_batch in front, as in color_batch: every launch then reads the full-range BT.601 planes that pass leaves in scratch.
// `restart`: the restart interval in MCUs (1 .. 65535), or 0 for the file without -- the launches below are then what they were
// before there were restart intervals: k_mcu_segments<false>, k_finalize, k_mcu_totals.
// subsampling kSubNone (jpegamd_encode_gray_scan_batch_async alone): the grayscale file as a scan of ONE component, DESIGN.md 4.6.11 -- the luma of g0 / px
// tapped and coded, no chroma launch, two tables; always through the restart writer (the caller sends the plain Annex K file elsewhere).
static int32_t interleaved_batch_run(JpegAmdEncoder *e, const JpegAmdImage &g0, const PlaneSet &px, int32_t count, int32_t subsampling, int32_t restart,
                                     void *const *outs_dev, uint64_t out_capacity, uint64_t *const *out_sizes_dev, void *stream_,
                                     const YccSource *ycc_in, int progressive, const ProgScript *user_script, const FloatSource *fl) {
    // `progressive`: the same taps, plane pass, matrix pass and grouping; behind a group's taps its seven scans
    // (progressive_scans) in place of k_mcu_segments, k_finalize and k_mcu_totals.  Colour, the Annex K tables, no restart intervals.
    // kProgRuns: histograms, tables and the restart writer as well (progressive_runs_scans); the context's Huffman
    // mode is neither read nor changed.
    // kProgSuccessive: kProgRuns' steps over the script of ten scans.
    const bool runs = progressive >= kProgRuns;
    // kProgScript: kProgRuns' steps over the caller's script, which the entry validated; colour or grayscale.
    if ((progressive == kProgScript) != (user_script != nullptr)) return JPEGAMD_ERR_ARG;
    const ProgScript &script = user_script ? *user_script : prog_script(progressive);
    if (progressive && (restart || script.comps != (subsampling == kSubNone ? 1 : 3) || (!runs && e->huffman != JPEGAMD_HUFFMAN_STANDARD))) return JPEGAMD_ERR_ARG;
    // a front pass fills the scratch planes, as in color_batch_run: `fl` (a float batch; g0 a GRAY picture of its geometry, px not read)
    // has k_float_planes_batch there, which for a scan of one component writes the Y planes alone
    const bool front = fl || (ycc_in && ycc_in->matrix == JPEGAMD_MATRIX_BT709);
    const YccSource *const ycc = front ? nullptr : ycc_in;            // what the launches read: the caller's planes, or the scratch
    const bool planar = g0.channel_order == kOrderPlanar;
    const McuGeometry g = mcu_geometry(g0.width, g0.height, subsampling, restart);
    // A picture's own tables: k_mcu_histogram and k_huff_optimal in front of the coder, and the restart writer for
    // every interval -- it reads a prefix and its length per picture; without restart intervals the scan is its one interval.
    const bool gray = g.comps == 1;
    const bool optimized = !runs && e->huffman == JPEGAMD_HUFFMAN_OPTIMIZED, writer = restart || optimized || runs;
    if (gray && !writer) return JPEGAMD_ERR_ARG;                    // (that file is gray_batch's: the entry sends it there)
    // segments as short as one MCU: a picture whose scratch alone is beyond the group budget is refused, nothing allocated or launched
    if ((restart || gray) && mcu_scratch_per_pic(g, true) > kMcuScratchBudget) return JPEGAMD_ERR_TOO_LARGE;
    // every launch codes ONE picture's component: the Y plane and a chroma plane must fit the context
    const MatrixScratch ms = matrix_scratch(g0.width, g0.height, count, gray ? 0 : g.chroma.plane_bytes);
    JpegAmdImage gy = g0;                                            // the Y launches' picture: behind a front pass they read the scratch Y planes
    if (front) gy.row_stride = ms.ypitch;
    ImageDesc iy;
    int32_t rc = describe(e, &gy, &iy, kSegTiles, planar ? kAcceptPlanar : kAcceptPx4);
    if (rc) return rc;
    const ChromaGeom &cg = g.chroma;
    JpegAmdImage pimg = g0;
    pimg.width = cg.cw; pimg.height = cg.ch; pimg.row_stride = ycc ? ycc->c_stride : cg.pitch; pimg.bottom_up = 0; pimg.channel_order = JPEGAMD_ORDER_GRAY;
    pimg.pixels = ycc ? ycc->cb[0] : g0.pixels;                      // (a non-null placeholder: every launch sets its own plane)
    ImageDesc ic = {};
    rc = gray ? JPEGAMD_OK : describe(e, &pimg, &ic);
    if (rc) return rc;
    if (iy.blocks_w != g.bw || iy.blocks_h != g.bh || (!gray && (ic.blocks_w != g.mx || ic.blocks_h != g.my))) return JPEGAMD_ERR_ARG;

    const ProgSlots slots = progressive ? prog_slots(g, script, runs) : ProgSlots{};
    const size_t per_pic = (size_t)mcu_scratch_per_pic(g, writer) + (size_t)slots.pic_bytes;
    const int group = (int)std::max<size_t>(1, std::min<size_t>((size_t)count, kMcuScratchBudget / per_pic));
    rc = color_alloc_consts(e);
    if (rc) return rc;
    rc = color_batch_alloc(e, front ? ms.total : (ycc || gray ? 0 : 2 * (size_t)count * cg.plane_bytes + 256), 0);
    if (rc) return rc;
    rc = mcu_alloc(e, g, group, writer, optimized ? count : 0);
    if (rc) return rc;
    rc = prepare_constants(e, &g0, false);
    if (rc) return rc;
    rc = gray ? JPEGAMD_OK : prepare_color_constants(e, &g0, subsampling);
    if (rc) return rc;
    rc = prepare_mcu_prefix(e, &g0, subsampling, restart, progressive != kProgNone);
    if (rc) return rc;
    auto &c = e->color;
    auto &m = e->mcu;
    if (progressive) {
        rc = prog_alloc(e, (size_t)group * (size_t)slots.pic_bytes);
        if (rc) return rc;
        rc = runs ? prog_tables_alloc(e, count) : JPEGAMD_OK;
        if (rc) return rc;
        rc = user_script ? prog_upload_sos(e, script) : JPEGAMD_OK;
        if (rc) return rc;
    }
    unsigned long long *pic = reinterpret_cast<unsigned long long *>(c.bmeta + kBatchMetaStats);
    hipStream_t stream = (hipStream_t)stream_;

    hipEvent_t *cev;
    rc = claim_slot(e, true, true, &cev);
    if (rc) return rc;
    if (cev) HIP_TRY(hipEventRecord(cev[0], stream));                // ns_total: from here to behind the last kernel
    HIP_TRY(hipMemsetAsync(c.bmeta + kBatchMetaStats, 0, kBatchMetaPic, stream));
    HIP_TRY(hipMemsetAsync(m.scan_stats, 0, sizeof(ScanStats), stream));
    HIP_TRY(hipMemsetAsync(e->stats_dev, 0, offsetof(ScanStats, status), stream));      // the sums and the size; the status stays sticky

    if (fl) {                                                        // once for the whole call, in front of the groups
        if (gray ? launch_float_luma_pass(e, *fl, gy, count, stream, nullptr)
                 : launch_float_pass(e, *fl, g0.width, g0.height, count, kFloatOutColor, subsampling, cg, ms, stream, nullptr))
            return JPEGAMD_ERR_HIP;
    } else if (front) {
        if (launch_matrix_pass(e, g0, px, *ycc_in, count, subsampling, cg, ms, stream, nullptr)) return JPEGAMD_ERR_HIP;
    } else if (!ycc && !gray) {
        if (launch_plane_pass(e, g0, px, count, subsampling, cg, stream, nullptr)) return JPEGAMD_ERR_HIP;
    }
    const size_t cb_off = (size_t)g.bw * g.bh * 64, cr_off = cb_off + (size_t)g.mx * g.my * 64;
    for (int first = 0; first < count; first += group) {
        const int n = std::min(group, count - first);
        for (int i = 0; i < n; ++i) {
            const int p = first + i;
            int16_t *coef = m.coef + (size_t)i * g.coef_per_pic;
            {   // Y
                ImageDesc im = iy;
                set_single_picture(&im, front ? c.bplanes + ms.y_off + (size_t)p * ms.yplane_bytes : px.p[0][p]);
                PlaneSet one = {};                                   // a planar picture: ITS G and B planes are image 0 of the launch
                if (planar) {
                    for (int k = 0; k < 3; ++k) one.p[k][0] = px.p[k][p];
                    im.fast_ok = dword_loader_ok((uintptr_t)px.p[0][p] | (uintptr_t)px.p[1][p] | (uintptr_t)px.p[2][p], im.row_stride);
                }
                const TileSource src = y_source_of(gy, ycc, &im);
                if (launch_transform(e, im, true, nullptr, coef, nullptr, stream, nullptr, src, planar ? &one : nullptr)) return JPEGAMD_ERR_HIP;
                const PictureStatsArgs ps = {e->tile_head, e->huff, im.num_tiles, 1, 0, 0, pic + (size_t)p * kPicStatWords};
                if (launch_picture_stats(ps, stream)) return JPEGAMD_ERR_HIP;
            }
            for (int k = 0; k < (gray ? 0 : 2); ++k) {   // Cb, Cr: planes 2 p and 2 p + 1 of the call
                ImageDesc im = ic;
                set_single_picture(&im, chroma_plane_of(e, ycc, cg, 2 * p + k));
                const TileSource src = chroma_source_of(ycc, 2 * p + k, &im);
                if (launch_transform(e, im, true, nullptr, coef + (k ? cr_off : cb_off), nullptr, stream, nullptr, src)) return JPEGAMD_ERR_HIP;
                const PictureStatsArgs ps = {e->tile_head, c.huff, im.num_tiles, 1, 1, 2 * p + k, pic};
                if (launch_picture_stats(ps, stream)) return JPEGAMD_ERR_HIP;
            }
        }
        McuSegArgs sa;
        std::memset(&sa, 0, sizeof(sa));
        sa.coef = m.coef; sa.pic_stride = g.coef_per_pic; sa.cb_off = cb_off; sa.cr_off = cr_off;
        sa.bw = g.bw; sa.bh = g.bh; sa.mx = g.mx; sa.my = g.my; sa.hs = g.hs; sa.vs = g.vs;
        sa.seg_mcus = g.seg_mcus; sa.num_segs = g.num_segs; sa.num_segs_pad = g.num_segs_pad; sa.batch = n;
        sa.huff_y = e->huff; sa.huff_c = c.huff;
        sa.seg = m.seg;
        sa.seg.words_stride = (uint32_t)g.cap_words;
        sa.status = &m.scan_stats->status;
        sa.restart = restart; sa.segs_per_interval = restart ? g.segs_per_interval : 0;
        sa.comps = g.comps;
        if (progressive) {
            if (runs ? progressive_runs_scans(e, g, script, slots, sa, first, n, count, first + n == count, outs_dev, out_capacity, out_sizes_dev,
                                              pic + (size_t)first * kPicStatWords, stream)
                     : progressive_scans(e, g, slots, sa, iy, first, n, first + n == count, outs_dev, out_capacity, out_sizes_dev,
                                         pic + (size_t)first * kPicStatWords, stream))
                return JPEGAMD_ERR_HIP;
            continue;
        }
        if (optimized) {                                             // the group's pictures are [first, first + n) of the call's table scratch
            unsigned long long *counts = m.hcounts + (size_t)first * kMcuTabWords;
            HIP_TRY(hipMemsetAsync(counts, 0, (size_t)n * kMcuTabWords * sizeof(unsigned long long), stream));
            if (launch_mcu_histogram(sa, counts, stream)) return JPEGAMD_ERR_HIP;
            HuffOptimalArgs ha;
            std::memset(&ha, 0, sizeof(ha));
            ha.tables = gray ? 2 : 4;
            ha.counts = counts; ha.jobs = ha.tables * n;
            ha.res = m.hres + (size_t)first * ha.tables * kHuffResBytes;
            ha.tabs = m.htabs + (size_t)first * kMcuTabWords;
            ha.prefix = m.hprefix + (size_t)first * kMcuPrefixSlot; ha.prefix_len = m.hprefix_len + first;
            ha.hdr = m.hdr;                                          // the standard prefix: head, the Annex K DHTs (four, or two), [DRI,] SOS
            ha.tail_len = (gray ? kSosBytes : kMcuSosBytes) + (restart ? kMcuDriBytes : 0);
            ha.tail_off = m.hdr_for.len - ha.tail_len; ha.head_len = ha.tail_off - (gray ? kStdDhtBytesGray : kStdDhtBytes);
            if (launch_huff_optimal(ha, stream)) return JPEGAMD_ERR_HIP;
            sa.huff_y = ha.tabs; sa.huff_c = ha.tabs + 272; sa.huff_stride = kMcuTabWords;
        }
        if (launch_mcu_segments(sa, stream)) return JPEGAMD_ERR_HIP;

        if (writer) {                                               // k_mcu_restart_offsets + k_mcu_restart_write in k_finalize's place
            McuRestartArgs ra;
            std::memset(&ra, 0, sizeof(ra));
            ra.seg = sa.seg;
            ra.num_segs_pad = g.num_segs_pad; ra.batch = n;
            ra.segs_per_interval = g.segs_per_interval; ra.intervals = g.intervals; ra.last_seg = g.last_seg;
            ra.pre = m.rst_words; ra.b0 = m.rst_words + m.rst_cap; ra.ff = m.rst_words + 2 * m.rst_cap;
            ra.pos = m.rst_pos; ra.pic_sums = m.rst_pic_sums;
            for (int i = 0; i < n; ++i) { ra.out[i] = (uint8_t *)outs_dev[first + i]; ra.out_size[i] = out_sizes_dev[first + i]; }
            ra.out_capacity = out_capacity;
            ra.prefix = m.hdr; ra.prefix_len = m.hdr_for.len;
            if (optimized) {
                ra.pic_prefix = m.hprefix + (size_t)first * kMcuPrefixSlot; ra.pic_prefix_len = m.hprefix_len + first;
                ra.pic_prefix_stride = kMcuPrefixSlot;
            }
            if (launch_mcu_restart_writer(ra, stream)) return JPEGAMD_ERR_HIP;
        } else {
            ImageDesc is = iy;                                       // what run_finalize reads of it: the segments per picture and their length
            is.num_segs = g.num_segs_pad; is.seg_tiles = kSegTiles;
            const ScanTarget tgt = {m.hdr, m.hdr_for.len, 1, m.scan_stats, false, &m.seg};
            if (run_finalize(e, is, outs_dev + first, out_capacity, out_sizes_dev + first, 1, stream, nullptr, n, false, &tgt)) return JPEGAMD_ERR_HIP;
        }

        McuTotalsArgs ta;
        std::memset(&ta, 0, sizeof(ta));
        ta.seg = m.seg;
        ta.num_segs_pad = g.num_segs_pad; ta.prefix_len = m.hdr_for.len;
        ta.pic_sums = writer ? m.rst_pic_sums : nullptr;          // (the writer's sums: prefix_len is not read then)
        ta.last_of_call = first + n == count ? 1 : 0;
        for (int i = 0; i < n; ++i) ta.out_size[i] = out_sizes_dev[first + i];
        ta.out_capacity = out_capacity;
        ta.pic = pic + (size_t)first * kPicStatWords;
        ta.scan_stats = m.scan_stats; ta.stats = e->stats_dev;
        if (launch_mcu_totals(ta, n, stream)) return JPEGAMD_ERR_HIP;
    }
    if (optimized) m.hlast = count;
    if (runs) { m.plast = count; m.plast_tables = script.tables; m.plast_script = script.id; }
    if (cev) HIP_TRY(hipEventRecord(cev[21], stream));
    return enqueued(e, stream, count * g.num_segs_pad, cev != nullptr, true);
}

// ... with the context's metadata in front: placed once, behind the last group's launches.
static int32_t interleaved_batch(JpegAmdEncoder *e, const JpegAmdImage &g0, const PlaneSet &px, int32_t count, int32_t subsampling, int32_t restart,
                                 void *const *outs_dev, uint64_t out_capacity, uint64_t *const *out_sizes_dev, void *stream_,
                                 const YccSource *ycc_in = nullptr, int progressive = kProgNone, const ProgScript *user_script = nullptr,
                                 const FloatSource *fl = nullptr) {
    return with_metadata(e, count, outs_dev, out_capacity, out_sizes_dev, stream_, true, [&](void *const *outs, uint64_t cap) {
        return interleaved_batch_run(e, g0, px, count, subsampling, restart, outs, cap, out_sizes_dev, stream_, ycc_in, progressive, user_script, fl);
    });
}

// Tests: k_huff_optimal on arbitrary counts -- `n` tables of 256 counts each (a table's sum below 2^54) -> BITS, HUFFVAL (zeros behind
// the used ones) and the number of HUFFVAL bytes of each.  Synchronous, host pointers.
extern "C" int32_t jpegamd_debug_optimal_huffman(JpegAmdEncoder *e, const uint64_t *freq, int32_t n, uint8_t *bits, uint8_t *vals, int32_t *nvals) {
    if (!e || !freq || !bits || !vals || !nvals || n < 1 || n > 4096) return JPEGAMD_ERR_ARG;
    for (int t = 0; t < n; ++t) {
        uint64_t sum = 0;
        for (int i = 0; i < 256; ++i) {
            if (freq[(size_t)t * 256 + i] >> 54) return JPEGAMD_ERR_ARG;
            sum += freq[(size_t)t * 256 + i];
        }
        if (sum >> 54) return JPEGAMD_ERR_ARG;
    }
    if (int32_t rc = wait_pending(e)) return rc;
    unsigned long long *f_dev = nullptr;
    uint8_t *r_dev = nullptr;
    const size_t fbytes = (size_t)n * 256 * sizeof(uint64_t), rbytes = (size_t)n * kHuffResBytes;
    std::vector<uint8_t> res(rbytes);
    int32_t rc = JPEGAMD_OK;
    HuffOptimalArgs ha;
    std::memset(&ha, 0, sizeof(ha));
    if (hipMalloc((void **)&f_dev, fbytes) != hipSuccess || hipMalloc((void **)&r_dev, rbytes) != hipSuccess) rc = JPEGAMD_ERR_HIP;
    if (!rc && hipMemcpy(f_dev, freq, fbytes, hipMemcpyHostToDevice) != hipSuccess) rc = JPEGAMD_ERR_HIP;
    ha.freq = f_dev; ha.jobs = n; ha.res = r_dev;
    if (!rc && launch_huff_optimal(ha, nullptr)) rc = JPEGAMD_ERR_HIP;
    if (!rc && hipMemcpy(res.data(), r_dev, rbytes, hipMemcpyDeviceToHost) != hipSuccess) rc = JPEGAMD_ERR_HIP;
    hipFree(f_dev); hipFree(r_dev);
    if (rc) return rc;
    for (int t = 0; t < n; ++t) {
        const uint8_t *r = res.data() + (size_t)t * kHuffResBytes;
        std::memcpy(bits + (size_t)t * 16, r, 16);
        uint32_t nv;
        std::memcpy(&nv, r + 16, sizeof(nv));
        nvals[t] = (int32_t)nv;
        std::memcpy(vals + (size_t)t * 256, r + 32, 256);
    }
    return JPEGAMD_OK;
}

// Tests: the symbol counts of the context's last call with optimised tables, [pictures][4][256] in the order luma DC, luma AC,
// chroma DC, chroma AC (a DC table's counts at 0 .. 15).  JPEGAMD_ERR_ARG when the context made no such call.  Synchronous.
extern "C" int32_t jpegamd_debug_huffman_counts(JpegAmdEncoder *e, uint64_t *counts) {
    if (!e || !counts || e->mcu.hlast < 1) return JPEGAMD_ERR_ARG;
    if (int32_t rc = wait_pending(e)) return rc;
    const int n = e->mcu.hlast;
    std::vector<unsigned long long> dev((size_t)n * kMcuTabWords);
    HIP_TRY(hipMemcpy(dev.data(), e->mcu.hcounts, dev.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    std::memset(counts, 0, (size_t)n * 4 * 256 * sizeof(uint64_t));
    for (int q = 0; q < n; ++q)
        for (int cls = 0; cls < 2; ++cls) {
            const unsigned long long *src = dev.data() + (size_t)q * kMcuTabWords + (size_t)cls * 272;
            uint64_t *dst = counts + ((size_t)q * 4 + 2 * cls) * 256;
            for (int i = 0; i < 16; ++i) dst[i] = src[256 + i];
            for (int i = 0; i < 256; ++i) dst[256 + i] = src[i];
        }
    return JPEGAMD_OK;
}

static bool restart_valid(int32_t restart) { return restart >= 0 && restart <= 65535; }

// `count` packed pictures in one scan: the argument checks (`px4`: the entry takes RGBA / BGRA as well), then the interleaved batch.
static int32_t interleaved_pixels(JpegAmdEncoder *e, const JpegAmdImage *imgs, int32_t count, int32_t subsampling, int32_t restart_interval, bool px4,
                                  void *const *outs_dev, uint64_t out_capacity, uint64_t *const *out_sizes_dev, void *stream_,
                                  int progressive = kProgNone, const ProgScript *user_script = nullptr) {
    // the arguments first: nothing of the context is read before they are known to be good
    if (!restart_valid(restart_interval)) return JPEGAMD_ERR_ARG;
    if (!e || !imgs || !outs_dev || !out_sizes_dev || count < 1 || count > kMaxBatch) return JPEGAMD_ERR_ARG;
    if (!sub_valid(subsampling)) return JPEGAMD_ERR_ARG;
    const JpegAmdImage &g0 = imgs[0];
    if (g0.channel_order != JPEGAMD_ORDER_BGR && g0.channel_order != JPEGAMD_ORDER_RGB && !(px4 && is_px4(g0.channel_order))) return JPEGAMD_ERR_ARG;
    if (g0.width <= 0 || g0.height <= 0 || g0.width > 65535 || g0.height > 65535 ||
        g0.row_stride < bytes_per_pixel(g0.channel_order) * (int64_t)g0.width)
        return JPEGAMD_ERR_ARG;
    PlaneSet ps;
    if (int32_t rc = uniform_batch_args(imgs, count, outs_dev, out_sizes_dev, &ps)) return rc;
    return interleaved_batch(e, g0, ps, count, subsampling, restart_interval, outs_dev, out_capacity, out_sizes_dev, stream_, nullptr, progressive, user_script);
}

// Progressive colour files of `count` RGB / BGR / RGBA / BGRA pictures: the argument checks of
// jpegamd_encode_color_interleaved_pixels_batch_async, then the interleaved batch with its seven scans.  A context set to
// JPEGAMD_HUFFMAN_OPTIMIZED is refused (interleaved_batch: before anything is allocated or launched).
extern "C" int32_t jpegamd_encode_color_progressive_batch_async(JpegAmdEncoder *e, const JpegAmdImage *imgs, int32_t count, int32_t subsampling,
                                                                void *const *outs_dev, uint64_t out_capacity, uint64_t *const *out_sizes_dev,
                                                                void *stream_) {
    return interleaved_pixels(e, imgs, count, subsampling, 0, true, outs_dev, out_capacity, out_sizes_dev, stream_, kProgStandard);
}

// ... with end-of-band runs and per-scan optimised tables: the same checks, pictures and batching.  The context's
// Huffman mode is not read.
extern "C" int32_t jpegamd_encode_color_progressive_optimized_batch_async(JpegAmdEncoder *e, const JpegAmdImage *imgs, int32_t count, int32_t subsampling,
                                                                          void *const *outs_dev, uint64_t out_capacity, uint64_t *const *out_sizes_dev,
                                                                          void *stream_) {
    return interleaved_pixels(e, imgs, count, subsampling, 0, true, outs_dev, out_capacity, out_sizes_dev, stream_, kProgRuns);
}

// Tests: the symbol counts of the context's last call with per-scan tables, [pictures][8][256] in the file's table order: Y DC,
// chroma DC, then the AC tables of the scans 2 .. 7.  JPEGAMD_ERR_ARG when the context made no such call.  Synchronous.
static int32_t debug_prog_counts(JpegAmdEncoder *e, uint64_t *counts, int tables, int script) {
    if (!e || !counts || e->mcu.plast < 1 || e->mcu.plast_tables != tables || e->mcu.plast_script != script) return JPEGAMD_ERR_ARG;
    if (int32_t rc = wait_pending(e)) return rc;
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "the counts are copied as they lie");
    HIP_TRY(hipMemcpy(counts, e->mcu.pcounts, (size_t)e->mcu.plast * (size_t)tables * 256 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return JPEGAMD_OK;
}
extern "C" int32_t jpegamd_debug_progressive_counts(JpegAmdEncoder *e, uint64_t *counts) { return debug_prog_counts(e, counts, kScriptSpectral.tables, kScriptSpectral.id); }

// Progressive files with successive approximation: the ten scans of libjpeg's jpeg_simple_progression, a table per
// scan, end-of-band runs.  The arguments, refusals, batching, capacity behaviour and statistics of the entry above; the context's
// Huffman mode is not read.
extern "C" int32_t jpegamd_encode_color_progressive_successive_batch_async(JpegAmdEncoder *e, const JpegAmdImage *imgs, int32_t count, int32_t subsampling,
                                                                           void *const *outs_dev, uint64_t out_capacity, uint64_t *const *out_sizes_dev,
                                                                           void *stream_) {
    return interleaved_pixels(e, imgs, count, subsampling, 0, true, outs_dev, out_capacity, out_sizes_dev, stream_, kProgSuccessive);
}

// Tests: the symbol counts of the context's last call of the successive entries, [pictures][10][256] in the file's table order.
// JPEGAMD_ERR_ARG when the context's last call with per-scan tables was not one of them.  Synchronous.
extern "C" int32_t jpegamd_debug_progressive_successive_counts(JpegAmdEncoder *e, uint64_t *counts) {
    return debug_prog_counts(e, counts, kScriptSuccessive.tables, kScriptSuccessive.id);
}

extern "C" int32_t jpegamd_encode_color_interleaved_restart_batch_async(JpegAmdEncoder *e, const JpegAmdImage *imgs, int32_t count, int32_t subsampling,
                                                                        int32_t restart_interval, void *const *outs_dev, uint64_t out_capacity,
                                                                        uint64_t *const *out_sizes_dev, void *stream_) {
    return interleaved_pixels(e, imgs, count, subsampling, restart_interval, false, outs_dev, out_capacity, out_sizes_dev, stream_);
}

// ... in any of the four pixel orders: RGBA / BGRA are read where they lie.
extern "C" int32_t jpegamd_encode_color_interleaved_pixels_batch_async(JpegAmdEncoder *e, const JpegAmdImage *imgs, int32_t count, int32_t subsampling,
                                                                       int32_t restart_interval, void *const *outs_dev, uint64_t out_capacity,
                                                                       uint64_t *const *out_sizes_dev, void *stream_) {
    return interleaved_pixels(e, imgs, count, subsampling, restart_interval, true, outs_dev, out_capacity, out_sizes_dev, stream_);
}

// The grayscale file as a scan of one component, with restart intervals and the context's Huffman mode.
// A block in either mode is below kMaxBlockBitsColor bits (optimised: 27 + 63 x 26), every byte may be stuffed; the scan rounds up
// to a byte once and ends with EOI; n intervals add the DRI segment and 4 (n - 1) bytes (jpegamd_max_jfif_bytes_interleaved_restart).
extern "C" uint64_t jpegamd_max_jfif_bytes_gray_scan(int32_t width, int32_t height, int32_t restart_interval) {
    if (width <= 0 || height <= 0 || width > 65535 || height > 65535 || !restart_valid(restart_interval)) return 0;
    const uint64_t nb = blocks_of(width, height);
    const uint64_t plain = JPEGAMD_JFIF_PREFIX_BYTES + scan_bound(nb, kMaxBlockBitsColor) + 2 + 16;
    if (!restart_interval) return plain;
    const uint64_t n = (nb + (uint64_t)restart_interval - 1) / (uint64_t)restart_interval;
    return plain + kMcuDriBytes + 4 * (n - 1);
}

extern "C" int32_t jpegamd_encode_gray_scan_batch_async(JpegAmdEncoder *e, const JpegAmdImage *imgs, int32_t count, int32_t restart_interval,
                                                        void *const *outs_dev, uint64_t out_capacity, uint64_t *const *out_sizes_dev, void *stream_) {
    // the arguments first: nothing of the context is read before they are known to be good
    if (!restart_valid(restart_interval)) return JPEGAMD_ERR_ARG;
    if (!e || !imgs || !outs_dev || !out_sizes_dev || count < 1 || count > kMaxBatch) return JPEGAMD_ERR_ARG;
    ImageDesc im;
    if (int32_t rc = describe(nullptr, &imgs[0], &im, kSegTiles, kAcceptPx4)) return rc;
    PlaneSet ps;
    if (int32_t rc = uniform_batch_args(imgs, count, outs_dev, out_sizes_dev, &ps)) return rc;
    // no intervals, the Annex K tables: the grayscale entry's file, and that entry writes it
    if (restart_interval == 0 && e->huffman == JPEGAMD_HUFFMAN_STANDARD) return gray_batch(e, imgs[0], ps, count, outs_dev, out_capacity, out_sizes_dev, 1, stream_);
    return interleaved_batch(e, imgs[0], ps, count, kSubNone, restart_interval, outs_dev, out_capacity, out_sizes_dev, stream_);
}

// `count` planar pictures in one scan.  No grayscale file here: subsampling 0 is refused.
extern "C" int32_t jpegamd_encode_planar_interleaved_batch_async(JpegAmdEncoder *e, const JpegAmdPlanarImage *imgs, int32_t count, int32_t subsampling,
                                                                 int32_t restart_interval, void *const *outs_dev, uint64_t out_capacity,
                                                                 void *const *out_sizes_dev, void *stream_) {
    // the arguments first: nothing of the context is read before they are known to be good
    if (!restart_valid(restart_interval)) return JPEGAMD_ERR_ARG;
    JpegAmdImage g0;
    PlaneSet ps;
    uint64_t *sizes[kMaxBatch];
    if (int32_t rc = planar_args(e, imgs, count, subsampling, false, outs_dev, out_sizes_dev, &g0, &ps, sizes)) return rc;
    return interleaved_batch(e, g0, ps, count, subsampling, restart_interval, outs_dev, out_capacity, sizes, stream_);
}

extern "C" int32_t jpegamd_encode_color_interleaved_batch_async(JpegAmdEncoder *e, const JpegAmdImage *imgs, int32_t count, int32_t subsampling,
                                                                void *const *outs_dev, uint64_t out_capacity, uint64_t *const *out_sizes_dev,
                                                                void *stream_) {
    return jpegamd_encode_color_interleaved_restart_batch_async(e, imgs, count, subsampling, 0, outs_dev, out_capacity, out_sizes_dev, stream_);
}

extern "C" int32_t jpegamd_encode_ycbcr_interleaved_restart_batch_async(JpegAmdEncoder *e, const JpegAmdYCbCrImage *imgs, int32_t count, int32_t subsampling,
                                                                        int32_t restart_interval, void *const *outs_dev, uint64_t out_capacity,
                                                                        void *const *out_sizes_dev, void *stream_) {
    // the arguments first: nothing of the context is read before they are known to be good
    if (!restart_valid(restart_interval)) return JPEGAMD_ERR_ARG;
    if (imgs && count >= 1 && count <= kMaxBatch)
        for (int i = 0; i < count; ++i) if (is_packed422(imgs[i].chroma_layout)) return JPEGAMD_ERR_ARG;      // packed 4:2:2 in one scan: a follow-up
    JpegAmdImage g0;
    PlaneSet ps;
    YccSource ycc;
    uint64_t *sizes[kMaxBatch];
    if (int32_t rc = ycbcr_args(e, imgs, count, subsampling, JPEGAMD_RANGE_FULL, JPEGAMD_SAMPLES_8, JPEGAMD_MATRIX_BT601, outs_dev, out_sizes_dev,
                                true, &g0, &ps, &ycc, sizes))
        return rc;
    return interleaved_batch(e, g0, ps, count, subsampling, restart_interval, outs_dev, out_capacity, sizes, stream_, &ycc);
}

// `count` YCbCr pictures of any kind jpegamd_encode_ycbcr_matrix_batch_async takes, in one scan: the same argument checks, then the
// interleaved batch, whose launches read the samples where they lie (BT.709: behind k_ycbcr_matrix_batch).
extern "C" int32_t jpegamd_encode_ycbcr_interleaved_matrix_batch_async(JpegAmdEncoder *e, const JpegAmdYCbCrImage *imgs, int32_t count, int32_t subsampling,
                                                                       int32_t sample_range, int32_t sample_format, int32_t matrix,
                                                                       int32_t restart_interval, void *const *outs_dev, uint64_t out_capacity,
                                                                       void *const *out_sizes_dev, void *stream_) {
    // the arguments first: nothing of the context is read before they are known to be good
    if (!restart_valid(restart_interval)) return JPEGAMD_ERR_ARG;
    JpegAmdImage g0;
    PlaneSet ps;
    YccSource ycc;
    uint64_t *sizes[kMaxBatch];
    if (int32_t rc = ycbcr_args(e, imgs, count, subsampling, sample_range, sample_format, matrix, outs_dev, out_sizes_dev, true, &g0, &ps, &ycc, sizes))
        return rc;
    return interleaved_batch(e, g0, ps, count, subsampling, restart_interval, outs_dev, out_capacity, sizes, stream_, &ycc);
}

// ... and their progressive files: the same argument checks, then the interleaved batch with its seven scans.
extern "C" int32_t jpegamd_encode_ycbcr_progressive_batch_async(JpegAmdEncoder *e, const JpegAmdYCbCrImage *imgs, int32_t count, int32_t subsampling,
                                                                int32_t sample_range, int32_t sample_format, int32_t matrix,
                                                                void *const *outs_dev, uint64_t out_capacity, void *const *out_sizes_dev,
                                                                void *stream_) {
    JpegAmdImage g0;
    PlaneSet ps;
    YccSource ycc;
    uint64_t *sizes[kMaxBatch];
    if (int32_t rc = ycbcr_args(e, imgs, count, subsampling, sample_range, sample_format, matrix, outs_dev, out_sizes_dev, true, &g0, &ps, &ycc, sizes))
        return rc;
    return interleaved_batch(e, g0, ps, count, subsampling, 0, outs_dev, out_capacity, sizes, stream_, &ycc, kProgStandard);
}

extern "C" int32_t jpegamd_encode_ycbcr_progressive_optimized_batch_async(JpegAmdEncoder *e, const JpegAmdYCbCrImage *imgs, int32_t count, int32_t subsampling,
                                                                          int32_t sample_range, int32_t sample_format, int32_t matrix,
                                                                          void *const *outs_dev, uint64_t out_capacity, void *const *out_sizes_dev,
                                                                          void *stream_) {
    JpegAmdImage g0;
    PlaneSet ps;
    YccSource ycc;
    uint64_t *sizes[kMaxBatch];
    if (int32_t rc = ycbcr_args(e, imgs, count, subsampling, sample_range, sample_format, matrix, outs_dev, out_sizes_dev, true, &g0, &ps, &ycc, sizes))
        return rc;
    return interleaved_batch(e, g0, ps, count, subsampling, 0, outs_dev, out_capacity, sizes, stream_, &ycc, kProgRuns);
}

extern "C" int32_t jpegamd_encode_ycbcr_progressive_successive_batch_async(JpegAmdEncoder *e, const JpegAmdYCbCrImage *imgs, int32_t count, int32_t subsampling,
                                                                           int32_t sample_range, int32_t sample_format, int32_t matrix,
                                                                           void *const *outs_dev, uint64_t out_capacity, void *const *out_sizes_dev,
                                                                           void *stream_) {
    JpegAmdImage g0;
    PlaneSet ps;
    YccSource ycc;
    uint64_t *sizes[kMaxBatch];
    if (int32_t rc = ycbcr_args(e, imgs, count, subsampling, sample_range, sample_format, matrix, outs_dev, out_sizes_dev, true, &g0, &ps, &ycc, sizes))
        return rc;
    return interleaved_batch(e, g0, ps, count, subsampling, 0, outs_dev, out_capacity, sizes, stream_, &ycc, kProgSuccessive);
}

// ---- a caller's scan script, and grayscale progressive files ----
// The script is validated first: a refused call allocates and launches nothing and leaves the context as it was.
extern "C" int32_t jpegamd_encode_color_progressive_script_batch_async(JpegAmdEncoder *e, const JpegAmdImage *imgs, int32_t count, int32_t subsampling,
                                                                       const JpegAmdScan *scans, int32_t scan_count, void *const *outs_dev,
                                                                       uint64_t out_capacity, uint64_t *const *out_sizes_dev, void *stream_) {
    ProgScript sc;
    if (!prog_script_from(scans, scan_count, 3, &sc)) return JPEGAMD_ERR_ARG;
    return interleaved_pixels(e, imgs, count, subsampling, 0, true, outs_dev, out_capacity, out_sizes_dev, stream_, kProgScript, &sc);
}

extern "C" int32_t jpegamd_encode_ycbcr_progressive_script_batch_async(JpegAmdEncoder *e, const JpegAmdYCbCrImage *imgs, int32_t count, int32_t subsampling,
                                                                       int32_t sample_range, int32_t sample_format, int32_t matrix,
                                                                       const JpegAmdScan *scans, int32_t scan_count, void *const *outs_dev,
                                                                       uint64_t out_capacity, void *const *out_sizes_dev, void *stream_) {
    ProgScript sc;
    if (!prog_script_from(scans, scan_count, 3, &sc)) return JPEGAMD_ERR_ARG;
    JpegAmdImage g0;
    PlaneSet ps;
    YccSource ycc;
    uint64_t *sizes[kMaxBatch];
    if (int32_t rc = ycbcr_args(e, imgs, count, subsampling, sample_range, sample_format, matrix, outs_dev, out_sizes_dev, true, &g0, &ps, &ycc, sizes))
        return rc;
    return interleaved_batch(e, g0, ps, count, subsampling, 0, outs_dev, out_capacity, sizes, stream_, &ycc, kProgScript, &sc);
}

// The grayscale file (SOF2, one component) of pictures in any of the five channel orders: the luma of the gray-scan entry, no chroma
// launch, no pad blocks; the DC tables are 0x00, the AC tables 0x10.
extern "C" int32_t jpegamd_encode_gray_progressive_script_batch_async(JpegAmdEncoder *e, const JpegAmdImage *imgs, int32_t count, const JpegAmdScan *scans,
                                                                      int32_t scan_count, void *const *outs_dev, uint64_t out_capacity,
                                                                      uint64_t *const *out_sizes_dev, void *stream_) {
    ProgScript sc;
    if (!prog_script_from(scans, scan_count, 1, &sc)) return JPEGAMD_ERR_ARG;
    if (!e || !imgs || !outs_dev || !out_sizes_dev || count < 1 || count > kMaxBatch) return JPEGAMD_ERR_ARG;
    ImageDesc im;
    if (int32_t rc = describe(nullptr, &imgs[0], &im, kSegTiles, kAcceptPx4)) return rc;
    PlaneSet ps;
    if (int32_t rc = uniform_batch_args(imgs, count, outs_dev, out_sizes_dev, &ps)) return rc;
    return interleaved_batch(e, imgs[0], ps, count, kSubNone, 0, outs_dev, out_capacity, out_sizes_dev, stream_, nullptr, kProgScript, &sc);
}

// ---------------------------------------------------------------------------------------------------------
// Float pictures: f32 / f16 / bf16 samples, read once where they lie by k_float_planes_batch, which leaves the
// planes of their bytes in context scratch; behind it every route is the one a BT.709 batch takes.
// ---------------------------------------------------------------------------------------------------------
constexpr float kFloatScaleMax = 16777216.0f;

// The arguments of a float batch, checked before anything of the context is read (outs_dev / out_sizes_dev: null for an entry that
// writes no files; subsampling 0: the grayscale file) -> the batch's geometry as a GRAY picture and what the pass reads.  ps holds
// placeholders: no launch behind the pass reads the caller's samples.
static int32_t float_args(const JpegAmdEncoder *e, const JpegAmdFloatImage *imgs, int32_t count, int32_t subsampling, int32_t sample_type,
                          float scale, float offset, void *const *outs_dev, void *const *out_sizes_dev, bool files, JpegAmdImage *g0,
                          PlaneSet *ps, FloatSource *fl, uint64_t **sizes) {
    if (!e || !imgs || (files && (!outs_dev || !out_sizes_dev)) || count < 1 || count > kMaxBatch) return JPEGAMD_ERR_ARG;
    if (subsampling != 0 && !sub_valid(subsampling)) return JPEGAMD_ERR_ARG;
    if (sample_type != JPEGAMD_FLOAT_F32 && sample_type != JPEGAMD_FLOAT_F16 && sample_type != JPEGAMD_FLOAT_BF16) return JPEGAMD_ERR_ARG;
    if (!std::isfinite(scale) || !std::isfinite(offset) || std::fabs(scale) > kFloatScaleMax) return JPEGAMD_ERR_ARG;
    const int64_t kb = sample_type == JPEGAMD_FLOAT_F32 ? 4 : 2;
    const JpegAmdFloatImage &p0 = imgs[0];
    if (p0.width <= 0 || p0.height <= 0 || p0.width > 65535 || p0.height > 65535) return JPEGAMD_ERR_ARG;
    if (p0.pixel_stride < kb || p0.pixel_stride % kb != 0 || p0.row_stride % kb != 0 || (int64_t)p0.row_stride < (int64_t)p0.pixel_stride * p0.width)
        return JPEGAMD_ERR_ARG;
    if (!p0.plane[0] || (p0.plane[1] == nullptr) != (p0.plane[2] == nullptr)) return JPEGAMD_ERR_ARG;
    const int channels = p0.plane[1] ? 3 : 1;
    if (channels == 1 && subsampling != 0) return JPEGAMD_ERR_ARG;
    *ps = PlaneSet{};
    *fl = FloatSource{};
    fl->channels = channels; fl->type = sample_type; fl->row_stride = p0.row_stride; fl->pixel_stride = p0.pixel_stride;
    fl->scale = scale; fl->offset = offset;
    for (int i = 0; i < count; ++i) {
        const JpegAmdFloatImage &g = imgs[i];
        if (files && (!outs_dev[i] || !out_sizes_dev[i])) return JPEGAMD_ERR_ARG;
        if (g.width != p0.width || g.height != p0.height || g.row_stride != p0.row_stride || g.pixel_stride != p0.pixel_stride ||
            g.quality != p0.quality)
            return JPEGAMD_ERR_ARG;
        for (int k = 0; k < 3; ++k) {
            if ((g.plane[k] != nullptr) != (k < channels) || (uintptr_t)g.plane[k] % (uintptr_t)kb != 0) return JPEGAMD_ERR_ARG;
            fl->plane[k][i] = (const uint8_t *)g.plane[k];
        }
        ps->p[0][i] = (const uint8_t *)g.plane[0];
        if (files) sizes[i] = (uint64_t *)out_sizes_dev[i];
    }
    g0->pixels = p0.plane[0];
    g0->width = p0.width; g0->height = p0.height; g0->row_stride = (p0.width + 3) / 4 * 4; g0->bottom_up = 0;
    g0->channel_order = JPEGAMD_ORDER_GRAY; g0->quality = p0.quality;
    return JPEGAMD_OK;
}

// The Y planes of a float batch's grayscale routes: sized here, filled by the route's front pass -> the pictures its launches code.
static int32_t float_luma_planes(JpegAmdEncoder *e, const JpegAmdImage &g0, int32_t count, JpegAmdImage *gy, PlaneSet *py) {
    const MatrixScratch ms = matrix_scratch(g0.width, g0.height, count, 0);
    if (int32_t rc = color_batch_alloc(e, ms.total, 0)) return rc;
    *gy = g0;
    *py = PlaneSet{};
    gy->pixels = e->color.bplanes; gy->row_stride = ms.ypitch;
    for (int i = 0; i < count; ++i) py->p[0][i] = e->color.bplanes + (size_t)i * ms.yplane_bytes;
    return JPEGAMD_OK;
}

// What the entries of a front-pass source share once its arguments are good (g0: the geometry of the files as a GRAY picture, fl: what
// the pass reads).  Three scans (SUBSAMPLE_444 / _420 / _422), or -- subsampling 0 -- the fused grayscale file of the luma or of the
// single channel: the files jpegamd_encode_planar_batch_async writes for the bytes the pass makes.
static int32_t front_batch(JpegAmdEncoder *e, const JpegAmdImage &g0, const PlaneSet &ps, const FloatSource &fl, int32_t count,
                           int32_t subsampling, void *const *outs_dev, uint64_t out_capacity, uint64_t *const *sizes, void *stream_) {
    JpegAmdImage gy;
    PlaneSet py;
    if (subsampling != 0) return color_batch(e, g0, ps, count, subsampling, outs_dev, out_capacity, sizes, stream_, nullptr, &fl);
    if (int32_t rc = float_luma_planes(e, g0, count, &gy, &py)) return rc;
    return gray_batch(e, gy, py, count, outs_dev, out_capacity, sizes, 1, stream_, &fl);
}
// ... in one scan, with restart intervals and the context's Huffman mode; subsampling 0 goes where jpegamd_encode_gray_scan_batch_async
// goes: the plain file is the fused entry's.
static int32_t front_interleaved_batch(JpegAmdEncoder *e, const JpegAmdImage &g0, const PlaneSet &ps, const FloatSource &fl, int32_t count,
                                       int32_t subsampling, int32_t restart_interval, void *const *outs_dev, uint64_t out_capacity,
                                       uint64_t *const *sizes, void *stream_) {
    if (subsampling == 0 && restart_interval == 0 && e->huffman == JPEGAMD_HUFFMAN_STANDARD)
        return front_batch(e, g0, ps, fl, count, 0, outs_dev, out_capacity, sizes, stream_);
    return interleaved_batch(e, g0, ps, count, subsampling == 0 ? kSubNone : subsampling, restart_interval, outs_dev, out_capacity, sizes, stream_,
                             nullptr, kProgNone, nullptr, &fl);
}
// Tests: the pass alone, into the same scratch, and its planes copied tightly packed into the caller's DEVICE buffers (y_out: count x
// height x width bytes; cb_out, cr_out: count x ch x cw, not written for subsampling 0 and then free to be null).  Returns when the
// copies are done.
static int32_t front_debug_planes(JpegAmdEncoder *e, const JpegAmdImage &g0, const FloatSource &fl, int32_t count, int32_t subsampling,
                                  void *y_out, void *cb_out, void *cr_out, void *stream_) {
    const bool gray = subsampling == 0;
    const ChromaGeom cg = gray ? ChromaGeom{} : chroma_geom(g0.width, g0.height, subsampling);
    const MatrixScratch ms = matrix_scratch(g0.width, g0.height, count, cg.plane_bytes);
    if (int32_t rc = color_batch_alloc(e, ms.total, 0)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const int out = gray ? (fl.channels == 1 ? kFloatOutSingle : kFloatOutLuma) : kFloatOutColor;
    if (launch_float_pass(e, fl, g0.width, g0.height, count, out, subsampling, cg, ms, stream, nullptr)) return JPEGAMD_ERR_HIP;
    const uint8_t *base = e->color.bplanes;
    for (int i = 0; i < count; ++i) {
        HIP_TRY(hipMemcpy2DAsync((uint8_t *)y_out + (size_t)i * g0.width * g0.height, (size_t)g0.width, base + ms.y_off + (size_t)i * ms.yplane_bytes,
                                 (size_t)ms.ypitch, (size_t)g0.width, (size_t)g0.height, hipMemcpyDeviceToDevice, stream));
        for (int k = 0; k < (gray ? 0 : 2); ++k)
            HIP_TRY(hipMemcpy2DAsync((uint8_t *)(k ? cr_out : cb_out) + (size_t)i * cg.cw * cg.ch, (size_t)cg.cw, base + (size_t)(2 * i + k) * cg.plane_bytes,
                                     (size_t)cg.pitch, (size_t)cg.cw, (size_t)cg.ch, hipMemcpyDeviceToDevice, stream));
    }
    HIP_TRY(hipStreamSynchronize(stream));
    return JPEGAMD_OK;
}

// `count` float pictures in three scans, or -- subsampling 0 -- as the fused grayscale file (front_batch).
extern "C" int32_t jpegamd_encode_float_batch_async(JpegAmdEncoder *e, const JpegAmdFloatImage *imgs, int32_t count, int32_t subsampling,
                                                    int32_t sample_type, float scale, float offset, void *const *outs_dev,
                                                    uint64_t out_capacity, void *const *out_sizes_dev, void *stream_) {
    // the arguments first: nothing of the context is read before they are known to be good
    JpegAmdImage g0;
    PlaneSet ps;
    FloatSource fl;
    uint64_t *sizes[kMaxBatch];
    if (int32_t rc = float_args(e, imgs, count, subsampling, sample_type, scale, offset, outs_dev, out_sizes_dev, true, &g0, &ps, &fl, sizes))
        return rc;
    return front_batch(e, g0, ps, fl, count, subsampling, outs_dev, out_capacity, sizes, stream_);
}

// ... in one scan (front_interleaved_batch).
extern "C" int32_t jpegamd_encode_float_interleaved_batch_async(JpegAmdEncoder *e, const JpegAmdFloatImage *imgs, int32_t count,
                                                                int32_t subsampling, int32_t sample_type, float scale, float offset,
                                                                int32_t restart_interval, void *const *outs_dev, uint64_t out_capacity,
                                                                void *const *out_sizes_dev, void *stream_) {
    // the arguments first: nothing of the context is read before they are known to be good
    if (!restart_valid(restart_interval)) return JPEGAMD_ERR_ARG;
    JpegAmdImage g0;
    PlaneSet ps;
    FloatSource fl;
    uint64_t *sizes[kMaxBatch];
    if (int32_t rc = float_args(e, imgs, count, subsampling, sample_type, scale, offset, outs_dev, out_sizes_dev, true, &g0, &ps, &fl, sizes))
        return rc;
    return front_interleaved_batch(e, g0, ps, fl, count, subsampling, restart_interval, outs_dev, out_capacity, sizes, stream_);
}

// ... as progressive files with a scan script (null: the default one); subsampling 0: the grayscale progressive file.
extern "C" int32_t jpegamd_encode_float_progressive_script_batch_async(JpegAmdEncoder *e, const JpegAmdFloatImage *imgs, int32_t count,
                                                                       int32_t subsampling, int32_t sample_type, float scale, float offset,
                                                                       const JpegAmdScan *scans, int32_t scan_count, void *const *outs_dev,
                                                                       uint64_t out_capacity, void *const *out_sizes_dev, void *stream_) {
    ProgScript sc;
    if (!prog_script_from(scans, scan_count, subsampling == 0 ? 1 : 3, &sc)) return JPEGAMD_ERR_ARG;
    JpegAmdImage g0;
    PlaneSet ps;
    FloatSource fl;
    uint64_t *sizes[kMaxBatch];
    if (int32_t rc = float_args(e, imgs, count, subsampling, sample_type, scale, offset, outs_dev, out_sizes_dev, true, &g0, &ps, &fl, sizes))
        return rc;
    return interleaved_batch(e, g0, ps, count, subsampling == 0 ? kSubNone : subsampling, 0, outs_dev, out_capacity, sizes, stream_, nullptr,
                             kProgScript, &sc, &fl);
}

// Tests: the pass of a float batch alone (front_debug_planes).  Not part of the public header.
extern "C" int32_t jpegamd_debug_float_planes(JpegAmdEncoder *e, const JpegAmdFloatImage *imgs, int32_t count, int32_t subsampling,
                                              int32_t sample_type, float scale, float offset, void *y_out, void *cb_out, void *cr_out,
                                              void *stream_) {
    JpegAmdImage g0;
    PlaneSet ps;
    FloatSource fl;
    if (!y_out || (subsampling != 0 && (!cb_out || !cr_out))) return JPEGAMD_ERR_ARG;
    if (int32_t rc = float_args(e, imgs, count, subsampling, sample_type, scale, offset, nullptr, nullptr, false, &g0, &ps, &fl, nullptr))
        return rc;
    return front_debug_planes(e, g0, fl, count, subsampling, y_out, cb_out, cr_out, stream_);
}

// ---------------------------------------------------------------------------------------------------------
// Reduced pictures: uint8 samples at any row and pixel stride, averaged in factor x factor boxes by
// k_reduce_planes_batch, which leaves the planes of the REDUCED picture in context scratch; behind it every route is a float batch's.
// ---------------------------------------------------------------------------------------------------------
extern "C" int32_t jpegamd_reduced_size(int32_t width, int32_t height, int32_t factor, int32_t *out_width, int32_t *out_height) {
    if (width <= 0 || height <= 0 || width > 65535 || height > 65535 || factor < 1 || factor > JPEGAMD_MAX_REDUCE || !out_width || !out_height)
        return JPEGAMD_ERR_ARG;
    *out_width = (width + factor - 1) / factor;
    *out_height = (height + factor - 1) / factor;
    return JPEGAMD_OK;
}

// The arguments of a reduced batch, checked before anything of the context is read, as float_args checks a float batch's -> the
// REDUCED geometry as a GRAY picture and what the pass reads.
static int32_t reduced_args(const JpegAmdEncoder *e, const JpegAmdStridedImage *imgs, int32_t count, int32_t subsampling, int32_t factor,
                            void *const *outs_dev, void *const *out_sizes_dev, bool files, JpegAmdImage *g0, PlaneSet *ps, FloatSource *fl,
                            uint64_t **sizes) {
    static_assert(JPEGAMD_MAX_REDUCE == kMaxReduce, "one bound");
    if (!e || !imgs || (files && (!outs_dev || !out_sizes_dev)) || count < 1 || count > kMaxBatch) return JPEGAMD_ERR_ARG;
    if (subsampling != 0 && !sub_valid(subsampling)) return JPEGAMD_ERR_ARG;
    const JpegAmdStridedImage &p0 = imgs[0];
    int32_t ow, oh;
    if (jpegamd_reduced_size(p0.width, p0.height, factor, &ow, &oh)) return JPEGAMD_ERR_ARG;
    if (p0.pixel_stride < 1 || (int64_t)p0.row_stride < (int64_t)p0.pixel_stride * p0.width) return JPEGAMD_ERR_ARG;
    if (!p0.plane[0] || (p0.plane[1] == nullptr) != (p0.plane[2] == nullptr)) return JPEGAMD_ERR_ARG;
    const int channels = p0.plane[1] ? 3 : 1;
    if (channels == 1 && subsampling != 0) return JPEGAMD_ERR_ARG;
    *ps = PlaneSet{};
    *fl = FloatSource{};
    fl->channels = channels; fl->row_stride = p0.row_stride; fl->pixel_stride = p0.pixel_stride;
    fl->reduce = factor; fl->src_width = p0.width; fl->src_height = p0.height;
    for (int i = 0; i < count; ++i) {
        const JpegAmdStridedImage &g = imgs[i];
        if (files && (!outs_dev[i] || !out_sizes_dev[i])) return JPEGAMD_ERR_ARG;
        if (g.width != p0.width || g.height != p0.height || g.row_stride != p0.row_stride || g.pixel_stride != p0.pixel_stride ||
            g.quality != p0.quality)
            return JPEGAMD_ERR_ARG;
        for (int k = 0; k < 3; ++k) {
            if ((g.plane[k] != nullptr) != (k < channels)) return JPEGAMD_ERR_ARG;
            fl->plane[k][i] = (const uint8_t *)g.plane[k];
        }
        ps->p[0][i] = (const uint8_t *)g.plane[0];
        if (files) sizes[i] = (uint64_t *)out_sizes_dev[i];
    }
    g0->pixels = p0.plane[0];
    g0->width = ow; g0->height = oh; g0->row_stride = (ow + 3) / 4 * 4; g0->bottom_up = 0;
    g0->channel_order = JPEGAMD_ORDER_GRAY; g0->quality = p0.quality;
    return JPEGAMD_OK;
}

// `count` pictures of bytes, each reduced by `factor` both ways, in three scans, or -- subsampling 0 -- as the fused grayscale file
// (front_batch): the files the uint8 entries write for the reduced bytes.
extern "C" int32_t jpegamd_encode_reduced_batch_async(JpegAmdEncoder *e, const JpegAmdStridedImage *imgs, int32_t count, int32_t subsampling,
                                                      int32_t factor, void *const *outs_dev, uint64_t out_capacity,
                                                      void *const *out_sizes_dev, void *stream_) {
    // the arguments first: nothing of the context is read before they are known to be good
    JpegAmdImage g0;
    PlaneSet ps;
    FloatSource fl;
    uint64_t *sizes[kMaxBatch];
    if (int32_t rc = reduced_args(e, imgs, count, subsampling, factor, outs_dev, out_sizes_dev, true, &g0, &ps, &fl, sizes)) return rc;
    return front_batch(e, g0, ps, fl, count, subsampling, outs_dev, out_capacity, sizes, stream_);
}

// ... in one scan (front_interleaved_batch); restart_interval counts MCUs of the reduced picture.
extern "C" int32_t jpegamd_encode_reduced_interleaved_batch_async(JpegAmdEncoder *e, const JpegAmdStridedImage *imgs, int32_t count,
                                                                  int32_t subsampling, int32_t factor, int32_t restart_interval,
                                                                  void *const *outs_dev, uint64_t out_capacity, void *const *out_sizes_dev,
                                                                  void *stream_) {
    // the arguments first: nothing of the context is read before they are known to be good
    if (!restart_valid(restart_interval)) return JPEGAMD_ERR_ARG;
    JpegAmdImage g0;
    PlaneSet ps;
    FloatSource fl;
    uint64_t *sizes[kMaxBatch];
    if (int32_t rc = reduced_args(e, imgs, count, subsampling, factor, outs_dev, out_sizes_dev, true, &g0, &ps, &fl, sizes)) return rc;
    return front_interleaved_batch(e, g0, ps, fl, count, subsampling, restart_interval, outs_dev, out_capacity, sizes, stream_);
}

// ... as progressive files with a scan script (null: the default one); subsampling 0: the grayscale progressive file.
extern "C" int32_t jpegamd_encode_reduced_progressive_script_batch_async(JpegAmdEncoder *e, const JpegAmdStridedImage *imgs, int32_t count,
                                                                         int32_t subsampling, int32_t factor, const JpegAmdScan *scans,
                                                                         int32_t scan_count, void *const *outs_dev, uint64_t out_capacity,
                                                                         void *const *out_sizes_dev, void *stream_) {
    ProgScript sc;
    if (!prog_script_from(scans, scan_count, subsampling == 0 ? 1 : 3, &sc)) return JPEGAMD_ERR_ARG;
    JpegAmdImage g0;
    PlaneSet ps;
    FloatSource fl;
    uint64_t *sizes[kMaxBatch];
    if (int32_t rc = reduced_args(e, imgs, count, subsampling, factor, outs_dev, out_sizes_dev, true, &g0, &ps, &fl, sizes)) return rc;
    return interleaved_batch(e, g0, ps, count, subsampling == 0 ? kSubNone : subsampling, 0, outs_dev, out_capacity, sizes, stream_, nullptr,
                             kProgScript, &sc, &fl);
}

// Tests: the pass of a reduced batch alone (front_debug_planes; the buffers hold planes of the REDUCED geometry) and the reciprocal the
// kernel divides by n with.  Not part of the public header.
extern "C" int32_t jpegamd_debug_reduced_planes(JpegAmdEncoder *e, const JpegAmdStridedImage *imgs, int32_t count, int32_t subsampling,
                                                int32_t factor, void *y_out, void *cb_out, void *cr_out, void *stream_) {
    JpegAmdImage g0;
    PlaneSet ps;
    FloatSource fl;
    if (!y_out || (subsampling != 0 && (!cb_out || !cr_out))) return JPEGAMD_ERR_ARG;
    if (int32_t rc = reduced_args(e, imgs, count, subsampling, factor, nullptr, nullptr, false, &g0, &ps, &fl, nullptr)) return rc;
    return front_debug_planes(e, g0, fl, count, subsampling, y_out, cb_out, cr_out, stream_);
}
extern "C" int32_t jpegamd_debug_reduce_reciprocal(int32_t n, uint32_t *multiplier, int32_t *shift) {
    if (n < 1 || n > kMaxReduce * kMaxReduce || !multiplier || !shift) return JPEGAMD_ERR_ARG;
    *multiplier = reduce_recip(n);
    *shift = kReduceShift;
    return JPEGAMD_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Resized pictures: uint8 samples at any row and pixel stride, resampled to out_width x out_height by exact area
// means by k_resize_planes_batch, which leaves the planes of the TARGET in context scratch; behind it every route is a float batch's.
// ---------------------------------------------------------------------------------------------------------
extern "C" int32_t jpegamd_resize_check(int32_t width, int32_t height, int32_t out_width, int32_t out_height) {
    static_assert(JPEGAMD_MAX_RESIZE_RATIO == kMaxResizeRatio, "one bound");
    if (width <= 0 || height <= 0 || width > 65535 || height > 65535) return JPEGAMD_ERR_ARG;
    if (out_width < 1 || out_width > width || (int64_t)width > (int64_t)JPEGAMD_MAX_RESIZE_RATIO * out_width) return JPEGAMD_ERR_ARG;
    if (out_height < 1 || out_height > height || (int64_t)height > (int64_t)JPEGAMD_MAX_RESIZE_RATIO * out_height) return JPEGAMD_ERR_ARG;
    return JPEGAMD_OK;
}

// The arguments of a resized batch: reduced_args' checks with jpegamd_resize_check in place of the factor's (a factor of 1 passes
// reduced_args whatever the source measures) -> the TARGET geometry as a GRAY picture and what the pass reads.
static int32_t resized_args(const JpegAmdEncoder *e, const JpegAmdStridedImage *imgs, int32_t count, int32_t subsampling, int32_t out_width,
                            int32_t out_height, void *const *outs_dev, void *const *out_sizes_dev, bool files, JpegAmdImage *g0, PlaneSet *ps,
                            FloatSource *fl, uint64_t **sizes) {
    if (!e || !imgs || count < 1 || count > kMaxBatch) return JPEGAMD_ERR_ARG;
    if (jpegamd_resize_check(imgs[0].width, imgs[0].height, out_width, out_height)) return JPEGAMD_ERR_ARG;
    if (int32_t rc = reduced_args(e, imgs, count, subsampling, 1, outs_dev, out_sizes_dev, files, g0, ps, fl, sizes)) return rc;
    fl->reduce = 0; fl->resize = 1; fl->out_width = out_width; fl->out_height = out_height;
    g0->width = out_width; g0->height = out_height; g0->row_stride = (out_width + 3) / 4 * 4;
    return JPEGAMD_OK;
}

// `count` pictures of bytes, each resized to out_width x out_height, in three scans, or -- subsampling 0 -- as the fused grayscale
// file (front_batch): the files the uint8 entries write for the resized bytes.
extern "C" int32_t jpegamd_encode_resized_batch_async(JpegAmdEncoder *e, const JpegAmdStridedImage *imgs, int32_t count, int32_t subsampling,
                                                      int32_t out_width, int32_t out_height, void *const *outs_dev, uint64_t out_capacity,
                                                      void *const *out_sizes_dev, void *stream_) {
    // the arguments first: nothing of the context is read before they are known to be good
    JpegAmdImage g0;
    PlaneSet ps;
    FloatSource fl;
    uint64_t *sizes[kMaxBatch];
    if (int32_t rc = resized_args(e, imgs, count, subsampling, out_width, out_height, outs_dev, out_sizes_dev, true, &g0, &ps, &fl, sizes))
        return rc;
    return front_batch(e, g0, ps, fl, count, subsampling, outs_dev, out_capacity, sizes, stream_);
}

// ... in one scan (front_interleaved_batch); restart_interval counts MCUs of the resized picture.
extern "C" int32_t jpegamd_encode_resized_interleaved_batch_async(JpegAmdEncoder *e, const JpegAmdStridedImage *imgs, int32_t count,
                                                                  int32_t subsampling, int32_t out_width, int32_t out_height,
                                                                  int32_t restart_interval, void *const *outs_dev, uint64_t out_capacity,
                                                                  void *const *out_sizes_dev, void *stream_) {
    // the arguments first: nothing of the context is read before they are known to be good
    if (!restart_valid(restart_interval)) return JPEGAMD_ERR_ARG;
    JpegAmdImage g0;
    PlaneSet ps;
    FloatSource fl;
    uint64_t *sizes[kMaxBatch];
    if (int32_t rc = resized_args(e, imgs, count, subsampling, out_width, out_height, outs_dev, out_sizes_dev, true, &g0, &ps, &fl, sizes))
        return rc;
    return front_interleaved_batch(e, g0, ps, fl, count, subsampling, restart_interval, outs_dev, out_capacity, sizes, stream_);
}

// ... as progressive files with a scan script (null: the default one); subsampling 0: the grayscale progressive file.
extern "C" int32_t jpegamd_encode_resized_progressive_script_batch_async(JpegAmdEncoder *e, const JpegAmdStridedImage *imgs, int32_t count,
                                                                         int32_t subsampling, int32_t out_width, int32_t out_height,
                                                                         const JpegAmdScan *scans, int32_t scan_count, void *const *outs_dev,
                                                                         uint64_t out_capacity, void *const *out_sizes_dev, void *stream_) {
    ProgScript sc;
    if (!prog_script_from(scans, scan_count, subsampling == 0 ? 1 : 3, &sc)) return JPEGAMD_ERR_ARG;
    JpegAmdImage g0;
    PlaneSet ps;
    FloatSource fl;
    uint64_t *sizes[kMaxBatch];
    if (int32_t rc = resized_args(e, imgs, count, subsampling, out_width, out_height, outs_dev, out_sizes_dev, true, &g0, &ps, &fl, sizes))
        return rc;
    return interleaved_batch(e, g0, ps, count, subsampling == 0 ? kSubNone : subsampling, 0, outs_dev, out_capacity, sizes, stream_, nullptr,
                             kProgScript, &sc, &fl);
}

// Tests: the pass of a resized batch alone (front_debug_planes; the buffers hold planes of the TARGET geometry) and the kernel's
// division, (s + (d >> 1)) / d for s <= 255 d + (d >> 1), by the text the kernel runs.  Not part of the public header.
extern "C" int32_t jpegamd_debug_resized_planes(JpegAmdEncoder *e, const JpegAmdStridedImage *imgs, int32_t count, int32_t subsampling,
                                                int32_t out_width, int32_t out_height, void *y_out, void *cb_out, void *cr_out,
                                                void *stream_) {
    JpegAmdImage g0;
    PlaneSet ps;
    FloatSource fl;
    if (!y_out || (subsampling != 0 && (!cb_out || !cr_out))) return JPEGAMD_ERR_ARG;
    if (int32_t rc = resized_args(e, imgs, count, subsampling, out_width, out_height, nullptr, nullptr, false, &g0, &ps, &fl, nullptr))
        return rc;
    return front_debug_planes(e, g0, fl, count, subsampling, y_out, cb_out, cr_out, stream_);
}
extern "C" int32_t jpegamd_debug_resize_divide(uint32_t d, uint64_t s, uint32_t *q) {
    if (d == 0 || !q || s > 255 * (uint64_t)d + (d >> 1)) return JPEGAMD_ERR_ARG;
    const ResizeDivide dv = resize_divide_for(d);
    *q = resize_divide(s + (d >> 1), dv.d, dv.mul, dv.shift);
    return JPEGAMD_OK;
}

// The bound of a file with a caller's script, scan by scan.  A scan is its DHT segments at most (a DC table 33 bytes: 21 + 12
// symbols; an AC table kProgDhtMax), its SOS (8 + 2 n bytes for n components), and its blocks (prog_scan_blocks: pad blocks
// included where the scan is interleaved) at the scan's worst bits per block, every byte stuffed, with ONE rounding up to a byte that
// may be stuffed (scan_bound).  The bits per block: a first DC scan 16 + 11 = 27; a DC refinement scan 1; a first AC scan 26 per
// coefficient of the band (16 + 10; a ZRL is at most a bit per zero) and 1 more -- the run's symbol, 16 + 8, is paid by a zero
// coefficient se that costs nothing else, which is 27 when the band is that one coefficient; an AC refinement scan 17 per
// coefficient, the run's symbol at a coefficient se that costs 1: 17 (n - 1) + 25 (kMaxBlockBitsRefine's derivation for n
// coefficients).  The file adds its head (no more than the whole standard prefix) and EOI.
static uint64_t prog_scan_block_bits(const ProgScan &c) {
    const uint64_t n = (uint64_t)(c.se - c.ss + 1);
    return c.ss == 0 ? (c.ah ? 1u : 27u) : (c.ah ? 17u * (n - 1) + 25u : 26u * n + 1u);
}
static_assert(27 <= kMaxBlockBitsColor && 63 * 26 + 1 <= kMaxBlockBitsColor && 62 * 17 + 25 == kMaxBlockBitsRefine && kMaxBlockBitsRefine <= kMaxBlockBitsColor,
              "one block's string of any scan of a script fits the reservation of a coder segment");
static_assert(26 * 63 + 1 <= 27 * 63 && 17 * 0 + 25 <= 27 && 26 + 1 <= 27, "a scan at its bound fits its slot (prog_slots: 27 bits a coefficient)");
extern "C" uint64_t jpegamd_max_jfif_bytes_progressive_script(int32_t width, int32_t height, int32_t subsampling, const JpegAmdScan *scans, int32_t scan_count) {
    if (width <= 0 || height <= 0 || width > 65535 || height > 65535 || (subsampling != kSubNone && !sub_valid(subsampling))) return 0;
    ProgScript sc;
    if (!prog_script_from(scans, scan_count, subsampling == kSubNone ? 1 : 3, &sc)) return 0;
    const McuGeometry g = mcu_geometry(width, height, subsampling);
    uint64_t total = (subsampling == kSubNone ? (uint64_t)JPEGAMD_JFIF_PREFIX_BYTES : (uint64_t)kColorPrefixMax) + 2 + 16;
    for (int k = 0; k < sc.scans; ++k) {
        const ProgScan &c = sc.scan[k];
        total += prog_scan_dht_max(c) + (uint64_t)(8 + 2 * popcount3(c.mask)) + scan_bound(prog_scan_blocks(g, c), prog_scan_block_bits(c));
    }
    return total;
}

// Tests: the symbol counts of the context's last call of the script entries, [pictures][tables][256] in the file's table order;
// `tables`: the tables of that call's script.  JPEGAMD_ERR_ARG when the last call with per-scan tables was not one of them.
extern "C" int32_t jpegamd_debug_progressive_script_counts(JpegAmdEncoder *e, uint64_t *counts, int32_t tables) {
    return debug_prog_counts(e, counts, tables, 2);
}

// Host-only (tests): whether the plain build has the k_tile_encode instantiation (taps, layout, chroma tables, expand): 1 or 0.  No
// device is needed.  Not part of the public header.
extern "C" int32_t jpegamd_debug_tile_variant(int32_t taps, int32_t layout, int32_t chroma, int32_t expand) {
    return tile_variant_exists(taps != 0, TileSource{layout, chroma != 0, expand != 0}) ? 1 : 0;
}

extern "C" int32_t jpegamd_encode_ycbcr_interleaved_batch_async(JpegAmdEncoder *e, const JpegAmdYCbCrImage *imgs, int32_t count, int32_t subsampling,
                                                                void *const *outs_dev, uint64_t out_capacity, void *const *out_sizes_dev,
                                                                void *stream_) {
    return jpegamd_encode_ycbcr_interleaved_restart_batch_async(e, imgs, count, subsampling, 0, outs_dev, out_capacity, out_sizes_dev, stream_);
}

// The capacity status is STICKY on the device: every kernel only ORs into it, and it is cleared here, after it was read.
// A pipelined caller that keeps several encodes in flight on one context therefore learns about an overflow in ANY of
// them (JPEGAMD_ERR_HUFF_CAPACITY, jpeg_compression.c:205-206) at its next finish; which one it was follows from the sizes
// (*out_size_dev holds the would-be size of each call even when it did not fit).
extern "C" int32_t jpegamd_encoder_finish(JpegAmdEncoder *e, JpegAmdStats *stats) {
    if (!e) return JPEGAMD_ERR_ARG;
    if (!e->pending) return JPEGAMD_ERR_ARG;
    if (stats && !e->last_color)        // symbol / exact-path totals are only summed when somebody asks (a colour call summed its own)
        if (launch_sum_stats(e->seg.syms, e->seg.exact, e->last_segs, e->stats_dev, e->last_stream)) return JPEGAMD_ERR_HIP;
    HIP_TRY(hipStreamSynchronize(e->last_stream));
    e->pending = false;
    HIP_TRY(hipMemcpy(&e->mirror, e->stats_dev, sizeof(ScanStats), hipMemcpyDeviceToHost));
    if (e->mirror.status) HIP_TRY(hipMemset(&e->stats_dev->status, 0, sizeof(uint32_t)));
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->jfif_bytes = e->mirror.out_size;
        stats->entropy_bits = e->mirror.total_bits;
        stats->stuffed_bytes = e->mirror.total_ff;
        stats->exact_fallbacks = e->mirror.total_exact;
        if (e->timed) {
            int32_t rc = read_slot(e, e->last_slot, stats);
            if (rc) return rc;
        }
    }
    if (e->mirror.status & 4u) return JPEGAMD_ERR_HIP;              // a look-back of k_stitch gave up waiting (never seen; the spins are bounded so that it cannot hang)
    if (e->mirror.status & 2u) return JPEGAMD_ERR_RLE_CAPACITY;     // a tile record outside its reservation (corrupt scratch)
    return (e->mirror.status & 1u) ? JPEGAMD_ERR_HUFF_CAPACITY : JPEGAMD_OK;
}

// Symbols coded by the last finished call (DTO rle_count).
static uint64_t last_symbol_count(const JpegAmdEncoder *e) { return e->mirror.total_syms; }

extern "C" int32_t jpegamd_debug_stages(JpegAmdEncoder *e, const JpegAmdImage *img, int8_t *y_centered,
                                        int16_t *quant_zigzag, uint64_t *exact_mask) {
    if (!e || !e->meta.empty()) return JPEGAMD_ERR_ARG;            // (no file, so no metadata: refused while some is set)
    ImageDesc im;
    int32_t rc = describe(e, img, &im);
    if (rc) return rc;
    rc = prepare_constants(e, img, false);
    if (rc) return rc;
    if (launch_transform_and_entropy(e, im, true, y_centered, quant_zigzag, exact_mask, nullptr, nullptr, src_of(img))) return JPEGAMD_ERR_HIP;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return JPEGAMD_OK;
}

// Fault injection (tests): the next encode on this context finds `value` in word 0 (the string's bit count) of tile `tile`'s
// record when k_segment_merge reads it.  Not part of the public header.
extern "C" int32_t jpegamd_debug_poison_tile_record(JpegAmdEncoder *e, int32_t tile, uint32_t value) {
    if (!e || tile < 0 || tile >= e->lim.max_tiles) return JPEGAMD_ERR_ARG;
    e->poison_tile = tile;
    e->poison_value = value;
    return JPEGAMD_OK;
}

// Diagnostic: copy the per-wave phase cycle sums of the last launch (null unless JPEGAMD_STAMPS is set
// in the environment AND the library was built with -DJPEGAMD_STAMPS).  Not part of the public header.
extern "C" int32_t jpegamd_debug_read_stamps(JpegAmdEncoder *e, unsigned long long *host, int64_t nwaves) {
    if (!e || !e->stamps_dev || !host || nwaves > (int64_t)(stamp_words(e->lim.max_segs) / 16)) return JPEGAMD_ERR_ARG;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(host, e->stamps_dev, (size_t)nwaves * 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return JPEGAMD_OK;
}

extern "C" int32_t jpegamd_debug_dct_exact(JpegAmdEncoder *e, const int8_t *blocks, float *coeffs, int64_t nblocks) {
    if (!e || !blocks || !coeffs || nblocks < 0) return JPEGAMD_ERR_ARG;
    if (launch_dct_exact(blocks, coeffs, nblocks, nullptr)) return JPEGAMD_ERR_HIP;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return JPEGAMD_OK;
}

// ---------------------------------------------------------------------------------------
// Level 2: JpegCompression_Init / convertToJpeg
// ---------------------------------------------------------------------------------------
static std::mutex g_mu;
static JpegAmdEncoder *g_ctx = nullptr;
static uint64_t *g_size_dev = nullptr;

static int32_t ensure_ctx(int w, int h) {
    if (g_ctx && context_fits(g_ctx, w, h)) return JPEGAMD_OK;
    int mw = w, mh = h;
    if (g_ctx) {
        if (g_ctx->max_w > mw) mw = g_ctx->max_w;
        if (g_ctx->max_h > mh) mh = g_ctx->max_h;
        jpegamd_encoder_destroy(g_ctx);
        g_ctx = nullptr;
    }
    int32_t rc = jpegamd_encoder_create(&g_ctx, mw, mh);
    if (rc) return rc;
    if (!g_size_dev) HIP_TRY(hipMalloc((void **)&g_size_dev, 16));
    return JPEGAMD_OK;
}

extern "C" int32_t JpegCompression_Init(void) {
    // dsp_port/jpeg_compression/src/jpeg_compression.c:18-33: 0 on success.
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_ctx) return 0;
    const char *env = std::getenv("JPEGAMD_INIT_DIM");
    int dim = env ? std::atoi(env) : 2048;
    if (dim <= 0) dim = 2048;
    return ensure_ctx(dim, dim);
}

extern "C" int32_t JpegCompression_Reserve(int32_t max_width, int32_t max_height) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (max_width <= 0 || max_height <= 0) return JPEGAMD_ERR_ARG;
    return ensure_ctx(max_width, max_height);
}

extern "C" int32_t JpegCompression_DeInit(void) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (g_ctx) { jpegamd_encoder_destroy(g_ctx); g_ctx = nullptr; }
    if (g_size_dev) { hipFree(g_size_dev); g_size_dev = nullptr; }
    return 0;
}

// Shared by convertToJpeg and the natural_c-shaped host functions (host_compat.cpp).
namespace jpegamd {
JpegAmdEncoder *shared_context(int w, int h, uint64_t **size_dev) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (ensure_ctx(w, h) != JPEGAMD_OK) return nullptr;
    if (size_dev) *size_dev = g_size_dev;
    return g_ctx;
}
}  // namespace jpegamd

namespace jpegamd {
// Block (0,0) through the stage taps: centred luma, exact-order DCT, quantised zigzag.
int32_t first_block_taps(JpegAmdEncoder *e, const JpegAmdImage *img, int8_t y[64], float dct[64], int16_t zz[64]) {
    ImageDesc im;
    int32_t rc = prepare_constants(e, img, false);
    if (rc) return rc;
    rc = describe(e, img, &im);
    if (rc) return rc;
    im.blocks_w = 1; im.blocks_h = 1; im.segs_per_row = 1; im.num_segs = 1;   // block (0,0) only
    im.tiles_per_row = 1; im.num_tiles = 1; im.tile_begin = 0; im.tile_end = 1; im.seg_begin = 0; im.seg_end = 1;
    int8_t *y_dev = nullptr; int16_t *zz_dev = nullptr; float *dct_dev = nullptr;
    int err = (int)hipMalloc((void **)&y_dev, 64);              // (every exit path below frees what was allocated)
    if (!err) err = (int)hipMalloc((void **)&zz_dev, 128);
    if (!err) err = (int)hipMalloc((void **)&dct_dev, 256);
    if (!err) err = launch_transform_and_entropy(e, im, true, y_dev, zz_dev, nullptr, nullptr, nullptr, src_of(img));
    if (!err) err = launch_dct_exact(y_dev, dct_dev, 1, nullptr);
    if (!err) err = (int)hipMemcpy(y, y_dev, 64, hipMemcpyDeviceToHost);
    if (!err) err = (int)hipMemcpy(zz, zz_dev, 128, hipMemcpyDeviceToHost);
    if (!err) err = (int)hipMemcpy(dct, dct_dev, 256, hipMemcpyDeviceToHost);
    hipFree(y_dev); hipFree(zz_dev); hipFree(dct_dev);
    return err ? JPEGAMD_ERR_HIP : JPEGAMD_OK;
}
}  // namespace jpegamd

extern "C" int32_t convertToJpeg(JPEG_COMPRESSION_DTO *dto) {
    if (!dto || is_px4(dto->channel_order)) return JPEGAMD_ERR_ARG;     // (the DTO boundary takes the reference's 3-byte and 1-byte layouts)
    {
        std::lock_guard<std::mutex> lk(g_mu);
        if (!g_ctx) return JPEGAMD_ERR_NOT_INIT;
    }
    if (dto->gb_phy_ptr != 0 || dto->rle_phy_ptr != 0) return JPEGAMD_ERR_ARG;
    uint64_t *size_dev = nullptr;
    JpegAmdEncoder *e = shared_context(dto->width > 0 ? dto->width : 1, dto->height > 0 ? dto->height : 1, &size_dev);
    if (!e) return JPEGAMD_ERR_NO_DEVICE;

    JpegAmdImage img;
    img.pixels = (const void *)(uintptr_t)dto->r_phy_ptr;
    img.width = dto->width; img.height = dto->height; img.row_stride = dto->row_stride;
    img.bottom_up = dto->bottom_up; img.channel_order = dto->channel_order; img.quality = dto->quality;

    if (e->ring.empty()) {
        int32_t prc = jpegamd_encoder_set_profiling(e, 1);     // the DTO always reports stage times
        if (prc) return prc;
    }
    // the six stage counters (jpeg_compression.c:188-210) come from the STAMPED variant of the fused kernel: the same code with its
    // phases bracketed by cycle-counter reads (~10 % slower; the asynchronous entry points never run it)
    const size_t stamp_bytes = stamp_words(e->lim.max_segs) * sizeof(unsigned long long);
    if (!e->stamps_dev) HIP_TRY(hipMalloc((void **)&e->stamps_dev, stamp_bytes));
    HIP_TRY(hipMemsetAsync(e->stamps_dev, 0, stamp_bytes, nullptr));
    e->stamp_next = true;
    int32_t rc = jpegamd_encode_async(e, &img, (void *)(uintptr_t)dto->huff_phy_ptr, dto->huff_size, size_dev, 0, nullptr);
    JpegAmdStats st;
    if (rc == JPEGAMD_OK) rc = jpegamd_encoder_finish(e, &st);
    if (rc != JPEGAMD_OK) return rc;   // -8 when huff_size was too small (jpeg_compression.c:205-206)

    dto->huff_size = (uint32_t)st.jfif_bytes;
    dto->rle_count = (uint32_t)last_symbol_count(e);
    // Stage counters (jpeg_compression.c:188-210 fills six), in nanoseconds.  Colour conversion, DCT, quantisation, run/size symbols
    // and Huffman coding are phases of ONE kernel here; this call ran its STAMPED variant (above), whose in-kernel cycle-counter
    // reads split the kernel's duration by the phases' shares of the waves' time.  Zigzag is the row order of the matrix operand
    // (no instruction, no phase): its counter stays 0.  cycles_rle / cycles_huffman also carry the stitching kernels.
    dto->cycles_color_conversion = 0;
    dto->cycles_dct = st.ns_transform;
    dto->cycles_quantization = 0;
    dto->cycles_zigzag = 0;
    dto->cycles_rle = st.ns_entropy;
    dto->cycles_huffman = st.ns_pack;
    dto->cycles_total = st.ns_total;
    if (e->stamps_dev) {
        const int tiles = tiles_for(dto->width, dto->height);
        const int wgs = (tiles + 7) / 8 < 512 ? (tiles + 7) / 8 : 512;
        std::vector<unsigned long long> stamps((size_t)wgs * 8 * 16);
        if (hipMemcpy(stamps.data(), e->stamps_dev, stamps.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess) {
            double ph[11] = {0};
            for (size_t w = 0; w < (size_t)wgs * 8; ++w)
                for (int i = 0; i < 11; ++i) ph[i] += (double)stamps[w * 16 + i];
            double all = 0;
            for (double v : ph) all += v;
            if (all > 0) {
                const double k = (double)st.ns_transform / all;
                // phases: 0 loop, 1 wait rows + luma, 2 luma -> LDS, 3 MFMA, 4 quantise, 5 exact order, 6 counts, 7 ticket / row
                // requests, 8 appends, 9 coding, 10 record / copy-out; the loop's own overhead (0, 7) goes with the colour stage
                dto->cycles_color_conversion = (uint64_t)(k * (ph[0] + ph[1] + ph[2] + ph[7]));
                dto->cycles_dct = (uint64_t)(k * ph[3]);
                dto->cycles_quantization = (uint64_t)(k * (ph[4] + ph[5]));
                dto->cycles_rle = (uint64_t)(k * (ph[6] + ph[8])) + st.ns_entropy;
                dto->cycles_huffman = (uint64_t)(k * (ph[9] + ph[10])) + st.ns_pack;
            }
        }
    }

    // First-block debug taps (jpeg_compression.c:150-169), host pointers.
    if (dto->y_phy_ptr || dto->dct_phy_ptr || dto->quant_phy_ptr || dto->zigzag_phy_ptr) {
        int8_t y[64]; int16_t zz[64]; float dct[64];
        rc = first_block_taps(e, &img, y, dct, zz);
        if (rc) return rc;
        if (dto->y_phy_ptr) std::memcpy((void *)(uintptr_t)dto->y_phy_ptr, y, 64);
        if (dto->dct_phy_ptr) std::memcpy((void *)(uintptr_t)dto->dct_phy_ptr, dct, 256);
        if (dto->zigzag_phy_ptr) std::memcpy((void *)(uintptr_t)dto->zigzag_phy_ptr, zz, 128);
        if (dto->quant_phy_ptr) {
            int16_t raster[64];
            for (int i = 0; i < 64; ++i) raster[kZigzagHost[i]] = zz[i];
            std::memcpy((void *)(uintptr_t)dto->quant_phy_ptr, raster, 128);
        }
    }
    return 0;
}

extern "C" int32_t JpegCompression_RemoteServiceHandler(char *service_name, uint32_t cmd, void *prm, uint32_t prm_size,
                                                        uint32_t flags) {
    // dsp_port/jpeg_compression/src/jpeg_compression.c:6-14: cast and forward.
    (void)service_name; (void)cmd; (void)flags;
    if (!prm || prm_size < sizeof(JPEG_COMPRESSION_DTO)) return JPEGAMD_ERR_ARG;
    return convertToJpeg((JPEG_COMPRESSION_DTO *)prm);
}
