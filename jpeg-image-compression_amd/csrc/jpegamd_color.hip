// jpegamd_color.hip -- the two kernels of a colour encode (jpegamd_encode_color_async) besides the grayscale pipeline's own.
//
// A colour file is three non-interleaved baseline scans (colour scans): Y through the unchanged RGB path of
// k_tile_encode, then Cb and Cr as 8-bit planes through its one-byte mode with the chroma tables.
//   k_chroma_planes   the picture, read once in any layout the API accepts -> the Cb and Cr planes in context scratch
//   k_append_scans    the two chroma scans (coded into context scratch) copied behind the Y scan in the caller's buffer, at the
//                     offsets the device computed: no host synchronisation between the scans
// A colour batch (jpegamd_encode_color_batch_async) has batched forms of both, and one kernel more:
//   k_chroma_planes_batch  every picture of the batch -> 2 x batch planes at one pitch, in one launch
//   k_picture_stats        per picture and scan: bits, symbols and exact-order fallbacks from one launch's tile records
//   k_append_scans_batch   per picture: SOS(2), Cb, SOS(3), Cr, EOI behind its Y scan, when the whole file fits
#include <hip/hip_ext.h>
#include "jpegamd_device.h"

namespace jpegamd {

// Cb = (32768 - 43 R - 85 G + 128 B) >> 8, Cr = (32768 + 128 R - 107 G - 21 B) >> 8 (the sums lie in [128, 65408]: no clamp).
__device__ __forceinline__ void cbcr(int r, int g, int b, int &cb, int &cr) {
    cb = (32768 - 43 * r - 85 * g + 128 * b) >> 8;
    cr = (32768 + 128 * r - 107 * g - 21 * b) >> 8;
}

constexpr int kPlaneOut = 4;              // chroma samples per thread: one 4-byte store per plane (the pitch is a multiple of 4)

// kSx x kSy pixels per sample: 2 x 2 (4:2:0), 2 x 1 (4:2:2: one source row per plane row) or 1 x 1 (4:4:4).  Thread (gx, cy) makes
// samples 4 gx .. 4 gx + 3 of plane row cy.
template <int kSx, int kSy>
__global__ __launch_bounds__(256) void k_chroma_planes(const ChromaPlanesArgs a) {
    static_assert((kSx == 1 || kSx == 2) && (kSy == 1 || kSy == 2) && kSy <= kSx, "4:4:4, 4:2:2 or 4:2:0");
    constexpr int kPix = kPlaneOut * kSx;                                    // source pixels per row and thread
    const int gx = (int)(blockIdx.x * blockDim.x + threadIdx.x), cy = (int)blockIdx.y;
    const int x0 = gx * kPix;
    if (kPlaneOut * gx >= a.cw) return;                                      // (then x0 < width as well)
    int cb[kSy][kPix], cr[kSy][kPix];
#pragma unroll
    for (int r = 0; r < kSy; ++r) {
        const int y = min(cy * kSy + r, a.height - 1);                      // the last row replicated (odd heights)
        const int stored = a.bottom_up ? a.height - 1 - y : y;
        const uint8_t *row = a.pixels + (size_t)stored * (size_t)a.row_stride;
        uint8_t px[3 * kPix];
        if ((((uintptr_t)row) & 3u) == 0 && x0 + kPix <= a.width) {         // whole dwords (3 kPix bytes from a multiple of 12)
            const uint32_t *src = reinterpret_cast<const uint32_t *>(row + 3 * (size_t)x0);
#pragma unroll
            for (int i = 0; i < 3 * kPix / 4; ++i) {
                const uint32_t d = src[i];
#pragma unroll
                for (int k = 0; k < 4; ++k) px[4 * i + k] = (uint8_t)(d >> (8 * k));
            }
        } else {                                                             // the right edge (replicated), or an unaligned row
#pragma unroll
            for (int j = 0; j < kPix; ++j) {
                const uint8_t *p = row + 3 * (size_t)min(x0 + j, a.width - 1);
                px[3 * j] = p[0]; px[3 * j + 1] = p[1]; px[3 * j + 2] = p[2];
            }
        }
#pragma unroll
        for (int j = 0; j < kPix; ++j) {
            const int c0 = px[3 * j], c1 = px[3 * j + 1], c2 = px[3 * j + 2];
            cbcr(a.rgb ? c0 : c2, c1, a.rgb ? c2 : c0, cb[r][j], cr[r][j]);
        }
    }
    uint32_t wcb = 0, wcr = 0;
#pragma unroll
    for (int k = 0; k < kPlaneOut; ++k) {
        int vb, vr;
        if (kSx == 2) {
            // the pair's right pixel is the replicated last column when 2 x + 1 == width; (a + b + c + d + 2) >> 2, or (a + b + 1) >> 1
            const int j0 = 2 * k, j1 = x0 + 2 * k + 1 < a.width ? 2 * k + 1 : 2 * k;
            if (kSy == 2) {
                vb = (cb[0][j0] + cb[0][j1] + cb[kSy - 1][j0] + cb[kSy - 1][j1] + 2) >> 2;
                vr = (cr[0][j0] + cr[0][j1] + cr[kSy - 1][j0] + cr[kSy - 1][j1] + 2) >> 2;
            } else {
                vb = (cb[0][j0] + cb[0][j1] + 1) >> 1;
                vr = (cr[0][j0] + cr[0][j1] + 1) >> 1;
            }
        } else {
            vb = cb[0][k]; vr = cr[0][k];
        }
        wcb |= (uint32_t)vb << (8 * k);
        wcr |= (uint32_t)vr << (8 * k);
    }
    const size_t o = (size_t)cy * (size_t)a.pitch + (size_t)kPlaneOut * gx;  // < pitch: 4 gx < cw <= pitch (a multiple of 4)
    *reinterpret_cast<uint32_t *>(a.cb + o) = wcb;
    *reinterpret_cast<uint32_t *>(a.cr + o) = wcr;
}

int launch_chroma_planes(const ChromaPlanesArgs &a, void *stream, void *const *ev) {
    if (a.cw <= 0 || a.ch <= 0 || a.pitch % 4 != 0 || a.pitch < (a.cw + 3) / 4 * 4) return (int)hipErrorInvalidValue;
    const int threads_x = (a.cw + kPlaneOut - 1) / kPlaneOut;
    const dim3 grid((unsigned)((threads_x + 255) / 256), (unsigned)a.ch), block(256);
    if (a.mode != kChromaMode444 && a.mode != kChromaMode420 && a.mode != kChromaMode422) return (int)hipErrorInvalidValue;
    const auto kernel = a.mode == kChromaMode420 ? k_chroma_planes<2, 2> : (a.mode == kChromaMode422 ? k_chroma_planes<2, 1> : k_chroma_planes<1, 1>);
    if (ev) hipExtLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)stream, (hipEvent_t)ev[0], (hipEvent_t)ev[1], 0, a);
    else hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

// Every workgroup derives the same offsets from the three sizes; 16 bytes per thread and step (aligned 16-byte reads of the
// scratch, byte writes: the destination offset is arbitrary).  Nothing is written unless the whole file fits.
constexpr int kAppendWgs = 256;
__global__ __launch_bounds__(256) void k_append_scans(const AppendArgs a) {
    const uint64_t s0 = a.scan_size[0], s1 = a.scan_size[1], s2 = a.scan_size[2];
    const uint32_t st = a.scan_stats[0].status | a.scan_stats[1].status | a.scan_stats[2].status;
    const uint64_t total = s0 + s1 + s2;
    const bool fit = (st & 1u) == 0u && total <= a.out_capacity;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *a.out_size = fit ? total : 0ull;
        ScanStats *t = a.stats;
        t->out_size = fit ? total : 0ull;
        t->total_bits = a.scan_stats[0].total_bits + a.scan_stats[1].total_bits + a.scan_stats[2].total_bits;
        t->total_ff = a.scan_stats[0].total_ff + a.scan_stats[1].total_ff + a.scan_stats[2].total_ff;
        t->total_syms = a.scan_stats[0].total_syms + a.scan_stats[1].total_syms + a.scan_stats[2].total_syms;
        t->total_exact = a.scan_stats[0].total_exact + a.scan_stats[1].total_exact + a.scan_stats[2].total_exact;
        const uint32_t add = st | (fit ? 0u : 1u);
        if (add) atomicOr(&t->status, add);
    }
    if (!fit) return;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x * 16u;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const uint64_t n = c ? s2 : s1;
        uint8_t *dst = a.out + (c ? s0 + s1 : s0);
        const uint8_t *src = a.src[c];
        for (uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16u; i < n; i += stride) {
            const uint4 v = *reinterpret_cast<const uint4 *>(src + i);          // (the scratch is padded to 16 bytes)
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            const uint64_t m = n - i < 16u ? n - i : 16u;
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if ((uint64_t)k < m) dst[i + k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
        }
    }
}

int launch_append_scans(const AppendArgs &a, void *stream, void *const *ev) {
    if (ev) hipExtLaunchKernelGGL(k_append_scans, dim3(kAppendWgs), dim3(256), 0, (hipStream_t)stream, (hipEvent_t)ev[0], (hipEvent_t)ev[1], 0, a);
    else hipLaunchKernelGGL(k_append_scans, dim3(kAppendWgs), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

// ---- colour batches (jpegamd_encode_color_batch_async) --------------------------------------------------------------------
// k_chroma_planes_batch: workgroup (bx, cy, p) makes samples [1024 bx, 1024 bx + 1024) of plane row cy of picture p, both planes.
// The source rows it needs (3 x 2048 bytes twice at 4:2:0, once at 4:2:2, 3 x 1024 bytes at 4:4:4) are staged in LDS by aligned 16-byte loads --
// one instruction covers 1 KiB of a row -- and every thread then reads its pixels from LDS as dwords, funnel-shifted by the row's
// misalignment.  Only chunks that lie wholly inside the row's bytes are loaded as vectors; the partial chunks at both
// ends are gathered byte by byte.  The arithmetic is k_chroma_planes's: the planes are the same, bit for bit.
// kLay is how the picture is stored: 3 or 4 bytes per pixel in one stream of bytes (the fourth byte is never looked at), or
// three streams -- the R, G and B planes -- of one byte per pixel, each staged like a row a third as long.
constexpr int kPbThreads = 256;
constexpr int kPbSpan = kPbThreads * kPlaneOut;            // plane samples per workgroup and row

template <int kSx, int kSy, int kLay>
__global__ __launch_bounds__(kPbThreads) void k_chroma_planes_batch(const ChromaPlanesBatchArgs a) {
    constexpr bool kPlanar = kLay == kChromaSrcPlanar;
    constexpr int kStreams = kPlanar ? 3 : 1;
    constexpr int kBpp = kPlanar ? 1 : (kLay == kChromaSrcPx4 ? 4 : 3);  // bytes per pixel of one stream
    static_assert((kSx == 1 || kSx == 2) && (kSy == 1 || kSy == 2) && kSy <= kSx, "4:4:4, 4:2:2 or 4:2:0");
    constexpr int kPix = kPlaneOut * kSx;                                // source pixels per row and thread
    constexpr int kRowBytes = kBpp * kSx * kPbSpan;                     // source bytes per row, stream and workgroup
    constexpr int kLdsBytes = kRowBytes + 32;                            // + the misalignment (< 16) and the funnel's extra dword
    constexpr int kDw = kBpp * kPix / 4;                                 // dwords of a thread's pixels in one stream
    __shared__ __attribute__((aligned(16))) uint8_t s_row[kSy][kStreams][kLdsBytes];
    const int p = (int)blockIdx.z, cy = (int)blockIdx.y, t = (int)threadIdx.x;
    const int s0 = (int)blockIdx.x * kPbSpan;                            // < cw
    const int x0 = s0 * kSx;                                             // < width
    const int x_end = min(x0 + kSx * kPbSpan, a.width);
    int mis[kSy][kStreams];
#pragma unroll
    for (int r = 0; r < kSy; ++r) {
        const int y = min(cy * kSy + r, a.height - 1);                  // the last row replicated (odd heights)
        const int stored = a.bottom_up ? a.height - 1 - y : y;
#pragma unroll
        for (int st = 0; st < kStreams; ++st) {
            const uint8_t *pic = st == 0 ? a.pixels[p] : (st == 1 ? a.pixels_g[p] : a.pixels_b[p]);
            const uintptr_t row = (uintptr_t)pic + (size_t)stored * (size_t)a.row_stride;
            const uintptr_t row_end = row + kBpp * (size_t)a.width;
            const uintptr_t base = row + kBpp * (size_t)x0;
            const int m = (int)(base & 15u);
            mis[r][st] = m;
            const uintptr_t abase = base - (uintptr_t)m;
            const int nch = (m + kBpp * (x_end - x0) + 15) >> 4;        // <= kRowBytes / 16 + 1
            for (int c = t; c < nch; c += kPbThreads) {
                const uintptr_t g = abase + 16u * (uintptr_t)c;
                uint4 v;
                if (g >= row && g + 16u <= row_end) {
                    v = *reinterpret_cast<const uint4 *>(g);
                } else {                                                 // a partial chunk at either end of the row
                    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                    for (int k = 0; k < 16; ++k)
                        if (g + k >= row && g + k < row_end) w[k >> 2] |= (uint32_t)(*reinterpret_cast<const uint8_t *>(g + k)) << (8 * (k & 3));
                    v = make_uint4(w[0], w[1], w[2], w[3]);
                }
                *reinterpret_cast<uint4 *>(&s_row[r][st][16 * c]) = v;
            }
        }
    }
    __syncthreads();
    const int s = s0 + kPlaneOut * t;
    if (s >= a.cw) return;
    const int xs = s * kSx;                                              // the thread's first pixel
    int cb[kSy][kPix], cr[kSy][kPix];
#pragma unroll
    for (int r = 0; r < kSy; ++r) {
        uint8_t px[kStreams][kBpp * kPix];
#pragma unroll
        for (int st = 0; st < kStreams; ++st) {
            if (xs + kPix <= a.width) {                                  // whole pixels: kDw dwords behind the misalignment
                const int off = mis[r][st] + kBpp * (xs - x0);
                const uint32_t *w32 = reinterpret_cast<const uint32_t *>(&s_row[r][st][off & ~3]);
                const uint32_t sh = (uint32_t)(off & 3);
                uint32_t d[kDw + 1];
#pragma unroll
                for (int i = 0; i < kDw + 1; ++i) d[i] = w32[i];
#pragma unroll
                for (int i = 0; i < kDw; ++i) {
                    const uint32_t v = __builtin_amdgcn_alignbyte(d[i + 1], d[i], sh);
#pragma unroll
                    for (int k = 0; k < 4; ++k) px[st][4 * i + k] = (uint8_t)(v >> (8 * k));
                }
            } else {                                                     // the right edge: the last column replicated
#pragma unroll
                for (int j = 0; j < kPix; ++j) {
                    const int off = mis[r][st] + kBpp * (min(xs + j, a.width - 1) - x0);
#pragma unroll
                    for (int k = 0; k < (kBpp < 3 ? kBpp : 3); ++k) px[st][kBpp * j + k] = s_row[r][st][off + k];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kPix; ++j) {
            if constexpr (kPlanar) {
                cbcr(px[0][j], px[1][j], px[2][j], cb[r][j], cr[r][j]);
            } else {
                const int c0 = px[0][kBpp * j], c1 = px[0][kBpp * j + 1], c2 = px[0][kBpp * j + 2];
                cbcr(a.rgb ? c0 : c2, c1, a.rgb ? c2 : c0, cb[r][j], cr[r][j]);
            }
        }
    }
    uint32_t wcb = 0, wcr = 0;
#pragma unroll
    for (int k = 0; k < kPlaneOut; ++k) {
        int vb, vr;
        if (kSx == 2) {
            const int j0 = 2 * k, j1 = xs + 2 * k + 1 < a.width ? 2 * k + 1 : 2 * k;
            if (kSy == 2) {
                vb = (cb[0][j0] + cb[0][j1] + cb[kSy - 1][j0] + cb[kSy - 1][j1] + 2) >> 2;
                vr = (cr[0][j0] + cr[0][j1] + cr[kSy - 1][j0] + cr[kSy - 1][j1] + 2) >> 2;
            } else {
                vb = (cb[0][j0] + cb[0][j1] + 1) >> 1;
                vr = (cr[0][j0] + cr[0][j1] + 1) >> 1;
            }
        } else {
            vb = cb[0][k]; vr = cr[0][k];
        }
        wcb |= (uint32_t)vb << (8 * k);
        wcr |= (uint32_t)vr << (8 * k);
    }
    uint8_t *cbp = a.planes + (size_t)(2 * p) * a.plane_bytes;
    const size_t o = (size_t)cy * (size_t)a.pitch + (size_t)s;           // s % 4 == 0, s < cw <= pitch (a multiple of 4)
    *reinterpret_cast<uint32_t *>(cbp + o) = wcb;
    *reinterpret_cast<uint32_t *>(cbp + a.plane_bytes + o) = wcr;
}

template <int kLay>
static void launch_planes_batch_as(const ChromaPlanesBatchArgs &a, dim3 grid, dim3 block, hipStream_t stream, hipEvent_t e0, hipEvent_t e1) {
    if (a.mode == kChromaMode420) hipExtLaunchKernelGGL((k_chroma_planes_batch<2, 2, kLay>), grid, block, 0, stream, e0, e1, 0, a);
    else if (a.mode == kChromaMode422) hipExtLaunchKernelGGL((k_chroma_planes_batch<2, 1, kLay>), grid, block, 0, stream, e0, e1, 0, a);
    else hipExtLaunchKernelGGL((k_chroma_planes_batch<1, 1, kLay>), grid, block, 0, stream, e0, e1, 0, a);
}

int launch_chroma_planes_batch(const ChromaPlanesBatchArgs &a, void *stream, void *const *ev) {
    if (a.cw <= 0 || a.ch <= 0 || a.batch < 1 || a.batch > kMaxBatch || a.pitch % 4 != 0 || a.pitch < (a.cw + 3) / 4 * 4 ||
        a.plane_bytes % 16 != 0 || a.plane_bytes < (uint64_t)a.pitch * (uint64_t)a.ch ||
        (a.mode != kChromaMode444 && a.mode != kChromaMode420 && a.mode != kChromaMode422))
        return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.cw + kPbSpan - 1) / kPbSpan), (unsigned)a.ch, (unsigned)a.batch), block(kPbThreads);
    hipEvent_t e0 = ev ? (hipEvent_t)ev[0] : nullptr, e1 = ev ? (hipEvent_t)ev[1] : nullptr;
    if (a.layout == kChromaSrcPx3) launch_planes_batch_as<kChromaSrcPx3>(a, grid, block, (hipStream_t)stream, e0, e1);
    else if (a.layout == kChromaSrcPx4) launch_planes_batch_as<kChromaSrcPx4>(a, grid, block, (hipStream_t)stream, e0, e1);
    else if (a.layout == kChromaSrcPlanar) launch_planes_batch_as<kChromaSrcPlanar>(a, grid, block, (hipStream_t)stream, e0, e1);
    else return (int)hipErrorInvalidValue;
    return (int)hipGetLastError();
}

// One thread per tile: the record's string bits, plus the DC symbol of the tile's first block as k_segment_merge codes it
// (predicted from the tile in front, 0 for a picture's first tile).
__global__ __launch_bounds__(256) void k_picture_stats(const PictureStatsArgs a) {
    __shared__ unsigned long long s_part[3][4];
    const int i = (int)blockIdx.y, t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    unsigned long long v[3] = {0ull, 0ull, 0ull};
    if (t < a.tiles_per_image) {
        const uint32_t *rec = a.tile_head + ((size_t)i * (size_t)a.tiles_per_image + (size_t)t) * kTileHeadWords;
        const uint4 r = *reinterpret_cast<const uint4 *>(rec);           // {string bits, first DC, last DC, exact-order fallbacks}
        const int pred = t > 0 ? (int)rec[2 - kTileHeadWords] : 0;
        const int diff = (int)(short)(((int)r.y - pred) & 0xFFFF);
        const uint32_t mag = (uint32_t)(diff < 0 ? -diff : diff);
        const uint32_t nb = mag ? 32u - (uint32_t)__clz((int)mag) : 0u;
        v[0] = (unsigned long long)min(r.x, (uint32_t)(kTileBlocks * kMaxBlockBits)) + (a.huff[256 + (nb & 15u)] >> 16) + nb;
        v[1] = rec[4];
        v[2] = r.w;
    }
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off, 64);
        if (lane == 0) s_part[k][wave] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int k = (int)threadIdx.x;
        const unsigned long long sum = s_part[k][0] + s_part[k][1] + s_part[k][2] + s_part[k][3];
        const int q = a.first_plane + i;
        const int slot = a.chroma ? (q >> 1) * kPicStatWords + 3 * (1 + (q & 1)) : i * kPicStatWords;
        if (sum) atomicAdd(a.pic + slot + k, sum);
    }
}

int launch_picture_stats(const PictureStatsArgs &a, void *stream) {
    if (a.tiles_per_image <= 0 || a.batch <= 0) return 0;
    hipLaunchKernelGGL(k_picture_stats, dim3((unsigned)((a.tiles_per_image + 255) / 256), (unsigned)a.batch), dim3(256), 0,
                       (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

// Workgroup (bx, p): picture p.  Every workgroup of a picture derives the same sizes and the same verdict; (0, p) writes the
// headers and the size, (0, 0) the context's record.
constexpr int kAppendBatchWgs = 64;
__global__ __launch_bounds__(256) void k_append_scans_batch(const AppendBatchArgs a) {
    const int p = (int)blockIdx.y;
    // Launch 0 is the Y batch: its capacity bit (0) only says that SOME picture's Y scan outgrew out_capacity, which the sizes
    // below tell picture by picture.  Every other status is "hard" and fails every picture: a corrupt record or a look-back that
    // gave up (bits 1, 2) anywhere, and bit 0 of a chroma launch.  A chroma scan cannot outgrow its slot -- the slot holds
    // scan_bound(), the plane's worst case, plus 64 bytes -- but if one ever did, its size would point past the slot into the
    // next plane's, and nothing may be copied from it.
    uint32_t st = a.launch_stats[0].status, hard = st & ~1u;
    for (int l = 1; l < a.n_launch; ++l) { st |= a.launch_stats[l].status; hard |= a.launch_stats[l].status; }
    const auto total_of = [&](int q) { return a.y_size[q] + kSosBytes + a.c_size[2 * q] + kSosBytes + a.c_size[2 * q + 1] + 2u; };
    const uint64_t total = total_of(p);
    const bool fit = hard == 0u && total <= a.out_capacity;
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < 64) {
        const int q = (int)threadIdx.x;
        unsigned long long bits = 0, ff = 0, syms = 0, exact = 0, fail = 0;
        if (q < a.batch) {
            const unsigned long long *s = a.pic + (size_t)q * kPicStatWords;
            const uint64_t size[3] = {a.y_size[q] - (uint64_t)a.hdr_len, a.c_size[2 * q], a.c_size[2 * q + 1]};
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                bits += s[3 * k];
                ff += size[k] - (s[3 * k] + 7u) / 8u;                    // a scan is its bits, the flush byte, and a 0x00 per 0xFF
                syms += s[3 * k + 1];
                exact += s[3 * k + 2];
            }
            fail = (hard == 0u && total_of(q) <= a.out_capacity) ? 0ull : 1ull;
        }
        for (int off = 32; off > 0; off >>= 1) {
            bits += __shfl_xor(bits, off, 64); ff += __shfl_xor(ff, off, 64); syms += __shfl_xor(syms, off, 64);
            exact += __shfl_xor(exact, off, 64); fail += __shfl_xor(fail, off, 64);
        }
        if (q == 0) {
            ScanStats *t = a.stats;
            const uint64_t last = total_of(a.batch - 1);
            t->out_size = (hard == 0u && last <= a.out_capacity) ? last : 0ull;
            t->total_bits = bits; t->total_ff = ff; t->total_syms = syms; t->total_exact = exact;
            const uint32_t add = st | (fail ? 1u : 0u);
            if (add) atomicOr(&t->status, add);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.out_size[p] = fit ? total : 0ull;
    if (!fit) return;
    uint8_t *dst = a.out[p];
    const uint64_t sy = a.y_size[p], s1 = a.c_size[2 * p], s2 = a.c_size[2 * p + 1];
    if (blockIdx.x == 0) {
        const int k = (int)threadIdx.x;
        if (k < kSosBytes) dst[sy + k] = a.sos[k];
        else if (k >= 16 && k < 16 + kSosBytes) dst[sy + kSosBytes + s1 + (k - 16)] = a.sos[k];
        else if (k == 32 || k == 33) dst[total - 34 + k] = k == 32 ? 0xFF : 0xD9;
    }
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x * 16u;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const uint64_t n = c ? s2 : s1;
        uint8_t *d = dst + sy + kSosBytes + (c ? s1 + kSosBytes : 0u);
        const uint8_t *src = a.scans + (size_t)(2 * p + c) * a.slot_bytes;
        for (uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16u; i < n; i += stride) {
            const uint4 v = *reinterpret_cast<const uint4 *>(src + i);          // (a slot is padded to 16 bytes)
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            const uint64_t m = n - i < 16u ? n - i : 16u;
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if ((uint64_t)k < m) d[i + k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
        }
    }
}

int launch_append_scans_batch(const AppendBatchArgs &a, void *stream, void *const *ev) {
    if (a.batch < 1 || a.batch > kMaxBatch || a.slot_bytes % 16 != 0) return (int)hipErrorInvalidValue;
    const dim3 grid(kAppendBatchWgs, (unsigned)a.batch);
    hipEvent_t e0 = ev ? (hipEvent_t)ev[0] : nullptr, e1 = ev ? (hipEvent_t)ev[1] : nullptr;
    hipExtLaunchKernelGGL(k_append_scans_batch, grid, dim3(256), 0, (hipStream_t)stream, e0, e1, 0, a);
    return (int)hipGetLastError();
}

}  // namespace jpegamd
