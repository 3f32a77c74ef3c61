// jpegamd_reduce.hip -- the one kernel a batch of reduced pictures (jpegamd_encode_reduced_batch_async and its twins) runs in front of
// the tile encoder.
//
//   k_reduce_planes_batch  every picture of the batch, the bytes of its source read once where they lie -> the mean of every
//                          factor x factor box (jpeg_compression.h, "Reduced pictures": (S + (n >> 1)) / n over the n samples inside
//                          the picture), then the header's RGB -> YCbCr map and chroma subsampling -> 8-bit Y, Cb and Cr planes of
//                          the REDUCED picture in context scratch, laid out as k_float_planes_batch lays them out
// Bound by reading the source; no LDS, no inline assembly.  A thread owns whole boxes (DESIGN.md 4.6.19 has what that costs).
#include <hip/hip_ext.h>
#include "jpegamd_device.h"

namespace jpegamd {

constexpr int kRdOut = 4;                 // chroma samples per thread: one 4-byte store per plane (the pitches are multiples of 4)

// ceil(2^22 / n) for every box size (reduce_recip, jpegamd_internal.h)
struct ReduceRecip { uint32_t m[kMaxReduce * kMaxReduce + 1]; };
constexpr ReduceRecip make_reduce_recip() {
    ReduceRecip t{};
    for (int n = 1; n <= kMaxReduce * kMaxReduce; ++n) t.m[n] = reduce_recip(n);
    return t;
}
__constant__ const ReduceRecip kReduceRecip = make_reduce_recip();

// (S + (n >> 1)) / n, exactly
__device__ __forceinline__ int box_mean(uint32_t sum, int n) {
    return (int)(((sum + (uint32_t)(n >> 1)) * kReduceRecip.m[n]) >> kReduceShift);
}

// The boxes of one source row by bytes: box j of the thread begins at sample sx0 + j f and has the samples of it below src_width (none
// past the row's end); samples lie `stride` bytes apart from q, the channel's first sample of the row.  Any pointer, any stride.
template <int kPix>
__device__ __forceinline__ void byte_sums(const uint8_t *q, size_t stride, int sx0, int f, int src_width, uint32_t *s) {
#pragma unroll
    for (int j = 0; j < kPix; ++j) {
        const int xb = sx0 + j * f;
        const int nx = min(f, src_width - xb);                               // <= 0: the box lies past the row's end
        for (int k = 0; k < nx; ++k) s[j] += q[(size_t)(xb + k) * stride];
    }
}

// The bytes of dword i of a thread's run that belong to channel c of box j, as a byte mask: kGroup bytes per pixel, kF pixels per box.
template <int kGroup, int kF>
__device__ constexpr uint32_t run_mask(int i, int c, int j) {
    uint32_t m = 0;
    for (int b = 0; b < 4; ++b) {
        const int pos = 4 * i + b;
        if (pos % kGroup == c && pos / (kGroup * kF) == j) m |= 0xFFu << (8 * b);
    }
    return m;
}

// A thread's run of one source row where it is contiguous -- kPix boxes of kF pixels of kGroup bytes from q, ALL inside the row (the
// caller has checked) -- in 16-byte (or 8-byte) loads where q allows, in dwords where it is a multiple of 4; box sums by v_sad_u8 against
// zero under the byte masks, s[c * kPix + j] for channel c of box j.  false: q is no multiple of 4 and nothing was read.
template <int kGroup, int kF, int kPix>
__device__ __forceinline__ bool contig_sums(const uint8_t *q, uint32_t *s) {
    constexpr int kBox = kGroup * kF, kRun = kBox * kPix;                    // 4 .. 192 bytes; kPix is 4 or 8, so whole dwords
    constexpr int kVec = kRun % 16 == 0 ? 16 : (kRun % 8 == 0 ? 8 : 4);
    static_assert(kRun % 4 == 0, "whole dwords");
    uint32_t d[kRun / 4];
    const uintptr_t addr = (uintptr_t)q;
    if (kVec == 16 && (addr & 15) == 0) {
#pragma unroll
        for (int i = 0; i < kRun / 16; ++i) {
            const uint4 v = reinterpret_cast<const uint4 *>(q)[i];
            d[4 * i] = v.x; d[4 * i + 1] = v.y; d[4 * i + 2] = v.z; d[4 * i + 3] = v.w;
        }
    } else if (kVec >= 8 && (addr & 7) == 0) {
#pragma unroll
        for (int i = 0; i < kRun / 8; ++i) {
            const uint2 v = reinterpret_cast<const uint2 *>(q)[i];
            d[2 * i] = v.x; d[2 * i + 1] = v.y;
        }
    } else if ((addr & 3) == 0) {
#pragma unroll
        for (int i = 0; i < kRun / 4; ++i) d[i] = reinterpret_cast<const uint32_t *>(q)[i];
    } else {
        return false;
    }
#pragma unroll
    for (int j = 0; j < kPix; ++j) {
#pragma unroll
        for (int i = j * kBox / 4; i <= ((j + 1) * kBox - 1) / 4; ++i) {
#pragma unroll
            for (int c = 0; c < kGroup; ++c) {
                const uint32_t m = run_mask<kGroup, kF>(i, c, j);
                if (m) s[c * kPix + j] = __builtin_amdgcn_sad_u8(d[i] & m, 0u, s[c * kPix + j]);
            }
        }
    }
    return true;
}

// Thread (gx, cy, p) owns chroma samples 4 gx .. 4 gx + 3 of chroma row cy of reduced picture p, the kSx x kSy reduced pixels under
// each and the f x f source box under each of those, as k_float_planes_batch's threads own pixels; rows are addressed in 64 bits.
// kWalk is the memory walk the host chose from the pointers and strides; kF the factor where the walk is contiguous (1, 2, 4, 8), or
// 0: a.factor, byte by byte (kReduceWalkGeneric: every other factor, every other stride).  kOut is what is written: Y, Cb and Cr
// planes; the Y plane alone of three channels; or the single channel's means as the Y plane (the last two at kSx = kSy = 1).  Box sums
// accumulate over the f rows in registers; nothing outside a row's own pixel_stride x src_width bytes is read.  Every store is a dword
// into the kernel's own pitched scratch; the bytes of a stored dword past the plane's width are never coded.
template <int kSx, int kSy, int kWalk, int kF, int kOut>
__global__ __launch_bounds__(256) void k_reduce_planes_batch(const ReducePlanesBatchArgs a) {
    static_assert((kSx == 1 || kSx == 2) && (kSy == 1 || kSy == 2) && kSy <= kSx, "4:4:4, 4:2:2 or 4:2:0");
    static_assert(kOut == kReduceOutColor || (kSx == 1 && kSy == 1), "a Y plane alone has no chroma grid");
    static_assert(kOut != kReduceOutSingle || kWalk != kReduceWalkPacked3, "one channel is not packed in threes");
    static_assert((kWalk == kReduceWalkGeneric) == (kF == 0), "the generic walk takes its factor at run time, the others by template");
    constexpr int kC = kOut == kReduceOutSingle ? 1 : 3;                     // channels read
    constexpr int kPix = kRdOut * kSx;                                       // reduced pixels per row and thread
    const int p = (int)blockIdx.z, cy = (int)blockIdx.y, gx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int c0 = kRdOut * gx;
    if (c0 >= a.cw) return;
    const int f = kF ? kF : a.factor;
    const int x0 = c0 * kSx;                                                 // < width: 4 gx < cw = ceil(width / kSx)
    const int npx = min(kPix, a.width - x0);                                 // the thread's reduced pixels inside the row (>= 1)
    const int sx0 = x0 * f;                                                  // its first source column (< src_width)
    const bool whole = sx0 + kPix * f <= a.src_width;                        // its whole run lies inside the source row
    int cb[kSy][kPix], cr[kSy][kPix];
    uint8_t *yp = a.yplanes + (size_t)p * a.yplane_bytes;
#pragma unroll
    for (int r = 0; r < kSy; ++r) {
        const int y = min(cy * kSy + r, a.height - 1);                      // the last row replicated (an odd height: not stored below)
        const int sy0 = y * f;                                               // < src_height
        const int ny = min(f, a.src_height - sy0);                           // the box rows inside the picture (>= 1)
        uint32_t s[kC * kPix];
#pragma unroll
        for (int i = 0; i < kC * kPix; ++i) s[i] = 0;
        for (int yy = 0; yy < ny; ++yy) {
            const size_t row = (size_t)(sy0 + yy) * (size_t)a.row_stride;
            if constexpr (kWalk == kReduceWalkPacked3) {
                // the three channels of a pixel side by side from the lowest of the three pointers (a.reversed: B G R, swapped below)
                const uint8_t *q = a.plane[0][p] + row;
                if (!(whole && contig_sums<3, kF, kPix>(q + (size_t)sx0 * 3, s))) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) byte_sums<kPix>(q + c, 3, sx0, f, a.src_width, s + c * kPix);
                }
            } else if constexpr (kWalk == kReduceWalkPlanar) {
#pragma unroll
                for (int c = 0; c < kC; ++c) {
                    const uint8_t *q = a.plane[c][p] + row;
                    if (!(whole && contig_sums<1, kF, kPix>(q + sx0, s + c * kPix))) byte_sums<kPix>(q, 1, sx0, f, a.src_width, s + c * kPix);
                }
            } else {
#pragma unroll
                for (int c = 0; c < kC; ++c) byte_sums<kPix>(a.plane[c][p] + row, (size_t)a.pixel_stride, sx0, f, a.src_width, s + c * kPix);
            }
        }
        // the means; a reduced pixel past the row's end holds the row's last one
        int v[kC][kPix];
#pragma unroll
        for (int j = 0; j < kPix; ++j) {
            if (j == 0 || j < npx) {
                const int n = min(f, a.src_width - (sx0 + j * f)) * ny;      // 1 .. f^2: j < npx, so the box begins inside the row
#pragma unroll
                for (int c = 0; c < kC; ++c) v[c][j] = box_mean(s[c * kPix + j], n);
            } else {
#pragma unroll
                for (int c = 0; c < kC; ++c) v[c][j] = v[c][j - 1];
            }
        }
        if constexpr (kWalk == kReduceWalkPacked3) {
            if (a.reversed) {
#pragma unroll
                for (int j = 0; j < kPix; ++j) { const int t = v[0][j]; v[0][j] = v[2][j]; v[2][j] = t; }
            }
        }
        const bool stored = cy * kSy + r < a.height;
#pragma unroll
        for (int i = 0; i < kSx; ++i) {
            uint32_t wy = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int j = 4 * i + k;
                int luma;
                if constexpr (kOut == kReduceOutSingle) luma = v[0][j];
                else luma = (77 * v[0][j] + 150 * v[1][j] + 29 * v[2][j]) >> 8;
                wy |= (uint32_t)luma << (8 * k);
            }
            // x0 + 4 i is a multiple of 4 below the width, so the dword lies inside the row's ypitch bytes
            if (stored && x0 + 4 * i < a.width) *reinterpret_cast<uint32_t *>(yp + (size_t)y * (size_t)a.ypitch + (size_t)(x0 + 4 * i)) = wy;
        }
        if constexpr (kOut == kReduceOutColor) {
            // Cb = (32768 - 43 R - 85 G + 128 B) >> 8, Cr = (32768 + 128 R - 107 G - 21 B) >> 8, per reduced pixel (k_chroma_planes' cbcr)
#pragma unroll
            for (int j = 0; j < kPix; ++j) {
                cb[r][j] = (32768 - 43 * v[0][j] - 85 * v[1][j] + 128 * v[2][j]) >> 8;
                cr[r][j] = (32768 + 128 * v[0][j] - 107 * v[1][j] - 21 * v[2][j]) >> 8;
            }
        }
    }
    if constexpr (kOut == kReduceOutColor) {
        uint32_t wcb = 0, wcr = 0;
#pragma unroll
        for (int k = 0; k < kRdOut; ++k) {
            int vb, vr;
            if constexpr (kSx == 2) {
                // (a pixel past the row's end holds the last column already): (a + b + c + d + 2) >> 2, or (a + b + 1) >> 1
                const int j0 = 2 * k, j1 = 2 * k + 1;
                if constexpr (kSy == 2) {
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
        const size_t oc = (size_t)cy * (size_t)a.pitch + (size_t)c0;        // c0 % 4 == 0, c0 < cw <= pitch (a multiple of 4)
        *reinterpret_cast<uint32_t *>(cbp + oc) = wcb;
        *reinterpret_cast<uint32_t *>(cbp + a.plane_bytes + oc) = wcr;
    }
}

template <int kWalk, int kF>
static void launch_reduce_as(const ReducePlanesBatchArgs &a, dim3 grid, dim3 block, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    if (a.out == kReduceOutColor) {
        if (a.mode == kChromaMode420) hipExtLaunchKernelGGL((k_reduce_planes_batch<2, 2, kWalk, kF, kReduceOutColor>), grid, block, 0, s, e0, e1, 0, a);
        else if (a.mode == kChromaMode422) hipExtLaunchKernelGGL((k_reduce_planes_batch<2, 1, kWalk, kF, kReduceOutColor>), grid, block, 0, s, e0, e1, 0, a);
        else hipExtLaunchKernelGGL((k_reduce_planes_batch<1, 1, kWalk, kF, kReduceOutColor>), grid, block, 0, s, e0, e1, 0, a);
    } else if (a.out == kReduceOutLuma) {
        hipExtLaunchKernelGGL((k_reduce_planes_batch<1, 1, kWalk, kF, kReduceOutLuma>), grid, block, 0, s, e0, e1, 0, a);
    } else if constexpr (kWalk != kReduceWalkPacked3) {
        hipExtLaunchKernelGGL((k_reduce_planes_batch<1, 1, kWalk, kF, kReduceOutSingle>), grid, block, 0, s, e0, e1, 0, a);
    }
}

template <int kWalk>
static void launch_reduce_walk(const ReducePlanesBatchArgs &a, dim3 grid, dim3 block, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    if (a.factor == 1) launch_reduce_as<kWalk, 1>(a, grid, block, s, e0, e1);
    else if (a.factor == 2) launch_reduce_as<kWalk, 2>(a, grid, block, s, e0, e1);
    else if (a.factor == 4) launch_reduce_as<kWalk, 4>(a, grid, block, s, e0, e1);
    else launch_reduce_as<kWalk, 8>(a, grid, block, s, e0, e1);
}

int launch_reduce_planes_batch(const ReducePlanesBatchArgs &a, void *stream, void *const *ev) {
    const bool color = a.out == kReduceOutColor;
    const int sx = color && a.mode != kChromaMode444 ? 2 : 1, sy = color && a.mode == kChromaMode420 ? 2 : 1;
    const bool pow2 = a.factor == 1 || a.factor == 2 || a.factor == 4 || a.factor == 8;
    if ((a.out != kReduceOutColor && a.out != kReduceOutLuma && a.out != kReduceOutSingle) ||
        (color && a.mode != kChromaMode444 && a.mode != kChromaMode420 && a.mode != kChromaMode422) ||
        (a.walk != kReduceWalkPlanar && a.walk != kReduceWalkPacked3 && a.walk != kReduceWalkGeneric) ||
        (a.walk == kReduceWalkPacked3 && a.out == kReduceOutSingle) || a.batch < 1 || a.batch > kMaxBatch ||
        a.factor < 1 || a.factor > kMaxReduce || (a.walk != kReduceWalkGeneric && !pow2) ||
        a.src_width <= 0 || a.src_height <= 0 || a.src_width > 65535 || a.src_height > 65535 ||
        a.width != (a.src_width + a.factor - 1) / a.factor || a.height != (a.src_height + a.factor - 1) / a.factor ||
        a.cw != (a.width + sx - 1) / sx || a.ch != (a.height + sy - 1) / sy ||
        a.pixel_stride < 1 || (int64_t)a.row_stride < (int64_t)a.pixel_stride * a.src_width ||
        (a.walk == kReduceWalkPlanar && a.pixel_stride != 1) || (a.walk == kReduceWalkPacked3 && a.pixel_stride != 3) ||
        a.ypitch % 4 != 0 || a.ypitch < (a.width + 3) / 4 * 4 || a.yplane_bytes % 16 != 0 ||
        a.yplane_bytes < (uint64_t)a.ypitch * (uint64_t)a.height || !a.yplanes ||
        (color && (a.pitch % 4 != 0 || a.pitch < (a.cw + 3) / 4 * 4 || a.plane_bytes % 16 != 0 ||
                   a.plane_bytes < (uint64_t)a.pitch * (uint64_t)a.ch || !a.planes)))
        return (int)hipErrorInvalidValue;
    const int threads_x = (a.cw + kRdOut - 1) / kRdOut;
    const dim3 grid((unsigned)((threads_x + 255) / 256), (unsigned)a.ch, (unsigned)a.batch), block(256);
    hipEvent_t e0 = ev ? (hipEvent_t)ev[0] : nullptr, e1 = ev ? (hipEvent_t)ev[1] : nullptr;
    hipStream_t s = (hipStream_t)stream;
    if (a.walk == kReduceWalkPlanar) launch_reduce_walk<kReduceWalkPlanar>(a, grid, block, s, e0, e1);
    else if (a.walk == kReduceWalkPacked3) launch_reduce_walk<kReduceWalkPacked3>(a, grid, block, s, e0, e1);
    else launch_reduce_as<kReduceWalkGeneric, 0>(a, grid, block, s, e0, e1);
    return (int)hipGetLastError();
}

}  // namespace jpegamd
