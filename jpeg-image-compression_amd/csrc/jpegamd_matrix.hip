// jpegamd_matrix.hip -- the one kernel a BT.709 YCbCr batch (jpegamd_encode_ycbcr_matrix_batch_async) runs in front of the tile encoder.
//
//   k_ycbcr_matrix_batch   every picture of the batch, read once in whatever layout, depth and range it has -> 8-bit full-range BT.601
//                          Y, Cb and Cr planes in context scratch, which the full-range plane launches then code
// The conversion needs all three components at every site, so it is a pass of its own and not a per-sample map of the tile loader.  It
// is bound by memory: the range and depth maps are plain 32-bit integer arithmetic from their definitions (jpeg_compression.h), not
// the loader's packed forms.  No LDS, no inline assembly.
#include <hip/hip_ext.h>
#include "jpegamd_device.h"

namespace jpegamd {

constexpr int kMxOut = 4;                 // chroma samples per thread: one 4-byte store per plane (the pitches are multiples of 4)

// kN dwords from p, of which `valid` (>= 1) bytes belong to the row: one vector load or kN dword loads where p allows and the whole
// run is inside the row; byte loads of the valid bytes alone otherwise (an unaligned plane, an odd stride, the right edge).  Nothing
// outside the row's bytes is read.
template <int kN>
__device__ __forceinline__ void load_run(const uint8_t *p, int valid, uint32_t (&d)[kN]) {
    static_assert(kN == 1 || kN == 2 || kN == 4, "4, 8 or 16 bytes");
    const uintptr_t a = (uintptr_t)p;
    if (valid >= 4 * kN && (a & 3u) == 0) {
        if constexpr (kN == 4) {
            if ((a & 15u) == 0) {
                const uint4 v = *reinterpret_cast<const uint4 *>(p);
                d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
                return;
            }
        }
        if constexpr (kN == 2) {
            if ((a & 7u) == 0) {
                const uint2 v = *reinterpret_cast<const uint2 *>(p);
                d[0] = v.x; d[1] = v.y;
                return;
            }
        }
#pragma unroll
        for (int i = 0; i < kN; ++i) d[i] = reinterpret_cast<const uint32_t *>(p)[i];
    } else {
#pragma unroll
        for (int i = 0; i < kN; ++i) d[i] = 0u;
#pragma unroll
        for (int k = 0; k < 4 * kN; ++k)
            if (k < valid) d[k >> 2] |= (uint32_t)p[k] << (8 * (k & 3));
    }
}

// kCount stored samples of kBytes bytes (16-bit words little-endian) from p -> their raw values; samples past `valid` bytes read as 0.
template <int kCount, int kBytes>
__device__ __forceinline__ void load_samples(const uint8_t *p, int valid, int (&s)[kCount]) {
    constexpr int kN = kCount * kBytes / 4;
    uint32_t d[kN];
    load_run<kN>(p, valid, d);
#pragma unroll
    for (int j = 0; j < kCount; ++j)
        s[j] = kBytes == 1 ? (int)((d[j >> 2] >> (8 * (j & 3))) & 0xFFu) : (int)((d[j >> 1] >> (16 * (j & 1))) & 0xFFFFu);
}

// A stored sample -> the 8-bit full-range sample the existing entries would code (jpeg_compression.h: JPEGAMD_RANGE_*, _SAMPLES_*).
template <int kBytes>
__device__ __forceinline__ int sample8(int w, bool chroma, int shift, bool limited) {
    if (kBytes == 2) {
        const int v = shift ? (w >> shift) : min(w, 1023);
        if (!limited) return min(255, (v + 2) >> 2);
        return chroma ? (255 * (min(max(v, 64), 960) - 64) + 448) / 896 : (255 * (min(max(v, 64), 940) - 64) + 438) / 876;
    }
    if (!limited) return w;
    return chroma ? (255 * (min(max(w, 16), 240) - 16) + 112) / 224 : (255 * (min(max(w, 16), 235) - 16) + 109) / 219;
}

__device__ __forceinline__ int clamp255(int v) { return min(max(v, 0), 255); }

// Thread (gx, cy, p) owns chroma samples 4 gx .. 4 gx + 3 of chroma row cy of picture p, and the kSx x kSy luma samples under each:
// luma (x, y) takes chroma (x / kSx, y / kSy), no interpolation.  Rows are addressed in 64 bits.  kWalk is the memory walk (three
// planes, a Y plane and a pair plane, or one packed 4:2:2 plane), kBytes the bytes per sample; the component order, the alignment shift
// and the range are uniform arguments.  Every store is a dword into the kernel's own pitched scratch; the bytes of a stored dword
// past the plane's width are never coded.
template <int kSx, int kSy, int kWalk, int kBytes>
__global__ __launch_bounds__(256) void k_ycbcr_matrix_batch(const YccMatrixBatchArgs a) {
    static_assert((kSx == 1 || kSx == 2) && (kSy == 1 || kSy == 2) && kSy <= kSx, "4:4:4, 4:2:2 or 4:2:0");
    static_assert(kWalk != kMatrixWalkPacked || (kSx == 2 && kSy == 1 && kBytes == 1), "packed planes are 8-bit 4:2:2");
    constexpr int kLuma = kMxOut * kSx;                                      // luma samples per row and thread
    const int p = (int)blockIdx.z, cy = (int)blockIdx.y, gx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int c0 = kMxOut * gx;
    if (c0 >= a.cw) return;
    const int x0 = c0 * kSx;                                                 // < width: 4 gx < cw = ceil(width / kSx)
    const bool limited = a.limited != 0;
    int cb[kMxOut], cr[kMxOut];                                              // raw samples
    int yraw[kSy][kLuma];
    if constexpr (kWalk == kMatrixWalkPacked) {
        // groups of four bytes, two pixels each: Y0 Cb Y1 Cr (first = 0) or Cb Y0 Cr Y1 (1); the last byte of a row of odd width is
        // the second Y of its last group, which UYVY stores last: not part of the row
        const int row_bytes = 4 * a.cw - ((a.first && (a.width & 1)) ? 1 : 0);
        const uint8_t *row = a.y[p] + (size_t)cy * (size_t)a.y_stride + (size_t)(4 * c0);
        uint32_t d[kMxOut];
        load_run<kMxOut>(row, row_bytes - 4 * c0, d);
        const int yb = a.first ? 8 : 0;
#pragma unroll
        for (int k = 0; k < kMxOut; ++k) {
            yraw[0][2 * k] = (int)((d[k] >> yb) & 0xFFu);
            yraw[0][2 * k + 1] = (int)((d[k] >> (16 + yb)) & 0xFFu);
            cb[k] = (int)((d[k] >> (8 - yb)) & 0xFFu);
            cr[k] = (int)((d[k] >> (24 - yb)) & 0xFFu);
        }
    } else {
        const size_t crow = (size_t)cy * (size_t)a.c_stride;
        if constexpr (kWalk == kMatrixWalkPairs) {
            int pr[2 * kMxOut];
            load_samples<2 * kMxOut, kBytes>(a.cb[p] + crow + (size_t)(2 * kBytes * c0), 2 * kBytes * (a.cw - c0), pr);
#pragma unroll
            for (int k = 0; k < kMxOut; ++k) {
                cb[k] = a.first ? pr[2 * k + 1] : pr[2 * k];
                cr[k] = a.first ? pr[2 * k] : pr[2 * k + 1];
            }
        } else {
            load_samples<kMxOut, kBytes>(a.cb[p] + crow + (size_t)(kBytes * c0), kBytes * (a.cw - c0), cb);
            load_samples<kMxOut, kBytes>(a.cr[p] + crow + (size_t)(kBytes * c0), kBytes * (a.cw - c0), cr);
        }
#pragma unroll
        for (int r = 0; r < kSy; ++r) {
            const int y = min(cy * kSy + r, a.height - 1);                  // (an odd height: the second row is not stored below)
            load_samples<kLuma, kBytes>(a.y[p] + (size_t)y * (size_t)a.y_stride + (size_t)(kBytes * x0), kBytes * (a.width - x0), yraw[r]);
        }
    }
    // the three matrix terms of every chroma sample; the chroma planes' dwords
    int ty[kMxOut];
    uint32_t wcb = 0, wcr = 0;
#pragma unroll
    for (int k = 0; k < kMxOut; ++k) {
        const int b = sample8<kBytes>(cb[k], true, a.shift, limited) - 128, r = sample8<kBytes>(cr[k], true, a.shift, limited) - 128;
        ty[k] = (kMatrix709[0] * b + kMatrix709[1] * r + (1 << (kMatrixShift - 1))) >> kMatrixShift;
        const int nb = clamp255(128 + ((kMatrix709[2] * b + kMatrix709[3] * r + (1 << (kMatrixShift - 1))) >> kMatrixShift));
        const int nr = clamp255(128 + ((kMatrix709[4] * b + kMatrix709[5] * r + (1 << (kMatrixShift - 1))) >> kMatrixShift));
        wcb |= (uint32_t)nb << (8 * k);
        wcr |= (uint32_t)nr << (8 * k);
    }
    uint8_t *cbp = a.planes + (size_t)(2 * p) * a.plane_bytes;
    const size_t oc = (size_t)cy * (size_t)a.pitch + (size_t)c0;            // c0 % 4 == 0, c0 < cw <= pitch (a multiple of 4)
    *reinterpret_cast<uint32_t *>(cbp + oc) = wcb;
    *reinterpret_cast<uint32_t *>(cbp + a.plane_bytes + oc) = wcr;
    uint8_t *yp = a.yplanes + (size_t)p * a.yplane_bytes;
#pragma unroll
    for (int r = 0; r < kSy; ++r) {
        const int y = cy * kSy + r;
        if (y >= a.height) break;
#pragma unroll
        for (int i = 0; i < kSx; ++i) {
            uint32_t wy = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int j = 4 * i + k;                                     // the luma sample; its chroma sample is j / kSx
                wy |= (uint32_t)clamp255(sample8<kBytes>(yraw[r][j], false, a.shift, limited) + ty[j / kSx]) << (8 * k);
            }
            // x0 + 4 i is a multiple of 4 below the width, so the dword lies inside the row's ypitch bytes
            if (x0 + 4 * i < a.width) *reinterpret_cast<uint32_t *>(yp + (size_t)y * (size_t)a.ypitch + (size_t)(x0 + 4 * i)) = wy;
        }
    }
}

template <int kWalk, int kBytes>
static void launch_matrix_as(const YccMatrixBatchArgs &a, dim3 grid, dim3 block, hipStream_t stream, hipEvent_t e0, hipEvent_t e1) {
    if (a.mode == kChromaMode420) hipExtLaunchKernelGGL((k_ycbcr_matrix_batch<2, 2, kWalk, kBytes>), grid, block, 0, stream, e0, e1, 0, a);
    else if (a.mode == kChromaMode422) hipExtLaunchKernelGGL((k_ycbcr_matrix_batch<2, 1, kWalk, kBytes>), grid, block, 0, stream, e0, e1, 0, a);
    else hipExtLaunchKernelGGL((k_ycbcr_matrix_batch<1, 1, kWalk, kBytes>), grid, block, 0, stream, e0, e1, 0, a);
}

int launch_ycbcr_matrix_batch(const YccMatrixBatchArgs &a, void *stream, void *const *ev) {
    const int sx = a.mode == kChromaMode444 ? 1 : 2, sy = a.mode == kChromaMode420 ? 2 : 1;
    if ((a.mode != kChromaMode444 && a.mode != kChromaMode420 && a.mode != kChromaMode422) || a.batch < 1 || a.batch > kMaxBatch ||
        a.width <= 0 || a.height <= 0 || a.cw != (a.width + sx - 1) / sx || a.ch != (a.height + sy - 1) / sy || a.ch > 65535 ||
        a.pitch % 4 != 0 || a.pitch < (a.cw + 3) / 4 * 4 || a.ypitch % 4 != 0 || a.ypitch < (a.width + 3) / 4 * 4 ||
        a.plane_bytes % 16 != 0 || a.plane_bytes < (uint64_t)a.pitch * (uint64_t)a.ch ||
        a.yplane_bytes % 16 != 0 || a.yplane_bytes < (uint64_t)a.ypitch * (uint64_t)a.height ||
        (a.sample_bytes != 1 && a.sample_bytes != 2) || (a.first != 0 && a.first != 1) || !a.planes || !a.yplanes)
        return (int)hipErrorInvalidValue;
    const int threads_x = (a.cw + kMxOut - 1) / kMxOut;
    const dim3 grid((unsigned)((threads_x + 255) / 256), (unsigned)a.ch, (unsigned)a.batch), block(256);
    hipEvent_t e0 = ev ? (hipEvent_t)ev[0] : nullptr, e1 = ev ? (hipEvent_t)ev[1] : nullptr;
    hipStream_t s = (hipStream_t)stream;
    if (a.walk == kMatrixWalkPacked) {
        if (a.mode != kChromaMode422 || a.sample_bytes != 1) return (int)hipErrorInvalidValue;
        hipExtLaunchKernelGGL((k_ycbcr_matrix_batch<2, 1, kMatrixWalkPacked, 1>), grid, block, 0, s, e0, e1, 0, a);
    } else if (a.walk == kMatrixWalkPairs) {
        if (a.sample_bytes == 1) launch_matrix_as<kMatrixWalkPairs, 1>(a, grid, block, s, e0, e1);
        else launch_matrix_as<kMatrixWalkPairs, 2>(a, grid, block, s, e0, e1);
    } else if (a.walk == kMatrixWalkPlanes) {
        if (a.sample_bytes == 1) launch_matrix_as<kMatrixWalkPlanes, 1>(a, grid, block, s, e0, e1);
        else launch_matrix_as<kMatrixWalkPlanes, 2>(a, grid, block, s, e0, e1);
    } else {
        return (int)hipErrorInvalidValue;
    }
    return (int)hipGetLastError();
}

}  // namespace jpegamd
