// jpegamd_float.hip -- the one kernel a batch of float pictures (jpegamd_encode_float_batch_async and its twins) runs in front of
// the tile encoder.
//
//   k_float_planes_batch   every picture of the batch, f32 / f16 / bf16 samples read once where they lie -> the byte of each sample
//                          (jpeg_compression.h, "Float pictures": one multiply, one add, round half to even, clamp), then the header's
//                          RGB -> YCbCr map and chroma subsampling -> 8-bit Y, Cb and Cr planes in context scratch, laid out as
//                          k_ycbcr_matrix_batch lays them out, which the full-range plane launches then code
// Bound by memory for f32 input; no LDS, no inline assembly.
#include <hip/hip_ext.h>
#include <hip/hip_fp16.h>
#include "jpegamd_device.h"

namespace jpegamd {

constexpr int kFpOut = 4;                 // chroma samples per thread: one 4-byte store per plane (the pitches are multiples of 4)

// The stored bits of a sample -> float32, exactly: bf16 is the high half of a float32; f16 converts in hardware, subnormals included.
template <int kType>
__device__ __forceinline__ float sample_f32(uint32_t bits) {
    if constexpr (kType == kFloatF32) return __uint_as_float(bits);
    else if constexpr (kType == kFloatBF16) return __uint_as_float(bits << 16);
    else return __half2float(__ushort_as_half((unsigned short)bits));
}

// The byte of a sample: the product and the sum are rounded to float32 one after the other (never fused, whatever the build's
// contraction flag says), NaN -> 0, round half to even, clamp (+inf -> 255, -inf -> 0).
__device__ __forceinline__ int float_byte(float x, float scale, float offset) {
#pragma clang fp contract(off)
    const float p = __fmul_rn(x, scale);
    const float t = __fadd_rn(p, offset);
    return t != t ? 0 : (int)fminf(fmaxf(rintf(t), 0.0f), 255.0f);
}

// One stored sample of kB bytes at q, which the host has checked to be a multiple of kB.
template <int kB>
__device__ __forceinline__ uint32_t load_elem(const uint8_t *q) {
    if constexpr (kB == 4) return *reinterpret_cast<const uint32_t *>(q);
    else return (uint32_t)*reinterpret_cast<const uint16_t *>(q);
}

// kCount contiguous samples of kB bytes from q -- kGroup samples per pixel, `npx` (>= 1) pixels of them inside the row -> their bits;
// a pixel past the row's end reads as the row's last one.  The whole run in 16-byte (a run of 8 or 24 bytes: 8-byte) loads where q
// allows and every pixel is inside the row; loads of the row's own samples alone otherwise (an unaligned base or stride, the right
// edge).  Nothing outside the row's bytes is read.
template <int kB, int kCount, int kGroup>
__device__ __forceinline__ void load_contig(const uint8_t *q, int npx, uint32_t (&e)[kCount]) {
    constexpr int kRun = kB * kCount;                                        // 8, 16, 24, 32, 48 or 96 bytes
    constexpr int kVec = kRun % 16 == 0 ? 16 : 8;
    static_assert(kRun % kVec == 0 && kCount % kGroup == 0, "whole vectors, whole pixels");
    if (npx * kGroup == kCount && ((uintptr_t)q & (uintptr_t)(kVec - 1)) == 0) {
        uint32_t d[kRun / 4];
        if constexpr (kVec == 16) {
#pragma unroll
            for (int i = 0; i < kRun / 16; ++i) {
                const uint4 v = reinterpret_cast<const uint4 *>(q)[i];
                d[4 * i] = v.x; d[4 * i + 1] = v.y; d[4 * i + 2] = v.z; d[4 * i + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < kRun / 8; ++i) {
                const uint2 v = reinterpret_cast<const uint2 *>(q)[i];
                d[2 * i] = v.x; d[2 * i + 1] = v.y;
            }
        }
#pragma unroll
        for (int j = 0; j < kCount; ++j) e[j] = kB == 4 ? d[j] : (d[j >> 1] >> (16 * (j & 1))) & 0xFFFFu;
    } else {
#pragma unroll
        for (int j = 0; j < kCount; ++j) {
            const int px = min(j / kGroup, npx - 1);                         // < npx: inside the row
            e[j] = load_elem<kB>(q + (size_t)(px * kGroup + j % kGroup) * kB);
        }
    }
}

// Thread (gx, cy, p) owns chroma samples 4 gx .. 4 gx + 3 of chroma row cy of picture p and the kSx x kSy pixels under each, as in
// k_ycbcr_matrix_batch; rows are addressed in 64 bits.  kWalk is the memory walk the host chose from the pointers and strides, kType
// the sample type, kOut what is written: Y, Cb and Cr planes; the Y plane alone of three channels; or the single channel's bytes as
// the Y plane (the last two at kSx = kSy = 1).  Every store is a dword into the kernel's own pitched scratch; the bytes of a stored
// dword past the plane's width are never coded.
template <int kSx, int kSy, int kWalk, int kType, int kOut>
__global__ __launch_bounds__(256) void k_float_planes_batch(const FloatPlanesBatchArgs a) {
    static_assert((kSx == 1 || kSx == 2) && (kSy == 1 || kSy == 2) && kSy <= kSx, "4:4:4, 4:2:2 or 4:2:0");
    static_assert(kOut == kFloatOutColor || (kSx == 1 && kSy == 1), "a Y plane alone has no chroma grid");
    static_assert(kOut != kFloatOutSingle || kWalk != kFloatWalkPacked3, "one channel is not packed in threes");
    constexpr int kB = kType == kFloatF32 ? 4 : 2;                           // bytes per sample
    constexpr int kC = kOut == kFloatOutSingle ? 1 : 3;                      // channels read
    constexpr int kPix = kFpOut * kSx;                                       // pixels per row and thread
    const int p = (int)blockIdx.z, cy = (int)blockIdx.y, gx = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int c0 = kFpOut * gx;
    if (c0 >= a.cw) return;
    const int x0 = c0 * kSx;                                                 // < width: 4 gx < cw = ceil(width / kSx)
    const int npx = min(kPix, a.width - x0);                                 // the thread's pixels inside the row (>= 1)
    int cb[kSy][kPix], cr[kSy][kPix];
    uint8_t *yp = a.yplanes + (size_t)p * a.yplane_bytes;
#pragma unroll
    for (int r = 0; r < kSy; ++r) {
        const int y = min(cy * kSy + r, a.height - 1);                      // the last row replicated (an odd height: not stored below)
        const size_t row = (size_t)y * (size_t)a.row_stride;
        uint32_t e[kC][kPix];
        if constexpr (kWalk == kFloatWalkPacked3) {
            // the three channels of a pixel side by side from the lowest of the three pointers; a.reversed: B G R
            uint32_t t[3 * kPix];
            load_contig<kB, 3 * kPix, 3>(a.plane[0][p] + row + (size_t)x0 * (3 * kB), npx, t);
#pragma unroll
            for (int j = 0; j < kPix; ++j) {
                e[0][j] = a.reversed ? t[3 * j + 2] : t[3 * j];
                e[1][j] = t[3 * j + 1];
                e[2][j] = a.reversed ? t[3 * j] : t[3 * j + 2];
            }
        } else if constexpr (kWalk == kFloatWalkPlanar) {
#pragma unroll
            for (int c = 0; c < kC; ++c) load_contig<kB, kPix, 1>(a.plane[c][p] + row + (size_t)x0 * kB, npx, e[c]);
        } else {
#pragma unroll
            for (int c = 0; c < kC; ++c) {
                const uint8_t *q = a.plane[c][p] + row;
#pragma unroll
                for (int j = 0; j < kPix; ++j) e[c][j] = load_elem<kB>(q + (size_t)(x0 + min(j, npx - 1)) * (size_t)a.pixel_stride);
            }
        }
        int v[kC][kPix];
#pragma unroll
        for (int c = 0; c < kC; ++c)
#pragma unroll
            for (int j = 0; j < kPix; ++j) v[c][j] = float_byte(sample_f32<kType>(e[c][j]), a.scale, a.offset);
        const bool stored = cy * kSy + r < a.height;
#pragma unroll
        for (int i = 0; i < kSx; ++i) {
            uint32_t wy = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int j = 4 * i + k;
                int luma;
                if constexpr (kOut == kFloatOutSingle) luma = v[0][j];
                else luma = (77 * v[0][j] + 150 * v[1][j] + 29 * v[2][j]) >> 8;
                wy |= (uint32_t)luma << (8 * k);
            }
            // x0 + 4 i is a multiple of 4 below the width, so the dword lies inside the row's ypitch bytes
            if (stored && x0 + 4 * i < a.width) *reinterpret_cast<uint32_t *>(yp + (size_t)y * (size_t)a.ypitch + (size_t)(x0 + 4 * i)) = wy;
        }
        if constexpr (kOut == kFloatOutColor) {
            // Cb = (32768 - 43 R - 85 G + 128 B) >> 8, Cr = (32768 + 128 R - 107 G - 21 B) >> 8, per pixel (k_chroma_planes' cbcr)
#pragma unroll
            for (int j = 0; j < kPix; ++j) {
                cb[r][j] = (32768 - 43 * v[0][j] - 85 * v[1][j] + 128 * v[2][j]) >> 8;
                cr[r][j] = (32768 + 128 * v[0][j] - 107 * v[1][j] - 21 * v[2][j]) >> 8;
            }
        }
    }
    if constexpr (kOut == kFloatOutColor) {
        uint32_t wcb = 0, wcr = 0;
#pragma unroll
        for (int k = 0; k < kFpOut; ++k) {
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

template <int kWalk, int kType>
static void launch_float_as(const FloatPlanesBatchArgs &a, dim3 grid, dim3 block, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    if (a.out == kFloatOutColor) {
        if (a.mode == kChromaMode420) hipExtLaunchKernelGGL((k_float_planes_batch<2, 2, kWalk, kType, kFloatOutColor>), grid, block, 0, s, e0, e1, 0, a);
        else if (a.mode == kChromaMode422) hipExtLaunchKernelGGL((k_float_planes_batch<2, 1, kWalk, kType, kFloatOutColor>), grid, block, 0, s, e0, e1, 0, a);
        else hipExtLaunchKernelGGL((k_float_planes_batch<1, 1, kWalk, kType, kFloatOutColor>), grid, block, 0, s, e0, e1, 0, a);
    } else if (a.out == kFloatOutLuma) {
        hipExtLaunchKernelGGL((k_float_planes_batch<1, 1, kWalk, kType, kFloatOutLuma>), grid, block, 0, s, e0, e1, 0, a);
    } else if constexpr (kWalk != kFloatWalkPacked3) {
        hipExtLaunchKernelGGL((k_float_planes_batch<1, 1, kWalk, kType, kFloatOutSingle>), grid, block, 0, s, e0, e1, 0, a);
    }
}

template <int kWalk>
static void launch_float_walk(const FloatPlanesBatchArgs &a, dim3 grid, dim3 block, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    if (a.type == kFloatF32) launch_float_as<kWalk, kFloatF32>(a, grid, block, s, e0, e1);
    else if (a.type == kFloatF16) launch_float_as<kWalk, kFloatF16>(a, grid, block, s, e0, e1);
    else launch_float_as<kWalk, kFloatBF16>(a, grid, block, s, e0, e1);
}

int launch_float_planes_batch(const FloatPlanesBatchArgs &a, void *stream, void *const *ev) {
    const bool color = a.out == kFloatOutColor;
    const int sx = color && a.mode != kChromaMode444 ? 2 : 1, sy = color && a.mode == kChromaMode420 ? 2 : 1;
    const int kb = a.type == kFloatF32 ? 4 : 2;
    if ((a.out != kFloatOutColor && a.out != kFloatOutLuma && a.out != kFloatOutSingle) ||
        (color && a.mode != kChromaMode444 && a.mode != kChromaMode420 && a.mode != kChromaMode422) ||
        (a.type != kFloatF32 && a.type != kFloatF16 && a.type != kFloatBF16) ||
        (a.walk != kFloatWalkPlanar && a.walk != kFloatWalkPacked3 && a.walk != kFloatWalkGeneric) ||
        (a.walk == kFloatWalkPacked3 && a.out == kFloatOutSingle) || a.batch < 1 || a.batch > kMaxBatch ||
        a.width <= 0 || a.height <= 0 || a.cw != (a.width + sx - 1) / sx || a.ch != (a.height + sy - 1) / sy || a.ch > 65535 ||
        a.pixel_stride < kb || a.pixel_stride % kb != 0 || a.row_stride % kb != 0 || (int64_t)a.row_stride < (int64_t)a.pixel_stride * a.width ||
        (a.walk == kFloatWalkPlanar && a.pixel_stride != kb) || (a.walk == kFloatWalkPacked3 && a.pixel_stride != 3 * kb) ||
        a.ypitch % 4 != 0 || a.ypitch < (a.width + 3) / 4 * 4 || a.yplane_bytes % 16 != 0 ||
        a.yplane_bytes < (uint64_t)a.ypitch * (uint64_t)a.height || !a.yplanes ||
        (color && (a.pitch % 4 != 0 || a.pitch < (a.cw + 3) / 4 * 4 || a.plane_bytes % 16 != 0 ||
                   a.plane_bytes < (uint64_t)a.pitch * (uint64_t)a.ch || !a.planes)))
        return (int)hipErrorInvalidValue;
    const int threads_x = (a.cw + kFpOut - 1) / kFpOut;
    const dim3 grid((unsigned)((threads_x + 255) / 256), (unsigned)a.ch, (unsigned)a.batch), block(256);
    hipEvent_t e0 = ev ? (hipEvent_t)ev[0] : nullptr, e1 = ev ? (hipEvent_t)ev[1] : nullptr;
    hipStream_t s = (hipStream_t)stream;
    if (a.walk == kFloatWalkPlanar) launch_float_walk<kFloatWalkPlanar>(a, grid, block, s, e0, e1);
    else if (a.walk == kFloatWalkPacked3) launch_float_walk<kFloatWalkPacked3>(a, grid, block, s, e0, e1);
    else launch_float_walk<kFloatWalkGeneric>(a, grid, block, s, e0, e1);
    return (int)hipGetLastError();
}

}  // namespace jpegamd
