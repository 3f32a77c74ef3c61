// jpegamd_color.hip -- the two kernels of a colour encode (jpegamd_encode_color_async) besides the grayscale pipeline's own.
//
// A colour file is three non-interleaved baseline scans (colour scans): Y through the unchanged RGB path of
// k_tile_encode, then Cb and Cr as 8-bit planes through its one-byte mode with the chroma tables.
//   k_chroma_planes   the picture, read once in any layout the API accepts -> the Cb and Cr planes in context scratch
//   k_append_scans    the two chroma scans (coded into context scratch) copied behind the Y scan in the caller's buffer, at the
//                     offsets the device computed: no host synchronisation between the scans
#include <hip/hip_ext.h>
#include "jpegamd_device.h"

namespace jpegamd {

// Cb = (32768 - 43 R - 85 G + 128 B) >> 8, Cr = (32768 + 128 R - 107 G - 21 B) >> 8 (the sums lie in [128, 65408]: no clamp).
__device__ __forceinline__ void cbcr(int r, int g, int b, int &cb, int &cr) {
    cb = (32768 - 43 * r - 85 * g + 128 * b) >> 8;
    cr = (32768 + 128 * r - 107 * g - 21 * b) >> 8;
}

constexpr int kPlaneOut = 4;              // chroma samples per thread: one 4-byte store per plane (the pitch is a multiple of 4)

// kSub: 2 (4:2:0, 2 x 2 pixels per sample) or 1 (4:4:4).  Thread (gx, cy) makes samples 4 gx .. 4 gx + 3 of plane row cy.
template <int kSub>
__global__ __launch_bounds__(256) void k_chroma_planes(const ChromaPlanesArgs a) {
    constexpr int kPix = kPlaneOut * kSub;                                   // source pixels per row and thread
    const int gx = (int)(blockIdx.x * blockDim.x + threadIdx.x), cy = (int)blockIdx.y;
    const int x0 = gx * kPix;
    if (kPlaneOut * gx >= a.cw) return;                                      // (then x0 < width as well)
    int cb[kSub][kPix], cr[kSub][kPix];
#pragma unroll
    for (int r = 0; r < kSub; ++r) {
        const int y = min(cy * kSub + r, a.height - 1);                      // the last row replicated (odd heights)
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
        if (kSub == 2) {
            // the pair's right pixel is the replicated last column when 2 x + 1 == width; (a + b + c + d + 2) >> 2
            const int j0 = 2 * k, j1 = x0 + 2 * k + 1 < a.width ? 2 * k + 1 : 2 * k;
            vb = (cb[0][j0] + cb[0][j1] + cb[kSub - 1][j0] + cb[kSub - 1][j1] + 2) >> 2;
            vr = (cr[0][j0] + cr[0][j1] + cr[kSub - 1][j0] + cr[kSub - 1][j1] + 2) >> 2;
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
    if (a.sub420) {
        if (ev) hipExtLaunchKernelGGL(k_chroma_planes<2>, grid, block, 0, (hipStream_t)stream, (hipEvent_t)ev[0], (hipEvent_t)ev[1], 0, a);
        else hipLaunchKernelGGL(k_chroma_planes<2>, grid, block, 0, (hipStream_t)stream, a);
    } else {
        if (ev) hipExtLaunchKernelGGL(k_chroma_planes<1>, grid, block, 0, (hipStream_t)stream, (hipEvent_t)ev[0], (hipEvent_t)ev[1], 0, a);
        else hipLaunchKernelGGL(k_chroma_planes<1>, grid, block, 0, (hipStream_t)stream, a);
    }
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

}  // namespace jpegamd
