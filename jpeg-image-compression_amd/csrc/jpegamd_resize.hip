// jpegamd_resize.hip -- the one kernel a batch of resized pictures (jpegamd_encode_resized_batch_async and its twins) runs in front of
// the tile encoder.
//
//   k_resize_planes_batch  every picture of the batch -> every sample of the width x height target as the exact area mean of the
//                          source (jpeg_compression.h, "Resized pictures": (S + (D >> 1)) / D with S the source samples weighted
//                          by their share of the target sample's footprint and D = src_width src_height), then the header's
//                          RGB -> YCbCr map and chroma subsampling -> 8-bit Y, Cb and Cr planes of the TARGET in context scratch,
//                          laid out as k_float_planes_batch lays them out
// A workgroup owns a band of target rows and a span of target columns, stages the source rows under them in LDS a few at a time with
// lane-contiguous loads, and its threads read their windows from there.  No inline assembly.
#include <hip/hip_ext.h>
#include <algorithm>
#include "jpegamd_device.h"

namespace jpegamd {

constexpr int kRsOut = 4;                 // chroma samples per thread: one 4-byte store per plane (the pitches are multiples of 4)

// Thread (tx, ty) of workgroup (bx, by, p) owns chroma samples c0 .. c0 + 3 of chroma row cy of target picture p, the kSx x kSy target
// pixels under each and the footprint of each of those in the source, with c0 = 4 (bx blockDim.x + tx), cy = by blockDim.y + ty.  The
// block's shape is the host's choice (launch_resize_planes_batch): as wide as the staged rows allow, and whole waves.
//
// The workgroup walks the source rows of its band, a.lds_rows at a time.  Staging: wave w takes row-and-run u = w, w + waves, ...;
// a run is the bytes of one source row under the workgroup's columns -- one per channel (kPacked false), or the pixels themselves with
// their channels side by side (kPacked) -- copied in 16-byte pieces where a piece lies inside the row's own pixel_stride x src_width
// bytes and byte by byte where it does not, to the LDS position that has the global address's low four bits; kResizeWalkGeneric
// gathers bytes pixel_stride apart instead.  Nothing outside a row's own bytes is read.  Then every thread adds, for each of its pixels
// and each staged row of that pixel's footprint, wy * (sum over the window of wx * s): the horizontal sum is below 2^24, the total
// needs 64 bits.  The first and the last sample of a window carry partial weights, the ones between them a.width (a.height for rows).
// kOut is what is written: Y, Cb and Cr planes; the Y plane alone of three channels; or the single channel's means as the Y plane (the
// last two at kSx = kSy = 1).  Every store is a dword into the kernel's own pitched scratch; the bytes of a stored dword past the
// plane's width are never coded.
template <int kSx, int kSy, bool kPacked, int kOut>
__global__ __launch_bounds__(256) void k_resize_planes_batch(const ResizePlanesBatchArgs a) {
    static_assert((kSx == 1 || kSx == 2) && (kSy == 1 || kSy == 2) && kSy <= kSx, "4:4:4, 4:2:2 or 4:2:0");
    static_assert(kOut == kResizeOutColor || (kSx == 1 && kSy == 1), "a Y plane alone has no chroma grid");
    static_assert(kOut != kResizeOutSingle || !kPacked, "one channel is not packed");
    extern __shared__ __align__(16) uint8_t staged[];
    constexpr int kC = kOut == kResizeOutSingle ? 1 : 3;                     // channels read
    constexpr int kRuns = kPacked ? 1 : kC;                                  // staged runs per source row
    constexpr int kPix = kRsOut * kSx;                                       // target pixels per row and thread
    const int p = (int)blockIdx.z, bw = (int)blockDim.x, bh = (int)blockDim.y;
    const uint32_t W = (uint32_t)a.src_width, H = (uint32_t)a.src_height, ow = (uint32_t)a.width, oh = (uint32_t)a.height;
    const int step = kPacked ? a.pixel_stride : 1;                          // bytes between the samples of a channel in LDS
    // the workgroup's target pixels [X0, X1) x [Y0, Y1) and the source samples under them [xs, xe) x [ys, ye); every product is
    // below 65535^2 + 65535 < 2^32
    const uint32_t X0 = blockIdx.x * (uint32_t)(bw * kPix), X1 = min(ow, X0 + (uint32_t)(bw * kPix));
    const uint32_t Y0 = blockIdx.y * (uint32_t)(bh * kSy), Y1 = min(oh, Y0 + (uint32_t)(bh * kSy));
    const int xs = (int)(X0 * W / ow), xe = (int)((X1 * W + ow - 1) / ow);  // xe <= W
    const int ys = (int)(Y0 * H / oh), ye = (int)((Y1 * H + oh - 1) / oh);  // ye <= H
    // the thread's own samples
    const int c0 = kRsOut * (int)(blockIdx.x * blockDim.x + threadIdx.x), cy = (int)(blockIdx.y * blockDim.y + threadIdx.y);
    const bool active = c0 < a.cw && cy < a.ch;
    const int x0 = c0 * kSx;                                                 // active: < width, as 4 gx < cw = ceil(width / kSx)
    const int npx = active ? min(kPix, a.width - x0) : 0;                    // the thread's target pixels inside the row (>= 1)
    int fa[kPix], fn[kPix];                                                  // a window's first column from xs; its columns less one
    uint32_t fw[kPix];                                                       // the weight of its first column
#pragma unroll
    for (int j = 0; j < kPix; ++j) {
        fa[j] = 0; fn[j] = 0; fw[j] = 0;
        if (j < npx) {
            const uint32_t lo = (uint32_t)(x0 + j) * W, hi = lo + W, first = lo / ow;
            fa[j] = (int)first - xs;
            fn[j] = (int)((hi + ow - 1) / ow - 1 - first);
            fw[j] = min((first + 1) * ow, hi) - lo;
        }
    }
    uint32_t ylo[kSy], ya[kSy], yb[kSy];                                     // Y H; the footprint's first and last row
#pragma unroll
    for (int r = 0; r < kSy; ++r) {
        const uint32_t y = (uint32_t)min(cy * kSy + r, a.height - 1);       // the last row replicated (an odd height: not stored below)
        ylo[r] = y * H;
        ya[r] = ylo[r] / oh;
        yb[r] = (ylo[r] + H + oh - 1) / oh - 1;
    }
    uint64_t acc[kSy][kC][kPix];
#pragma unroll
    for (int r = 0; r < kSy; ++r)
#pragma unroll
        for (int c = 0; c < kC; ++c)
#pragma unroll
            for (int j = 0; j < kPix; ++j) acc[r][c][j] = 0;

    const int tid = (int)(threadIdx.y * blockDim.x + threadIdx.x), lane = tid & 63, wave = tid >> 6;
    const int waves = (bw * bh + 63) >> 6;
    const size_t row_bytes = (size_t)a.pixel_stride * W;                    // a row's own bytes from the run's first
    const bool gather = a.walk == kResizeWalkGeneric;                        // uniform: bytes pixel_stride apart, no lead in LDS
    for (int yc = ys; yc < ye; yc += a.lds_rows) {
        const int yce = min(ye, yc + a.lds_rows);
        for (int u = wave; u < (yce - yc) * kRuns; u += waves) {
            const int li = u / kRuns, k = u - li * kRuns;
            const uint8_t *g = a.plane[k][p] + (size_t)(yc + li) * (size_t)a.row_stride;
            uint8_t *l = staged + (size_t)u * (size_t)a.lds_pitch;
            if (gather) {
                for (int x = lane; x < xe - xs; x += 64) l[x] = g[(size_t)(xs + x) * (size_t)a.pixel_stride];
            } else {
                const uint8_t *b = g + (size_t)xs * (size_t)step;
                const int lead = (int)((uintptr_t)b & 15);
                const uint8_t *b16 = b - lead;                               // (never dereferenced below g)
                const int pieces = (lead + (xe - xs) * step + 15) >> 4;      // 16 pieces <= lds_pitch
                for (int i = lane; i < pieces; i += 64) {
                    const uint8_t *q = b16 + 16 * i;
                    if ((uintptr_t)q >= (uintptr_t)g && (uintptr_t)(q + 16) <= (uintptr_t)(g + row_bytes)) {
                        *reinterpret_cast<uint4 *>(l + 16 * i) = *reinterpret_cast<const uint4 *>(q);
                    } else {
                        for (int t = 0; t < 16; ++t)
                            if ((uintptr_t)(q + t) >= (uintptr_t)g && (uintptr_t)(q + t) < (uintptr_t)(g + row_bytes)) l[16 * i + t] = q[t];
                    }
                }
            }
        }
        __syncthreads();
        if (active) {
#pragma unroll
            for (int r = 0; r < kSy; ++r) {
                const int y_first = max((int)ya[r], yc), y_last = min((int)yb[r], yce - 1);
                for (int y = y_first; y <= y_last; ++y) {
                    const uint32_t wy = min(ylo[r] + H, (uint32_t)(y + 1) * oh) - max(ylo[r], (uint32_t)y * oh);
                    const uint8_t *row[kC];
#pragma unroll
                    for (int c = 0; c < kC; ++c) {
                        const int k = kPacked ? 0 : c;
                        const uint8_t *l = staged + (size_t)((y - yc) * kRuns + k) * (size_t)a.lds_pitch;
                        if (!gather)
                            l += (uintptr_t)(a.plane[k][p] + (size_t)y * (size_t)a.row_stride + (size_t)xs * (size_t)step) & 15;
                        row[c] = kPacked ? l + a.offset[c] : l;
                    }
#pragma unroll
                    for (int j = 0; j < kPix; ++j) {
                        if (j < npx) {
#pragma unroll
                            for (int c = 0; c < kC; ++c) {
                                const uint8_t *s = row[c] + fa[j] * step;
                                uint32_t hsum = fw[j] * s[0];
                                if (fn[j] > 0) {
                                    // the weights of a window add up to W: the first, fn[j] - 1 whole samples, the last
                                    const uint32_t w_last = W - fw[j] - (uint32_t)(fn[j] - 1) * ow;
                                    uint32_t mid = 0;
                                    for (int t = 1; t < fn[j]; ++t) mid += s[t * step];
                                    hsum += ow * mid + w_last * s[fn[j] * step];
                                }
                                acc[r][c][j] += (uint64_t)wy * hsum;
                            }
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
    if (!active) return;

    int cb[kSy][kPix], cr[kSy][kPix];
    uint8_t *yp = a.yplanes + (size_t)p * a.yplane_bytes;
#pragma unroll
    for (int r = 0; r < kSy; ++r) {
        const int y = min(cy * kSy + r, a.height - 1);
        // the means; a target pixel past the row's end holds the row's last one
        int v[kC][kPix];
#pragma unroll
        for (int j = 0; j < kPix; ++j) {
            if (j == 0 || j < npx) {
#pragma unroll
                for (int c = 0; c < kC; ++c) v[c][j] = (int)resize_divide(acc[r][c][j] + (a.div.d >> 1), a.div.d, a.div.mul, a.div.shift);
            } else {
#pragma unroll
                for (int c = 0; c < kC; ++c) v[c][j] = v[c][j - 1];
            }
        }
        const bool stored = cy * kSy + r < a.height;
#pragma unroll
        for (int i = 0; i < kSx; ++i) {
            uint32_t word = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int j = 4 * i + k;
                int luma;
                if constexpr (kOut == kResizeOutSingle) luma = v[0][j];
                else luma = (77 * v[0][j] + 150 * v[1][j] + 29 * v[2][j]) >> 8;
                word |= (uint32_t)luma << (8 * k);
            }
            // x0 + 4 i is a multiple of 4 below the width, so the dword lies inside the row's ypitch bytes
            if (stored && x0 + 4 * i < a.width) *reinterpret_cast<uint32_t *>(yp + (size_t)y * (size_t)a.ypitch + (size_t)(x0 + 4 * i)) = word;
        }
        if constexpr (kOut == kResizeOutColor) {
            // Cb = (32768 - 43 R - 85 G + 128 B) >> 8, Cr = (32768 + 128 R - 107 G - 21 B) >> 8, per target pixel (k_chroma_planes' cbcr)
#pragma unroll
            for (int j = 0; j < kPix; ++j) {
                cb[r][j] = (32768 - 43 * v[0][j] - 85 * v[1][j] + 128 * v[2][j]) >> 8;
                cr[r][j] = (32768 + 128 * v[0][j] - 107 * v[1][j] - 21 * v[2][j]) >> 8;
            }
        }
    }
    if constexpr (kOut == kResizeOutColor) {
        uint32_t wcb = 0, wcr = 0;
#pragma unroll
        for (int k = 0; k < kRsOut; ++k) {
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

template <bool kPacked>
static void launch_resize_as(const ResizePlanesBatchArgs &a, dim3 grid, dim3 block, unsigned lds, hipStream_t s, hipEvent_t e0, hipEvent_t e1) {
    if (a.out == kResizeOutColor) {
        if (a.mode == kChromaMode420) hipExtLaunchKernelGGL((k_resize_planes_batch<2, 2, kPacked, kResizeOutColor>), grid, block, lds, s, e0, e1, 0, a);
        else if (a.mode == kChromaMode422) hipExtLaunchKernelGGL((k_resize_planes_batch<2, 1, kPacked, kResizeOutColor>), grid, block, lds, s, e0, e1, 0, a);
        else hipExtLaunchKernelGGL((k_resize_planes_batch<1, 1, kPacked, kResizeOutColor>), grid, block, lds, s, e0, e1, 0, a);
    } else if (a.out == kResizeOutLuma) {
        hipExtLaunchKernelGGL((k_resize_planes_batch<1, 1, kPacked, kResizeOutLuma>), grid, block, lds, s, e0, e1, 0, a);
    } else if constexpr (!kPacked) {
        hipExtLaunchKernelGGL((k_resize_planes_batch<1, 1, false, kResizeOutSingle>), grid, block, lds, s, e0, e1, 0, a);
    }
}

int launch_resize_planes_batch(const ResizePlanesBatchArgs &args, void *stream, void *const *ev) {
    ResizePlanesBatchArgs a = args;
    const bool color = a.out == kResizeOutColor, packed = a.walk == kResizeWalkPacked;
    const int sx = color && a.mode != kChromaMode444 ? 2 : 1, sy = color && a.mode == kChromaMode420 ? 2 : 1;
    if ((a.out != kResizeOutColor && a.out != kResizeOutLuma && a.out != kResizeOutSingle) ||
        (color && a.mode != kChromaMode444 && a.mode != kChromaMode420 && a.mode != kChromaMode422) ||
        (a.walk != kResizeWalkPlanar && a.walk != kResizeWalkPacked && a.walk != kResizeWalkGeneric) ||
        (packed && a.out == kResizeOutSingle) || a.batch < 1 || a.batch > kMaxBatch ||
        a.src_width <= 0 || a.src_height <= 0 || a.src_width > 65535 || a.src_height > 65535 ||
        a.width < 1 || a.width > a.src_width || (int64_t)a.src_width > (int64_t)kMaxResizeRatio * a.width ||
        a.height < 1 || a.height > a.src_height || (int64_t)a.src_height > (int64_t)kMaxResizeRatio * a.height ||
        a.cw != (a.width + sx - 1) / sx || a.ch != (a.height + sy - 1) / sy ||
        a.pixel_stride < 1 || (int64_t)a.row_stride < (int64_t)a.pixel_stride * a.src_width ||
        (a.walk == kResizeWalkPlanar && a.pixel_stride != 1) ||
        (packed && (a.pixel_stride > kResizePackedMax || a.offset[0] < 0 || a.offset[1] < 0 || a.offset[2] < 0 ||
                    a.offset[0] >= a.pixel_stride || a.offset[1] >= a.pixel_stride || a.offset[2] >= a.pixel_stride)) ||
        a.ypitch % 4 != 0 || a.ypitch < (a.width + 3) / 4 * 4 || a.yplane_bytes % 16 != 0 ||
        a.yplane_bytes < (uint64_t)a.ypitch * (uint64_t)a.height || !a.yplanes ||
        (color && (a.pitch % 4 != 0 || a.pitch < (a.cw + 3) / 4 * 4 || a.plane_bytes % 16 != 0 ||
                   a.plane_bytes < (uint64_t)a.pitch * (uint64_t)a.ch || !a.planes)))
        return (int)hipErrorInvalidValue;
    a.div = resize_divide_for((uint32_t)a.src_width * (uint32_t)a.src_height);
    // The block: 32 x 8 threads, halved in x and doubled in y while one staged source row of every run is more than the budget holds
    // (4 or 8 target pixels are at most 513 samples of at most 4 bytes) or the row of workgroups would be half idle, then cut in y to
    // the rows there are -- down to one wave, never below: the staging loops stride by 64 lanes.
    const int kpix = kRsOut * sx, runs = packed || a.out == kResizeOutSingle ? 1 : 3, step = packed ? a.pixel_stride : 1;
    const auto pitch_of = [&](int bw) {
        const int64_t span = std::min<int64_t>(a.src_width, ((int64_t)bw * kpix * a.src_width + a.width - 1) / a.width + 1);
        return (int)((span * step + 45) & ~(int64_t)15);                     // 15 bytes of lead, the last 16-byte piece whole
    };
    int bw = 32, bh = 8;
    while (bw > 1 && (kRsOut * (bw / 2) >= a.cw || runs * pitch_of(bw) > kResizeLdsBudget)) { bw /= 2; bh *= 2; }
    while (bh / 2 >= a.ch && bw * (bh / 2) >= 64) bh /= 2;
    a.lds_pitch = pitch_of(bw);
    const int64_t band = std::min<int64_t>(a.src_height, ((int64_t)bh * sy * a.src_height + a.height - 1) / a.height + 1);
    a.lds_rows = (int)std::max<int64_t>(1, std::min<int64_t>(band, kResizeLdsBudget / (runs * a.lds_pitch)));
    const unsigned lds = (unsigned)(a.lds_rows * runs * a.lds_pitch);
    if (lds > (unsigned)kResizeLdsBudget) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.cw + kRsOut * bw - 1) / (kRsOut * bw)), (unsigned)((a.ch + bh - 1) / bh), (unsigned)a.batch), block(bw, bh);
    hipEvent_t e0 = ev ? (hipEvent_t)ev[0] : nullptr, e1 = ev ? (hipEvent_t)ev[1] : nullptr;
    hipStream_t s = (hipStream_t)stream;
    if (packed) launch_resize_as<true>(a, grid, block, lds, s, e0, e1);
    else launch_resize_as<false>(a, grid, block, lds, s, e0, e1);
    return (int)hipGetLastError();
}

}  // namespace jpegamd
