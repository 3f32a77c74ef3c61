// jpegamd_metadata.hip -- k_metadata_place: the caller's marker segments in front of the tables.
//
// A context that holds metadata of M bytes runs every entry's own launches with out + M and out_capacity - M, so the file F of the
// call lies at out + M.  This kernel, launched once behind them, copies 20 + M bytes from context scratch -- F's 20 leading bytes
// (SOI, APP0) with the caller's density, then the segments -- to out[0, 20 + M): over the shifted copy of F[0, 20) at out + M, which
// the segments end on, and F[20, ..) stays where it belongs.  No coder, writer or header cache knows about it.
//
// A copy and nothing else, so it is shaped for bandwidth: M is a 3 KiB sRGB profile in the common case, but may be megabytes (a
// printer profile) times 32 pictures.  Workgroup (bx, p) copies 16-byte pieces of picture p; the stores are whole 16-byte stores
// on the destination's absolute 16-byte boundaries, whatever the caller's pointer; the source then sits at a fixed byte offset h
// (0 .. 15) from its own boundaries, and every piece is made of the two aligned pieces it straddles, shifted.  At most 15 single
// bytes in front of the first piece and 15 behind the last.  No LDS, no atomics.
#include <hip/hip_ext.h>
#include "jpegamd_device.h"

namespace jpegamd {

constexpr int kPlaceThreads = 256;
constexpr int kPlacePieces = 4;           // 16-byte pieces per thread, kPlaceThreads apart (each of the four rounds is coalesced)

// Bytes [4 kQ + r, 4 kQ + r + 16) of the 32 that a and b hold.
template <int kQ>
__device__ __forceinline__ uint4 straddle(const uint4 &a, const uint4 &b, uint32_t r) {
    const uint32_t d[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    const auto two = [&](int k) { return (uint32_t)(((((uint64_t)d[k + 1]) << 32) | d[k]) >> (8u * r)); };
    return make_uint4(two(kQ), two(kQ + 1), two(kQ + 2), two(kQ + 3));
}

__global__ __launch_bounds__(kPlaceThreads) void k_metadata_place(const MetadataPlaceArgs a) {
    const int p = (int)blockIdx.y;
    const uint64_t n = a.bytes, m = n - (uint64_t)kJfifHeadBytes;
    // one lane per picture: the size (a zero -- the file did not fit -- stays zero); the last picture's lane: the context's record too
    if (blockIdx.x == 0 && threadIdx.x == 63) {
        const uint64_t size = *a.out_size[p];
        if (size) *a.out_size[p] = size + m;
        if (p == a.batch - 1 && a.stats->out_size) a.stats->out_size += m;
    }
    if (n > a.out_capacity) return;                                   // nothing of this picture's buffer is touched
    uint8_t *dst = a.out[p];
    const uint64_t to_boundary = (0u - (uint64_t)(uintptr_t)dst) & 15u;
    const uint32_t h = (uint32_t)(to_boundary < n ? to_boundary : n);
    const uint64_t pieces = (n - h) >> 4, tail = h + (pieces << 4);
    if (blockIdx.x == 0 && threadIdx.x < 32) {                        // the ends: lanes 0 .. 15 the bytes in front, 16 .. 31 those behind
        const uint32_t k = threadIdx.x;
        if (k < 16u) { if (k < h) dst[k] = a.src[k]; }
        else if (tail + (k - 16u) < n) dst[tail + (k - 16u)] = a.src[tail + (k - 16u)];
    }
    const uint4 *src16 = reinterpret_cast<const uint4 *>(a.src);      // piece i of the destination is source bytes [16 i + h, 16 i + h + 16)
    uint4 *dst16 = reinterpret_cast<uint4 *>(dst + h);
    const uint32_t r = h & 3u;
    const uint64_t first = (uint64_t)blockIdx.x * (kPlaceThreads * kPlacePieces) + threadIdx.x;
    uint4 lo[kPlacePieces], hi[kPlacePieces];
#pragma unroll
    for (int u = 0; u < kPlacePieces; ++u) {
        const uint64_t i = first + (uint64_t)u * kPlaceThreads;
        if (i < pieces) { lo[u] = src16[i]; hi[u] = src16[i + 1]; }   // (the scratch is padded: piece `pieces` exists)
    }
#pragma unroll
    for (int u = 0; u < kPlacePieces; ++u) {
        const uint64_t i = first + (uint64_t)u * kPlaceThreads;
        if (i >= pieces) continue;
        uint4 v;
        switch (h >> 2) {                                             // (uniform over the workgroup)
            case 0: v = straddle<0>(lo[u], hi[u], r); break;
            case 1: v = straddle<1>(lo[u], hi[u], r); break;
            case 2: v = straddle<2>(lo[u], hi[u], r); break;
            default: v = straddle<3>(lo[u], hi[u], r); break;
        }
        dst16[i] = v;
    }
}

int launch_metadata_place(const MetadataPlaceArgs &a, void *stream, void *end_event) {
    if (a.batch < 1 || a.batch > kMaxBatch || a.bytes < (uint64_t)kJfifHeadBytes || !a.src || ((uintptr_t)a.src & 15u)) return (int)hipErrorInvalidValue;
    const uint64_t per_wg = (uint64_t)kPlaceThreads * kPlacePieces;
    const uint64_t wgs = ((a.bytes >> 4) + per_wg - 1) / per_wg;
    const dim3 grid((unsigned)(wgs ? wgs : 1), (unsigned)a.batch);
    hipExtLaunchKernelGGL(k_metadata_place, grid, dim3(kPlaceThreads), 0, (hipStream_t)stream, nullptr, (hipEvent_t)end_event, 0, a);
    return (int)hipGetLastError();
}

}  // namespace jpegamd
