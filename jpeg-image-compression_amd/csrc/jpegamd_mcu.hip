// jpegamd_mcu.hip -- k_mcu_segments: the quantised zigzag coefficients of a colour picture's three components -> the bit string
// of ONE scan of interleaved MCUs (T.81 A.2.3, F.1.2), cut into segments that the unchanged k_finalize stitches and stuffs.
//
// The coefficients are what the stage-tap build of k_tile_encode stores (int16 [blocks][64], raster block order, zigzag inside a
// block): the same numbers the three-scan entries code.  A segment is a run of S consecutive MCUs of the raster MCU order
// (S = 256 / blocks per MCU, rounded down: at most 256 blocks, so seg_cap_words(kSegTiles) holds it); one wave codes it:
//   pass 1   lane l takes blocks l, l + 64, ... of the segment (MCU order) and adds up each block's bit length.  The DC predictor
//            is the previous block of the component in scan order -- plain memory: a coefficient of another block, maybe of the
//            segment in front;
//   scan     a wave prefix sum in MCU order places the blocks;
//   pass 2   every lane codes its blocks into a bit window in LDS (ds_or).  The window owns kMcuWin words and computes one more,
//            the successor the 0xFF census of its last word needs; a longer segment takes several rounds over the window, and a
//            lane skips the blocks that lie outside the round's bits;
//   census   bits, edge, ffin[8], syms as k_segment_merge defines them (jpegamd_entropy.hip).
// A pad Y block (beyond the picture's last block column / row when the MCU grid overhangs it) is DC-only, its DC that of the
// nearest real block: a zero difference wherever that neighbour precedes it in the scan.
// k_mcu_totals: the per-call record (sums over the batch) and each picture's size word (0 when the file did not fit).
#include <hip/hip_ext.h>
#include "jpegamd_device.h"

namespace jpegamd {

constexpr int kWavesM = 4;                      // segments per workgroup
constexpr int kMcuWin = 2048;                   // window words a round owns (64 Kbit: every segment of photo-like content in one round)

// 0xFF bytes wholly inside the bit string, by byte phase (k_segment_merge's ones8_starts): bit (31 - o) of the result is set when
// the 8 stream bits from offset o of `cur` (followed by `nxt`, MSB-first) are all ones.
__device__ __forceinline__ uint32_t mcu_ones8_starts(uint32_t cur, uint32_t nxt) {
    uint32_t hi = cur & __builtin_amdgcn_alignbit(cur, nxt, 31u), lo = nxt & (nxt << 1);
    hi &= __builtin_amdgcn_alignbit(hi, lo, 30u); lo &= lo << 2;
    hi &= __builtin_amdgcn_alignbit(hi, lo, 28u);
    return hi;
}

// size and amplitude bits of a value (T.81 F.1.2.1: a negative value is coded as value - 1, low `size` bits)
__device__ __forceinline__ uint32_t mcu_size(int v) { const uint32_t mag = (uint32_t)(v < 0 ? -v : v); return mag ? 32u - (uint32_t)__clz((int)mag) : 0u; }
__device__ __forceinline__ uint32_t mcu_amp(int v, uint32_t size) { return (uint32_t)(v + (v >> 31)) & ((1u << size) - 1u); }

// The symbols of one block in order: emit(bits right-aligned, count).  tab: [272] (len << 16) | code, AC by run/size, DC sizes at 256.
template <class Emit>
__device__ __forceinline__ void mcu_walk_block(const uint4 *__restrict__ p, bool pad, int pred, const uint32_t *tab, Emit &&emit) {
    uint4 v = p[0];
    {
        const int diff = (int)(short)(v.x & 0xFFFFu) - pred;
        const uint32_t nb = mcu_size(diff), t = tab[256u + (nb & 15u)];
        emit(((t & 0xFFFFu) << nb) | mcu_amp(diff, nb), (t >> 16) + nb);
    }
    const uint32_t eob = tab[0x00], zrl = tab[0xF0];
    if (pad) { emit(eob & 0xFFFFu, eob >> 16); return; }
    v.x &= 0xFFFF0000u;                             // the DC's slot counts as one zero: the run starts at -1
    uint32_t run = 0xFFFFFFFFu;
#pragma unroll 1
    for (int q = 0; q < 8; ++q) {
        if (q) v = p[q];
        if ((v.x | v.y | v.z | v.w) == 0u) { run += 8u; continue; }
        const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int c = (int)(short)((w4[i >> 1] >> (16 * (i & 1))) & 0xFFFFu);
            if (c == 0) { ++run; continue; }
            while (run >= 16u) { emit(zrl & 0xFFFFu, zrl >> 16); run -= 16u; }
            const uint32_t nb = mcu_size(c), t = tab[((run << 4) | nb) & 0xFFu];
            emit(((t & 0xFFFFu) << nb) | mcu_amp(c, nb), (t >> 16) + nb);
            run = 0u;
        }
    }
    if (run) emit(eob & 0xFFFFu, eob >> 16);       // zigzag 63 is zero
}

struct McuBlock { const uint4 *p; int pred; bool pad, chroma; };

// Block j of MCU m of a picture whose planes start at `base`: where its coefficients lie, and its DC predictor.
__device__ __forceinline__ McuBlock mcu_block(const McuSegArgs &a, const int16_t *base, int m, int j) {
    const int ny = a.hs * a.vs;
    McuBlock b;
    const auto y_at = [&](int mm, int jj, bool *pad) {           // Y block jj of MCU mm, clamped to the picture's blocks
        const int my_ = mm / a.mx, mx_ = mm - my_ * a.mx;
        const int v = jj / a.hs, u = jj - v * a.hs;
        const int bx = mx_ * a.hs + u, by = my_ * a.vs + v;
        if (pad) *pad = bx >= a.bw || by >= a.bh;
        return base + ((size_t)min(by, a.bh - 1) * (size_t)a.bw + (size_t)min(bx, a.bw - 1)) * 64;
    };
    if (j < ny) {
        b.chroma = false;
        b.p = reinterpret_cast<const uint4 *>(y_at(m, j, &b.pad));
        b.pred = j > 0 ? (int)*y_at(m, j - 1, nullptr) : (m > 0 ? (int)*y_at(m - 1, ny - 1, nullptr) : 0);
    } else {
        const int16_t *plane = base + (j == ny ? a.cb_off : a.cr_off);
        b.chroma = true; b.pad = false;
        b.p = reinterpret_cast<const uint4 *>(plane + (size_t)m * 64);
        b.pred = m > 0 ? (int)plane[(size_t)(m - 1) * 64] : 0;
    }
    return b;
}

__global__ __launch_bounds__(64 * kWavesM) void k_mcu_segments(const McuSegArgs a) {
    __shared__ uint32_t s_tab[2][272];
    __shared__ uint32_t s_win[kWavesM][kMcuWin + 2];
    const int lane = lane_id(), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int i = (int)threadIdx.x; i < 2 * 272; i += 64 * kWavesM) s_tab[i / 272][i % 272] = (i < 272 ? a.huff_y : a.huff_c)[i % 272];
    __syncthreads();                                               // (the only workgroup-wide meeting: every wave is on its own below)
    const int seg = (int)blockIdx.x * kWavesM + wave;
    if (seg >= a.batch * a.num_segs_pad) return;
    const int image = seg / a.num_segs_pad, sl = seg - image * a.num_segs_pad;
    uint16_t *const ffin = a.seg.ffin + (size_t)seg * 8;
    if (sl >= a.num_segs) {                                        // an empty segment that rounds the picture's count up: no bits, no ones at either end
        if (lane < 8) ffin[lane] = 0;
        if (lane == 0) { a.seg.bits[seg] = 0u; a.seg.edge[seg] = 0u; a.seg.syms[seg] = 0u; a.seg.exact[seg] = 0u; }
        return;
    }
    const int16_t *base = a.coef + (size_t)image * a.pic_stride;
    const int bpm = a.hs * a.vs + 2;
    const int m0 = sl * a.seg_mcus;
    const int nblk = min(a.seg_mcus, a.mx * a.my - m0) * bpm;       // 3 .. 256
    uint32_t *win = s_win[wave];

    // ---- pass 1: bit lengths, then the blocks' places ----
    uint32_t len[4], off[4], nsym = 0, carry = 0;
    int pred[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int k = r * 64 + lane;
        len[r] = 0u; pred[r] = 0;
        if (k < nblk) {
            const int mi = k / bpm;
            const McuBlock b = mcu_block(a, base, m0 + mi, k - mi * bpm);
            pred[r] = b.pred;
            uint32_t n = 0;
            mcu_walk_block(b.p, b.pad, b.pred, s_tab[b.chroma ? 1 : 0], [&](uint32_t, uint32_t c) { n += c; ++nsym; });
            len[r] = n;
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const uint32_t incl = wave_incl_scan_u32(len[r]);
        off[r] = carry + incl - len[r];
        carry += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    }
    const uint32_t seg_bits = carry;                               // <= 256 x kMaxBlockBitsColor
    const uint32_t nwords = (seg_bits + 31u) >> 5;
    const uint32_t seg_syms = (uint32_t)wave_sum_i32((int)nsym);
    uint32_t *const segw = a.seg.words + (size_t)seg * a.seg.words_stride;

    // ---- pass 2: the window, round by round ----
    uint32_t ffc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t first_word = 0, before_last = 0, tail_last = 0, tail_part = 0;
    const uint32_t done = seg_bits >> 5;                            // complete words of the string
    for (uint32_t wbase = 0; wbase < nwords; wbase += (uint32_t)kMcuWin) {
        for (int i = lane; i < kMcuWin + 2; i += 64) win[i] = 0u;
        __builtin_amdgcn_wave_barrier();
        const uint32_t lo_bit = wbase * 32u, hi_bit = (wbase + (uint32_t)kMcuWin + 1u) * 32u;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = r * 64 + lane;
            if (k < nblk && off[r] < hi_bit && off[r] + len[r] > lo_bit) {
                const int mi = k / bpm;
                const McuBlock b = mcu_block(a, base, m0 + mi, k - mi * bpm);
                uint32_t pos = off[r];
                mcu_walk_block(b.p, b.pad, pred[r], s_tab[b.chroma ? 1 : 0], [&](uint32_t sym, uint32_t n) {
                    if (n == 0u) return;
                    const unsigned long long s64 = ((unsigned long long)sym << (64u - n)) >> (pos & 31u);   // left-aligned at the bit's place in a word pair
                    const uint32_t j = (pos >> 5) - wbase;          // (wraps for a word in front of the window)
                    const uint32_t hi = (uint32_t)(s64 >> 32), lo = (uint32_t)s64;
                    if (j <= (uint32_t)kMcuWin && hi) atomicOr(&win[j], hi);
                    if (j + 1u <= (uint32_t)kMcuWin && lo) atomicOr(&win[j + 1u], lo);
                    pos += n;
                });
            }
        }
        __builtin_amdgcn_wave_barrier();
        const uint32_t nown = min((uint32_t)kMcuWin, nwords - wbase);   // words this round owns; win[nown] is final too (computed, or zero behind the string)
        for (uint32_t i0 = 0; i0 < nown; i0 += 64u) {
            const uint32_t i = i0 + (uint32_t)lane;
            uint32_t cw = 0, nw = 0;
            if (i < nown) { cw = win[i]; nw = win[i + 1u]; segw[wbase + i] = cw; }
            const uint32_t m = mcu_ones8_starts(cw, nw);
            if (__ballot(m != 0u) != 0ull) {
#pragma unroll
                for (int p = 0; p < 8; ++p) ffc[p] += (uint32_t)__popc(m & (0x80808080u >> ((8 - p) & 7)));
            }
        }
        if (wbase == 0u) first_word = win[0];
        if (done >= wbase && done <= wbase + (uint32_t)kMcuWin) {  // a round that holds the string's end (word `done` may be the one computed beyond the owned ones)
            tail_last = done > wbase ? win[done - 1u - wbase] : before_last;
            tail_part = win[done - wbase];
        }
        before_last = win[nown - 1u];
        __builtin_amdgcn_wave_barrier();
    }
    {
        const uint32_t p = seg_bits & 31u;
        const uint32_t tail = p ? ((tail_last << p) | (tail_part >> (32u - p))) : tail_last;
        if (lane == 0) {
            a.seg.edge[seg] = ((first_word >> 24) << 8) | (tail & 0x7Fu);   // first 8 bits | last 7 bits (a segment is never shorter than 14 bits)
            a.seg.bits[seg] = seg_bits;
            a.seg.syms[seg] = seg_syms;
            a.seg.exact[seg] = 0u;                                  // (the exact-order fallbacks are counted from the tile records: k_picture_stats)
        }
    }
    uint32_t mine = 0;
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        const uint32_t t = (uint32_t)wave_sum_i32((int)ffc[p]);
        if (lane == p) mine = t;
    }
    if (lane < 8) {
        ffin[lane] = (uint16_t)min(mine, 65535u);
        if (mine > 65535u) atomicOr(a.status, 2u);
    }
}

int launch_mcu_segments(const McuSegArgs &a, void *stream) {
    const int n = a.batch * a.num_segs_pad;
    if (n <= 0) return 0;
    if (a.seg_mcus < 1 || a.seg_mcus * (a.hs * a.vs + 2) > kSegBlocks || a.num_segs_pad % kSegGroup != 0 ||
        (int64_t)a.num_segs * a.seg_mcus < (int64_t)a.mx * a.my || a.num_segs > a.num_segs_pad)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_mcu_segments, dim3((unsigned)((n + kWavesM - 1) / kWavesM)), dim3(64 * kWavesM), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

// Workgroup q: picture q of the launch.  Sums of its segments' bits and symbols; its stuffed bytes follow from its size (a file is
// its prefix, the scan's bits, the flush byte, a 0x00 per 0xFF, and EOI); the size word becomes 0 when the file did not fit.
__global__ __launch_bounds__(256) void k_mcu_totals(const McuTotalsArgs a) {
    __shared__ unsigned long long s_part[2][4];
    const int q = (int)blockIdx.x;
    unsigned long long bits = 0, syms = 0;
    for (int i = (int)threadIdx.x; i < a.num_segs_pad; i += 256) {
        bits += a.seg.bits[(size_t)q * a.num_segs_pad + i];
        syms += a.seg.syms[(size_t)q * a.num_segs_pad + i];
    }
    for (int off = 32; off > 0; off >>= 1) { bits += __shfl_xor(bits, off, 64); syms += __shfl_xor(syms, off, 64); }
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    if (lane == 0) { s_part[0][wave] = bits; s_part[1][wave] = syms; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    bits = s_part[0][0] + s_part[0][1] + s_part[0][2] + s_part[0][3];
    syms = s_part[1][0] + s_part[1][1] + s_part[1][2] + s_part[1][3];
    const uint32_t st = a.scan_stats->status;
    const uint64_t size = *a.out_size[q];                           // k_finalize's: the would-be size when it did not fit
    const bool fit = (st & ~1u) == 0u && size <= a.out_capacity;
    const unsigned long long *pic = a.pic + (size_t)q * kPicStatWords;
    ScanStats *t = a.stats;
    atomicAdd((unsigned long long *)&t->total_bits, bits);
    atomicAdd((unsigned long long *)&t->total_syms, syms);
    atomicAdd((unsigned long long *)&t->total_exact, pic[2] + pic[5] + pic[8]);
    atomicAdd((unsigned long long *)&t->total_ff, (unsigned long long)(size - (uint64_t)a.prefix_len - 2u - (bits + 7u) / 8u));
    if (!fit) *a.out_size[q] = 0ull;
    if (a.last_of_call && q == (int)gridDim.x - 1) t->out_size = fit ? size : 0ull;
    const uint32_t add = st | (fit ? 0u : 1u);
    if (add) atomicOr(&t->status, add);
}

int launch_mcu_totals(const McuTotalsArgs &a, int batch, void *stream, void *const *ev) {
    if (batch < 1 || batch > kMaxBatch) return (int)hipErrorInvalidValue;
    hipEvent_t e0 = ev ? (hipEvent_t)ev[0] : nullptr, e1 = ev ? (hipEvent_t)ev[1] : nullptr;
    hipExtLaunchKernelGGL(k_mcu_totals, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, e0, e1, 0, a);
    return (int)hipGetLastError();
}

}  // namespace jpegamd
