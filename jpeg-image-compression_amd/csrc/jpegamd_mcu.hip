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
// With restart intervals a segment is a run of MCUs of ONE interval, the predictors are 0 at the interval's first
// MCU, and k_mcu_restart_offsets + k_mcu_restart_write stand in for k_finalize: per-interval padding with 1-bits, stuffing, RSTn.
// k_mcu_totals: the per-call record (sums over the batch) and each picture's size word (0 when the file did not fit).
// Per-picture optimised Huffman tables: k_mcu_histogram walks the coder's segments and counts every symbol,
// k_huff_optimal makes each picture's four tables (T.81 K.2 as libjpeg carries it out), its coder tables and its prefix with its own
// DHT segments; k_mcu_segments then codes with the picture's tables and the restart writer places the picture's prefix.
// A scan of ONE component (the grayscale file with restart intervals and its own tables) is the kComps = 1
// instantiation of both walks: the MCU is one block, a segment 256 consecutive blocks of one interval, the predictor the block in
// front; no pad blocks, no chroma tables.  The three-component instantiations are what they were.
// Progressive files: the segment coder is mcu_code_segments, which k_mcu_segments instantiates with the walk of a
// whole block and k_mcu_band_segments with the DC-only walk (the three-component DC scan) or the walk of a band ss .. se (an AC scan of
// one component); k_scans_concat joins the seven scans k_finalize wrote.
// ... with end-of-band runs and a table per scan: the band walk without end symbols plus mcu_band_runs
// (kWalkBandRuns), k_mcu_band_histogram counting what that walk codes, k_huff_optimal over all eight tables of a picture at once,
// k_prog_tables making the coder's tables and every scan's DHT + SOS, and the restart writer placing each scan behind its header.
// ... with successive approximation: four more walks -- the DC and a band by a point transform, one bit of the DC,
// one bit of a band (T.81 G.1.2.3) --, raw bits through an outlet of their own that the counting kernel does not see, and a scan and
// table count that k_prog_tables and k_scans_concat take at run time.
// ... with a scan script of the caller's, and grayscale files: the DC scan of ONE component (kComps = 1 with the DC
// walks) and of TWO interleaved components (kComps = 2, McuSegArgs::mask) as instantiations of their own, up to 16 scans and tables.
#include <algorithm>

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

// ---- the walks of a progressive file's scans (spectral selection, Ah = Al = 0) --------------------------------
// The DC scan: a block is its DC difference alone -- a pad block's too: its DC is the nearest real block's.
template <class Tab, class Emit>
__device__ __forceinline__ void mcu_walk_dc(const uint4 *__restrict__ p, int pred, const Tab &tab, Emit &&emit) {
    const int diff = (int)*reinterpret_cast<const int16_t *>(p) - pred;
    const uint32_t nb = mcu_size(diff), t = tab[256u + (nb & 15u)];
    emit(((t & 0xFFFFu) << nb) | mcu_amp(diff, nb), (t >> 16) + nb);
}

// Bits 16 i .. 16 i + 15 of a word that holds coefficients j0 and j0 + 1 of a group of eight: all ones where lo <= j <= hi.
__device__ __forceinline__ uint32_t mcu_band_mask(int j0, int lo, int hi) {
    return ((j0 >= lo && j0 <= hi) ? 0x0000FFFFu : 0u) | ((j0 + 1 >= lo && j0 + 1 <= hi) ? 0xFFFF0000u : 0u);
}

// An AC scan of the band ss .. se (1 <= ss <= se <= 63, the same for the whole launch): T.81 G.1.2.2 without EOB runs -- the zero
// run is 0 at ss, sixteen zeros are a ZRL, and the block ends with EOB0 (symbol 0x00) when coefficient se is zero, with nothing when
// it is not.  Only the 16-byte groups that hold ss .. se are read (1 .. 5: p[0] alone); what a group holds outside the band is
// masked to zero, and the run starts at minus the coefficients masked in front of ss.  A band's string is never longer than the
// whole block's (the same symbols at most, one per coefficient, a ZRL per sixteen zeros, an EOB for a zero coefficient se).
// kRuns: nothing is emitted for the trailing zeros -- the caller codes end-of-band runs over the blocks of a
// segment (mcu_band_runs).  Returns whether coefficient se is zero.  Tab: a coder table, or McuSymbolTab to count symbols.
// kPoint: the walk is over v = sign(c) (|c| >> al), the first scan of a band cut by successive approximation.
template <bool kRuns = false, bool kPoint = false, class Tab, class Emit>
__device__ __forceinline__ bool mcu_walk_band(const uint4 *__restrict__ p, int ss, int se, const Tab &tab, Emit &&emit, [[maybe_unused]] int al = 0) {
    const uint32_t eob = kRuns ? 0u : tab[0x00], zrl = tab[0xF0];
    const int q1 = se >> 3;
    uint32_t run = 0u - (uint32_t)(ss & 7);
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll 1
    for (int q = ss >> 3; q <= q1; ++q) {
        v = p[q];
        const int lo = ss - 8 * q, hi = se - 8 * q;                // the band in this group: coefficients max(lo, 0) .. min(hi, 7)
        if (lo > 0 || hi < 7) {
            v.x &= mcu_band_mask(0, lo, hi); v.y &= mcu_band_mask(2, lo, hi);
            v.z &= mcu_band_mask(4, lo, hi); v.w &= mcu_band_mask(6, lo, hi);
        }
        if ((v.x | v.y | v.z | v.w) == 0u) { run += 8u; continue; }
        const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            int c = (int)(short)((w4[i >> 1] >> (16 * (i & 1))) & 0xFFFFu);
            if constexpr (kPoint) c = c < 0 ? -((-c) >> al) : c >> al;
            if (c == 0) { ++run; continue; }
            while (run >= 16u) { emit(zrl & 0xFFFFu, zrl >> 16); run -= 16u; }
            const uint32_t nb = mcu_size(c), t = tab[((run << 4) | nb) & 0xFFu];
            emit(((t & 0xFFFFu) << nb) | mcu_amp(c, nb), (t >> 16) + nb);
            run = 0u;
        }
    }
    // coefficient se itself, of the last group's words (`run` also counts the zeros masked behind se)
    const int i = se & 7;
    const uint32_t w = (i & 4) ? ((i & 2) ? v.w : v.z) : ((i & 2) ? v.y : v.x);
    bool end_zero = (((i & 1) ? w >> 16 : w) & 0xFFFFu) == 0u;
    if constexpr (kPoint) { const int c = (int)(short)(((i & 1) ? w >> 16 : w) & 0xFFFFu); end_zero = ((c < 0 ? -c : c) >> al) == 0; }
    if (!kRuns && end_zero) emit(eob & 0xFFFFu, eob >> 16);
    return end_zero;
}

// ---- the walks of successive approximation (T.81 G.1.2.1 and G.1.2.3 as libjpeg carries them out) ------------------
// A walk has two outlets: emit(code word with the bits that belong to it, count) for what a Huffman table codes -- the counting
// kernel sees these alone, through McuSymbolTab -- and raw(bits, count <= 32) for correction bits and the DC refinement bit.
// The first DC scan: the difference of DC >> al (an arithmetic shift) to the shifted DC in front.
template <class Tab, class Emit>
__device__ __forceinline__ void mcu_walk_dc_point(const uint4 *__restrict__ p, int pred, int al, const Tab &tab, Emit &&emit) {
    const int diff = ((int)*reinterpret_cast<const int16_t *>(p) >> al) - (pred >> al);
    const uint32_t nb = mcu_size(diff), t = tab[256u + (nb & 15u)];
    emit(((t & 0xFFFFu) << nb) | mcu_amp(diff, nb), (t >> 16) + nb);
}
// The DC refinement scan: bit al of the DC, no table.
template <class Raw>
__device__ __forceinline__ void mcu_walk_dc_refine(const uint4 *__restrict__ p, int al, Raw &&raw) {
    raw(((uint32_t)(int)*reinterpret_cast<const int16_t *>(p) >> al) & 1u, 1u);
}

// `n` <= 64 bits, right-aligned in `bits`, through an outlet that takes at most 32 a call.
template <class Raw>
__device__ __forceinline__ void mcu_raw64(unsigned long long bits, uint32_t n, Raw &&raw) {
    if (n > 32u) { raw((uint32_t)(bits >> 32) & (0xFFFFFFFFu >> (64u - n)), n - 32u); raw((uint32_t)bits, 32u); }
    else if (n) raw((uint32_t)bits & (0xFFFFFFFFu >> (32u - n)), n);
}

// An AC refinement scan of the band ss .. se that codes bit al: a[k] = |c[k]| >> al, a coefficient is NEW if a = 1, OLD if a > 1.
// The block's string is head, the symbol of the run it starts (`run` blocks: the caller knows it in its second pass, 0 for none and
// in a pass that only measures -- the symbol's place does not change a length), tail.  Head, k = ss .. K (the last new k): r counts
// zeros, B collects the bits a & 1 of old coefficients; at every non-zero coefficient, while r > 15: ZRL, B; an old coefficient adds
// its bit to B; a new one codes (r << 4) | 1, its sign bit (1: positive) and B.  Tail: the bits of the old coefficients behind K.
// The data: 64-bit masks of new, old and value bits (sign of a new, a & 1 of an old coefficient) built from the band's 16-byte groups,
// walked with ctz; B and the tail are a 64-bit register each (at most 63 bits), no scratch.
// Returns bit 0: E, a[se] != 1 -- bit 1: Z, the band has no new coefficient.
template <class Tab, class Emit, class Raw>
__device__ __forceinline__ uint32_t mcu_walk_band_refine(const uint4 *__restrict__ p, int ss, int se, int al, uint32_t run, const Tab &tab, Emit &&emit, Raw &&raw) {
    unsigned long long newm = 0ull, oldm = 0ull, valm = 0ull;
    const int q1 = se >> 3;
#pragma unroll 1
    for (int q = ss >> 3; q <= q1; ++q) {
        const uint4 v = p[q];
        if ((v.x | v.y | v.z | v.w) == 0u) continue;
        const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
        uint32_t n8 = 0, o8 = 0, v8 = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int c = (int)(short)((w4[i >> 1] >> (16 * (i & 1))) & 0xFFFFu);
            const uint32_t a = (uint32_t)(c < 0 ? -c : c) >> al;
            n8 |= (a == 1u ? 1u : 0u) << i;
            o8 |= (a > 1u ? 1u : 0u) << i;
            v8 |= (a == 1u ? (c > 0 ? 1u : 0u) : (a & 1u)) << i;
        }
        newm |= (unsigned long long)n8 << (8 * q); oldm |= (unsigned long long)o8 << (8 * q); valm |= (unsigned long long)v8 << (8 * q);
    }
    const unsigned long long band = (~0ull << ss) & (~0ull >> (63 - se));
    newm &= band; oldm &= band;
    const uint32_t flags = (((newm >> se) & 1ull) ? 0u : 1u) | (newm ? 0u : 2u);
    const unsigned long long head = newm ? ~0ull >> __builtin_clzll(newm) : 0ull;     // bits 0 .. K
    const uint32_t zrl = tab[0xF0];
    unsigned long long m = (newm | oldm) & head, b = 0ull;
    uint32_t r = 0u, nb = 0u;
    int prev = ss - 1;
    while (m) {
        const int k = __builtin_ctzll(m);
        m &= m - 1ull;
        r += (uint32_t)(k - prev - 1); prev = k;                     // (everything between two non-zero coefficients is zero)
        while (r > 15u) { emit(zrl & 0xFFFFu, zrl >> 16); mcu_raw64(b, nb, raw); b = 0ull; nb = 0u; r -= 16u; }
        const uint32_t bit = (uint32_t)(valm >> k) & 1u;
        if ((oldm >> k) & 1ull) { b = (b << 1) | bit; ++nb; continue; }
        const uint32_t t = tab[((r << 4) | 1u) & 0xFFu];
        emit(((t & 0xFFFFu) << 1) | bit, (t >> 16) + 1u);
        mcu_raw64(b, nb, raw); b = 0ull; nb = 0u; r = 0u;
    }
    if (run) {
        const uint32_t n = 31u - (uint32_t)__clz((int)run), t = tab[n << 4];
        emit(((t & 0xFFFFu) << n) | (run - (1u << n)), (t >> 16) + n);
    }
    m = oldm & ~head;
    nb = (uint32_t)__popcll(m);
    b = 0ull;
    while (m) { const int k = __builtin_ctzll(m); m &= m - 1ull; b = (b << 1) | ((valm >> k) & 1ull); }
    mcu_raw64(b, nb, raw);
    return flags;
}

// what a coder launch codes of a block: all of it, its DC, a band of its AC, a band of its AC with end-of-band runs; with successive
// approximation: its DC by a point transform, one bit of its DC, a band by a point transform (with runs), one bit of a band (with runs)
constexpr int kWalkBlock = 0, kWalkDc = 1, kWalkBand = 2, kWalkBandRuns = 3, kWalkDcPoint = 4, kWalkDcRefine = 5, kWalkBandPoint = 6, kWalkBandRefine = 7;
constexpr bool mcu_walk_has_runs(int walk) { return walk == kWalkBandRuns || walk == kWalkBandPoint || walk == kWalkBandRefine; }

// A table that gives symbol i the 1-bit code word i: a walk over it emits (symbol << size | amplitude, 1 + size) -- the symbol
// itself is what the counting kernel takes from it, so the walks that count are the walks that code.
struct McuSymbolTab { __device__ __forceinline__ uint32_t operator[](uint32_t i) const { return (1u << 16) | i; } };

// End-of-band runs of one segment.  The lane holds the segment's blocks lane + 64 r; z[r]: the
// band of that block is all zero, e[r]: its coefficient se is zero (both false behind the segment's last block).  Block k starts a
// run iff e[k] and not (z[k] and k > 0 and e[k - 1]); the run is 1 + the blocks behind it with z, up to the segment's end: a run
// never leaves its segment, so nothing is read from a neighbour and nothing is pending at the end.  run[r]: 1 .. 256, 0 for none.
__device__ __forceinline__ void mcu_band_runs(int lane, const bool (&z)[4], const bool (&e)[4], uint32_t (&run)[4]) {
    unsigned long long zm[4], em[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { zm[r] = __ballot(z[r]); em[r] = __ballot(e[r]); }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const bool e_prev = lane > 0 ? ((em[r] >> (lane - 1)) & 1ull) != 0ull : (r > 0 && (em[r > 0 ? r - 1 : 0] >> 63) != 0ull);
        run[r] = 0u;
        if (!e[r] || (z[r] && e_prev)) continue;                   // (block 0 of the segment has no e_prev: it starts a run whenever e)
        uint32_t n = 1u;
        bool go = true;
#pragma unroll
        for (int w = r; w < 4; ++w) {                              // the set bits of z from block 64 r + lane + 1 on
            const int bit = w == r ? lane + 1 : 0;
            if (!go || bit > 63) continue;
            const unsigned long long inv = ~(zm[w] >> bit);
            const uint32_t avail = 64u - (uint32_t)bit, c = min(inv ? (uint32_t)__builtin_ctzll(inv) : 64u, avail);
            n += c;
            go = c == avail;
        }
        run[r] = n;
    }
}

struct McuBlock { const uint4 *p; int pred; bool pad, chroma; };

// Block j of MCU m of a picture whose planes start at `base`: where its coefficients lie, and its DC predictor -- 0 where the
// component's previous block lies in front of MCU `mstart` (the scan's first MCU, or the first of m's restart interval).
// kComps = 1 (a scan of ONE component): the MCU is one block, block m of the plane in raster order -- no pad
// blocks, no chroma.
template <int kComps>
__device__ __forceinline__ McuBlock mcu_block(const McuSegArgs &a, const int16_t *base, int m, int j, int mstart) {
    McuBlock b;
    if (kComps == 1) {
        b.chroma = false; b.pad = false;
        b.p = reinterpret_cast<const uint4 *>(base + (size_t)m * 64);
        b.pred = m > mstart ? (int)base[(size_t)(m - 1) * 64] : 0;
        return b;
    }
    // kComps = 2 (the DC scan of two interleaved components, a.mask): the three-component MCU without the
    // component that is not in the scan -- Y's blocks, pad blocks and predictors as they are, a chroma component its one block.
    const int ny = kComps == 2 && !(a.mask & 1) ? 0 : a.hs * a.vs;
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
        b.pred = j > 0 ? (int)*y_at(m, j - 1, nullptr) : (m > mstart ? (int)*y_at(m - 1, ny - 1, nullptr) : 0);
    } else {
        const bool cb = kComps == 2 ? (a.mask == 6 ? j == 0 : (a.mask & 2) != 0) : j == ny;
        const int16_t *plane = base + (cb ? a.cb_off : a.cr_off);
        b.chroma = kComps == 2 ? ny != 0 : true; b.pad = false;       // (the table class: {Cb, Cr} code with the scan's one table)
        b.p = reinterpret_cast<const uint4 *>(plane + (size_t)m * 64);
        b.pred = m > mstart ? (int)plane[(size_t)(m - 1) * 64] : 0;
    }
    return b;
}

// kRestart: the segments are cut per restart interval (McuSegArgs::restart > 0) and the predictors restart with it; the plain
// scan is the instantiation it always was.
// Segment sl of a picture: its first MCU, the first MCU of its interval (of the scan), its MCUs -- none: an EMPTY segment that rounds
// the picture's count up, or lies behind the last MCU of the last interval.
struct McuRange { int m0, mstart, nmcu; };
template <bool kRestart>
__device__ __forceinline__ McuRange mcu_range(const McuSegArgs &a, int sl) {
    McuRange r = {sl * a.seg_mcus, 0, 0};
    r.nmcu = min(a.seg_mcus, a.mx * a.my - r.m0);
    if (kRestart) {                                                // segment (iv, k): the k-th run of seg_mcus MCUs of interval iv
        const int iv = sl / a.segs_per_interval, k = sl - iv * a.segs_per_interval;
        r.mstart = iv * a.restart;
        r.m0 = r.mstart + k * a.seg_mcus;
        r.nmcu = min(min(a.seg_mcus, a.restart - k * a.seg_mcus), a.mx * a.my - r.m0);
    }
    if (sl >= a.num_segs || r.nmcu < 0) r.nmcu = 0;
    return r;
}

// Returns bit 0: E, the block may start or join a run (a walk with runs alone: coefficient se is zero -- of a refinement scan: not
// new); bit 1: Z, of a refinement scan alone (the others' Z is "nothing emitted").  raw, run: mcu_walk_band_refine's.
template <int kWalk, class Tab, class Emit, class Raw>
__device__ __forceinline__ uint32_t mcu_walk(const McuSegArgs &a, const McuBlock &b, int pred, const Tab &tab, Emit &&emit, Raw &&raw, [[maybe_unused]] uint32_t run = 0u) {
    if constexpr (kWalk == kWalkDc) mcu_walk_dc(b.p, pred, tab, emit);
    else if constexpr (kWalk == kWalkBand) mcu_walk_band(b.p, a.ss, a.se, tab, emit);
    else if constexpr (kWalk == kWalkBandRuns) return mcu_walk_band<true>(b.p, a.ss, a.se, tab, emit) ? 1u : 0u;
    else if constexpr (kWalk == kWalkDcPoint) mcu_walk_dc_point(b.p, pred, (int)a.al, tab, emit);
    else if constexpr (kWalk == kWalkDcRefine) mcu_walk_dc_refine(b.p, (int)a.al, raw);
    else if constexpr (kWalk == kWalkBandPoint) return mcu_walk_band<true, true>(b.p, a.ss, a.se, tab, emit, (int)a.al) ? 1u : 0u;
    else if constexpr (kWalk == kWalkBandRefine) return mcu_walk_band_refine(b.p, a.ss, a.se, (int)a.al, run, tab, emit, raw);
    else mcu_walk_block(b.p, b.pad, pred, tab, emit);
    return 0u;
}

// The symbol of a run of `run` blocks: EOBn, n = floor(log2 run), followed by the n low bits of run - 2^n.
__device__ __forceinline__ uint32_t mcu_run_log2(uint32_t run) { return 31u - (uint32_t)__clz((int)run); }

// The segment coder, shared by k_mcu_segments (kWalkBlock) and k_mcu_band_segments (a progressive file's scans): s_tab and s_win are
// the kernel's LDS.  A band launch also adds every segment's bits and symbols to its picture's pair in a.sums (the scans of a
// file share one set of segment arrays, so the sums are taken as the segments are made).
template <bool kRestart, int kComps, int kWalk>
__device__ __forceinline__ void mcu_code_segments(const McuSegArgs &a, uint32_t (*s_tab)[272], uint32_t (*s_win)[kMcuWin + 2]) {
    constexpr int kTabs = kComps == 1 ? 1 : 2;                     // one component: its two tables alone
    constexpr bool kRuns = mcu_walk_has_runs(kWalk);
    const int lane = lane_id(), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    {   // the tables of the workgroup's picture (its four segments are one picture's: num_segs_pad is a multiple of kWavesM)
        const size_t toff = a.huff_stride ? (size_t)(((int)blockIdx.x * kWavesM) / a.num_segs_pad) * a.huff_stride : 0;
        for (int i = (int)threadIdx.x; i < kTabs * 272; i += 64 * kWavesM) s_tab[i / 272][i % 272] = ((i < 272 ? a.huff_y : a.huff_c) + toff)[i % 272];
    }
    __syncthreads();                                               // (the only workgroup-wide meeting: every wave is on its own below)
    const int seg = (int)blockIdx.x * kWavesM + wave;
    if (seg >= a.batch * a.num_segs_pad) return;
    const int image = seg / a.num_segs_pad, sl = seg - image * a.num_segs_pad;
    uint16_t *const ffin = a.seg.ffin + (size_t)seg * 8;
    const McuRange rg = mcu_range<kRestart>(a, sl);
    const int m0 = rg.m0, mstart = rg.mstart, nmcu = rg.nmcu;
    if (nmcu == 0) {                                               // an EMPTY segment: no bits, no ones at either end
        if (lane < 8) ffin[lane] = 0;
        if (lane == 0) { a.seg.bits[seg] = 0u; a.seg.edge[seg] = 0u; a.seg.syms[seg] = 0u; a.seg.exact[seg] = 0u; }
        return;
    }
    const int16_t *base = a.coef + (size_t)image * a.pic_stride;
    const int bpm = kComps == 1 ? 1 : (kComps == 2 ? mcu_blocks_per_mcu2(a.hs, a.vs, a.mask) : a.hs * a.vs + 2);
    const int nblk = nmcu * bpm;                                    // 3 .. 256 (two components: 2 .. 256, one: 1 .. 256)
    uint32_t *win = s_win[wave];

    // ---- pass 1: bit lengths, then the blocks' places ----
    uint32_t len[4], off[4], nsym = 0, carry = 0;
    int pred[4];
    [[maybe_unused]] bool z[4], e[4];
    [[maybe_unused]] uint32_t run[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int k = r * 64 + lane;
        len[r] = 0u; pred[r] = 0;
        if constexpr (kRuns) z[r] = e[r] = false;
        if (k < nblk) {
            const int mi = k / bpm;
            const McuBlock b = mcu_block<kComps>(a, base, m0 + mi, k - mi * bpm, mstart);
            pred[r] = b.pred;
            uint32_t n = 0;
            const uint32_t flags = mcu_walk<kWalk>(a, b, b.pred, (const uint32_t *)s_tab[kTabs > 1 && b.chroma ? 1 : 0], [&](uint32_t, uint32_t c) { n += c; ++nsym; },
                                                   [&](uint32_t, uint32_t c) { n += c; });
            len[r] = n;
            // (every code word has a bit: no symbols, no bits -- but a Z block of a refinement scan has its correction bits: the walk says)
            if constexpr (kRuns) { z[r] = kWalk == kWalkBandRefine ? (flags & 2u) != 0u : n == 0u; e[r] = (flags & 1u) != 0u; }
        }
    }
    if constexpr (kRuns) {                                         // the runs the lane's blocks start: their symbols behind the blocks' own (a refinement scan: behind their heads)
        mcu_band_runs(lane, z, e, run);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (run[r]) { const uint32_t n = mcu_run_log2(run[r]); len[r] += (s_tab[0][n << 4] >> 16) + n; ++nsym; }
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
                const McuBlock b = mcu_block<kComps>(a, base, m0 + mi, k - mi * bpm, mstart);
                uint32_t pos = off[r];
                const auto put = [&](uint32_t sym, uint32_t n) {
                    if (n == 0u) return;
                    const unsigned long long s64 = ((unsigned long long)sym << (64u - n)) >> (pos & 31u);   // left-aligned at the bit's place in a word pair
                    const uint32_t j = (pos >> 5) - wbase;          // (wraps for a word in front of the window)
                    const uint32_t hi = (uint32_t)(s64 >> 32), lo = (uint32_t)s64;
                    if (j <= (uint32_t)kMcuWin && hi) atomicOr(&win[j], hi);
                    if (j + 1u <= (uint32_t)kMcuWin && lo) atomicOr(&win[j + 1u], lo);
                    pos += n;
                };
                if constexpr (kWalk == kWalkBandRefine) mcu_walk<kWalk>(a, b, pred[r], (const uint32_t *)s_tab[0], put, put, run[r]);     // (the run's symbol between head and tail)
                else mcu_walk<kWalk>(a, b, pred[r], (const uint32_t *)s_tab[kTabs > 1 && b.chroma ? 1 : 0], put, put);
                if constexpr (kRuns && kWalk != kWalkBandRefine)
                    if (run[r]) {
                        const uint32_t n = mcu_run_log2(run[r]), t = s_tab[0][n << 4];
                        put(((t & 0xFFFFu) << n) | (run[r] - (1u << n)), (t >> 16) + n);
                    }
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
            // first 8 bits | last 7 bits.  With the Annex K tables a three-component segment is never shorter than 14 bits; with a
            // picture's own tables, or one component, an interval's (the scan's) last segment may be shorter than 8 -- one block of one
            // component is 6 bits with the Annex K tables and as little as 2 with its own: its bits then stand at the left of the 8 and
            // at the right of the 7, zeros elsewhere (the window's; p = seg_bits, tail_last = 0 above).  The readers that take that into
            // account: mcu_tail7, fin_owned_ff; rst_tail and the writer's `lead` bits read what mcu_tail7 and a FULL segment in front give.
            a.seg.edge[seg] = ((first_word >> 24) << 8) | (tail & 0x7Fu);
            a.seg.bits[seg] = seg_bits;
            a.seg.syms[seg] = seg_syms;
            a.seg.exact[seg] = 0u;                                  // (the exact-order fallbacks are counted from the tile records: k_picture_stats)
            if constexpr (kWalk != kWalkBlock) {
                atomicAdd(a.sums + 2 * (size_t)image, (unsigned long long)seg_bits);
                atomicAdd(a.sums + 2 * (size_t)image + 1, (unsigned long long)seg_syms);
            }
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

template <bool kRestart, int kComps>
__global__ __launch_bounds__(64 * kWavesM) void k_mcu_segments(const McuSegArgs a) {
    __shared__ uint32_t s_tab[kComps == 1 ? 1 : 2][272];
    __shared__ uint32_t s_win[kWavesM][kMcuWin + 2];
    mcu_code_segments<kRestart, kComps, kWalkBlock>(a, s_tab, s_win);
}

// A scan of a progressive file: k_mcu_segments' segments, window and census over another walk of a block --
// <3, kWalkDc> the DC scan of the three components in MCU order, <1, kWalkBand> the band ss .. se of ONE component's plane.
// <1, kWalkBandRuns> the same band with end-of-band runs inside the segment and the picture's own table.
// No restart intervals.  A band's string is never longer than the whole block's (mcu_walk_band), a DC difference is at most
// 11 + 11 bits (16 + 11 with a table of the picture's own, a band's coefficient then 16 + 10 and a run's symbol 16 + 8 for a zero
// coefficient se: kMaxBlockBitsOptimized): seg_cap_words(kSegTiles) holds every segment, as it holds k_mcu_segments'.
template <int kComps, int kWalk>
__global__ __launch_bounds__(64 * kWavesM) void k_mcu_band_segments(const McuSegArgs a) {
    static_assert(((kComps == 3 || kComps == 2 || kComps == 1) && (kWalk == kWalkDc || kWalk == kWalkDcPoint || kWalk == kWalkDcRefine)) ||
                  (kComps == 1 && (kWalk == kWalkBand || kWalk == kWalkBandRuns || kWalk == kWalkBandPoint || kWalk == kWalkBandRefine)),
                  "the scans of DESIGN.md 4.6.12 .. 4.6.15");
    static_assert(22 <= kMaxBlockBitsColor && 63 * 27 <= kMaxBlockBitsColor, "a block of either walk fits the reservation of a whole block");
    // successive approximation: a point transform only shortens amplitudes; a refinement block is kMaxBlockBitsRefine, the DC bit 1
    static_assert(kMaxBlockBitsRefine <= kMaxBlockBitsOptimized && kMaxBlockBitsOptimized <= kMaxBlockBitsColor, "one block's string in any single scan fits the segment's reservation");
    __shared__ uint32_t s_tab[kComps == 1 ? 1 : 2][272];
    __shared__ uint32_t s_win[kWavesM][kMcuWin + 2];
    mcu_code_segments<false, kComps, kWalk>(a, s_tab, s_win);
}

// What both walks of the coefficients need of their arguments: every MCU lies in a segment, and the widest segment fits its reservation.
// A scan of one component (comps = 1): the MCU grid is the block grid, and a segment is kSegBlocks blocks.
static bool mcu_seg_args_ok(const McuSegArgs &a) {
    if (a.comps != 1 && a.comps != 2 && a.comps != 3) return false;
    if (a.comps == 1 && (a.hs != 1 || a.vs != 1 || a.mx != a.bw || a.my != a.bh || a.seg_mcus != kSegBlocks)) return false;
    // two components (a DC scan of a caller's script): two of Y, Cb, Cr; the three-component grid, no restart intervals
    if (a.comps == 2 && ((a.mask != 3 && a.mask != 5 && a.mask != 6) || a.restart != 0 || a.hs < 1 || a.hs > 2 || a.vs < 1 || a.vs > 2)) return false;
    const int bpm = a.comps == 2 ? mcu_blocks_per_mcu2(a.hs, a.vs, a.mask) : mcu_blocks_per_mcu(a.hs, a.vs, a.comps);
    if (a.seg_mcus < 1 || a.seg_mcus * bpm > kSegBlocks || a.num_segs_pad % kSegGroup != 0 || a.num_segs > a.num_segs_pad)
        return false;
    static_assert(kSegGroup % kWavesM == 0, "a workgroup's segments belong to one picture");
    const int64_t mcus = (int64_t)a.mx * a.my;
    if (a.restart == 0) return (int64_t)a.num_segs * a.seg_mcus >= mcus;
    const int64_t spi = a.segs_per_interval, in_interval = std::min<int64_t>(a.restart, mcus);
    return !(a.restart < 0 || spi < 1 || spi * a.seg_mcus < in_interval || (int64_t)a.num_segs < (mcus + a.restart - 1) / a.restart * spi ||
             (int64_t)mcu_restart_cap_words((int)std::min<int64_t>(a.restart, a.seg_mcus) * bpm) > (int64_t)a.seg.words_stride);
}

int launch_mcu_segments(const McuSegArgs &a, void *stream) {
    const int n = a.batch * a.num_segs_pad;
    if (n <= 0) return 0;
    if (a.comps == 2 || !mcu_seg_args_ok(a)) return (int)hipErrorInvalidValue;    // (two components: a progressive DC scan alone)
    const dim3 grid((unsigned)((n + kWavesM - 1) / kWavesM)), block(64 * kWavesM);
    const auto kernel = a.comps == 1 ? (a.restart == 0 ? k_mcu_segments<false, 1> : k_mcu_segments<true, 1>)
                                     : (a.restart == 0 ? k_mcu_segments<false, 3> : k_mcu_segments<true, 3>);
    hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

// A scan of a progressive file: three components and ss = se = 0 the DC scan, one component and 1 <= ss <= se <= 63 an AC band.
// A caller's script also has DC scans of one component and of two (McuSegArgs::mask): instantiations of their
// own -- the ones above are launched for what they always were --, with the pictures' own tables alone.
int launch_mcu_band_segments(const McuSegArgs &a, void *stream) {
    const int n = a.batch * a.num_segs_pad;
    if (n <= 0) return 0;
    const bool dc12 = (a.comps == 1 || a.comps == 2) && a.ss == 0 && a.se == 0 && a.runs;
    const bool dc = (a.comps == 3 && a.ss == 0 && a.se == 0) || dc12, band = a.comps == 1 && a.ss >= 1 && a.ss <= a.se && a.se <= 63;
    // (runs: the scans of DESIGN.md 4.6.13 -- every picture codes with its own tables, huff_stride words apart)
    if (!a.sums || a.restart != 0 || (a.huff_stride != 0) != (a.runs != 0) || !(dc || band) || !mcu_seg_args_ok(a)) return (int)hipErrorInvalidValue;
    // successive approximation: own tables alone; a first scan with al > 0, or the refinement of bit al = ah - 1
    const bool point = a.ah == 0 && a.al > 0, refine = a.ah > 0;
    if ((point || refine) && (!a.runs || a.al > 13 || (refine && a.ah != a.al + 1))) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)((n + kWavesM - 1) / kWavesM)), block(64 * kWavesM);
    const auto kernel = a.comps == 2 ? (refine ? k_mcu_band_segments<2, kWalkDcRefine> : (point ? k_mcu_band_segments<2, kWalkDcPoint> : k_mcu_band_segments<2, kWalkDc>))
                        : dc12 ? (refine ? k_mcu_band_segments<1, kWalkDcRefine> : (point ? k_mcu_band_segments<1, kWalkDcPoint> : k_mcu_band_segments<1, kWalkDc>))
                        : dc ? (refine ? k_mcu_band_segments<3, kWalkDcRefine> : (point ? k_mcu_band_segments<3, kWalkDcPoint> : k_mcu_band_segments<3, kWalkDc>))
                           : (refine ? k_mcu_band_segments<1, kWalkBandRefine>
                                     : (point ? k_mcu_band_segments<1, kWalkBandPoint> : (a.runs ? k_mcu_band_segments<1, kWalkBandRuns> : k_mcu_band_segments<1, kWalkBand>)));
    hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

// The symbols of one scan of a file of DESIGN.md 4.6.13 or 4.6.14 counted, not coded: the coder's grid, segments and walks over
// McuSymbolTab, one wave per segment, the workgroup's counts in LDS, then added to its picture's tables in counts [pictures][tables][256]:
// <3, kWalkDc | kWalkDcPoint> the DC sizes of Y into table 0 and of Cb and Cr into table 1, <1, a walk with runs> the band's symbols
// into `table`.  Raw bits (a refinement scan's correction bits) leave the walk through its other outlet and are not seen here.
template <int kComps, int kWalk>
__global__ __launch_bounds__(64 * kWavesM) void k_mcu_band_histogram(const McuSegArgs a, unsigned long long *__restrict__ counts, int table, int tables) {
    static_assert(kComps >= 1 && kComps <= 3 && (kWalk == kWalkDc || kWalk == kWalkDcPoint || (kComps == 1 && mcu_walk_has_runs(kWalk))), "the scans of DESIGN.md 4.6.13 .. 4.6.15 that have a table");
    constexpr int kTabs = kComps == 1 ? 1 : 2;
    constexpr bool kRuns = mcu_walk_has_runs(kWalk);
    __shared__ uint32_t s_cnt[kTabs][256];                         // (a workgroup walks at most 4 x 256 blocks of 64 symbols: 32 bits hold it)
    const int lane = lane_id(), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int i = (int)threadIdx.x; i < kTabs * 256; i += 64 * kWavesM) (&s_cnt[0][0])[i] = 0u;
    __syncthreads();
    const int seg = (int)blockIdx.x * kWavesM + wave;
    const int image = ((int)blockIdx.x * kWavesM) / a.num_segs_pad; // the workgroup's picture
    if (seg < a.batch * a.num_segs_pad) {
        const McuRange rg = mcu_range<false>(a, seg - image * a.num_segs_pad);
        const int16_t *base = a.coef + (size_t)image * a.pic_stride;
        const int bpm = kComps == 1 ? 1 : (kComps == 2 ? mcu_blocks_per_mcu2(a.hs, a.vs, a.mask) : a.hs * a.vs + 2), nblk = rg.nmcu * bpm;      // 0 (EMPTY: nothing counted) .. 256
        [[maybe_unused]] bool z[4], e[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = r * 64 + lane;
            if constexpr (kRuns) z[r] = e[r] = false;
            if (k < nblk) {
                const int mi = k / bpm;
                const McuBlock b = mcu_block<kComps>(a, base, rg.m0 + mi, k - mi * bpm, rg.mstart);
                uint32_t *const cnt = s_cnt[kTabs > 1 && b.chroma ? 1 : 0];
                uint32_t n = 0;
                const uint32_t flags = mcu_walk<kWalk>(a, b, b.pred, McuSymbolTab(), [&](uint32_t v, uint32_t c) {
                    atomicAdd(&cnt[(v >> (c - 1u)) & 0xFFu], 1u);  // (a DC size s arrives as 256 + s)
                    ++n;
                }, [](uint32_t, uint32_t) {});
                if constexpr (kRuns) { z[r] = kWalk == kWalkBandRefine ? (flags & 2u) != 0u : n == 0u; e[r] = (flags & 1u) != 0u; }
            }
        }
        if constexpr (kRuns) {
            uint32_t run[4];
            mcu_band_runs(lane, z, e, run);
#pragma unroll
            for (int r = 0; r < 4; ++r) if (run[r]) atomicAdd(&s_cnt[0][mcu_run_log2(run[r]) << 4], 1u);
        }
    }
    __syncthreads();
    if (image < a.batch)
        for (int i = (int)threadIdx.x; i < kTabs * 256; i += 64 * kWavesM) {
            const uint32_t v = (&s_cnt[0][0])[i];
            if (v) atomicAdd(&counts[((size_t)image * (size_t)tables + (size_t)(table + (i >> 8))) * 256 + (size_t)(i & 255)], (unsigned long long)v);
        }
}

// `tables`: the tables of a picture in `counts` (the script's); a DC scan with Y and chroma counts into `table` and `table` + 1.
int launch_mcu_band_histogram(const McuSegArgs &a, unsigned long long *counts, int table, int tables, void *stream) {
    const int n = a.batch * a.num_segs_pad;
    if (n <= 0) return 0;
    // a DC scan counts into as many tables as its components have classes: Y one, Cb and Cr one together
    const int dc_tables = a.comps == 3 || (a.comps == 2 && (a.mask & 1)) ? 2 : 1;
    const bool dc = a.comps >= 1 && a.comps <= 3 && a.ss == 0 && a.se == 0 && table >= 0 && table + dc_tables <= tables && a.ah == 0;
    const bool band = a.comps == 1 && a.ss >= 1 && a.ss <= a.se && a.se <= 63 && table >= 1 && table < tables;
    const bool point = a.ah == 0 && a.al > 0, refine = a.ah > 0;
    if (!counts || a.restart != 0 || !(dc || band) || tables > kProgTablesMax || a.al > 13 || (refine && a.ah != a.al + 1) || !mcu_seg_args_ok(a)) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)((n + kWavesM - 1) / kWavesM)), block(64 * kWavesM);
    const auto kernel = dc && a.comps == 2 ? (point ? k_mcu_band_histogram<2, kWalkDcPoint> : k_mcu_band_histogram<2, kWalkDc>)
                        : dc && a.comps == 1 ? (point ? k_mcu_band_histogram<1, kWalkDcPoint> : k_mcu_band_histogram<1, kWalkDc>)
                        : dc ? (point ? k_mcu_band_histogram<3, kWalkDcPoint> : k_mcu_band_histogram<3, kWalkDc>)
                           : (refine ? k_mcu_band_histogram<1, kWalkBandRefine> : (point ? k_mcu_band_histogram<1, kWalkBandPoint> : k_mcu_band_histogram<1, kWalkBandRuns>));
    hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)stream, a, counts, table, tables);
    return (int)hipGetLastError();
}

// Workgroup q: picture q of the launch; wave t: its table t in the file's order (Y DC, chroma DC, then the AC tables of the scans
// 2 .. 7), as k_huff_optimal left it in res (BITS, the number of HUFFVAL bytes, HUFFVAL).  The wave writes the coder's table --
// [272] words at tabs + (q kProgTables + t) 272: an AC table's code words by run/size at 0, a DC table's by size at 256, unused
// symbols 0 -- and the table's DHT segment into its scan's header slot: scan 1's is the file's head (hdr[0, head_len)), the two DC
// tables and the DC scan's SOS (hdr[sos_off, sos_off + kMcuSosLen)); scan k's (from 0) its table and sos + 16 k.
// The script is the launch's: a.tables waves, table t belongs to scan a.table_scan[t] and is written with the
// Tc/Th byte a.table_id[t]; the tables of a scan are consecutive, its header is [the head,] their DHT segments in that order and
// its SOS (a.sos + 16 k, a.sos_len[k] bytes), written by the scan's last table.  A caller's script (4.6.15): 1 .. 16 tables and
// scans; scan 0 owns table 0 and, when it has two, table 1; any other scan may own two tables as well.  A scan without a table (bit k of a.bare) gets a
// header of its SOS alone, from wave 0.
constexpr int kMcuSosLen = 14;
__global__ __launch_bounds__(64 * kProgTablesMax) void k_prog_tables(const ProgTablesArgs a) {
    __shared__ uint32_t s_nvals[kProgTablesMax];
    const int lane = lane_id(), t = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), q = (int)blockIdx.x;   // (64 a.tables threads: every wave has a table)
    const int ntab = a.tables;
    const bool dc_table = (a.table_id[t] & 0x10) == 0;
    const uint8_t *res = a.res + ((size_t)q * ntab + (size_t)t) * kHuffResBytes;
    const uint32_t nvals = min(*reinterpret_cast<const uint32_t *>(res + 16), 256u);
    if (lane == 0) s_nvals[t] = nvals;
    uint32_t first[17], cum[17];                                   // by length: the first code word, the HUFFVAL places up to and with it
    first[0] = cum[0] = 0u;
    uint32_t code = 0;
#pragma unroll
    for (int l = 1; l <= 16; ++l) { const uint32_t n = res[l - 1]; first[l] = code; cum[l] = cum[l - 1] + n; code = (code + n) << 1; }
    uint32_t *const tab = a.tabs + ((size_t)q * ntab + (size_t)t) * 272;
    for (int i = lane; i < 272; i += 64) tab[i] = 0u;
    __syncthreads();                                               // (the zeros are in place before a code word; s_nvals is complete)
    for (uint32_t i = (uint32_t)lane; i < nvals; i += 64u) {
        uint32_t l = 1, f = 0, c0 = 0;
#pragma unroll
        for (int k = 1; k <= 16; ++k) if (cum[k] <= i) l = (uint32_t)k + 1u;
#pragma unroll
        for (int k = 1; k <= 16; ++k) if ((uint32_t)k == l) { f = first[k]; c0 = cum[k - 1]; }
        const uint32_t sym = res[32 + i];
        if (l <= 16u && (!dc_table || sym < 16u)) tab[(dc_table ? 256u : 0u) + sym] = (l << 16) | (f + i - c0);
    }
    const int scan = a.table_scan[t];
    uint32_t at = scan == 0 ? (uint32_t)a.head_len : 0u;
    bool last_of_scan = true;
    for (int u = 0; u < ntab; ++u)
        if ((int)a.table_scan[u] == scan) { if (u < t) at += 21u + s_nvals[u]; if (u > t) last_of_scan = false; }
    {
        uint8_t *const out = a.hdr_out + ((size_t)scan * a.pictures + (size_t)(a.first + q)) * kMcuPrefixSlot;
        const auto put = [&](uint32_t pos, uint8_t v) { if (pos < (uint32_t)kMcuPrefixSlot) out[pos] = v; };
        if (lane == 0) {
            put(at, 0xFF); put(at + 1, 0xC4); put(at + 2, (uint8_t)((19u + nvals) >> 8)); put(at + 3, (uint8_t)(19u + nvals));
            put(at + 4, a.table_id[t]);
        }
        if (lane < 16) put(at + 5 + lane, res[lane]);
        for (uint32_t i = (uint32_t)lane; i < nvals; i += 64u) put(at + 21 + i, res[32 + i]);
        at += 21u + nvals;
        if (t == 0)
            for (int i = lane; i < a.head_len; i += 64) put((uint32_t)i, a.hdr[i]);
        if (last_of_scan) {                                        // the SOS behind the scan's last table, and the slot's length
            const uint8_t *sos = a.sos + 16 * scan;
            const uint32_t nsos = a.sos_len[scan];
            if ((uint32_t)lane < nsos) put(at + (uint32_t)lane, sos[lane]);
            if (lane == 0) a.hdr_len[(size_t)scan * a.pictures + (size_t)(a.first + q)] = min(at + nsos, (uint32_t)kMcuPrefixSlot);
        }
    }
    if (t == 0)
        for (int k = 1; k < a.scans; ++k)
            if ((a.bare >> k) & 1u) {                              // a scan of raw bits: its SOS alone
                const uint32_t nsos = a.sos_len[k];
                if ((uint32_t)lane < nsos) a.hdr_out[((size_t)k * a.pictures + (size_t)(a.first + q)) * kMcuPrefixSlot + (size_t)lane] = a.sos[16 * k + lane];
                if (lane == 0) a.hdr_len[(size_t)k * a.pictures + (size_t)(a.first + q)] = nsos;
            }
}

int launch_prog_tables(const ProgTablesArgs &a, int batch, void *stream) {
    if (batch < 1 || batch > kMaxBatch || !a.res || !a.tabs || !a.hdr_out || !a.hdr_len || !a.hdr || !a.sos || a.head_len < 0 ||
        a.head_len + 2 * 33 + kMcuSosLen > kMcuPrefixSlot || a.first < 0 || a.first + batch > a.pictures || a.tables < 1 ||
        a.tables > kProgTablesMax || a.scans < 1 || a.scans > kProgScansMax || a.table_scan[0] != 0 || (a.bare & 1u))
        return (int)hipErrorInvalidValue;
    for (int t = 0; t < a.tables; ++t)                             // (a scan's tables are consecutive; scan 0 has the DC tables in front of the head's end)
        if (a.table_scan[t] >= a.scans || ((a.bare >> a.table_scan[t]) & 1u) || (t && a.table_scan[t] < a.table_scan[t - 1])) return (int)hipErrorInvalidValue;
    for (int k = 0; k < a.scans; ++k) if (a.sos_len[k] < 1 || a.sos_len[k] > 16) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_prog_tables, dim3((unsigned)batch), dim3(64 * (unsigned)a.tables), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

// Workgroup (bx, p): picture p of the launch.  Every workgroup of a picture derives the same sizes and the same verdict
// (k_append_scans_batch's plan); (0, p) writes the picture's size word and adds its numbers to the context's record.
// A file is scan 1 as k_finalize left it in the caller's buffer -- the prefix in front --, then the scans 2 .. a.scans out of their
// slots, each with its SOS in front and the last with EOI behind it.  Its stuffed bytes follow from its size: every scan is its
// header, its bits rounded up to a byte, and a 0x00 per 0xFF.
constexpr int kConcatWgs = 64;
__global__ __launch_bounds__(256) void k_scans_concat(const ScansConcatArgs a) {
    const int p = (int)blockIdx.y;
    // bit 0 of scan 1's record only says that SOME picture's first scan outgrew out_capacity, which the sizes tell picture by
    // picture; anything else there, and any bit of the slots' record (a slot holds its scan's bound: it cannot overflow), fails
    // every picture, and nothing is copied out of a slot.
    const uint32_t st = a.scan_stats[0].status | a.scan_stats[1].status, hard = (a.scan_stats[0].status & ~1u) | a.scan_stats[1].status;
    uint64_t size[kProgScansMax], total = 0;                       // (a.scans of them: the loops below are unrolled to the maximum, so nothing is indexed at run time)
#pragma unroll
    for (int k = 0; k < kProgScansMax; ++k) { size[k] = k < a.scans ? a.size[k * kMaxBatch + p] : 0ull; total += size[k]; }
    const bool fit = hard == 0u && total <= a.out_capacity;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        unsigned long long bits = 0, syms = 0, bytes = 0, ff = 0;
#pragma unroll
        for (int k = 0; k < kProgScansMax; ++k) {
            if (k >= a.scans) continue;
            const unsigned long long b = a.sums[2 * (k * kMaxBatch + p)];
            bits += b; syms += a.sums[2 * (k * kMaxBatch + p) + 1]; bytes += (b + 7u) / 8u;
            if (a.writer_sums) ff += a.writer_sums[(k * kMaxBatch + p) * kMcuPicSums + 2];
        }
        const unsigned long long *pic = a.pic + (size_t)p * kPicStatWords;
        ScanStats *t = a.stats;
        atomicAdd((unsigned long long *)&t->total_bits, bits);
        atomicAdd((unsigned long long *)&t->total_syms, syms);
        atomicAdd((unsigned long long *)&t->total_exact, pic[2] + pic[5] + pic[8]);
        // the stuffed bytes follow from the size -- or the restart writer counted them (4.6.13: the headers differ from picture to picture)
        atomicAdd((unsigned long long *)&t->total_ff,
                  a.writer_sums ? ff : (unsigned long long)(total - (uint64_t)a.prefix_len - (uint64_t)(a.scans - 1) * kSosBytes - 2u) - bytes);
        *a.out_size[p] = fit ? total : 0ull;
        if (a.last_of_call && p == (int)gridDim.y - 1) t->out_size = fit ? total : 0ull;
        const uint32_t add = st | (fit ? 0u : 1u);
        if (add) atomicOr(&t->status, add);
    }
    if (!fit) return;
    uint8_t *d = a.out[p] + size[0];
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x * 16u;
#pragma unroll
    for (int k = 1; k < kProgScansMax; ++k) {
        if (k >= a.scans) continue;
        const uint64_t n = size[k];
        const uint8_t *src = a.slots + (size_t)p * a.pic_bytes + a.slot_off[k];
        for (uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16u; i < n; i += stride) {
            const uint4 v = *reinterpret_cast<const uint4 *>(src + i);              // (a slot is padded to 16 bytes)
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            const uint64_t m = n - i < 16u ? n - i : 16u;
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if ((uint64_t)j < m) d[i + j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
        }
        d += n;
    }
}

int launch_scans_concat(const ScansConcatArgs &a, void *stream) {
    if (a.batch < 1 || a.batch > kMaxBatch || a.pic_bytes % 16 != 0 || a.scans < 1 || a.scans > kProgScansMax) return (int)hipErrorInvalidValue;
    for (int k = 1; k < a.scans; ++k) if (a.slot_off[k] % 16 != 0) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_scans_concat, dim3(kConcatWgs, (unsigned)a.batch), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

// ---- per-picture optimised Huffman tables ---------------------------------------------------------------------
// The symbols of one block counted, not coded: mcu_walk_block's walk without a table.  count(i): symbol i of the class's [272] layout
// (AC run/size at 0, DC size at 256); the two hot symbols -- DC size 0 and EOB -- go to the caller's registers instead.
template <class Count>
__device__ __forceinline__ void mcu_count_block(const uint4 *__restrict__ p, bool pad, int pred, uint32_t &dc0, uint32_t &eobs, Count &&count) {
    uint4 v = p[0];
    const uint32_t dc = mcu_size((int)(short)(v.x & 0xFFFFu) - pred) & 15u;
    if (dc) count(256u + dc); else ++dc0;
    if (pad) { ++eobs; return; }
    v.x &= 0xFFFF0000u;
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
            while (run >= 16u) { count(0xF0u); run -= 16u; }
            count(((run << 4) | mcu_size(c)) & 0xFFu);
            run = 0u;
        }
    }
    if (run) ++eobs;
}

// k_mcu_segments' grid and segments, one wave per segment: the workgroup's counts in LDS, then added to its picture's.
// Photo-like content codes a handful of symbols nearly all the time, and 64 lanes adding to one LDS address take turns.  So the
// symbols that are hot go to counters of the lane's own: EOB and DC size 0 to registers, the AC symbols of run 0 .. 3 and size
// 1 .. 4 and the other DC sizes to a 16-bit column per lane in LDS (a lane walks at most 4 blocks: no count passes 252) -- plain
// adds, nobody else writes there -- and only the rest to the shared table with atomics.  The columns are summed over the wave at the end.
constexpr int kHotRows = 28;                    // 16 AC symbols (run << 2 | size - 1), then DC sizes 0 .. 11 at 16 + size
__device__ __forceinline__ uint32_t mcu_hot_symbol(int row) { return row < 16 ? (uint32_t)(((row >> 2) << 4) | ((row & 3) + 1)) : 256u + (uint32_t)(row - 16); }
template <bool kRestart, int kComps>
__global__ __launch_bounds__(64 * kWavesM) void k_mcu_histogram(const McuSegArgs a, unsigned long long *__restrict__ counts) {
    __shared__ uint32_t s_cnt[2][272];                             // (a workgroup walks at most 4 x 256 blocks of 64 symbols: 32 bits hold it)
    __shared__ uint16_t s_hot[kWavesM][2][kHotRows][64];
    const int lane = lane_id(), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int i = (int)threadIdx.x; i < 2 * 272; i += 64 * kWavesM) (&s_cnt[0][0])[i] = 0u;
    for (int i = 0; i < 2 * kHotRows; ++i) (&s_hot[wave][0][0][0])[i * 64 + lane] = 0;
    __syncthreads();
    const int seg = (int)blockIdx.x * kWavesM + wave;
    const int image = ((int)blockIdx.x * kWavesM) / a.num_segs_pad; // the workgroup's picture
    if (seg < a.batch * a.num_segs_pad) {
        const McuRange rg = mcu_range<kRestart>(a, seg - image * a.num_segs_pad);
        const int16_t *base = a.coef + (size_t)image * a.pic_stride;
        const int bpm = kComps == 1 ? 1 : a.hs * a.vs + 2, nblk = rg.nmcu * bpm;      // 0 (EMPTY: nothing counted), 3 .. 256 (one component: 1 .. 256)
        uint32_t dc0_y = 0, dc0_c = 0, eob_y = 0, eob_c = 0;
#pragma unroll 1
        for (int r = 0; r < 4; ++r) {
            const int k = r * 64 + lane;
            if (k < nblk) {
                const int mi = k / bpm;
                const McuBlock b = mcu_block<kComps>(a, base, rg.m0 + mi, k - mi * bpm, rg.mstart);
                uint32_t *const cnt = s_cnt[b.chroma ? 1 : 0];
                uint16_t *const hot = &s_hot[wave][b.chroma ? 1 : 0][0][lane];
                uint32_t d = 0, e = 0;
                mcu_count_block(b.p, b.pad, b.pred, d, e, [&](uint32_t i) {
                    const uint32_t run = (i >> 4) & 15u, size = i & 15u;
                    if (i >= 256u && size < 12u) hot[(16u + size) * 64u] += 1;                 // a DC size 1 .. 11
                    else if (i < 256u && run < 4u && size - 1u < 4u) hot[((run << 2) | (size - 1u)) * 64u] += 1;
                    else atomicAdd(&cnt[i], 1u);
                });
                if (b.chroma) { dc0_c += d; eob_c += e; } else { dc0_y += d; eob_y += e; }
            }
        }
        if (nblk) {
            const uint32_t t0 = (uint32_t)wave_sum_i32((int)dc0_y), t1 = (uint32_t)wave_sum_i32((int)eob_y);
            const uint32_t t2 = (uint32_t)wave_sum_i32((int)dc0_c), t3 = (uint32_t)wave_sum_i32((int)eob_c);
            if (lane == 0) {
                if (t0) atomicAdd(&s_cnt[0][256], t0);
                if (t1) atomicAdd(&s_cnt[0][0], t1);
                if (t2) atomicAdd(&s_cnt[1][256], t2);
                if (t3) atomicAdd(&s_cnt[1][0], t3);
            }
#pragma unroll 1
            for (int i = 0; i < 2 * kHotRows; ++i) {
                const uint32_t t = (uint32_t)wave_sum_i32((int)(&s_hot[wave][0][0][0])[i * 64 + lane]);
                if (lane == 0 && t) atomicAdd(&s_cnt[i / kHotRows][mcu_hot_symbol(i % kHotRows)], t);
            }
        }
    }
    __syncthreads();
    if (image < a.batch)
        for (int i = (int)threadIdx.x; i < 2 * 272; i += 64 * kWavesM) {
            const uint32_t v = (&s_cnt[0][0])[i];
            if (v) atomicAdd(&counts[(size_t)image * kMcuTabWords + i], (unsigned long long)v);
        }
}

int launch_mcu_histogram(const McuSegArgs &a, unsigned long long *counts, void *stream) {
    const int n = a.batch * a.num_segs_pad;
    if (n <= 0) return 0;
    if (!counts || !mcu_seg_args_ok(a)) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)((n + kWavesM - 1) / kWavesM)), block(64 * kWavesM);
    const auto kernel = a.comps == 1 ? (a.restart == 0 ? k_mcu_histogram<false, 1> : k_mcu_histogram<true, 1>)
                                     : (a.restart == 0 ? k_mcu_histogram<false, 3> : k_mcu_histogram<true, 3>);
    hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)stream, a, counts);
    return (int)hipGetLastError();
}

// Minimum of a 64-bit value across the wave, in every lane: the DPP steps of wave_max_u32, a lane without a source keeping its own.
template <int kCtrl, int kRowMask>
__device__ __forceinline__ unsigned long long min_dpp_u64(unsigned long long v) {
    const int lo = (int)(uint32_t)v, hi = (int)(uint32_t)(v >> 32);
    const uint32_t olo = (uint32_t)__builtin_amdgcn_update_dpp(lo, lo, kCtrl, kRowMask, 0xF, false);
    const uint32_t ohi = (uint32_t)__builtin_amdgcn_update_dpp(hi, hi, kCtrl, kRowMask, 0xF, false);
    const unsigned long long o = ((unsigned long long)ohi << 32) | olo;
    return o < v ? o : v;
}
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
    v = min_dpp_u64<0x111, 0xF>(v);
    v = min_dpp_u64<0x112, 0xF>(v);
    v = min_dpp_u64<0x114, 0xF>(v);
    v = min_dpp_u64<0x118, 0xF>(v);
    v = min_dpp_u64<0x142, 0xA>(v);
    v = min_dpp_u64<0x143, 0xC>(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, 63), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), 63);
    return ((unsigned long long)hi << 32) | lo;
}

// Wave w of a workgroup: table w of its picture (0 luma DC, 1 luma AC, 2 chroma DC, 3 chroma AC), or job 4 g + w of a debug call.
// A picture of one component has the first two tables alone (HuffOptimalArgs::tables = 2): waves 2 and 3 then have no job.
// The 257 slots of K.2 -- 256 symbols and the reserved point -- lie over the lanes, slot s in lane s & 63: count, tree id (its root's
// slot) and depth.  Only a tree's root has a non-zero count (every other member was a c2 once), so "the root with the least count,
// the highest index among equals" is the minimum of (count << 9 | 511 - slot) over the non-zero counts: one merge is two such
// minima, then every slot of either tree goes one level down and takes c1's id -- what libjpeg's two chain walks do to codesize[].
__global__ __launch_bounds__(256) void k_huff_optimal(const HuffOptimalArgs a) {
    __shared__ uint32_t s_n[4][260];                               // n[l], l = 0 .. 256
    __shared__ __attribute__((aligned(16))) uint32_t s_key[4][256]; // (depth << 8) | symbol of the used symbols, all ones for the rest
    __shared__ uint32_t s_first[4][18], s_cum[4][18];              // by final length: the first code word, the HUFFVAL places in front of and at it
    __shared__ uint8_t s_vals[4][256];
    const int tid = (int)threadIdx.x, lane = lane_id(), w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ntab = a.freq ? 4 : a.tables;                        // jobs of a workgroup
    const int g = (int)blockIdx.x, job = ntab * g + w;
    const bool active = w < ntab && job < a.jobs;
    const int nsym = a.freq ? 256 : ((w & 1) ? 256 : 16);
    const unsigned long long *src = a.freq ? a.freq + (size_t)job * 256 : a.counts + (size_t)g * kMcuTabWords + (size_t)(w >> 1) * 272 + ((w & 1) ? 0 : 256);
    constexpr unsigned long long kNone = ~0ull;
    unsigned long long f[5];
    int tree[5];
    uint32_t depth[5];
    bool used[5];
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        const int s = lane + 64 * r;
        f[r] = r == 4 ? (lane == 0 ? 1ull : 0ull) : ((active && s < nsym) ? src[s] : 0ull);
        tree[r] = s; depth[r] = 0u; used[r] = f[r] != 0ull;
    }
    for (;;) {                                                     // (every value that steers the loop is the same in all lanes)
        unsigned long long m = kNone;
#pragma unroll
        for (int r = 0; r < 5; ++r) if (f[r]) m = min(m, (f[r] << 9) | (unsigned long long)(511 - (lane + 64 * r)));
        const unsigned long long k1 = wave_min_u64(m);
        const int c1 = 511 - (int)(k1 & 511ull);
        m = kNone;
#pragma unroll
        for (int r = 0; r < 5; ++r) if (f[r] && lane + 64 * r != c1) m = min(m, (f[r] << 9) | (unsigned long long)(511 - (lane + 64 * r)));
        const unsigned long long k2 = wave_min_u64(m);
        if (k2 == kNone) break;
        const int c2 = 511 - (int)(k2 & 511ull);
        const unsigned long long sum = (k1 >> 9) + (k2 >> 9);
#pragma unroll
        for (int r = 0; r < 5; ++r) {
            const int s = lane + 64 * r;
            if (s == c1) f[r] = sum;
            if (s == c2) f[r] = 0ull;
            if (tree[r] == c1 || tree[r] == c2) { ++depth[r]; tree[r] = c1; }
        }
    }
    // n[l], then the symbols of lengths beyond 16 moved up (K.2's Adjust_BITS) and the reserved point taken out: one lane, a few steps
    uint32_t *const n = s_n[w];
    for (int i = lane; i < 260; i += 64) n[i] = 0u;
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int r = 0; r < 5; ++r) if (used[r]) atomicAdd(&n[min(depth[r], 256u)], 1u);
#pragma unroll
    for (int r = 0; r < 4; ++r) s_key[w][lane + 64 * r] = used[r] ? (depth[r] << 8) | (uint32_t)(lane + 64 * r) : 0xFFFFFFFFu;
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) {
        int top = 256;
        while (top > 0 && n[top] == 0u) --top;
        for (int l = top; l > 16; --l)
            while (n[l] > 0u) {
                int j = l - 2;
                while (j > 0 && n[j] == 0u) --j;
                if (j <= 0 || n[l] < 2u) { n[l] = 0u; break; }     // (cannot happen for the lengths of a code tree: no index leaves the array)
                n[l] -= 2u; n[l - 1] += 1u; n[j + 1] += 2u; n[j] -= 1u;
            }
        int l = 16;
        while (l > 0 && n[l] == 0u) --l;
        if (l > 0) n[l] -= 1u;
        uint32_t code = 0, cum = 0;
        s_cum[w][0] = 0u; s_first[w][0] = 0u;
        for (l = 1; l <= 16; ++l) {
            s_first[w][l] = code; cum += n[l]; s_cum[w][l] = cum;
            code = (code + n[l]) << 1;
        }
    }
    __builtin_amdgcn_wave_barrier();
    const uint32_t nvals = min(s_cum[w][16], 256u);
    // a used symbol's place in HUFFVAL: the used symbols in front of it by (depth, symbol); its code follows from the place
    uint32_t word[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        word[r] = 0u;
        if (!used[r]) continue;
        const uint32_t mine = (depth[r] << 8) | (uint32_t)(lane + 64 * r);
        uint32_t rank = 0;
        for (int i = 0; i < 64; ++i) {
            const uint4 k = *reinterpret_cast<const uint4 *>(&s_key[w][4 * i]);
            rank += (k.x < mine) + (k.y < mine) + (k.z < mine) + (k.w < mine);
        }
        if (rank >= nvals) continue;
        s_vals[w][rank] = (uint8_t)(lane + 64 * r);
        uint32_t l = 1;
        while (l < 16u && s_cum[w][l] <= rank) ++l;
        word[r] = (l << 16) | (s_first[w][l] + rank - s_cum[w][l - 1]);
    }
    __builtin_amdgcn_wave_barrier();
    if (active && a.res) {
        uint8_t *res = a.res + (size_t)job * kHuffResBytes;
        if (lane < 16) res[lane] = (uint8_t)n[lane + 1];
        if (lane == 16) *reinterpret_cast<uint32_t *>(res + 16) = nvals;
        for (int i = lane; i < 256; i += 64) res[32 + i] = (uint32_t)i < nvals ? s_vals[w][i] : (uint8_t)0;
    }
    if (a.freq) return;                                            // (the same for the whole launch)
    uint32_t *const tab = a.tabs + (size_t)g * kMcuTabWords + (size_t)(w >> 1) * 272 + ((w & 1) ? 0 : 256);
#pragma unroll
    for (int r = 0; r < 4; ++r) if (active && lane + 64 * r < nsym) tab[lane + 64 * r] = word[r];
    __syncthreads();                                               // the tables' sizes place the DHT segments
    uint8_t *const out = a.prefix + (size_t)g * kMcuPrefixSlot;
    uint32_t at = (uint32_t)a.head_len, end = (uint32_t)a.head_len;
    for (int t = 0; t < ntab; ++t) {
        const uint32_t len = 21u + min(s_cum[t][16], 256u);
        if (t < w) at += len;
        end += len;
    }
    const auto put = [&](uint32_t pos, uint8_t v) { if (pos < (uint32_t)kMcuPrefixSlot) out[pos] = v; };   // (a picture of this coder's coefficients never comes near the slot's end)
    if (active && lane == 0) {
        put(at, 0xFF); put(at + 1, 0xC4); put(at + 2, (uint8_t)((19u + nvals) >> 8)); put(at + 3, (uint8_t)(19u + nvals));
        put(at + 4, (uint8_t)(((w & 1) << 4) | (w >> 1)));
    }
    if (active && lane < 16) put(at + 5 + lane, (uint8_t)n[lane + 1]);
    for (uint32_t i = (uint32_t)lane; active && i < nvals; i += 64u) put(at + 21 + i, s_vals[w][i]);
    for (int i = tid; i < a.head_len; i += 256) put((uint32_t)i, a.hdr[i]);
    for (int i = tid; i < a.tail_len; i += 256) put(end + (uint32_t)i, a.hdr[a.tail_off + i]);
    if (tid == 0) a.prefix_len[g] = min(end + (uint32_t)a.tail_len, (uint32_t)kMcuPrefixSlot);
}

int launch_huff_optimal(const HuffOptimalArgs &a, void *stream) {
    if (a.jobs < 1 || (!a.freq) == (!a.counts) || (a.freq && !a.res)) return (int)hipErrorInvalidValue;
    if (a.counts && ((a.tables != 2 && a.tables != 4) || a.jobs % a.tables != 0 || !a.tabs || !a.prefix || !a.prefix_len || !a.hdr || a.head_len < 0 || a.tail_len < 0 || a.tail_off < a.head_len ||
                     a.head_len + a.tail_len > kMcuPrefixSlot))
        return (int)hipErrorInvalidValue;
    const int per_wg = a.freq ? 4 : a.tables;
    hipLaunchKernelGGL(k_huff_optimal, dim3((unsigned)((a.jobs + per_wg - 1) / per_wg)), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

// ---- the writer of a scan with restart intervals ------------------------------------------------------------
// Every interval starts on a byte with its bit offset at 0, so a segment's byte phase is the bits of the segments in front of it
// in ITS interval, and an interval's length in the file follows from its own segments' numbers: where everything goes is one
// exclusive sum per picture over what each segment writes.  Two launches: the sums must be complete before a byte is placed,
// and no workgroup waits for another.
constexpr int kRstThreads = 1024, kRstPer = 8;  // k_mcu_restart_offsets: threads of the workgroup, segments a thread takes per round
constexpr int kRstStripWords = 132;             // k_mcu_restart_write: a wave's staging strip -- 3 bytes kept + 256 bytes of a pass, every one stuffed, + the word read behind them

// What an interval's last segment writes behind its own bytes: the byte that holds the interval's last r = bits & 7 bits (the
// last 7 bits of the segment are in `edge`) -- filled up with ones, and stuffed when that makes it 0xFF, in front of RSTn; filled
// up with zeros in front of EOI -- and the two marker bytes.
struct RstTail { uint32_t r, byte, bytes, pad_ff; };
// The last 7 bits of an interval whose last segment has `bits` bits: that segment's, or -- it is shorter, 1 .. 6 bits (a picture's own
// tables, or one component: one MCU may be 2 bits) -- the bits in front of them from the segment in front, which is a full run of MCUs
// (at least 512 bits) and never that short.  (An interval's first segment has nothing in front: r <= bits there, and the bits taken
// from edge_prev are never looked at.)
__device__ __forceinline__ uint32_t mcu_tail7(uint32_t edge, uint32_t bits, uint32_t edge_prev) {
    return bits >= 7u ? edge & 0x7Fu : (((edge_prev & 0x7Fu) << bits) | (edge & ((1u << bits) - 1u))) & 0x7Fu;
}
__device__ __forceinline__ RstTail rst_tail(uint32_t interval_bits, uint32_t edge /*mcu_tail7*/, bool last_interval) {
    RstTail t;
    t.r = interval_bits & 7u;
    const uint32_t fill = last_interval ? 0u : (0xFFu >> t.r);
    t.byte = t.r ? (((edge & ((1u << t.r) - 1u)) << (8u - t.r)) | fill) : 0u;
    t.pad_ff = (t.r && t.byte == 0xFFu) ? 1u : 0u;
    t.bytes = (t.r ? 1u : 0u) + t.pad_ff + 2u;
    return t;
}

// Exclusive prefix sums over a round's kRstThreads x kRstPer values, v[j] of a lane being the value of element
// 64 kRstPer wave + 64 j + lane of the round; *total: their sum.  s_w: 16 words, free again on return.
__device__ __forceinline__ void rst_round_scan(const uint32_t (&v)[kRstPer], uint32_t (&ex)[kRstPer], uint32_t *s_w, int lane, int wave, uint32_t *total) {
    static_assert(kRstThreads == 16 * 64, "the waves' totals are scanned in one DPP row");
    uint32_t carry = 0;
#pragma unroll
    for (int j = 0; j < kRstPer; ++j) {
        const uint32_t incl = wave_incl_scan_u32(v[j]);
        ex[j] = carry + incl - v[j];
        carry += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    }
    if (lane == 0) s_w[wave] = carry;
    __syncthreads();
    const uint32_t wt = lane < 16 ? s_w[lane] : 0u;
    const uint32_t wincl = half_incl_scan_dpp(wt);
    *total = (uint32_t)__builtin_amdgcn_readlane((int)wincl, 15);
    const uint32_t woff = (uint32_t)__builtin_amdgcn_readlane((int)(wincl - wt), wave);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kRstPer; ++j) ex[j] += woff;
}

// Workgroup q: picture q of the launch, its segments in rounds of kRstThreads x kRstPer with the sums carried from round to round.
// A wave takes 64 kRstPer consecutive segments of the round, lane l the segments l, l + 64, ...: every load is contiguous over the
// lanes, and a lane's loads of a round are all issued before any is used -- a round costs one trip to memory.
__global__ __launch_bounds__(kRstThreads) void k_mcu_restart_offsets(const McuRestartArgs a) {
    __shared__ uint32_t s_w[16];
    __shared__ unsigned long long s_sum[3][16];
    const int tid = (int)threadIdx.x, lane = lane_id(), wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q = (int)blockIdx.x, n = a.num_segs_pad, spi = a.segs_per_interval;
    const size_t base = (size_t)q * (size_t)n;
    const int first = wave * 64 * kRstPer + lane;                    // the lane's first element of a round
    const int last_first = (a.intervals - 1) * spi;                 // the first segment of the last interval
    // 1. Intervals of several segments: the bit counts' running sum over the picture (mod 2^32: only differences inside an interval
    //    are read).  An interval of one segment has its bit offset, 0, without it.
    const bool chained = spi > 1;
    if (chained) {
        uint32_t run = 0;
        for (int c0 = 0; c0 < n; c0 += kRstThreads * kRstPer) {
            uint32_t v[kRstPer], ex[kRstPer], round;
#pragma unroll
            for (int j = 0; j < kRstPer; ++j) { const int i = c0 + first + 64 * j; v[j] = i < n ? a.seg.bits[base + i] : 0u; }
            rst_round_scan(v, ex, s_w, lane, wave, &round);
#pragma unroll
            for (int j = 0; j < kRstPer; ++j) { const int i = c0 + first + 64 * j; if (i < n) a.pre[base + i] = run + ex[j]; }
            run += round;
        }
        __syncthreads();                                            // (the sums are read back by other threads of this workgroup)
    }
    // 2. per segment: bit offset in its interval, owned 0xFF bytes at that phase, bytes written; their sums
    unsigned long long pos = 0, sum_bits = 0, sum_syms = 0, sum_ff = 0;
    for (int c0 = 0; c0 < n; c0 += kRstThreads * kRstPer) {
        uint32_t bits[kRstPer], edge[kRstPer], edge_prev[kRstPer], syms[kRstPer], pre_i[kRstPer], pre_0[kRstPer];
        int k[kRstPer];
        uint4 ffin[kRstPer];
#pragma unroll
        for (int j = 0; j < kRstPer; ++j) {                         // every load of the round (an element behind the last segment reads the last)
            const int i = min(c0 + first + 64 * j, a.last_seg);
            k[j] = i % spi;
            bits[j] = a.seg.bits[base + i]; edge[j] = a.seg.edge[base + i]; syms[j] = a.seg.syms[base + i];
            edge_prev[j] = a.seg.edge[base + (i > 0 ? i - 1 : 0)];
            ffin[j] = *reinterpret_cast<const uint4 *>(a.seg.ffin + (base + i) * 8);
            pre_i[j] = chained ? a.pre[base + i] : 0u;
            pre_0[j] = chained ? a.pre[base + i - k[j]] : 0u;
        }
        uint32_t b0[kRstPer], ff[kRstPer], bytes[kRstPer], ex[kRstPer], round;
#pragma unroll
        for (int j = 0; j < kRstPer; ++j) {
            const int i = c0 + first + 64 * j;
            b0[j] = ff[j] = bytes[j] = 0u;
            if (i <= a.last_seg) {                                  // (behind it: EMPTY segments, which write nothing)
                uint32_t pad_ff = 0;
                b0[j] = pre_i[j] - pre_0[j];
                ff[j] = fin_owned_ff(ffin[j], k[j], b0[j] & 7u, edge[j], edge_prev[j]);
                bytes[j] = ((b0[j] + bits[j]) >> 3) - (b0[j] >> 3) + ff[j];
                const bool last = i == a.last_seg;
                if (last || (k[j] == spi - 1 && i < last_first)) {
                    const RstTail t = rst_tail(b0[j] + bits[j], mcu_tail7(edge[j], bits[j], edge_prev[j]), last);
                    bytes[j] += t.bytes - (last && a.no_eoi ? 2u : 0u); pad_ff = t.pad_ff;
                }
                sum_ff += ff[j] + pad_ff; sum_bits += bits[j]; sum_syms += syms[j];
            }
        }
        rst_round_scan(bytes, ex, s_w, lane, wave, &round);
#pragma unroll
        for (int j = 0; j < kRstPer; ++j) {
            const int i = c0 + first + 64 * j;
            if (i < n) { a.pos[base + i] = pos + ex[j]; a.b0[base + i] = b0[j]; a.ff[base + i] = ff[j]; }
        }
        pos += round;
    }
    for (int off = 32; off > 0; off >>= 1) {
        sum_bits += __shfl_xor(sum_bits, off, 64); sum_syms += __shfl_xor(sum_syms, off, 64); sum_ff += __shfl_xor(sum_ff, off, 64);
    }
    if (lane == 0) { s_sum[0][wave] = sum_bits; s_sum[1][wave] = sum_syms; s_sum[2][wave] = sum_ff; }
    __syncthreads();
    if (tid == 0) {
        sum_bits = sum_syms = sum_ff = 0;
        for (int w = 0; w < 16; ++w) { sum_bits += s_sum[0][w]; sum_syms += s_sum[1][w]; sum_ff += s_sum[2][w]; }
        *a.out_size[q] = (uint64_t)(a.pic_prefix_len ? a.pic_prefix_len[q] : (uint32_t)a.prefix_len) + pos;              // the would-be size: k_mcu_totals makes it 0 when the file did not fit
        unsigned long long *rec = a.pic_sums + (size_t)q * kMcuPicSums;
        rec[0] = sum_bits; rec[1] = sum_syms; rec[2] = sum_ff;
    }
}

// Wave w of workgroup g of a picture: its segment 4 g + w.  An output byte is owned by the segment that holds its last bit
// (k_finalize's rule, inside an interval) and written once: 256 owned bytes a pass, four per lane, go with their stuffing bytes
// into a zeroed strip in LDS whose offset is the output address mod 4, and whole words of the strip leave as aligned stores.
__global__ __launch_bounds__(64 * kWavesM) void k_mcu_restart_write(const McuRestartArgs a) {
    __shared__ uint32_t s_strip[kWavesM][kRstStripWords];
    const int lane = lane_id(), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int wgs = (a.num_segs_pad + kWavesM - 1) / kWavesM;
    const int image = (int)blockIdx.x / wgs, g = (int)blockIdx.x - image * wgs;
    uint8_t *const out = a.out[image];
    const int prefix_len = a.pic_prefix_len ? (int)a.pic_prefix_len[image] : a.prefix_len;   // (a picture with its own tables has its own prefix)
    const uint8_t *const prefix = a.pic_prefix ? a.pic_prefix + (size_t)image * a.pic_prefix_stride : a.prefix;
    if (g == 0)
        for (int i = (int)threadIdx.x; i < prefix_len; i += 64 * kWavesM)
            if ((uint64_t)i < a.out_capacity) out[i] = prefix[i];
    const int sl = g * kWavesM + wave;
    if (sl > a.last_seg) return;                                    // (no workgroup-wide meeting below)
    const size_t seg = (size_t)image * (size_t)a.num_segs_pad + (size_t)sl;
    const int iv = sl / a.segs_per_interval, k = sl - iv * a.segs_per_interval;
    const uint32_t bits = a.seg.bits[seg], edge = a.seg.edge[seg], b0 = a.b0[seg], my_ff = a.ff[seg];
    const uint32_t lead = b0 & 7u;                                  // bits of the segment in front that its first byte begins with (0 for k = 0)
    const uint32_t edge_prev = sl > 0 ? a.seg.edge[seg - 1] : 0u;
    const uint32_t leadbits = lead ? (edge_prev & ((1u << lead) - 1u)) : 0u;   // (lead > 0: the segment in front is a full run of MCUs -- never shorter than 7 bits; this one may be 2)
    const uint32_t nown = ((b0 + bits) >> 3) - (b0 >> 3);
    const bool last = sl == a.last_seg, tail = last || (k == a.segs_per_interval - 1 && iv < a.intervals - 1);
    const RstTail t = rst_tail(b0 + bits, mcu_tail7(edge, bits, edge_prev), last);
    const bool marker = !(last && a.no_eoi);                        // (a scan that another follows is flushed and ends there: no EOI)
    const uint64_t base = (uint64_t)prefix_len + a.pos[seg];
    if (base + nown + my_ff + (tail ? t.bytes - (marker ? 0u : 2u) : 0u) > a.out_capacity) return;    // the file does not fit: k_mcu_totals reports it from the size

    const uint32_t *words = a.seg.words + seg * a.seg.words_stride;
    uint32_t *const strip32 = s_strip[wave];
    uint8_t *const strip = reinterpret_cast<uint8_t *>(strip32);
    for (int p = lane; p < kRstStripWords; p += 64) strip32[p] = 0u;
    uint8_t *const dst = out + base;
    const uint32_t fill0 = (uint32_t)((uintptr_t)dst & 3u);          // the bytes in front of it in the first word belong to the segment in front
    uint8_t *gdst = dst - fill0;                                    // where strip byte 0 goes: 4-byte aligned
    uint32_t fill = fill0;
    bool first = true;
    __builtin_amdgcn_wave_barrier();
    for (uint32_t done = 0; done < nown; done += 256u) {
        const uint32_t j = (done >> 2) + (uint32_t)lane;            // owned bytes 4 j .. 4 j + 3: 32 bits from `lead` bits in front of word j
        uint32_t v = 0;
        const bool have = 4u * j < nown;
        if (have) {
            if (lead) {
                const uint32_t hi = j ? words[j - 1u] : leadbits;
                v = __builtin_amdgcn_alignbit(hi, words[j], lead);
            } else {
                v = words[j];
            }
            const uint32_t nv = nown - 4u * j;
            if (nv < 4u) v &= 0xFFFFFFFFu << (8u * (4u - nv));
        }
        const uint32_t m = ((v & 0x7F7F7F7Fu) + 0x01010101u) & v & 0x80808080u;   // bit 7 of a byte: the byte is 0xFF
        const uint32_t c = (uint32_t)__popc(m);
        const uint32_t incl = wave_incl_scan_u32(c);
        const uint32_t nfill = fill + min(nown - done, 256u) + (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);   // <= 3 + 512
        if (have) {                                                 // a byte goes behind the lane's place + the 0xFF bytes in front of it; the 0x00 is the strip's
            uint32_t at = fill + 4u * (uint32_t)lane + incl - c;
            strip[at] = (uint8_t)(v >> 24); at += 1u + (m >> 31);
            strip[at] = (uint8_t)(v >> 16); at += 1u + ((m >> 23) & 1u);
            strip[at] = (uint8_t)(v >> 8);  at += 1u + ((m >> 15) & 1u);
            strip[at] = (uint8_t)v;
        }
        __builtin_amdgcn_wave_barrier();
        const uint32_t npieces = nfill >> 2;                        // whole words: <= 128
        const uint32_t rest = strip32[npieces];
        for (uint32_t p = (uint32_t)lane; p < npieces; p += 64u) {
            const uint32_t piece = strip32[p];
            if (first && fill0 && p == 0u) {                        // the segment's first word: its own bytes one by one
                for (uint32_t b = fill0; b < 4u; ++b) gdst[b] = (uint8_t)(piece >> (8u * b));
            } else {
                *reinterpret_cast<uint32_t *>(gdst + 4u * p) = piece;
            }
            strip32[p] = 0u;
        }
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) { strip32[npieces] = 0u; strip32[0] = rest; }
        __builtin_amdgcn_wave_barrier();
        gdst += 4u * npieces;
        fill = nfill & 3u;
        first = first && npieces == 0u;
    }
    if ((uint32_t)lane < fill && !(first && (uint32_t)lane < fill0)) gdst[lane] = strip[lane];   // what is left of the last word
    if (tail && lane == 0) {
        uint8_t *e = dst + nown + my_ff;
        if (t.r) { *e++ = (uint8_t)t.byte; if (t.pad_ff) *e++ = 0x00; }
        if (marker) { e[0] = 0xFF; e[1] = last ? 0xD9 : (uint8_t)(0xD0 + (iv & 7)); }
    }
}

int launch_mcu_restart_writer(const McuRestartArgs &a, void *stream) {
    if (a.batch < 1 || a.batch > kMaxBatch || a.num_segs_pad < 1 || a.segs_per_interval < 1 || a.intervals < 1 || a.last_seg < 0 ||
        a.last_seg >= a.num_segs_pad || (int64_t)a.intervals * a.segs_per_interval > (int64_t)a.num_segs_pad ||
        a.last_seg / a.segs_per_interval != a.intervals - 1 || (!a.pic_prefix) != (!a.pic_prefix_len))
        return (int)hipErrorInvalidValue;
    const int wgs = (a.num_segs_pad + kWavesM - 1) / kWavesM;
    hipLaunchKernelGGL(k_mcu_restart_offsets, dim3((unsigned)a.batch), dim3(kRstThreads), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(k_mcu_restart_write, dim3((unsigned)(a.batch * wgs)), dim3(64 * kWavesM), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

// Workgroup q: picture q of the launch.  Sums of its segments' bits and symbols; its stuffed bytes follow from its size (a file is
// its prefix, the scan's bits, the flush byte, a 0x00 per 0xFF, and EOI) unless the writer counted them (restart intervals: markers
// and a padded byte per interval); the size word becomes 0 when the file did not fit.
__global__ __launch_bounds__(256) void k_mcu_totals(const McuTotalsArgs a) {
    __shared__ unsigned long long s_part[2][4];
    const int q = (int)blockIdx.x;
    unsigned long long bits = 0, syms = 0;
    const unsigned long long *sums = a.pic_sums ? a.pic_sums + (size_t)q * kMcuPicSums : nullptr;   // (the writer summed them: segments may be as many as MCUs)
    for (int i = (int)threadIdx.x; i < (sums ? 0 : a.num_segs_pad); i += 256) {
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
    if (sums) { bits = sums[0]; syms = sums[1]; }
    const uint32_t st = a.scan_stats->status;
    const uint64_t size = *a.out_size[q];                           // k_finalize's: the would-be size when it did not fit
    const bool fit = (st & ~1u) == 0u && size <= a.out_capacity;
    const unsigned long long *pic = a.pic + (size_t)q * kPicStatWords;
    ScanStats *t = a.stats;
    atomicAdd((unsigned long long *)&t->total_bits, bits);
    atomicAdd((unsigned long long *)&t->total_syms, syms);
    atomicAdd((unsigned long long *)&t->total_exact, pic[2] + pic[5] + pic[8]);
    atomicAdd((unsigned long long *)&t->total_ff,
              sums ? sums[2] : (unsigned long long)(size - (uint64_t)a.prefix_len - 2u - (bits + 7u) / 8u));
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
