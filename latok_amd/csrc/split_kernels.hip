// split_kernels.hip -- the tile pipeline around the tile function (tile_core.h): the block-wide scans, the LDS map and the
// table loads of a workgroup, k_tiles_main (stage 1), k_resolve_fix (stage 2), k_tile_index (stage 0), k_one_segment (the
// three in one launch), k_small_batch / k_small_block_mask (a batch of one tile in one launch of one wave), the launch plan
// and the launchers.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "bitscan.h"
#include "feat_records.h"
#include "kernels.h"
#include "tile_core.h"

namespace latok {

// diagnostic build (`make ablate`): k_tiles_main computes every mask word and stores none of them -- the stores hang on a
// condition that never holds and that the compiler cannot see through.  What the mask stores cost = normal - ablated.
#ifdef LATOK_ABLATE_MASK_STORES
#define LATOK_MASK_STORE_GATE && P.total < 0
#else
#define LATOK_MASK_STORE_GATE
#endif

#ifdef LATOK_STAMPS
__device__ unsigned long long g_stamp_sum[16];
__device__ unsigned long long g_stamp_cnt;
#endif

// ---------------------------------------------------------------------------------------------------------------
// stage 2: resolve, for every tile, (a) the number of pending starts entering it (forward scan of the tile transfer
// functions) and (b) whether the block that is open at its end gets zeroed (needs the starts that follow before the
// next closing event: backward scan).  Tiles whose provisional assumptions (q_in == 0, tail = "pending at end") do
// not hold are appended to the fix list.  One workgroup; each thread owns a contiguous chunk of tiles.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ Fn64 fn_then(Fn64 f1, Fn64 f2) {
    Fn64 f;
    const bool c1 = f1.a <= kNegInf64, c2 = f2.a <= kNegInf64;
    if (c2) { f.a = kNegInf64; f.b = f2.b; return f; }
    f.a = c1 ? kNegInf64 : f1.a + f2.a;
    const long long c = f1.b + f2.a;
    f.b = c > f2.b ? c : f2.b;
    return f;
}
__device__ __forceinline__ long long fn_apply(Fn64 f, long long q) {
    if (f.a <= kNegInf64) return f.b;
    const long long c = q + f.a;
    return c > f.b ? c : f.b;
}
__device__ __forceinline__ Fn64 fn_of(int4 s) {
    Fn64 f;
    f.a = s.x <= LK_NEG_INF / 2 ? kNegInf64 : (long long)s.x;
    f.b = s.y;
    return f;
}
// backward element: (has_closing, head_starts); (c1,h1) followed by (c2,h2) = (c1|c2, c1 ? h1 : h1+h2)
__device__ __forceinline__ Hd64 hd_then(Hd64 x, Hd64 y) {
    Hd64 r;
    r.c = x.c | y.c;
    r.h = x.c ? x.h : x.h + y.h;
    return r;
}

constexpr int kScanWaves = kWPB;

__device__ __forceinline__ Fn64 fn_identity() { Fn64 f; f.a = 0; f.b = 0; return f; }   // identity on q >= 0
__device__ __forceinline__ Hd64 hd_identity() { Hd64 h; h.h = 0; h.c = 0; return h; }

// Ordered block-wide scans over kScanThreads elements (one per thread).  Returns, for this thread, the composition of
// all EARLIER elements (fn: exclusive prefix) and of all LATER elements (hd: exclusive suffix); *tot_* get the
// composition of the whole block.  Wave-level shuffles + 16 wave aggregates in LDS.
template <int NW>
struct ScanLdsT {
    Fn64 fn_w[NW];
    Hd64 hd_w[NW];
};
typedef ScanLdsT<kScanWaves> ScanLds;
template <int NW = kScanWaves>
__device__ __forceinline__ void block_scan(Fn64 f, Hd64 h, ScanLdsT<NW>& L, Fn64* excl_fn, Hd64* excl_hd, Fn64* tot_fn,
                                           Hd64* tot_hd) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    Fn64 fi = f;
    Hd64 hi = h;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        Fn64 o; o.a = __shfl_up(fi.a, d); o.b = __shfl_up(fi.b, d);
        if (lane >= d) fi = fn_then(o, fi);
        Hd64 oh; oh.h = __shfl_down(hi.h, d); oh.c = __shfl_down(hi.c, d);
        if (lane + d < 64) hi = hd_then(hi, oh);
    }
    __syncthreads();  // protects L against the previous use
    if (lane == 63) L.fn_w[wave] = fi;
    if (lane == 0) L.hd_w[wave] = hi;
    __syncthreads();
    Fn64 ef; ef.a = __shfl_up(fi.a, 1); ef.b = __shfl_up(fi.b, 1);
    if (lane == 0) ef = fn_identity();
    Hd64 eh; eh.h = __shfl_down(hi.h, 1); eh.c = __shfl_down(hi.c, 1);
    if (lane == 63) eh = hd_identity();
    // second level: every wave scans the 16 wave aggregates with shuffles (lanes 0..15), then picks its own entry
    Fn64 wf = lane < NW ? L.fn_w[lane] : fn_identity();
    Hd64 wh = lane < NW ? L.hd_w[lane] : hd_identity();
#pragma unroll
    for (int d = 1; d < NW; d <<= 1) {
        Fn64 o; o.a = __shfl_up(wf.a, d); o.b = __shfl_up(wf.b, d);
        if (lane >= d) wf = fn_then(o, wf);
        Hd64 oh; oh.h = __shfl_down(wh.h, d); oh.c = __shfl_down(wh.c, d);
        if (lane + d < NW) wh = hd_then(wh, oh);
    }
    // inclusive prefix of waves 0..lane in wf, inclusive suffix of waves lane..15 in wh
    Fn64 before; before.a = __shfl(wf.a, wave > 0 ? wave - 1 : 0); before.b = __shfl(wf.b, wave > 0 ? wave - 1 : 0);
    if (wave == 0) before = fn_identity();
    Hd64 after; after.h = __shfl(wh.h, wave < NW - 1 ? wave + 1 : 0); after.c = __shfl(wh.c, wave < NW - 1 ? wave + 1 : 0);
    if (wave == NW - 1) after = hd_identity();
    Fn64 all_f; all_f.a = __shfl(wf.a, NW - 1); all_f.b = __shfl(wf.b, NW - 1);
    Hd64 all_h; all_h.h = __shfl(wh.h, 0); all_h.c = __shfl(wh.c, 0);
    *excl_fn = fn_then(before, ef);
    *excl_hd = hd_then(eh, after);
    *tot_fn = all_f;
    *tot_hd = all_h;
}


// clear mask bits [lo, hi) (clamped to limit); afterwards re-set the first / last bit of the range on request
// (last_back: the kept last bit sits that many positions before hi - 1 -- byte space: the lead byte of the block's last char)
__device__ __forceinline__ void clear_range(uint64_t* bits, int64_t lo, int64_t hi, int64_t limit, int keep_first,
                                            int keep_last, int last_back = 0) {
    if (hi > limit) hi = limit;
    if (lo >= hi) return;
    const int64_t last = hi - 1 - last_back;
    for (int64_t w = lo >> 6; w <= (hi - 1) >> 6; ++w) {
        const int64_t base = w << 6;
        uint64_t m = ~0ull;
        if (lo > base) m &= ~0ull << (lo - base);
        if (hi < base + 64) m &= (1ull << (hi - base)) - 1ull;
        uint64_t v = bits[w] & ~m;
        if (keep_first && (lo >> 6) == w) v |= 1ull << (lo & 63);
        if (keep_last && last >= lo && (last >> 6) == w) v |= 1ull << (last & 63);
        bits[w] = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// LDS map of both kernels (one workgroup of kWPB waves per CU)
// ---------------------------------------------------------------------------------------------------------------
constexpr int kLdsWaves = kTablesLdsBytes;                         // 16 x kWaveLdsBytes
constexpr int kLdsTf = kLdsWaves + kWPB * kWaveLdsBytes;           // int32[kSegMax]: k_resolve_fix's list of tiles to recompute
constexpr int kLdsSumm = kLdsTf + kSegMax * 4;                     // int4[kSegMax]: tile summaries of the segment
constexpr int kLdsScan = kLdsSumm + kSegMax * 16;                  // ScanLds
constexpr int kLdsMisc = kLdsScan + 512;                           // 64 ints of scratch
constexpr int kLdsSlice = kLdsMisc + 256;                          // end of the map (Latin-1 has its [slice LUT | code table] at 0)
// Byte space's tables are larger than the other modes' ([stage 1, uint16 | stage 2 | byte decode table] at 0, all of it below
// 64 KiB, so that a lookup's table base fits the 16-bit offset field of its ds_read); everything behind the tables moves up by
// the difference.  The kernels add lds_shift(MODE) to every offset above but the tables'.
constexpr int kLdsLeadTab = kB6TablesBytes;                       // kModeBytes: the byte decode table, behind the class table,
constexpr int kLdsByteCodes = kLdsLeadTab + kLeadTabBytes;        //   then code[256] of a byte taken as a char of its own: the ASCII codes, 0 from 0x80 on
constexpr int kByteCodesBytes = 256;
constexpr int lds_shift(int mode) { return mode_base(mode) == kModeBytes ? kLdsByteCodes + kByteCodesBytes - kTablesLdsBytes : 0; }
static_assert(lds_shift(kModeBytes) % 16 == 0 && kLdsByteCodes + kByteCodesBytes < 65536, "alignment / immediate offsets");
constexpr int kLdsTotalBase = kLdsSlice;
constexpr int kLdsTotalBytes = kLdsSlice + lds_shift(kModeBytes);
constexpr int lds_total(int mode) { return mode_base(mode) == kModeBytes ? kLdsTotalBytes : kLdsTotalBase; }
// Waves per workgroup of the TILE kernel.  The Latin-1 kernel needs <= 128 VGPRs and its LDS map has room, so it runs 16 waves
// per CU (4 per SIMD): its waves spend half their life in s_waitcnt, a fourth wave per SIMD fills part of that.  The
// buffers of waves 12..15 sit behind the rest of the map, so that every other offset is the same for all kernels.
// (kNarrowWPB, kernels.h)
constexpr int tile_wpb(int mode) {
    return mode_base(mode) == kModeLatin1 && !mode_rules(mode) ? kNarrowWPB
         : (mode_base(mode) == kModeUcs2 && !mode_rules(mode) ? kNarrowWPB : kWPB);   // (the rule interpreter needs > 128 VGPRs)
}
constexpr int lds_total_tiles(int mode) { return lds_total(mode) + (tile_wpb(mode) > kWPB ? (tile_wpb(mode) - kWPB) * kWaveLdsBytes : 0); }
static_assert(lds_total_tiles(kModeLatin1) <= 160 * 1024 && lds_total_tiles(kModeUcs2) <= 160 * 1024, "LDS budget of one CU");
constexpr int kLdsTotal = kLdsTotalBytes;
static_assert(sizeof(ScanLds) <= 512, "scan scratch");
static_assert(kSegMax == kWPB * 64, "one tile per thread in the block-wide scans");
static_assert(kLdsTotal <= 160 * 1024, "LDS budget of one CU");
static_assert(kLdsSumm % 16 == 0 && kLdsScan % 16 == 0 && kLdsSlice % 16 == 0, "alignment");
// k_tiles_main<.., HOLD>, the tile kernel of the UTF-32 bitmask modes (no lds_shift there) for plans with short segments: a segment of at most kSegHoldTiles tiles keeps its mask words in the
// workgroup and stores them as ONE contiguous run at its end (run_segment).  The words of a wave's first kSegHoldLdsRounds tiles go
// straight to a region of their own behind the map, the rest wait in the wave's registers (obuf) and are dropped, once the segment's
// last tile is done, over what is dead by then: the staging buffers and the resolve list area, [kLdsWaves, kLdsSumm).
constexpr bool tile_holds(int mode) { return mode_writes_bits(mode) && !mode_is_bytes(mode); }
constexpr int kTileMaskBytes = kTile / 8;                                       // 512: a tile's 64 mask words
constexpr int kSegHoldLdsTiles = kSegHoldLdsRounds * kWPB;                      // 48
constexpr int kLdsHold = kLdsSlice;                                             // lk_u64[kSegHoldLdsTiles][64]
constexpr int kSegHoldLdsBytes = kSegHoldLdsTiles * kTileMaskBytes;             // 24 576
constexpr int lds_total_main(int mode) { return lds_total_tiles(mode) + (tile_holds(mode) ? kSegHoldLdsBytes : 0); }
static_assert(kSegHoldTiles == kSegHoldRounds * kWPB && kSegHoldRounds - kSegHoldLdsRounds <= 8, "what is not in LDS fits obuf[8]");
static_assert((kSegHoldTiles - kSegHoldLdsTiles) * kTileMaskBytes <= kLdsSumm - kLdsWaves, "the rest of the run fits the dead regions");
static_assert(lds_shift(kModeBits) == 0 && lds_shift(kModeRules) == 0 && lds_total_tiles(kModeBits) == kLdsHold && lds_total_tiles(kModeRules) == kLdsHold,
              "the hold region sits right behind the map");
static_assert(kLdsWaves % 16 == 0 && kLdsHold % 16 == 0 && lds_total_main(kModeBits) <= 160 * 1024 && lds_total_main(kModeRules) <= 160 * 1024,
              "16-byte LDS reads of the write-out; LDS budget of one CU");

// byte space: code[256] of a byte taken as a char of its own -- the 128 ASCII codes (stage-2 blocks 0 and 1), 0 from 0x80 on: the
// lookups of phase 1 then need no masking of the non-ASCII positions (threads 0..15)
__device__ __forceinline__ void load_byte_codes(uint8_t* lds, const SplitParams& P) {
    if (threadIdx.x < 8) reinterpret_cast<uint4*>(lds + kLdsByteCodes)[threadIdx.x] = reinterpret_cast<const uint4*>(P.t2)[threadIdx.x];
    else if (threadIdx.x < 16) reinterpret_cast<uint4*>(lds + kLdsByteCodes)[threadIdx.x] = make_uint4(0u, 0u, 0u, 0u);
}

// Both tables are contiguous in LDS ([stage1 | stage2]) and in global memory (api.cpp uploads them back to back), so the
// copy is one stream of kTablesLdsBytes / 16 vectors; all of a thread's loads are issued before its first LDS write.
template <int NT = kWPB * 64, int MODE = kModeBits>
__device__ __forceinline__ void load_tables(uint8_t* lds, const SplitParams& P) {
    if (mode_base(MODE) == kModeLatin1) {
        build_latin1_tables<NT>(lds, P);
        return;
    }
    if (mode_base(MODE) == kModeBytes) {
        // byte space: its own class table -- stage 1 (uint16 offsets) to 0, stage 2 behind it
        build_lead_table<NT>(lds + kLdsLeadTab);
        load_byte_codes(lds, P);
        const uint4* src1 = reinterpret_cast<const uint4*>(P.t1);
        const uint4* src2 = reinterpret_cast<const uint4*>(P.t2);
        uint4* dst1 = reinterpret_cast<uint4*>(lds);
        uint4* dst2 = reinterpret_cast<uint4*>(lds + kB6Stage1Bytes);
        constexpr int kVec1 = kB6Stage1Bytes / 16, kVecB = kVec1 + kB6Stage2Bytes / 16;   // 2240 + 1600
        constexpr int kPerB = (kVecB + NT - 1) / NT;                                       // 5 with 768 threads
        if (kPerB <= 5) {
            uint4 tmp[kPerB <= 5 ? kPerB : 1];   // all of a thread's loads are issued before its first LDS write
#pragma unroll
            for (int j = 0; j < (kPerB <= 5 ? kPerB : 1); ++j) {
                const int i = threadIdx.x + j * NT;
                if (i < kVecB) tmp[j] = i < kVec1 ? src1[i] : src2[i - kVec1];
            }
#pragma unroll
            for (int j = 0; j < (kPerB <= 5 ? kPerB : 1); ++j) {
                const int i = threadIdx.x + j * NT;
                if (i < kVecB) { if (i < kVec1) dst1[i] = tmp[j]; else dst2[i - kVec1] = tmp[j]; }
            }
        } else {
            for (int i = threadIdx.x; i < kVec1; i += NT) dst1[i] = src1[i];
            for (int i = threadIdx.x; i < kVecB - kVec1; i += NT) dst2[i] = src2[i];
        }
        if (threadIdx.x == 0) {   // (tables_ensure_bytes: nothing left to fetch)
            int* ctl = reinterpret_cast<int*>(lds + lds_shift(kModeBytes) + kLdsMisc) + 16;
            ctl[0] = ctl[1] = 64 * kLazyGrabs;
        }
        return;
    }
    constexpr int kVec = kTablesLdsBytes / 16;                    // 2585
    constexpr int kPer = (kVec + NT - 1) / NT;                    // 4 with 768 threads
    const uint4* src = reinterpret_cast<const uint4*>(P.t1);
    uint4* dst = reinterpret_cast<uint4*>(lds);
    if (kPer <= 4) {
        uint4 tmp[kPer <= 4 ? kPer : 1];
#pragma unroll
        for (int j = 0; j < (kPer <= 4 ? kPer : 1); ++j) {
            const int i = threadIdx.x + j * NT;
            if (i < kVec) tmp[j] = src[i];
        }
#pragma unroll
        for (int j = 0; j < (kPer <= 4 ? kPer : 1); ++j) {
            const int i = threadIdx.x + j * NT;
            if (i < kVec) dst[i] = tmp[j];
        }
    } else {
        for (int i = threadIdx.x; i < kVec; i += NT) dst[i] = src[i];
    }
}

// k_tiles_main in byte space: the ASCII part of the class table now, the rest when a tile asks for it (tables_ensure_bytes)
__device__ __forceinline__ void load_tables_ascii_bytes(uint8_t* lds, const SplitParams& P) {
    load_byte_codes(lds, P);
    if (threadIdx.x == 16) {
        int* ctl = reinterpret_cast<int*>(lds + lds_shift(kModeBytes) + kLdsMisc) + 16;
        ctl[0] = ctl[1] = 0;
    }
}
// the rest of it: pieces of kLazyPer rows of 1 KiB, handed out by ctl[0]; ctl[1] counts the pieces that are in place.  The rows go
// from global memory straight to LDS (global_load_lds_dwordx4: wave-uniform LDS base + 16 x lane, no registers in between -- the
// wave that fetches holds its tile's bytes in registers), the last piece is the byte decode table, which is computed.
__device__ __attribute__((noinline, cold)) void tables_fetch_bytes(const uint8_t* t1, const uint8_t* t2, uint8_t* tables, int* ctl) {
    const int lane = (int)(threadIdx.x & 63u);
    struct { const uint8_t* t1; const uint8_t* t2; } P = {t1, t2};
    struct { uint8_t* tables; int* ctl; } L = {tables, ctl};
    typedef const void __attribute__((address_space(1))) * gptr_t;
    typedef void __attribute__((address_space(3))) * lptr_t;
    for (;;) {
        const int ticket = __hip_atomic_fetch_add(&L.ctl[0], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        const int g = __builtin_amdgcn_readfirstlane(ticket) >> 6;                 // wave-uniform: 64 tickets per piece
        if (g >= kLazyGrabs) break;
        if (g == kLazyGrabs - 1) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const lk_lead_entry e = lk_lead_entry_of((uint32_t)(64 * j + lane));
                reinterpret_cast<uint2*>(L.tables + kLdsLeadTab)[64 * j + lane] = make_uint2(e.sel, e.hi0);
            }
        } else {
#pragma unroll
            for (int j = 0; j < kLazyPer; ++j) {
                const int row = g * kLazyPer + j;                                  // wave-uniform
                if (row < kLazyRows)   // (both stages are back to back, in global memory as in LDS)
                    __builtin_amdgcn_global_load_lds((gptr_t)(P.t1 + 1024 * row + 16 * lane), (lptr_t)(L.tables + 1024 * row), 16, 0, 0);
            }
            __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): the rows have landed
        }
        // (the LDS executes one wave's instructions in order: the piece is in place before the count says so)
        __hip_atomic_fetch_add(&L.ctl[1], 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    while (__hip_atomic_load(&L.ctl[1], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < 64 * kLazyGrabs) __builtin_amdgcn_s_sleep(2);
}

template <int MODE = kModeBits>
__device__ __forceinline__ TileLds wave_lds(uint8_t* lds, int wave) {
    TileLds L;
    L.t1 = lds;
    L.t2 = lds + kStage1Pad;
    uint8_t* const w = lds + lds_shift(MODE);
    uint8_t* mine = wave < kWPB ? w + kLdsWaves + wave * kWaveLdsBytes : lds + lds_total(MODE) + (wave - kWPB) * kWaveLdsBytes;
    L.stage = mine;
    L.halo = mine + kStageBytes;
    L.bw = reinterpret_cast<lk_u64*>(mine + kStageBytes + 16);
    L.lut = lds;                                                     // build_latin1_tables (kModeLatin1: in place of the Unicode tables)
    L.ltab = lds + kLdsLeadTab;
    L.tables = lds;
    L.ctl = reinterpret_cast<int*>(w + kLdsMisc) + 16;
    L.t1b = lds;
    L.t2b = lds + kB6Stage1Bytes;
    L.ctab = mode_base(MODE) == kModeBytes ? lds + kLdsByteCodes : L.lut + kSliceLutBytes;   // (byte space: code of a byte taken as a char, 0 from 0x80 on)
    L.small_bits = L.small_space = nullptr;
    return L;
}

// ---------------------------------------------------------------------------------------------------------------
// stage 1: the tiles.  The tile range is cut into segments of P.seg_tiles (<= 1024) consecutive tiles; a workgroup
// owns whole segments (grid-stride), its kWPB waves take the segment's tiles round-robin.  Per segment the workgroup
//   (a) fetches the first string of each of its tiles from the index stage 0 (k_tile_index) left in P.tile_first,
//   (b) runs the tiles, each publishing its 16-byte summary to LDS and to global memory,
//   (c) composes the segment's transfer function / head descriptor with a block-wide scan -> one aggregate per segment.
// ---------------------------------------------------------------------------------------------------------------
//   (d) HOLD (k_tiles_main<.., HOLD>: UTF-32 bitmask modes, segments of at most kSegHoldTiles tiles): stores the segment's mask words, which
//       no wave has stored until now, as one run of n_seg x 512 consecutive bytes.
template <int MODE, bool FAST_TAIL = false, int WPB = kWPB, int PF = kCpsPrefetchRows, bool HOLD = false>
__device__ __forceinline__ void run_segment(const SplitParams& P, uint8_t* lds, int64_t seg, int tid, int lane,
                                            int wave, bool tables LATOK_STAMP_PARAM) {
    const int S = P.seg_tiles;
    const TileLds L = wave_lds<MODE>(lds, wave);
    int4* sm = reinterpret_cast<int4*>(lds + lds_shift(MODE) + kLdsSumm);
    ScanLdsT<WPB>& scan = *reinterpret_cast<ScanLdsT<WPB>*>(lds + lds_shift(MODE) + kLdsScan);

    const int64_t T0 = seg * S;
    const int64_t T1 = min(T0 + S, P.n_tiles);
    const int n_seg = (int)(T1 - T0);
    // (a) first string of each tile: P.tile_first, written by k_tile_index before this kernel.  A wave takes the tiles
    //     wave, wave + kWPB, ... of the segment -- at most 64 -- so one load per lane holds the whole segment's worth.
    int64_t tfv = 0;
    if (wave + WPB * lane < n_seg) tfv = P.tile_first[T0 + wave + WPB * lane];
    tfv = tfv < 0 ? 0 : (tfv > P.n_str ? P.n_str : tfv);   // (row offsets that are not non-decreasing leave holes in the index)
    if (tables) __syncthreads();   // the class tables (first segment of the workgroup) are in LDS
    // (b) the tiles
    // Output write combining (bitmask mode): the words of up to 8 tiles stay in registers and are stored together.
    // One 512-byte store per 16 KiB tile, interleaved with the read stream, costs ~5 % of HBM throughput.
    // UTF-32 input only: that kernel is HBM bound.  The narrow-input kernels are bound by instruction issue and registers: without
    // the 16 VGPRs of the buffer Latin-1 104 VGPRs (was 121), UCS-2 123 + 64 B scratch (128 + 96), byte space 128 B scratch (192);
    // C3 byte space 0.538 -> 0.506 ms, UCS-2 0.157 -> 0.142, C2 byte space 0.085 -> 0.073, Latin-1 0.069 -> 0.067.
    // A segment of at most kSegHoldTiles tiles (C2 under both plans) stores nothing here: eight 512-byte pieces 6 KiB apart are
    // still eight bursts.  Its words wait -- rounds 0 .. kSegHoldLdsRounds - 1 in LDS, the others in obuf -- for step (d).
    constexpr bool kDefer = mode_writes_bits(MODE) && !mode_is_bytes(MODE);
    static_assert(!HOLD || (kDefer && WPB == kWPB), "held segments: UTF-32 bitmask modes");
    lk_u64* const hold_lo = reinterpret_cast<lk_u64*>(lds + kLdsHold);     // words of tiles 0 .. kSegHoldLdsTiles - 1 of the segment
    lk_u64* const hold_hi = reinterpret_cast<lk_u64*>(lds + kLdsWaves);    // ... of the tiles behind them (valid in step (d) only)
    lk_u64 obuf[8];
    int slot = 0, k_first = wave;   // buffered tiles are k_first, k_first + kWPB, ...
    const int64_t n_words = (P.total + 63) >> 6;
    auto flush = [&]() {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (j < slot) {
                const int64_t w = (T0 + k_first + j * WPB) * 64 + lane;
                if (w < n_words LATOK_MASK_STORE_GATE) P.bits_out[w] = obuf[j];
            }
        }
        slot = 0;
    };
    auto put = [&](lk_u64 w, int k, bool keep) {   // keep = false: the word is in LDS already (the selects run all the same: no branch around obuf)
        if (slot == 0 && keep) k_first = k;
        const int sel = keep ? slot : -1;
#pragma unroll
        for (int j = 0; j < 8; ++j) obuf[j] = (j == sel) ? w : obuf[j];
        if (keep && ++slot == 8 && !HOLD) flush();   // (held: at most 8 rounds come here)
    };
    CpsPrefetch pf;
    pf.valid = false;
    for (int k = wave, j = 0; k < n_seg; k += WPB, ++j) {
        const lk_u64 w = process_tile<MODE, kDefer, false, FAST_TAIL, PF>(P, L, T0 + k, lane_read64(tfv, j), 0, -1, true, &sm[k], lane LATOK_STAMP_ARG
                                                                      , MODE == kModeBits && !FAST_TAIL ? &pf : nullptr, k + WPB < n_seg ? T0 + k + WPB : (int64_t)-1
                                                                      );
        if (kDefer) {
            const bool to_lds = HOLD && j < kSegHoldLdsRounds;
            if (to_lds) hold_lo[k * 64 + lane] = w;
            put(w, k, !to_lds);
        }
#ifdef LATOK_STAMPS
        stamp_acc[0] += 1;
#endif
    }
    if (kDefer && !HOLD) flush();
    __syncthreads();
    // (held segments: every tile is done, so the staging buffers are dead, and this kernel never uses the list area: each wave drops
    // its registers' words at its tiles' places over them; the summaries behind them are still needed.  The barriers of the scan
    // below publish the words.)
    if (HOLD) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (j < slot) hold_hi[(k_first + j * WPB - kSegHoldLdsTiles) * 64 + lane] = obuf[j];
    }
    // (c) segment aggregate
    {
        Fn64 f = fn_identity();
        Hd64 h = hd_identity();
        if (tid < n_seg) {
            const int4 s = sm[tid];
            P.summ[T0 + tid] = s;            // coalesced: 16 B per thread, one burst per segment
            f = fn_of(s);
            h.h = s.z; h.c = s.w & 1;
        }
        Fn64 ef, tfn; Hd64 eh, th;
        block_scan<WPB>(f, h, scan, &ef, &eh, &tfn, &th);
        if (tid == 0) { P.seg_fn[seg] = tfn; P.seg_hd[seg] = th; }
    }
    // (d) the held mask words: every thread is past the scan's barriers, so all of them are in LDS.  All threads store the run in
    //     address order, 16 B per lane: 1 KiB per wave instruction, 12 KiB per sweep.
    if (HOLD) {
        const int64_t w0 = T0 * 64;                                                  // first word of the run
        int n_run = (int)min((int64_t)n_seg * 64, n_words - w0);                     // the batch ends inside its last tile
#ifdef LATOK_ABLATE_MASK_STORES
        if (P.total >= 0) n_run = 0;
#endif
        uint64_t* const dst = P.bits_out + w0;
        auto held = [&](int w) -> const lk_u64* {
            return w < kSegHoldLdsTiles * 64 ? hold_lo + w : hold_hi + (w - kSegHoldLdsTiles * 64);
        };
        if ((reinterpret_cast<uintptr_t>(P.bits_out) & 15u) == 0) {                  // (w0 is even: the pairs are 16-byte aligned)
            for (int w = 2 * tid; w < n_run; w += 2 * WPB * 64) {
                if (w + 1 < n_run) *reinterpret_cast<uint4*>(dst + w) = *reinterpret_cast<const uint4*>(held(w));
                else dst[w] = *held(w);                                              // the batch's last word, alone
            }
        } else {                                                                     // a mask that is only 8-byte aligned
            for (int w = tid; w < n_run; w += WPB * 64) dst[w] = *held(w);
        }
    }
    __syncthreads();   // (the LDS is the next segment's)
}

// FAST_TAIL: the batch's last, partial tile requests all its rows before the first lookup (process_tile).  Chosen for small
// batches, where that tile's latency is a visible share of the call (a 4-tile batch in pinned host memory: 31 -> 16 us);
// the large-batch instantiation keeps the serial tail: the unified form costs its full-tile loop 16 VGPRs and 4 % on C2.
// HOLD: the same with held segments (UTF-32 bitmask modes, plans whose segments have at most kSegHoldTiles tiles: LaunchPlan::hold)
template <int MODE, bool FAST_TAIL = false, int PF = kCpsPrefetchRows, bool HOLD = false>
__global__ __launch_bounds__(tile_wpb(MODE) * 64) void k_tiles_main(SplitParams P) {
    constexpr int WPB = tile_wpb(MODE);
    static_assert(!HOLD || tile_holds(MODE), "UTF-32 bitmask modes");
    __shared__ __attribute__((aligned(16))) uint8_t lds[HOLD ? lds_total_main(MODE) : lds_total_tiles(MODE)];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave-uniform -> scalar tile arithmetic
    if (blockIdx.x == 0 && tid == 0) *P.fix_count = 0;            // statistics counter of the resolve stage

    bool tables = MODE != kModeBlockMask;
    // (published by the barrier at the top of the workgroup's first segment)
    if (tables) {
        if (mode_base(MODE) == kModeBytes) load_tables_ascii_bytes(lds, P);
        else load_tables<WPB * 64, MODE>(lds, P);
    }
#ifdef LATOK_STAMPS
    unsigned long long stamp_acc[16];
    for (int i = 0; i < 16; ++i) stamp_acc[i] = 0;
#endif
    for (int64_t seg = blockIdx.x; seg < P.n_segs; seg += gridDim.x) {
        run_segment<MODE, FAST_TAIL, WPB, PF, HOLD>(P, lds, seg, tid, lane, wave, tables LATOK_STAMP_ARG);
        tables = false;
    }
#ifdef LATOK_STAMPS
    if (lane == 0)
        for (int i = 0; i < 16; ++i) atomicAdd(&g_stamp_sum[i], stamp_acc[i]);
#endif
}

// ---------------------------------------------------------------------------------------------------------------
// stage 2: resolve + repair.  Same segment ownership.  Per segment the workgroup composes the aggregates of the
// segments before it (pending starts entering the segment) and after it (starts before the next closing event),
// scans its own tiles, and for every tile whose provisional assumptions (no pending start enters, tail block decided
// by "pending at the tile end") were wrong: patches the bitmask in place for the common cases, or recomputes the tile
// with the exact inputs (the same tile code; Unicode tables are only copied to LDS if that ever happens).
// ---------------------------------------------------------------------------------------------------------------
// NW = waves per workgroup: NW * 64 threads must cover a segment's tiles (one tile per thread).  Batches whose segments
// are short (C2: 122 tiles) run it with 2 or 4 waves instead of 12 -- the stage is all latency, fewer waves start faster.
// Stage 2.  ONE = false: k_resolve_fix, every segment of the batch, a workgroup per segment at a time.  ONE = true: the only
// segment of a small batch, inside the launch that computed it (k_one_segment; the class tables are still in LDS).
template <int MODE, int NW, bool ONE>
__device__ __forceinline__ void resolve_segments(const SplitParams& P, uint8_t* lds, int tid, int lane, int wave) {
    const int S = P.seg_tiles;
    ScanLdsT<NW>& scan = *reinterpret_cast<ScanLdsT<NW>*>(lds + lds_shift(MODE) + kLdsScan);
    int* misc = reinterpret_cast<int*>(lds + lds_shift(MODE) + kLdsMisc);          // misc[0] = number of tiles to recompute
    int* fix_t = reinterpret_cast<int*>(lds + lds_shift(MODE) + kLdsTf);           // tile index inside the segment (tiles to recompute)
    int2* fix_in = reinterpret_cast<int2*>(lds + lds_shift(MODE) + kLdsSumm);      // {q_in, tail_zero}
    bool tables_loaded = ONE;

    for (int64_t seg = ONE ? 0 : (int64_t)blockIdx.x; seg < (ONE ? 1 : P.n_segs); seg += ONE ? 1 : (int64_t)gridDim.x) {
        const int64_t T0 = seg * S;
        const int64_t T1 = min(T0 + S, P.n_tiles);
        const int n_seg = (int)(T1 - T0);
        // my tile's summary is requested first: its latency overlaps the scan of the segment aggregates
        if (tid == 0) misc[0] = 0;
        const int64_t t = T0 + tid;
        int4 s = make_int4(0, 0, 0, 0);
        if (tid < n_seg) s = P.summ[t];
        // (1) aggregates of the other segments: contiguous range per thread, ordered
        Fn64 pf = fn_identity();
        Hd64 sh = hd_identity();
        if (P.n_segs > 1) {
            const int64_t per = (P.n_segs + NW * 64 - 1) / (NW * 64);
            const int64_t lo = min((int64_t)tid * per, P.n_segs), hi = min(lo + per, P.n_segs);
            Fn64 f = fn_identity();
            Hd64 h = hd_identity();
            for (int64_t j = lo; j < hi; ++j) {
                if (j < seg) f = fn_then(f, P.seg_fn[j]);
                if (j > seg) h = hd_then(h, P.seg_hd[j]);
            }
            Fn64 ef; Hd64 eh;
            block_scan<NW>(f, h, scan, &ef, &eh, &pf, &sh);
        }
        const long long q_seg_in = fn_apply(pf, 0);
        Hd64 rest; rest.h = sh.h; rest.c = 1;   // what follows the segment: sh.h starts before the next closing

        // (2) my tile
        Fn64 f = fn_identity();
        Hd64 h = hd_identity();
        if (tid < n_seg) {
            f = fn_of(s);
            h.h = s.z; h.c = s.w & 1;
        }
        Fn64 ef, tfn; Hd64 eh, th;
        block_scan<NW>(f, h, scan, &ef, &eh, &tfn, &th);   // (its barriers also publish misc[0] = 0)
        if (tid < n_seg) {
            const long long q_in = fn_apply(ef, q_seg_in);
            const long long q_end = fn_apply(f, q_in);
            const long long h_next = hd_then(eh, rest).h;
            const int tz = (q_end + h_next) > 0;
            const int tz0 = s.y > 0;
            if (q_in != 0 || tz != tz0) {
                const int geom = s.w;
                if (!mode_rules(MODE) && (MODE == kModeBits || mode_is_bytes(MODE)) && (geom & 1) && q_in <= 1 &&
                    (q_in == 0 || s.z == 0)) {
                    // Patch in place: one pending start entering a tile whose head block has no start of its own
                    // zeroes that head block; a tail block that turns out to be zeroed is cleared.  What stays in a
                    // cleared block: the C_SYM bit of its last char and the bit of a string start.
                    // (byte space, tiles with multi-byte chars: the last char's bit is at its lead byte, up to 3 bytes before the
                    // block's last position -- found in the bytes themselves)
                    const int64_t t0 = t * kTile;
                    const int64_t t_end = min(t0 + kTile, P.total);
                    auto lead_back = [&](int64_t lo, int64_t hi) -> int {
                        int back = 0;
                        if (mode_base(MODE) == kModeBytes && ((geom >> 30) & 1)) {
                            if (hi > t_end) hi = t_end;
                            while (back < 3 && hi - 1 - back > lo && (P.u8[hi - 1 - back] & 0xC0u) == 0x80u) ++back;
                        }
                        return back;
                    };
                    if (q_in == 1) {
                        const int64_t hi = t0 + ((geom >> 1) & 0x1FFF);
                        const int keep = (geom >> 27) & 1;
                        clear_range(P.bits_out, t0, hi, t_end, 0, keep, keep ? lead_back(t0, hi) : 0);
                    }
                    if (tz != tz0) {
                        const int64_t lo = t0 + ((geom >> 14) & 0x1FFF);
                        const int keep = (geom >> 29) & 1;
                        clear_range(P.bits_out, lo, t_end, t_end, (geom >> 28) & 1, keep, keep ? lead_back(lo, t_end) : 0);
                    }
                } else {
                    const int slot = atomicAdd(&misc[0], 1);
                    fix_t[slot] = tid;
                    fix_in[slot] = make_int2((int)(q_in < (1 << 20) ? q_in : (1 << 20)), tz);   // <= 4096 closings/tile
                }
            }
        }
        __syncthreads();
        // (3) recompute what could not be patched (rare)
        const int n_fix = misc[0];
        if (n_fix > 0) {
            if (!tables_loaded && MODE != kModeBlockMask) {
                load_tables<NW * 64, MODE>(lds, P);
                tables_loaded = true;
                __syncthreads();
            }
            const TileLds L = wave_lds<MODE>(lds, wave);
            for (int i = wave; i < n_fix; i += NW) {
                const int64_t tt = T0 + fix_t[i];
                const int2 in = fix_in[i];
                const int64_t idx0 = wave_lower_bound(P.row_off, P.n_str + 1, tt * kTile, lane);
                process_tile<MODE>(P, L, tt, idx0, in.x, in.y, false, nullptr, lane);
            }
            if (tid == 0) atomicAdd(reinterpret_cast<unsigned long long*>(P.fix_count), (unsigned long long)n_fix);
        }
        __syncthreads();
    }
}

template <int MODE, int NW>
__global__ __launch_bounds__(NW * 64) void k_resolve_fix(SplitParams P) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[lds_total(MODE)];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    resolve_segments<MODE, NW, false>(P, lds, tid, lane, wave);
    signal_block_done(P.done);
}

// stage 0 (k_tile_index below, k_one_segment): entry s of row_off (s > n_str: nothing); must be called by whole waves (the wide form below uses wave operations)
__device__ __forceinline__ void tile_index_entry(const int64_t* __restrict__ row_off, int64_t n_str, int64_t n_tiles,
                                                 int64_t* __restrict__ tile_first, int64_t s, int lane) {
    int64_t w0 = 0, w1 = -1;
    if (s <= n_str) {
        const int64_t p = row_off[s];
        const int64_t prev = s > 0 ? row_off[s - 1] : -1;
        w0 = prev < 0 ? 0 : prev / kTile + 1;
        w1 = p / kTile;
        if (w1 > n_tiles - 1) w1 = n_tiles - 1;
    }
    const bool wide = w1 - w0 >= 16;
    if (!wide)
        for (int64_t w = w0; w <= w1; ++w) tile_first[w] = s;
    unsigned long long m = __ballot(wide);
    while (m) {   // wave-uniform
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        const int64_t a = lane_read64(w0, src), b = lane_read64(w1, src), v = lane_read64(s, src);
        for (int64_t w = a + lane; w <= b; w += 64) tile_first[w] = v;
    }
}


// A batch of at most kOneSegTiles tiles (P.n_segs == 1, P.seg_tiles >= P.n_tiles): the three stages in ONE launch of one
// workgroup -- the per-tile string index, the tiles, the resolve stage -- with workgroup barriers where the stream order
// of the three launches was.  Three dependent launches of a few microseconds of work each cost ~5 us apiece in dispatch
// and drain; a host batch of 40 ... 1000 short strings is nothing but that.
template <int MODE>
__global__ __launch_bounds__(kWPB * 64) void k_one_segment(SplitParams P) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[lds_total(MODE)];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (tid == 0) *P.fix_count = 0;
    load_tables<kWPB * 64, MODE>(lds, P);                       // (published by the barriers below)
    for (int64_t base = 0; base <= P.n_str; base += kWPB * 64)  // stage 0
        tile_index_entry(P.row_off, P.n_str, P.n_tiles, P.tile_first, base + tid, lane);
    __threadfence_block();
    __syncthreads();
    run_segment<MODE, true>(P, lds, 0, tid, lane, wave, true LATOK_STAMP_NULL);   // stage 1 (ends with a barrier)
    __threadfence_block();
    __syncthreads();
    resolve_segments<MODE, kWPB, true>(P, lds, tid, lane, wave);                  // stage 2
    signal_block_done(P.done);
}

// flags[0] = any(a1 != 0), flags[1] = any(a2 != 0) (flags zeroed by the caller)
__global__ void k_any_nonzero(const int8_t* __restrict__ a1, const int8_t* __restrict__ a2, int64_t n,
                              int* __restrict__ flags) {
    int f1 = 0, f2 = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        f1 |= a1[i] != 0;
        f2 |= a2[i] != 0;
    }
    if (__any(f1) && (threadIdx.x & 63) == 0) atomicOr(&flags[0], 1);
    if (__any(f2) && (threadIdx.x & 63) == 0) atomicOr(&flags[1], 1);
}

hipError_t launch_any_nonzero(const int8_t* a1, const int8_t* a2, int64_t n, int* flags, hipStream_t st) {
    hipError_t e = hipMemsetAsync(flags, 0, 2 * sizeof(int), st);
    if (e != hipSuccess || n <= 0) return e;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(k_any_nonzero, dim3((unsigned)blocks), dim3(256), 0, st, a1, a2, n, flags);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// Small batches in ONE launch (the drop-in tokenize(text) surface: one string per call).  A batch of at most one tile
// (4096 chars) needs no tile index, no resolve stage and no device-wide scan: a single wave classifies it, runs the
// tile function -- whose two provisional assumptions are exact here: nothing enters the batch's first tile, and the
// batch ends inside it or at its end --, counts, ranks and scatters.  What was six dependent launches (~45 us of launch
// latency for ~2 us of work) is one.  Inputs and outputs live in pinned host memory the kernel reads and writes over
// the bus (api.cpp), the class tables are read from global memory (they sit in L2; the 41 KB LDS copy would cost more
// than the few hundred lookups).
// ---------------------------------------------------------------------------------------------------------------
struct SmallParams {
    SplitParams P;          // cps, row_off, n_str, total (<= kTile), t1 / t2 (global memory), rules
    void* counts;           // OUT[n_str]
    void* items;            // KIND 0: OUT[n_items] offsets; KIND 1: OUT[n_items][2] stripped token spans
    int64_t* n_items;       // [1]
    unsigned long long* done;   // pinned host word that receives `seq` after every output has been stored (or NULL)
    unsigned long long seq;
    int8_t* features;       // KIND 2 (featurize): [n_items][25] sums; items = [n_items][4] {raw start, raw end, stripped start, stripped end}
};

template <int MODE, int KIND, typename OUT>
__global__ __launch_bounds__(64) void k_small_batch(SmallParams S) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kWaveLdsBytes];
    __shared__ uint64_t s_bits[66], s_space[66], s_items[66];
    __shared__ int s_pref[66];
    const int lane = threadIdx.x;
    TileLds L;
    L.t1 = S.P.t1;          // global memory
    L.t2 = S.P.t2;
    L.lut = L.ctab = L.ltab = L.t1b = L.t2b = nullptr; L.tables = nullptr; L.ctl = nullptr;
    L.stage = lds;
    L.halo = lds + kStageBytes;
    L.bw = reinterpret_cast<lk_u64*>(lds + kStageBytes + 16);
    s_bits[lane] = 0ull;
    s_space[lane] = ~0ull;   // positions behind the batch read as SPACE
    if (lane < 2) { s_bits[64 + lane] = 0ull; s_space[64 + lane] = ~0ull; }
    const SplitParams& P = S.P;
    L.small_bits = s_bits;
    L.small_space = KIND >= 1 ? s_space : nullptr;
    wave_lds_sync();
    const int64_t total = P.total, n_str = P.n_str;
    const int64_t n_words = (total + 63) >> 6;
    // the bounds of the first 64 strings, requested now: they travel over the bus together with the tile's chars
    int64_t ro_a = 0, ro_b = 0;
    if (lane < n_str) { ro_a = P.row_off[lane]; ro_b = P.row_off[lane + 1]; }
    const lk_u64 xb = process_tile<MODE, false, true, true>(P, L, 0, 0, 0, -1, false, nullptr, lane);   // boundaries of my word
    wave_lds_sync();
    const int64_t base = 64 * (int64_t)lane;
    // ---- which boundaries are items (spans: those whose token holds a non-SPACE char), like k_word_counts -------------
    lk_u64 x = xb;
    const lk_u64 nn = KIND >= 1 ? (~s_space[lane] & valid_mask(lane, total)) : 0ull;
    lk_u64 xb1 = 0, nn1 = 0;
    if (KIND >= 1) {
        xb1 = __shfl_down(xb, 1);
        nn1 = __shfl_down(nn, 1);
        if (lane == 63) { xb1 = 0; nn1 = 0; }
        bool cin;
        if (xb1) cin = (nn1 & ((xb1 & (~xb1 + 1ull)) - 1ull)) != 0;
        else cin = nn1 != 0 || (xb != 0 && lane + 1 < n_words && tail_has_nonspace(s_bits, s_space, lane + 1, n_words, total));
        x = kept_boundaries(xb, nn, cin);
    }
    const int cnt = lk_popc(x);
    int inc = cnt;   // (shfl_scan_add, written out: the call reorders this kernel's instructions)
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    const int n_items = __shfl(inc, 63);
    s_items[lane] = x;
    s_pref[lane] = inc - cnt;
    if (lane == 0) { s_items[64] = 0ull; s_pref[64] = n_items; *S.n_items = n_items; }
    wave_lds_sync();
    // ---- per-string counts: rank(end) - rank(start) ----------------------------------------------------------------
    OUT* counts = reinterpret_cast<OUT*>(S.counts);
    auto rank_of = [&](int64_t p) -> int {
        if (p >= total) return n_items;
        return s_pref[p >> 6] + lk_popc(s_items[p >> 6] & low_mask((int)(p & 63)));
    };
    if (lane < n_str) counts[lane] = (OUT)(rank_of(ro_b) - rank_of(ro_a));
    for (int64_t s = 64 + lane; s < n_str; s += 64) counts[s] = (OUT)(rank_of(P.row_off[s + 1]) - rank_of(P.row_off[s]));
    // ---- where the string that owns a position begins: last string start at or before it (L.bw: the tile's string starts)
    const lk_u64 Bw = L.bw[lane];
    const int carry = last_start_before(Bw, lane);
    const int64_t lo_in = carry >= 0 ? carry : 0;
    if (KIND == 2) {
        // ---- featurize: the 25 feature planes of every word go to LDS, then lane = TOKEN: its span from the bitmasks, its
        //      sums = popcounts of the planes over the span.  (k_features_tiles is built for throughput -- ~7 K dependent
        //      instructions per tile, 26 us when a single tile is all there is; this is ~1 K.)
        __shared__ lk_u64 s_planes[64 * LK_N_FEATURES];
        __shared__ int s_lo[64];
        __shared__ __attribute__((aligned(16))) uint8_t s_win[64 * kFeatRec + 16];
        {
            uint32_t d[16];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint4 q = *reinterpret_cast<const uint4*>(L.stage + 80u * lane + 16u * k);
                d[4 * k + 0] = q.x; d[4 * k + 1] = q.y; d[4 * k + 2] = q.z; d[4 * k + 3] = q.w;
            }
            lk_halo h;
            h.prev = lane > 0 ? L.stage[80u * lane - 17u] : L.halo[0];
            h.next0 = lane < 63 ? L.stage[80u * lane + 80u] : L.halo[1];
            h.next1 = lane < 63 ? L.stage[80u * lane + 81u] : L.halo[2];
            lk_u64 plane[8];
            lk_bitslice64(d, plane);
            lk_planes F;
            lk_feature_planes(plane, h, Bw, L.bw[lane + 1] & 3ull, F);
#pragma unroll
            for (int c = 0; c < LK_N_FEATURES; ++c) s_planes[lane * LK_N_FEATURES + c] = LK_PLANE_GET(F, c);
        }
        s_lo[lane] = (int)lo_in;
        wave_lds_sync();
        OUT* spans4 = reinterpret_cast<OUT*>(S.items);
        for (int k0 = 0; k0 < n_items; k0 += 64) {
            const int k = k0 + lane;
            FeatSums sum;
#pragma unroll
            for (int j = 0; j < 7; ++j) sum.v[j] = 0;
            if (k < n_items) {
                // the word that holds kept token k: the last w with s_pref[w] <= k (s_pref[64] = n_items)
                int wl = 0, wh = 64;
                while (wh - wl > 1) {
                    const int mid = (wl + wh) >> 1;
                    if (s_pref[mid] <= k) wl = mid; else wh = mid;
                }
                lk_u64 m = s_items[wl];
                for (int r = k - s_pref[wl]; r > 0; --r) m &= m - 1ull;
                const int b = lk_ctz(m);
                const int64_t a = 64 * (int64_t)wl + b;                       // raw start
                const int64_t e = next_set_bit(s_bits, a + 1, total);         // raw end: the next boundary
                const int64_t a2 = next_zero_bit(s_space, a, e);              // stripped span (a kept token has a non-SPACE char)
                const int64_t e2 = prev_zero_end(s_space, a2, e);
                const lk_u64 bl = L.bw[wl] & ((2ull << b) - 1ull);            // string starts at or before the token
                const int64_t lo = bl ? 64 * (int64_t)wl + 63 - __builtin_clzll(bl) : (int64_t)s_lo[wl];
                OUT* rec = spans4 + 4 * (int64_t)k;
                rec[0] = (OUT)(a - lo); rec[1] = (OUT)(e - lo); rec[2] = (OUT)(a2 - lo); rec[3] = (OUT)(e2 - lo);
                uint32_t acc[LK_N_FEATURES];
#pragma unroll
                for (int c = 0; c < LK_N_FEATURES; ++c) acc[c] = 0;
                for (int64_t w = wl; 64 * w < e; ++w) {
                    lk_u64 msk = ~0ull;
                    if (w == wl) msk &= ~0ull << b;
                    if (e < 64 * w + 64) msk &= (1ull << (e - 64 * w)) - 1ull;
#pragma unroll
                    for (int c = 0; c < LK_N_FEATURES; ++c) acc[c] += (uint32_t)__popcll(s_planes[w * LK_N_FEATURES + c] & msk);
                }
#pragma unroll
                for (int c = 0; c < LK_N_FEATURES; ++c) sum.v[c >> 2] |= (acc[c] & 0xFFu) << (8 * (c & 3));   // uint8 wrap-around (latok.c:342-354)
            }
            const int n_here = min(64, n_items - k0);
            uint8_t* const fdst = reinterpret_cast<uint8_t*>(S.features) + (int64_t)k0 * kFeatRec;
            if (k < n_items) put_record(s_win + record_shift(fdst), lane, sum);
            wave_lds_sync();
            flush_records(s_win, n_here, fdst, lane);
            wave_lds_sync();
        }
    }
    // ---- the records, word-major: lane = word walks its items -------------------------------------------------------
    OUT* out = reinterpret_cast<OUT*>(S.items);
    lk_u64 rest = KIND == 2 ? 0ull : x;
    int k = inc - cnt;
    while (rest) {
        const int b = lk_ctz(rest);
        rest &= rest - 1;
        const lk_u64 bl = Bw & ((2ull << b) - 1ull);      // string starts at or before the item (b = 63: all)
        const int64_t lo = bl ? base + 63 - __builtin_clzll(bl) : lo_in;
        if (KIND == 0) {
            out[k] = (OUT)(base + b - lo);
        } else {
            const lk_u64 above = xb & (~1ull << b);
            int64_t a2, e2;
            if (above) {
                const int eb = lk_ctz(above);
                const lk_u64 seg = nn & (~0ull << b) & ((1ull << eb) - 1ull);
                a2 = base + lk_ctz(seg);
                e2 = base + 64 - __builtin_clzll(seg);
            } else if (xb1) {
                const int eb = lk_ctz(xb1);
                const lk_u64 seg0 = nn & (~0ull << b);
                const lk_u64 seg1 = nn1 & ((1ull << eb) - 1ull);
                a2 = seg0 ? base + lk_ctz(seg0) : base + 64 + lk_ctz(seg1);
                e2 = seg1 ? base + 128 - __builtin_clzll(seg1) : base + 64 - __builtin_clzll(seg0);
            } else {
                const int64_t e = next_set_bit(s_bits, base + 64, total);
                const lk_u64 seg = nn & (~0ull << b);
                a2 = seg ? base + lk_ctz(seg) : next_zero_bit(s_space, base + 64, e);
                e2 = prev_zero_end(s_space, a2, e);
            }
            out[2 * k] = (OUT)(a2 - lo);
            out[2 * k + 1] = (OUT)(e2 - lo);
        }
        ++k;
    }
    // completion word: the host polls it instead of waiting for the end-of-kernel signal to travel through the runtime.
    // One wave wrote everything, its stores leave in order, the fence drains them to system scope before the word follows.
    if (S.done) {
        __threadfence_system();
        if (lane == 0) __hip_atomic_store(S.done, S.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

hipError_t launch_small_batch(const SplitParams& P, bool rules, int kind, bool out32, void* counts, void* items, int8_t* features,
                              int64_t* n_items, unsigned long long* done, unsigned long long seq, hipStream_t st) {
    SmallParams S;
    S.P = P;
    S.counts = counts;
    S.items = items;
    S.features = features;
    S.n_items = n_items;
    S.done = done;
    S.seq = seq;
#define LATOK_SB(M, K, T) hipLaunchKernelGGL((k_small_batch<M, K, T>), dim3(1), dim3(64), 0, st, S)
#define LATOK_SB_K(M, T) do { if (kind == 0) LATOK_SB(M, 0, T); else if (kind == 1) LATOK_SB(M, 1, T); else LATOK_SB(M, 2, T); } while (0)
    if (rules) {
        if (out32) LATOK_SB_K(kModeRules, int32_t); else LATOK_SB_K(kModeRules, int64_t);
    } else {
        if (out32) LATOK_SB_K(kModeBits, int32_t); else LATOK_SB_K(kModeBits, int64_t);
    }
#undef LATOK_SB_K
#undef LATOK_SB
    return hipGetLastError();
}

// _gen_block_mask (latok.c:150-270) of ONE small array pair: the tile function in block-mask mode on a single tile, the
// {any(a1), any(a2)} flags of the reference's element-0 quirk computed by the same wave, the completion word at the end.
__global__ __launch_bounds__(64) void k_small_block_mask(SmallParams S) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kWaveLdsBytes];
    __shared__ int s_flags[2];
    const int lane = threadIdx.x;
    TileLds L;
    L.t1 = L.t2 = L.lut = L.ctab = L.ltab = L.t1b = L.t2b = nullptr; L.tables = nullptr; L.ctl = nullptr;
    L.small_bits = L.small_space = nullptr;
    L.stage = lds;
    L.halo = lds + kStageBytes;
    L.bw = reinterpret_cast<lk_u64*>(lds + kStageBytes + 16);
    SplitParams P = S.P;
    const int64_t n = P.total;
    uint32_t f1 = 0, f2 = 0;
    for (int64_t i = 4 * (int64_t)lane; i < n; i += 256) {
        if (i + 4 <= n) {
            f1 |= *reinterpret_cast<const uint32_t*>(P.bm_a1 + i);
            f2 |= *reinterpret_cast<const uint32_t*>(P.bm_a2 + i);
        } else {
            for (int64_t j = i; j < n; ++j) { f1 |= (uint8_t)P.bm_a1[j]; f2 |= (uint8_t)P.bm_a2[j]; }
        }
    }
    const int any1 = __any(f1 != 0u), any2 = __any(f2 != 0u);
    if (lane == 0) { s_flags[0] = any1; s_flags[1] = any2; }
    wave_lds_sync();
    P.bm_flags = s_flags;
    process_tile<kModeBlockMask, false, true, true>(P, L, 0, 0, 0, -1, false, nullptr, lane);
    if (S.done) {
        __threadfence_system();
        if (lane == 0) __hip_atomic_store(S.done, S.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

hipError_t launch_small_block_mask(const SplitParams& P, unsigned long long* done, unsigned long long seq, hipStream_t st) {
    SmallParams S;
    S.P = P;
    S.counts = S.items = nullptr;
    S.features = nullptr;
    S.n_items = nullptr;
    S.done = done;
    S.seq = seq;
    hipLaunchKernelGGL(k_small_block_mask, dim3(1), dim3(64), 0, st, S);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// stage 0: the per-tile string index.  tile_first[t] = first s in [0, n_str] with row_off[s] >= t * kTile (row_off[n_str]
// = total closes the list).  One thread per entry: entry s is the first string of every tile that begins in
// (row_off[s-1], row_off[s]].  Entries that cover many tiles (a long document, the tail of the batch) are written by
// the whole wave.  ~3 us for 1 M strings; inside k_tiles_main the same work was a ~9 us serial prologue of every segment
// (tables -> row_off window -> barriers -> first tile: three dependent trips to memory before the stream started).
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tile_index(const int64_t* __restrict__ row_off, int64_t n_str, int64_t n_tiles,
                                                   int64_t* __restrict__ tile_first) {
    tile_index_entry(row_off, n_str, n_tiles, tile_first, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, threadIdx.x & 63);
}

hipError_t launch_tile_index(const SplitParams& P, hipStream_t st) {
    if (P.n_tiles <= 0) return hipSuccess;
    const int64_t entries = P.n_str + 1;
    hipLaunchKernelGGL(k_tile_index, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, st, P.row_off, P.n_str, P.n_tiles,
                       P.tile_first);
    return hipGetLastError();
}

void plan_segments(int64_t n_tiles, int n_cu, int* seg_tiles, int64_t* n_segs) {
    // every workgroup gets the same number of (almost) equally sized segments: `rounds` segments of
    // ceil(n_tiles / (n_cu * rounds)) tiles, rounds = smallest count that keeps a segment within kSegMax tiles
    const int64_t per_cu = (n_tiles + n_cu - 1) / n_cu;
    const int64_t rounds = per_cu > kSegMax ? (per_cu + kSegMax - 1) / kSegMax : 1;
    int64_t s = (n_tiles + (int64_t)n_cu * rounds - 1) / ((int64_t)n_cu * rounds);
    // (A segment's tiles go round-robin over the workgroup's kWPB waves, so a length that is not a multiple of kWPB ends in a
    // round with most waves idle.  Rounding long segments to whole rounds was measured for the blocking calls and not kept;
    // the flow picks, among three CU shares, one whose last round is at least half full: api.cpp run_pipeline.)
    if (s < kWPB) s = kWPB;
    if (s > kSegMax) s = kSegMax;
    *seg_tiles = (int)s;
    *n_segs = (n_tiles + s - 1) / s;
}

void plan_launch(int64_t n_tiles, int n_cu, bool in_flow, int mode, bool one_launch_ok, LaunchPlan* L, const PlanForce* force) {
    const int wpb = tile_wpb(mode);
    // A batch of a FLOW leaves part of the chip to the other batch in flight: its persistent tile kernel is planned for 7/8 of
    // the CUs (4 free per XCD on MI355X), so the first workgroups of the NEXT batch's tile kernel start on the free CUs while
    // this one still runs, finish early and free CUs for the batch after it -- the start-up (table copy, first tile) and the
    // ragged end of every tile kernel then overlap another kernel's steady state instead of idling the chip.  Alone, the kernel
    // is as fast on 224 CUs as on 256 (it is memory bound); in the flow C2 goes from 96 to 85.5-87 us per batch.  Measured on
    // C2 (profiles/r03_ab_flow_cus.txt): fewer than 32 free CUs gain nothing (16: 97, 24: 96, 28: 94 us), 32: 85.5-87,
    // 48: 87-90, 64: 87-91, 128 (two kernels side by side on half the chip each): 89.  A segment's tiles go round-robin over
    // the workgroup's 12 waves, so a plan whose last round holds only a wave or two (216 CUs: 145 tiles = 12 rounds + 1 tile:
    // 93-96 us) wastes what the free CUs gain: of the candidate shares the first whose last round is at least half full is taken.
    int n_cu_eff = n_cu;
    if (in_flow && n_cu >= 64) {
        const int cand[3] = {n_cu * 7 / 8, n_cu * 13 / 16, n_cu * 3 / 4};
        int best = cand[0], best_fill = -1;
        for (int c = 0; c < 3; ++c) {
            int st_ = 0;
            int64_t ns_ = 0;
            plan_segments(n_tiles, cand[c], &st_, &ns_);
            const int fill = (st_ - 1) % wpb + 1;                  // waves busy in a segment's last round
            if (fill * 2 >= wpb) { best = cand[c]; break; }
            if (fill > best_fill) { best = cand[c]; best_fill = fill; }
        }
        n_cu_eff = best;
    }
    if (n_cu_eff < 8) n_cu_eff = n_cu < 8 ? n_cu : 8;
    L->n_cu_eff = n_cu_eff;
    plan_segments(n_tiles, n_cu_eff, &L->seg_tiles, &L->n_segs);
    if (force && force->seg_tiles > 0) {
        const int s = force->seg_tiles < kWPB ? kWPB : (force->seg_tiles > kSegMax ? kSegMax : force->seg_tiles);
        L->seg_tiles = s;
        L->n_segs = (n_tiles + s - 1) / s;
        one_launch_ok = false;
    }
    // a small UTF-32 batch: one segment, and one launch for the three stages
    L->one_launch = one_launch_ok && n_tiles <= kOneSegTiles && (mode == kModeBits || mode == kModeRules);
    if (L->one_launch) {
        L->seg_tiles = (int)(n_tiles < kOneSegTiles ? kOneSegTiles : n_tiles);
        L->n_segs = 1;
    }
    // (the plan may leave CUs free; the grid never exceeds the chip)
    L->grid = L->one_launch ? 1 : (int)(L->n_segs < n_cu ? (L->n_segs < 1 ? 1 : L->n_segs) : n_cu);
    if (force && force->grid > 0 && force->grid < L->grid) L->grid = force->grid;
    L->rounds = (L->n_segs + L->grid - 1) / L->grid;
    L->fast_tail = !L->one_launch && n_tiles <= kFastTailTiles && (mode == kModeBits || mode == kModeRules);
    L->pf = mode == kModeBits && in_flow && !L->fast_tail && !L->one_launch ? kCpsPrefetchRowsFlow : kCpsPrefetchRows;
    L->wpb = L->one_launch ? kWPB : wpb;
    L->hold = !L->one_launch && tile_holds(mode) && L->seg_tiles <= kSegHoldTiles && !(force && force->hold == 0);
    // The bitmask modes repair almost everything in place, so their resolve stage is pure latency and runs with as few
    // waves as cover a segment; the modes that recompute tiles keep all 12 waves for that.
    const bool narrow_resolve = mode == kModeBits || mode == kModeBytes || mode == kModeLatin1 || mode == kModeUcs2;
    L->nw = L->one_launch || !narrow_resolve ? kWPB : (L->seg_tiles <= 128 ? 2 : (L->seg_tiles <= 256 ? 4 : kWPB));
}

hipError_t launch_split_tiles(const SplitParams& P, int mode, const LaunchPlan& L, hipStream_t st) {
    const dim3 grid(L.grid), block(kWPB * 64);
    if (L.hold) {
        if (!tile_holds(mode) || P.seg_tiles > kSegHoldTiles) return hipErrorInvalidValue;
        if (mode == kModeBits && L.pf == kCpsPrefetchRowsFlow) hipLaunchKernelGGL((k_tiles_main<kModeBits, false, kCpsPrefetchRowsFlow, true>), grid, block, 0, st, P);
        else if (mode == kModeBits && L.fast_tail) hipLaunchKernelGGL((k_tiles_main<kModeBits, true, kCpsPrefetchRows, true>), grid, block, 0, st, P);
        else if (mode == kModeRules && L.fast_tail) hipLaunchKernelGGL((k_tiles_main<kModeRules, true, kCpsPrefetchRows, true>), grid, block, 0, st, P);
        else if (mode == kModeBits) hipLaunchKernelGGL((k_tiles_main<kModeBits, false, kCpsPrefetchRows, true>), grid, block, 0, st, P);
        else hipLaunchKernelGGL((k_tiles_main<kModeRules, false, kCpsPrefetchRows, true>), grid, block, 0, st, P);
        return hipGetLastError();
    }
    if (mode == kModeBits && L.pf == kCpsPrefetchRowsFlow) hipLaunchKernelGGL((k_tiles_main<kModeBits, false, kCpsPrefetchRowsFlow>), grid, block, 0, st, P);
    else if (mode == kModeBits && L.fast_tail) hipLaunchKernelGGL((k_tiles_main<kModeBits, true>), grid, block, 0, st, P);
    else if (mode == kModeRules && L.fast_tail) hipLaunchKernelGGL((k_tiles_main<kModeRules, true>), grid, block, 0, st, P);
    else if (mode == kModeBits) hipLaunchKernelGGL((k_tiles_main<kModeBits>), grid, block, 0, st, P);
    else if (mode == kModeValues) hipLaunchKernelGGL((k_tiles_main<kModeValues>), grid, block, 0, st, P);
    else if (mode == kModeRules) hipLaunchKernelGGL((k_tiles_main<kModeRules>), grid, block, 0, st, P);
    else if (mode == kModeBytes) hipLaunchKernelGGL((k_tiles_main<kModeBytes>), grid, dim3(tile_wpb(kModeBytes) * 64), 0, st, P);
    else if (mode == kModeLatin1) hipLaunchKernelGGL((k_tiles_main<kModeLatin1>), grid, dim3(tile_wpb(kModeLatin1) * 64), 0, st, P);
    else if (mode == kModeUcs2) hipLaunchKernelGGL((k_tiles_main<kModeUcs2>), grid, dim3(tile_wpb(kModeUcs2) * 64), 0, st, P);
    else if (mode == kModeBytesRules) hipLaunchKernelGGL((k_tiles_main<kModeBytesRules>), grid, block, 0, st, P);
    else if (mode == kModeLatin1Rules) hipLaunchKernelGGL((k_tiles_main<kModeLatin1Rules>), grid, block, 0, st, P);
    else if (mode == kModeUcs2Rules) hipLaunchKernelGGL((k_tiles_main<kModeUcs2Rules>), grid, block, 0, st, P);
    else if (mode == kModeValuesRules) hipLaunchKernelGGL((k_tiles_main<kModeValuesRules>), grid, block, 0, st, P);
    else hipLaunchKernelGGL((k_tiles_main<kModeBlockMask>), grid, block, 0, st, P);
    return hipGetLastError();
}

hipError_t launch_one_segment(const SplitParams& P, int mode, hipStream_t st) {
    if (P.n_segs != 1 || P.seg_tiles < P.n_tiles || P.n_tiles > kOneSegTiles || (mode != kModeBits && mode != kModeRules))
        return hipErrorInvalidValue;
    if (mode == kModeBits) hipLaunchKernelGGL((k_one_segment<kModeBits>), dim3(1), dim3(kWPB * 64), 0, st, P);
    else hipLaunchKernelGGL((k_one_segment<kModeRules>), dim3(1), dim3(kWPB * 64), 0, st, P);
    return hipGetLastError();
}

hipError_t launch_resolve_fix(const SplitParams& P, int mode, const LaunchPlan& L, hipStream_t st) {
    if (L.nw * 64 < P.seg_tiles) return hipErrorInvalidValue;   // one thread per tile of a segment
    const dim3 grid(L.grid), block(kWPB * 64);
    // (byte space: ASCII tiles are repaired in place here too; measured better with few waves on C2 and C3)
#define LATOK_RESOLVE_NW(M)                                                                            \
    if (L.nw == 2) hipLaunchKernelGGL((k_resolve_fix<M, 2>), grid, dim3(128), 0, st, P);               \
    else if (L.nw == 4) hipLaunchKernelGGL((k_resolve_fix<M, 4>), grid, dim3(256), 0, st, P);          \
    else hipLaunchKernelGGL((k_resolve_fix<M, kWPB>), grid, block, 0, st, P)
    if (mode == kModeBits) { LATOK_RESOLVE_NW(kModeBits); }
    else if (mode == kModeValues) hipLaunchKernelGGL((k_resolve_fix<kModeValues, kWPB>), grid, block, 0, st, P);
    else if (mode == kModeRules) hipLaunchKernelGGL((k_resolve_fix<kModeRules, kWPB>), grid, block, 0, st, P);
    else if (mode == kModeBytesRules) hipLaunchKernelGGL((k_resolve_fix<kModeBytesRules, kWPB>), grid, block, 0, st, P);
    else if (mode == kModeLatin1Rules) hipLaunchKernelGGL((k_resolve_fix<kModeLatin1Rules, kWPB>), grid, block, 0, st, P);
    else if (mode == kModeUcs2Rules) hipLaunchKernelGGL((k_resolve_fix<kModeUcs2Rules, kWPB>), grid, block, 0, st, P);
    else if (mode == kModeValuesRules) hipLaunchKernelGGL((k_resolve_fix<kModeValuesRules, kWPB>), grid, block, 0, st, P);
    else if (mode == kModeBytes) { LATOK_RESOLVE_NW(kModeBytes); }
    else if (mode == kModeLatin1) { LATOK_RESOLVE_NW(kModeLatin1); }
    else if (mode == kModeUcs2) { LATOK_RESOLVE_NW(kModeUcs2); }
    else hipLaunchKernelGGL((k_resolve_fix<kModeBlockMask, kWPB>), grid, block, 0, st, P);
#undef LATOK_RESOLVE_NW
    return hipGetLastError();
}

#ifdef LATOK_STAMPS
extern "C" int latok_diag_stamps(unsigned long long* out16, int reset) {
    hipError_t e = hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_stamp_sum), 16 * sizeof(unsigned long long));
    if (reset) {
        unsigned long long z[16] = {0};
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_stamp_sum), z, sizeof(z));
    }
    return (int)e;
}
#endif

}  // namespace latok
