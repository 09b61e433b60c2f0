// tile_core.h -- the tile function of the fused character-feature + split-mask kernels for gfx950 (MI355X, CDNA4).
//
// What the reference does per string with an n x 25 int8 matrix and five passes over it
// (reference latok/core/src/latok/latok.c:31-138 gen_parse_matrix, :275-370 combine_matrix_rows x3, :140-258
// gen_block_mask, glued by latok/core/default_tokenizer.py:113-134) is done here in ONE pass over the packed
// UTF-32 batch, without ever materialising the matrix: 4 B read and 1 bit written per character.
//
// Work decomposition: the packed code-point buffer is cut into fixed tiles of 4096 chars = 64 words of 64 chars.
// One wavefront (64 lanes) owns one tile at a time:
//   phase 1 (lane = 4 consecutive chars, coalesced):  16 x global_load_dwordx4 (1 KiB per wave instruction) ->
//            two-stage Unicode class lookup in LDS -> one 8-bit "split code" per char -> wave-private LDS staging.
//   phase 2 (lane = one 64-char word):  lane reads its 64 code bytes back (4 x ds_read_b128, 80-byte padded rows,
//            conflict-free), bit-slices them into 8 feature planes, and evaluates all rules as 64-bit boolean algebra
//            (lane_math.h).  PREV/NEXT/AFTER_NEXT features are word shifts plus three neighbour bytes from LDS.
//   block mask: exact queue semantics of gen_block_mask via carry-propagating adds; cross-lane state is a (max,+)
//            scan over lanes (forward) and a carry chain over lane ballots (backward).
// Tiles are not string-aligned, so a block (whitespace-delimited span) may straddle tiles.  Each tile is first
// computed assuming no pending start enters it and with a provisional decision for its open tail block, and
// publishes a 16-byte summary (k_tiles_main); k_resolve_fix then resolves the two unknowns per tile exactly (block-wide
// scans over the tile summaries of a segment + the aggregates of the other segments) and repairs the few tiles whose
// assumption was wrong: a patch of the bitmask in place for the common cases, else a recomputation by the same tile
// code with the exact inputs.  Stage 0 (k_tile_index) gives every tile the first string that starts in it.
//
// No MFMA: this is integer/bit work bounded by HBM reads (4 B/char), not a contraction.
//
// Device code only, all of it inlined into its callers: the tile pipeline and the one-launch kernels for small batches
// (split_kernels.hip); feature_kernels.hip borrows TileLds and the wave's staging layout.
#ifndef LATOK_TILE_CORE_H
#define LATOK_TILE_CORE_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "lane_math.h"
#include "utf8_decode.h"
#include "wave_ops.h"

namespace latok {

// Diagnostic build only (-DLATOK_STAMPS): s_memtime stamps at phase boundaries of the tile function, summed per wave and
// added to a global array at the end of the kernel (split_kernels.hip).  Never compiled into the shipped library.
#ifdef LATOK_STAMPS
#define LATOK_STAMP(k)                                                                           \
    do {                                                                                         \
        __builtin_amdgcn_sched_barrier(0);                                                       \
        unsigned long long t_;                                                                   \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");            \
        __builtin_amdgcn_sched_barrier(0);                                                       \
        if ((k) > 0) stamp_acc[(k)] += t_ - stamp_prev;                                          \
        stamp_prev = t_;                                                                         \
    } while (0)
#define LATOK_STAMP_ARG , stamp_acc
#define LATOK_STAMP_PARAM , unsigned long long* stamp_acc
#define LATOK_STAMP_NULL , nullptr
#else
#define LATOK_STAMP(k) do { } while (0)
#define LATOK_STAMP_ARG
#define LATOK_STAMP_PARAM
#define LATOK_STAMP_NULL
#endif

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// staging layout: 64-byte rows padded to 80 bytes: byte p of the tile lives at p + 16 * (p / 64)
__device__ __forceinline__ uint32_t stage_addr(uint32_t p) { return p + ((p >> 6) << 4); }

__device__ __forceinline__ uint32_t classify1(const uint8_t* t1, const uint8_t* t2, uint32_t cp) {
    const uint32_t hi = min(cp >> kTblShift, (uint32_t)(kStage1Len - 1));
    const uint32_t blk = t1[hi];
    return t2[(blk << kTblShift) | (cp & ((1u << kTblShift) - 1u))];
}

// byte space: the same through its own table (stage 1 by cp >> 6 as uint16 block offsets; kernels.h: kB6*)
__device__ __forceinline__ uint32_t classify1_b6(const uint8_t* t1b, const uint8_t* t2b, uint32_t cp) {
    const uint32_t hi = min(cp >> LK_B6_SHIFT, (uint32_t)(kB6Stage1Len - 1));
    const uint32_t off = *reinterpret_cast<const uint16_t*>(t1b + 2u * hi);
    return t2b[off | (cp & 63u)];
}

__device__ __forceinline__ uint32_t classify4(const uint8_t* t1, const uint8_t* t2, u32x4 v, bool* not_ascii = nullptr) {
    // wave-uniform fast path: all 256 chars of this wave instruction are ASCII -> stage-2 block 0, no stage-1 lookup.
    // Either way the four lookups of a table level are requested together (the empty asm pins them): left alone hipcc shares the
    // fourth lookup between the two branches and strings the others along -- two LDS round trips per ASCII row instead of one,
    // five per non-ASCII row instead of two.
    const bool ascii = __all((v.x | v.y | v.z | v.w) < 128u);
    if (not_ascii && !ascii) *not_ascii = true;
    uint32_t c0, c1, c2, c3;
    if (ascii) {
        c0 = t2[v.x]; c1 = t2[v.y]; c2 = t2[v.z]; c3 = t2[v.w];
        asm volatile("" : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3));
    } else {
        const uint32_t last = (uint32_t)(kStage1Len - 1), low = (1u << kTblShift) - 1u;
        uint32_t b0 = t1[min(v.x >> kTblShift, last)], b1 = t1[min(v.y >> kTblShift, last)],
                 b2 = t1[min(v.z >> kTblShift, last)], b3 = t1[min(v.w >> kTblShift, last)];
        asm volatile("" : "+v"(b0), "+v"(b1), "+v"(b2), "+v"(b3));
        c0 = t2[(b0 << kTblShift) | (v.x & low)]; c1 = t2[(b1 << kTblShift) | (v.y & low)];
        c2 = t2[(b2 << kTblShift) | (v.z & low)]; c3 = t2[(b3 << kTblShift) | (v.w & low)];
        asm volatile("" : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3));
    }
    return c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
}

// inclusive scan over the 64 lanes of the queue transfer functions, earlier lanes applied first; (0,0) is neutral
// for the functions that occur here (a <= b, b >= 0)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ lk_qfn qfn_scan_step(lk_qfn inc) {
    lk_qfn o;
    o.a = dpp_mov<CTRL, ROW_MASK>(0, inc.a);
    o.b = dpp_mov<CTRL, ROW_MASK>(0, inc.b);
    return lk_qfn_then(o, inc);
}
__device__ __forceinline__ lk_qfn qfn_wave_scan(lk_qfn f) {
    f = qfn_scan_step<kDppRowShr1, 0xF>(f);
    f = qfn_scan_step<kDppRowShr2, 0xF>(f);
    f = qfn_scan_step<kDppRowShr4, 0xF>(f);
    f = qfn_scan_step<kDppRowShr8, 0xF>(f);
    f = qfn_scan_step<kDppRowBcast15, 0xA>(f);   // rows 1 and 3 take the total of the row before them
    f = qfn_scan_step<kDppRowBcast31, 0xC>(f);   // rows 2 and 3 take the total of rows 0..1
    return f;
}

// ---------------------------------------------------------------------------------------------------------------
// the tile function
// ---------------------------------------------------------------------------------------------------------------
struct TileLds {
    const uint8_t* t1;     // stage-1 table (LDS)
    const uint8_t* t2;     // stage-2 table of split codes (LDS)
    uint8_t* stage;        // kStageBytes, wave private
    uint8_t* halo;         // 16 bytes, wave private
    lk_u64* bw;            // 65 words of string-start bits, wave private
    const uint8_t* lut;    // kModeLatin1: slice LUT (kSliceLutBytes) in place of the Unicode tables
    const uint8_t* ctab;   // kModeLatin1: split code of each of the 256 Latin-1 chars (kModeBytes: the stage-2 block of U+0000, for its ASCII tiles)
    const uint8_t* ltab;   // kModeBytes: decode table of the multi-byte lead bytes (kLeadTabBytes, build_lead_table)
    const uint8_t* t1b;    // kModeBytes: its own class table (kernels.h: kB6*) -- stage 1, uint16 block offsets by cp >> 6 ...
    const uint8_t* t2b;    //             ... and stage 2, 64-entry blocks (t1 / t2 are unused there; ctab = t2b: ASCII is blocks 0, 1)
    uint8_t* tables;       // the workgroup's table area (LDS offset 0) and the two counters of the on-demand table load
    int* ctl;              // (tables_ensure); ctl == nullptr: the kernel reads its tables from global memory
    uint64_t* small_bits;  // k_small_batch: where the tile's boundary / SPACE words go (LDS) in place of P.bits_out /
    uint64_t* small_space; // P.space_out -- the kernel arguments stay where they are (no private copy of the rule tables)
};

// ---------------------------------------------------------------------------------------------------------------
// Latin-1 input: classification and bit-slicing by ONE table.  A lane holds 64 raw bytes; what phase 2 needs from
// them are the 8 planes of their split codes.  Looking a byte up in the code table and then transposing 8 x 64 bits
// with shifts and masks costs ~7 VALU instructions per char; instead the table itself holds the code already spread
// out -- entry c = {lo, hi}: bit 8 b of lo = bit b of code(c) (b < 4), of hi = bit 4 + b -- so that OR-ing the entries
// of 8 consecutive chars, each shifted by its position, gives exactly the byte-per-plane words lk_bitslice64 has
// after its three delta-swap stages.  The shift is folded into the table: 8 pre-shifted copies (2 KiB each), the
// copy is selected by the immediate offset of the LDS instruction -> per char one address computation, two
// ds_read_b32 and one v_or3 shared by two values.  (The narrow-input kernels are VALU-bound, not HBM-bound: 1 B/char
// in, and the rule algebra per char is the same as for UTF-32.)
// ---------------------------------------------------------------------------------------------------------------
constexpr int kSliceHiOff = 1024 + 64;                   // hi[c] sits 16 banks away from lo[c]: the two reads of a char never collide
constexpr int kSliceCopyBytes = kSliceHiOff + 1024;      // {lo[256], pad, hi[256]} as uint32
constexpr int kSliceLutBytes = 8 * kSliceCopyBytes;      // copy j = entries << j
static_assert(kSliceLutBytes + 256 <= kTablesLdsBytes, "the Latin-1 tables live where the Unicode tables would");

constexpr int kSlicePin = 2;   // groups of 8 chars whose lookups are requested together (slice_lut64)
__device__ __forceinline__ void slice_lut64(const uint32_t (&d)[16], const uint8_t* lut, lk_u64 (&plane)[8]) {
    uint32_t lo[8], hi[8];
#pragma unroll
    for (int g = 0; g < 8; ++g) {
        uint32_t l = 0, h = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t w = d[2 * g + (j >> 2)];
            const uint32_t off = ((w >> (8 * (j & 3))) & 0xFFu) << 2;
            const uint8_t* e = lut + j * kSliceCopyBytes + off;
            l |= *reinterpret_cast<const uint32_t*>(e);
            h |= *reinterpret_cast<const uint32_t*>(e + kSliceHiOff);
        }
        lo[g] = l;
        hi[g] = h;
        // pin the words every kSlicePin groups: without it the compiler requests all 128 lookups first (one result
        // register each, spills) and ORs them afterwards
        if ((g + 1) % kSlicePin == 0) {
#pragma unroll
            for (int q = g + 1 - kSlicePin; q <= g; ++q) asm volatile("" : "+v"(lo[q]), "+v"(hi[q]));
        }
    }
    lk_planes_from_groups(lo, hi, plane);
}

// split code of Latin-1 char c from the global tables (U+0000..U+00FF live in the first two stage-2 blocks)
__device__ __forceinline__ uint32_t latin1_code_global(const SplitParams& P, uint32_t c) {
    const uint32_t blk = P.t1[c >> kTblShift];
    return P.t2[(blk << kTblShift) | (c & ((1u << kTblShift) - 1u))];
}

// build [slice LUT | code table] in LDS (NT threads)
template <int NT>
__device__ __forceinline__ void build_latin1_tables(uint8_t* lds, const SplitParams& P) {   // lds = where the LUT goes
    for (int c = threadIdx.x; c < 256; c += NT) {
        const uint32_t code = latin1_code_global(P, (uint32_t)c);
        lds[kSliceLutBytes + c] = (uint8_t)code;
        const uint32_t lo = ((code & 15u) * 0x00204081u) & 0x01010101u;
        const uint32_t hi = ((code >> 4) * 0x00204081u) & 0x01010101u;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            uint32_t* copy = reinterpret_cast<uint32_t*>(lds + j * kSliceCopyBytes);
            copy[c] = lo << j;
            copy[kSliceHiOff / 4 + c] = hi << j;
        }
    }
}

// One tile = 4096 chars, one wave.  (Register prefetch of the next tile -- full, half, quarter; 8/10/12/16 waves per
// CU -- was measured and gives nothing: see DESIGN.md, so the tile function stays simple.)
// idx0 = index of the first string that starts at or after the tile's first char.
// With write_summary the tile summary is written to *summ_l (LDS copy of the segment).
// Returns this lane's 64-bit boundary word (kModeBits); with DEFER the caller stores it later (write combining).
// ---------------------------------------------------------------------------------------------------------------
// kModeBytes: the tile is 4096 BYTES of UTF-8; a char lives at its lead byte.  An all-ASCII tile (the common case) is one
// table lookup per byte.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool u8_is_cont(uint32_t b) { return (b & 0xC0u) == 0x80u; }

// bit i = byte i of the dword has its top bit set (is not ASCII)
__device__ __forceinline__ uint32_t u8_high_nibble(uint32_t w) { return ((((w >> 7) & 0x01010101u) * 0x00204081u) >> 21) & 0xFu; }

// kModeLatin1 / kModeUcs2 (PEP 393 kinds 1 / 2: Latin-1 / UCS-2 code units), phase 1: the tile is 4096 CHARS of 1 or
// 2 bytes each.  Nothing is decoded and there are no continuation bytes, so the staging buffer receives plain codes and
// phase 2 evaluates the char-space rules (lk_rules), exactly like a UTF-32 tile; only the LDS layout is the byte-space one.
// Halo: halo[0] = code of unit t0-1, halo[8], halo[9] = codes of units t0+4096, t0+4097 (0 where there is no such char).
// Returns (KIND 1 only) whether every byte of the tile is ASCII (wave-uniform): phase 2 then classifies without a table.
template <int KIND>
__device__ __forceinline__ bool units_phase1(const SplitParams& P, const TileLds& L, int64_t t0, int lane) {
    const int64_t total = P.total;
    if (lane < 2) *reinterpret_cast<lk_u64*>(L.halo + 8u * lane) = 0ull;
    uint32_t halo_u = 0xFFFFFFFFu;                                              // out of range -> class 0
    if (lane < 3) {
        const int64_t hp = lane == 0 ? t0 - 1 : t0 + kTile + (lane - 1);
        if (hp >= 0 && hp < total)
            halo_u = KIND == 1 ? (uint32_t)P.u8[hp] : (uint32_t)reinterpret_cast<const uint16_t*>(P.u8)[hp];
    }
    if (KIND == 1) {
        // Latin-1: the RAW bytes go to the staging buffer (phase 2 classifies and bit-slices them with one table,
        // slice_lut64); only the three halo chars are classified here
        u32x4 v[4];
        if (t0 + kTile <= total) {
            const u32x4* src = reinterpret_cast<const u32x4*>(P.u8 + t0) + lane;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = __builtin_nontemporal_load(src + 64 * i);
        } else {
#pragma unroll 1
            for (int i = 0; i < 4; ++i) {
                uint32_t d[4] = {0, 0, 0, 0};
                const int64_t p = t0 + 1024 * i + 16 * lane;
                for (int j = 0; j < 16; ++j)
                    if (p + j < total) d[j >> 2] |= (uint32_t)P.u8[p + j] << (8 * (j & 3));
                v[i].x = d[0]; v[i].y = d[1]; v[i].z = d[2]; v[i].w = d[3];
            }
        }
        wave_lds_sync();   // the zero stores to the halo are ordered before the halo stores below
        // positions past the end of the batch hold unit 0 here; their codes are masked by `valid` in phase 2
#pragma unroll
        for (int i = 0; i < 4; ++i)
            *reinterpret_cast<uint4*>(L.stage + stage_addr(1024u * i + 16u * lane)) = make_uint4(v[i].x, v[i].y, v[i].z, v[i].w);
        if (lane < 3 && halo_u != 0xFFFFFFFFu) L.halo[lane == 0 ? 0 : 7 + lane] = L.ctab[halo_u & 0xFFu];
        uint32_t hi_bits = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) hi_bits |= (v[i].x | v[i].y | v[i].z | v[i].w) & 0x80808080u;
        return __all(hi_bits == 0u);
    } else {
        // UCS-2: 8 units per 16-byte load, row i of the tile = units 512 i + 8 lane ..
        u32x4 v[8];
        if (t0 + kTile <= total) {
            const u32x4* src = reinterpret_cast<const u32x4*>(reinterpret_cast<const uint16_t*>(P.u8) + t0) + lane;
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = __builtin_nontemporal_load(src + 64 * i);
        } else {
            const uint16_t* __restrict__ u16 = reinterpret_cast<const uint16_t*>(P.u8);
#pragma unroll 1
            for (int i = 0; i < 8; ++i) {
                uint32_t d[4] = {0, 0, 0, 0};   // units past the end read as 0, like the bytes of a UTF-8 tail tile
                const int64_t p = t0 + 512 * i + 8 * lane;
                for (int j = 0; j < 8; ++j)
                    if (p + j < total) d[j >> 1] |= (uint32_t)u16[p + j] << (16 * (j & 1));
                v[i].x = d[0]; v[i].y = d[1]; v[i].z = d[2]; v[i].w = d[3];
            }
        }
        wave_lds_sync();
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint32_t d[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
            uint32_t lo, hi;
            if (__all(((d[0] | d[1] | d[2] | d[3]) & 0xFF80FF80u) == 0u)) {      // 512 ASCII chars: stage-2 block of U+0000
                const uint32_t off0 = (uint32_t)L.t1[0] << kTblShift;
                lo = (uint32_t)L.t2[off0 + (d[0] & 0xFFFFu)] | ((uint32_t)L.t2[off0 + (d[0] >> 16)] << 8) |
                     ((uint32_t)L.t2[off0 + (d[1] & 0xFFFFu)] << 16) | ((uint32_t)L.t2[off0 + (d[1] >> 16)] << 24);
                hi = (uint32_t)L.t2[off0 + (d[2] & 0xFFFFu)] | ((uint32_t)L.t2[off0 + (d[2] >> 16)] << 8) |
                     ((uint32_t)L.t2[off0 + (d[3] & 0xFFFFu)] << 16) | ((uint32_t)L.t2[off0 + (d[3] >> 16)] << 24);
            } else {
                lo = classify1(L.t1, L.t2, d[0] & 0xFFFFu) | (classify1(L.t1, L.t2, d[0] >> 16) << 8) |
                     (classify1(L.t1, L.t2, d[1] & 0xFFFFu) << 16) | (classify1(L.t1, L.t2, d[1] >> 16) << 24);
                hi = classify1(L.t1, L.t2, d[2] & 0xFFFFu) | (classify1(L.t1, L.t2, d[2] >> 16) << 8) |
                     (classify1(L.t1, L.t2, d[3] & 0xFFFFu) << 16) | (classify1(L.t1, L.t2, d[3] >> 16) << 24);
            }
            *reinterpret_cast<uint2*>(L.stage + stage_addr(512u * i + 8u * lane)) = make_uint2(lo, hi);
        }
        if (lane < 3 && halo_u != 0xFFFFFFFFu) L.halo[lane == 0 ? 0 : 7 + lane] = (uint8_t)classify1(L.t1, L.t2, halo_u);
    }
    return false;
}

// ---------------------------------------------------------------------------------------------------------------
// Class tables on demand (k_tiles_main, byte space).  A workgroup used to copy its tables to LDS before its first tile: 60 KB
// per CU from L2 with nothing else in flight, ~2 us at the head of every launch -- for tables that a batch of ASCII text never
// reads beyond the 128 codes of U+0000..U+007F.  Now the launch copies those 128 bytes, and the first wave that meets a
// multi-byte char brings in the rest: the copy is cut into kLazyGrabs pieces handed out by an LDS counter, so every wave that
// arrives while it is under way takes a share (text that is not ASCII anywhere: all twelve at once, as fast as before), and a
// second counter says when the last piece is in place.  Waves that find both counters full pay one LDS read per tile.
// (Both counters count LANES, 64 per piece: every lane of the wave executes the same atomic -- hipcc folds them into one
// ds_add of 64 per wave -- so no lane-0 branch surrounds the wave-wide copy instructions.)
// ---------------------------------------------------------------------------------------------------------------
constexpr int kLazyPer = 4;                                    // 1 KiB rows (one global_load_lds_dwordx4 of the wave each) per piece

constexpr int kLazyRows = kB6TablesBytes / 1024;                 // byte space: [stage 1 | stage 2], then (computed, the last piece) the byte decode table
constexpr int kLazyGrabs = (kLazyRows + kLazyPer - 1) / kLazyPer + 1;
__device__ __attribute__((noinline, cold)) void tables_fetch_bytes(const uint8_t* t1, const uint8_t* t2, uint8_t* tables, int* ctl);
__device__ __forceinline__ void tables_ensure_bytes(const SplitParams& P, const TileLds& L, int lane) {
    if (L.ctl == nullptr) return;
    if (__hip_atomic_load(&L.ctl[1], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) >= 64 * kLazyGrabs) return;
    tables_fetch_bytes(P.t1, P.t2, L.tables, L.ctl);
}

// kModeBytes, phase 1 (lane = 16 consecutive bytes per 1 KiB row).  What reaches the staging buffer: the split code of
// its char at every LEAD byte (any non-continuation byte), the marker LK_CODE_CONT at continuation bytes (the continuation
// plane of a word then falls out of phase 2's bit-slicing).  Nothing is carried from lane to lane: the continuation bytes take their owner's code in phase 2, as
// mask arithmetic on the word's planes (lane_math.h: lk_smear_planes).  An ASCII byte is one table lookup; only the
// NON-ASCII LEAD bytes are decoded and classified through the two-stage table -- two slots per dword (well-formed UTF-8
// has at most two multi-byte leads in 4 bytes), all eight slots of a row independent and branch-free so that their LDS
// lookups overlap; a dword with more (malformed input) takes a wave-uniform loop afterwards.
// Halo: halo[0] = code of the char that owns byte t0-1, halo[4] = how many more continuation bytes it may take,
// halo[8..15] = staging bytes of the 8 bytes after the tile.
// the window of slot (dword Q, lead mask m within the dword): its 4 bytes and where in the dword the lead sits
// the window of a slot of dword Q: m = lead mask within the dword in "bit 7 of the byte" form; the slot takes its lowest
// lead: *r8_out = the bit position of that byte in the dword, returns the 4 bytes from there on
// ---------------------------------------------------------------------------------------------------------------
// kModeBytes: class of a multi-byte char straight from its bytes (lane_math.h: lk_lead_index has the scheme).  The code point is
// never assembled: byte space has its own two-stage class table cut at 6 bits, so stage 1 wants "every byte but the last" and
// stage 2 the last byte's payload.  Per decode slot: one ds_read_b64 of the 8-byte entry of the window's first byte, v_perm,
// v_dot4_u32_u8 (the stage-1 offset), a clamp, the "cut short" test (2), ds_read_u16, v_and_or (stage-2 index), ds_read_u8 --
// 7 VALU instructions where utf8_cp_of + classify1 took 27 and the 7-bit table (hi = cp >> 7, lo = cp & 127 by shifts and masks)
// 15.  Same results as utf8_cp_of + classify1: a sequence cut short is U+FFFD, overlong / surrogate forms decode as they are,
// 0xF8..0xFF are 4-byte leads with 3 payload bits.  The table has an entry for EVERY byte value: a slot that holds no lead
// decodes whatever byte its window starts at, and the entries below 0xC0 yield code 0 (nothing to OR into the staging bytes).
// ---------------------------------------------------------------------------------------------------------------
constexpr int kLeadTabBytes = 256 * 8;
template <int NT>
__device__ __forceinline__ void build_lead_table(uint8_t* lds) {
    for (int i = threadIdx.x; i < 256; i += NT) {
        const lk_lead_entry e = lk_lead_entry_of((uint32_t)i);
        reinterpret_cast<uint2*>(lds)[i] = make_uint2(e.sel, e.hi0);
    }
}
// the entry of the byte a slot's window W starts with
__device__ __forceinline__ uint2 lead_entry(const uint8_t* ltab, uint32_t W) {
    return *reinterpret_cast<const uint2*>(ltab + ((W & 0xFFu) << 3));
}
// W = the 4 bytes from a slot's first byte on (memory order), q = its entry: *off2 = byte offset of the char's stage-1 entry
// (clamped), *R = the sequence in lk_lead_index's order (low 6 bits = stage-2 index); returns whether the sequence is cut short
__device__ __forceinline__ bool lead_index(uint2 q, uint32_t W, uint32_t* off2, uint32_t* R) {
    lk_lead_entry e;
    e.sel = q.x; e.hi0 = q.y;
    uint32_t o;
    const bool bad = lk_lead_index(e, W, &o, R);
    *off2 = min(o, 2u * (uint32_t)(kB6Stage1Len - 1));
    return bad;
}

template <int Q>
__device__ __forceinline__ uint32_t bytes_slot_window(const uint32_t (&w)[5], uint32_t m, uint32_t* r8_out) {
    const uint32_t r8 = (uint32_t)__builtin_ctz(m | 0x80000000u) & 24u;   // bit position of the byte; m == 0: byte 3, whatever it is
    *r8_out = r8;
    return __builtin_amdgcn_alignbit(w[Q + 1], w[Q], r8);
}

// byte space: the halo bytes of the tile at t0 -- lane 0: the dword before the tile, lanes 1..11: the 11 bytes after it
__device__ __forceinline__ uint32_t bytes_halo_load(const uint8_t* __restrict__ u8, int64_t t0, int64_t total, int lane) {
    uint32_t hb = 0;
    if (lane == 0) {
        if (t0 > 0) hb = *reinterpret_cast<const uint32_t*>(u8 + t0 - 4);
    } else if (lane < 12) {
        const int64_t q = t0 + kTile + (lane - 1);
        if (q < total) hb = u8[q];
    }
    return hb;
}

// kCpsPrefetchRows (kernels.h): rows (1 KiB) of the wave's next UTF-32 tile requested before phase 2 of the current one
// ... and in the tile kernel of a FLOW batch (two batches in flight, each planned for 7/8 of the CUs): six.  Same box, R = 2 / 4 / 5 / 6:
// C2 through the flow 1 424 / 1 434 / 1 439 / 1 448 GB/s (sustained 1 472 / 1 487 / 1 489 / 1 500), C3 2 450 -> 2 585 (+5 %) -- but
// one batch at a time 1 213 -> 1 205 on C2, 2 306 -> 2 266 on C3, the isolated kernel 94.5 -> 95.2 us: the depth that pays while another
// kernel shares the memory system costs a little when the kernel is alone, so the launch scheme picks the instantiation
// (kCpsPrefetchRowsFlow, kernels.h).
constexpr int kCpsPrefetchMax = kCpsPrefetchRowsFlow;
struct CpsPrefetch {
    u32x4 v[kCpsPrefetchMax];
    bool valid;
};

__device__ __forceinline__ bool bytes_phase1(const SplitParams& P, const TileLds& L, int64_t t0, int lane
#ifdef LATOK_STAMPS
                                             , unsigned long long* stamp_acc, unsigned long long& stamp_prev
#endif
                                             ) {
    const int64_t total = P.total;
    const uint8_t* __restrict__ u8 = P.u8;
    // halo bytes: lane 0 holds the dword before the tile (t0 is a multiple of 4096 and u8 is 16-byte aligned; byte j of it
    // = byte t0 - 4 + j), lanes 1..11 the 11 bytes after the tile (0 where the batch has ended).  Requested BEFORE the rows: loads
    // come back in order, and the decision below wants the halo and row 0 only.
    uint32_t hb = bytes_halo_load(u8, t0, total, lane);
    // the tile: 4 x 16 bytes per lane (row i covers bytes 1024 i + 16 lane ..)
    u32x4 v[4];
    if (t0 + kTile <= total) {
        const u32x4* src = reinterpret_cast<const u32x4*>(u8 + t0) + lane;
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = __builtin_nontemporal_load(src + 64 * i);
    } else {
#pragma unroll 1
        for (int i = 0; i < 4; ++i) {
            uint32_t d[4] = {0, 0, 0, 0};
            const int64_t p = t0 + 1024 * i + 16 * lane;
            for (int j = 0; j < 16; ++j)
                if (p + j < total) d[j >> 2] |= (uint32_t)u8[p + j] << (8 * (j & 3));
            v[i].x = d[0]; v[i].y = d[1]; v[i].z = d[2]; v[i].w = d[3];
        }
    }
    // All-ASCII tiles take their own road, which needs all four rows; a tile whose row 0 already holds a multi-byte char does not
    // wait for the others to find that out.  (Requesting row 0 and the halo bytes of the wave's NEXT tile during phase 2 was
    // measured on top of this: C3 0.505 -> 0.515 ms, C2 0.073 -> 0.077; the 16 extra bytes of scratch cost more than the wait.)
    uint32_t hi_bits = (hb | v[0].x | v[0].y | v[0].z | v[0].w) & 0x80808080u;
    if (__all(hi_bits == 0u)) {
#pragma unroll
        for (int i = 1; i < 4; ++i) hi_bits |= (v[i].x | v[i].y | v[i].z | v[i].w) & 0x80808080u;
    }
    if (lane < 2) *reinterpret_cast<lk_u64*>(L.halo + 8u * lane) = 0ull;
    const bool all_ascii = __all(hi_bits == 0u);
    wave_lds_sync();   // the zero stores are ordered before everything below
    LATOK_STAMP(11);   // (share of stamp 2: the tile's bytes have arrived)

    if (all_ascii) {
        // no multi-byte char in or around the tile (the common case): the RAW bytes go to the staging buffer and phase 2
        // classifies and bit-slices them with one table (slice_lut64), exactly like a Latin-1 tile
#pragma unroll
        for (int i = 0; i < 4; ++i)
            *reinterpret_cast<uint4*>(L.stage + stage_addr(1024u * i + 16u * lane)) = make_uint4(v[i].x, v[i].y, v[i].z, v[i].w);
        if (lane == 0 && t0 > 0) L.halo[0] = L.ctab[hb >> 24];
        if (lane >= 1 && lane < 9 && t0 + kTile + (lane - 1) < total) L.halo[8 + (lane - 1)] = L.ctab[hb & 0xFFu];
        return true;
    }

    tables_ensure_bytes(P, L, lane);   // from here on the whole class table is read, not just its ASCII part
    // The char that owns byte t0-1: its lead is byte t0-k, k = 1..4 (further back: nobody owns it).  The 8 bytes
    // t0-4 .. t0+3 sit in lane 0's registers; every lane computes (no divergence), lane 0 stores.
    {
        const bool c1 = u8_is_cont(hb >> 24), c2 = u8_is_cont((hb >> 16) & 0xFFu), c3 = u8_is_cont((hb >> 8) & 0xFFu);
        const uint32_t k = !c1 ? 1u : (!c2 ? 2u : (!c3 ? 3u : 4u));
        const lk_u64 Z = (lk_u64)hb | ((lk_u64)v[0].x << 32);
        const uint32_t W = (uint32_t)(Z >> (8u * (4u - k)));
        const uint32_t b0 = W & 0xFFu;
        const uint32_t code = classify1_b6(L.t1b, L.t2b, b0 < 0x80u ? b0 : utf8_cp_of(W));
        if (lane == 0 && t0 > 0 && !u8_is_cont(b0)) {
            L.halo[0] = (uint8_t)code;
            L.halo[4] = (uint8_t)(4u - k);
        }
    }

    const uint32_t code_fffd = classify1_b6(L.t1b, L.t2b, 0xFFFDu);   // a sequence that is cut short
    LATOK_STAMP(12);   // (share of stamp 2: owner of the byte before the tile)
    // R rows (1 KiB each) per round, every stage over all of them: the table lookups of a round -- R x 16 ASCII, then R x 8 per
    // level of the multi-byte decode (byte entry, stage 1, stage 2) -- are in flight together, so a round is four trips to the
    // LDS whatever R is.  (Stamped build on C3: the rows were 3.7 K clocks each for ~250 VALU instructions -- the wave sat in the
    // LDS latency of one row at a time.)
    constexpr int R = 1;   // (2 rows per round: 128 B more scratch, 0.505 -> 0.56 ms on C3; 4: 0.78 KB of scratch, 1.4 ms)
#pragma unroll
    for (int i0 = 0; i0 < 4; i0 += R) {
        uint32_t d[R][4], out[R][4];
#pragma unroll
        for (int a = 0; a < R; ++a) { d[a][0] = v[i0 + a].x; d[a][1] = v[i0 + a].y; d[a][2] = v[i0 + a].z; d[a][3] = v[i0 + a].w; }
        // every byte as if it were a char of its own: one lookup each in code[256] (the ASCII codes; 0 from 0x80 on, so the
        // positions of multi-byte chars come back empty)
#pragma unroll
        for (int a = 0; a < R; ++a) {
            // all 16 lookups of the row requested before the first one is used: left to itself hipcc keeps two or three in flight
            // (a register each), and the row waits for the LDS eight times instead of once
            uint32_t c[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) c[k] = L.ctab[(d[a][k >> 2] >> (8 * (k & 3))) & 0xFFu];
            asm volatile("" : "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]), "+v"(c[4]), "+v"(c[5]), "+v"(c[6]), "+v"(c[7]),
                              "+v"(c[8]), "+v"(c[9]), "+v"(c[10]), "+v"(c[11]), "+v"(c[12]), "+v"(c[13]), "+v"(c[14]), "+v"(c[15]));
#pragma unroll
            for (int j = 0; j < 4; ++j) out[a][j] = c[4 * j] | (c[4 * j + 1] << 8) | (c[4 * j + 2] << 16) | (c[4 * j + 3] << 24);
        }
        uint32_t any_hi = 0;
#pragma unroll
        for (int a = 0; a < R; ++a) any_hi |= (d[a][0] | d[a][1] | d[a][2] | d[a][3]) & 0x80808080u;
        if (__all(any_hi == 0u)) {        // these rows are pure ASCII
#pragma unroll
            for (int a = 0; a < R; ++a)
                *reinterpret_cast<uint4*>(L.stage + stage_addr(1024u * (i0 + a) + 16u * lane)) = make_uint4(out[a][0], out[a][1], out[a][2], out[a][3]);
            continue;
        }
        // bytes 16..18 after my chunk: the next lane's first dword; lane 63: lane 0's next row, or the bytes after the tile
        uint32_t w[R][5];
#pragma unroll
        for (int a = 0; a < R; ++a) {
            const int i = i0 + a;
            uint32_t nx = (uint32_t)dpp_mov<kDppWaveShl1, 0xF>(0, (int)d[a][0]);
            const uint32_t wrap = i < 3 ? (uint32_t)lane_read((int)v[(i + 1) & 3].x, 0)
                                        : ((uint32_t)lane_read((int)hb, 1) | ((uint32_t)lane_read((int)hb, 2) << 8) |
                                           ((uint32_t)lane_read((int)hb, 3) << 16));
            if (lane == 63) nx = wrap;
            w[a][0] = d[a][0]; w[a][1] = d[a][1]; w[a][2] = d[a][2]; w[a][3] = d[a][3]; w[a][4] = nx;
        }
        // Per dword, all masks in "bit 7 of the byte" form (no bit gathering): hi = not ASCII, cont = 10xxxxxx, nl = the
        // leads that need a decode.  (Bytes past the end of the batch were loaded as 0: ASCII, never a continuation.)
        uint32_t m1[R][4], m2[R][4], rest[R][4];
#pragma unroll
        for (int a = 0; a < R; ++a)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t hi = d[a][q] & 0x80808080u;
                const uint32_t cont = hi & ~(d[a][q] << 1);
                out[a][q] |= cont;                                              // ASCII codes | LK_CODE_CONT at continuation bytes
                m1[a][q] = hi ^ cont;
                m2[a][q] = m1[a][q] & (m1[a][q] - 1u);
                rest[a][q] = m2[a][q] & (m2[a][q] - 1u);                        // leads beyond two per dword (malformed input)
            }
        {
            // stage by stage over the 8 R slots (slot s < 4: the first lead of dword s, else the second of dword s - 4)
            uint32_t r8[R][8], W[R][8], off2[R][8], Rs[R][8], blk[R][8], code[R][8];
            bool bad[R][8];
#pragma unroll
            for (int a = 0; a < R; ++a) {
                W[a][0] = bytes_slot_window<0>(w[a], m1[a][0], &r8[a][0]);
                W[a][1] = bytes_slot_window<1>(w[a], m1[a][1], &r8[a][1]);
                W[a][2] = bytes_slot_window<2>(w[a], m1[a][2], &r8[a][2]);
                W[a][3] = bytes_slot_window<3>(w[a], m1[a][3], &r8[a][3]);
                W[a][4] = bytes_slot_window<0>(w[a], m2[a][0], &r8[a][4]);
                W[a][5] = bytes_slot_window<1>(w[a], m2[a][1], &r8[a][5]);
                W[a][6] = bytes_slot_window<2>(w[a], m2[a][2], &r8[a][6]);
                W[a][7] = bytes_slot_window<3>(w[a], m2[a][3], &r8[a][7]);
            }
            // (the eight entries requested together, like the ASCII lookups above: left alone hipcc reads, waits and decodes slot by slot)
            static_assert(R == 1, "the pin below names the entries of one row");
            uint2 ent[R][8];
#pragma unroll
            for (int a = 0; a < R; ++a)
#pragma unroll
                for (int s = 0; s < 8; ++s) ent[a][s] = lead_entry(L.ltab, W[a][s]);
            asm volatile("" : "+v"(ent[0][0].x), "+v"(ent[0][0].y), "+v"(ent[0][1].x), "+v"(ent[0][1].y), "+v"(ent[0][2].x), "+v"(ent[0][2].y),
                              "+v"(ent[0][3].x), "+v"(ent[0][3].y), "+v"(ent[0][4].x), "+v"(ent[0][4].y), "+v"(ent[0][5].x), "+v"(ent[0][5].y),
                              "+v"(ent[0][6].x), "+v"(ent[0][6].y), "+v"(ent[0][7].x), "+v"(ent[0][7].y));
#pragma unroll
            for (int a = 0; a < R; ++a)
#pragma unroll
                for (int s = 0; s < 8; ++s)
                    bad[a][s] = lead_index(ent[a][s], W[a][s], &off2[a][s], &Rs[a][s]);
#pragma unroll
            for (int a = 0; a < R; ++a)
#pragma unroll
                for (int s = 0; s < 8; ++s) blk[a][s] = *reinterpret_cast<const uint16_t*>(L.t1b + off2[a][s]);
#pragma unroll
            for (int a = 0; a < R; ++a)
#pragma unroll
                for (int s = 0; s < 8; ++s) code[a][s] = L.t2b[blk[a][s] | (Rs[a][s] & 0x3Fu)];
            // A slot without a lead decoded the dword's last byte: an ASCII or continuation byte gives code 0 (its table entry),
            // a lead -- then the dword's first or second lead -- its own code once more, at its own place: OR-ing is right either way.
#pragma unroll
            for (int a = 0; a < R; ++a)
#pragma unroll
                for (int s = 0; s < 8; ++s) out[a][s & 3] |= code[a][s] << r8[a][s];
            // Sequences that are cut short (malformed input) are U+FFFD: looked for once per row, wave-wide, instead of a compare
            // and a select per slot; the rare row that holds one puts U+FFFD's code in place of what the slot looked up.
            bool any_bad = false;
#pragma unroll
            for (int a = 0; a < R; ++a)
#pragma unroll
                for (int s = 0; s < 8; ++s) any_bad = any_bad || bad[a][s];
            if (__any(any_bad)) {
#pragma unroll
                for (int a = 0; a < R; ++a)
#pragma unroll
                    for (int s = 0; s < 8; ++s)
                        if (bad[a][s]) out[a][s & 3] = (out[a][s & 3] & ~(0xFFu << r8[a][s])) | (code_fffd << r8[a][s]);
            }
        }
#pragma unroll
        for (int a = 0; a < R; ++a) {
            while (__any((rest[a][0] | rest[a][1] | rest[a][2] | rest[a][3]) != 0u)) {   // wave-uniform; never taken on well-formed UTF-8
                uint32_t r8[4], cp[4];
                cp[0] = utf8_cp_of(bytes_slot_window<0>(w[a], rest[a][0], &r8[0]));
                cp[1] = utf8_cp_of(bytes_slot_window<1>(w[a], rest[a][1], &r8[1]));
                cp[2] = utf8_cp_of(bytes_slot_window<2>(w[a], rest[a][2], &r8[2]));
                cp[3] = utf8_cp_of(bytes_slot_window<3>(w[a], rest[a][3], &r8[3]));
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    out[a][q] |= (rest[a][q] ? classify1_b6(L.t1b, L.t2b, cp[q]) : 0u) << r8[q];
                    rest[a][q] &= rest[a][q] - 1u;
                }
            }
            *reinterpret_cast<uint4*>(L.stage + stage_addr(1024u * (i0 + a) + 16u * lane)) = make_uint4(out[a][0], out[a][1], out[a][2], out[a][3]);
        }
    }
    LATOK_STAMP(13);   // (share of stamp 2: the four rows)
    // the 8 bytes after the tile -> halo[8..15] as staging bytes (code at a lead, LK_CODE_CONT at a continuation byte).
    // Lane k+1 owns byte k.
    {
        const int k = lane - 1;
        const bool in_win = lane >= 1 && lane < 9 && t0 + kTile + k < total;
        // the 3 bytes after mine (lanes 2..11 hold them; 0 = "no such byte", which is not a continuation byte)
        const uint32_t b1 = (uint32_t)dpp_mov<kDppWaveShl1, 0xF>(0, (int)hb) & 0xFFu;
        const uint32_t b2 = (uint32_t)dpp_mov<kDppWaveShl1, 0xF>(0, (int)b1) & 0xFFu;
        const uint32_t b3 = (uint32_t)dpp_mov<kDppWaveShl1, 0xF>(0, (int)b2) & 0xFFu;
        const uint32_t W = (hb & 0xFFu) | (b1 << 8) | (b2 << 16) | (b3 << 24);
        const uint32_t b0 = W & 0xFFu;
        const uint32_t my_code = classify1_b6(L.t1b, L.t2b, b0 < 0x80u ? b0 : utf8_cp_of(W));
        if (in_win) L.halo[8 + k] = (uint8_t)(u8_is_cont(b0) ? LK_CODE_CONT : my_code);
    }
    return false;
}

// byte space, phase 2: what a word needs from its surroundings -- the staging bytes of the 8 bytes after it (lane 63: the
// halo), whether one of them is a continuation byte, the string starts after it, and the owner state in front of it (the
// last four staging bytes of the row before; lane 0: the halo)
__device__ __forceinline__ void bytes_word_context(const TileLds& L, int lane, lk_halo_bytes* hb, bool* next_has_cont, uint32_t* own_code,
                                                   int* own_left) {
    hb->next_codes = lane < 63 ? *reinterpret_cast<const lk_u64*>(L.stage + 80u * lane + 80u) : *reinterpret_cast<const lk_u64*>(L.halo + 8);
    hb->next_B = (uint32_t)(L.bw[lane + 1] & 0xFFFFull);
    const lk_u64 y = hb->next_codes ^ 0x8080808080808080ull;          // a byte equals LK_CODE_CONT
    *next_has_cont = (~(((y & 0x7F7F7F7F7F7F7F7Full) + 0x7F7F7F7F7F7F7F7Full) | y) & 0x8080808080808080ull) != 0ull;
    lk_owner_before(lane > 0 ? *reinterpret_cast<const uint32_t*>(L.stage + 80u * lane - 20u) : 0u, own_code, own_left);
    if (lane == 0) {
        *own_code = L.halo[0];
        *own_left = L.halo[4];
    }
    hb->prev = *own_code;
}
// Phase 2 of a tile (lane = one 64-char word): everything after the code bytes, the halo codes and the string-start
// words are in the wave's LDS buffer L.  (A separate function because a producer / consumer variant of the kernel ran
// the two phases in different waves; see DESIGN.md, negative results.)
template <int MODE, bool DEFER = false, bool SMALL = false>
__device__ __forceinline__ lk_u64 tile_phase2(const SplitParams& P, const TileLds& L, int64_t t, int q_in, int tail_zero,
                                            bool write_summary, int4* summ_l, int lane, bool raw_stage, bool ascii_tile
#ifdef LATOK_STAMPS
                                            , unsigned long long* stamp_acc, unsigned long long& stamp_prev
#endif
                                            ) {
    const int64_t t0 = t * kTile;
    const int64_t total = P.total;
    // ---- phase 2: lane = one 64-char word ---------------------------------------------------------------------
    const lk_u64 B = L.bw[lane];
    const int64_t base = t0 + 64 * (int64_t)lane;
    lk_local loc;
    lk_rule_counts counts;    // kModeValuesRules only: rows of C_SPLIT / C_SYM that hold at each char
    lk_u64 space_plane = 0;   // SPACE plane for the token-span passes (byte mode: smeared over continuation bytes)
    lk_u64 cont_plane = 0;    // byte mode: continuation bytes of my word (P.lead_out)
    int no_patch = 0;         // byte mode: the tile holds multi-byte chars: the one bit a patch of the resolve stage keeps (the C_SYM
                              // bit of a block's last char) sits at that char's LEAD byte, which the stage finds in the bytes
    if (MODE == kModeBlockMask) {
        // a1 -> start plane, a2 -> space plane; 64 bytes each, non-zero = set (PyArray_Nonzero, latok.c:178,198)
        lk_u64 st = 0, sp = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int64_t p = base + 4 * k;
            uint32_t w1 = 0, w2 = 0;
            if (p + 4 <= total) {
                w1 = *reinterpret_cast<const uint32_t*>(P.bm_a1 + p);
                w2 = *reinterpret_cast<const uint32_t*>(P.bm_a2 + p);
            } else {
                for (int b = 0; b < 4; ++b)
                    if (p + b < total) {
                        w1 |= (uint32_t)(uint8_t)P.bm_a1[p + b] << (8 * b);
                        w2 |= (uint32_t)(uint8_t)P.bm_a2[p + b] << (8 * b);
                    }
            }
            // byte != 0 -> one bit per byte -> 4-bit nibble
            const uint32_t n1 = ((((w1 & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w1) & 0x80808080u) >> 7;
            const uint32_t n2 = ((((w2 & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w2) & 0x80808080u) >> 7;
            st |= (lk_u64)(((n1 * 0x00204081u) >> 21) & 0xFu) << (4 * k);
            sp |= (lk_u64)(((n2 * 0x00204081u) >> 21) & 0xFu) << (4 * k);
        }
        loc.start = st;
        loc.S = sp;
        loc.raw = ~0ull;
        loc.sym = 0;
        loc.t_space = loc.t_sym = loc.t_prevsym = loc.t_camel_next = loc.t_camel_prev = 0;
    } else {
        uint32_t d[16];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint4 q = *reinterpret_cast<const uint4*>(L.stage + 80u * lane + 16u * k);   // == stage_addr(64 lane + 16 k)
            d[4 * k + 0] = q.x; d[4 * k + 1] = q.y; d[4 * k + 2] = q.z; d[4 * k + 3] = q.w;
        }
        lk_halo h;
        // neighbours of the word in the padded layout: stage_addr(64 lane - 1) = 80 lane - 17, (64 lane + 64) = 80 lane + 80
        h.prev = lane > 0 ? L.stage[80u * lane - 17u] : L.halo[0];
        h.next0 = lane < 63 ? L.stage[80u * lane + 80u] : L.halo[1];
        h.next1 = lane < 63 ? L.stage[80u * lane + 81u] : L.halo[2];
        const lk_u64 Bn = L.bw[lane + 1] & 3ull;
        lk_u64 plane[8];
        if (mode_base(MODE) == kModeLatin1 || (mode_base(MODE) == kModeBytes && raw_stage)) {
            // d = raw bytes: classify + slice through the LUT; the neighbour bytes become codes through the code table
            LATOK_STAMP(9);    // (share of stamp 4: the four ds_read_b128 + neighbour bytes)
            if (ascii_tile) {
                // all 4096 bytes are ASCII: bit-slice the raw bytes and derive the code planes as boolean functions of the
                // raw planes -- no table, nothing through the LDS pipe (128 ds_read_b32 per word otherwise, which hit a bank
                // twice in ~90 % of the passes and kept the pipe busy for about half of a tile round)
                lk_u64 rawp[8];
                lk_bitslice64(d, rawp);
                lk_ascii_code_planes<mode_rules(MODE)>(rawp, plane);
            } else {
                slice_lut64(d, L.lut, plane);   // (Latin-1 tiles with chars >= 0x80; a raw byte-space tile is always ASCII)
            }
            LATOK_STAMP(10);   // (share of stamp 4: LUT slicing)
            h.prev = lane > 0 ? L.ctab[h.prev] : h.prev;
            h.next0 = lane < 63 ? L.ctab[h.next0] : h.next0;
            h.next1 = lane < 63 ? L.ctab[h.next1] : h.next1;
        } else {
            lk_bitslice64(d, plane);
        }
        if (mode_is_units(MODE)) {
            // one code per char like a UTF-32 tile, in the byte-space layout: the two chars after my row are the next row's
            // first codes (lane 63: halo[8], halo[9])
            lk_halo ha;
            ha.prev = h.prev;
            ha.next0 = lane < 63 ? h.next0 : L.halo[8];
            ha.next1 = lane < 63 ? h.next1 : L.halo[9];
            if (mode_rules(MODE)) loc = lk_rules_generic(plane, ha, B, Bn, P.rules);   // (the staging bytes are rule codes then)
            else loc = lk_rules(lk_decode(plane), ha, B, Bn);
            space_plane = loc.S;
        } else if (mode_base(MODE) == kModeBytes && raw_stage) {
            // all-ASCII tile: byte positions are char positions, the plain rules apply (codes of the neighbours: above)
            lk_halo ha;
            ha.prev = h.prev;
            ha.next0 = lane < 63 ? h.next0 : L.halo[8];
            ha.next1 = lane < 63 ? h.next1 : L.halo[9];
            if (mode_rules(MODE)) loc = lk_rules_generic(plane, ha, B, Bn, P.rules);
            else loc = lk_rules(lk_decode(plane), ha, B, Bn);
            space_plane = loc.S;
        } else if (mode_base(MODE) == kModeBytes) {
            // byte space: the continuation bytes carry LK_CODE_CONT -> continuation plane of my word
            const lk_u64 C = lk_take_cont_plane(plane);
            cont_plane = C;
            lk_halo_bytes hb;
            bool next_has_cont;
            uint32_t own_code;
            int own_left;
            bytes_word_context(L, lane, &hb, &next_has_cont, &own_code, &own_left);
            no_patch = __ballot(C != 0ull || next_has_cont) != 0ull;
            if (!no_patch) {
                // no multi-byte char in or right after the tile: positions are chars, the plain rules apply
                lk_halo ha;
                ha.prev = h.prev;
                ha.next0 = (uint32_t)(hb.next_codes & 0xFFull);
                ha.next1 = (uint32_t)((hb.next_codes >> 8) & 0xFFull);
                if (mode_rules(MODE)) loc = lk_rules_generic(plane, ha, B, Bn, P.rules);
                else loc = lk_rules(lk_decode(plane), ha, B, Bn);
                space_plane = loc.S;
            } else if (mode_rules(MODE)) {
                // run-time rule tables in byte space: every NEXT_* / AFTER_NEXT_* column through the next-lead operator
                lk_smear_planes<0x37u>(plane, C, own_code, own_left);
                hb.prev = own_code;
                loc = lk_rules_generic_bytes(plane, C, hb, B, P.rules, &space_plane);
            } else if (__ballot(lk_rules_bytes_weird(plane, C, hb.next_codes)) == 0ull) {
                // codes sit at lead bytes only: give the continuation bytes their owner's code in the planes the PREV_*
                // columns and the token stripping read (SPACE, SYMBOL, LOWER, ALPHA_NUM, ALPHA = bits 0, 1, 2, 4, 5)
                lk_smear_planes<0x37u>(plane, C, own_code, own_left);
                hb.prev = own_code;
                loc = lk_rules_bytes_fast(plane, C, hb, B, &space_plane);
            } else {
                // a continuation byte right after '#' '$' '^' '@' ':' '/' '.' somewhere in the tile (malformed UTF-8): the
                // general form.  (Inlined: round 3 had it as a __noinline__ call for the sake of the hot loop's registers, which
                // cost a 240-byte scratch frame; without the write-combining buffer the kernel holds both forms in 168 VGPRs, 0 B scratch.)
                lk_smear_planes<0x37u>(plane, C, own_code, own_left);
                hb.prev = own_code;
                loc = lk_rules_bytes_general(plane, C, hb, B, &space_plane);
            }
        } else if (mode_rules(MODE)) {
            loc = lk_rules_generic(plane, h, B, Bn, P.rules, MODE == kModeValuesRules ? &counts : nullptr);
        } else {
            const lk_feat f = lk_decode(plane);
            loc = lk_rules(f, h, B, Bn);
        }
    }
    LATOK_STAMP(4);
    lk_fwd fw = lk_forward(loc.start, loc.S, B);

    // forward: inclusive (max,+) scan of the per-word queue transfer functions over the 64 lanes
    const lk_qfn inc = qfn_wave_scan(lk_qfn_of(fw));
    lk_qfn exc;   // exclusive: the function of lanes 0..lane-1 (identity for lane 0)
    exc.a = dpp_mov<kDppWaveShr1, 0xF>(0, inc.a);
    exc.b = dpp_mov<kDppWaveShr1, 0xF>(0, inc.b);
    const int r = lk_qfn_apply(exc, q_in);
    lk_qfn tile_fn;
    tile_fn.a = lane_read(inc.a, 63);
    tile_fn.b = lane_read(inc.b, 63);
    if (r > 0) lk_apply_extra(fw, r);
    LATOK_STAMP(5);

    if (write_summary) {
        const lk_u64 cl = loc.S | B;                       // closing events of my word
        const lk_u64 closing_lanes = __ballot(cl != 0);
        const int first_lane = closing_lanes ? lk_ctz(closing_lanes) : 64;
        const int contrib = lane < first_lane ? lk_popc(loc.start) : (lane == first_lane ? fw.head_starts : 0);
        const int head = __ballot(contrib != 0) ? wave_sum(contrib) : 0;   // starts are rare: usually no sum needed
        // geometry of the two blocks that straddle the tile edges, so that the scan stage can patch the common cases
        // in place instead of recomputing the tile:
        //   c_rel : first closing event (4096 if none)       -> head block = [0, c_rel)
        //   p_rel : first char of the open tail block          -> tail block = [p_rel, 4096)
        //   head_sym / tail_sym : the one position of each block that can carry a C_SYM bit (its last char)
        //   tail_keep : the tail block begins with a string start (its bit stays 1)
        int c_rel = kTile, p_rel = 0, tail_keep = 0;
        if (closing_lanes) {
            const int last_lane = 63 - __builtin_clzll(closing_lanes);
            const int my_first = cl ? 64 * lane + lk_ctz(cl) : 0;
            const int top = cl ? 63 - __builtin_clzll(cl) : 0;
            const int s_top = (int)((loc.S >> top) & 1ull);
            c_rel = lane_read(my_first, first_lane);
            p_rel = lane_read(64 * lane + top + s_top, last_lane);
            tail_keep = lane_read(1 - s_top, last_lane);
        }
        int head_sym, tail_sym;
        if (mode_base(MODE) == kModeBytes && no_patch) {   // (wave-uniform; tiles without multi-byte chars take the char form below)
            // A block holds no closing event, and C_SYM = SYMBOL & NEXT_SPACE is set only in front of one: the only C_SYM bit a block
            // can hold is its last char's, wherever that char's lead byte is -- "any C_SYM bit in the block" is the flag.
            const int64_t lo_w = 64 * (int64_t)lane;
            const lk_u64 in_head = c_rel >= lo_w + 64 ? ~0ull : (c_rel <= lo_w ? 0ull : ((1ull << (c_rel - lo_w)) - 1ull));
            const lk_u64 in_tail = p_rel <= lo_w ? ~0ull : (p_rel >= lo_w + 64 ? 0ull : (~0ull << (p_rel - lo_w)));
            head_sym = __ballot((loc.sym & in_head) != 0ull) != 0ull;
            tail_sym = __ballot((loc.sym & in_tail) != 0ull) != 0ull;
        } else {
            const int hs_pos = c_rel > 0 ? c_rel - 1 : 0;
            head_sym = c_rel > 0 ? lane_read((int)((loc.sym >> (hs_pos & 63)) & 1ull), hs_pos >> 6) : 0;
            tail_sym = lane_read((int)(loc.sym >> 63), 63);
        }
        if (lane == 0) {
            const int geom = (closing_lanes != 0) | (c_rel << 1) | (p_rel << 14) | (head_sym << 27) | (tail_keep << 28) |
                             (tail_sym << 29) | (no_patch << 30);
            *summ_l = make_int4(tile_fn.a, tile_fn.b, head, geom);   // LDS; the segment publishes them in one burst
        }
    }

    // backward: zeroing closings clear the block below them; the carry chain over lanes is one 64-bit add on ballots
    LATOK_STAMP(6);
    const lk_u64 zall = fw.zs | fw.zb;
    const int z0_next = dpp_mov<kDppWaveShl1, 0xF>(0, (int)(zall & 1ull));   // lane 63 gets 0
    const lk_bwd bw = lk_backward_prepare(zall, loc.S, B, z0_next);
    const int tz = tail_zero >= 0 ? tail_zero : (lk_qfn_apply(tile_fn, q_in) > 0);
    // chain order is lane 63 -> 0, so reverse the ballots: bit i' = lane 63 - i'
    const lk_u64 G = lk_rev(__ballot(bw.g)), Pm = lk_rev(__ballot(bw.p));
    const lk_u64 X = G | Pm, Y = G;
    const lk_u64 carries_in = (X + Y + (lk_u64)tz) ^ X ^ Y;
    const int cin = (int)((carries_in >> (63 - lane)) & 1ull);
    const lk_u64 cleared = lk_backward_fill(bw, cin, loc.S);

    LATOK_STAMP(7);
    lk_u64 out_word = 0;
    if (base < total) {
        const int64_t remain = total - base;
        const lk_u64 valid = remain >= 64 ? ~0ull : ((1ull << remain) - 1ull);
        const lk_u64 keep = ~cleared;
        if (mode_writes_bits(MODE)) {
            out_word = ((loc.raw & keep) | loc.sym | B) & valid;
            uint64_t* const bits_out = SMALL ? L.small_bits : P.bits_out;
            uint64_t* const space_out = SMALL ? L.small_space : P.space_out;
            if (!DEFER) bits_out[base >> 6] = out_word;
            if (space_out) space_out[base >> 6] = (mode_is_bytes(MODE) ? space_plane : loc.S) & valid;   // token-span mode only
        } else {
            // kModeValues: split VALUES 0..5 = (sum of the five C_SPLIT terms) * mask + C_SYM term; string start = 1
            // kModeBlockMask: the 1/0 block mask itself; element 0 follows the reference's quirk (never zeroed on the
            //   general path because "previous space" starts at 0, latok.c:224; zero only when there is no space at all)
            uint8_t* dst = P.values_out + base;
            const int n = remain >= 64 ? 64 : (int)remain;
#pragma unroll 1
            for (int w = 0; w < 16; ++w) {
                uint32_t packed = 0;
                if (MODE == kModeBlockMask) {
                    packed = ((uint32_t)((keep >> (4 * w)) & 0xFull) * 0x00204081u) & 0x01010101u;
                    if (base == 0 && w == 0) {
                        const int first = (P.bm_flags[0] != 0 && P.bm_flags[1] == 0) ? 0 : 1;
                        packed = (packed & ~0xFFu) | (uint32_t)first;
                    }
                } else {
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const int i = 4 * w + b;
                        int v, vy;
                        if (MODE == kModeValuesRules) {
                            // what the reference returns for ANY tables: (number of C_SPLIT rows that hold) * mask + (number
                            // of C_SYM rows that hold), default_tokenizer.py:121-132 over latok.c:329-338
                            v = vy = 0;
#pragma unroll
                            for (int c = 0; c < LK_COUNT_BITS; ++c) {
                                v |= (int)((counts.split[c] >> i) & 1) << c;
                                vy |= (int)((counts.sym[c] >> i) & 1) << c;
                            }
                        } else {
                            v = (int)((loc.t_space >> i) & 1) + (int)((loc.t_sym >> i) & 1) + (int)((loc.t_prevsym >> i) & 1) +
                                (int)((loc.t_camel_next >> i) & 1) + (int)((loc.t_camel_prev >> i) & 1);
                            vy = (int)((loc.sym >> i) & 1);
                        }
                        v = ((keep >> i) & 1) ? v : 0;
                        v += vy;
                        if ((B >> i) & 1) v = 1;
                        packed |= (uint32_t)v << (8 * b);
                    }
                }
                if (4 * w + 4 <= n) {
                    *reinterpret_cast<uint32_t*>(dst + 4 * w) = packed;
                } else {
                    for (int b = 0; b < 4 && 4 * w + b < n; ++b) dst[4 * w + b] = (uint8_t)(packed >> (8 * b));
                }
            }
        }
    }
    if (mode_base(MODE) == kModeBytes && !SMALL && P.lead_out) {
        // code-point results (k_lead_compress): the lead bytes of my word, how many leads the tile has before it, leads per tile
        const int64_t remain = total - base;
        const lk_u64 valid = remain >= 64 ? ~0ull : (remain <= 0 ? 0ull : ((1ull << remain) - 1ull));
        const lk_u64 leadw = ~cont_plane & valid;
        const int cnt = lk_popc(leadw);
        int inc = cnt;
        inc += dpp_mov<kDppRowShr1, 0xF>(0, inc);
        inc += dpp_mov<kDppRowShr2, 0xF>(0, inc);
        inc += dpp_mov<kDppRowShr4, 0xF>(0, inc);
        inc += dpp_mov<kDppRowShr8, 0xF>(0, inc);
        inc += dpp_mov<kDppRowBcast15, 0xA>(0, inc);
        inc += dpp_mov<kDppRowBcast31, 0xC>(0, inc);
        if (base < total) {
            P.lead_out[base >> 6] = leadw;
            P.lead_pref_out[base >> 6] = (uint16_t)(inc - cnt);
        }
        if (lane == 63) P.lead_cnt_out[t] = inc;
    }
    LATOK_STAMP(8);
    wave_lds_sync();  // staging buffer is reused by this wave's next tile
    return out_word;
}

// UTF-32 bitmask mode: the first R rows (1 KiB each) of the wave's NEXT tile are requested into registers right
// before phase 2 of the current one, so that the wave has loads in flight while it computes.  The wait counts are explicit
// (a vmcnt(0) on every path in front of the requests; the pass that inserts waits otherwise drains the queue at the first
// register it loses track of, and the prefetch silently does nothing).  Measured on C2, same box, twice: kernel 96.1-96.3 ->
// 94.4-94.5 us with R = 2 (R = 1: 93.9-94.1, R = 4: 95-99), step 106.6-107.3 -> 105.0-105.1; C3 / C4 / C5 within their noise
// (profiles/r03_ab_headline_prefetch.txt).

template <int MODE, bool DEFER = false, bool SMALL = false, bool FAST_TAIL = false, int PF = kCpsPrefetchRows>
__device__ __forceinline__ lk_u64 process_tile(const SplitParams& P, const TileLds& L, int64_t t, int64_t idx0, int q_in,
                                             int tail_zero, bool write_summary, int4* summ_l, int lane
#ifdef LATOK_STAMPS
                                             , unsigned long long* stamp_acc = nullptr
#endif
                                             , CpsPrefetch* pf = nullptr, int64_t t_next = -1
                                             ) {
#ifdef LATOK_STAMPS
    unsigned long long stamp_prev = 0, stamp_dummy[16];
    if (!stamp_acc) stamp_acc = stamp_dummy;
#endif
    const int64_t t0 = t * kTile;
    const int64_t total = P.total;
    const uint32_t st_lane = 4u * lane + 16u * ((uint32_t)lane >> 4);   // stage_addr(4 lane); row i adds 320 i
    bool raw_stage = mode_base(MODE) == kModeLatin1;   // the staging buffer holds raw bytes, not codes (Latin-1; all-ASCII tiles of byte mode)
    bool ascii_tile = false;                // ... and every one of them is ASCII (wave-uniform)
    bool tile_not_ascii = false;            // UTF-32: some row of the tile took the two-stage lookup (wave-uniform)
    LATOK_STAMP(0);

    // small loads first, so that their latency flies together with the 16 KiB of code points: the start offsets of
    // the next 64 strings and the three halo characters
    int64_t ro = idx0 + lane <= P.n_str ? P.row_off[idx0 + lane] : INT64_MAX;
    uint32_t halo_cp = 0xFFFFFFFFu;   // out of range -> class 0
    if (MODE != kModeBlockMask && !mode_is_bytes(MODE) && lane < 3) {
        const int64_t hp = lane == 0 ? t0 - 1 : t0 + kTile + (lane - 1);
        if (hp >= 0 && hp < total) halo_cp = P.cps[hp];
    }

    // ---- phase 1: classify 4096 chars, 4 per lane per step, into the staging buffer --------------------------
    if (MODE == kModeBlockMask) {
        // planes come straight from the caller's byte arrays (compat _gen_block_mask): nothing to classify
    } else if (mode_base(MODE) == kModeLatin1) {
        ascii_tile = units_phase1<1>(P, L, t0, lane);
    } else if (mode_base(MODE) == kModeUcs2) {
        units_phase1<2>(P, L, t0, lane);
    } else if (mode_base(MODE) == kModeBytes) {
        raw_stage = bytes_phase1(P, L, t0, lane
#ifdef LATOK_STAMPS
                                 , stamp_acc, stamp_prev
#endif
                                 );
        ascii_tile = raw_stage;
    } else if (FAST_TAIL) {
        // Small batches: the batch's last, partial tile takes the same road as a full one -- only the rows of 256 chars that
        // exist are requested, all of them before the first table lookup; chars that do not exist read as 0 and their
        // codes are masked to 0 ("nothing") -- because its latency is a visible share of the call: a one-tile batch with
        // its chars in host memory (k_small_batch) spent most of its 13 us in the 16 serial load -> lookup rounds of the
        // general form below, a 4-tile batch on the pinned path 15 of its 31 us.  (Not for large batches: the shared
        // loop costs the full-tile path 16 VGPRs and 4 % on C2.)
        const bool full = t0 + kTile <= total;
        u32x4 v[16];
        const u32x4* src = reinterpret_cast<const u32x4*>(P.cps + t0) + lane;
        const int64_t remain0 = total - t0 - 4 * (int64_t)lane;       // chars that exist from my first char on (row 0)
        int n_rows = 16;
        if (full) {
#pragma unroll
            for (int i = 0; i < 16; ++i) v[i] = __builtin_nontemporal_load(src + 64 * i);
        } else {
            // One 16-byte load per existing row and lane, nothing divergent around it and no zero-fill before it (a divergent
            // x4 / scalar-tail choice, or a register write the compiler cannot order against loads in flight, makes it wait
            // for outstanding loads between the rows: they would arrive one by one again).  A lane beyond the end re-reads
            // the 16-byte block that holds the last char; a lane whose 4 chars straddle the end reads up to 12 bytes past
            // the last char inside that block (cps is 16-byte aligned: the same page).  The codes of chars that do not
            // exist are masked below.
            const int64_t last_blk = (total - 1) & ~(int64_t)3;
            n_rows = (int)((total - t0 + 255) >> 8);                  // wave-uniform, 1..16
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                if (i < n_rows) {
                    int64_t p = t0 + 256 * i + 4 * (int64_t)lane;
                    p = p < last_blk ? p : last_blk;
                    v[i] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(P.cps + p));
                }
            }
        }
        uint32_t* codes = P.codes_out ? reinterpret_cast<uint32_t*>(P.codes_out + t0) + lane : nullptr;   // wave-uniform
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            uint32_t c = 0;
            if (i < n_rows) {
                c = classify4(L.t1, L.t2, v[i]);
                if (!full) {
                    const int64_t remain = remain0 - 256 * i;
                    c &= remain >= 4 ? 0xFFFFFFFFu : (remain <= 0 ? 0u : ((1u << (8 * (int)remain)) - 1u));
                }
            }
            *reinterpret_cast<uint32_t*>(L.stage + st_lane + 320u * i) = c;   // == stage_addr(256 i + 4 lane)
            if (codes) codes[64 * i] = c;
        }
    } else if (t0 + kTile <= total) {
        u32x4 v[16];
        const u32x4* src = reinterpret_cast<const u32x4*>(P.cps + t0) + lane;
        constexpr int R = PF;
        const bool pre = R > 0 && pf && pf->valid;      // wave-uniform
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (i < R && pre) v[i] = pf->v[i < R ? i : 0];
            else v[i] = __builtin_nontemporal_load(src + 64 * i);
        }
        LATOK_STAMP(1);
        uint32_t* codes = P.codes_out ? reinterpret_cast<uint32_t*>(P.codes_out + t0) + lane : nullptr;   // wave-uniform
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t c = classify4(L.t1, L.t2, v[i], &tile_not_ascii);
            *reinterpret_cast<uint32_t*>(L.stage + st_lane + 320u * i) = c;   // == stage_addr(256 i + 4 lane)
            if (codes) codes[64 * i] = c;                                     // 256 contiguous bytes per wave instruction
        }
    } else {
        // the batch's last, partial tile of a large batch (its code bytes are written up to the end of the tile: 0 behind
        // the last char)
        uint32_t* codes = P.codes_out ? reinterpret_cast<uint32_t*>(P.codes_out + t0) + lane : nullptr;
#pragma unroll 1
        for (int i = 0; i < 16; ++i) {
            const int64_t p = t0 + 256 * i + 4 * lane;
            u32x4 v;
            v.x = p + 0 < total ? P.cps[p + 0] : 0xFFFFFFFFu;   // out of range -> class 0 ("nothing")
            v.y = p + 1 < total ? P.cps[p + 1] : 0xFFFFFFFFu;
            v.z = p + 2 < total ? P.cps[p + 2] : 0xFFFFFFFFu;
            v.w = p + 3 < total ? P.cps[p + 3] : 0xFFFFFFFFu;
            const uint32_t c = classify4(L.t1, L.t2, v);
            *reinterpret_cast<uint32_t*>(L.stage + st_lane + 320u * i) = c;   // == stage_addr(256 i + 4 lane)
            if (codes) codes[64 * i] = c;
        }
    }
    // halo chars t0-1, t0+4096, t0+4097 (lanes 0..2) and the string-start words
    if (MODE != kModeBlockMask && !mode_is_bytes(MODE) && lane < 3) L.halo[lane] = (uint8_t)classify1(L.t1, L.t2, halo_cp);
    L.bw[lane] = 0;
    if (lane == 0) L.bw[64] = 0;
    LATOK_STAMP(2);
    wave_lds_sync();
    for (;;) {
        const int64_t rel = ro - t0;
        if (rel >= 0 && rel < kTile + 64) atomicOr(&L.bw[rel >> 6], 1ull << (rel & 63));
        const int64_t last = lane_read64(ro, 63);
        if (last >= t0 + kTile + 64) break;
        idx0 += 64;
        ro = idx0 + lane <= P.n_str ? P.row_off[idx0 + lane] : INT64_MAX;
    }
    wave_lds_sync();
    LATOK_STAMP(3);
    if (MODE == kModeBits && pf) {
        __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): every load of this tile has been consumed -- said on every path
        pf->valid = false;
        const bool want = true;
        if (want && t_next >= 0 && (t_next + 1) * kTile <= total) {
            const u32x4* nsrc = reinterpret_cast<const u32x4*>(P.cps + t_next * kTile) + lane;
#pragma unroll
            for (int i = 0; i < PF; ++i) pf->v[i] = __builtin_nontemporal_load(nsrc + 64 * i);
            pf->valid = true;
        }
    }

    return tile_phase2<MODE, DEFER, SMALL>(P, L, t, q_in, tail_zero, write_summary, summ_l, lane, raw_stage, ascii_tile
#ifdef LATOK_STAMPS
                                    , stamp_acc, stamp_prev
#endif
                                    );
}

}  // namespace latok
#endif
