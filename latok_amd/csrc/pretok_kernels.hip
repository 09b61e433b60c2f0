// pretok_kernels.hip -- GPT-2's pre-tokenizer as the front of the byte-space token calls (pretok.h; the definition: include/latok_hip.h,
// latok_pretokens_utf8_bytes_batch).  ONE launch over the batch's bytes writes what the three launches of the tile pipeline leave for a
// token call: the boundary plane (a bit at every byte where a pre-token starts), the SPACE plane (all zero: k_word_counts<true> then
// keeps every pre-token and no span is stripped) and the per-tile string index.  Everything behind the planes is the token calls' own.
//
// The rule has no carry (pretok.h: a start bit depends on the bytes from 7 behind it to 6 ahead of it), so there are no segments, no
// aggregates and no resolve launch: one wave per tile of 4096 bytes, lane = word of 64 bytes, and every lane computes its word alone
// from a window of the word and kPtHalo = 16 bytes on either side.
//   (a) the wave copies its tile and the two halos into LDS with coalesced 16-byte loads, in rows of 64 bytes + 16 bytes of padding
//       (the stride of 80 bytes keeps the lanes' 16-byte reads of (c) off each other's banks);
//   (b) the strings that start in [tile - 64, tile + 4096 + 64) and the batch's end become bits of a 66-word bitmap in LDS (one
//       atomicOr each); the entries below the tile are counted on the way, which gives tile_first[tile] without a launch of its own;
//   (c) lane = word: six 16-byte LDS reads are its window, three bitmap words its string starts; pt_word_starts does the rest.  A word
//       without a byte >= 0x80 in its window touches no table; every other character costs two dependent loads from the 7.5 KiB class
//       tables, which live in global memory and stay in the caches.
// Bytes outside the batch read as 0, and the bits of positions outside the batch are stored as 0.  All stores are plain vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bitscan.h"
#include "kernels.h"
#include "pretok.h"
#include "spbpe.h"
#include "wave_ops.h"

namespace latok {

#define PRETOK_TABLE __device__ const
#include "pretok_tables.inc"

constexpr int kPretokRow = 80;                                  // bytes of one LDS row: 64 of the tile + 16 of padding
constexpr int kPretokRows = kTile / 64 + 2;                     // the tile's rows, the row that ends with the halo in front, the one that begins with the halo behind
constexpr int kPretokMapWords = kTile / 64 + 2;                 // string-start bits over [tile - 64, tile + 4096 + 64)
static_assert(kPtHalo == 16 && kPtWord == 64 && kTile == 64 * kPtWord, "one wave, one tile; one lane, one word; a halo is one 16-byte load");

// byte `o` of the wave's LDS image, o = tile-relative position + 64
__device__ __forceinline__ int pretok_lds_at(int o) { return o + ((o >> 6) << 4); }

struct PretokWindow {
    uint64_t q[kPtWindow / 8];
    const uint8_t* lds;     // the wave's image
    int o0;                 // image position of the window's byte 0
    __device__ __forceinline__ uint64_t qword(int j) const { return q[j]; }
    __device__ __forceinline__ uint32_t byte(int i) const { return lds[pretok_lds_at(o0 + i)]; }
};

// sixteen bytes at batch position p (a multiple of 16; the buffer is 16-byte aligned), bytes outside [0, total) as 0
__device__ __forceinline__ uint4 pretok_load16(const uint8_t* __restrict__ u8, int64_t p, int64_t total) {
    if (p >= 0 && p + 16 <= total) return *reinterpret_cast<const uint4*>(u8 + p);
    uint32_t d[4] = {0u, 0u, 0u, 0u};
    if (p >= 0)
        for (int i = 0; i < 16 && p + i < total; ++i) d[i >> 2] |= (uint32_t)u8[p + i] << (8 * (i & 3));
    return make_uint4(d[0], d[1], d[2], d[3]);
}

__global__ __launch_bounds__(kPretokWaves * 64) void k_pretok_planes(const uint8_t* __restrict__ u8, int64_t total, const int64_t* __restrict__ row_off,
                                                                     int64_t n_str, uint64_t* __restrict__ bits, uint64_t* __restrict__ space,
                                                                     int64_t* __restrict__ tile_first) {
    __shared__ __attribute__((aligned(16))) uint8_t image_s[kPretokWaves][kPretokRows * kPretokRow];
    __shared__ unsigned long long map_s[kPretokWaves][kPretokMapWords];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t t = (int64_t)blockIdx.x * kPretokWaves + wave;
    const int64_t t0 = t * kTile;
    if (t0 >= total) return;                                    // whole wave (no workgroup barrier below)
    uint8_t* image = image_s[wave];
    unsigned long long* map = map_s[wave];
    // (a) the tile and its halos
#pragma unroll
    for (int j = 0; j < kTile / (64 * 16); ++j) {
        const int c = lane + 64 * j;                            // 16-byte chunk of the tile
        *reinterpret_cast<uint4*>(image + pretok_lds_at(64 + 16 * c)) = pretok_load16(u8, t0 + 16 * c, total);
    }
    if (lane == 0) *reinterpret_cast<uint4*>(image + pretok_lds_at(64 - 16)) = pretok_load16(u8, t0 - 16, total);
    if (lane == 1) *reinterpret_cast<uint4*>(image + pretok_lds_at(64 + kTile)) = pretok_load16(u8, t0 + kTile, total);
    // (b) the string starts around the tile; row_off[n_str] = total closes the list and is a start bit like the others
    map[lane] = 0ull;
    if (lane < kPretokMapWords - 64) map[64 + lane] = 0ull;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int64_t m0 = t0 - 64;
    int64_t first = wave_lower_bound(row_off, n_str + 1, m0, lane);   // (the first entry at or behind m0)
    int64_t below = 0;                                          // entries of [first, ..) in front of the tile
    for (int64_t i0 = first; i0 <= n_str; i0 += 64) {
        const int64_t sidx = i0 + lane;
        const int64_t ro = sidx <= n_str ? row_off[sidx] : INT64_MAX;
        const int64_t rel = ro - m0;
        if (rel >= 0 && rel < 64 * kPretokMapWords) atomicOr(&map[rel >> 6], 1ull << (rel & 63));
        below += __popcll(__ballot(ro < t0));
        if (__shfl(ro, 63) >= m0 + 64 * kPretokMapWords) break;
    }
    if (lane == 0) tile_first[t] = min(first + below, n_str);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // (c) my word
    const int64_t w = t * 64 + lane;
    if (w * 64 >= total) return;
    PretokWindow win;
    win.lds = image;
    win.o0 = 64 + 64 * lane - kPtHalo;
#pragma unroll
    for (int j = 0; j < kPtWindow / 16; ++j) {
        const uint4 v = *reinterpret_cast<const uint4*>(image + pretok_lds_at(win.o0 + 16 * j));
        win.q[2 * j] = (uint64_t)v.x | ((uint64_t)v.y << 32);
        win.q[2 * j + 1] = (uint64_t)v.z | ((uint64_t)v.w << 32);
    }
    // the window begins at bit 64 - kPtHalo of map word `lane`
    const pt_u128 B = (pt_u128)(map[lane] >> (64 - kPtHalo)) | ((pt_u128)map[lane + 1] << kPtHalo) | ((pt_u128)map[lane + 2] << (64 + kPtHalo));
    const PretokTables T{kPretokStage1, kPretokStage2, PRETOK_TABLE_LIMIT};
    bits[w] = pt_word_starts(win, B, T) & valid_mask(w, total);
    space[w] = 0ull;
}

// ---- the cl100k / Llama 3 rule (pretok.h, second half) ----------------------------------------------------------------------------------
// The same geometry, image and string-start map, but the rule has four carries (d, absorbed, notopen, nl_ahead), so there are TWO
// launches, and the text is read twice:
//   k_pretok_cl100k_records   every lane forms its word's record from the class planes, the wave composes the 64 with nine ballots and
//                             lane 0 stores ONE 4-byte record per tile
//   k_pretok_cl100k_planes    the wave first resolves what enters its tile: it composes the records of the 64 tiles in front of it
//                             (one per lane, nine ballots), and the 64 before those while a carry still passes -- 256 KiB of run per step,
//                             one step for anything but a run of that length -- and likewise forwards for nl_ahead.  Then every lane
//                             takes its own carries from the tile's and the in-wave records by the same ballots, and finishes its word.
// No workgroup waits for another (the records are complete when the second launch starts), no lane reads text outside its window, and
// only tile records are walked serially.  All stores are plain vector stores.

// (a) and (b) of k_pretok_planes; returns the tile's string index
__device__ __forceinline__ int64_t pretok_stage(const uint8_t* __restrict__ u8, int64_t total, const int64_t* __restrict__ row_off, int64_t n_str, int64_t t0,
                                                int lane, uint8_t* image, unsigned long long* map) {
#pragma unroll
    for (int j = 0; j < kTile / (64 * 16); ++j) {
        const int c = lane + 64 * j;
        *reinterpret_cast<uint4*>(image + pretok_lds_at(64 + 16 * c)) = pretok_load16(u8, t0 + 16 * c, total);
    }
    if (lane == 0) *reinterpret_cast<uint4*>(image + pretok_lds_at(64 - 16)) = pretok_load16(u8, t0 - 16, total);
    if (lane == 1) *reinterpret_cast<uint4*>(image + pretok_lds_at(64 + kTile)) = pretok_load16(u8, t0 + kTile, total);
    map[lane] = 0ull;
    if (lane < kPretokMapWords - 64) map[64 + lane] = 0ull;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int64_t m0 = t0 - 64;
    const int64_t first = wave_lower_bound(row_off, n_str + 1, m0, lane);
    int64_t below = 0;
    for (int64_t i0 = first; i0 <= n_str; i0 += 64) {
        const int64_t sidx = i0 + lane;
        const int64_t ro = sidx <= n_str ? row_off[sidx] : INT64_MAX;
        const int64_t rel = ro - m0;
        if (rel >= 0 && rel < 64 * kPretokMapWords) atomicOr(&map[rel >> 6], 1ull << (rel & 63));
        below += __popcll(__ballot(ro < t0));
        if (__shfl(ro, 63) >= m0 + 64 * kPretokMapWords) break;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    return min(first + below, n_str);
}

// my word's planes and its record; a word behind the batch's end has the record "every carry is 0"
__device__ __forceinline__ uint32_t pretok_cl100k_word(const uint8_t* image, const unsigned long long* map, int lane, bool live, PtCl& c) {
    if (!live) return kPtRecZero;
    PretokWindow win;
    win.lds = image;
    win.o0 = 64 + 64 * lane - kPtHalo;
#pragma unroll
    for (int j = 0; j < kPtWindow / 16; ++j) {
        const uint4 v = *reinterpret_cast<const uint4*>(image + pretok_lds_at(win.o0 + 16 * j));
        win.q[2 * j] = (uint64_t)v.x | ((uint64_t)v.y << 32);
        win.q[2 * j + 1] = (uint64_t)v.z | ((uint64_t)v.w << 32);
    }
    const pt_u128 B = (pt_u128)(map[lane] >> (64 - kPtHalo)) | ((pt_u128)map[lane + 1] << kPtHalo) | ((pt_u128)map[lane + 2] << (64 + kPtHalo));
    const PretokTables T{kPretokStage1, kPretokStage2, PRETOK_TABLE_LIMIT};
    pt_cl100k_prepare(win, B, T, c);
    return pt_cl100k_record(c);
}
__device__ __forceinline__ void pretok_ballots(uint32_t rec, uint64_t* K) {
#pragma unroll
    for (int b = 0; b < kPtRecBits; ++b) K[b] = __ballot((rec >> b) & 1u);
}

__global__ __launch_bounds__(kPretokWaves * 64) void k_pretok_cl100k_records(const uint8_t* __restrict__ u8, int64_t total, const int64_t* __restrict__ row_off,
                                                                             int64_t n_str, uint32_t* __restrict__ tile_rec) {
    __shared__ __attribute__((aligned(16))) uint8_t image_s[kPretokWaves][kPretokRows * kPretokRow];
    __shared__ unsigned long long map_s[kPretokWaves][kPretokMapWords];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t t = (int64_t)blockIdx.x * kPretokWaves + wave;
    const int64_t t0 = t * kTile;
    if (t0 >= total) return;                                    // whole wave
    pretok_stage(u8, total, row_off, n_str, t0, lane, image_s[wave], map_s[wave]);
    PtCl c;
    const uint32_t rec = pretok_cl100k_word(image_s[wave], map_s[wave], lane, (t * 64 + lane) * 64 < total, c);
    uint64_t K[kPtRecBits];
    pretok_ballots(rec, K);
    if (lane == 0) tile_rec[t] = (pt_rec_left(K, ~0ull) & 0x7Fu) | (pt_rec_right(K, ~0ull) & 0x180u);
}

__global__ __launch_bounds__(kPretokWaves * 64) void k_pretok_cl100k_planes(const uint8_t* __restrict__ u8, int64_t total, const int64_t* __restrict__ row_off,
                                                                            int64_t n_str, const uint32_t* __restrict__ tile_rec, uint64_t* __restrict__ bits,
                                                                            uint64_t* __restrict__ space, int64_t* __restrict__ tile_first) {
    __shared__ __attribute__((aligned(16))) uint8_t image_s[kPretokWaves][kPretokRows * kPretokRow];
    __shared__ unsigned long long map_s[kPretokWaves][kPretokMapWords];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t t = (int64_t)blockIdx.x * kPretokWaves + wave;
    const int64_t t0 = t * kTile;
    if (t0 >= total) return;                                    // whole wave
    const int64_t n_tiles = (total + kTile - 1) / kTile;
    const int64_t first = pretok_stage(u8, total, row_off, n_str, t0, lane, image_s[wave], map_s[wave]);
    if (lane == 0) tile_first[t] = first;
    const int64_t w = t * 64 + lane;
    const bool live = w * 64 < total;
    PtCl c;
    const uint32_t rec = pretok_cl100k_word(image_s[wave], map_s[wave], lane, live, c);
    // what enters the tile: the records of the tiles in front of it, 64 at a time (lane j: tile base + j), while a carry still passes;
    // in front of the batch every carry is 0, so the walk ends there at the latest
    uint64_t K[kPtRecBits];
    uint32_t in = kPtRecPass;
    for (int64_t base = t - 64; in & 0x54u; base -= 64) {
        pretok_ballots(base + lane >= 0 ? tile_rec[base + lane] : kPtRecZero, K);
        in = (pt_rec_then(pt_rec_left(K, ~0ull), in) & 0x7Fu) | (in & 0x180u);
    }
    for (int64_t base = t + 1; in & 0x100u; base += 64) {       // nl_ahead: the tiles behind it
        pretok_ballots(base + lane < n_tiles ? tile_rec[base + lane] : kPtRecZero, K);
        in = (in & 0x7Fu) | (pt_rec_then(in, pt_rec_right(K, ~0ull)) & 0x180u);
    }
    // what enters my word: the tile's carries through the words in front of mine (behind mine: nl_ahead)
    pretok_ballots(rec, K);
    if (!live) return;
    const uint64_t lt = (1ull << lane) - 1ull, gt = ~lt & ~(1ull << lane);
    const uint32_t left = pt_rec_then(in, pt_rec_left(K, lt)), right = pt_rec_then(pt_rec_right(K, gt), in);
    bits[w] = pt_cl100k_finish(c, pt_carry_of((left & 0x7Fu) | (right & 0x180u))) & valid_mask(w, total);
    space[w] = 0ull;
}

// ---- SentencePiece's segments (spbpe.h; LATOK_PRETOK_SPM) ------------------------------------------------------------------------------
// The rule has no carry (a start bit depends on 3 bytes behind it and 3 ahead), so this is k_pretok_planes' geometry once more: one
// launch, one wave per tile, the image and the string-start map of pretok_stage, every lane its word alone.  No table is read.
__global__ __launch_bounds__(kPretokWaves * 64) void k_pretok_spm_planes(const uint8_t* __restrict__ u8, int64_t total, const int64_t* __restrict__ row_off,
                                                                         int64_t n_str, uint64_t* __restrict__ bits, uint64_t* __restrict__ space,
                                                                         int64_t* __restrict__ tile_first) {
    __shared__ __attribute__((aligned(16))) uint8_t image_s[kPretokWaves][kPretokRows * kPretokRow];
    __shared__ unsigned long long map_s[kPretokWaves][kPretokMapWords];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t t = (int64_t)blockIdx.x * kPretokWaves + wave;
    const int64_t t0 = t * kTile;
    if (t0 >= total) return;                                    // whole wave (no workgroup barrier below)
    const uint8_t* image = image_s[wave];
    const unsigned long long* map = map_s[wave];
    const int64_t first = pretok_stage(u8, total, row_off, n_str, t0, lane, image_s[wave], map_s[wave]);
    if (lane == 0) tile_first[t] = first;
    const int64_t w = t * 64 + lane;
    if (w * 64 >= total) return;
    PretokWindow win;
    win.lds = image;
    win.o0 = 64 + 64 * lane - kPtHalo;
#pragma unroll
    for (int j = 0; j < kPtWindow / 16; ++j) {
        const uint4 v = *reinterpret_cast<const uint4*>(image + pretok_lds_at(win.o0 + 16 * j));
        win.q[2 * j] = (uint64_t)v.x | ((uint64_t)v.y << 32);
        win.q[2 * j + 1] = (uint64_t)v.z | ((uint64_t)v.w << 32);
    }
    const pt_u128 B = (pt_u128)(map[lane] >> (64 - kPtHalo)) | ((pt_u128)map[lane + 1] << kPtHalo) | ((pt_u128)map[lane + 2] << (64 + kPtHalo));
    bits[w] = sp_word_starts(win, B) & valid_mask(w, total);
    space[w] = 0ull;
}

hipError_t launch_pretok_spm_planes(const uint8_t* u8, int64_t total, const int64_t* row_off, int64_t n_str, uint64_t* bits, uint64_t* space,
                                    int64_t* tile_first, hipStream_t st) {
    if (total <= 0 || n_str <= 0) return hipSuccess;
    const int64_t n_tiles = (total + kTile - 1) / kTile;
    hipLaunchKernelGGL(k_pretok_spm_planes, dim3((unsigned)((n_tiles + kPretokWaves - 1) / kPretokWaves)), dim3(kPretokWaves * 64), 0, st, u8, total,
                       row_off, n_str, bits, space, tile_first);
    return hipGetLastError();
}

hipError_t launch_pretok_cl100k_planes(const uint8_t* u8, int64_t total, const int64_t* row_off, int64_t n_str, uint32_t* tile_rec, uint64_t* bits,
                                       uint64_t* space, int64_t* tile_first, hipStream_t st) {
    if (total <= 0 || n_str <= 0) return hipSuccess;
    const int64_t n_tiles = (total + kTile - 1) / kTile;
    const dim3 grid((unsigned)((n_tiles + kPretokWaves - 1) / kPretokWaves)), block(kPretokWaves * 64);
    hipLaunchKernelGGL(k_pretok_cl100k_records, grid, block, 0, st, u8, total, row_off, n_str, tile_rec);
    hipLaunchKernelGGL(k_pretok_cl100k_planes, grid, block, 0, st, u8, total, row_off, n_str, (const uint32_t*)tile_rec, bits, space, tile_first);
    return hipGetLastError();
}

hipError_t launch_pretok_planes(const uint8_t* u8, int64_t total, const int64_t* row_off, int64_t n_str, uint64_t* bits, uint64_t* space,
                                int64_t* tile_first, hipStream_t st) {
    if (total <= 0 || n_str <= 0) return hipSuccess;
    const int64_t n_tiles = (total + kTile - 1) / kTile;
    hipLaunchKernelGGL(k_pretok_planes, dim3((unsigned)((n_tiles + kPretokWaves - 1) / kPretokWaves)), dim3(kPretokWaves * 64), 0, st, u8, total, row_off,
                       n_str, bits, space, tile_first);
    return hipGetLastError();
}

}  // namespace latok
