// fold_kernels.hip -- case folding and accent stripping of a UTF-8 batch on the device (latok_fold_utf8_bytes_batch,
// include/latok_hip.h; the map itself: fold_map.h).  UTF-8 in, folded UTF-8 out, every character's image 0 .. 12 bytes long:
//   k_fold_starts    bit p of a bitmap = a string ends in front of byte p (from byte_off; bit `total` closes the batch).  It is all
//                    the tile kernels need for the per-string rule: a lead byte opens a sequence only if none of these bits lies
//                    on its tail.
//   k_fold_counts    one wave per tile of kFoldTile bytes, four rounds of one aligned 16-byte group per lane: output bytes of
//                    every group as its exclusive prefix inside the tile (uint16, at most 3 * kFoldTile + 9), and per tile
//   k_scan_chained   tile ranks and the byte total (launch_tile_scan, unchanged)
//   k_fold_write     one wave per tile: every lane folds its groups again into an LDS window at the recorded prefix; the window
//                    leaves as one contiguous run of dwords.  Behind the tiles one thread per row offset:
//                    out_off[s] = rank of byte_off[s] = tile rank + group prefix + the group's bytes in front of it.
// A group sees 4 bytes in front of it and 4 behind it (sequences that reach into it or out of it) and the bitmap's 32 bits over
// those 24 positions; nothing else crosses lanes.  A group without a byte >= 0x80 takes no table: LOWER is A-Z + 32, CLEAN a range
// test.  The tables (190 KB of records, 37 KB of second stage) are read through the cache hierarchy; the characters of running text
// share a few blocks.
#include <hip/hip_runtime.h>

#include "fold_map.h"
#include "kernels.h"
#include "wave_ops.h"

namespace latok {

constexpr int kFoldWaves = 4;
constexpr int kFoldGroups = kFoldTile / 16;        // groups per tile: 64 lanes x 4 rounds
// Output bytes of a tile at most: a sequence belongs to the tile of its lead byte, so the tile's last byte may open a sequence of 4
// bytes with an image of 12 -- 3 * (kFoldTile - 1) + 12.  The window adds the run's offset inside its first dword.
constexpr int kFoldTileOut = 3 * kFoldTile + 9;
constexpr int kFoldWin = (kFoldTileOut + 3 + 15) & ~15;

__global__ __launch_bounds__(256) void k_fold_starts(const int64_t* __restrict__ byte_off, int64_t n_str, int64_t total,
                                                     uint32_t* __restrict__ start32) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s > n_str) return;
    const int64_t p = s == n_str ? total : byte_off[s];
    if (p > 0 && p <= total) atomicOr(&start32[p >> 5], 1u << (p & 31));
}

// One group as a lane holds it: 24 bytes, index 0 .. 3 = the bytes in front of the group (0 where there are none), 4 .. 19 its
// own (0 behind the batch's end), 20 .. 23 the bytes behind it; sb bit j = a string ends in front of index j.
struct FoldGroup {
    uint64_t q0, q1, q2;
    uint32_t sb;
    int n_own;   // own bytes inside the batch, 1 .. 16
};
__device__ __forceinline__ uint32_t fold_tail_dword(const uint8_t* __restrict__ u8, int64_t p, int64_t total) {
    uint32_t x = 0;
    for (int j = 0; j < 4; ++j)
        if (p + j < total) x |= (uint32_t)u8[p + j] << (8 * j);
    return x;
}
// (base < total, base a multiple of 16, u8 16-byte aligned: every load is aligned and inside [0, total))
__device__ __forceinline__ FoldGroup fold_load_group(const uint8_t* __restrict__ u8, int64_t total, int64_t base) {
    FoldGroup G;
    uint32_t d[6];
    d[0] = base >= 4 ? *reinterpret_cast<const uint32_t*>(u8 + base - 4) : 0u;
    if (base + 16 <= total) {
        const uint4 v = *reinterpret_cast<const uint4*>(u8 + base);
        d[1] = v.x; d[2] = v.y; d[3] = v.z; d[4] = v.w;
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) d[1 + q] = fold_tail_dword(u8, base + 4 * q, total);
    }
    d[5] = base + 20 <= total ? *reinterpret_cast<const uint32_t*>(u8 + base + 16) : fold_tail_dword(u8, base + 16, total);
    G.q0 = ((uint64_t)d[1] << 32) | d[0];
    G.q1 = ((uint64_t)d[3] << 32) | d[2];
    G.q2 = ((uint64_t)d[5] << 32) | d[4];
    G.sb = 0;
    G.n_own = total - base >= 16 ? 16 : (int)(total - base);
    return G;
}
// the bitmap's bits over positions base - 4 .. base + 27 (the bitmap has a spare dword behind the one that holds bit `total`)
__device__ __forceinline__ uint32_t fold_start_bits(const uint32_t* __restrict__ start32, int64_t base) {
    if (base == 0) return start32[0] << 4;
    const int64_t p = base - 4;
    const uint32_t lo = start32[p >> 5], hi = start32[(p >> 5) + 1];
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (p & 31));
}
__device__ __forceinline__ bool fold_group_ascii(const FoldGroup& G) {   // no own byte >= 0x80
    return (((G.q0 >> 32) | G.q1 | (G.q2 & 0xFFFFFFFFull)) & 0x8080808080808080ull) == 0ull;
}
__device__ __forceinline__ uint32_t fold_get4(const FoldGroup& G, int j) {   // the 4 bytes at index j, j <= 19
    const int wi = j >> 3, s = (j & 7) * 8;
    const uint64_t a = wi == 0 ? G.q0 : wi == 1 ? G.q1 : G.q2;
    const uint64_t b = wi == 0 ? G.q1 : wi == 1 ? G.q2 : 0ull;
    return s ? (uint32_t)((a >> s) | (b << (64 - s))) : (uint32_t)a;
}
__device__ __forceinline__ int fold_avail(uint32_t sb, int j) {   // bytes from index j to the end of its string, 4 = more
    const uint32_t m = (sb >> (j + 1)) & 7u;
    return m ? __builtin_ctz(m) + 1 : 4;
}
// bit 7 of byte i = byte i of x (all < 0x80) is dropped by CLEAN
__device__ __forceinline__ uint32_t fold_ascii_drop(uint32_t x) {
    const uint32_t H = 0x80808080u;
    auto eq = [&](uint32_t v) { return (((x ^ (v * 0x01010101u)) + 0x7F7F7F7Fu) & H) ^ H; };
    const uint32_t lt20 = ~(x + 0x60606060u) & H;
    return (lt20 & ~(eq(9u) | eq(10u) | eq(13u))) | eq(0x7Fu);
}

// Output bytes of the own bytes 0 .. upto - 1 of a group (upto <= n_own; a string ends at `upto` or upto == n_own); EMIT: stored at dst,
// which has room for `room` bytes (the count pass saw the same bytes, so they fit; the test keeps a batch that changed between the
// passes inside the window).
template <bool EMIT>
__device__ __forceinline__ int fold_group(const FoldGroup& G, int upto, int fold, const FoldTables& T, uint8_t* dst, int room = 0) {
    const int end = 4 + upto;
    int n = 0;
    if (fold_group_ascii(G)) {
        if (!EMIT) {
            if (!(fold & kFoldClean)) return upto;
            const uint32_t own[4] = {(uint32_t)(G.q0 >> 32), (uint32_t)G.q1, (uint32_t)(G.q1 >> 32), (uint32_t)G.q2};
            uint32_t drop = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) drop |= ((((fold_ascii_drop(own[q]) >> 7) * 0x00204081u) >> 21) & 0xFu) << (4 * q);
            return upto - __popc(drop & ((1u << upto) - 1u));
        }
#pragma unroll
        for (int j = 4; j < 20; ++j) {
            if (j < end) {
                uint32_t x = fold_get4(G, j) & 0xFFu;
                if (fold & kFoldClean) x = fold_ascii_clean(x);
                if ((fold & kFoldLower) && x >= 'A' && x <= 'Z') x += 32u;
                if ((x != 0u || !(fold & kFoldClean)) && n < room) dst[n++] = (uint8_t)x;
            }
        }
        return n;
    }
    // own bytes that a sequence from in front of the group consumed (a byte that announces a tail is never itself consumed)
    int j = 4;
    for (int i = 1; i < 4; ++i) {
        const int len = fold_seq_len(fold_get4(G, i), fold_avail(G.sb, i));
        if (i + len > j) j = i + len;
    }
    while (j < end) {
        const FoldStep st = fold_step(fold_get4(G, j), fold_avail(G.sb, j), fold, T);
        if (EMIT) {
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (b < st.len[r] && n < room) dst[n++] = (uint8_t)(st.w[r] >> (8 * b));
        } else {
            n += st.total;
        }
        j += st.used;
    }
    return n;
}

__global__ __launch_bounds__(kFoldWaves * 64) void k_fold_counts(const uint8_t* __restrict__ u8, int64_t total,
                                                                 const uint32_t* __restrict__ start32, int fold, FoldTables T,
                                                                 uint16_t* __restrict__ group_pref, int64_t* __restrict__ tile_cnt) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t t = (int64_t)blockIdx.x * kFoldWaves + wave;
    if (t * kFoldTile >= total) return;                             // whole wave
    int carry = 0;
    for (int rd = 0; rd < 4; ++rd) {
        const int64_t g = t * kFoldGroups + rd * 64 + lane;
        const int64_t base = g * 16;
        int cnt = 0;
        if (base < total) {
            FoldGroup G = fold_load_group(u8, total, base);
            if (!fold_group_ascii(G)) G.sb = fold_start_bits(start32, base);
            cnt = fold_group<false>(G, G.n_own, fold, T, nullptr);
        }
        const int inc = shfl_scan_add(cnt, lane);
        if (base < total) group_pref[g] = (uint16_t)(carry + inc - cnt);
        carry += __shfl(inc, 63);
    }
    if (lane == 0) tile_cnt[t] = carry;
}

__global__ __launch_bounds__(kFoldWaves * 64) void k_fold_write(const uint8_t* __restrict__ u8, int64_t total,
                                                                const uint32_t* __restrict__ start32, int fold, FoldTables T,
                                                                const uint16_t* __restrict__ group_pref, const int64_t* __restrict__ tile_rank,
                                                                const int64_t* __restrict__ tile_cnt, const int64_t* __restrict__ row_off,
                                                                int64_t n_str, uint8_t* __restrict__ out, int64_t cap,
                                                                const int64_t* __restrict__ n_items_dev, int64_t* __restrict__ out_off,
                                                                unsigned n_tile_blocks) {
    if (blockIdx.x >= n_tile_blocks) {   // role 2: one thread per row offset (and the end of the batch)
        const int64_t s = (int64_t)(blockIdx.x - n_tile_blocks) * (kFoldWaves * 64) + threadIdx.x;
        if (s > n_str) return;
        const int64_t p = row_off[s];
        int64_t rank = *n_items_dev;
        if (p <= 0) {
            rank = 0;
        } else if (p < total) {
            const int64_t g = p >> 4;
            const int u = (int)(p & 15);
            rank = tile_rank[g / kFoldGroups] + group_pref[g];
            if (u) {
                FoldGroup G = fold_load_group(u8, total, g * 16);
                if (!fold_group_ascii(G)) G.sb = fold_start_bits(start32, g * 16);
                rank += fold_group<false>(G, u, fold, T, nullptr);
            }
        }
        out_off[s] = rank;
        return;
    }
    // role 1: one wave per tile.  The caller's buffer holds `cap` bytes; when the batch needs more, nothing is written.
    if (*n_items_dev > cap) return;
    __shared__ __attribute__((aligned(16))) uint8_t win_s[kFoldWaves][kFoldWin];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t t = (int64_t)blockIdx.x * kFoldWaves + wave;
    if (t * kFoldTile >= total) return;                             // whole wave
    const int n_wave = (int)tile_cnt[t];
    if (n_wave <= 0 || n_wave > kFoldTileOut) return;
    uint8_t* dst = out + tile_rank[t];
    const int a = (int)((uintptr_t)dst & 3u);                       // window byte j <-> dst - a + j: dwords of the two coincide
    uint8_t* win = win_s[wave];
    for (int rd = 0; rd < 4; ++rd) {
        const int64_t g = t * kFoldGroups + rd * 64 + lane;
        const int64_t base = g * 16;
        if (base < total) {
            const int pref = group_pref[g];
            FoldGroup G = fold_load_group(u8, total, base);
            if (!fold_group_ascii(G)) G.sb = fold_start_bits(start32, base);
            fold_group<true>(G, G.n_own, fold, T, win + a + pref, kFoldTileOut - pref);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // the run [a, a + n_wave) of the window: whole dwords, the ragged <= 3 bytes at each end as bytes -- one writer per byte
    const int lo = a, hi = a + n_wave;
    uint8_t* base = dst - a;
    const int d0 = (lo + 3) & ~3, d1 = hi & ~3;
    if (d0 >= d1) {
        if (lo + lane < hi) base[lo + lane] = win[lo + lane];
    } else {
        if (lo + lane < d0) base[lo + lane] = win[lo + lane];
        for (int j = d0 + 4 * lane; j < d1; j += 256)
            __builtin_nontemporal_store(*reinterpret_cast<const uint32_t*>(win + j), reinterpret_cast<uint32_t*>(base + j));
        if (d1 + lane < hi) base[d1 + lane] = win[d1 + lane];
    }
}

int64_t fold_start_words(int64_t total) { return (total >> 5) + 2; }
int64_t fold_groups(int64_t total) { return (total + 15) / 16; }
int64_t fold_tiles(int64_t total) { return (total + kFoldTile - 1) / kFoldTile; }

hipError_t launch_fold_starts(const int64_t* byte_off, int64_t n_str, int64_t total, uint32_t* start32, hipStream_t st) {
    hipError_t e = hipMemsetAsync(start32, 0, (size_t)fold_start_words(total) * 4, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_fold_starts, dim3((unsigned)((n_str + 1 + 255) / 256)), dim3(256), 0, st, byte_off, n_str, total, start32);
    return hipGetLastError();
}
hipError_t launch_fold_counts(const uint8_t* u8, int64_t total, const uint32_t* start32, int fold, const FoldTables& T, uint16_t* group_pref,
                              int64_t* tile_cnt, hipStream_t st) {
    const int64_t n_tiles = fold_tiles(total);
    if (n_tiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_fold_counts, dim3((unsigned)((n_tiles + kFoldWaves - 1) / kFoldWaves)), dim3(kFoldWaves * 64), 0, st, u8, total, start32,
                       fold, T, group_pref, tile_cnt);
    return hipGetLastError();
}
// out == NULL: the row offsets only (a size query)
hipError_t launch_fold_write(const uint8_t* u8, int64_t total, const uint32_t* start32, int fold, const FoldTables& T, const uint16_t* group_pref,
                             const int64_t* tile_rank, const int64_t* tile_cnt, const int64_t* row_off, int64_t n_str, uint8_t* out, int64_t cap,
                             const int64_t* n_items_dev, int64_t* out_off, hipStream_t st) {
    const int64_t n_tiles = fold_tiles(total);
    if (n_tiles <= 0) return hipSuccess;
    const unsigned nb_tiles = out ? (unsigned)((n_tiles + kFoldWaves - 1) / kFoldWaves) : 0u;
    const unsigned nb_rows = (unsigned)((n_str + 1 + kFoldWaves * 64 - 1) / (kFoldWaves * 64));
    hipLaunchKernelGGL(k_fold_write, dim3(nb_tiles + nb_rows), dim3(kFoldWaves * 64), 0, st, u8, total, start32, fold, T, group_pref, tile_rank,
                       tile_cnt, row_off, n_str, out, cap, n_items_dev, out_off, nb_tiles);
    return hipGetLastError();
}

}  // namespace latok
