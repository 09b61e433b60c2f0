// feat_records.h -- a token's 25 feature sums as a packed record and the record stream out of a wave's LDS window: shared by
// k_features_tiles (feature_kernels.hip) and the featurize form of k_small_batch (split_kernels.hip).  Device code only.
#ifndef LATOK_FEAT_RECORDS_H
#define LATOK_FEAT_RECORDS_H
#include "tile_core.h"

namespace latok {

struct FeatSums {
    uint32_t v[7];   // byte c of the 28 = column c (bytes 25..27 unused)
};

// A token's 25 sums enter the window packed (25-byte stride: the dword stores become byte stores).  Padding the records
// to 28 or 32 bytes for aligned LDS stores was measured: the LDS pipe's busy time drops 2.5x (PMC), but the un-padding
// on the way out costs more instructions than it saves and only 832 tokens fit a round at six waves: 796 vs 691 us on
// C2 (32-byte records: every slot lands in one of four bank groups, 913 us).  The kernel is bound by the dependent
// chain of ~7 K instructions per tile at 1.5 waves per SIMD, not by a pipe.
__device__ __forceinline__ void put_record(uint8_t* win, int slot, const FeatSums& s) {
    uint8_t* rec = win + slot * kFeatRec;
#pragma unroll
    for (int q = 0; q < 6; ++q) __builtin_memcpy(rec + 4 * q, &s.v[q], 4);
    rec[24] = (uint8_t)s.v[6];
}
// Stream n_rec records out as n_rec * 25 contiguous bytes at dst (any alignment).  The records were put at
// win + record_shift(dst): LDS and global address then agree modulo 16, so after at most 15 head bytes the stream leaves as
// aligned 16-byte vectors (one ds_read_b128 + one global_store_dwordx4 per lane and step).  With the records at the
// window's start the LDS side was unaligned whenever dst was: four byte reads + shifts per dword, ~800 of the kernel's
// ~7 K instructions per tile.
__device__ __forceinline__ int record_shift(const void* dst) { return (int)((uintptr_t)dst & 15u); }
__device__ __forceinline__ void flush_records(const uint8_t* win, int n_rec, uint8_t* dst, int lane) {
    const int n_bytes = n_rec * 25;
    const uint8_t* src = win + record_shift(dst);
    const int head = min((16 - record_shift(dst)) & 15, n_bytes);
    if (lane < head) dst[lane] = src[lane];
    const int n_vec = (n_bytes - head) >> 4;
    for (int i = lane; i < n_vec; i += 64) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(src + head + 16 * i);
        __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(dst + head + 16 * i));
    }
    const int tail0 = head + 16 * n_vec;
    if (lane < n_bytes - tail0) dst[tail0 + lane] = src[tail0 + lane];
}

}  // namespace latok
#endif
