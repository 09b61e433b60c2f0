// bpe_device.h -- what the two BPE kernel files share on the device (bpe_kernels.hip: byte-level BPE; spbpe_kernels.hip: SentencePiece
// BPE): the view of a BpeTable, the lane form's LDS column, the wave form's state of bpe_merge (bpe.h) and the piece store.  Device
// code only; the walk itself is bpe.h's.
#ifndef LATOK_BPE_DEVICE_H
#define LATOK_BPE_DEVICE_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_ops.h"
#include "bpe.h"
#include "kernels.h"

namespace latok {

static_assert(kBpeBlock % 64 == 0 && kBpeLaneBytes == 64, "the wave's LDS slice is 64 positions x 64 lanes");
static_assert(kBpeLaneBytes * 64 >= kBpeMaxBytes, "the wave's slice holds the ranks of the longest token");

#define LATOK_BPE_VIEW(bt)                                                                                                          \
    const VtSlot* const slots = reinterpret_cast<const VtSlot*>((bt).table.slots);                                                  \
    const uint32_t* const blob = (bt).table.blob;                                                                                   \
    const uint32_t* const text = T.text;                                                                                            \
    const uint32_t seed = (bt).table.seed;                                                                                          \
    const auto ld = [text](int64_t i) { return text[i]; };                                                                          \
    const auto tab = wp_table_view([slots](uint64_t i) { return slots[i]; }, [blob](uint64_t i) { return blob[i]; },               \
                                   (bt).table.n_slots, (bt).max_len)

// a lane's column of the workgroup's rank array: position i at p[i * kBpeBlock]
struct BpeLdsColumn {
    uint32_t* p;
    __device__ __forceinline__ uint32_t get(int i) const { return p[i * kBpeBlock]; }
    __device__ __forceinline__ void set(int i, uint32_t r) const { p[i * kBpeBlock] = r; }
};

// The wave form's state.  Every member function is called by all 64 lanes with wave-uniform arguments and returns a wave-uniform value.
template <class Look>
struct BpeWaveState {
    uint32_t* slice;   // the wave's 64 columns: position p at slice[(p >> 6) * kBpeBlock + (p & 63)]
    Look look;
    int lane;
    uint64_t bits;     // the part starts 64 lane .. 64 lane + 63
    __device__ __forceinline__ uint32_t* at(int p) const { return slice + (p >> 6) * kBpeBlock + (p & 63); }
    __device__ __forceinline__ uint64_t word(int l) const { return (uint64_t)lane_read64((int64_t)bits, to_scalar(l)); }
    __device__ __forceinline__ void fill(int L) {
        for (int base = 0; base < L; base += 64) {   // the initial pairs, 64 at a time
            const int p = base + lane;
            if (p < L) *at(p) = p + 2 <= L ? look(p, p + 2) : kBpeAbsent;
        }
        const int mine = L - 64 * lane;
        bits = mine <= 0 ? 0ull : bpe_mask_all(mine);
    }
    __device__ __forceinline__ int argmin(int L, uint32_t* r) const {
        wave_lds_sync();   // (the ranks the round before stored)
        uint32_t best = kBpeAbsent;
        uint32_t pos = 0x7FFFFFFFu;
        for (int p = lane; p < L; p += 64) {   // ascending: of equal ranks the first stays
            const uint32_t v = *at(p);
            if (v < best) {
                best = v;
                pos = (uint32_t)p;
            }
        }
        const uint32_t lowest = wave_min_u32(best);
        *r = lowest;
        if (lowest == kBpeAbsent) return 0;
        return (int)wave_min_u32(best == lowest ? pos : 0x7FFFFFFFu);   // the leftmost among the lanes that hold it
    }
    __device__ __forceinline__ int start_next(int i, int L) const {
        const int l = i >> 6;
        const uint64_t own = word(l);
        const int n = bpe_mask_next(own, i & 63);
        if (n < 64) return 64 * l + n;   // (bits behind L - 1 are never set)
        const uint64_t later = l >= 63 ? 0ull : __ballot(bits != 0ull) & (~0ull << (l + 1));
        if (!later) return L;
        const int l2 = (int)__builtin_ctzll(later);
        return 64 * l2 + (int)__builtin_ctzll(word(l2));
    }
    __device__ __forceinline__ int start_prev(int i) const {   // i > 0; position 0 is always a start
        const int l = i >> 6;
        const uint64_t below = word(l) & ((1ull << (i & 63)) - 1ull);
        if (below) return 64 * l + 63 - (int)__builtin_clzll(below);
        const uint64_t earlier = __ballot(bits != 0ull) & ((1ull << l) - 1ull);
        if (!earlier) return 0;
        const int l2 = 63 - (int)__builtin_clzll(earlier);
        return 64 * l2 + 63 - (int)__builtin_clzll(word(l2));
    }
    __device__ __forceinline__ void start_clear(int j) {
        if (lane == (j >> 6)) bits &= ~(1ull << (j & 63));
    }
    __device__ __forceinline__ void set_rank(int i, uint32_t r) const {
        if (lane == 0) *at(i) = r;
    }
    __device__ __forceinline__ void look2(int h, int k, int i, int q, uint32_t* rl, uint32_t* rr) const {
        uint32_t v = kBpeAbsent;   // two lanes, one new pair each
        if (lane == 0 && h >= 0) v = look(h, k);
        else if (lane == 1 && q > k) v = look(i, q);
        *rl = (uint32_t)lane_read((int)v, 0);
        *rr = (uint32_t)lane_read((int)v, 1);
    }
};
template <class Look>
__device__ __forceinline__ BpeWaveState<Look> bpe_wave_state(uint32_t* slice, Look look, int lane) {
    return BpeWaveState<Look>{slice, look, lane, 0ull};
}

template <typename OUT>
__device__ __forceinline__ void bpe_store(int32_t* __restrict__ ids, OUT* __restrict__ spans, int64_t at, int32_t id, int64_t s, int64_t e) {
    typedef OUT out2 __attribute__((ext_vector_type(2)));
    __builtin_nontemporal_store(id, ids + at);
    if (spans) {
        out2 v;
        v.x = (OUT)s;
        v.y = (OUT)e;
        __builtin_nontemporal_store(v, reinterpret_cast<out2*>(spans) + at);
    }
}
__device__ __forceinline__ int32_t bpe_id(const BpeTable& bt, uint32_t rank, int32_t unk) {
    return (int64_t)rank < bt.n_words ? bt.rank_id[rank] : unk;   // (kBpeAbsent is no rank)
}

}  // namespace latok

#endif
