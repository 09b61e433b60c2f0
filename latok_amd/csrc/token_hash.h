// token_hash.h -- MurmurHash3 x86_32 (Austin Appleby, public domain) of a token's bytes, in the two forms the hash kernel uses
// (compact_kernels.hip: HashTokens of scatter_block).  Plain C++: it compiles on the host (tests/helpers/token_hash_harness.cpp
// runs it against an independent implementation) and, under hipcc, on the device.
//
//   the function     h = seed
//                    for every whole 4-byte block (little endian), in order:  h = th_mix_h(h, th_mix_k(block))
//                    the 1..3 bytes behind the last block, little endian, upper bytes zero:  h ^= th_mix_k(tail)
//                    h = th_fmix32(h ^ length)
//   th_hash_lane     one thread walks one token: the form of short tokens (lane j of a wave holds token j)
//   th_wave_blocks / th_wave_fold / th_wave_tail
//                    a wave takes one long token 64 blocks (256 bytes) at a time: lane l mixes block 64 r + l on its own
//                    (th_mix_k is the expensive half and needs no neighbour), then the h chain -- which is sequential by
//                    construction -- folds the 64 mixed blocks in lane order 0, 1, .. 63
//
// The text is read as ALIGNED dwords through a loader `ld(i)` = dword i of the buffer (bytes 4i .. 4i + 3, little endian), and a
// block that starts at any byte is cut out of the pair (ld(i), ld(i + 1)).  No form asks the loader for a dword behind the one
// that holds the token's last byte (the index is clamped to it), so nothing is read beyond the aligned dword that holds the last
// byte of the batch; what the clamp repeats and what lies in front of the token's first byte is shifted out, what lies behind
// its last byte is masked off before it can reach the hash.
#ifndef LATOK_TOKEN_HASH_H
#define LATOK_TOKEN_HASH_H
#include <stdint.h>

#if defined(__HIPCC__)
#define TH_FN __host__ __device__ __forceinline__
#else
#define TH_FN inline
#endif

constexpr uint32_t kThC1 = 0xcc9e2d51u, kThC2 = 0x1b873593u, kThN = 0xe6546b64u;
constexpr int kThWaveBlocks = 64;                    // blocks a wave mixes per round: one per lane
constexpr int kThWaveRound = 4 * kThWaveBlocks;      // = 256 bytes

TH_FN uint32_t th_rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
TH_FN uint32_t th_mix_k(uint32_t k) { return th_rotl32(k * kThC1, 15) * kThC2; }
TH_FN uint32_t th_mix_h(uint32_t h, uint32_t mixed_k) { return th_rotl32(h ^ mixed_k, 13) * 5u + kThN; }
TH_FN uint32_t th_fmix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}
// the 4 bytes from byte `sh` (0..3) of the dword pair (lo, hi) on
TH_FN uint32_t th_align(uint32_t hi, uint32_t lo, uint32_t sh) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, sh);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * sh));
#endif
}
// the tail: `n` = 1..3 bytes, the low bytes of `word`; whatever the upper bytes hold stays out
TH_FN uint32_t th_tail(uint32_t h, uint32_t word, int n) { return h ^ th_mix_k(word & ((1u << (8 * n)) - 1u)); }
TH_FN uint32_t th_finish(uint32_t h, uint32_t len) { return th_fmix32(h ^ len); }

// One thread, one token: bytes [a, e) of the buffer.  One aligned load per block: the upper dword of a pair is the lower of the next.
template <class Load>
TH_FN uint32_t th_hash_lane(Load ld, int64_t a, int64_t e, uint32_t seed) {
    if (e <= a) return th_finish(seed, 0u);
    const int64_t q = a >> 2, last = (e - 1) >> 2;           // dwords of the first and of the last byte
    const uint32_t sh = (uint32_t)(a & 3), len = (uint32_t)(e - a);
    const int64_t nb = (e - a) >> 2;                         // (the length enters the hash as 32 bits, as in the original)
    uint32_t h = seed, lo = ld(q);
    for (int64_t i = 0; i < nb; ++i) {
        const int64_t qi = q + i + 1;
        const uint32_t hi = ld(qi < last ? qi : last);       // (clamped: only read where a byte of the block lies in it)
        h = th_mix_h(h, th_mix_k(th_align(hi, lo, sh)));
        lo = hi;
    }
    if (len & 3u) {
        const int64_t qi = q + nb + 1;
        const uint32_t hi = ld(qi < last ? qi : last);
        h = th_tail(h, th_align(hi, lo, sh), (int)(len & 3u));
    }
    return th_finish(h, len);
}

// A wave, one token [a, e), round r: the mixed block of lane `lane` -- block 64 r + lane of the token --, 0 behind the last
// whole block.  th_wave_count(a, e, r) = how many lanes of the round hold a block.
TH_FN int th_wave_count(int64_t a, int64_t e, int64_t r) {
    const int64_t left = ((e - a) >> 2) - r * kThWaveBlocks;
    return left >= kThWaveBlocks ? kThWaveBlocks : (left > 0 ? (int)left : 0);
}
template <class Load>
TH_FN uint32_t th_wave_block(Load ld, int64_t a, int64_t e, int64_t r, int lane) {
    const int64_t i = r * kThWaveBlocks + lane;
    if (i >= ((e - a) >> 2)) return 0u;
    const int64_t q = (a >> 2) + i, last = (e - 1) >> 2;
    return th_mix_k(th_align(ld(q + 1 < last ? q + 1 : last), ld(q), (uint32_t)(a & 3)));
}
// the order of the fold: mixed block of lane 0 first, then lane 1, .. lane n - 1; `k_of(l)` = lane l's mixed block
template <class LaneValue>
TH_FN uint32_t th_wave_fold(uint32_t h, LaneValue k_of, int n) {
    for (int l = 0; l < n; ++l) h = th_mix_h(h, k_of(l));
    return h;
}
// behind the last round: the tail bytes and the length
template <class Load>
TH_FN uint32_t th_wave_tail(Load ld, int64_t a, int64_t e, uint32_t h) {
    const uint32_t len = (uint32_t)(e - a);
    if (len & 3u) {
        const int64_t q = (a >> 2) + ((e - a) >> 2), last = (e - 1) >> 2;
        h = th_tail(h, th_align(ld(q + 1 < last ? q + 1 : last), ld(q), (uint32_t)(a & 3)), (int)(len & 3u));
    }
    return th_finish(h, len);
}

#endif
