// bpe_kernels.hip -- byte-level BPE ids of a UTF-8 batch in byte space: the kernels behind latok_bpe_ids_utf8_bytes_batch and
// latok_bpe_padded_utf8_bytes_batch.  They work in TOKEN space, one lane per token, behind the same front as the WordPiece kernels
// (wordpiece_kernels.hip): the span record of every token at its rank, the row starts in token space.  The row pointers and the padded
// block are that file's k_wp_rows and k_wp_pad, called as they are.
//
//   k_bpe_count  pieces of token t = the parts the merge walk of bpe.h leaves -> cnt[t]; cnt[n_tok] = 0, so that the scan of the
//                n_tok + 1 entries leaves the piece total behind the last token's rank.  For a token of the lane form it also leaves
//                the final part-start mask in masks[t], so that the emit pass does not merge again
//   k_bpe_emit   behind the scan, only if the piece total fits the capacity: ids[rank[t] + k] (through the rank -> id array), and the
//                piece's string-relative byte range if asked for.  Nothing is ever written outside the token's own range of ranks
//
// Two forms of the walk, both bpe_merge of bpe.h on a state of their own:
//   lane form    a token of at most kBpeLaneBytes = 64 bytes, by its lane: the part starts are a 64-bit mask in registers, neighbours
//                are bit scans, the pair ranks a lane-private column in LDS laid out [position][lane], so that a wave's access to one
//                position is 64 consecutive dwords: conflict-free
//   wave form    a token of 65 .. max_bytes bytes, by its whole wave, after the wave's lane tokens are done: the long tokens are
//                taken one at a time (ballot, lowest lane first, the range broadcast by v_readlane), as the hash kernel takes its
//                kHashWaveBytes tokens.  The wave's own LDS slice -- 64 positions x 64 lanes = 4096 entries -- is one rank array for the
//                whole token (64 consecutive positions are 64 consecutive dwords); the initial pairs are looked up 64 at a time; a round
//                is a per-lane scan of the positions lane, lane + 64, .., a wave-wide minimum of the rank and then of the position
//                among the lanes that hold it (DPP), one merge, and the two new pairs looked up by two lanes; the part starts are one
//                64-bit word per lane
// 64 KB of LDS per workgroup of 256: two workgroups per CU.  The text is read as aligned dwords up to the one that holds the token's
// last byte; with lead_space the byte in front of a token is read only where it lies inside the token's own string.  A token that is not
// ok (lane_token of block_ops.h) is skipped, so no load leaves the buffer whatever the workspace holds.  No kernel here waits for
// another workgroup; all stores are vector stores from plain C++.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bpe_device.h"   // the table view, the LDS column, the wave form's state, the piece store: shared with spbpe_kernels.hip

namespace latok {

// the token of a lane as the BPE cut takes it: with lead_space, the space in front of it (inside its own string) belongs to it
__device__ __forceinline__ TokenBytes bpe_token(const TokenText& T, const LaneToken& k, int lead_space) {
    TokenBytes b = k.b;
    if (b.ok && lead_space && b.a > k.base) {
        const uint32_t* const text = T.text;
        if (wp_byte([text](int64_t i) { return text[i]; }, b.a - 1) == 0x20u) --b.a;
    }
    return b;
}

__global__ __launch_bounds__(kBpeBlock) void k_bpe_count(TokenText T, BpeTable bt, int64_t* __restrict__ cnt, uint64_t* __restrict__ masks) {
    __shared__ uint32_t s_rank[kBpeLaneBytes * kBpeBlock];
    const LaneToken k = lane_token<kBpeBlock>(T);
    const int lane = threadIdx.x & 63;
    const TokenBytes b = bpe_token(T, k, bt.lead_space);
    const int64_t len = b.ok ? b.e - b.a : 0;
    const bool wide = len > kBpeLaneBytes && len <= (int64_t)bt.max_bytes;
    LATOK_BPE_VIEW(bt);
    int64_t n = 0;
    uint64_t mask = 1ull;   // one part: a whole-token piece
    if (b.ok && !wide) {
        uint32_t r;
        n = 1;
        if (!bpe_whole(ld, b.a, b.e, tab, seed, bt.max_bytes, &r)) {
            const int64_t a = b.a;
            auto s = bpe_lane_state(BpeLdsColumn{s_rank + threadIdx.x},
                                    [&](int i, int p) { return bpe_look(ld, a + i, a + p, tab, seed); });
            n = bpe_merge((int)len, s);
            mask = s.mask;
        }
    }
    // the long tokens of the wave, one at a time by the whole wave (wave-uniform loop: `todo` is a ballot)
    for (uint64_t todo = __ballot(wide); todo; todo &= todo - 1ull) {
        const int src = (int)__builtin_ctzll(todo);
        const int64_t a = lane_read64(b.a, src), e = lane_read64(b.e, src);
        int parts = 1;
        if (bpe_look(ld, a, e, tab, seed) == kBpeAbsent) {
            auto s = bpe_wave_state(s_rank + (threadIdx.x & ~63), [&](int i, int p) { return bpe_look(ld, a + i, a + p, tab, seed); }, lane);
            parts = bpe_merge((int)(e - a), s);
        }
        if (lane == src) n = parts;
        wave_lds_sync();   // (the next token's fill behind this one's last reads)
    }
    if (k.t <= T.n_tok) cnt[k.t] = n;   // (t == n_tok: the entry behind the last token)
    if (k.t < T.n_tok) masks[k.t] = mask;
}

template <typename OUT>
__global__ __launch_bounds__(kBpeBlock) void k_bpe_emit(TokenText T, BpeTable bt, int32_t unk, const int64_t* __restrict__ rank,
                                                        const uint64_t* __restrict__ masks, const int64_t* __restrict__ n_pieces_dev,
                                                        int64_t cap, int32_t* __restrict__ ids, OUT* __restrict__ spans) {
    __shared__ uint32_t s_rank[kBpeLaneBytes * kBpeBlock];
    if (*n_pieces_dev > cap) return;   // the caller's buffers hold `cap` pieces: nothing is written when the batch has more
    const LaneToken k = lane_token<kBpeBlock>(T);
    const int lane = threadIdx.x & 63;
    const TokenBytes b = bpe_token(T, k, bt.lead_space);
    int64_t at = 0;
    int64_t n_mine = 0;
    if (b.ok) {
        at = rank[k.t];
        n_mine = rank[k.t + 1] - at;   // (rank has n_tok + 1 entries)
    }
    const bool mine = b.ok && n_mine >= 1 && at >= 0 && at + n_mine <= cap;
    const int64_t len = mine ? b.e - b.a : 0;
    const bool wide = len > kBpeLaneBytes && len <= (int64_t)bt.max_bytes;
    LATOK_BPE_VIEW(bt);
    if (mine && !wide) {
        const int64_t a = b.a, rel = b.a - k.base;
        if (len > (int64_t)bt.max_bytes) {
            bpe_store<OUT>(ids, spans, at, unk, rel, rel + len);
        } else {   // the parts the count pass left: one lookup each
            const int L = (int)len;
            uint64_t m = (masks[k.t] & bpe_mask_all(L)) | 1ull;
            for (int64_t ord = 0; m && ord < n_mine; ++ord) {
                const int i = (int)__builtin_ctzll(m);
                m &= m - 1ull;
                const int p = m ? (int)__builtin_ctzll(m) : L;
                bpe_store<OUT>(ids, spans, at + ord, bpe_id(bt, bpe_look(ld, a + i, a + p, tab, seed), unk), rel + i, rel + p);
            }
        }
    }
    for (uint64_t todo = __ballot(wide); todo; todo &= todo - 1ull) {
        const int src = (int)__builtin_ctzll(todo);
        const int64_t a = lane_read64(b.a, src), e = lane_read64(b.e, src);
        const int64_t at_w = lane_read64(at, src), n_w = lane_read64(n_mine, src), rel = a - lane_read64(k.base, src);
        const int L = (int)(e - a);
        const uint32_t whole = bpe_look(ld, a, e, tab, seed);
        if (whole != kBpeAbsent) {
            if (lane == src) bpe_store<OUT>(ids, spans, at_w, bpe_id(bt, whole, unk), rel, rel + L);
            continue;
        }
        auto s = bpe_wave_state(s_rank + (threadIdx.x & ~63), [&](int i, int p) { return bpe_look(ld, a + i, a + p, tab, seed); }, lane);
        bpe_merge(L, s);
        int64_t ord = 0;
        for (int i = 0; i < L;) {   // the parts in order, 64 at a time: lane c takes the c-th of the group
            int my_i = 0, my_p = 0, got = 0;
            for (; got < 64 && i < L; ++got) {
                const int p = s.start_next(i, L);
                if (lane == got) {
                    my_i = i;
                    my_p = p;
                }
                i = p;
            }
            if (lane < got && ord + lane < n_w)
                bpe_store<OUT>(ids, spans, at_w + ord + lane, bpe_id(bt, bpe_look(ld, a + my_i, a + my_p, tab, seed), unk), rel + my_i, rel + my_p);
            ord += got;
        }
        wave_lds_sync();
    }
}

// ---- launchers -----------------------------------------------------------------------------------------------------
hipError_t launch_bpe_count(const TokenText& t, const BpeTable& bt, int64_t* cnt, uint64_t* masks, hipStream_t st) {
    if (t.n_str <= 0 || t.n_tok <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)((t.n_tok + 1 + kBpeBlock - 1) / kBpeBlock);   // (+ 1: the entry behind the last token)
    hipLaunchKernelGGL(k_bpe_count, dim3(blocks), dim3(kBpeBlock), 0, st, t, bt, cnt, masks);
    return hipGetLastError();
}

hipError_t launch_bpe_emit(bool out32, const TokenText& t, const BpeTable& bt, int32_t unk_id, const int64_t* rank, const uint64_t* masks,
                           const int64_t* n_pieces_dev, int64_t cap, int32_t* ids, void* spans, hipStream_t st) {
    if (t.n_str <= 0 || t.n_tok <= 0 || !ids) return hipSuccess;
    const dim3 grid((unsigned)((t.n_tok + kBpeBlock - 1) / kBpeBlock)), block(kBpeBlock);
    if (out32) hipLaunchKernelGGL((k_bpe_emit<int32_t>), grid, block, 0, st, t, bt, unk_id, rank, masks, n_pieces_dev, cap, ids, (int32_t*)spans);
    else hipLaunchKernelGGL((k_bpe_emit<int64_t>), grid, block, 0, st, t, bt, unk_id, rank, masks, n_pieces_dev, cap, ids, (int64_t*)spans);
    return hipGetLastError();
}

}  // namespace latok
