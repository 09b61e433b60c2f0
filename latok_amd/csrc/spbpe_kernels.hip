// spbpe_kernels.hip -- SentencePiece BPE ids of a UTF-8 batch in byte space: the kernels behind latok_bpe_ids_utf8_bytes_batch and
// latok_bpe_padded_utf8_bytes_batch for an object of latok_bpe_create_spm (spbpe.h; the definition: include/latok_hip.h).  The frame is
// bpe_kernels.hip's: TOKEN space, one lane per token, where a token is a SEGMENT of k_pretok_spm_planes; k_spbpe_count leaves the pieces of
// every segment (and the lane form's final part-start mask), the caller scans them, k_spbpe_emit stores ids and spans at the piece ranks.
// The row pointers and the padded block are k_wp_rows and k_wp_pad, called as they are.
//
//   virtual text  every lookup reads the segment's VIRTUAL text (one marker for the dummy prefix, one per lead character, then the bytes
//                 verbatim).  It is COMPOSED dword by dword on the fly (SpVirtual of spbpe.h: the periodic lead from three constants, the
//                 rest by v_alignbyte over two aligned dwords of the text, both clamped into the segment's own dwords) and never staged:
//                 LDS stays the 64 KB of ranks per workgroup of 256 that k_bpe_count takes, two workgroups per CU.
//   lane form     virtual length <= 64: SpLaneState (the character starts are the part starts), bpe_merge, the ranks in the lane's LDS
//                 column.  A part that is no word is a single character: with byte ids the lane counts, and later stores, one piece per
//                 byte, so a lane may store several pieces for one part
//   wave form     virtual length 65 .. max_bytes, by the whole wave: BpeWaveState with a fill of its own (the character-start words by
//                 ballot, every lane the pair of its position), bpe_merge, then the parts 64 at a time: lane c looks up the c-th, the
//                 piece counts are summed (count) or scanned (emit) over the wave.  Without byte ids and with fuse_unk the emit walks
//                 the parts one after the other instead (a run of unknowns may cross a group of 64)
// Every store is bounded by the segment's own range of piece ranks from the scan of the first pass, and that range by the capacity.  A
// segment that is not ok (lane_token of block_ops.h) is skipped; every text load lies inside the segment's own dwords; all stores are
// vector stores from plain C++.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bpe_device.h"
#include "spbpe.h"

namespace latok {

// the wave form's state: BpeWaveState with the part starts at character starts.  `reach` = the longest word: a longer span needs no probe.
template <class Look, class IsStart>
struct SpWaveState : BpeWaveState<Look> {
    IsStart is_start;
    int reach;
    __device__ __forceinline__ void fill(int L) {
        const int lane = this->lane;
        this->bits = 0ull;
        for (int base = 0; base < L; base += 64) {
            const int p = base + lane;
            bool st = false;
            if (p < L) st = is_start(p);
            const uint64_t w = __ballot(st);
            if (lane == (base >> 6)) this->bits = w;
        }
        for (int base = 0; base < L; base += 64) {   // the pair of every character start: this character and the next
            const int p = base + lane;
            if (p >= L) continue;
            uint32_t r = kBpeAbsent;
            if (is_start(p)) {
                int j = p + 1;
                while (j < L && j - p <= reach && !is_start(j)) ++j;
                if (j < L && j - p <= reach) {
                    int k = j + 1;
                    while (k < L && k - p <= reach && !is_start(k)) ++k;
                    if (k - p <= reach) r = this->look(p, k);
                }
            }
            *this->at(p) = r;
        }
    }
};
template <class Look, class IsStart>
__device__ __forceinline__ SpWaveState<Look, IsStart> sp_wave_state(uint32_t* slice, Look look, int lane, IsStart is_start, int reach) {
    SpWaveState<Look, IsStart> s{{slice, look, lane, 0ull}, is_start, reach};
    return s;
}

// the segment of a lane: its token, with the dummy prefix where the object has one and the segment is its string's first
__device__ __forceinline__ int sp_dummy_of(const SpBpeTable& sp, const LaneToken& k) { return sp.add_dummy_prefix && k.b.a == k.base ? 1 : 0; }

__global__ __launch_bounds__(kBpeBlock) void k_spbpe_count(TokenText T, SpBpeTable sp, int64_t* __restrict__ cnt, uint64_t* __restrict__ masks) {
    __shared__ uint32_t s_rank[kBpeLaneBytes * kBpeBlock];
    const LaneToken k = lane_token<kBpeBlock>(T);
    const int lane = threadIdx.x & 63;
    const TokenBytes b = k.b;
    const BpeTable& bt = sp.bt;
    LATOK_BPE_VIEW(bt);
    const bool bytes = sp.byte_ids != nullptr;
    const bool fuse = !bytes && sp.fuse_unk;
    SpSeg g;
    if (b.ok) g = sp_segment(ld, b.a, b.e, sp_dummy_of(sp, k), bt.max_bytes);
    const bool wide = b.ok && !g.over && g.VL > kSpLaneBytes;
    int64_t n = 0;
    uint64_t mask = 1ull;
    if (b.ok && !wide) {
        n = 1;   // (over max_bytes: one unknown piece)
        if (!g.over) {
            const int L = (int)g.VL;
            const auto vld = sp_virtual(ld, g);
            const auto look = [&](int i, int p) { return bpe_look(vld, i, p, tab, seed); };
            const uint64_t chars = sp_char_mask(vld, g.P, L);
            auto s = sp_lane_state(BpeLdsColumn{s_rank + threadIdx.x}, look, chars);
            bpe_merge(L, s);
            mask = s.mask;
            n = 0;
            bool run = false;   // the part in front is unknown
            for (uint64_t m = mask; m;) {
                const int i = (int)__builtin_ctzll(m);
                m &= m - 1ull;
                const int p = m ? (int)__builtin_ctzll(m) : L;
                const uint64_t inner = chars & bpe_mask_all(p) & ~bpe_mask_all(i + 1);   // character starts inside the part: a merged part, a word
                const bool unknown = !inner && look(i, p) == kBpeAbsent;
                if (!unknown) n += 1;
                else if (bytes) n += p - i;
                else if (!(fuse && run)) n += 1;
                run = unknown;
            }
        }
    }
    // the long segments of the wave, one at a time by the whole wave (wave-uniform loop: `todo` is a ballot)
    const int dummy_mine = b.ok ? g.dummy : 0;
    for (uint64_t todo = __ballot(wide); todo; todo &= todo - 1ull) {
        const int src = (int)__builtin_ctzll(todo);
        const int64_t a = lane_read64(b.a, src), e = lane_read64(b.e, src);
        const SpSeg w = sp_segment(ld, a, e, lane_read(dummy_mine, src), bt.max_bytes);   // (every lane the same walk)
        const int L = (int)w.VL;
        const auto vld = sp_virtual(ld, w);
        const auto look = [&](int i, int p) { return bpe_look(vld, i, p, tab, seed); };
        const int64_t P = w.P;
        auto s = sp_wave_state(s_rank + (threadIdx.x & ~63), look, lane, [&](int v) { return sp_vstart(vld, P, v); }, (int)bt.max_len);
        bpe_merge(L, s);
        int64_t pieces = 0;
        bool carry = false;   // the last part of the group in front is unknown
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
            const bool have = lane < got;
            bool unknown = false;
            if (have) unknown = look(my_i, my_p) == kBpeAbsent;
            const uint64_t u = __ballot(unknown);
            int c = !have ? 0 : (!unknown ? 1 : (bytes ? my_p - my_i : 1));
            if (fuse && unknown && (lane > 0 ? ((u >> (lane - 1)) & 1ull) != 0ull : carry)) c = 0;
            carry = ((u >> (got - 1)) & 1ull) != 0ull;
            pieces += wave_sum(c);
        }
        if (lane == src) n = pieces;
        wave_lds_sync();   // (the next segment's fill behind this one's last reads)
    }
    if (k.t <= T.n_tok) cnt[k.t] = n;   // (t == n_tok: the entry behind the last token)
    if (k.t < T.n_tok) masks[k.t] = mask;
}

template <typename OUT>
__global__ __launch_bounds__(kBpeBlock) void k_spbpe_emit(TokenText T, SpBpeTable sp, int32_t unk, const int64_t* __restrict__ rank,
                                                          const uint64_t* __restrict__ masks, const int64_t* __restrict__ n_pieces_dev,
                                                          int64_t cap, int32_t* __restrict__ ids, OUT* __restrict__ spans) {
    __shared__ uint32_t s_rank[kBpeLaneBytes * kBpeBlock];
    if (*n_pieces_dev > cap) return;   // the caller's buffers hold `cap` pieces: nothing is written when the batch has more
    const LaneToken k = lane_token<kBpeBlock>(T);
    const int lane = threadIdx.x & 63;
    const TokenBytes b = k.b;
    const BpeTable& bt = sp.bt;
    LATOK_BPE_VIEW(bt);
    const int32_t* const byte_ids = sp.byte_ids;
    const bool bytes = byte_ids != nullptr;
    const bool fuse = !bytes && sp.fuse_unk;
    int64_t at = 0;
    int64_t n_mine = 0;
    if (b.ok) {
        at = rank[k.t];
        n_mine = rank[k.t + 1] - at;   // (rank has n_tok + 1 entries)
    }
    const bool mine = b.ok && n_mine >= 1 && at >= 0 && at + n_mine <= cap;
    SpSeg g;
    if (mine) g = sp_segment(ld, b.a, b.e, sp_dummy_of(sp, k), bt.max_bytes);
    const bool wide = mine && !g.over && g.VL > kSpLaneBytes;
    if (mine && !wide) {
        const int64_t base = k.base;
        if (g.over) {
            bpe_store<OUT>(ids, spans, at, unk, b.a - base, b.e - base);
        } else {   // the parts the count pass left: one lookup each
            const int L = (int)g.VL;
            const auto vld = sp_virtual(ld, g);
            int64_t ord = 0;
            const auto put = [&](int32_t id, int64_t lo, int64_t hi) {   // (the count pass bounds every store)
                if (ord < n_mine) bpe_store<OUT>(ids, spans, at + ord, id, lo, hi);
                ++ord;
            };
            bool run = false;
            int64_t run_lo = 0, run_hi = 0;
            uint64_t m = (masks[k.t] & bpe_mask_all(L)) | 1ull;
            while (m) {
                const int i = (int)__builtin_ctzll(m);
                m &= m - 1ull;
                const int p = m ? (int)__builtin_ctzll(m) : L;
                const uint32_t r = bpe_look(vld, i, p, tab, seed);
                const int64_t lo = sp_real(ld, g, i) - base, hi = sp_real(ld, g, p) - base;
                if (r != kBpeAbsent) {
                    if (run) put(unk, run_lo, run_hi);
                    run = false;
                    put(bpe_id(bt, r, unk), lo, hi);
                } else if (bytes) {
                    for (int v = i; v < p; ++v) put(byte_ids[wp_byte(vld, v)], lo, hi);
                } else if (fuse) {
                    if (!run) run_lo = lo;
                    run = true;
                    run_hi = hi;
                } else {
                    put(unk, lo, hi);
                }
            }
            if (run) put(unk, run_lo, run_hi);
        }
    }
    const int dummy_mine = mine ? g.dummy : 0;
    for (uint64_t todo = __ballot(wide); todo; todo &= todo - 1ull) {
        const int src = (int)__builtin_ctzll(todo);
        const int64_t a = lane_read64(b.a, src), e = lane_read64(b.e, src);
        const int64_t at_w = lane_read64(at, src), n_w = lane_read64(n_mine, src), base = lane_read64(k.base, src);
        const SpSeg w = sp_segment(ld, a, e, lane_read(dummy_mine, src), bt.max_bytes);
        const int L = (int)w.VL;
        const auto vld = sp_virtual(ld, w);
        const auto look = [&](int i, int p) { return bpe_look(vld, i, p, tab, seed); };
        const int64_t P = w.P;
        auto s = sp_wave_state(s_rank + (threadIdx.x & ~63), look, lane, [&](int v) { return sp_vstart(vld, P, v); }, (int)bt.max_len);
        bpe_merge(L, s);
        int64_t ord = 0;
        if (fuse) {   // one part after the other, every lane the same walk, the source lane stores
            bool run = false;
            int64_t run_lo = 0;
            const auto put = [&](int32_t id, int64_t lo, int64_t hi) {
                if (lane == src && ord < n_w) bpe_store<OUT>(ids, spans, at_w + ord, id, lo, hi);
                ++ord;
            };
            for (int i = 0; i < L;) {
                const int p = s.start_next(i, L);
                const uint32_t r = look(i, p);
                const int64_t lo = sp_real(ld, w, i) - base;
                if (r != kBpeAbsent) {
                    if (run) put(unk, run_lo, lo);
                    run = false;
                    put(bpe_id(bt, r, unk), lo, sp_real(ld, w, p) - base);
                } else if (!run) {
                    run = true;
                    run_lo = lo;
                }
                i = p;
            }
            if (run) put(unk, run_lo, e - base);
            wave_lds_sync();
            continue;
        }
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
            const bool have = lane < got;
            uint32_t r = kBpeAbsent;
            if (have) r = look(my_i, my_p);
            const int c = !have ? 0 : (r != kBpeAbsent || !bytes ? 1 : my_p - my_i);
            const int incl = shfl_scan_add(c, lane);
            const int64_t first = ord + incl - c;   // my first piece inside the segment
            if (have) {
                const int64_t lo = sp_real(ld, w, my_i) - base, hi = sp_real(ld, w, my_p) - base;
                if (r != kBpeAbsent || !bytes) {
                    if (first < n_w) bpe_store<OUT>(ids, spans, at_w + first, bpe_id(bt, r, unk), lo, hi);
                } else {
                    for (int v = 0; v < c && first + v < n_w; ++v) bpe_store<OUT>(ids, spans, at_w + first + v, byte_ids[wp_byte(vld, my_i + v)], lo, hi);
                }
            }
            ord += lane_read(incl, 63);
        }
        wave_lds_sync();
    }
}

// ---- launchers -----------------------------------------------------------------------------------------------------
hipError_t launch_spbpe_count(const TokenText& t, const SpBpeTable& sp, int64_t* cnt, uint64_t* masks, hipStream_t st) {
    if (t.n_str <= 0 || t.n_tok <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)((t.n_tok + 1 + kBpeBlock - 1) / kBpeBlock);   // (+ 1: the entry behind the last token)
    hipLaunchKernelGGL(k_spbpe_count, dim3(blocks), dim3(kBpeBlock), 0, st, t, sp, cnt, masks);
    return hipGetLastError();
}

hipError_t launch_spbpe_emit(bool out32, const TokenText& t, const SpBpeTable& sp, int32_t unk_id, const int64_t* rank, const uint64_t* masks,
                             const int64_t* n_pieces_dev, int64_t cap, int32_t* ids, void* spans, hipStream_t st) {
    if (t.n_str <= 0 || t.n_tok <= 0 || !ids) return hipSuccess;
    const dim3 grid((unsigned)((t.n_tok + kBpeBlock - 1) / kBpeBlock)), block(kBpeBlock);
    if (out32) hipLaunchKernelGGL((k_spbpe_emit<int32_t>), grid, block, 0, st, t, sp, unk_id, rank, masks, n_pieces_dev, cap, ids, (int32_t*)spans);
    else hipLaunchKernelGGL((k_spbpe_emit<int64_t>), grid, block, 0, st, t, sp, unk_id, rank, masks, n_pieces_dev, cap, ids, (int64_t*)spans);
    return hipGetLastError();
}

}  // namespace latok
