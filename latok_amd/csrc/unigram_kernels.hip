// unigram_kernels.hip -- Unigram (Viterbi) piece ids of a UTF-8 batch in byte space: the kernels behind
// latok_unigram_ids_utf8_bytes_batch and latok_unigram_padded_utf8_bytes_batch.  They work in TOKEN space, one lane per token, behind
// the same front as the WordPiece and BPE kernels: the span record of every token at its rank, the row starts in token space.  The row
// pointers and the padded block are k_wp_rows and k_wp_pad of wordpiece_kernels.hip, called as they are.
//
//   k_uni_count  pieces of token t = what the forward pass and the backtrack of unigram.h leave -> cnt[t]; cnt[n_tok] = 0, so that the
//                scan of the n_tok + 1 entries leaves the piece total behind the last token's rank.  For a token of the lane form it
//                also leaves three words in marks[]: the piece starts, which of them are unknown, and whether the marker's piece is, so
//                that the emit pass neither searches again nor asks the table whether a (fused) part is unknown
//   k_uni_emit   behind the scan, only if the piece total fits the capacity: ids[rank[t] + k] (through the position -> id array), and
//                the piece's string-relative byte range if asked for.  Nothing is ever written outside the token's own range of ranks
//
// A token is MARKED if the marker is not empty and it is the first token of its string or the token before it ends in front of it.
// Two forms of the walk, both uni_forward / uni_backtrack of unigram.h on a state of their own:
//   lane form    a token of at most kUniLaneBytes = 64 bytes, by its lane: the positions are a 64-bit mask in registers, best and back
//                two lane-private columns in LDS laid out [node][lane], so that a wave's access to one node is 64 consecutive dwords:
//                conflict-free
//   wave form    a token of 65 .. max_bytes bytes, by its whole wave, after the wave's lane tokens are done: the long tokens are
//                taken one at a time (ballot, lowest lane first, the range broadcast by v_readlane).  The wave's own LDS slices -- 66
//                nodes x 64 lanes = 4224 entries each -- hold best and back of the whole token (64 consecutive nodes are 64
//                consecutive dwords).  The starts go in ascending order; for one start the 64 lanes take the candidate ends 64 at a
//                time, each lane the update of its own end: no two lanes of a step write the same node, and because the starts ascend
//                and the comparison is strict the lower start stays with no cross-lane tie-break.  The emit pass runs the forward
//                pass again; lane 0 walks back and leaves one record per piece at the piece's start node (in the slice that held
//                best); the lanes then sweep the nodes 64 at a time, number the records by ballot and store them
// 2 x 66 x 128 x 4 = 67 584 B of LDS per workgroup of 128: two workgroups per CU.  The text is read as aligned dwords of the token's own
// range.  A token that is not ok (lane_token of block_ops.h) is skipped, so no load leaves the buffer whatever the workspace holds.  No
// kernel here waits for another workgroup; all stores are vector stores from plain C++.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_ops.h"
#include "kernels.h"
#include "unigram.h"

namespace latok {

static_assert(kUniBlock % 64 == 0 && kUniLaneBytes == 64, "the wave's LDS slice is 66 nodes x 64 lanes");
static_assert(kUniLaneNodes * 64 >= kUniMaxBytes + 2, "the wave's slice holds the nodes of the longest token");
static_assert((uint32_t)(kUniMaxBytes + 1) <= kUniStartMask, "a start node fits its field of back[]");

constexpr uint32_t kUniRecBit = 0x40000000u;   // a piece record of the wave form: a piece starts at this node

#define LATOK_UNI_VIEW(ut)                                                                                                          \
    const VtSlot* const slots_p = reinterpret_cast<const VtSlot*>((ut).plain.slots);                                                \
    const VtSlot* const slots_m = reinterpret_cast<const VtSlot*>((ut).marked.slots);                                               \
    const uint32_t* const blob_p = (ut).plain.blob;                                                                                 \
    const uint32_t* const blob_m = (ut).marked.blob;                                                                                \
    const uint32_t* const text = T.text;                                                                                            \
    const uint32_t seed = (ut).plain.seed;                                                                                          \
    const int32_t marker_pos = (ut).marker_pos;                                                                                     \
    const float* const pos_score = (ut).pos_score;                                                                                  \
    const int64_t n_words = (ut).n_words;                                                                                           \
    const auto ld = [text](int64_t i) { return text[i]; };                                                                          \
    const auto tab_p = wp_table_view([slots_p](uint64_t i) { return slots_p[i]; }, [blob_p](uint64_t i) { return blob_p[i]; },     \
                                     (ut).plain.n_slots, (ut).max_len_plain);                                                       \
    const auto tab_m = wp_table_view([slots_m](uint64_t i) { return slots_m[i]; }, [blob_m](uint64_t i) { return blob_m[i]; },     \
                                     (ut).marked.n_slots, (ut).max_len_marked);                                                     \
    const auto score = [pos_score, n_words](uint32_t w) { return (int64_t)w < n_words ? pos_score[w] : 0.0f; }

// 1: the lane's token is marked
__device__ __forceinline__ int uni_marked(const TokenText& T, const LaneToken& k, int marker_len) {
    if (!k.b.ok || marker_len <= 0) return 0;
    if (k.t <= 0 || k.t <= T.row_start[k.row]) return 1;   // the first token of its string
    return T.tok_spans[2 * (k.t - 1) + 1] < k.b.a - k.base ? 1 : 0;   // whitespace was dropped in front of it
}
__device__ __forceinline__ int uni_reach(uint32_t max_len) { return max_len > (uint32_t)kUniMaxBytes ? kUniMaxBytes + 2 : (int)max_len; }

// a lane's columns of the workgroup's two arrays: node v at p[v * kUniBlock]
struct UniLdsColumns {
    uint32_t* best_p;
    uint32_t* back_p;
    __device__ __forceinline__ float best(int v) const { return __uint_as_float(best_p[v * kUniBlock]); }
    __device__ __forceinline__ void set_best(int v, float x) const { best_p[v * kUniBlock] = __float_as_uint(x); }
    __device__ __forceinline__ uint32_t back(int v) const { return back_p[v * kUniBlock]; }
    __device__ __forceinline__ void set_back(int v, uint32_t b) const { back_p[v * kUniBlock] = b; }
};

// The wave form's state.  Every member function is called by all 64 lanes with wave-uniform arguments and returns a wave-uniform value.
template <class Look, class Score>
struct UniWaveState {
    uint32_t* best_s;   // the wave's 64 columns of either array: node v at [(v >> 6) * kUniBlock + (v & 63)]
    uint32_t* back_s;
    Look look;
    Score score;
    int lane, mk;
    float unk_score;
    uint64_t bits;      // bit x: text offset 64 lane + x is a position: the one statement of it, for next_pos and for the candidate ends
    bool record;        // the backtrack leaves piece records in best_s
    __device__ __forceinline__ static int at(int v) { return (v >> 6) * kUniBlock + (v & 63); }
    __device__ __forceinline__ uint64_t word(int l) const { return (uint64_t)lane_read64((int64_t)bits, to_scalar(l)); }
    // node j, 0 < j < N, is a position: the bit of its text offset, read from the lane that holds it.  Called by all 64 lanes, each with its own j
    __device__ __forceinline__ bool is_pos(int j) const {
        const int x = j - mk;
        const uint64_t w = (uint64_t)__shfl((unsigned long long)bits, (x >> 6) & 63);
        return ((w >> (x & 63)) & 1ull) != 0ull;
    }
    __device__ __forceinline__ void begin(int N) {
        for (int base = 0; base <= N; base += 64) {
            const int v = base + lane;
            if (v <= N) back_s[at(v)] = v == 0 ? 0u : kUniUnset;
        }
        if (lane == 0) best_s[at(0)] = __float_as_uint(0.0f);
    }
    __device__ __forceinline__ int next_pos(int i, int N) const {
        const int x = i - mk + 1, l = x >> 6;
        if (l >= 64) return N;
        const int n = uni_mask_from(word(l), x & 63);
        int found = -1;
        if (n < 64) {
            found = 64 * l + n;
        } else {
            const uint64_t later = l >= 63 ? 0ull : __ballot(bits != 0ull) & (~0ull << (l + 1));
            if (later) {
                const int l2 = (int)__builtin_ctzll(later);
                found = 64 * l2 + (int)__builtin_ctzll(word(l2));
            }
        }
        return found >= 0 && found + mk < N ? found + mk : N;
    }
    __device__ __forceinline__ void update(int j, float cand, uint32_t b) const {
        if (back_s[at(j)] == kUniUnset || cand > __uint_as_float(best_s[at(j)])) {
            best_s[at(j)] = __float_as_uint(cand);
            back_s[at(j)] = b;
        }
    }
    __device__ __forceinline__ bool words(int i, int j1, int hi, int N) const {
        wave_lds_sync();   // (what the starts before this one stored)
        const float from = __uint_as_float(best_s[at(i)]);
        bool single = false;
        for (int base = j1; base <= hi; base += 64) {   // the candidate ends, 64 at a time: each lane the update of its own end
            const int j = base + lane;
            const bool pos = is_pos(j < N ? j : 1);   // (every lane takes part in the exchange)
            bool hit = false;
            if (j <= hi && (j == N || pos)) {
                const uint32_t w = look(i, j);
                if (w != kUniAbsent) {
                    update(j, from + score(w), (uint32_t)i);
                    hit = true;
                }
            }
            if (base == j1) single = (__ballot(hit) & 1ull) != 0ull;   // (lane 0 holds j1)
        }
        return single;
    }
    __device__ __forceinline__ void unknown(int i, int j1) const {
        if (lane == 0) update(j1, __uint_as_float(best_s[at(i)]) + unk_score, (uint32_t)i | kUniUnkBit);
    }
    __device__ __forceinline__ uint32_t back_of(int p) const { return back_s[at(p)]; }
    __device__ __forceinline__ void part(int i, int p, bool unk, bool joins, int end) const {
        if (!record || lane != 0) return;
        best_s[at(i)] = (uint32_t)end | kUniRecBit | (unk ? kUniUnkBit : 0u);
        if (joins) best_s[at(p)] = 0u;   // the right neighbour is no piece of its own any more
    }
};
template <class Look, class Score>
__device__ __forceinline__ UniWaveState<Look, Score> uni_wave_state(uint32_t* best_s, uint32_t* back_s, Look look, Score score, int lane, int mk,
                                                                    float unk_score, uint64_t bits, bool record) {
    return UniWaveState<Look, Score>{best_s, back_s, look, score, lane, mk, unk_score, bits, record};
}
// the positions among the text offsets 64 lane .. 64 lane + 63 of the token [a, a + L)
template <class TextLoad>
__device__ __forceinline__ uint64_t uni_wave_bits(TextLoad ld, int64_t a, int L, int lane, int mk) {
    const int mine = L - 64 * lane;
    uint64_t bits = mine <= 0 ? 0ull : uni_char_starts(ld, a + 64 * lane, mine < 64 ? mine : 64);
    if (!mk && lane == 0) bits |= 1ull;
    return bits;
}

__global__ __launch_bounds__(kUniBlock) void k_uni_count(TokenText T, UniTable ut, int64_t* __restrict__ cnt, uint64_t* __restrict__ marks) {
    __shared__ uint32_t s_best[kUniLaneNodes * kUniBlock];
    __shared__ uint32_t s_back[kUniLaneNodes * kUniBlock];
    const LaneToken k = lane_token<kUniBlock>(T);
    const int lane = threadIdx.x & 63;
    const TokenBytes b = k.b;
    const int mk = uni_marked(T, k, ut.marker_len);
    const int64_t len = b.ok ? b.e - b.a : 0;
    const bool wide = len > kUniLaneBytes && len <= (int64_t)ut.max_bytes;
    LATOK_UNI_VIEW(ut);
    const int reach = uni_reach(ut.max_len_plain), reach_m = uni_reach(ut.max_len_marked) + 1;
    const float unk_score = ut.unk_score;
    int64_t n = 0;
    uint64_t starts = 1ull, unks = 0ull, head = 0ull;
    if (b.ok && !wide) {
        n = 1;   // (longer than max_bytes: one unknown piece)
        if (len <= (int64_t)ut.max_bytes) {
            const int64_t a = b.a;
            const int L = (int)len;
            uint64_t pos = uni_char_starts(ld, a, L);
            if (!mk) pos |= 1ull;
            auto s = uni_lane_state(UniLdsColumns{s_best + threadIdx.x, s_back + threadIdx.x},
                                    [&](int i, int j) { return uni_look(ld, a, mk, i, j, tab_p, tab_m, marker_pos, seed); }, score, pos, mk, unk_score);
            uni_forward(L + mk, mk ? reach_m : reach, reach, s);
            n = uni_backtrack(L + mk, ut.fuse_unk, s);
            starts = s.starts;
            unks = s.unks;
            head = (uint64_t)s.head_unk;
        }
    }
    // the long tokens of the wave, one at a time by the whole wave (wave-uniform loop: `todo` is a ballot)
    uint32_t* const best_s = s_best + (threadIdx.x & ~63);
    uint32_t* const back_s = s_back + (threadIdx.x & ~63);
    for (uint64_t todo = __ballot(wide); todo; todo &= todo - 1ull) {
        const int src = (int)__builtin_ctzll(todo);
        const int64_t a = lane_read64(b.a, src), e = lane_read64(b.e, src);
        const int mkw = lane_read(mk, src);
        const int L = (int)(e - a), N = L + mkw;
        auto s = uni_wave_state(best_s, back_s, [&](int i, int j) { return uni_look(ld, a, mkw, i, j, tab_p, tab_m, marker_pos, seed); }, score,
                                lane, mkw, unk_score, uni_wave_bits(ld, a, L, lane, mkw), false);
        uni_forward(N, mkw ? reach_m : reach, reach, s);
        wave_lds_sync();
        const int parts = uni_backtrack(N, ut.fuse_unk, s);
        if (lane == src) n = parts;
        wave_lds_sync();   // (the next token's begin behind this one's last reads)
    }
    if (k.t <= T.n_tok) cnt[k.t] = n;   // (t == n_tok: the entry behind the last token)
    if (k.t < T.n_tok) {
        marks[k.t] = starts;
        marks[T.n_tok + k.t] = unks;
        marks[2 * T.n_tok + k.t] = head;
    }
}

template <typename OUT>
__device__ __forceinline__ void uni_store(int32_t* __restrict__ ids, OUT* __restrict__ spans, int64_t at, int32_t id, int64_t s, int64_t e) {
    typedef OUT out2 __attribute__((ext_vector_type(2)));
    __builtin_nontemporal_store(id, ids + at);
    if (spans) {
        out2 v;
        v.x = (OUT)s;
        v.y = (OUT)e;
        __builtin_nontemporal_store(v, reinterpret_cast<out2*>(spans) + at);
    }
}
__device__ __forceinline__ int32_t uni_id(const UniTable& ut, uint32_t w, int32_t unk) {
    return (int64_t)w < ut.n_words ? ut.pos_id[w] : unk;   // (kUniAbsent is no position)
}

template <typename OUT>
__global__ __launch_bounds__(kUniBlock) void k_uni_emit(TokenText T, UniTable ut, int32_t unk, const int64_t* __restrict__ rank,
                                                        const uint64_t* __restrict__ marks, const int64_t* __restrict__ n_pieces_dev,
                                                        int64_t cap, int32_t* __restrict__ ids, OUT* __restrict__ spans) {
    __shared__ uint32_t s_best[kUniLaneNodes * 64 * (kUniBlock / 64)];
    __shared__ uint32_t s_back[kUniLaneNodes * 64 * (kUniBlock / 64)];
    if (*n_pieces_dev > cap) return;   // the caller's buffers hold `cap` pieces: nothing is written when the batch has more
    const LaneToken k = lane_token<kUniBlock>(T);
    const int lane = threadIdx.x & 63;
    const TokenBytes b = k.b;
    const int mk = uni_marked(T, k, ut.marker_len);
    int64_t at = 0;
    int64_t n_mine = 0;
    if (b.ok) {
        at = rank[k.t];
        n_mine = rank[k.t + 1] - at;   // (rank has n_tok + 1 entries)
    }
    const bool mine = b.ok && n_mine >= 1 && at >= 0 && at + n_mine <= cap;
    const int64_t len = mine ? b.e - b.a : 0;
    const bool wide = len > kUniLaneBytes && len <= (int64_t)ut.max_bytes;
    LATOK_UNI_VIEW(ut);
    if (mine && !wide) {
        const int64_t a = b.a, rel = b.a - k.base;
        if (len > (int64_t)ut.max_bytes) {
            uni_store<OUT>(ids, spans, at, unk, rel, rel + len);
        } else {   // the pieces the count pass left: one lookup for each that is a word
            uni_lane_parts(marks[k.t], marks[T.n_tok + k.t], (int)(marks[2 * T.n_tok + k.t] & 1ull), (int)len, mk, [&](int ord, bool is_unk, int i, int j) {
                if (ord >= n_mine) return;
                const int32_t id = is_unk ? unk : uni_id(ut, uni_look(ld, a, mk, i, j, tab_p, tab_m, marker_pos, seed), unk);
                uni_store<OUT>(ids, spans, at + ord, id, uni_span_start(rel, mk, i), uni_span_end(rel, mk, j));
            });
        }
    }
    const int reach = uni_reach(ut.max_len_plain), reach_m = uni_reach(ut.max_len_marked) + 1;
    uint32_t* const best_s = s_best + (threadIdx.x & ~63);
    uint32_t* const back_s = s_back + (threadIdx.x & ~63);
    for (uint64_t todo = __ballot(wide); todo; todo &= todo - 1ull) {
        const int src = (int)__builtin_ctzll(todo);
        const int64_t a = lane_read64(b.a, src), e = lane_read64(b.e, src);
        const int64_t at_w = lane_read64(at, src), n_w = lane_read64(n_mine, src), rel = a - lane_read64(k.base, src);
        const int mkw = lane_read(mk, src);
        const int L = (int)(e - a), N = L + mkw;
        auto s = uni_wave_state(best_s, back_s, [&](int i, int j) { return uni_look(ld, a, mkw, i, j, tab_p, tab_m, marker_pos, seed); }, score,
                                lane, mkw, ut.unk_score, uni_wave_bits(ld, a, L, lane, mkw), true);
        uni_forward(N, mkw ? reach_m : reach, reach, s);
        wave_lds_sync();
        for (int base = 0; base <= N; base += 64)   // best is done with: its slice takes the piece records
            if (base + lane <= N) best_s[s.at(base + lane)] = 0u;
        wave_lds_sync();
        uni_backtrack(N, ut.fuse_unk, s);
        wave_lds_sync();
        int64_t ord = 0;
        for (int base = 0; base < N; base += 64) {   // the records in node order, 64 nodes at a time, numbered by ballot
            const int i = base + lane;
            const uint32_t v = i < N ? best_s[s.at(i)] : 0u;
            const bool piece = (v & kUniRecBit) != 0u;
            const uint64_t pieces = __ballot(piece);
            const int64_t o = ord + __builtin_popcountll(pieces & ((1ull << lane) - 1ull));
            const int j = (int)(v & kUniStartMask);
            if (piece && o < n_w && j > i && j <= N) {
                const int32_t id = (v & kUniUnkBit) ? unk : uni_id(ut, uni_look(ld, a, mkw, i, j, tab_p, tab_m, marker_pos, seed), unk);
                uni_store<OUT>(ids, spans, at_w + o, id, uni_span_start(rel, mkw, i), uni_span_end(rel, mkw, j));
            }
            ord += __builtin_popcountll(pieces);
        }
        wave_lds_sync();
    }
}

// ---- launchers -----------------------------------------------------------------------------------------------------
hipError_t launch_uni_count(const TokenText& t, const UniTable& ut, int64_t* cnt, uint64_t* marks, hipStream_t st) {
    if (t.n_str <= 0 || t.n_tok <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)((t.n_tok + 1 + kUniBlock - 1) / kUniBlock);   // (+ 1: the entry behind the last token)
    hipLaunchKernelGGL(k_uni_count, dim3(blocks), dim3(kUniBlock), 0, st, t, ut, cnt, marks);
    return hipGetLastError();
}

hipError_t launch_uni_emit(bool out32, const TokenText& t, const UniTable& ut, int32_t unk_id, const int64_t* rank, const uint64_t* marks,
                           const int64_t* n_pieces_dev, int64_t cap, int32_t* ids, void* spans, hipStream_t st) {
    if (t.n_str <= 0 || t.n_tok <= 0 || !ids) return hipSuccess;
    const dim3 grid((unsigned)((t.n_tok + kUniBlock - 1) / kUniBlock)), block(kUniBlock);
    if (out32) hipLaunchKernelGGL((k_uni_emit<int32_t>), grid, block, 0, st, t, ut, unk_id, rank, marks, n_pieces_dev, cap, ids, (int32_t*)spans);
    else hipLaunchKernelGGL((k_uni_emit<int64_t>), grid, block, 0, st, t, ut, unk_id, rank, marks, n_pieces_dev, cap, ids, (int64_t*)spans);
    return hipGetLastError();
}

}  // namespace latok
