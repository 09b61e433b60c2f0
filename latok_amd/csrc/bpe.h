// bpe.h -- the byte-level BPE cut of one token (bpe_kernels.hip: k_bpe_count, k_bpe_emit): the merge walk over the token's bytes by
// the ranks of a vocabulary.  Plain C++17, like wordpiece.h: the build runs on the host only; the walk compiles on the host
// (tests/helpers/bpe_harness.cpp runs it against a plain-Python restatement of the definition) and, under hipcc, on the device.
//
//   table      ONE vocab_table.h table built by vt_build, unchanged, without ids: the id slot holds the word's RANK, its position in
//              the list.  Of duplicate words the first wins, so the lowest rank is kept; the empty word gets no slot.  Beside it an
//              int32 array rank -> id (the identity when no ids are given) and the byte length of the longest word.
//   lookup     the concatenation of two adjacent parts is the contiguous bytes [s_i, s_(i+2)) of the text: bpe_look hashes and
//              compares them in place (wp_find of wordpiece.h: aligned dwords through a loader, the index clamped to the dword of
//              the span's last byte).  No bytes are copied or joined.  A span longer than the longest word needs no probe.
//   the cut    token T = bytes [a, e), L = e - a.  L > max_bytes: ONE piece (unk, a, e).  T is a word: ONE piece (id(T), a, e).
//              Else the parts are the L single bytes; repeat: among all adjacent parts whose concatenation is a word, the pair with the
//              LOWEST rank, of equal ranks the LEFTMOST, becomes one part; stop when no adjacent pair is a word.  Every remaining part
//              is a piece: a word's id, or unk (a single byte only: every merged part is a word).
//   the walk   bpe_merge is the one statement of the repeat step.  It works on a STATE that says where the part starts and the pair
//              ranks live and how the minimum is found: BpeLaneState below (a 64-bit start mask; the lane form of the kernels and the
//              host harness), the wave form of bpe_kernels.hip (64 start words, one per lane, the ranks in LDS), the wide host state
//              of the harness.  rank(i) is kept for every part start i: the rank of the part at i joined with the next, kBpeAbsent if
//              that is no word or i is the last part.
//   bounds     every one of the token's L - 1 initial pairs is looked up once (fill); a merge looks up at most two new pairs, the
//              left and the right neighbour's; ranks are stored, never recomputed; the minimum search rescans the stored ranks.
//              The loop runs by its own counter: at most L - 1 rounds.  With the whole-token lookup in front and one lookup per
//              remaining part behind: at most 1 + (L - 1) + 2 merges + parts lookups per token.
#ifndef LATOK_BPE_H
#define LATOK_BPE_H
#include <stdint.h>

#include "wordpiece.h"

constexpr int kBpeMaxBytes = 4096;           // max_bytes at most
constexpr int kBpeLaneBytes = 64;            // a token of at most this many bytes keeps its part starts in one 64-bit mask
constexpr uint32_t kBpeAbsent = 0xFFFFFFFFu; // the rank of a pair that is no word (n_words < 2^31: no rank is that large)

// the rank of bytes [s, p) of the text, p > s, or kBpeAbsent
template <class TextLoad, class Table>
TH_FN uint32_t bpe_look(TextLoad ld, int64_t s, int64_t p, const Table& t, uint32_t seed) {
    if (p - s > (int64_t)t.max_len) return kBpeAbsent;
    int32_t rank = 0;
    return wp_find(ld, s, p, t, seed, &rank) ? (uint32_t)rank : kBpeAbsent;
}

// The merge walk of a token of L >= 1 bytes, positions token-relative.  The state S:
//   fill(L)                         every position a part start; rank(i) = look(i, i + 2) for i + 2 <= L, kBpeAbsent for i = L - 1
//   argmin(L, &r)                   the leftmost part start with the lowest stored rank, r = that rank (kBpeAbsent: no pair is a word)
//   start_next(i, L)                the next part start behind i, L if there is none;  start_prev(i): the one before i > 0
//   start_clear(j) / set_rank(i, r)
//   look2(h, k, i, q, &rl, &rr)     rl = h >= 0 ? look(h, k) : kBpeAbsent;  rr = q > k ? look(i, q) : kBpeAbsent
// Returns the number of parts left.
template <class S>
TH_FN int bpe_merge(int L, S& s) {
    s.fill(L);
    int parts = L;
    for (int round = 0; round + 1 < L; ++round) {
        uint32_t r = kBpeAbsent;
        const int i = s.argmin(L, &r);
        if (r == kBpeAbsent) break;
        const int j = s.start_next(i, L);                // the parts [i, j) and [j, k) become [i, k)
        if (j >= L) break;                               // (cannot be: the last part's rank is absent)
        const int k = s.start_next(j, L);
        const int h = i > 0 ? s.start_prev(i) : -1;      // the left neighbour [h, i), if any
        const int q = k < L ? s.start_next(k, L) : k;    // the right neighbour [k, q), if any
        s.start_clear(j);
        uint32_t rl = kBpeAbsent, rr = kBpeAbsent;
        s.look2(h, k, i, q, &rl, &rr);
        s.set_rank(j, kBpeAbsent);
        s.set_rank(i, rr);
        if (h >= 0) s.set_rank(h, rl);
        --parts;
    }
    return parts;
}

// bit helpers of a 64-bit start mask: the lowest start above bit i (64: none), the highest below bit i > 0
TH_FN int bpe_mask_next(uint64_t m, int i) {
    const uint64_t above = i >= 63 ? 0ull : m & (~0ull << (i + 1));
    return above ? (int)__builtin_ctzll(above) : 64;
}
TH_FN int bpe_mask_prev(uint64_t m, int i) {
    const uint64_t below = m & ((1ull << i) - 1ull);
    return below ? 63 - (int)__builtin_clzll(below) : 0;
}
TH_FN uint64_t bpe_mask_all(int L) { return L >= 64 ? ~0ull : (1ull << L) - 1ull; }

// The state of a token of at most kBpeLaneBytes bytes walked by one thread: the part starts are the bits of `mask`, the ranks live
// where `Ranks` puts them (get(i) / set(i, r), i < 64: an LDS column on the device, an array in the harness), look(i, k) = the rank
// of the token's bytes [i, k).
template <class Ranks, class Look>
struct BpeLaneState {
    Ranks ranks;
    Look look;
    uint64_t mask;
    TH_FN void fill(int L) {
        mask = bpe_mask_all(L);
        for (int i = 0; i + 2 <= L; ++i) ranks.set(i, look(i, i + 2));
        ranks.set(L - 1, kBpeAbsent);
    }
    TH_FN int argmin(int, uint32_t* r) const {
        uint32_t best = kBpeAbsent;
        int at = 0;
        for (uint64_t m = mask; m; m &= m - 1ull) {   // ascending: of equal ranks the first stays
            const int i = (int)__builtin_ctzll(m);
            const uint32_t v = ranks.get(i);
            if (v < best) {
                best = v;
                at = i;
            }
        }
        *r = best;
        return at;
    }
    TH_FN int start_next(int i, int L) const {
        const int n = bpe_mask_next(mask, i);
        return n < L ? n : L;
    }
    TH_FN int start_prev(int i) const { return bpe_mask_prev(mask, i); }
    TH_FN void start_clear(int j) { mask &= ~(1ull << j); }
    TH_FN void set_rank(int i, uint32_t r) { ranks.set(i, r); }
    TH_FN void look2(int h, int k, int i, int q, uint32_t* rl, uint32_t* rr) const {
        *rl = h >= 0 ? look(h, k) : kBpeAbsent;
        *rr = q > k ? look(i, q) : kBpeAbsent;
    }
};
template <class Ranks, class Look>
TH_FN BpeLaneState<Ranks, Look> bpe_lane_state(Ranks ranks, Look look) {
    return BpeLaneState<Ranks, Look>{ranks, look, 0ull};
}

// The first two steps of the cut, which need no state: 1 = the token is one piece whose rank is *rank (kBpeAbsent: unk, the token is
// longer than max_bytes), 0 = the token has to be walked.
template <class TextLoad, class Table>
TH_FN int bpe_whole(TextLoad ld, int64_t a, int64_t e, const Table& t, uint32_t seed, int max_bytes, uint32_t* rank) {
    *rank = kBpeAbsent;
    if (e - a > (int64_t)max_bytes) return 1;
    *rank = bpe_look(ld, a, e, t, seed);
    return *rank != kBpeAbsent ? 1 : 0;
}

// ---- the build: host only ---------------------------------------------------------------------------------------------------
struct BpeTables {
    VtTable table;                   // id slot = rank
    std::vector<int32_t> rank_id;    // at least one entry, so that its address is never NULL
    uint32_t max_len = 0;            // bytes of the longest word
};
// words / word_off / ids as vt_build takes them.  The caller has checked the offsets and the sizes.
inline void bpe_build(const uint8_t* words, const int64_t* word_off, int64_t n_words, const int32_t* ids, uint32_t seed, BpeTables* t) {
    vt_build(words, word_off, n_words, nullptr, seed, &t->table);
    t->rank_id.assign((size_t)(n_words > 0 ? n_words : 1), 0);
    t->max_len = 0;
    for (int64_t i = 0; i < n_words; ++i) {
        t->rank_id[(size_t)i] = ids ? ids[i] : (int32_t)i;
        const uint64_t len = (uint64_t)(word_off[i + 1] - word_off[i]);
        if (len > t->max_len) t->max_len = (uint32_t)len;
    }
}

#endif
