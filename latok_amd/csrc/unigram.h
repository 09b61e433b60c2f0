// unigram.h -- the Unigram cut of one token (unigram_kernels.hip: k_uni_count, k_uni_emit): the best-scoring split of the token into
// words of a scored vocabulary, found by a dynamic programme over the token's character positions (Viterbi).  Plain C++17, like bpe.h
// and wordpiece.h: the build runs on the host only; the walk compiles on the host (tests/helpers/unigram_harness.cpp runs it against a
// plain-Python restatement of the definition) and, under hipcc, on the device.
//
//   tables     TWO vocab_table.h tables built by vt_build, unchanged, as WordPiece keeps two.  PLAIN: every word.  MARKED: every word
//              that begins with the marker and is longer than it, stored WITHOUT the marker.  In both the id slot holds the word's
//              POSITION in the list; of duplicate words the first wins, the empty word gets no slot.  Beside them an int32 array
//              position -> id (the identity when no ids are given), a float32 array position -> score, the longest word of either
//              table in bytes and the position of the word that is the marker alone (-1: none).
//   nodes      token T = bytes [a, e), L = e - a, mk = 1 if T is marked else 0.  The virtual text (marker + T, or T) is never
//              materialised: NODE v in 0 .. N, N = L + mk, stands for text offset v - mk; node 0 of a marked token is the marker's
//              first byte.  A node is a POSITION if it is 0 or N or the byte at its text offset is no continuation byte
//              ((b & 0xC0) != 0x80): the character rule of chargram_text.h on the virtual text.  (The marker is one character, so
//              its later bytes are no positions and need no node.)
//   lookup     uni_look(i, j): nodes [0, 1) of a marked token: the marker-alone entry.  [0, j), j > 1: text [a, a + j - 1) in MARKED.
//              Else text [a + i - mk, a + j - mk) in PLAIN.  All through wp_find of wordpiece.h on the text in place.  A span longer
//              than the table's longest word needs no probe.
//   forward    uni_forward is the one statement of the forward pass: best[0] = 0.0f, every other node unset; for the positions i in
//              ascending order, for every position j behind i within the longest word's reach whose nodes [i, j) are a word w:
//              cand = best[i] + score(w), ONE float32 addition; best[j] unset or cand > best[j] (strictly): best[j] = cand,
//              back[j] = i.  If the single character at i is no word the same update is tried for the next position with unk_score,
//              back[j] = i | kUniUnkBit.  So every position is set when the loop reaches it, and of equal scores the lower start stays.
//   backtrack  uni_backtrack is the one statement of the walk back from N through back[].  With fuse, a piece that is unknown and
//              whose right neighbour is unknown JOINS it: the state is told so, and the piece count does not grow.
//   states     both are function templates over a STATE that says where best / back live: UniLaneState below (one thread, the
//              positions a 64-bit mask, the result two 64-bit masks and one flag: the lane form of the kernels and the harness), the
//              wave form of unigram_kernels.hip (64 candidate ends per step, one per lane), the wide host state of the harness.
//   bounds     every (start, end) pair of positions within the reach is looked up at most once per pass; every loop runs by its own
//              counter: at most N starts, at most N ends per start, at most N steps back.
#ifndef LATOK_UNIGRAM_H
#define LATOK_UNIGRAM_H
#include <stdint.h>

#include "wordpiece.h"

constexpr int kUniMaxBytes = 4096;             // max_bytes at most
constexpr int kUniLaneBytes = 64;              // a token of at most this many bytes keeps its positions in one 64-bit mask
constexpr int kUniLaneNodes = kUniLaneBytes + 2;   // nodes 0 .. L + 1 of such a token at most
constexpr int kUniMaxMarker = 4;               // bytes of the marker at most
constexpr uint32_t kUniAbsent = 0xFFFFFFFFu;   // the position of bytes that are no word (n_words < 2^31)
constexpr uint32_t kUniUnset = 0xFFFFFFFFu;    // back[] of a node that no candidate has reached
constexpr uint32_t kUniUnkBit = 0x80000000u;   // back[]: the piece that ends here is unknown
constexpr uint32_t kUniStartMask = 0x1FFFu;    // back[]: the start node (at most kUniMaxBytes + 1)

// the position in the list of the word that nodes [i, j), j > i, of the token at byte `a` spell, or kUniAbsent
template <class TextLoad, class TableP, class TableM>
TH_FN uint32_t uni_look(TextLoad ld, int64_t a, int mk, int i, int j, const TableP& plain, const TableM& marked, int32_t marker_pos, uint32_t seed) {
    int32_t pos = 0;
    if (mk && i == 0) {
        if (j == 1) return marker_pos < 0 ? kUniAbsent : (uint32_t)marker_pos;
        if ((uint32_t)(j - 1) > marked.max_len) return kUniAbsent;
        return wp_find(ld, a, a + (j - 1), marked, seed, &pos) ? (uint32_t)pos : kUniAbsent;
    }
    if ((uint32_t)(j - i) > plain.max_len) return kUniAbsent;
    return wp_find(ld, a + (i - mk), a + (j - mk), plain, seed, &pos) ? (uint32_t)pos : kUniAbsent;
}

// The forward pass over the nodes 0 .. N of a token, N >= 1.  reach0 / reach: the most nodes a word that starts at node 0 / at a later
// node spans.  The state S:
//   begin(N)             best[0] = 0.0f; back[v] = kUniUnset for every node v
//   next_pos(i, N)       the first position behind node i; N if there is none in front of it
//   words(i, j1, hi, N)  for every position j in [j1, hi] whose nodes [i, j) are a word w: the update of j with best[i] + score(w) and
//                        back = i.  Returns whether [i, j1), the single character at i, is a word
//   unknown(i, j1)       the update of j1 with best[i] + unk_score and back = i | kUniUnkBit
// where the update of j with (cand, b) is: back[j] == kUniUnset or cand > best[j]: best[j] = cand, back[j] = b.
template <class S>
TH_FN void uni_forward(int N, int reach0, int reach, S& s) {
    s.begin(N);
    int i = 0;
    for (int step = 0; step < N && i < N; ++step) {   // the positions in ascending order: i was set by an earlier start (or is 0)
        const int j1 = s.next_pos(i, N);
        const int r = i == 0 ? reach0 : reach;
        const int hi = N - i > r ? i + r : N;
        if (!s.words(i, j1, hi, N)) s.unknown(i, j1);
        i = j1;
    }
}

// The walk back from node N.  The state S:
//   back_of(p)                       back[p]
//   part(i, p, unk, joins, end)      nodes [i, p) are a piece of the best path, unknown if unk; joins: with fuse, it and its right
//                                    neighbour (which starts at p) are unknown and become one piece, which ends at `end`
// Pieces are reported from the last to the first.  Returns the number of pieces of the token, >= 1.
template <class S>
TH_FN int uni_backtrack(int N, int fuse, S& s) {
    int pieces = 0, p = N, end = N;
    bool right_unk = false;
    for (int step = 0; step < N && p > 0; ++step) {
        const uint32_t b = s.back_of(p);
        int i = (int)(b & kUniStartMask);
        if (i >= p) i = p - 1;   // (cannot be: every position of the path was set from a lower one)
        const bool unk = (b & kUniUnkBit) != 0u;
        const bool joins = fuse && unk && right_unk;
        if (!joins) {
            ++pieces;
            end = p;
        }
        s.part(i, p, unk, joins, end);
        right_unk = unk;
        p = i;
    }
    return pieces;
}

// the lowest set bit of m at or above bit x (x in 0 .. 64), 64 if there is none
TH_FN int uni_mask_from(uint64_t m, int x) {
    const uint64_t at = x >= 64 ? 0ull : m & (~0ull << x);
    return at ? (int)__builtin_ctzll(at) : 64;
}
TH_FN uint64_t uni_mask_all(int L) { return L >= 64 ? ~0ull : (1ull << L) - 1ull; }

// bit x of the result: text offset x of the token [a, a + L), L <= 64, is no continuation byte (one pass over the token's dwords)
template <class TextLoad>
TH_FN uint64_t uni_char_starts(TextLoad ld, int64_t a, int L) {
    uint64_t m = 0;
    const int64_t e = a + L, q0 = a >> 2, q1 = (e - 1) >> 2;
    for (int64_t q = q0; q <= q1; ++q) {
        const uint32_t w = ld(q);
        for (int k = 0; k < 4; ++k) {
            const int64_t at = 4 * q + k;
            if (at >= a && at < e && !wp_is_cont((w >> (8 * k)) & 0xFFu)) m |= 1ull << (at - a);
        }
    }
    return m;
}

// The state of a token of at most kUniLaneBytes bytes walked by one thread.  best / back live where `Cols` puts them (best(v) /
// set_best(v, x) / back(v) / set_back(v, b), v < kUniLaneNodes: two LDS columns on the device, arrays in the harness); look(i, j) = the
// word of nodes [i, j); score(w) = the score of word w.  The result of the backtrack: bit x of `starts` = a piece starts at text offset x,
// bit x of `unks` = that piece is unknown; head_unk = the piece that starts at node 0 of a MARKED token (which has no text offset) is unknown.
template <class Cols, class Look, class Score>
struct UniLaneState {
    Cols c;
    Look look;
    Score score;
    uint64_t pos;      // bit x: text offset x is a position
    int mk;
    float unk_score;
    uint64_t starts, unks;
    int head_unk;
    TH_FN void begin(int N) {
        for (int v = 0; v <= N; ++v) c.set_back(v, kUniUnset);
        c.set_best(0, 0.0f);
        c.set_back(0, 0u);
        starts = unks = 0ull;
        head_unk = 0;
    }
    TH_FN int next_pos(int i, int N) const {
        const int n = uni_mask_from(pos, i - mk + 1) + mk;
        return n < N ? n : N;
    }
    TH_FN void update(int j, float cand, uint32_t b) const {
        if (c.back(j) == kUniUnset || cand > c.best(j)) {
            c.set_best(j, cand);
            c.set_back(j, b);
        }
    }
    TH_FN bool words(int i, int j1, int hi, int N) const {
        const float from = c.best(i);
        bool single = false;
        int j = j1;
        for (int k = 0; k < kUniLaneNodes && j <= hi; ++k) {
            const uint32_t w = look(i, j);
            if (w != kUniAbsent) {
                update(j, from + score(w), (uint32_t)i);
                single = single || j == j1;
            }
            if (j >= N) break;
            j = next_pos(j, N);
        }
        return single;
    }
    TH_FN void unknown(int i, int j1) const { update(j1, c.best(i) + unk_score, (uint32_t)i | kUniUnkBit); }
    TH_FN uint32_t back_of(int p) const { return c.back(p); }
    TH_FN void part(int i, int p, bool unk, bool joins, int) {
        if (joins) {   // the right neighbour is no piece of its own any more
            starts &= ~(1ull << (p - mk));
            unks &= ~(1ull << (p - mk));
        }
        if (mk && i == 0) {
            head_unk = unk ? 1 : 0;
        } else {
            starts |= 1ull << (i - mk);
            if (unk) unks |= 1ull << (i - mk);
        }
    }
};
template <class Cols, class Look, class Score>
TH_FN UniLaneState<Cols, Look, Score> uni_lane_state(Cols c, Look look, Score score, uint64_t pos, int mk, float unk_score) {
    return UniLaneState<Cols, Look, Score>{c, look, score, pos, mk, unk_score, 0ull, 0ull, 0};
}

// The pieces that the masks of a lane-form token stand for, in order: out(ord, unk, i, j) for the piece of nodes [i, j).  Returns their number.
template <class Out>
TH_FN int uni_lane_parts(uint64_t starts, uint64_t unks, int head_unk, int L, int mk, Out out) {
    uint64_t m = starts & uni_mask_all(L);
    if (!mk) m |= 1ull;
    int ord = 0;
    if (mk) {
        const int q = m ? (int)__builtin_ctzll(m) : L;
        out(ord++, head_unk != 0, 0, q + 1);
    }
    while (m) {
        const int i = (int)__builtin_ctzll(m);
        m &= m - 1ull;
        const int p = m ? (int)__builtin_ctzll(m) : L;
        out(ord++, ((unks >> i) & 1ull) != 0ull, i + mk, p + mk);
    }
    return ord;
}

// the string-relative byte range of the piece of nodes [i, j) of a token that starts at string-relative byte rel
TH_FN int64_t uni_span_start(int64_t rel, int mk, int i) { return rel + (i > mk ? i - mk : 0); }
TH_FN int64_t uni_span_end(int64_t rel, int mk, int j) { return rel + (j - mk); }

// ---- the build: host only ---------------------------------------------------------------------------------------------------
struct UniTables {
    VtTable plain, marked;            // id slot = the word's position in the list
    std::vector<int32_t> pos_id;      // at least one entry each, so that the address is never NULL
    std::vector<float> pos_score;
    uint32_t max_len_plain = 0, max_len_marked = 0;   // bytes of the longest word of either table
    int32_t marker_pos = -1;          // the word that is the marker alone
};
// true: the marker is empty or exactly one character
inline bool uni_marker_ok(const uint8_t* marker, int marker_len) {
    if (marker_len < 0 || marker_len > kUniMaxMarker) return false;
    for (int b = 1; b < marker_len; ++b)
        if (!wp_is_cont(marker[b])) return false;
    return true;
}
// words / word_off / ids as vt_build takes them; marker_len in 0 .. kUniMaxMarker.  The caller has checked the offsets, the sizes, the scores.
inline void uni_build(const uint8_t* words, const int64_t* word_off, int64_t n_words, const float* scores, const int32_t* ids, const uint8_t* marker,
                      int marker_len, uint32_t seed, UniTables* t) {
    std::vector<int32_t> all((size_t)(n_words > 0 ? n_words : 1), 0);
    for (int64_t i = 0; i < n_words; ++i) all[(size_t)i] = (int32_t)i;
    vt_build(words, word_off, n_words, all.data(), seed, &t->plain);
    t->pos_id.assign((size_t)(n_words > 0 ? n_words : 1), 0);
    t->pos_score.assign((size_t)(n_words > 0 ? n_words : 1), 0.0f);
    t->max_len_plain = t->max_len_marked = 0;
    t->marker_pos = -1;
    std::vector<uint8_t> mw;
    std::vector<int64_t> moff(1, 0);
    std::vector<int32_t> mpos;
    for (int64_t i = 0; i < n_words; ++i) {
        t->pos_id[(size_t)i] = ids ? ids[i] : (int32_t)i;
        t->pos_score[(size_t)i] = scores[i];
        const int64_t w0 = word_off[i], len = word_off[i + 1] - w0;
        if ((uint64_t)len > t->max_len_plain) t->max_len_plain = (uint32_t)len;
        if (marker_len == 0 || len < marker_len) continue;
        bool has = true;
        for (int b = 0; b < marker_len && has; ++b) has = words[w0 + b] == marker[b];
        if (!has) continue;
        if (len == marker_len) {
            if (t->marker_pos < 0) t->marker_pos = (int32_t)i;   // (of duplicates the first wins)
            continue;
        }
        mw.insert(mw.end(), words + w0 + marker_len, words + w0 + len);
        moff.push_back((int64_t)mw.size());
        mpos.push_back((int32_t)i);
        if ((uint64_t)(len - marker_len) > t->max_len_marked) t->max_len_marked = (uint32_t)(len - marker_len);
    }
    mw.push_back(0);     // (never read: non-NULL pointers for an empty table)
    mpos.push_back(0);
    vt_build(mw.data(), moff.data(), (int64_t)moff.size() - 1, mpos.data(), seed, &t->marked);
}

#endif
