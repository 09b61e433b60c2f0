// wordpiece.h -- the WordPiece cut of one token (wordpiece_kernels.hip: k_wp_count, k_wp_emit): greedy longest-match-first into
// vocabulary pieces, the continuation pieces looked up in a table of their own.  Plain C++17, like vocab_table.h and term_key.h: the
// build runs on the host only; wp_walk compiles on the host (tests/helpers/wordpiece_harness.cpp runs it against a plain-Python
// restatement of the definition) and, under hipcc, on the device.
//
//   tables     two vocab_table.h tables built by vt_build, unchanged.  INITIAL: every word.  CONTINUATION: every word that starts
//              with the prefix P and is longer than P, stored WITHOUT P, with the word's id.  A piece at a token's start is looked up
//              in the first, any later piece in the second: the lookups of one dictionary that gets `piece` at the start and
//              `P + piece` elsewhere, with no concatenation hashed.  Of duplicate words the first wins in both (the order is kept).
//              Each table records the byte length of its longest word.
//   chars      a CHAR START is the token's first byte and any later byte b with (b & 0xC0) != 0x80.  chars(token) = their number.
//   the cut    chars(token) > max_chars: ONE piece (unk, a, e).  Else start = a; while start < e: among the ends p in (start, e]
//              with p == e or p a char start, the LARGEST p such that bytes[start:p] is a word of the table; none: the WHOLE token is
//              one piece (unk, a, e) and what was found so far is withdrawn; else piece (id, start, p), start = p.
//   bounds     every loop runs by its own counter: at most max_chars ends per piece, at most max_chars pieces, and the walk back
//              to a char start at most as many bytes as the table's longest word.  The first candidate end is
//              min(e, start + max_len) moved back to a char start, so a long unknown token does not hash its whole length per end.
//   the text   is read as th_hash_lane reads it: aligned dwords through a loader, never a dword in front of the one that holds byte
//              a or behind the one that holds byte e - 1.
//   emit       emit(k, id, start, end) is called for piece k = 0, 1, .. as it is found.  A LATER call with k = 0 withdraws
//              every piece reported before it (the miss after hits): a consumer keeps piece 0 back until wp_walk returns, and
//              stores a piece k >= 1 only if k is below the count a counting walk of the same token returned.  wp_walk returns the
//              number of pieces of the token, >= 1.
#ifndef LATOK_WORDPIECE_H
#define LATOK_WORDPIECE_H
#include <stdint.h>

#include "vocab_table.h"

constexpr int kWpMaxPrefix = 8;       // bytes of the continuation prefix at most
constexpr int kWpMaxChars = 1024;     // max_chars at most

// one table as wp_walk reads it: slot(i) = VtSlot i, blob(i) = dword i of the words
template <class SlotLoad, class BlobLoad>
struct WpTableView {
    SlotLoad slot;
    BlobLoad blob;
    uint64_t n_slots;    // a power of two
    uint32_t max_len;    // bytes of the longest word; 0: the table is empty
};
template <class SlotLoad, class BlobLoad>
TH_FN WpTableView<SlotLoad, BlobLoad> wp_table_view(SlotLoad slot, BlobLoad blob, uint64_t n_slots, uint32_t max_len) {
    return WpTableView<SlotLoad, BlobLoad>{slot, blob, n_slots, max_len};
}

// byte i of the text
template <class TextLoad>
TH_FN uint32_t wp_byte(TextLoad ld, int64_t i) {
    return (ld(i >> 2) >> (8u * (uint32_t)(i & 3))) & 0xFFu;
}
TH_FN bool wp_is_cont(uint32_t b) { return (b & 0xC0u) == 0x80u; }

// chars(token), token = bytes [a, e), e > a: one pass over the token's dwords
template <class TextLoad>
TH_FN int64_t wp_chars(TextLoad ld, int64_t a, int64_t e) {
    const int64_t q0 = a >> 2, q1 = (e - 1) >> 2;
    int64_t n = 0;
    for (int64_t q = q0; q <= q1; ++q) {
        const uint32_t w = ld(q);
        uint32_t cont = (w & 0x80808080u) & ~((w << 1) & 0x80808080u);   // bit 7 of every continuation byte
        uint32_t valid = 0x80808080u;
        if (q == q0) valid &= 0xFFFFFFFFu << (8u * (uint32_t)(a & 3));
        if (q == q1 && (e & 3)) valid &= (1u << (8u * (uint32_t)(e & 3))) - 1u;
        cont = ~cont & valid;
        for (; cont; cont &= cont - 1u) ++n;
    }
    return n + (wp_is_cont(wp_byte(ld, a)) ? 1 : 0);   // the first byte starts a char whatever it is
}

// the largest end p in (start, hi], p == e or a char start, no further back than `span` bytes; start: there is none
template <class TextLoad>
TH_FN int64_t wp_end_at_or_before(TextLoad ld, int64_t start, int64_t hi, int64_t e, uint32_t span) {
    int64_t p = hi;
    for (uint32_t i = 0; i < span && p > start; ++i) {
        if (p == e || !wp_is_cont(wp_byte(ld, p))) return p;
        --p;
    }
    return start;
}

// the id of bytes [s, p) in one table, or found = false
template <class TextLoad, class Table>
TH_FN bool wp_find(TextLoad ld, int64_t s, int64_t p, const Table& t, uint32_t seed, int32_t* id) {
    const uint32_t h = th_hash_lane(ld, s, p, seed);
    bool found = false;
    auto blob = t.blob;
    // (vt_probe returns the id: the hit itself is reported through `found`, so that every int32 stays a legal id)
    const int32_t v = vt_probe(t.slot, t.n_slots, h, (uint32_t)(p - s),
                               [ld, s, p, blob, &found](uint32_t off) { return found = vt_equal_lane(ld, s, p, blob, off); }, 0);
    *id = v;
    return found;
}

// The cut of the token [a, e), e > a.  See the head of the file for emit's contract.  Returns the number of pieces.
template <class TextLoad, class Table0, class Table1, class Emit>
TH_FN int wp_walk(TextLoad ld, int64_t a, int64_t e, const Table0& initial, const Table1& cont, uint32_t seed, int max_chars, int32_t unk,
                  Emit emit) {
    if (wp_chars(ld, a, e) > (int64_t)max_chars) {
        emit(0, unk, a, e);
        return 1;
    }
    int64_t start = a;
    int n = 0;
    while (start < e && n < max_chars) {   // (a piece holds a char at least: more pieces than chars cannot be)
        const uint32_t max_len = start == a ? initial.max_len : cont.max_len;
        const int64_t hi = e - start > (int64_t)max_len ? start + (int64_t)max_len : e;
        int64_t p = wp_end_at_or_before(ld, start, hi, e, max_len);
        int32_t id = 0;
        bool hit = false;
        for (int tries = 0; tries < max_chars && p > start; ++tries) {
            hit = start == a ? wp_find(ld, start, p, initial, seed, &id) : wp_find(ld, start, p, cont, seed, &id);
            if (hit) break;
            p = wp_end_at_or_before(ld, start, p - 1, e, max_len);
        }
        if (!hit) break;
        emit(n, id, start, p);
        ++n;
        start = p;
    }
    if (start < e) {   // a miss: the whole token is unknown
        emit(0, unk, a, e);
        return 1;
    }
    return n;
}

// ---- the build: host only ---------------------------------------------------------------------------------------------------
struct WpTables {
    VtTable initial, cont;
    uint32_t max_len0 = 0, max_len1 = 0;   // bytes of the longest word of either table
    int64_t n_cont = 0;                    // words that went to the continuation table's build
};
// words / word_off / ids as vt_build takes them; prefix_len in 0 .. kWpMaxPrefix.  The caller has checked the offsets and the sizes.
inline void wp_build(const uint8_t* words, const int64_t* word_off, int64_t n_words, const int32_t* ids, const uint8_t* prefix, int prefix_len,
                     uint32_t seed, WpTables* t) {
    vt_build(words, word_off, n_words, ids, seed, &t->initial);
    std::vector<uint8_t> cw;
    std::vector<int64_t> coff(1, 0);
    std::vector<int32_t> cid;
    t->max_len0 = t->max_len1 = 0;
    for (int64_t i = 0; i < n_words; ++i) {
        const int64_t w0 = word_off[i], len = word_off[i + 1] - w0;
        if ((uint64_t)len > t->max_len0) t->max_len0 = (uint32_t)len;
        if (len <= prefix_len) continue;
        bool has = true;
        for (int b = 0; b < prefix_len && has; ++b) has = words[w0 + b] == prefix[b];
        if (!has) continue;
        cw.insert(cw.end(), words + w0 + prefix_len, words + w0 + len);
        coff.push_back((int64_t)cw.size());
        cid.push_back(ids ? ids[i] : (int32_t)i);
        if ((uint64_t)(len - prefix_len) > t->max_len1) t->max_len1 = (uint32_t)(len - prefix_len);
    }
    t->n_cont = (int64_t)cid.size();
    vt_build(cw.data(), coff.data(), t->n_cont, cid.data(), seed, &t->cont);
}

#endif
