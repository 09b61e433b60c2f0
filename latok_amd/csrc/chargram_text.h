// chargram_text.h -- the character n-grams of one token (scikit-learn's analyzer="char_wb"), whose bytes lie nowhere in memory: runs
// of neighbouring characters of the PADDED word pad, c_0 .. c_(L-1), pad (chargram_kernels.hip: k_cgram_count sizes, k_cgram_keys
// hashes and looks up every gram of a batch).  Plain C++17 on top of ngram_text.h: it compiles on the host
// (tests/helpers/chargram_harness.cpp runs it against a plain-Python restatement of the definition) and, under hipcc, on the device.
//
//   character     a character of the token [a, e) starts at a and at every later byte b with (b & 0xC0) != 0x80; its bytes run to the
//                 next start or to e.  For valid UTF-8 these are the code points; for malformed bytes the rule is still total (a
//                 leading run of continuation bytes belongs to the first character).  cg_count_chars counts the starts over the
//                 token's ALIGNED dwords -- a mask of the non-continuation bytes per dword and a popcount, no per-byte loop.
//   positions     the padded word has W = L + 2 positions: 0 and W - 1 are the one-byte pad, 1 .. L the characters.
//   the grams     for n = min_n .. max_n: if n < W the W - n + 1 runs of n neighbouring positions; the first order n >= W of the range
//                 gives the whole padded word ONCE and no higher order contributes ("count a short word only once").
//                 cg_gram_count is G(W), cg_order_grams the share of one order.
//   the slots     gram (n, i) -- order n, start position i -- lies at (the sum of cg_order_grams over the orders [min_n, n)) + i of the
//                 token's G(W) slots: order by order, a bijection onto [0, G(W)).  The short word's gram takes the one slot its order
//                 max(min_n, W) has.  cg_walk keeps no table of offsets: behind every order c it emits, its slot grows by W - c + 1.
//   cg_walk       every gram of the token, once: from every start position i one forward walk that feeds at most max_n positions
//                 through the streaming MurmurHash3 of ngram_text.h -- ng_hash_byte(pad) for a pad position, ng_hash_token over a
//                 character's bytes -- with a finish behind every position (ng_hash_finish leaves the state usable): one walk yields
//                 every order that starts at i.  The real characters of a gram are one contiguous byte range [gs, ge) of the token,
//                 with the pad in front (i == 0) and / or behind (the gram ends at W - 1).
//   cg_equal      such a gram against the word at dword `off` of a vocabulary blob (vocab_table.h): the `equal` of tk_vocab_probe,
//                 the same stream with a comparing sink, as ng_equal.
//
// The loader rules of token_hash.h hold unchanged: the text is read as ALIGNED dwords through `ld(i)`, no index beyond the dword of the
// token's last byte and none below the dword of its first; what lies outside [a, e) in those dwords never reaches a hash or a count.
// Every loop runs by its own counter: the dwords of a token, the bytes of a character up to e, the positions, the orders.  One caller
// walks a long token alone; there is no whole-wave form.
#ifndef LATOK_CHARGRAM_TEXT_H
#define LATOK_CHARGRAM_TEXT_H
#include <stdint.h>

#include "ngram_text.h"

TH_FN bool cg_is_start(uint32_t b) { return (b & 0xC0u) != 0x80u; }
// bit 8k set: byte k of the dword is no continuation byte
TH_FN uint32_t cg_start_mask(uint32_t w) { return ~((w >> 7) & ~(w >> 6)) & 0x01010101u; }
TH_FN int cg_popcount(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popc(x);
#else
    return __builtin_popcount(x);
#endif
}
template <class Load>
TH_FN uint32_t cg_byte(Load ld, int64_t p) {
    return (ld(p >> 2) >> (8 * (uint32_t)(p & 3))) & 0xFFu;
}

// L: the characters of the token [a, e), e > a (0 for an empty range)
template <class Load>
TH_FN int64_t cg_count_chars(Load ld, int64_t a, int64_t e) {
    if (e <= a) return 0;
    const int64_t qa = a >> 2, ql = (e - 1) >> 2;
    int64_t n = 0;
    uint32_t first = 0;
    for (int64_t q = qa; q <= ql; ++q) {
        const uint32_t w = ld(q);
        uint32_t keep = 0x01010101u;
        if (q == qa) {
            keep <<= 8 * (uint32_t)(a & 3);
            first = (w >> (8 * (uint32_t)(a & 3))) & 0xFFu;
        }
        if (q == ql) keep &= 0x01010101u >> (8 * (3u - (uint32_t)((e - 1) & 3)));
        n += cg_popcount(cg_start_mask(w) & keep);
    }
    return n + (cg_is_start(first) ? 0 : 1);   // (the token's first byte starts a character whatever it is)
}
// the end of the character that begins at byte p of a token that ends at e
template <class Load>
TH_FN int64_t cg_char_end(Load ld, int64_t p, int64_t e) {
    int64_t q = p + 1;
    while (q < e && !cg_is_start(cg_byte(ld, q))) ++q;
    return q < e ? q : e;
}

// the grams of order n of a padded word of W positions, min_n the lowest order of the call
TH_FN int64_t cg_order_grams(int n, int64_t W, int min_n) {
    if (n < W) return W - n + 1;
    return n == (W > min_n ? W : (int64_t)min_n) ? 1 : 0;   // the whole word, for the first order that holds it
}
TH_FN int64_t cg_gram_count(int64_t W, int min_n, int max_n) {
    int64_t g = 0;
    for (int n = min_n; n <= max_n; ++n) g += cg_order_grams(n, W, min_n);
    return g;
}

// One gram as cg_walk reports it: its slot among the token's G(W), the hash and the length of its bytes, the byte range of its real
// characters and whether the pad stands in front of and behind them.
struct CgGram {
    int64_t slot;
    uint32_t hash, len;
    int64_t gs, ge;
    bool front, back;
};
// every gram of the token [a, e) of L = W - 2 >= 1 characters, once: emit(CgGram)
template <class Load, class Emit>
TH_FN void cg_walk(Load ld, int64_t a, int64_t e, int64_t W, int min_n, int max_n, uint32_t pad, uint32_t seed, Emit emit) {
    int64_t p = a;                                  // where position max(i, 1) begins
    for (int64_t i = 0; i < W; ++i) {
        NgHash st = ng_hash_init(seed);
        const int64_t left = W - i;
        const int n_walk = left < max_n ? (int)left : max_n;
        int64_t at = i;                             // the slot of gram (c, i): the orders before c add their W - m + 1 each
        int64_t q = p, first_end = p;
        bool back = false;
        for (int c = 1; c <= n_walk; ++c) {
            const int64_t pos = i + c - 1;          // the position fed now
            if (pos == 0 || pos == W - 1) {
                ng_hash_byte(st, pad);
                back = pos != 0;
            } else {
                const int64_t ce = cg_char_end(ld, q, e);
                ng_hash_token(st, ld, q, ce);
                if (c == 1) first_end = ce;
                q = ce;
            }
            const bool whole = c == W;              // (only from i == 0: the short word's one gram)
            if (c < min_n && !whole) continue;
            emit(CgGram{whole && c < min_n ? 0 : at, ng_hash_finish(st), st.s.len, p, q, i == 0, back});
            at += W - c + 1;
        }
        if (i > 0) p = first_end;                   // (position 1 begins where position 0's walk began: at a)
    }
}

template <class Load, class BlobLoad>
TH_FN bool cg_equal(Load ld, int64_t gs, int64_t ge, bool front, bool back, uint32_t pad, BlobLoad blob, uint32_t off, uint32_t word_len) {
    const uint32_t len = (ge > gs ? (uint32_t)(ge - gs) : 0u) + (front ? 1u : 0u) + (back ? 1u : 0u);
    if (len != word_len) return false;   // (the blob is read as far as the word goes, whoever asks)
    NgStream s;
    uint64_t at = off;
    bool differs = false;
    auto cmp = [&at, &differs, blob](uint32_t k) {
        differs |= k != blob(at);
        ++at;
    };
    if (front) ng_put_byte(s, pad, cmp);
    ng_put_token(s, ld, gs, ge, cmp);
    if (back) ng_put_byte(s, pad, cmp);
    if (!differs && s.nc) differs = ((s.carry ^ blob(at)) & vt_tail_mask(s.nc)) != 0u;
    return !differs;
}

#endif
