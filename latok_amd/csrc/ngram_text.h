// ngram_text.h -- the bytes of a word n-gram, which lie nowhere in memory: the tokens t_i .. t_(i+n-1) of one string with a one-byte
// separator between neighbours (ngram_kernels.hip: k_ngram_keys hashes and looks up every gram of a batch).  Plain C++17, like
// token_hash.h: it compiles on the host (tests/helpers/ngram_harness.cpp runs it against an independent MurmurHash3 over
// sep.join(tokens) and against a byte compare) and, under hipcc, on the device.
//
//   NgStream      the bytes fed so far that do not fill a 4-byte block yet: up to 3 carried bytes (low byte first), their count,
//                 and the length so far.  ng_put_token feeds the bytes [a, e) of the text, ng_put_byte one byte; every whole block
//                 (little endian, in order) goes to a sink.  A token that arrives behind c carried bytes is cut into blocks at
//                 4 - c, 8 - c, ..: each aligned pair (ld(i), ld(i + 1)) gives one token dword through th_align, and a block is
//                 the carry below the dword's low bytes -- every carry count 0..3 against every start alignment 0..3.
//   NgHash        MurmurHash3 x86_32 (token_hash.h) over such a stream: the sink is the h chain.  ng_hash_finish returns the hash of
//                 everything fed so far -- the carried bytes are the tail, the length enters as 32 bits -- and leaves the state as
//                 it was: one walk over t_i, sep, t_(i+1), sep, .. with a finish behind every token yields the hash of every order.
//   ng_equal      the gram of n span records against the word at dword `off` of a vocabulary blob (vocab_table.h): the `equal` of
//                 tk_vocab_probe.  It is asked only where hash and length agree, so it may walk the gram again; its loops run over
//                 the gram's own tokens and bytes, and it reads ceil(length / 4) dwords of the blob, which are the word's: a word
//                 of another length (`word_len` = the slot's) is unequal before the blob is read.
//
// The loader rules of token_hash.h hold unchanged: the text is read as ALIGNED dwords through `ld(i)`, the index is clamped to the
// dword that holds the token's last byte, so nothing is read behind the aligned dword that holds the last byte of the batch; what
// the clamp repeats and what lies in front of a token's first byte is shifted out, what lies behind its last byte is masked off.
#ifndef LATOK_NGRAM_TEXT_H
#define LATOK_NGRAM_TEXT_H
#include <stdint.h>

#include "token_hash.h"
#include "vocab_table.h"

constexpr int kNgMax = 8;   // the highest order of a gram

struct NgStream {
    uint32_t carry = 0;   // the pending bytes, low byte first; the bytes above them are zero
    uint32_t nc = 0;      // how many: 0..3
    uint32_t len = 0;     // bytes fed so far (32 bits, as the length enters the hash)
};

template <class Sink>
TH_FN void ng_put_byte(NgStream& s, uint32_t b, Sink blk) {
    s.carry |= (b & 0xFFu) << (8 * s.nc);
    ++s.len;
    if (++s.nc == 4) {
        blk(s.carry);
        s.carry = 0;
        s.nc = 0;
    }
}

// bytes [a, e) of the text.  One aligned load per token dword: the upper dword of a pair is the lower of the next.
template <class Load, class Sink>
TH_FN void ng_put_token(NgStream& s, Load ld, int64_t a, int64_t e, Sink blk) {
    if (e <= a) return;
    const int64_t q = a >> 2, last = (e - 1) >> 2;            // dwords of the first and of the last byte
    const uint32_t sh = (uint32_t)(a & 3), r = (uint32_t)((e - a) & 3);
    const int64_t nd = ((e - a) + 3) >> 2;                    // token dwords, the partial one included
    const uint32_t up = 8 * s.nc, down = 32 - up;             // (whole dwords leave the carry count as it is)
    uint32_t lo = ld(q);
    for (int64_t i = 0; i < nd; ++i) {
        const int64_t qi = q + i + 1;
        const uint32_t hi = ld(qi < last ? qi : last);        // (clamped: only read where a byte of the token lies in it)
        uint32_t w = th_align(hi, lo, sh);
        lo = hi;
        if (i + 1 < nd || r == 0) {
            blk(s.carry | (w << up));                         // (up == 0: the carry is empty)
            s.carry = up ? w >> down : 0u;
        } else {                                              // the last r = 1..3 bytes
            w &= (1u << (8 * r)) - 1u;
            if (s.nc + r >= 4) {                              // (then nc >= 1, up >= 8)
                blk(s.carry | (w << up));
                s.carry = w >> down;
                s.nc = s.nc + r - 4;
            } else {
                s.carry |= w << up;
                s.nc += r;
            }
        }
    }
    s.len += (uint32_t)(e - a);
}

struct NgHash {
    uint32_t h = 0;
    NgStream s;
};
TH_FN NgHash ng_hash_init(uint32_t seed) {
    NgHash st;
    st.h = seed;
    return st;
}
template <class Load>
TH_FN void ng_hash_token(NgHash& st, Load ld, int64_t a, int64_t e) {
    uint32_t h = st.h;
    ng_put_token(st.s, ld, a, e, [&h](uint32_t k) { h = th_mix_h(h, th_mix_k(k)); });
    st.h = h;
}
TH_FN void ng_hash_byte(NgHash& st, uint32_t b) {
    uint32_t h = st.h;
    ng_put_byte(st.s, b, [&h](uint32_t k) { h = th_mix_h(h, th_mix_k(k)); });
    st.h = h;
}
// the hash of everything fed so far; the state stays usable
TH_FN uint32_t ng_hash_finish(const NgHash& st) {
    return th_finish(st.s.nc ? th_tail(st.h, st.s.carry, (int)st.s.nc) : st.h, st.s.len);
}

// span(k) = the absolute byte range of token k of the gram, k = 0 .. n - 1, as an NgSpan
struct NgSpan {
    int64_t a, e;
};
template <class Load, class Span, class BlobLoad>
TH_FN bool ng_equal(Load ld, Span span, int n, uint32_t sep, BlobLoad blob, uint32_t off, uint32_t word_len) {
    uint32_t len = n > 0 ? (uint32_t)(n - 1) : 0u;
    for (int k = 0; k < n; ++k) {
        const NgSpan t = span(k);
        len += t.e > t.a ? (uint32_t)(t.e - t.a) : 0u;
    }
    if (len != word_len) return false;   // (the blob is read as far as the word goes, whoever asks)
    NgStream s;
    uint64_t at = off;
    bool differs = false;
    auto cmp = [&at, &differs, blob](uint32_t k) {
        differs |= k != blob(at);
        ++at;
    };
    for (int k = 0; k < n && !differs; ++k) {
        if (k > 0) ng_put_byte(s, sep, cmp);
        const NgSpan t = span(k);
        ng_put_token(s, ld, t.a, t.e, cmp);
    }
    if (!differs && s.nc) differs = ((s.carry ^ blob(at)) & vt_tail_mask(s.nc)) != 0u;
    return !differs;
}

#endif
