// spbpe.h -- SentencePiece BPE of one segment (spbpe_kernels.hip: k_spbpe_count, k_spbpe_emit; the front: pretok_kernels.hip,
// k_pretok_spm_planes; the definition in full: include/latok_hip.h behind latok_bpe_create_spm).  Plain C++17, like bpe.h and pretok.h: it
// compiles on the host (tests/helpers/spbpe_harness.cpp runs it against a plain-Python restatement of the definition) and, under hipcc, on
// the device.  bpe_look and bpe_merge are bpe.h's, the table is vt_build's: nothing of them is restated here.
//
//   segments   a character is SPACE-LIKE if its bytes are exactly 20 or exactly E2 96 81.  A segment starts at a string's first byte and
//              at every space-like character whose previous character in the same string is not space-like: a (possibly empty) lead run
//              of space-like characters, then characters that are not.  sp_starts_scalar walks one string; sp_word_starts is the same
//              rule as boolean algebra over the bit planes of a pretok.h window (a start bit depends on 3 bytes behind and 3 ahead: no
//              carry).
//   virtual    the text the lookups read: one E2 96 81 if the object has a dummy prefix and the segment is its string's first, one
//              E2 96 81 per character of the lead run, then the remaining bytes verbatim.  The first P = 3 (dummy + lead characters)
//              bytes are periodic, the rest is an unaligned view of the text: SpVirtual composes dword q of it from the period's three
//              phases and th_align over two aligned dwords of the text, whose indices are clamped to the segment's own dwords.  No
//              byte is copied or staged.
//   parts      the characters of the virtual text (SpLaneState::fill: only character starts are part starts), then bpe_merge,
//              unchanged.  A part that is no word is a single character: one piece per byte with byte ids, else unk.
//   spans      sp_real: virtual position -> real byte.  The dummy maps to the empty range at the segment's start, the j-th lead marker
//              to the j-th lead character, everything else to itself.
#ifndef LATOK_SPBPE_H
#define LATOK_SPBPE_H
#include <stdint.h>

#include "bpe.h"
#include "pretok.h"

constexpr int kPretokSpm = 5;                // (LATOK_PRETOK_SPM of include/latok_hip.h, restated so that this header stands alone)
constexpr int kSpLaneBytes = kBpeLaneBytes;  // a segment of at most this many VIRTUAL bytes keeps its part starts in one 64-bit mask

// ---- the segment rule ----------------------------------------------------------------------------------------------------------------
// start[i] = 1 where a segment of the string s[0 .. n) starts, else 0
inline void sp_starts_scalar(const uint8_t* s, int64_t n, uint8_t* start) {
    auto is_start = [&](int64_t i) { return i == 0 || (s[i] & 0xC0u) != 0x80u; };
    bool prev = false;   // the character in front is space-like
    for (int64_t i = 0; i < n;) {
        int64_t e = i + 1;
        while (e < n && !is_start(e)) ++e;
        const bool sl = (e - i == 1 && s[i] == 0x20u) || (e - i == 3 && s[i] == 0xE2u && s[i + 1] == 0x96u && s[i + 2] == 0x81u);
        for (int64_t j = i; j < e; ++j) start[j] = 0;
        if (i == 0 || (sl && !prev)) start[i] = 1;
        prev = sl;
        i = e;
    }
}

// The start bits of the 64 bytes in the middle of a window (win, B: as pt_word_starts of pretok.h takes them).  The caller clears the
// bits of positions outside the batch.
template <class Window>
PT_FN uint64_t sp_word_starts(const Window& win, pt_u128 B) {
    pt_u128 cont = 0, b20 = 0, bE2 = 0, b96 = 0, b81 = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < kPtWindow / 8; ++j) {
        const uint64_t x = win.qword(j), top = x & kPtTop;
        cont |= (pt_u128)pt_gather8(top & ~(x << 1)) << (8 * j);
        b20 |= (pt_u128)pt_gather8(pt_eq8(x, 0x20u)) << (8 * j);
        bE2 |= (pt_u128)pt_gather8(pt_eq8(x, 0xE2u)) << (8 * j);
        b96 |= (pt_u128)pt_gather8(pt_eq8(x, 0x96u)) << (8 * j);
        b81 |= (pt_u128)pt_gather8(pt_eq8(x, 0x81u)) << (8 * j);
    }
    const pt_u128 kAll = ((pt_u128)0xFFFFFFFFull << 64) | ~0ull;
    B &= kAll;
    const pt_u128 st = (~cont | B) & kAll;                                // character starts
    const pt_u128 one = b20 & st & (st >> 1);                             // the character 20
    const pt_u128 three = bE2 & (b96 >> 1) & (b81 >> 2) & st & ~(st >> 1) & ~(st >> 2) & (st >> 3);   // the character E2 96 81
    const pt_u128 prev = ((one << 1) | (three << 3)) & ~B;                // the character in front is space-like
    return (uint64_t)(((B | ((one | three) & ~prev)) & st) >> kPtHalo);
}

// ---- one segment ---------------------------------------------------------------------------------------------------------------------
struct SpSeg {
    int64_t a = 0, e = 0;        // the segment's real bytes [a, e) of the batch
    int64_t r0 = 0;              // the first byte behind the lead run
    int64_t P = 0;               // the periodic bytes in front of the virtual text: 3 (dummy + lead characters)
    int64_t VL = 0;              // the virtual length in bytes (exact only up to `over`)
    int64_t lead_chars = 0;
    uint64_t lead3 = 0;          // bit j: the j-th lead character has three bytes (the first 64 of them)
    int dummy = 0;
    bool over = false;           // VL > max_bytes: the segment is ONE unknown piece
};
// the segment [a, e), e > a, of a string; dummy = 1: the object has a dummy prefix and a is its string's first byte.  The walk over the
// lead run ends as soon as the virtual length is known to pass max_bytes.
template <class TextLoad>
TH_FN SpSeg sp_segment(TextLoad ld, int64_t a, int64_t e, int dummy, int max_bytes) {
    SpSeg g;
    g.a = a;
    g.e = e;
    g.dummy = dummy;
    int64_t i = a, n = 0;
    while (i < e && 3 * (n + dummy) <= (int64_t)max_bytes) {
        const uint32_t b = wp_byte(ld, i);
        int len = 0;
        if (b == 0x20u) len = 1;
        else if (b == 0xE2u && i + 3 <= e && wp_byte(ld, i + 1) == 0x96u && wp_byte(ld, i + 2) == 0x81u) len = 3;
        if (!len || (i + len < e && wp_is_cont(wp_byte(ld, i + len)))) break;   // (followed by a continuation byte: another character)
        if (len == 3 && n < 64) g.lead3 |= 1ull << n;
        i += len;
        ++n;
    }
    g.lead_chars = n;
    g.r0 = i;
    g.P = 3 * (n + dummy);
    g.VL = g.P + (e - i);
    g.over = g.VL > (int64_t)max_bytes;
    return g;
}
// bytes of the first j lead characters, j <= lead_chars
template <class TextLoad>
TH_FN int64_t sp_lead_off(TextLoad ld, const SpSeg& g, int64_t j) {
    if (g.lead_chars <= 64) return j + 2 * (int64_t)__builtin_popcountll(j >= 64 ? g.lead3 : g.lead3 & ((1ull << j) - 1ull));
    int64_t i = g.a;
    for (int64_t c = 0; c < j && i < g.r0; ++c) i += wp_byte(ld, i) == 0x20u ? 1 : 3;
    return i - g.a;
}
// The real byte of the virtual position v in [0, VL]: where the character that starts at v begins, and where the one that ends at v
// ends.  A piece [i, p) of the virtual text reports [sp_real(i), sp_real(p)).
template <class TextLoad>
TH_FN int64_t sp_real(TextLoad ld, const SpSeg& g, int64_t v) {
    if (v >= g.P) return g.r0 + (v - g.P);
    const int64_t j = v / 3 - g.dummy;
    return g.a + (j > 0 ? sp_lead_off(ld, g, j) : 0);
}

// dword q of the virtual text, q <= (VL - 1) >> 2.  Loads: at most two aligned dwords of the text, both inside the segment's own.
template <class TextLoad>
struct SpVirtual {
    TextLoad ld;
    int64_t r0, P, q_lo, q_hi;   // q_lo / q_hi: the dwords of the segment's first and last byte
    TH_FN uint32_t operator()(int64_t q) const {
        const int64_t v0 = 4 * q;
        uint32_t pre = 0;
        if (v0 < P) {
            const int ph = (int)(q % 3);   // (4 q) mod 3
            pre = ph == 0 ? 0xE28196E2u : ph == 1 ? 0x96E28196u : 0x8196E281u;
            if (v0 + 4 <= P) return pre;
        }
        const int64_t x = r0 + (v0 - P);   // the real byte of the dword's first (>= -3)
        const int64_t k = x >> 2;
        const int64_t k0 = k < q_lo ? q_lo : (k > q_hi ? q_hi : k), k1 = k + 1 < q_lo ? q_lo : (k + 1 > q_hi ? q_hi : k + 1);
        const uint32_t real = th_align(ld(k1), ld(k0), (uint32_t)(x & 3));
        if (v0 >= P) return real;
        const uint32_t m = (1u << (8u * (uint32_t)(P - v0))) - 1u;   // the periodic bytes of this dword: 1 .. 3
        return (pre & m) | (real & ~m);
    }
};
template <class TextLoad>
TH_FN SpVirtual<TextLoad> sp_virtual(TextLoad ld, const SpSeg& g) {
    return SpVirtual<TextLoad>{ld, g.r0, g.P, g.a >> 2, (g.e - 1) >> 2};
}
// is the virtual position v < VL a character start?  (vld: the virtual text's loader.)  The first byte behind the periodic lead is one
// whatever it is: it is its string's first byte, or it follows a whole lead character.
template <class VLoad>
TH_FN bool sp_vstart(VLoad vld, int64_t P, int64_t v) {
    if (v < P) return v % 3 == 0;
    return v == P || !wp_is_cont(wp_byte(vld, v));
}
// the character starts of a virtual text of L <= 64 bytes as a mask
template <class VLoad>
TH_FN uint64_t sp_char_mask(VLoad vld, int64_t P, int L) {
    uint64_t m = 0;
    for (int q = 0; 4 * q < L; ++q) {
        const uint32_t w = vld(q);
        const uint32_t cont = (w & 0x80808080u) & ~((w << 1) & 0x80808080u);   // bit 7 of every continuation byte
        const uint32_t st = ~cont & 0x80808080u;
        m |= (uint64_t)(((st >> 7) & 1u) | ((st >> 14) & 2u) | ((st >> 21) & 4u) | ((st >> 28) & 8u)) << (4 * q);
    }
    return (m | 1ull | (P < 64 ? 1ull << P : 0ull)) & bpe_mask_all(L);
}

// The lane state of bpe.h with another fill: the part starts are the character starts in `chars` (bit 0 set, no bit at or behind L),
// and a rank is kept at part starts only.
template <class Ranks, class Look>
struct SpLaneState : BpeLaneState<Ranks, Look> {
    uint64_t chars;
    TH_FN void fill(int L) {
        this->mask = chars;
        for (uint64_t m = chars; m;) {
            const int i = (int)__builtin_ctzll(m);
            m &= m - 1ull;
            if (!m) {
                this->ranks.set(i, kBpeAbsent);
                break;
            }
            const uint64_t m2 = m & (m - 1ull);
            this->ranks.set(i, this->look(i, m2 ? (int)__builtin_ctzll(m2) : L));
        }
    }
};
template <class Ranks, class Look>
TH_FN SpLaneState<Ranks, Look> sp_lane_state(Ranks ranks, Look look, uint64_t chars) {
    SpLaneState<Ranks, Look> s{{ranks, look, 0ull}, chars};
    return s;
}

// the pieces of a final part of `bytes` virtual bytes whose rank is `rank`: a word is one piece; what is no word is a single character:
// one piece per byte with byte ids, else one unk (the caller fuses)
TH_FN int64_t sp_part_pieces(uint32_t rank, int64_t bytes, bool byte_ids) { return rank != kBpeAbsent || !byte_ids ? 1 : bytes; }

// does the word list break the segment rule?  A word must not hold E2 96 81 directly behind a character that is not E2 96 81: the
// position of the first word that does, or -1
inline int64_t sp_first_bad_word(const uint8_t* words, const int64_t* word_off, int64_t n_words) {
    for (int64_t w = 0; w < n_words; ++w) {
        const uint8_t* s = words + word_off[w];
        const int64_t n = word_off[w + 1] - word_off[w];
        bool prev_marker = true;   // (nothing in front: fine)
        for (int64_t i = 0; i < n;) {
            int64_t e = i + 1;
            while (e < n && (s[e] & 0xC0u) == 0x80u) ++e;
            const bool marker = e - i == 3 && s[i] == 0xE2u && s[i + 1] == 0x96u && s[i + 2] == 0x81u;
            if (marker && !prev_marker) return w;
            prev_marker = marker;
            i = e;
        }
    }
    return -1;
}

#endif
