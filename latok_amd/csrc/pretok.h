// pretok.h -- GPT-2's pre-tokenizer in byte space (latok_pretokens_utf8_bytes_batch, include/latok_hip.h, which states the definition in
// full): the class of one character, the scalar walk over one string and the rule over one 64-byte word.  Plain C++17, like fold_map.h
// and bpe.h: it compiles on the host (tests/helpers/pretok_harness.cpp runs it against a plain-Python restatement of the definition)
// and, under hipcc, on the device, where pretok_kernels.hip calls the very same pt_class_char and pt_word_starts.
//
//   classes    S (White_Space, 25 code points), L (general category L*), N (N*), O (everything else, every malformed character).  Code
//              points below U+0080 and the S set are arithmetic; the others take pretok_tables.inc (tools/gen_pretok_tables.py; the
//              Unicode version is the file's first line and PRETOK_UNICODE_VERSION): stage 1 by cp >> 7 names a block of 128 code
//              points, stage 2 holds eight dwords of sixteen 2-bit classes per block; no code point at or above `limit` (U+31380, behind
//              the last letter of Unicode 13.0.0) is L or N, so the tables end there.  7 719 bytes in all.
//   characters a character starts at a string's first byte and at every byte that is not 10xxxxxx; it carries the class of its code point
//              when its bytes are exactly one well-formed sequence (no overlong form, no surrogate, at most U+10FFFF), else O.
//   the walk   pt_starts_scalar: one string, character by character, the rules as include/latok_hip.h numbers them.
//   the word   pt_word_starts: the same rules as boolean algebra over bit planes of a WINDOW of kPtWindow = 96 bytes, the word's 64 with
//              kPtHalo = 16 bytes on either side, every byte outside the batch read as 0.  A start bit depends on the bytes from 7 behind it
//              (an apostrophe three bytes back whose own left neighbour is a four-byte character) to 6 ahead of it (the character behind
//              a three-byte space), so a word needs nothing from its neighbours but those bytes and the string-start bits over them:
//              there is no carry, every word is computed alone, and what the planes hold within 8 positions of the window's edges is
//              never looked at.  Planes are 128-bit integers of which 96 bits are used.
// The second half of the file is the cl100k / Llama 3 rule (LATOK_PRETOK_CL100K) in the same three forms; that rule does have carries.
#ifndef LATOK_PRETOK_H
#define LATOK_PRETOK_H
#include <stdint.h>

#if defined(__HIPCC__)
#define PT_FN __host__ __device__ __forceinline__
#else
#define PT_FN inline
#endif

constexpr int kPtO = 0, kPtL = 1, kPtN = 2, kPtS = 3;
constexpr int kPtHalo = 16, kPtWord = 64, kPtWindow = kPtWord + 2 * kPtHalo;
constexpr int kPretokLatok = 0, kPretokGpt2 = 1;   // (the public constants of include/latok_hip.h, restated so that this header stands alone)
typedef unsigned __int128 pt_u128;

struct PretokTables {
    const uint8_t* stage1 = nullptr;    // [limit >> 7]
    const uint32_t* stage2 = nullptr;   // [blocks * 8]
    uint32_t limit = 0;                 // PRETOK_TABLE_LIMIT: every code point from here on is O
};

// Unicode White_Space
PT_FN bool pt_is_space(uint32_t c) {
    return (c >= 0x09u && c <= 0x0Du) || c == 0x20u || c == 0x85u || c == 0xA0u || c == 0x1680u || (c >= 0x2000u && c <= 0x200Au) || c == 0x2028u ||
           c == 0x2029u || c == 0x202Fu || c == 0x205Fu || c == 0x3000u;
}
// the class of a scalar value
PT_FN int pt_class_cp(uint32_t c, const PretokTables& T) {
    if (c < 0x80u) {
        if (((c | 0x20u) - 'a') < 26u) return kPtL;
        if (c - '0' < 10u) return kPtN;
        return pt_is_space(c) ? kPtS : kPtO;
    }
    if (pt_is_space(c)) return kPtS;
    if (c >= T.limit) return kPtO;
    const uint32_t d = T.stage2[(uint32_t)T.stage1[c >> 7] * 8u + ((c & 127u) >> 4)];
    return (int)((d >> (2u * (c & 15u))) & 3u);
}
// The class of a character of `len` bytes that begins with b0 (b1 .. b3: its next bytes; what lies behind the character is not looked
// at).  Every byte of a character but its first is 10xxxxxx by the definition of a character, so the length and the value decide.
PT_FN int pt_class_char(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3, int len, const PretokTables& T) {
    if (b0 < 0x80u) return len == 1 ? pt_class_cp(b0, T) : kPtO;
    if (b0 < 0xC2u || b0 > 0xF4u) return kPtO;   // a stray continuation byte, the overlong leads C0 / C1, F5 .. FF
    const int n = b0 < 0xE0u ? 2 : b0 < 0xF0u ? 3 : 4;
    if (len != n) return kPtO;                   // truncated, or followed by more continuation bytes
    uint32_t c;
    if (n == 2) {
        c = ((b0 & 0x1Fu) << 6) | (b1 & 0x3Fu);
    } else if (n == 3) {
        c = ((b0 & 0x0Fu) << 12) | ((b1 & 0x3Fu) << 6) | (b2 & 0x3Fu);
        if (c < 0x800u || (c >= 0xD800u && c <= 0xDFFFu)) return kPtO;
    } else {
        c = ((b0 & 0x07u) << 18) | ((b1 & 0x3Fu) << 12) | ((b2 & 0x3Fu) << 6) | (b3 & 0x3Fu);
        if (c < 0x10000u || c > 0x10FFFFu) return kPtO;
    }
    return pt_class_cp(c, T);
}
// the bytes of a contraction that an apostrophe opens when b1, b2 follow it: 2, 3, or 0 for none
PT_FN int pt_contraction(uint32_t b1, uint32_t b2) {
    if (b1 == 's' || b1 == 't' || b1 == 'm' || b1 == 'd') return 2;
    if ((b1 == 'r' || b1 == 'v') && b2 == 'e') return 3;
    return (b1 == 'l' && b2 == 'l') ? 3 : 0;
}

// ---- the scalar walk ---------------------------------------------------------------------------------------------------------------
// start[i] = 1 where a pre-token of the string s[0 .. n) starts, else 0.  `cls` is scratch of n bytes (the class of every byte).
inline void pt_starts_scalar(const uint8_t* s, int64_t n, const PretokTables& T, uint8_t* cls, uint8_t* start) {
    auto is_start = [&](int64_t i) { return i == 0 || (s[i] & 0xC0u) != 0x80u; };
    for (int64_t i = 0; i < n;) {                  // the class of every character, smeared over its bytes
        int64_t e = i + 1;
        while (e < n && !is_start(e)) ++e;
        const int c = pt_class_char(s[i], e - i > 1 ? s[i + 1] : 0xFFu, e - i > 2 ? s[i + 2] : 0xFFu, e - i > 3 ? s[i + 3] : 0xFFu,
                                    e - i > 4 ? 5 : (int)(e - i), T);
        for (int64_t j = i; j < e; ++j) { cls[j] = (uint8_t)c; start[j] = 0; }
        i = e;
    }
    // rule 1: bit 1 of start[] = inside a contraction, bit 2 = forced
    for (int64_t i = 0; i < n; ++i) {
        if (s[i] != 0x27u || (i + 1 < n && !is_start(i + 1))) continue;
        const bool scan = i == 0 || cls[i - 1] == kPtL || cls[i - 1] == kPtN || (cls[i - 1] == kPtS && s[i - 1] != 0x20u);
        if (!scan) continue;
        const int k = pt_contraction(i + 1 < n ? s[i + 1] : 0u, i + 2 < n ? s[i + 2] : 0u);
        if (k == 0 || i + k > n || (i + k < n && !is_start(i + k))) continue;
        for (int j = 1; j < k; ++j) start[i + j] |= 2u;
        if (i + k < n) start[i + k] |= 4u;
    }
    for (int64_t i = 0; i < n; ++i) {
        const uint8_t f = start[i];
        start[i] = 0;
        if (!is_start(i) || (f & 2u)) continue;
        bool st = i == 0 || (f & 4u);
        if (!st && cls[i] == kPtS) {               // rule 2
            int64_t e = i + 1;
            while (e < n && !is_start(e)) ++e;
            st = cls[i - 1] != kPtS || (e < n && cls[e] != kPtS);
        } else if (!st) {                          // rule 3
            st = cls[i - 1] == kPtS ? s[i - 1] != 0x20u : cls[i - 1] != cls[i];
        }
        start[i] = st ? 1u : 0u;
    }
}

// ---- the word ----------------------------------------------------------------------------------------------------------------------
// eight bytes at once: the top bit of every byte of the result says whether the byte of x ...
constexpr uint64_t kPtOnes = 0x0101010101010101ull, kPtTop = 0x8080808080808080ull, kPtLow7 = 0x7F7F7F7F7F7F7F7Full;
PT_FN uint64_t pt_eq8(uint64_t x, uint32_t c) {          // ... equals c
    const uint64_t y = x ^ (kPtOnes * c);
    return ~(((y & kPtLow7) + kPtLow7) | y) & kPtTop;
}
PT_FN uint64_t pt_ge8(uint64_t x7, uint32_t c) {         // ... is >= c, for bytes x7 < 0x80 and 1 <= c <= 0x80
    return (x7 + kPtOnes * (0x80u - c)) & kPtTop;
}
PT_FN uint32_t pt_gather8(uint64_t top) {               // the eight top bits as one byte, byte 0's in bit 0
    return (uint32_t)(((top >> 7) * 0x0002040810204081ull) >> 49) & 0xFFu;
}

// The start bits of the 64 bytes in the middle of a window.  win.qword(j): bytes 8j .. 8j + 7 of the window, little-endian, j = 0 .. 11;
// win.byte(i): byte i.  B: bit i = byte i of the window is a string's first byte (the batch's end counts as a string start: what lies
// behind it is no string's).  The caller clears the bits of positions outside the batch.
template <class Window>
PT_FN uint64_t pt_word_starts(const Window& win, pt_u128 B, const PretokTables& T) {
    const pt_u128 kAll = ((pt_u128)0xFFFFFFFFull << 64) | ~0ull;
    pt_u128 hi = 0, cont = 0, aS = 0, aL = 0, aN = 0, sp = 0, ap = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < kPtWindow / 8; ++j) {
        const uint64_t x = win.qword(j), top = x & kPtTop, x7 = x & kPtLow7, lower = x7 | (kPtOnes * 0x20u);
        const uint64_t space = pt_eq8(x, 0x20u);
        hi |= (pt_u128)pt_gather8(top) << (8 * j);
        cont |= (pt_u128)pt_gather8(top & ~(x << 1)) << (8 * j);
        aL |= (pt_u128)pt_gather8(pt_ge8(lower, 'a') & ~pt_ge8(lower, 'z' + 1)) << (8 * j);
        aN |= (pt_u128)pt_gather8(pt_ge8(x7, '0') & ~pt_ge8(x7, '9' + 1)) << (8 * j);
        aS |= (pt_u128)pt_gather8((pt_ge8(x7, 0x09u) & ~pt_ge8(x7, 0x0Eu)) | space) << (8 * j);
        sp |= (pt_u128)pt_gather8(space) << (8 * j);
        ap |= (pt_u128)pt_gather8(pt_eq8(x, 0x27u)) << (8 * j);
    }
    B &= kAll;
    const pt_u128 st = (~cont | B) & kAll;               // character starts
    const pt_u128 one = ~hi & st & (st >> 1);            // characters of exactly one byte below 0x80
    pt_u128 S = aS & one, L = aL & one, N = aN & one;
    sp &= one;
    ap &= one;
    for (pt_u128 todo = hi & st; todo;) {                // every other character: its length, its value, the table
        const uint64_t lo = (uint64_t)todo;
        const int i = lo ? __builtin_ctzll(lo) : 64 + __builtin_ctzll((uint64_t)(todo >> 64));
        todo &= todo - 1;
        const pt_u128 next = st >> (i + 1);
        const uint64_t nlo = (uint64_t)next;             // (a character of more than four bytes is O whatever its length)
        const int len = (nlo & 15u) ? __builtin_ctzll(nlo) + 1 : 5;
        if (len == 1 || i + len > kPtWindow) continue;   // (one byte of 0x80 or more: O)
        const int c = pt_class_char(win.byte(i), win.byte(i + 1), len > 2 ? win.byte(i + 2) : 0xFFu, len > 3 ? win.byte(i + 3) : 0xFFu, len, T);
        const pt_u128 bit = (pt_u128)1 << i;
        if (c == kPtS) S |= bit;
        else if (c == kPtL) L |= bit;
        else if (c == kPtN) N |= bit;
    }
    for (int r = 0; r < 3; ++r) {                        // a character's class on all its bytes (a classed character has at most four)
        S |= (S << 1) & ~st;
        L |= (L << 1) & ~st;
        N |= (N << 1) & ~st;
    }
    const pt_u128 pS = S << 1, pL = L << 1, pN = N << 1, pSp = sp << 1;   // the class of the byte in front
    const pt_u128 after_space = pS & ~pSp;               // behind white space that is not the byte 0x20
    // rule 1
    pt_u128 inside = 0, forced = 0;
    for (pt_u128 todo = ap & (B | pL | pN | after_space); todo;) {
        const uint64_t lo = (uint64_t)todo;
        const int i = lo ? __builtin_ctzll(lo) : 64 + __builtin_ctzll((uint64_t)(todo >> 64));
        todo &= todo - 1;
        if (i + 3 >= kPtWindow) continue;
        const int k = pt_contraction(win.byte(i + 1), win.byte(i + 2));
        if (k == 0) continue;
        const pt_u128 letters = (((pt_u128)1 << (k - 1)) - 1) << (i + 1);
        if ((B & letters) || !((st >> (i + k)) & 1)) continue;   // the letters are whole characters of this string
        inside |= letters;
        forced |= ((pt_u128)1 << (i + k)) & ~B;
    }
    // rule 2: T = the last byte of a white-space character whose next character exists and is not white space, moved to its first byte
    const pt_u128 t = S & ~(S >> 1) & ~(B >> 1);
    const pt_u128 st1 = st >> 1, st2 = st >> 2, st3 = st >> 3;
    const pt_u128 t_lead = (st1 & t) | (~st1 & st2 & (t >> 1)) | (~st1 & ~st2 & st3 & (t >> 2));
    const pt_u128 start2 = S & (B | forced | ~pS | t_lead);
    // rule 3
    const pt_u128 start3 = ~S & (B | forced | after_space | (~pS & ((L ^ pL) | (N ^ pN))));
    return (uint64_t)(((start2 | start3) & st & ~inside) >> kPtHalo);
}

// ==== the cl100k / Llama 3 pre-tokenizer (LATOK_PRETOK_CL100K; the definition: include/latok_hip.h behind latok_bpe_pretokenizer) ====
// Characters and classes are the ones above.  Unlike GPT-2's rule this one is not local: four facts reach as far along the text as a
// run of characters goes, and each of them is CARRIED from word to word:
//   d          the number of N characters directly in front of a position, mod 3 (digits are cut in threes)        left to right
//   absorbed   an NL behind "O NL*" belongs to the O's pre-token                                                    left to right
//   notopen    the character in front is an O that does not open a pre-token.  Only a malformed character of more
//              than a dozen bytes moves its lead byte out of the window, but then the fact has to come from there    left to right
//   nl_ahead   an NL follows in this run of white space                                                             right to left
// A character belongs to the word that holds its lead byte.  The left-to-right carries of a word say what holds for the last character
// whose lead byte lies in front of the word; nl_ahead says what holds for the byte behind the word's last.  String starts cut every
// carry, inside the word function: a carry is never wrong for arriving across one.
// A RECORD says what a word (a tile, any stretch of words) does to the carries that pass through it: for each either "pass it on" (d:
// "add my count") or "replace it with this value".  Records compose associatively (pt_rec_then), so a wave combines 64 of them with
// ballots (pt_rec_left / pt_rec_right over the nine ballot words) and nothing is ever waited for.
//   bits 0-1 d value / count, bit 2 d pass; bit 3 absorbed, bit 4 pass; bit 5 notopen, bit 6 pass; bit 7 nl_ahead, bit 8 pass
constexpr int kPretokCl100k = 3;
constexpr uint32_t kPtRecPass = 0x154u, kPtRecZero = 0u;   // the identity; "every carry is 0 behind me" (the batch's two ends)
constexpr int kPtRecBits = 9;

PT_FN uint32_t pt_rec_then(uint32_t a, uint32_t b) {      // a stretch with record a, then (to its right) one with record b
    uint32_t r = 0;
    if (b & 4u) r |= (a & 4u) | (((a & 3u) + (b & 3u)) % 3u);
    else r |= b & 7u;
    r |= (b & 0x10u) ? (a & 0x18u) : (b & 0x18u);
    r |= (b & 0x40u) ? (a & 0x60u) : (b & 0x60u);
    r |= (a & 0x100u) ? (b & 0x180u) : (a & 0x180u);
    return r;
}
PT_FN int pt_popc64(uint64_t x) { return __builtin_popcountll(x); }
// K[b] = bit b of the records of 64 consecutive stretches, stretch j in bit j.  The record of the stretches in `m` = the lowest n bits
// (left-to-right carries only; the nl_ahead field comes back as "pass") ...
PT_FN uint32_t pt_rec_left(const uint64_t* K, uint64_t m) {
    uint32_t r = 0x100u;
    uint64_t np = ~K[2] & m, rng = m;
    uint32_t v = 0;
    if (np) {
        const int j = 63 - __builtin_clzll(np);
        rng = m & ~((2ull << j) - 1ull);
        v = (uint32_t)((K[0] >> j) & 1u) + 2u * (uint32_t)((K[1] >> j) & 1u);
    } else {
        r |= 4u;
    }
    r |= (v + (uint32_t)pt_popc64(K[0] & rng) + 2u * (uint32_t)pt_popc64(K[1] & rng)) % 3u;
    np = ~K[4] & m;
    r |= np ? (uint32_t)((K[3] >> (63 - __builtin_clzll(np))) & 1u) << 3 : 0x10u;
    np = ~K[6] & m;
    r |= np ? (uint32_t)((K[5] >> (63 - __builtin_clzll(np))) & 1u) << 5 : 0x40u;
    return r;
}
// ... and, for nl_ahead, of the stretches in `m` = some highest bits (the other fields come back as "pass")
PT_FN uint32_t pt_rec_right(const uint64_t* K, uint64_t m) {
    const uint64_t np = ~K[8] & m;
    return 0x54u | (np ? (uint32_t)((K[7] >> __builtin_ctzll(np)) & 1u) << 7 : 0x100u);
}

struct PtCarry {        // what enters a word (the value fields of a record that no longer passes anything)
    uint32_t d = 0;     // 0 .. 2
    bool absorbed = false, notopen = false, nl_ahead = false;
};
PT_FN PtCarry pt_carry_of(uint32_t rec) {
    PtCarry c;
    c.d = rec & 3u;
    c.absorbed = (rec & 8u) != 0;
    c.notopen = (rec & 0x20u) != 0;
    c.nl_ahead = (rec & 0x80u) != 0;
    return c;
}

PT_FN uint64_t pt_rev64(uint64_t x) {
#if defined(__clang__)
    return __builtin_bitreverse64(x);
#else
    x = ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
    return __builtin_bswap64(x);
#endif
}
PT_FN pt_u128 pt_rev128(pt_u128 x) { return ((pt_u128)pt_rev64((uint64_t)x) << 64) | pt_rev64((uint64_t)(x >> 64)); }
// r(i) = s(i) | (p(i) & r(i - 1)): the seeds s spread upwards through p.  It is the carry-out vector of (s | p) + s.
PT_FN pt_u128 pt_flood_up(pt_u128 s, pt_u128 p) {
    const pt_u128 a = s | p;
    return ((a + s) ^ a ^ s) >> 1;
}
// r(i) = s(i) | (p(i) & r(i + 1))
PT_FN pt_u128 pt_flood_down(pt_u128 s, pt_u128 p) { return pt_rev128(pt_flood_up(pt_rev128(s), pt_rev128(p))); }
// q holds facts about characters, at their lead bytes: the same facts at the lead byte of the NEXT character of the same string (the
// carry of the addition runs through the continuation bytes in between)
PT_FN pt_u128 pt_to_next(pt_u128 q, pt_u128 st, pt_u128 B, pt_u128 all) { return (((q << 1) + (~st & all)) & st & ~B) & all; }

// the bytes of a contraction that an apostrophe opens when b1, b2 follow it: 2, 3, or 0 for none ((?i): either case; U+017F is C5 BF)
PT_FN int pt_cl100k_contraction(uint32_t b1, uint32_t b2) {
    const uint32_t l1 = b1 | 0x20u, l2 = b2 | 0x20u;
    if (l1 == 's' || l1 == 't' || l1 == 'm' || l1 == 'd') return 2;
    if ((l1 == 'r' || l1 == 'v') && l2 == 'e') return 3;
    if (l1 == 'l' && l2 == 'l') return 3;
    return (b1 == 0xC5u && b2 == 0xBFu) ? 3 : 0;
}

// ---- the scalar walk ---------------------------------------------------------------------------------------------------------------
// start[i] = 1 where a pre-token of the string s[0 .. n) starts, else 0.  `cls` is scratch of n bytes.
inline void pt_cl100k_starts_scalar(const uint8_t* s, int64_t n, const PretokTables& T, uint8_t* cls, uint8_t* start) {
    auto is_start = [&](int64_t i) { return i == 0 || (s[i] & 0xC0u) != 0x80u; };
    auto next_of = [&](int64_t i) { int64_t e = i + 1; while (e < n && !is_start(e)) ++e; return e; };
    auto prev_of = [&](int64_t i) { int64_t p = i - 1; while (!is_start(p)) --p; return p; };
    for (int64_t i = 0; i < n;) {
        const int64_t e = next_of(i);
        const int c = pt_class_char(s[i], e - i > 1 ? s[i + 1] : 0xFFu, e - i > 2 ? s[i + 2] : 0xFFu, e - i > 3 ? s[i + 3] : 0xFFu,
                                    e - i > 4 ? 5 : (int)(e - i), T);
        for (int64_t j = i; j < e; ++j) { cls[j] = (uint8_t)c; start[j] = 0; }
        i = e;
    }
    auto is_nl = [&](int64_t i) { return (s[i] == 0x0Au || s[i] == 0x0Du) && cls[i] == kPtS; };   // (cls: a single byte, not a malformed character)
    auto is_open = [&](int64_t i) { return i == 0 || !(cls[i - 1] == kPtO || (s[i - 1] == 0x20u && cls[i - 1] == kPtS)); };
    // rule 1: bit 1 = inside a contraction, bit 2 = forced, bit 3 = absorbed, bit 4 = nl_ahead
    for (int64_t i = 0; i < n; ++i) {
        if (s[i] != 0x27u || cls[i] != kPtO || !is_start(i) || next_of(i) != i + 1 || !is_open(i)) continue;
        const int k = pt_cl100k_contraction(i + 1 < n ? s[i + 1] : 0u, i + 2 < n ? s[i + 2] : 0u);
        if (k == 0 || i + k > n || (i + k < n && !is_start(i + k))) continue;
        if (k == 3 && s[i + 1] < 0x80u && !is_start(i + 2)) continue;
        for (int j = 1; j < k; ++j) start[i + j] |= 2u;
        if (i + k < n) start[i + k] |= 4u;
    }
    for (int64_t i = 1; i < n; ++i)
        if (is_start(i) && is_nl(i) && (cls[i - 1] == kPtO || (start[i - 1] & 8u))) start[i] |= 8u;
    for (int64_t i = n - 1; i >= 0; --i) {
        if (!is_start(i) || cls[i] != kPtS) continue;
        const int64_t e = next_of(i);
        if (is_nl(i) || (e < n && cls[e] == kPtS && (start[e] & 16u))) start[i] |= 16u;
    }
    int64_t d = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (!is_start(i)) continue;
        const uint8_t f = start[i];
        const int64_t p = i > 0 ? prev_of(i) : 0;
        d = (i > 0 && cls[p] == kPtN) ? d + 1 : 0;
        if (f & 2u) continue;
        bool st = i == 0 || (f & 4u);
        if (st) {
        } else if (cls[i] == kPtL) {
            st = cls[p] == kPtN || is_nl(p) || (cls[p] == kPtO && !is_open(p));
        } else if (cls[i] == kPtN) {
            st = cls[p] != kPtN || d % 3 == 0;
        } else if (cls[i] == kPtO) {
            st = is_open(i);
        } else if (f & 8u) {
            st = false;
        } else if (cls[p] != kPtS || (start[p] & 8u)) {
            st = true;
        } else {
            const int64_t e = next_of(i);
            st = (is_nl(p) && !(f & 16u)) || (e < n && cls[e] != kPtS && !is_nl(i));
        }
        if (st) start[i] |= 1u;
    }
    for (int64_t i = 0; i < n; ++i) start[i] &= 1u;
}

// ---- the word ----------------------------------------------------------------------------------------------------------------------
// What a word's window says without any carry: character starts, the classes and the three single bytes AT LEAD BYTES, and what follows
// from them.  pt_cl100k_prepare fills it; pt_cl100k_record and pt_cl100k_finish read it.
struct PtCl {
    pt_u128 st, B, has_prev;         // character starts; string starts (and the batch's end); characters with one in front of them
    pt_u128 S, L, N, O;              // classes, at lead bytes
    pt_u128 nl, Sm;                  // NL characters; S on all the bytes of its characters
    pt_u128 pS, pN, pO, pNl;         // the class of the character in front, at lead bytes
    pt_u128 open, notopen;           // open(i); O characters that are not open
    pt_u128 inside, forced;          // rule 1
    pt_u128 next_not_s;              // S characters whose next character exists and is not S
};
constexpr pt_u128 kPtAll = ((pt_u128)0xFFFFFFFFull << 64) | ~0ull;
constexpr pt_u128 kPtWordBits = (pt_u128)~0ull << kPtHalo;           // the word's own bytes in its window
constexpr pt_u128 kPtFrom = kPtAll & ~(((pt_u128)1 << kPtHalo) - 1);  // ... and everything behind them
PT_FN int pt_ctz128(pt_u128 x) {
    const uint64_t lo = (uint64_t)x;
    return lo ? __builtin_ctzll(lo) : 64 + __builtin_ctzll((uint64_t)(x >> 64));
}

template <class Window>
PT_FN void pt_cl100k_prepare(const Window& win, pt_u128 B, const PretokTables& T, PtCl& c) {
    pt_u128 hi = 0, cont = 0, aS = 0, aL = 0, aN = 0, sp = 0, ap = 0, nl = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < kPtWindow / 8; ++j) {
        const uint64_t x = win.qword(j), top = x & kPtTop, x7 = x & kPtLow7, lower = x7 | (kPtOnes * 0x20u);
        const uint64_t space = pt_eq8(x, 0x20u);
        hi |= (pt_u128)pt_gather8(top) << (8 * j);
        cont |= (pt_u128)pt_gather8(top & ~(x << 1)) << (8 * j);
        aL |= (pt_u128)pt_gather8(pt_ge8(lower, 'a') & ~pt_ge8(lower, 'z' + 1)) << (8 * j);
        aN |= (pt_u128)pt_gather8(pt_ge8(x7, '0') & ~pt_ge8(x7, '9' + 1)) << (8 * j);
        aS |= (pt_u128)pt_gather8((pt_ge8(x7, 0x09u) & ~pt_ge8(x7, 0x0Eu)) | space) << (8 * j);
        sp |= (pt_u128)pt_gather8(space) << (8 * j);
        ap |= (pt_u128)pt_gather8(pt_eq8(x, 0x27u)) << (8 * j);
        nl |= (pt_u128)pt_gather8(pt_eq8(x, 0x0Au) | pt_eq8(x, 0x0Du)) << (8 * j);
    }
    B &= kPtAll;
    const pt_u128 st = (~cont | B) & kPtAll;
    const pt_u128 one = ~hi & st & (st >> 1);            // characters of exactly one byte below 0x80
    pt_u128 S = aS & one, L = aL & one, N = aN & one;
    sp &= one;
    ap &= one;
    nl &= one;
    for (pt_u128 todo = hi & st; todo;) {
        const int i = pt_ctz128(todo);
        todo &= todo - 1;
        const uint64_t nlo = (uint64_t)(st >> (i + 1));
        const int len = (nlo & 15u) ? __builtin_ctzll(nlo) + 1 : 5;
        if (len == 1 || i + len > kPtWindow) continue;
        const int k = pt_class_char(win.byte(i), win.byte(i + 1), len > 2 ? win.byte(i + 2) : 0xFFu, len > 3 ? win.byte(i + 3) : 0xFFu, len, T);
        const pt_u128 bit = (pt_u128)1 << i;
        if (k == kPtS) S |= bit;
        else if (k == kPtL) L |= bit;
        else if (k == kPtN) N |= bit;
    }
    c.st = st;
    c.B = B;
    c.has_prev = st & ~B;
    c.S = S;
    c.L = L;
    c.N = N;
    c.O = st & ~(S | L | N);
    c.nl = nl;
    c.Sm = S | ((S << 1) & ~st);
    c.Sm |= (c.Sm << 1) & ~st & kPtAll;
    c.pS = pt_to_next(S, st, B, kPtAll);
    c.pN = pt_to_next(N, st, B, kPtAll);
    const pt_u128 pL = pt_to_next(L, st, B, kPtAll);
    c.pO = c.has_prev & ~(c.pS | pL | c.pN);             // (whatever is in front and none of the three: also a character that began far away)
    c.pNl = (nl << 1) & c.has_prev;
    c.open = st & ~(c.pO | ((sp << 1) & c.has_prev));
    c.notopen = c.O & ~c.open;
    // rule 1
    pt_u128 inside = 0, forced = 0;
    for (pt_u128 todo = ap & c.open; todo;) {
        const int i = pt_ctz128(todo);
        todo &= todo - 1;
        if (i + 3 >= kPtWindow) continue;
        const int k = pt_cl100k_contraction(win.byte(i + 1), win.byte(i + 2));
        if (k == 0) continue;
        const pt_u128 letters = (((pt_u128)1 << (k - 1)) - 1) << (i + 1);
        if ((B & letters) || !((st >> (i + k)) & 1)) continue;   // the letters are whole characters of this string
        inside |= letters;
        forced |= ((pt_u128)1 << (i + k)) & ~B;
    }
    c.inside = inside;
    c.forced = forced;
    const pt_u128 z = c.has_prev & ~S, st1 = st >> 1, st2 = st >> 2, st3 = st >> 3;
    c.next_not_s = S & ((st1 & (z >> 1)) | (~st1 & st2 & (z >> 2)) | (~st1 & ~st2 & st3 & (z >> 3)));
}

// absorbed on every byte, given the value at the byte in front of the word (bit kPtHalo - 1)
PT_FN pt_u128 pt_cl100k_absorbed(const PtCl& c, bool in) {
    const pt_u128 p = c.nl & c.has_prev;
    return pt_flood_up((p & c.pO & kPtFrom) | (in ? (c.nl & ((pt_u128)1 << (kPtHalo - 1))) : 0), p);
}

// what the word does to the carries that pass through it
PT_FN uint32_t pt_cl100k_record(const PtCl& c) {
    uint32_t r = 0;
    const uint64_t leads = (uint64_t)(c.st >> kPtHalo);
    // d: the N characters at the word's end, back to a character that is not N or starts a string
    const uint64_t stop = leads & (uint64_t)((~c.N | c.B) >> kPtHalo);
    if (leads == 0) {
        r |= 0x40u;                                          // no character starts here: one long O goes on (d = 0, absorbed = 0, notopen passes)
    } else {
        const int top = 63 - __builtin_clzll(leads);
        r |= (uint32_t)((c.notopen >> (kPtHalo + top)) & 1) << 5;
        if (stop == 0) {
            r |= 4u | (uint32_t)(pt_popc64(leads) % 3);
        } else {
            const int h = 63 - __builtin_clzll(stop);
            const uint64_t above = leads & ~((2ull << h) - 1ull);
            r |= (uint32_t)((pt_popc64(above) + (int)((c.N >> (kPtHalo + h)) & 1)) % 3);
        }
    }
    // absorbed: passes through 64 NL bytes of one string, unless the first of them follows an O and sets it
    const pt_u128 p = c.nl & c.has_prev;
    if ((pt_cl100k_absorbed(c, false) >> (kPtHalo + kPtWord - 1)) & 1) r |= 8u;
    else if ((uint64_t)(p >> kPtHalo) == ~0ull) r |= 0x10u;
    // nl_ahead: passes downwards through 64 bytes of S characters without an NL or a string's end
    const uint64_t m = (uint64_t)((c.Sm & ~(c.B >> 1)) >> kPtHalo), s = (uint64_t)((c.nl & c.Sm) >> kPtHalo);
    const int tz = ~m ? __builtin_ctzll(~m) : 64;
    const uint64_t reach = tz >= 63 ? ~0ull : (2ull << tz) - 1ull;   // the bytes up to and with the first that stops the run
    if (s & reach) r |= 0x80u;
    else if (tz == 64) r |= 0x100u;
    return r;
}

// the start bits of the word's 64 bytes, given the carries that enter it
PT_FN uint64_t pt_cl100k_finish(const PtCl& c, const PtCarry& in) {
    const pt_u128 st = c.st, B = c.B;
    const pt_u128 first = (st & kPtFrom) & (~(st & kPtFrom) + 1);   // the first character of the word
    // rule 2
    const pt_u128 pNO = pt_to_next(c.notopen & kPtFrom, st, B, kPtAll) | (in.notopen ? first & c.has_prev : 0);
    const pt_u128 startL = c.L & (c.pN | c.pNl | pNO);
    // rule 3: the first of every three, counted from the run's start (or from what the carry says about a run that enters the word)
    auto next_n = [&](pt_u128 q) { return pt_to_next(q, st, B, kPtAll) & c.N; };
    pt_u128 every3 = c.N & ~c.pN & kPtFrom;
    if (first & c.N & c.pN) every3 |= in.d == 0 ? first : in.d == 2 ? next_n(first) : next_n(next_n(first));
    for (pt_u128 cur = every3; cur;) {
        cur = next_n(next_n(next_n(cur)));
        every3 |= cur;
    }
    // rule 5
    const pt_u128 A = pt_cl100k_absorbed(c, in.absorbed);
    const pt_u128 R = pt_flood_down((c.nl | (in.nl_ahead ? (pt_u128)1 << (kPtHalo + kPtWord) : 0)) & c.Sm, c.Sm & ~(B >> 1));
    const pt_u128 startS = c.S & ~A & (~c.pS | (A << 1) | (c.pNl & ~R) | (c.next_not_s & ~c.nl));
    const pt_u128 start = (B | c.forced | startL | every3 | (c.O & c.open) | startS) & st & ~c.inside;
    return (uint64_t)(start >> kPtHalo);
}

// The start bits of the 64 bytes in the middle of a window (win, B: as for pt_word_starts), given the carries that enter the word.
template <class Window>
PT_FN uint64_t pt_cl100k_word_starts(const Window& win, pt_u128 B, const PtCarry& carry, const PretokTables& T) {
    PtCl c;
    pt_cl100k_prepare(win, B, T, c);
    return pt_cl100k_finish(c, carry);
}

#endif
