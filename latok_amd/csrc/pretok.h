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

#endif
