// fold_map.h -- case folding and accent stripping of UTF-8 (latok_fold_utf8_bytes_batch, include/latok_hip.h): the map of one
// code point, the UTF-8 encoder, the step over one byte position and the scalar walk over one string.  Plain C++17, like
// wordpiece.h and vocab_table.h: it compiles on the host (tests/helpers/fold_harness.cpp runs it against a plain-Python
// restatement of the definition) and, under hipcc, on the device, where fold_kernels.hip calls the very same fold_step.
//
//   tables     fold_tables.inc (tools/gen_fold_tables.py): two stages over the code points below U+30000 lead to a record of
//              ten dwords, {meta, image under LOWER, under STRIP_MARKS, under both}; above it three ranges.  Code points below
//              U+0080, Hangul syllables and the CJK ranges are arithmetic and never touch the tables.
//   fold_cp    F_fold(c): 0 .. 3 code points; `same` = the image is [c].
//   fold_step  one byte position of a string: a lead byte that opens a sequence inside the string gives the sequence's image
//              (its own bytes where the image is [c]), every other byte itself.  The caller skips the bytes a sequence consumed.
#ifndef LATOK_FOLD_MAP_H
#define LATOK_FOLD_MAP_H
#include <stdint.h>

#if defined(__HIPCC__)
#define FOLD_FN __host__ __device__ __forceinline__
#else
#define FOLD_FN inline
#endif

// (the public constants of include/latok_hip.h, restated so that this header stands alone)
constexpr int kFoldLower = 1, kFoldStripMarks = 2, kFoldClean = 4, kFoldCjkSpace = 8, kFoldAll = 15;
constexpr uint32_t kFoldMetaDrop = 1u << 6, kFoldMetaSpace = 1u << 7, kFoldMetaMn = 1u << 8;
constexpr uint32_t kFoldTableLimit = 0x30000u, kFoldTableShift = 7;
constexpr int kFoldRecWords = 10;
constexpr uint32_t kHangulSBase = 0xAC00u, kHangulLBase = 0x1100u, kHangulVBase = 0x1161u, kHangulTBase = 0x11A7u;
constexpr uint32_t kHangulSCount = 11172u, kHangulNCount = 588u, kHangulTCount = 28u;

struct FoldTables {
    const uint16_t* stage1 = nullptr;   // [kFoldTableLimit >> kFoldTableShift]
    const uint16_t* stage2 = nullptr;   // [blocks << kFoldTableShift]
    const uint32_t* rec = nullptr;      // [records * kFoldRecWords]
    const uint32_t* high = nullptr;     // [n_high * 3]: first, last, meta
    int n_high = 0;
};

FOLD_FN bool fold_is_cjk(uint32_t c) {
    return (c >= 0x4E00u && c <= 0x9FFFu) || (c >= 0x3400u && c <= 0x4DBFu) || (c >= 0x20000u && c <= 0x2A6DFu) ||
           (c >= 0x2A700u && c <= 0x2B73Fu) || (c >= 0x2B740u && c <= 0x2B81Fu) || (c >= 0x2B820u && c <= 0x2CEAFu) ||
           (c >= 0xF900u && c <= 0xFAFFu) || (c >= 0x2F800u && c <= 0x2FA1Fu);
}

struct FoldImage {
    uint32_t cp[3];
    int n;        // 0 .. 3
    bool same;    // the image is [c]
};

// CLEAN on a code point below U+0080: 0 = dropped, else the image
FOLD_FN uint32_t fold_ascii_clean(uint32_t c) {
    if (c == 9u || c == 10u || c == 13u) return 0x20u;
    return (c < 0x20u || c == 0x7Fu) ? 0u : c;
}

// F_fold(c); fold == 0 is the identity
FOLD_FN FoldImage fold_cp(uint32_t c, int fold, const FoldTables& T) {
    FoldImage r;
    r.cp[0] = c; r.cp[1] = 0; r.cp[2] = 0;
    r.n = 1;
    r.same = true;
    if (fold == 0) return r;
    if ((c >= 0xD800u && c <= 0xDFFFu) || c > 0x10FFFFu) return r;
    if (c < 0x80u) {
        uint32_t x = c;
        if (fold & kFoldClean) {
            x = fold_ascii_clean(c);
            if (x == 0u) { r.n = 0; r.same = false; return r; }
        }
        if ((fold & kFoldLower) && x >= 'A' && x <= 'Z') x += 32u;
        r.cp[0] = x;
        r.same = x == c;
        return r;
    }
    const int v = fold & 3;
    if (c - kHangulSBase < kHangulSCount) {   // (no Hangul syllable is Cc, Cf or Zs, lower-cases or is a CJK ideograph)
        if (v & kFoldStripMarks) {
            const uint32_t s = c - kHangulSBase, t = s % kHangulTCount;
            r.cp[0] = kHangulLBase + s / kHangulNCount;
            r.cp[1] = kHangulVBase + (s % kHangulNCount) / kHangulTCount;
            r.cp[2] = kHangulTBase + t;
            r.n = t ? 3 : 2;
            r.same = false;
        }
        return r;
    }
    uint32_t meta = 0;
    const uint32_t* rec = nullptr;
    if (c < kFoldTableLimit) {
        const uint32_t ri = T.stage2[((uint32_t)T.stage1[c >> kFoldTableShift] << kFoldTableShift) | (c & ((1u << kFoldTableShift) - 1u))];
        if (ri) {
            rec = T.rec + (size_t)ri * kFoldRecWords;
            meta = rec[0];
        }
    } else {
        for (int i = 0; i < T.n_high; ++i)
            if (c >= T.high[3 * i] && c <= T.high[3 * i + 1]) meta = T.high[3 * i + 2];
    }
    if (fold & kFoldClean) {
        if (meta & kFoldMetaDrop) { r.n = 0; r.same = false; return r; }
        if (meta & kFoldMetaSpace) { r.cp[0] = 0x20u; r.same = false; return r; }
    }
    if (v && rec) {
        r.n = (int)((meta >> (2 * (v - 1))) & 3u);
        const uint32_t* img = rec + 1 + 3 * (v - 1);
        r.cp[0] = img[0]; r.cp[1] = img[1]; r.cp[2] = img[2];
        r.same = r.n == 1 && r.cp[0] == c;
    } else if ((v & kFoldStripMarks) && (meta & kFoldMetaMn)) {
        r.n = 0;
        r.same = false;
    }
    if ((fold & kFoldCjkSpace) && fold_is_cjk(c)) {   // (an ideograph's image is one code point under every variant)
        r.cp[1] = r.cp[0];
        r.cp[0] = 0x20u;
        r.cp[2] = 0x20u;
        r.n = 3;
        r.same = false;
    }
    return r;
}

// shortest-form UTF-8 of a scalar value: the bytes in memory order in the low end of the result, *len = 1 .. 4
FOLD_FN uint32_t fold_utf8_word(uint32_t c, int* len) {
    if (c < 0x80u) { *len = 1; return c; }
    if (c < 0x800u) { *len = 2; return (0xC0u | (c >> 6)) | ((0x80u | (c & 0x3Fu)) << 8); }
    if (c < 0x10000u) { *len = 3; return (0xE0u | (c >> 12)) | ((0x80u | ((c >> 6) & 0x3Fu)) << 8) | ((0x80u | (c & 0x3Fu)) << 16); }
    *len = 4;
    return (0xF0u | (c >> 18)) | ((0x80u | ((c >> 12) & 0x3Fu)) << 8) | ((0x80u | ((c >> 6) & 0x3Fu)) << 16) | ((0x80u | (c & 0x3Fu)) << 24);
}

// continuation bytes the lead byte b0 announces (tests/helpers/utf8_ref.py: n_cont)
FOLD_FN int fold_n_cont(uint32_t b0) { return (int)(b0 >= 0xC0u) + (int)(b0 >= 0xE0u) + (int)(b0 >= 0xF0u); }

// Bytes of the sequence that the byte position with the 4 bytes W (memory order; bytes that do not exist: anything) opens, 1 if it
// opens none: a lead byte whose k continuation bytes lie inside the string (`avail` >= 1 = bytes from this position to the end of its
// string, 4 stands for more) and are all 10xxxxxx.
FOLD_FN int fold_seq_len(uint32_t W, int avail) {
    const int k = fold_n_cont(W & 0xFFu);
    if (k == 0 || k >= avail) return 1;                                   // ASCII, a stray continuation byte; a tail that leaves the string
    const uint32_t need = 0x00C0C0C0u >> (8 * (3 - k));                   // the top two bits of tail bytes 1 .. k
    return (((W >> 8) ^ 0x00808080u) & need) != 0u ? 1 : k + 1;           // one of them is not 10xxxxxx
}

// What the byte position whose 4 bytes in memory order are W gives (bytes that do not exist: anything), `avail` >= 1 = bytes from
// this position to the end of its string (4 stands for more).  w[j] / len[j]: up to three runs of 1 .. 4 output bytes; `used` = source
// bytes the position stands for (1, or the length of the sequence it opens); total = output bytes.
struct FoldStep {
    uint32_t w[3];
    int len[3];
    int used, total;
};
FOLD_FN FoldStep fold_step(uint32_t W, int avail, int fold, const FoldTables& T) {
    FoldStep s;
    const uint32_t b0 = W & 0xFFu;
    s.w[0] = b0; s.w[1] = 0; s.w[2] = 0;
    s.len[0] = 1; s.len[1] = 0; s.len[2] = 0;
    s.used = 1;
    s.total = 1;
    const int k = fold_seq_len(W, avail) - 1;
    uint32_t c = b0;
    if (b0 >= 0x80u) {
        if (k == 0) return s;                                             // no sequence: the byte itself
        c = b0 & (0x3Fu >> k);
        for (int j = 1; j <= 3; ++j)
            if (j <= k) c = (c << 6) | ((W >> (8 * j)) & 0x3Fu);
    }
    const FoldImage im = fold_cp(c, fold, T);
    if (im.same) {                                                        // verbatim: the source bytes, overlong forms included
        s.w[0] = k == 3 ? W : W & ((1u << (8 * (k + 1))) - 1u);
        s.len[0] = k + 1;
        s.used = k + 1;
        s.total = k + 1;
        return s;
    }
    s.used = k + 1;
    s.total = 0;
    s.len[0] = 0;
    for (int j = 0; j < 3; ++j)
        if (j < im.n) {
            s.w[j] = fold_utf8_word(im.cp[j], &s.len[j]);
            s.total += s.len[j];
        }
    return s;
}

// The scalar walk over one string s[0 .. n): the folded bytes go to out (NULL: count only); returns their number (<= 3 * n).
// fold == 0 is the copy.
inline int64_t fold_string(const uint8_t* s, int64_t n, int fold, const FoldTables& T, uint8_t* out) {
    int64_t o = 0;
    for (int64_t i = 0; i < n;) {
        if (fold == 0) {
            if (out) out[o] = s[i];
            ++o; ++i;
            continue;
        }
        uint32_t W = 0;
        const int avail = n - i >= 4 ? 4 : (int)(n - i);
        for (int j = 0; j < avail; ++j) W |= (uint32_t)s[i + j] << (8 * j);
        const FoldStep st = fold_step(W, avail, fold, T);
        for (int j = 0; j < 3; ++j)
            for (int b = 0; b < st.len[j]; ++b) {
                if (out) out[o] = (uint8_t)(st.w[j] >> (8 * b));
                ++o;
            }
        i += st.used;
    }
    return o;
}

#endif
