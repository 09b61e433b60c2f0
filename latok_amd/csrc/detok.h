// detok.h -- decoding: ids back to bytes (detok_kernels.hip: k_detok_count, k_detok_write; include/latok_hip.h: latok_detok_*).
// Plain C++17, like vocab_table.h, wordpiece.h and bpe.h: the build runs on the host only; the lookup, the per-piece rule, the look-back
// and the byte copy compile on the host (tests/helpers/detok_harness.cpp runs them against tests/helpers/detok_ref.py, a restatement
// over Python lists and a dict) and, under hipcc, on the device.
//
//   the object   three things.  BLOB: the bytes of every entry, each word starting on a dword and zero-padded to one, below 2^32 bytes
//                (vocab_table.h's bound), one spare dword behind.  ENTRIES: one 16-byte record per word, in index order -- byte offset,
//                length, and in WORDPIECE mode the continuation bit and the offset past the prefix.  A word is a CONTINUATION word iff it
//                starts with the prefix and is longer than the prefix (the rule of wordpiece.h's continuation table); that is decided
//                here, on the host: the device compares no prefix byte.  MAP id -> entry: DENSE, an int32 array indexed by id - min_id
//                (-1 = no entry), when max_id - min_id + 1 <= kDtDenseSpread * n_words -- default ids, every .tiktoken file, BERT's
//                vocab.txt --, else SORTED, the distinct ids in increasing order beside their entries, searched by bisection.
//                Every int32 is a legal id; of several words with one id the LOWEST INDEX wins; the empty word is a legal entry;
//                duplicate words with different ids are all kept.
//   the rule     a piece is DROPPED when its id is in the caller's skip list or not in the map (unknown); a dropped piece leaves no
//                trace.  The other pieces of a row are KEPT, words w_0 .. w_k.  CONCAT: the row is w_0 + .. + w_k.  WORDPIECE: w_0
//                verbatim, prefix included; for j >= 1 a continuation word without its prefix, any other word as the sep byte followed
//                by the word (dt_piece).
//   look-back    "a kept piece stands in front of me in my row" (dt_has_prev) is asked only by a kept word in WORDPIECE mode, and
//                walks back over the run of dropped pieces directly in front of it, to the first kept piece or the row start.
//                Those runs are disjoint: the walks of a batch total at most its piece count.  The usual walk is 0 or 1 steps.
//   the bytes    are read from the blob as aligned dwords through a loader (dt_copy), one load per dword a piece's range touches;
//                an entry's range lies inside the blob, so nothing behind the blob's last dword is read.
#ifndef LATOK_DETOK_H
#define LATOK_DETOK_H
#include <stdint.h>

#include "token_hash.h"

#include <algorithm>
#include <vector>

constexpr int kDtConcat = 0, kDtWordPiece = 1;   // == LATOK_DETOK_CONCAT / LATOK_DETOK_WORDPIECE
constexpr int kDtMaxPrefix = 8;                  // bytes of the continuation prefix at most
constexpr int kDtMaxSkip = 16;                   // ids of a call's skip list at most
constexpr int64_t kDtDenseSpread = 4;            // the map is dense when the id range is at most this many times the word count
constexpr uint32_t kDtCont = 1u;                 // DtEntry::flags: a continuation word

struct alignas(16) DtEntry {
    uint32_t off;     // first byte of the word in the blob (a multiple of 4)
    uint32_t len;     // bytes
    uint32_t body;    // a continuation word: off + prefix_len; else off
    uint32_t flags;   // kDtCont
};
static_assert(sizeof(DtEntry) == 16, "an entry is one 16-byte load");

// the map as the lookup reads it: n = the id range (dense) or the number of distinct ids (sorted)
struct DtMap {
    int64_t n;
    int32_t min_id;
    int dense;
};
TH_FN bool dt_is_dense(int64_t id_range, int64_t n_words) { return n_words > 0 && id_range <= kDtDenseSpread * n_words; }

// the entry of `id`, -1 if there is none.  val(i) = entry i of the dense array / the entry beside sorted id i; key(i) = sorted id i
// (asked only in the sorted form).  The bisection runs at most 32 rounds by its own bounds, whatever the arrays hold.
template <class KeyLoad, class ValLoad>
TH_FN int32_t dt_lookup(const DtMap& m, KeyLoad key, ValLoad val, int32_t id) {
    if (m.dense) {
        const int64_t d = (int64_t)id - (int64_t)m.min_id;
        return d < 0 || d >= m.n ? -1 : val(d);
    }
    int64_t lo = 0, hi = m.n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (key(mid) < id) lo = mid + 1;
        else hi = mid;
    }
    return lo < m.n && key(lo) == id ? val(lo) : -1;
}

TH_FN bool dt_skipped(const int32_t* skip, int n_skip, int32_t id) {
    bool hit = false;
    for (int i = 0; i < kDtMaxSkip; ++i) hit |= i < n_skip && skip[i] == id;
    return hit;
}

// what a kept piece contributes: `sep` bytes of separator (0 / 1), then n bytes of the blob from byte src
struct DtPiece {
    uint32_t src, n, sep;
};
TH_FN uint32_t dt_piece_bytes(const DtPiece& p) { return p.n + p.sep; }
// THE RULE.  has_prev: a kept piece stands in front of this one in its row.  CONCAT never asks.  In WORDPIECE mode every kept word
// whose two forms differ asks: a continuation word is w_0 (verbatim) or not (without the prefix) by the same answer that gives any
// other word its separator.  Each walks over the dropped pieces directly in front of it only, so the bound above holds for all of them.
TH_FN bool dt_needs_prev(const DtEntry& e, int mode) { return mode == kDtWordPiece && (!(e.flags & kDtCont) || e.body != e.off); }
TH_FN DtPiece dt_piece(const DtEntry& e, int mode, bool has_prev) {
    if (mode != kDtWordPiece || !has_prev) return DtPiece{e.off, e.len, 0u};
    if (e.flags & kDtCont) return DtPiece{e.body, e.len - (e.body - e.off), 0u};
    return DtPiece{e.off, e.len, 1u};
}
// is a piece in [row_first, t) kept?  kept(u) = piece u is kept.  Walks back from t - 1 over dropped pieces.
template <class Kept>
TH_FN bool dt_has_prev(int64_t t, int64_t row_first, Kept kept) {
    for (int64_t u = t - 1; u >= row_first; --u)
        if (kept(u)) return true;
    return false;
}
// The write pass knows the entry and the byte count c > 0 the count pass recorded, and reads the form back from the two: len + 1 = behind a
// separator, len = verbatim, anything else = the continuation body (with an empty prefix the last two coincide, and are the same
// bytes).  A count that fits no form (the ids changed between the passes) contributes no blob byte.
TH_FN DtPiece dt_piece_of_count(const DtEntry& e, uint32_t c) {
    if (c == e.len + 1u) return DtPiece{e.off, e.len, 1u};
    if (c == e.len) return DtPiece{e.off, e.len, 0u};
    if ((e.flags & kDtCont) && c == e.len - (e.body - e.off)) return DtPiece{e.body, c, 0u};
    return DtPiece{e.off, 0u, 0u};
}

// output bytes [k0, k1) of piece p (0 <= k0 < k1 <= dt_piece_bytes(p)): put(k, byte).  blob(i) = dword i of the blob.
template <class BlobLoad, class Put>
TH_FN void dt_copy(const DtPiece& p, uint32_t sep_byte, BlobLoad blob, uint64_t k0, uint64_t k1, Put put) {
    uint64_t k = k0;
    if (p.sep && k == 0) {
        put(k, sep_byte);
        ++k;
    }
    if (k >= k1) return;
    uint64_t pos = (uint64_t)p.src + (k - p.sep);   // < src + n <= the blob's bytes
    uint32_t w = blob(pos >> 2);
    for (;;) {
        put(k, (w >> (8u * (uint32_t)(pos & 3u))) & 0xFFu);
        ++k;
        ++pos;
        if (k >= k1) return;
        if ((pos & 3u) == 0u) w = blob(pos >> 2);
    }
}

// ---- the build: host only ---------------------------------------------------------------------------------------------------
struct DtTable {
    std::vector<uint32_t> blob;     // at least one dword
    std::vector<DtEntry> entries;   // at least one record (so that its address is never NULL); n_words are real
    std::vector<int32_t> keys;      // sorted form: the distinct ids, increasing; at least one element
    std::vector<int32_t> vals;      // dense: entry by id - min_id, -1 = none; sorted: the entry beside keys[i]; at least one element
    DtMap map{0, 0, 0};
    int64_t n_words = 0, n_ids = 0;   // n_ids: distinct ids
    uint64_t blob_bytes = 0;          // of the padded words
    uint32_t max_len = 0;
    int mode = kDtConcat;
};
// words[word_off[i] : word_off[i+1]] = word i; ids may be NULL (id_i = i).  The caller has checked the offsets, the sizes and the mode
// (CONCAT: prefix_len = 0).
inline void dt_build(const uint8_t* words, const int64_t* word_off, int64_t n_words, const int32_t* ids, int mode, const uint8_t* prefix,
                     int prefix_len, DtTable* t) {
    t->mode = mode;
    t->n_words = n_words;
    t->max_len = 0;
    uint64_t padded = 0;
    for (int64_t i = 0; i < n_words; ++i) padded += ((uint64_t)(word_off[i + 1] - word_off[i]) + 3u) & ~3ull;
    t->blob_bytes = padded;
    t->blob.assign(padded / 4 + 1, 0u);
    t->entries.assign((size_t)std::max<int64_t>(n_words, 1), DtEntry{0u, 0u, 0u, 0u});
    uint8_t* bytes = reinterpret_cast<uint8_t*>(t->blob.data());
    uint64_t at = 0;
    int64_t lo = 0, hi = -1;
    for (int64_t i = 0; i < n_words; ++i) {
        const uint64_t len = (uint64_t)(word_off[i + 1] - word_off[i]);
        const uint8_t* w = words + word_off[i];
        for (uint64_t b = 0; b < len; ++b) bytes[at + b] = w[b];
        bool cont = mode == kDtWordPiece && len > (uint64_t)prefix_len;
        for (int b = 0; cont && b < prefix_len; ++b) cont = w[b] == prefix[b];
        t->entries[(size_t)i] = DtEntry{(uint32_t)at, (uint32_t)len, (uint32_t)(at + (cont ? (uint64_t)prefix_len : 0u)), cont ? kDtCont : 0u};
        if (len > t->max_len) t->max_len = (uint32_t)len;
        at += (len + 3u) & ~3ull;
        const int64_t id = ids ? (int64_t)ids[i] : i;
        if (i == 0 || id < lo) lo = id;
        if (i == 0 || id > hi) hi = id;
    }
    const int64_t range = n_words > 0 ? hi - lo + 1 : 0;
    t->keys.assign(1, 0);
    if (dt_is_dense(range, n_words)) {
        t->map = DtMap{range, (int32_t)lo, 1};
        t->vals.assign((size_t)range, -1);
        t->n_ids = 0;
        for (int64_t i = 0; i < n_words; ++i) {   // index order: the lowest index wins
            int32_t& slot = t->vals[(size_t)((ids ? (int64_t)ids[i] : i) - lo)];
            if (slot < 0) {
                slot = (int32_t)i;
                ++t->n_ids;
            }
        }
        return;
    }
    std::vector<int32_t> order((size_t)n_words);
    for (int64_t i = 0; i < n_words; ++i) order[(size_t)i] = (int32_t)i;
    std::stable_sort(order.begin(), order.end(), [ids](int32_t a, int32_t b) { return ids[a] < ids[b]; });   // (ids != NULL: default ids are dense)
    t->keys.clear();
    t->vals.clear();
    for (int32_t i : order)
        if (t->keys.empty() || t->keys.back() != ids[i]) {   // stable: the first of equal ids is the lowest index
            t->keys.push_back(ids[i]);
            t->vals.push_back(i);
        }
    t->n_ids = (int64_t)t->keys.size();
    t->map = DtMap{t->n_ids, 0, 0};
    if (t->keys.empty()) {
        t->keys.assign(1, 0);
        t->vals.assign(1, -1);
    }
}

#endif
