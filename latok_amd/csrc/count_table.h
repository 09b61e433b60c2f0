// count_table.h -- the counting table of the token-count call (compact_kernels.hip: CountTokens of scatter_block and the two
// commit kernels): an exact, insert-only map from a token's bytes to a 64-bit count, filled by many threads at once.  Plain C++17,
// like vocab_table.h: it compiles on the host (tests/helpers/count_table_harness.cpp runs it with std::atomic, single-threaded and
// with 8 threads on one table) and, under hipcc, on the device.  The atomic operations come through a policy parameter `A`:
//     A::load(const uint64_t* p)                      relaxed atomic load
//     A::cas(uint64_t* p, uint64_t expect, uint64_t v) relaxed compare-and-swap, returns the word that was there
// (on the device both are agent-scope __hip_atomic_* operations; on the host std::atomic_ref-like __atomic_* builtins).
//
//   layout     open addressing, linear probing.  n_slots = a power of two, >= 2 * max_words and >= 64 (ct_slot_count).  A slot is
//              ONE aligned 8-byte word that holds everything a prober needs; counts live in a parallel uint64[n_slots].
//                  bit  63      form: 1 = fresh (the position is a byte position in THIS batch's text), 0 = resident
//                  bits 62..55  length - 1                                   (a word has 1 .. 256 bytes)
//                  bits 54..39  the upper 16 bits of the word's hash, a filter (the lower bits chose the home slot)
//                  bits 38..0   position: fresh -- byte position of a representative token in the batch's text (< 2^39);
//                                         resident -- first dword of the word in the counter's own blob (>= 1)
//              0 = empty.  No occupied word is 0: a fresh word has bit 63, a resident word a position >= 1 (dword 0 of the blob
//              is reserved, as in VtTable).  Words in the blob start on a dword and are zero-padded to one.
//   find-or-insert (ct_find_or_insert)
//              from the home slot hash & (n_slots - 1) on: load the slot; empty -> CAS(0 -> my fresh word), and if that fails
//              look at the SAME slot again with the word the CAS returned (it is occupied now: at most one retry per slot);
//              length and filter agree -> compare the bytes (resident: vt_equal_lane against the blob; fresh: ct_equal_text
//              against the representative's bytes in the text), equal -> this is the slot; else the next slot, wrapping.
//              Nothing waits for another thread.  A slot goes empty -> occupied once and keeps its word's identity, so every
//              prober of a word walks the same occupied slots and meets either the word or the first empty slot: a word
//              never gets two slots.  The only memory shared inside a launch is the slot word, touched by atomics alone; the
//              bytes it points to (the input text, blob bytes stored by an earlier launch) are written by nobody meanwhile.
//   bound      the loop runs at most min(n_slots, probe_max) steps BY ITS OWN COUNTER; exhausted -> kCtDropped.
//   commit     (ct_commit_word) behind a batch every fresh slot gets its bytes copied into the blob and its word rewritten in
//              the resident form, so that no slot points into the caller's text once the call returns.
#ifndef LATOK_COUNT_TABLE_H
#define LATOK_COUNT_TABLE_H
#include <stdint.h>

#include "token_hash.h"
#include "vocab_table.h"

constexpr uint64_t kCtEmpty = 0ull;
constexpr uint64_t kCtFresh = 1ull << 63;
constexpr int kCtLenShift = 55, kCtFilterShift = 39;
constexpr uint64_t kCtPosMask = (1ull << kCtFilterShift) - 1ull;            // 39 bits
constexpr uint64_t kCtKeyMask = ~kCtFresh & ~kCtPosMask;                     // length and filter
constexpr int64_t kCtMaxTextBytes = (int64_t)1 << 39;                        // a fresh position must fit
constexpr int kCtMaxWordBytes = 256;                                         // 8 bits of length - 1
constexpr uint64_t kCtMinSlots = 64;
constexpr int64_t kCtDropped = -1;                                           // ct_find_or_insert: no slot within the bound

// slots of a table for max_words words
TH_FN uint64_t ct_slot_count(int64_t max_words) {
    uint64_t n = kCtMinSlots;
    while (n < 2ull * (uint64_t)max_words) n <<= 1;
    return n;
}
TH_FN uint64_t ct_key(uint32_t len, uint32_t hash) {
    return ((uint64_t)(len - 1u) << kCtLenShift) | ((uint64_t)(hash >> 16) << kCtFilterShift);
}
TH_FN uint64_t ct_fresh_word(uint32_t len, uint32_t hash, int64_t a) { return kCtFresh | ct_key(len, hash) | (uint64_t)a; }
TH_FN uint64_t ct_resident_word(uint64_t fresh, uint64_t dword) { return (fresh & kCtKeyMask) | dword; }
TH_FN uint32_t ct_len(uint64_t word) { return (uint32_t)((word >> kCtLenShift) & 0xFFu) + 1u; }
TH_FN uint64_t ct_pos(uint64_t word) { return word & kCtPosMask; }
TH_FN bool ct_is_fresh(uint64_t word) { return (word & kCtFresh) != 0ull; }
TH_FN uint32_t ct_padded_dwords(uint64_t word) { return (ct_len(word) + 3u) >> 2; }

// Two ranges of the text, both of e - a bytes (e > a): [a, e) against [b, b + e - a).  Each side is read as th_hash_lane reads a
// token: aligned dwords, th_align on the pair, the index clamped to the dword that holds that range's last byte.
template <class TextLoad>
TH_FN bool ct_equal_text(TextLoad ld, int64_t a, int64_t e, int64_t b) {
    const uint32_t len = (uint32_t)(e - a);
    const int64_t qa = a >> 2, last_a = (e - 1) >> 2, qb = b >> 2, last_b = (b + (e - a) - 1) >> 2;
    const uint32_t sa = (uint32_t)(a & 3), sb = (uint32_t)(b & 3);
    const int64_t nd = ((e - a) + 3) >> 2;
    uint32_t lo_a = ld(qa), lo_b = ld(qb);
    for (int64_t i = 0; i < nd; ++i) {
        const int64_t ia = qa + i + 1, ib = qb + i + 1;
        const uint32_t hi_a = ld(ia < last_a ? ia : last_a), hi_b = ld(ib < last_b ? ib : last_b);
        const uint32_t m = i + 1 < nd ? 0xFFFFFFFFu : vt_tail_mask(len);
        if ((th_align(hi_a, lo_a, sa) ^ th_align(hi_b, lo_b, sb)) & m) return false;
        lo_a = hi_a;
        lo_b = hi_b;
    }
    return true;
}

// The slot of the token [a, e) of the text (1 <= e - a <= kCtMaxWordBytes, a < 2^39) whose hash with the table's seed is `hash`:
// found, or claimed with a fresh word.  kCtDropped if neither the word nor a free slot lies within the bound.
template <class A, class TextLoad, class BlobLoad>
TH_FN int64_t ct_find_or_insert(TextLoad ld, int64_t a, int64_t e, uint32_t hash, uint64_t* slots, BlobLoad blob, uint64_t n_slots,
                                uint32_t probe_max) {
    const uint64_t mask = n_slots - 1;
    const uint64_t mine = ct_fresh_word((uint32_t)(e - a), hash, a);
    const uint64_t bound = n_slots < (uint64_t)probe_max ? n_slots : (uint64_t)probe_max;
    uint64_t s = hash & mask;
    for (uint64_t step = 0; step < bound; ++step) {   // (bounded here, not by the load factor)
        uint64_t v = A::load(slots + s);
        if (v == kCtEmpty) {
            v = A::cas(slots + s, kCtEmpty, mine);
            if (v == kCtEmpty) return (int64_t)s;     // claimed
        }
        if (((v ^ mine) & kCtKeyMask) == 0ull) {      // (v is occupied: whoever holds the slot holds it for good)
            const bool eq = ct_is_fresh(v) ? ct_equal_text(ld, a, e, (int64_t)ct_pos(v))
                                           : vt_equal_lane(ld, a, e, blob, (uint32_t)ct_pos(v));
            if (eq) return (int64_t)s;
        }
        s = (s + 1) & mask;
    }
    return kCtDropped;
}

// Commit of one fresh slot word: its bytes go from the text to dwords [at, at + ct_padded_dwords) of the blob, zero-padded;
// returns the resident word.  store(i, v): blob dword i = v.
template <class TextLoad, class BlobStore>
TH_FN uint64_t ct_commit_word(TextLoad ld, uint64_t fresh, uint64_t at, BlobStore store) {
    const uint32_t len = ct_len(fresh);
    const int64_t a = (int64_t)ct_pos(fresh), e = a + (int64_t)len;
    const int64_t q = a >> 2, last = (e - 1) >> 2;
    const uint32_t sh = (uint32_t)(a & 3);
    const int64_t nd = ((int64_t)len + 3) >> 2;
    uint32_t lo = ld(q);
    for (int64_t i = 0; i < nd; ++i) {
        const int64_t qi = q + i + 1;
        const uint32_t hi = ld(qi < last ? qi : last);
        store(at + (uint64_t)i, th_align(hi, lo, sh) & (i + 1 < nd ? 0xFFFFFFFFu : vt_tail_mask(len)));
        lo = hi;
    }
    return ct_resident_word(fresh, at);
}

#endif
