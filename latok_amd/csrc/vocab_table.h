// vocab_table.h -- the vocabulary table of the token-id call (compact_kernels.hip: IdTokens of scatter_block): an exact map
// from a token's bytes to an int32 id.  Plain C++17, like token_hash.h: the build runs on the host only; the probe and the
// compares compile on the host (tests/helpers/vocab_harness.cpp runs them against a Python dict) and, under hipcc, on the device.
//
//   layout     open addressing, linear probing.  n_slots = a power of two, >= 2 * n_words and >= 64.  One slot is 16 bytes
//              {hash, id, word offset (in dwords of the blob), word length (bytes)}: a probe step is one 16-byte load.  An empty
//              slot has len = kVtEmpty -- every 32-bit value is a legal hash, but no word is that long (the blob is < 2^32 bytes).
//              The words lie in a blob of dwords, each starting on a dword and zero-padded to one, so a compare reads whole
//              dwords and never leaves the blob.  Home slot = murmur3_x86_32(word, seed) & (n_slots - 1).
//   build      words in index order; a word equal to one already present is skipped (the first occurrence wins); the empty word
//              gets no slot (no token is empty, so it can never match).
//   probe      from the home slot on: an empty slot -> unknown; hash and length equal -> compare the bytes, equal -> the id;
//              else the next slot, wrapping at the end.  The loop runs at most n_slots steps BY ITS OWN COUNTER, whatever the
//              table holds: a table without an empty slot gives unk, it cannot spin.
//   compares   the token side is read as th_hash_lane reads it: aligned dwords through a loader, th_align on the pair, the index
//              clamped to the dword that holds the token's last byte, the last 1..3 bytes masked.  Nothing behind the aligned
//              dword that holds the batch's last byte is read.  vt_equal_lane: one thread walks the token.  vt_wave_differs:
//              lane l of a wave takes dword 64 r + l of a long token (coalesced loads); the caller ballots.
#ifndef LATOK_VOCAB_TABLE_H
#define LATOK_VOCAB_TABLE_H
#include <stdint.h>

#include "token_hash.h"

#include <vector>

constexpr uint32_t kVtEmpty = 0xFFFFFFFFu;   // VtSlot::len of an empty slot
constexpr uint64_t kVtMinSlots = 64;

struct alignas(16) VtSlot {
    uint32_t hash;
    int32_t id;
    uint32_t off;   // first dword of the word in the blob
    uint32_t len;   // bytes; kVtEmpty: the slot is empty
};
static_assert(sizeof(VtSlot) == 16, "a probe step is one 16-byte load");

// slots of a table for n_words words
TH_FN uint64_t vt_slot_count(int64_t n_words) {
    uint64_t n = kVtMinSlots;
    while (n < 2ull * (uint64_t)n_words) n <<= 1;
    return n;
}
TH_FN uint32_t vt_tail_mask(uint32_t len) { return (len & 3u) ? (1u << (8 * (len & 3u))) - 1u : 0xFFFFFFFFu; }

// The probe loop.  slot(i) = slot i of the table; equal(off) = "the token's bytes are the word at dword `off` of the blob" (asked
// only where hash and length agree).  n_slots is a power of two.
template <class SlotLoad, class Equal>
TH_FN int32_t vt_probe(SlotLoad slot, uint64_t n_slots, uint32_t hash, uint32_t len, Equal equal, int32_t unk) {
    const uint64_t mask = n_slots - 1;
    uint64_t s = hash & mask;
    for (uint64_t step = 0; step < n_slots; ++step) {   // (bounded here, not by the load factor)
        const VtSlot v = slot(s);
        if (v.len == kVtEmpty) return unk;
        if (v.hash == hash && v.len == len && equal(v.off)) return v.id;
        s = (s + 1) & mask;
    }
    return unk;
}

// One thread, one token: bytes [a, e) of the text (e > a) against the word of e - a bytes at dword `off` of the blob.
template <class TextLoad, class BlobLoad>
TH_FN bool vt_equal_lane(TextLoad ld, int64_t a, int64_t e, BlobLoad blob, uint32_t off) {
    const int64_t q = a >> 2, last = (e - 1) >> 2;
    const uint32_t sh = (uint32_t)(a & 3), len = (uint32_t)(e - a);
    const int64_t nd = ((e - a) + 3) >> 2;   // dwords of the word, the partial one included
    uint32_t lo = ld(q);
    for (int64_t i = 0; i < nd; ++i) {
        const int64_t qi = q + i + 1;
        const uint32_t hi = ld(qi < last ? qi : last);   // (clamped: only read where a byte of the token lies in it)
        const uint32_t m = i + 1 < nd ? 0xFFFFFFFFu : vt_tail_mask(len);
        if ((th_align(hi, lo, sh) ^ blob((uint64_t)off + (uint64_t)i)) & m) return false;
        lo = hi;
    }
    return true;
}

// A wave, one long token, round r: does dword 64 r + lane of the token differ from the word's?  (false behind the last dword)
TH_FN int64_t vt_wave_rounds(int64_t a, int64_t e) { return ((((e - a) + 3) >> 2) + kThWaveBlocks - 1) / kThWaveBlocks; }
template <class TextLoad, class BlobLoad>
TH_FN bool vt_wave_differs(TextLoad ld, int64_t a, int64_t e, BlobLoad blob, uint32_t off, int64_t r, int lane) {
    const int64_t nd = ((e - a) + 3) >> 2, i = r * kThWaveBlocks + lane;
    if (i >= nd) return false;
    const int64_t q = (a >> 2) + i, last = (e - 1) >> 2;
    const uint32_t m = i + 1 < nd ? 0xFFFFFFFFu : vt_tail_mask((uint32_t)(e - a));
    return ((th_align(ld(q + 1 < last ? q + 1 : last), ld(q), (uint32_t)(a & 3)) ^ blob((uint64_t)off + (uint64_t)i)) & m) != 0u;
}

// The id of the token [a, e) of the text, e > a, whose hash (with the table's seed) is `hash`: the lane form of the lookup.
template <class TextLoad, class SlotLoad, class BlobLoad>
TH_FN int32_t vt_lookup_lane(TextLoad ld, int64_t a, int64_t e, uint32_t hash, SlotLoad slot, BlobLoad blob, uint64_t n_slots, int32_t unk) {
    return vt_probe(slot, n_slots, hash, (uint32_t)(e - a),
                    [ld, a, e, blob](uint32_t off) { return vt_equal_lane(ld, a, e, blob, off); }, unk);
}

// ---- the build: host only ---------------------------------------------------------------------------------------------------
struct VtTable {
    std::vector<VtSlot> slots;
    std::vector<uint32_t> blob;   // at least one dword, so that its address is never NULL
    uint32_t seed = 0;
    int64_t n_words = 0;
};
// bytes of the padded blob of these words (word_off is non-decreasing from 0)
inline uint64_t vt_blob_bytes(const int64_t* word_off, int64_t n_words) {
    uint64_t n = 0;
    for (int64_t i = 0; i < n_words; ++i) n += ((uint64_t)(word_off[i + 1] - word_off[i]) + 3u) & ~3ull;
    return n;
}
// words[word_off[i] : word_off[i+1]] = word i; ids may be NULL (id_i = i).  The caller has checked the offsets and the sizes.
inline void vt_build(const uint8_t* words, const int64_t* word_off, int64_t n_words, const int32_t* ids, uint32_t seed, VtTable* t) {
    const uint64_t n_slots = vt_slot_count(n_words);
    t->seed = seed;
    t->n_words = n_words;
    t->slots.assign(n_slots, VtSlot{0u, 0, 0u, kVtEmpty});
    t->blob.assign(vt_blob_bytes(word_off, n_words) / 4 + 1, 0u);
    uint8_t* bytes = reinterpret_cast<uint8_t*>(t->blob.data());
    const uint32_t* blob = t->blob.data();
    auto ld = [blob](uint64_t i) { return blob[i]; };
    uint64_t at = 0;   // next free dword of the blob
    for (int64_t i = 0; i < n_words; ++i) {
        const uint64_t len = (uint64_t)(word_off[i + 1] - word_off[i]);
        if (len == 0) continue;
        for (uint64_t b = 0; b < len; ++b) bytes[4 * at + b] = words[word_off[i] + (int64_t)b];
        const int64_t a = (int64_t)(4 * at), e = a + (int64_t)len;
        const uint32_t h = th_hash_lane([blob](int64_t k) { return blob[k]; }, a, e, seed);
        const uint64_t mask = n_slots - 1;
        uint64_t s = h & mask;
        bool dup = false;
        while (t->slots[s].len != kVtEmpty) {   // (ends: at most n_words <= n_slots / 2 slots are taken)
            const VtSlot& v = t->slots[s];
            if (v.hash == h && v.len == (uint32_t)len && vt_equal_lane([blob](int64_t k) { return blob[k]; }, a, e, ld, v.off)) {
                dup = true;
                break;
            }
            s = (s + 1) & mask;
        }
        if (dup) {   // the first occurrence wins: take the copy back
            for (uint64_t b = 0; b < len; ++b) bytes[4 * at + b] = 0;
            continue;
        }
        t->slots[s] = VtSlot{h, ids ? ids[i] : (int32_t)i, (uint32_t)at, (uint32_t)len};
        at += (len + 3) >> 2;
    }
}

#endif
