// term_key.h -- the per-token key of the term-count calls (compact_kernels.hip: TermTokens of scatter_block writes it at the
// token's rank, terms_kernels.hip sorts and reduces it).  Plain C++17, like token_hash.h: it compiles on the host
// (tests/helpers/term_key_harness.cpp runs it against a Python restatement of the rule) and, under hipcc, on the device.
//
//   the key      one 64-bit word per token, sortable as an unsigned integer without a second look at the text:
//                  bit  0        the token's value is -1 (hashed form with alternate_sign and h < 0), else +1
//                  bits 1 .. 32  the column, order-preserving: the vocabulary id with its sign bit flipped (ascending unsigned =
//                                ascending signed int32), or the hash bucket (< 2^31)
//                  bit  33       the token is out of vocabulary: it sorts behind every found token of its row, whatever the ids
//                                are -- "not found" is a bit of its own, no int32 is taken from the ids
//                tokens of one column differ in bit 0 at most, so the entry of a key is key >> 1.
//   hashed form  column = |h| mod n_features in 64 bits (h = -2^31 gives 2^31 mod n_features: scikit-learn's _hashing_fast.pyx),
//                value = h >= 0 ? +1 : -1 with alternate_sign, else +1.  n_features is 1 .. 2^31 - 1 (the caller checks).
#ifndef LATOK_TERM_KEY_H
#define LATOK_TERM_KEY_H
#include <stdint.h>

#include "vocab_table.h"

constexpr int kTkColumnShift = 1, kTkOovShift = 33, kTkKeyBits = 34;
constexpr uint64_t kTkOov = 1ull << kTkOovShift;   // the key of every out-of-vocabulary token

TH_FN uint32_t tk_bucket(int32_t h, uint32_t n_features) {
    const int64_t a = h < 0 ? -(int64_t)h : (int64_t)h;
    return (uint32_t)(a % (int64_t)n_features);
}
TH_FN uint64_t tk_hashed_key(uint32_t hash, uint32_t n_features, bool alternate_sign) {
    const int32_t h = (int32_t)hash;
    return ((uint64_t)tk_bucket(h, n_features) << kTkColumnShift) | (uint64_t)(alternate_sign && h < 0);
}
TH_FN uint64_t tk_vocab_key(int32_t id) { return (uint64_t)((uint32_t)id ^ 0x80000000u) << kTkColumnShift; }

TH_FN bool tk_is_oov(uint64_t key) { return (key >> kTkOovShift) & 1ull; }
TH_FN int32_t tk_value(uint64_t key) { return (key & 1ull) ? -1 : 1; }
TH_FN int32_t tk_hashed_column(uint64_t key) { return (int32_t)(uint32_t)(key >> kTkColumnShift); }
TH_FN int32_t tk_vocab_column(uint64_t key) { return (int32_t)((uint32_t)(key >> kTkColumnShift) ^ 0x80000000u); }

// vt_probe with the key in the id's place: the found word's key, or kTkOov.
template <class SlotLoad, class Equal>
TH_FN uint64_t tk_vocab_probe(SlotLoad slot, uint64_t n_slots, uint32_t hash, uint32_t len, Equal equal) {
    const uint64_t mask = n_slots - 1;
    uint64_t s = hash & mask;
    for (uint64_t step = 0; step < n_slots; ++step) {   // (bounded here, as in vt_probe)
        const VtSlot v = slot(s);
        if (v.len == kVtEmpty) return kTkOov;
        if (v.hash == hash && v.len == len && equal(v.off)) return tk_vocab_key(v.id);
        s = (s + 1) & mask;
    }
    return kTkOov;
}

#endif
