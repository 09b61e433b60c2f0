// Host harness of latok_amd/csrc/vocab_table.h (tests/test_vocab_host.py): the build, the probe loop and both compares of the
// device's vocabulary lookup, run by g++ on tokens inside a poisoned buffer, so that the table layout, the wrap of the probe, its
// bound, the masks and the bounds of the aligned loads are tested without a device.  The hash is token_hash.h's, as in the kernel.
//   stdin:  poison(hex byte), then commands, one per line:
//             V <seed hex> <n_words>          a new vocabulary; n_words lines follow:  <id, or '-' for the default> <word as hex, '-' = empty>
//             F                               damage the table: every slot occupied, with a hash no probe asks for (hash ^ 0x5a5a5a5a)
//             <form> <pad> <unk> <token hex>  a probe: form l = vt_lookup_lane, w = the wave's compare (vt_wave_differs per lane
//                                             and round, any lane differing = unequal); pad = bytes in front of the token (its
//                                             start alignment); the buffer ends with the aligned dword of the token's last byte
//   stdout: per V:      "slots <n_slots> used <occupied slots> blob <dwords>"
//           per probe:  "<id> <slot loads>"
//   exit 2 if a text load left the buffer, 3 if a table or blob load left the table
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "token_hash.h"
#include "vocab_table.h"

static int g_bad = 0;

static std::vector<uint8_t> unhex(const char* hex) {
    std::vector<uint8_t> out;
    if (hex[0] == '-') return out;
    const size_t n = strlen(hex) / 2;
    for (size_t i = 0; i < n; ++i) {
        unsigned v = 0;
        sscanf(hex + 2 * i, "%2x", &v);
        out.push_back((uint8_t)v);
    }
    return out;
}

int main() {
    unsigned poison = 0;
    if (scanf("%x", &poison) != 1) return 1;
    static char tok[1 << 16], hex[1 << 16];
    VtTable t;
    vt_build(nullptr, std::vector<int64_t>{0}.data(), 0, nullptr, 0, &t);
    while (scanf(" %65535s", tok) == 1) {
        if (tok[0] == 'V') {
            unsigned seed;
            long n_words;
            if (scanf("%x %ld", &seed, &n_words) != 2) return 1;
            std::vector<uint8_t> words;
            std::vector<int64_t> off{0};
            std::vector<int32_t> ids;
            bool any_id = false, all_id = true;
            for (long i = 0; i < n_words; ++i) {
                char idtxt[32];
                if (scanf(" %31s %65535s", idtxt, hex) != 2) return 1;
                if (idtxt[0] == '-' && idtxt[1] == 0) { all_id = false; ids.push_back(0); }
                else { any_id = true; ids.push_back((int32_t)strtol(idtxt, nullptr, 10)); }
                const std::vector<uint8_t> w = unhex(hex);
                words.insert(words.end(), w.begin(), w.end());
                off.push_back((int64_t)words.size());
            }
            if (any_id && !all_id) return 1;
            words.push_back(0);   // (never read: a non-NULL pointer for an all-empty vocabulary)
            vt_build(words.data(), off.data(), n_words, any_id ? ids.data() : nullptr, seed, &t);
            size_t used = 0;
            for (const VtSlot& s : t.slots) used += s.len != kVtEmpty;
            printf("slots %zu used %zu blob %zu\n", t.slots.size(), used, t.blob.size());
            continue;
        }
        if (tok[0] == 'F') {
            for (VtSlot& s : t.slots)
                if (s.len == kVtEmpty) s = VtSlot{0u, -99, 0u, 0u};
            for (VtSlot& s : t.slots) s.hash ^= 0x5a5a5a5au;
            continue;
        }
        const char form = tok[0];
        long pad, unk;
        if (scanf("%ld %ld %65535s", &pad, &unk, hex) != 3) return 1;
        const std::vector<uint8_t> data = unhex(hex);
        const size_t n = data.size();
        if (n == 0) return 1;   // (no token is empty)
        const int64_t a = pad, e = pad + (int64_t)n;
        const size_t n_dwords = (size_t)((e - 1) >> 2) + 1;      // up to the dword of the last byte, no further
        std::vector<uint8_t> buf(4 * n_dwords, (uint8_t)poison);
        memcpy(buf.data() + pad, data.data(), n);
        const uint8_t* p = buf.data();
        auto ld = [p, n_dwords](int64_t i) -> uint32_t {
            if (i < 0 || (size_t)i >= n_dwords) { g_bad |= 2; return 0xDEADBEEFu; }
            uint32_t w;
            memcpy(&w, p + 4 * i, 4);
            return w;
        };
        long loads = 0;
        const VtTable* tp = &t;
        auto slot = [tp, &loads](uint64_t i) -> VtSlot {
            ++loads;
            if (i >= tp->slots.size()) { g_bad |= 3; return VtSlot{0u, 0, 0u, kVtEmpty}; }
            return tp->slots[i];
        };
        auto blob = [tp](uint64_t i) -> uint32_t {
            if (i >= tp->blob.size()) { g_bad |= 3; return 0xDEADBEEFu; }
            return tp->blob[i];
        };
        const uint32_t h = th_hash_lane(ld, a, e, t.seed);
        int32_t id;
        if (form == 'l') {
            id = vt_lookup_lane(ld, a, e, h, slot, blob, t.slots.size(), (int32_t)unk);
        } else {
            id = vt_probe(slot, t.slots.size(), h, (uint32_t)(e - a),
                          [&](uint32_t off) {
                              bool differs = false;
                              for (int64_t r = 0; r < vt_wave_rounds(a, e); ++r)
                                  for (int l = 0; l < kThWaveBlocks; ++l) differs |= vt_wave_differs(ld, a, e, blob, off, r, l);
                              return !differs;
                          },
                          (int32_t)unk);
        }
        printf("%d %ld\n", id, loads);
    }
    return g_bad;
}
