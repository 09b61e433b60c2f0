// Host harness of latok_amd/csrc/detok.h (tests/test_detok_host.py): the build of the object and the two passes of a decode call -- the
// lookup, the rule and the look-back per piece (what k_detok_count does), then the form read back from the count and the byte copy in
// stretches of at most `win` bytes (what k_detok_write does) -- run by g++ over a CSR of ids.  The blob is read from an exact-size copy
// whose padding bytes and spare dword are overwritten with the poison byte: a pad byte that reaches the output shows, a load behind the
// blob's last dword ends the run (and trips the address sanitizer).
//   stdin:  poison(hex byte), then commands, one per line:
//             V <mode> <prefix hex, '-' = empty> <sep> <n_words>   a new object; n_words lines follow:
//                                                                  <id, or '-' for the default> <word as hex, '-' = empty>
//             D <win> <n_skip> <skip ids ..> <n_rows> <n_0> <ids of row 0 ..> <n_1> ..   one decode call
//   stdout: per V:  "words <n> ids <distinct> dense <0/1> max <longest word> blob <padded bytes>"
//           per D:  "unknown <n> walks <kept() calls of all look-backs> bytes <total>", then one line per row: its bytes as hex, '-' = empty
//   exit 3 if a blob load left the blob, 4 if a map or entry load left its array, 5 if the two passes disagree
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "detok.h"

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
    DtTable t;
    uint32_t* blob = nullptr;   // the exact-size, poisoned copy
    size_t blob_dwords = 0;
    uint32_t sep = 0;
    char cmd[8];
    while (scanf("%7s", cmd) == 1) {
        if (cmd[0] == 'V') {
            int mode = 0, sep_in = 0;
            long long n_words = 0;
            char pre_hex[64];
            if (scanf("%d %63s %d %lld", &mode, pre_hex, &sep_in, &n_words) != 4) return 1;
            const std::vector<uint8_t> prefix = unhex(pre_hex);
            sep = (uint32_t)sep_in;
            std::vector<uint8_t> words;
            std::vector<int64_t> off(1, 0);
            std::vector<int32_t> ids;
            bool have_ids = false;
            for (long long i = 0; i < n_words; ++i) {
                static char id_s[64], hex[1 << 20];
                if (scanf("%63s %1048575s", id_s, hex) != 2) return 1;
                have_ids |= id_s[0] != '-' || id_s[1] != 0;
                ids.push_back(id_s[0] == '-' && id_s[1] == 0 ? (int32_t)i : (int32_t)atoll(id_s));
                const std::vector<uint8_t> w = unhex(hex);
                words.insert(words.end(), w.begin(), w.end());
                off.push_back((int64_t)words.size());
            }
            words.push_back(0);   // (never NULL)
            dt_build(words.data(), off.data(), (int64_t)n_words, have_ids ? ids.data() : nullptr, mode, prefix.data(), (int)prefix.size(), &t);
            free(blob);
            blob_dwords = t.blob.size();
            blob = (uint32_t*)malloc(blob_dwords * 4);
            memset(blob, (int)poison, blob_dwords * 4);
            for (long long i = 0; i < n_words; ++i) {
                const DtEntry& e = t.entries[(size_t)i];
                memcpy((uint8_t*)blob + e.off, (const uint8_t*)t.blob.data() + e.off, e.len);
            }
            printf("words %lld ids %lld dense %d max %u blob %llu\n", (long long)t.n_words, (long long)t.n_ids, t.map.dense, t.max_len,
                   (unsigned long long)t.blob_bytes);
        } else if (cmd[0] == 'D') {
            long long win = 0, n_rows = 0;
            int n_skip = 0;
            int32_t skip[kDtMaxSkip] = {0};
            if (scanf("%lld %d", &win, &n_skip) != 2 || n_skip < 0 || n_skip > kDtMaxSkip || win < 1) return 1;
            for (int i = 0; i < n_skip; ++i) {
                long long v;
                if (scanf("%lld", &v) != 1) return 1;
                skip[i] = (int32_t)v;
            }
            if (scanf("%lld", &n_rows) != 1) return 1;
            std::vector<int64_t> row_start(1, 0);
            std::vector<int32_t> ids;
            for (long long r = 0; r < n_rows; ++r) {
                long long n;
                if (scanf("%lld", &n) != 1) return 1;
                for (long long i = 0; i < n; ++i) {
                    long long v;
                    if (scanf("%lld", &v) != 1) return 1;
                    ids.push_back((int32_t)v);
                }
                row_start.push_back((int64_t)ids.size());
            }
            const size_t n_keys = t.keys.size(), n_vals = t.vals.size(), n_ent = t.entries.size();
            auto key = [&](int64_t i) {
                if (i < 0 || (size_t)i >= n_keys) exit(4);
                return t.keys[(size_t)i];
            };
            auto val = [&](int64_t i) {
                if (i < 0 || (size_t)i >= n_vals) exit(4);
                return t.vals[(size_t)i];
            };
            auto entry_of = [&](int32_t id, bool* unknown) -> int32_t {
                *unknown = false;
                if (dt_skipped(skip, n_skip, id)) return -1;
                const int32_t e = dt_lookup(t.map, key, val, id);
                *unknown = e < 0;
                if (e >= 0 && (size_t)e >= n_ent) exit(4);
                return e;
            };
            auto ld = [&](uint64_t i) {
                if (i >= blob_dwords) exit(3);
                return blob[i];
            };
            // pass 1: the bytes of every piece
            long long unknown = 0, walks = 0;
            std::vector<uint32_t> cnt(ids.size(), 0u);
            std::vector<uint64_t> start(ids.size() + 1, 0u);
            for (long long r = 0; r < n_rows; ++r)
                for (int64_t p = row_start[(size_t)r]; p < row_start[(size_t)r + 1]; ++p) {
                    bool unk;
                    const int32_t e = entry_of(ids[(size_t)p], &unk);
                    unknown += unk;
                    if (e < 0) continue;
                    const DtEntry& rec = t.entries[(size_t)e];
                    bool has_prev = false;
                    if (dt_needs_prev(rec, t.mode))
                        has_prev = dt_has_prev(p, row_start[(size_t)r], [&](int64_t u) {
                            bool unk2;
                            ++walks;
                            return entry_of(ids[(size_t)u], &unk2) >= 0;
                        });
                    cnt[(size_t)p] = dt_piece_bytes(dt_piece(rec, t.mode, has_prev));
                }
            for (size_t p = 0; p < ids.size(); ++p) start[p + 1] = start[p] + cnt[p];
            // pass 2: the form from the count, the copy in stretches
            std::vector<uint8_t> out((size_t)start[ids.size()] + 1, (uint8_t)~poison);
            for (size_t p = 0; p < ids.size(); ++p) {
                if (cnt[p] == 0u) continue;
                bool unk;
                const int32_t e = entry_of(ids[p], &unk);
                if (e < 0) return 5;
                const DtPiece pc = dt_piece_of_count(t.entries[(size_t)e], cnt[p]);
                if (dt_piece_bytes(pc) != cnt[p]) return 5;
                // (the first stretch ends where a window of `win` bytes that starts at output byte 0 would end)
                uint64_t k0 = 0;
                while (k0 < cnt[p]) {
                    const uint64_t room = (uint64_t)win - (start[p] + k0) % (uint64_t)win;
                    const uint64_t k1 = k0 + room < cnt[p] ? k0 + room : cnt[p];
                    dt_copy(pc, sep, ld, k0, k1, [&](uint64_t k, uint32_t b) { out[(size_t)(start[p] + k)] = (uint8_t)b; });
                    k0 = k1;
                }
            }
            printf("unknown %lld walks %lld bytes %llu\n", unknown, walks, (unsigned long long)start[ids.size()]);
            for (long long r = 0; r < n_rows; ++r) {
                const uint64_t a = start[(size_t)row_start[(size_t)r]], e = start[(size_t)row_start[(size_t)r + 1]];
                if (a == e) printf("-");
                for (uint64_t i = a; i < e; ++i) printf("%02x", out[(size_t)i]);
                printf("\n");
            }
        } else {
            return 1;
        }
    }
    free(blob);
    return 0;
}
