// Host harness of latok_amd/csrc/wordpiece.h (tests/test_wordpiece_host.py): the build of the two tables and wp_walk, the function
// the count kernel and the emit kernel instantiate, run by g++ on tokens inside a poisoned buffer.  Every token is walked twice, as
// on the device: once counting, once emitting under the consumer's contract (piece 0 kept back, a piece k >= 1 taken only below
// the count) -- the two must agree.
//   stdin:  poison(hex byte), then commands, one per line:
//             V <seed hex> <prefix hex, '-' = empty> <max_chars> <n_words>   a new vocabulary; n_words lines follow:
//                                                 <id, or '-' for the default> <word as hex, '-' = empty>
//             F                                   damage both tables: every slot occupied, with a hash no probe asks for
//             T <pad> <unk> <token hex>           a token; pad = bytes in front of it (its start alignment); the buffer ends with the
//                                                 aligned dword of the token's last byte
//   stdout: per V:  "slots <initial> <cont> used <initial> <cont> max <initial> <cont>"
//           per T:  "<n> <id>:<start>:<end> ..."  (positions inside the token) and, last, the slot loads of both walks together
//   exit 2 if a text load left the token's dwords, 3 if a table or blob load left the table, 4 if the two walks disagree
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "wordpiece.h"

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

struct Piece {
    int32_t id;
    int64_t a, e;
};

int main() {
    unsigned poison = 0;
    if (scanf("%x", &poison) != 1) return 1;
    static char tok[1 << 16], hex[1 << 16], pre[64];
    WpTables t;
    int max_chars = 100;
    uint32_t seed = 0;
    wp_build(nullptr, std::vector<int64_t>{0}.data(), 0, nullptr, nullptr, 0, 0, &t);
    while (scanf(" %65535s", tok) == 1) {
        if (tok[0] == 'V') {
            long n_words;
            if (scanf("%x %63s %d %ld", &seed, pre, &max_chars, &n_words) != 4) return 1;
            const std::vector<uint8_t> prefix = unhex(pre);
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
            wp_build(words.data(), off.data(), n_words, any_id ? ids.data() : nullptr, prefix.data(), (int)prefix.size(), seed, &t);
            size_t used0 = 0, used1 = 0;
            for (const VtSlot& s : t.initial.slots) used0 += s.len != kVtEmpty;
            for (const VtSlot& s : t.cont.slots) used1 += s.len != kVtEmpty;
            printf("slots %zu %zu used %zu %zu max %u %u\n", t.initial.slots.size(), t.cont.slots.size(), used0, used1, t.max_len0, t.max_len1);
            continue;
        }
        if (tok[0] == 'F') {
            for (VtTable* vt : {&t.initial, &t.cont}) {
                for (VtSlot& s : vt->slots)
                    if (s.len == kVtEmpty) s = VtSlot{0u, -99, 0u, 0u};
                for (VtSlot& s : vt->slots) s.hash ^= 0x5a5a5a5au;
            }
            continue;
        }
        long pad, unk;
        if (scanf("%ld %ld %65535s", &pad, &unk, hex) != 3) return 1;
        const std::vector<uint8_t> data = unhex(hex);
        const size_t n = data.size();
        if (n == 0) return 1;   // (no token is empty)
        const int64_t a = pad, e = pad + (int64_t)n;
        const size_t first = (size_t)(a >> 2), n_dwords = (size_t)((e - 1) >> 2) + 1;   // the token's own dwords, no other
        std::vector<uint8_t> buf(4 * n_dwords, (uint8_t)poison);
        memcpy(buf.data() + pad, data.data(), n);
        const uint8_t* p = buf.data();
        auto ld = [p, first, n_dwords](int64_t i) -> uint32_t {
            if (i < (int64_t)first || (size_t)i >= n_dwords) { g_bad |= 2; return 0xDEADBEEFu; }
            uint32_t w;
            memcpy(&w, p + 4 * i, 4);
            return w;
        };
        long loads = 0;
        auto view = [&loads](const VtTable* tp, uint32_t max_len) {
            return wp_table_view(
                [tp, &loads](uint64_t i) -> VtSlot {
                    ++loads;
                    if (i >= tp->slots.size()) { g_bad |= 3; return VtSlot{0u, 0, 0u, kVtEmpty}; }
                    return tp->slots[i];
                },
                [tp](uint64_t i) -> uint32_t {
                    if (i >= tp->blob.size()) { g_bad |= 3; return 0xDEADBEEFu; }
                    return tp->blob[i];
                },
                (uint64_t)tp->slots.size(), max_len);
        };
        const auto tab0 = view(&t.initial, t.max_len0), tab1 = view(&t.cont, t.max_len1);
        const int count = wp_walk(ld, a, e, tab0, tab1, seed, max_chars, (int32_t)unk, [](int, int32_t, int64_t, int64_t) {});
        std::vector<Piece> got((size_t)count, Piece{0, -1, -1});
        Piece first_piece{0, -1, -1};
        const int again = wp_walk(ld, a, e, tab0, tab1, seed, max_chars, (int32_t)unk, [&](int k, int32_t id, int64_t s, int64_t q) {
            if (k == 0) first_piece = Piece{id, s, q};
            else if (k < count) got[(size_t)k] = Piece{id, s, q};
        });
        if (again != count || count < 1) return 4;
        got[0] = first_piece;
        printf("%d", count);
        for (const Piece& q : got) printf(" %d:%lld:%lld", q.id, (long long)(q.a - a), (long long)(q.e - a));
        printf(" %ld\n", loads);
    }
    return g_bad;
}
