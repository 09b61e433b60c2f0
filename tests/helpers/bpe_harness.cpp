// Host harness of latok_amd/csrc/bpe.h (tests/test_bpe_host.py): the build of the table and the cut -- bpe_whole, then bpe_merge, the
// function the count kernel and the emit kernel instantiate -- run by g++ on tokens inside a poisoned buffer.  A token of at most
// kBpeLaneBytes bytes is walked on BpeLaneState, the state of the kernels' lane form (the ranks in an array instead of an LDS column),
// and every token on a wide state of the harness's own (64 start words and 4096 ranks, what the wave form keeps across its lanes):
// the two must agree.
//   stdin:  poison(hex byte), then commands, one per line:
//             V <seed hex> <max_bytes> <n_words>   a new vocabulary; n_words lines follow:
//                                                 <id, or '-' for the default> <word as hex, '-' = empty>
//             F                                   damage the table: every slot occupied, with a hash no probe asks for
//             T <pad> <unk> <token hex>           a token; pad = bytes in front of it (its start alignment); the buffer ends with the
//                                                 aligned dword of the token's last byte
//   stdout: per V:  "slots <n> used <n> max <longest word>"
//           per T:  "<n> <id>:<start>:<end> ... <lookups> <merges> <slot loads>"  (positions inside the token; the three counters are
//                   those of ONE cut on the wide state: lookups asked of bpe_look, the whole-token one and one per part included)
//   exit 2 if a text load left the token's dwords, 3 if a table or blob load left the table, 4 if the two states disagree
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "bpe.h"

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
    int a, e;
    bool operator==(const Piece& o) const { return id == o.id && a == o.a && e == o.e; }
};

struct ArrayRanks {
    uint32_t* p;
    uint32_t get(int i) const { return p[i]; }
    void set(int i, uint32_t r) const { p[i] = r; }
};

// the wide state: what the wave form holds, by one thread
template <class Look>
struct WideState {
    Look look;
    std::vector<uint64_t> bits = std::vector<uint64_t>(kBpeMaxBytes / 64, 0ull);
    std::vector<uint32_t> ranks = std::vector<uint32_t>(kBpeMaxBytes, 0xDEADBEEFu);
    explicit WideState(Look l) : look(l) {}
    void fill(int L) {
        for (int i = 0; i < L; ++i) {
            bits[(size_t)(i >> 6)] |= 1ull << (i & 63);
            ranks[(size_t)i] = i + 2 <= L ? look(i, i + 2) : kBpeAbsent;
        }
    }
    int argmin(int L, uint32_t* r) const {
        uint32_t best = kBpeAbsent;
        int at = 0;
        for (int i = 0; i < L; ++i)
            if (ranks[(size_t)i] < best) {
                best = ranks[(size_t)i];
                at = i;
            }
        *r = best;
        return at;
    }
    bool is_start(int i) const { return (bits[(size_t)(i >> 6)] >> (i & 63)) & 1ull; }
    int start_next(int i, int L) const {
        for (int j = i + 1; j < L; ++j)
            if (is_start(j)) return j;
        return L;
    }
    int start_prev(int i) const {
        for (int j = i - 1; j > 0; --j)
            if (is_start(j)) return j;
        return 0;
    }
    void start_clear(int j) { bits[(size_t)(j >> 6)] &= ~(1ull << (j & 63)); }
    void set_rank(int i, uint32_t r) { ranks[(size_t)i] = r; }
    void look2(int h, int k, int i, int q, uint32_t* rl, uint32_t* rr) const {
        *rl = h >= 0 ? look(h, k) : kBpeAbsent;
        *rr = q > k ? look(i, q) : kBpeAbsent;
    }
};

int main() {
    unsigned poison = 0;
    if (scanf("%x", &poison) != 1) return 1;
    static char tok[1 << 16], hex[1 << 16];
    BpeTables t;
    int max_bytes = kBpeMaxBytes;
    uint32_t seed = 0;
    int64_t n_words_now = 0;
    bpe_build(nullptr, std::vector<int64_t>{0}.data(), 0, nullptr, 0, &t);
    while (scanf(" %65535s", tok) == 1) {
        if (tok[0] == 'V') {
            long n_words;
            if (scanf("%x %d %ld", &seed, &max_bytes, &n_words) != 3) return 1;
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
            bpe_build(words.data(), off.data(), n_words, any_id ? ids.data() : nullptr, seed, &t);
            n_words_now = n_words;
            size_t used = 0;
            for (const VtSlot& s : t.table.slots) used += s.len != kVtEmpty;
            printf("slots %zu used %zu max %u\n", t.table.slots.size(), used, t.max_len);
            continue;
        }
        if (tok[0] == 'F') {
            for (VtSlot& s : t.table.slots)
                if (s.len == kVtEmpty) s = VtSlot{0u, -99, 0u, 0u};
            for (VtSlot& s : t.table.slots) s.hash ^= 0x5a5a5a5au;
            continue;
        }
        long pad, unk;
        if (scanf("%ld %ld %65535s", &pad, &unk, hex) != 3) return 1;
        const std::vector<uint8_t> data = unhex(hex);
        const size_t n = data.size();
        if (n == 0) return 1;   // (no token is empty)
        const int64_t a = pad, e = pad + (int64_t)n;
        const int L = (int)n;
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
        long loads = 0, lookups = 0;
        const VtTable* tp = &t.table;
        const auto tab = wp_table_view(
            [tp, &loads](uint64_t i) -> VtSlot {
                ++loads;
                if (i >= tp->slots.size()) { g_bad |= 3; return VtSlot{0u, 0, 0u, kVtEmpty}; }
                return tp->slots[i];
            },
            [tp](uint64_t i) -> uint32_t {
                if (i >= tp->blob.size()) { g_bad |= 3; return 0xDEADBEEFu; }
                return tp->blob[i];
            },
            (uint64_t)tp->slots.size(), t.max_len);
        const uint32_t sd = seed;
        auto look = [&](int i, int k) -> uint32_t {
            ++lookups;
            return bpe_look(ld, a + i, a + k, tab, sd);
        };
        const std::vector<int32_t>& rank_id = t.rank_id;
        const int64_t nw = n_words_now;
        auto id_of = [&rank_id, nw, unk](uint32_t r) { return (int64_t)r < nw ? rank_id[(size_t)r] : (int32_t)unk; };
        // one cut on a state made by make(): the whole-token step, the walk, one lookup per part
        auto cut = [&](auto make, int* n_merges) {
            std::vector<Piece> out;
            uint32_t r;
            if (L <= max_bytes) ++lookups;   // (bpe_whole asks bpe_look once, unless the token is longer than max_bytes)
            *n_merges = 0;
            if (bpe_whole(ld, a, e, tab, sd, max_bytes, &r)) {
                out.push_back(Piece{id_of(r), 0, L});
                return out;
            }
            auto s = make();
            const int parts = bpe_merge(L, s);
            *n_merges = L - parts;
            for (int i = 0; i < L;) {
                const int k = s.start_next(i, L);
                out.push_back(Piece{id_of(look(i, k)), i, k});
                i = k;
            }
            if ((int)out.size() != parts) g_bad |= 4;
            return out;
        };
        int m_wide = 0, m_lane = 0;
        const std::vector<Piece> wide = cut([&] { return WideState<decltype(look)>(look); }, &m_wide);
        const long wide_lookups = lookups, wide_loads = loads;
        if (L <= kBpeLaneBytes) {
            uint32_t column[kBpeLaneBytes];
            for (uint32_t& c : column) c = 0xDEADBEEFu;
            const std::vector<Piece> lane = cut([&] { return bpe_lane_state(ArrayRanks{column}, look); }, &m_lane);
            if (!(lane == wide) || m_lane != m_wide || lookups != 2 * wide_lookups) return 4;
        }
        printf("%zu", wide.size());
        for (const Piece& q : wide) printf(" %d:%d:%d", q.id, q.a, q.e);
        printf(" %ld %d %ld\n", wide_lookups, m_wide, wide_loads);
    }
    return g_bad;
}
