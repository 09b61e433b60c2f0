// Host harness of latok_amd/csrc/spbpe.h (tests/test_spbpe_host.py): the segment rule in its scalar and its plane form, the virtual text,
// and the cut -- bpe_merge of bpe.h on SpLaneState, the state of the kernels' lane form (the ranks in an array instead of an LDS column),
// and on a wide state of the harness's own (what the wave form keeps across its lanes) -- run by g++ on strings inside a poisoned buffer.
//   stdin:  commands, one per line:
//             V <seed hex> <max_bytes> <dummy> <fuse> <n_words>   a new vocabulary; n_words lines follow: <id, or '-'> <word as hex>
//             Y <256 ids, comma separated, or '-'>                byte ids ('-': no byte fallback)
//             E <pad> <unk> <string as hex, '-' = empty>          one string; `pad` bytes of another string lie in front of it
//             W                                                   is the word list fine?  prints sp_first_bad_word
//   stdout: per V:  "slots <n> used <n> max <longest word>"
//           per E:  "<starts as 0/1, '-' if empty> <n> <id>:<start>:<end> ..."   (positions inside the string)
//   exit 2 if a text load left the segment's dwords, 3 if a table or blob load left the table, 4 if the two states disagree,
//        5 if the plane form of the segment rule disagrees with the scalar walk, 6 if a piece count disagrees with the pieces
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "spbpe.h"

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
    bool operator==(const Piece& o) const { return id == o.id && a == o.a && e == o.e; }
};

struct ArrayRanks {
    uint32_t* p;
    uint32_t get(int i) const { return p[i]; }
    void set(int i, uint32_t r) const { p[i] = r; }
};

// the wide state: what the wave form holds, by one thread.  is_start(v): the virtual position is a character start
template <class Look, class IsStart>
struct WideState {
    Look look;
    IsStart vstart;
    std::vector<uint64_t> bits = std::vector<uint64_t>(kBpeMaxBytes / 64, 0ull);
    std::vector<uint32_t> ranks = std::vector<uint32_t>(kBpeMaxBytes, 0xDEADBEEFu);
    WideState(Look l, IsStart s) : look(l), vstart(s) {}
    void fill(int L) {
        for (int i = 0; i < L; ++i)
            if (vstart(i)) bits[(size_t)(i >> 6)] |= 1ull << (i & 63);
        for (int i = 0; i < L; ++i) {
            ranks[(size_t)i] = kBpeAbsent;
            if (!is_start(i)) continue;
            const int j = start_next(i, L);
            if (j < L) ranks[(size_t)i] = look(i, start_next(j, L));
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

// a window of the plane form over a host buffer: bytes outside it read as 0
struct HostWindow {
    const uint8_t* buf;
    int64_t n, w0;
    uint32_t byte(int i) const {
        const int64_t p = w0 + i;
        return p >= 0 && p < n ? buf[p] : 0u;
    }
    uint64_t qword(int j) const {
        uint64_t x = 0;
        for (int b = 0; b < 8; ++b) x |= (uint64_t)byte(8 * j + b) << (8 * b);
        return x;
    }
};

int main() {
    static char tok[1 << 16], hex[1 << 16];
    BpeTables t;
    int max_bytes = kBpeMaxBytes, dummy = 1, fuse = 0;
    uint32_t seed = 0;
    int64_t n_words_now = 0;
    std::vector<int32_t> byte_ids;
    std::vector<uint8_t> words;
    std::vector<int64_t> off{0};
    bpe_build(nullptr, off.data(), 0, nullptr, 0, &t);
    while (scanf(" %65535s", tok) == 1) {
        if (tok[0] == 'V') {
            long n_words;
            if (scanf("%x %d %d %d %ld", &seed, &max_bytes, &dummy, &fuse, &n_words) != 5) return 1;
            words.clear();
            off.assign(1, 0);
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
        if (tok[0] == 'W') {
            printf("%lld\n", (long long)sp_first_bad_word(words.data(), off.data(), n_words_now));
            continue;
        }
        if (tok[0] == 'Y') {
            if (scanf(" %65535s", hex) != 1) return 1;
            byte_ids.clear();
            if (hex[0] != '-')
                for (char* p = strtok(hex, ","); p; p = strtok(nullptr, ",")) byte_ids.push_back((int32_t)strtol(p, nullptr, 10));
            if (!byte_ids.empty() && byte_ids.size() != 256) return 1;
            continue;
        }
        long pad, unk;
        if (scanf("%ld %ld %65535s", &pad, &unk, hex) != 3) return 1;
        const std::vector<uint8_t> data = unhex(hex);
        const int64_t n = (int64_t)data.size();
        // the buffer: `pad` bytes of another string that ends with a truncated marker (pad even) or with a space (pad odd), the string,
        // poison up to a dword
        static const uint8_t filler[] = {'a', ' ', 0xE2, 0x96, 0x81, ' ', 0xE2, 0x96};
        const int64_t total = pad + n;
        std::vector<uint8_t> buf((size_t)((total + 3) & ~3ll) + 4, (uint8_t)0xAB);
        for (int64_t i = 0; i < pad; ++i) buf[(size_t)i] = filler[(size_t)((i + 8 * pad - pad + ((pad & 1) ? 6 : 0)) % 8)];
        if (n) memcpy(buf.data() + pad, data.data(), (size_t)n);
        // the segment rule: the scalar walk of the string against the plane form over the whole buffer
        std::vector<uint8_t> start((size_t)n + 1, 0);
        sp_starts_scalar(buf.data() + pad, n, start.data());
        for (int64_t w = 0; w * 64 < total; ++w) {
            const HostWindow win{buf.data(), total, w * 64 - kPtHalo};
            pt_u128 B = 0;
            for (int i = 0; i < kPtWindow; ++i) {
                const int64_t p = win.w0 + i;
                if (p == 0 || p == pad || p == total) B |= (pt_u128)1 << i;
            }
            const uint64_t bits = sp_word_starts(win, B);
            for (int i = 0; i < 64; ++i) {
                const int64_t p = w * 64 + i;
                if (p >= pad && p < total && (((bits >> i) & 1ull) != 0ull) != (start[(size_t)(p - pad)] != 0)) g_bad |= 5;
            }
        }
        std::string starts;
        for (int64_t i = 0; i < n; ++i) starts.push_back(start[(size_t)i] ? '1' : '0');
        if (starts.empty()) starts = "-";
        // the cut of every segment
        std::vector<Piece> all;
        const uint8_t* p = buf.data();
        const VtTable* tp = &t.table;
        const auto tab = wp_table_view(
            [tp](uint64_t i) -> VtSlot {
                if (i >= tp->slots.size()) { g_bad |= 3; return VtSlot{0u, 0, 0u, kVtEmpty}; }
                return tp->slots[i];
            },
            [tp](uint64_t i) -> uint32_t {
                if (i >= tp->blob.size()) { g_bad |= 3; return 0xDEADBEEFu; }
                return tp->blob[i];
            },
            (uint64_t)tp->slots.size(), t.max_len);
        const uint32_t sd = seed;
        const std::vector<int32_t>& rank_id = t.rank_id;
        const int64_t nw = n_words_now;
        auto id_of = [&rank_id, nw, unk](uint32_t r) { return (int64_t)r < nw ? rank_id[(size_t)r] : (int32_t)unk; };
        const bool bytes = !byte_ids.empty();
        for (int64_t a = pad; a < total;) {
            int64_t e = a + 1;
            while (e < total && !start[(size_t)(e - pad)]) ++e;
            const int64_t first = a >> 2, last = (e - 1) >> 2;   // the segment's own dwords, no other
            auto ld = [p, first, last](int64_t i) -> uint32_t {
                if (i < first || i > last) { g_bad |= 2; return 0xDEADBEEFu; }
                uint32_t w;
                memcpy(&w, p + 4 * i, 4);
                return w;
            };
            const SpSeg g = sp_segment(ld, a, e, dummy && a == pad ? 1 : 0, max_bytes);
            if (g.over) {
                all.push_back(Piece{(int32_t)unk, a - pad, e - pad});
                a = e;
                continue;
            }
            const int L = (int)g.VL;
            const auto vld = sp_virtual(ld, g);
            auto look = [&](int i, int k) -> uint32_t { return bpe_look(vld, i, k, tab, sd); };
            const int64_t P = g.P;
            auto vstart = [&](int v) { return sp_vstart(vld, P, v); };
            // the pieces of the parts a state left; `next(i)` = the part start behind i
            auto emit = [&](auto& s) {
                std::vector<Piece> out;
                int64_t counted = 0;
                bool run = false;
                for (int i = 0; i < L;) {
                    const int k = s.start_next(i, L);
                    const uint32_t r = look(i, k);
                    const int64_t lo = sp_real(ld, g, i) - pad, hi = sp_real(ld, g, k) - pad;
                    counted += sp_part_pieces(r, k - i, bytes);
                    if (r != kBpeAbsent) {
                        out.push_back(Piece{id_of(r), lo, hi});
                        run = false;
                    } else if (bytes) {
                        for (int v = i; v < k; ++v) out.push_back(Piece{byte_ids[wp_byte(vld, v)], lo, hi});
                    } else if (fuse && run) {
                        out.back().e = hi;
                        --counted;
                    } else {
                        out.push_back(Piece{(int32_t)unk, lo, hi});
                        run = true;
                    }
                    i = k;
                }
                if (counted != (int64_t)out.size()) g_bad |= 6;
                return out;
            };
            WideState<decltype(look), decltype(vstart)> wide(look, vstart);
            bpe_merge(L, wide);
            const std::vector<Piece> pw = emit(wide);
            if (L <= kSpLaneBytes) {
                uint32_t column[kSpLaneBytes];
                for (uint32_t& c : column) c = 0xDEADBEEFu;
                const uint64_t chars = sp_char_mask(vld, P, L);
                for (int v = 0; v < L; ++v)
                    if ((((chars >> v) & 1ull) != 0ull) != vstart(v)) g_bad |= 4;
                auto lane = sp_lane_state(ArrayRanks{column}, look, chars);
                bpe_merge(L, lane);
                if (!(emit(lane) == pw)) g_bad |= 4;
            }
            all.insert(all.end(), pw.begin(), pw.end());
            a = e;
        }
        printf("%s %zu", starts.c_str(), all.size());
        for (const Piece& q : all) printf(" %d:%lld:%lld", q.id, (long long)q.a, (long long)q.e);
        printf("\n");
    }
    return g_bad;
}
