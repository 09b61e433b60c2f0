// Host harness of latok_amd/csrc/unigram.h (tests/test_unigram_host.py): the build of the two tables and the cut -- uni_forward and
// uni_backtrack, the functions the count kernel and the emit kernel instantiate -- run by g++ on tokens inside a poisoned buffer.  A
// token of at most kUniLaneBytes bytes is walked on UniLaneState, the state of the kernels' lane form (best / back in arrays instead of
// LDS columns, the result in the three mask words), and every token on a wide state of the harness's own (arrays over all nodes and one
// piece record per start node): the two must agree.  The wide state is a restatement by one thread, NOT UniWaveState of
// unigram_kernels.hip: the device's wave state (64 candidate ends per step, the ballot numbering of the records, the LDS slices) is held
// to the reference by tests/test_gpu_unigram.py alone (tokens of 65, 130 and 4096 bytes, long and short tokens in one wave).
//   stdin:  poison(hex byte), then commands, one per line:
//             V <seed hex> <max_bytes> <fuse_unk> <unk_score: float32 bits, hex> <marker hex, '-' = empty> <n_words>
//                                                 a new vocabulary; n_words lines follow:
//                                                 <id, or '-' for the default> <score: float32 bits, hex> <word as hex, '-' = empty>
//             F                                   damage the tables: every slot occupied, with a hash no probe asks for
//             T <pad> <unk> <marked> <token hex>  a token; pad = bytes in front of it (its start alignment); the buffer ends with the
//                                                 aligned dword of the token's last byte
//   stdout: per V:  "slots <plain> <marked> used <plain> <marked> max <longest word of either table> marker <position or -1>"
//           per T:  "<n> <id>:<start>:<end> ... <lookups> <bound> <emit lookups> <slot loads>"  (byte positions inside the token;
//                   lookups: those of ONE forward pass on the wide state; bound: the pairs of positions within the longest word's
//                   reach, counted by the harness itself; emit lookups: one per piece that is a word)
//   exit 2 if a text load left the token's dwords, 3 if a table or blob load left the table, 4 if the two states disagree, 5 if a pass
//   looked one (start, end) pair up twice
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <set>
#include <string>
#include <utility>
#include <vector>

#include "unigram.h"

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
static float bits_float(unsigned bits) {
    const uint32_t b = (uint32_t)bits;
    float f;
    memcpy(&f, &b, 4);
    return f;
}

struct Piece {
    int32_t id;
    int a, e;
    bool operator==(const Piece& o) const { return id == o.id && a == o.a && e == o.e; }
};

struct ArrayCols {
    float* b;
    uint32_t* k;
    float best(int v) const { return b[v]; }
    void set_best(int v, float x) const { b[v] = x; }
    uint32_t back(int v) const { return k[v]; }
    void set_back(int v, uint32_t x) const { k[v] = x; }
};

// the wide state: the same two passes over plain arrays, by one thread (the harness's own; see the head of the file)
template <class Look, class Score, class IsPos>
struct WideState {
    Look look;
    Score score;
    IsPos is_pos;   // node j, 0 < j < N
    float unk_score;
    std::vector<float> best = std::vector<float>(kUniMaxBytes + 2, -12345.0f);
    std::vector<uint32_t> back = std::vector<uint32_t>(kUniMaxBytes + 2, 0xDEADBEEFu);
    std::vector<uint32_t> rec = std::vector<uint32_t>(kUniMaxBytes + 2, 0u);
    WideState(Look l, Score s, IsPos p, float u) : look(l), score(s), is_pos(p), unk_score(u) {}
    void begin(int N) {
        for (int v = 0; v <= N; ++v) back[(size_t)v] = kUniUnset;
        best[0] = 0.0f;
        back[0] = 0u;
    }
    int next_pos(int i, int N) const {
        for (int j = i + 1; j < N; ++j)
            if (is_pos(j)) return j;
        return N;
    }
    void update(int j, float cand, uint32_t b) {
        if (back[(size_t)j] == kUniUnset || cand > best[(size_t)j]) {
            best[(size_t)j] = cand;
            back[(size_t)j] = b;
        }
    }
    bool words(int i, int j1, int hi, int N) {
        const float from = best[(size_t)i];
        bool single = false;
        for (int j = j1; j <= hi; ++j) {
            if (j != N && !is_pos(j)) continue;
            const uint32_t w = look(i, j);
            if (w == kUniAbsent) continue;
            update(j, from + score(w), (uint32_t)i);
            single = single || j == j1;
        }
        return single;
    }
    void unknown(int i, int j1) { update(j1, best[(size_t)i] + unk_score, (uint32_t)i | kUniUnkBit); }
    uint32_t back_of(int p) const { return back[(size_t)p]; }
    void part(int i, int p, bool unk, bool joins, int end) {
        rec[(size_t)i] = (uint32_t)end | 0x40000000u | (unk ? kUniUnkBit : 0u);
        if (joins) rec[(size_t)p] = 0u;
    }
};

int main() {
    unsigned poison = 0;
    if (scanf("%x", &poison) != 1) return 1;
    static char tok[1 << 16], hex[1 << 16], mhex[64];
    UniTables t;
    int max_bytes = kUniMaxBytes, fuse = 1, marker_len = 0;
    uint32_t seed = 0;
    float unk_score = -10.0f;
    int64_t n_words_now = 0;
    {
        const int64_t zero = 0;
        uni_build(nullptr, &zero, 0, nullptr, nullptr, nullptr, 0, 0, &t);
    }
    while (scanf(" %65535s", tok) == 1) {
        if (tok[0] == 'V') {
            long n_words;
            unsigned ubits;
            if (scanf("%x %d %d %x %63s %ld", &seed, &max_bytes, &fuse, &ubits, mhex, &n_words) != 6) return 1;
            unk_score = bits_float(ubits);
            const std::vector<uint8_t> marker = unhex(mhex);
            marker_len = (int)marker.size();
            if (!uni_marker_ok(marker.data(), marker_len)) return 1;
            std::vector<uint8_t> words;
            std::vector<int64_t> off{0};
            std::vector<int32_t> ids;
            std::vector<float> scores;
            bool any_id = false, all_id = true;
            for (long i = 0; i < n_words; ++i) {
                char idtxt[32];
                unsigned sbits;
                if (scanf(" %31s %x %65535s", idtxt, &sbits, hex) != 3) return 1;
                if (idtxt[0] == '-' && idtxt[1] == 0) { all_id = false; ids.push_back(0); }
                else { any_id = true; ids.push_back((int32_t)strtol(idtxt, nullptr, 10)); }
                scores.push_back(bits_float(sbits));
                const std::vector<uint8_t> w = unhex(hex);
                words.insert(words.end(), w.begin(), w.end());
                off.push_back((int64_t)words.size());
            }
            if (any_id && !all_id) return 1;
            words.push_back(0);   // (never read: non-NULL pointers for an all-empty vocabulary)
            scores.push_back(0.0f);
            uni_build(words.data(), off.data(), n_words, scores.data(), any_id ? ids.data() : nullptr, marker.data(), marker_len, seed, &t);
            n_words_now = n_words;
            size_t used_p = 0, used_m = 0;
            for (const VtSlot& s : t.plain.slots) used_p += s.len != kVtEmpty;
            for (const VtSlot& s : t.marked.slots) used_m += s.len != kVtEmpty;
            printf("slots %zu %zu used %zu %zu max %u marker %d\n", t.plain.slots.size(), t.marked.slots.size(), used_p, used_m,
                   t.max_len_plain > t.max_len_marked ? t.max_len_plain : t.max_len_marked, t.marker_pos);
            continue;
        }
        if (tok[0] == 'F') {
            for (VtTable* vt : {&t.plain, &t.marked}) {
                for (VtSlot& s : vt->slots)
                    if (s.len == kVtEmpty) s = VtSlot{0u, -99, 0u, 0u};
                for (VtSlot& s : vt->slots) s.hash ^= 0x5a5a5a5au;
            }
            t.marker_pos = -1;
            continue;
        }
        long pad, unk, marked;
        if (scanf("%ld %ld %ld %65535s", &pad, &unk, &marked, hex) != 4) return 1;
        const std::vector<uint8_t> data = unhex(hex);
        const size_t n = data.size();
        if (n == 0) return 1;   // (no token is empty)
        const int64_t a = pad, e = pad + (int64_t)n;
        const int L = (int)n, mk = marked && marker_len > 0 ? 1 : 0, N = L + mk;
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
        if (L > max_bytes) {   // step 1 of the cut needs no state
            printf("1 %ld:0:%d 0 0 0 0\n", unk, L);
            continue;
        }
        long loads = 0, lookups = 0;
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
        const auto tab_p = view(&t.plain, t.max_len_plain);
        const auto tab_m = view(&t.marked, t.max_len_marked);
        const uint32_t sd = seed;
        const int32_t marker_pos = t.marker_pos;
        std::set<std::pair<int, int>> seen;
        auto look = [&](int i, int j) -> uint32_t {
            ++lookups;
            if (!seen.insert(std::make_pair(i, j)).second) g_bad |= 5;
            return uni_look(ld, a, mk, i, j, tab_p, tab_m, marker_pos, sd);
        };
        const std::vector<float>& pos_score = t.pos_score;
        const std::vector<int32_t>& pos_id = t.pos_id;
        const int64_t nw = n_words_now;
        auto score = [&pos_score, nw](uint32_t w) { return (int64_t)w < nw ? pos_score[(size_t)w] : 0.0f; };
        auto id_of = [&pos_id, nw, unk](uint32_t w) { return (int64_t)w < nw ? pos_id[(size_t)w] : (int32_t)unk; };
        auto is_pos = [&](int j) { return !wp_is_cont(wp_byte(ld, a + (j - mk))); };
        const int reach = (int)t.max_len_plain, reach0 = mk ? (int)t.max_len_marked + 1 : reach;
        // the bound, counted here: the pairs of positions i < j with j - i within the reach of i
        long bound = 0;
        for (int i = 0; i < N; ++i) {
            if (i != 0 && !is_pos(i)) continue;
            for (int j = i + 1; j <= N && j - i <= (i == 0 ? reach0 : reach); ++j) bound += j == N || is_pos(j);
        }
        // one cut on the wide state
        WideState<decltype(look), decltype(score), decltype(is_pos)> ws(look, score, is_pos, unk_score);
        uni_forward(N, reach0, reach, ws);
        const long wide_lookups = lookups, wide_loads = loads;
        for (int v = 0; v <= N; ++v) ws.rec[(size_t)v] = 0u;
        const int n_wide = uni_backtrack(N, fuse, ws);
        std::vector<Piece> wide;
        long emit_lookups = 0;
        for (int i = 0; i < N; ++i) {
            const uint32_t v = ws.rec[(size_t)i];
            if (!(v & 0x40000000u)) continue;
            const int j = (int)(v & kUniStartMask);
            int32_t id = (int32_t)unk;
            if (!(v & kUniUnkBit)) {
                ++emit_lookups;
                id = id_of(uni_look(ld, a, mk, i, j, tab_p, tab_m, marker_pos, sd));
            }
            wide.push_back(Piece{id, (int)uni_span_start(0, mk, i), (int)uni_span_end(0, mk, j)});
        }
        if ((int)wide.size() != n_wide) return 4;
        if (L <= kUniLaneBytes) {
            float bcol[kUniLaneNodes];
            uint32_t kcol[kUniLaneNodes];
            for (float& c : bcol) c = -12345.0f;
            for (uint32_t& c : kcol) c = 0xDEADBEEFu;
            seen.clear();
            uint64_t pos = uni_char_starts(ld, a, L);
            if (!mk) pos |= 1ull;
            auto s = uni_lane_state(ArrayCols{bcol, kcol}, look, score, pos, mk, unk_score);
            uni_forward(N, reach0, reach, s);
            if (lookups != 2 * wide_lookups) return 4;
            const int n_lane = uni_backtrack(N, fuse, s);
            std::vector<Piece> lane;
            const int n_parts = uni_lane_parts(s.starts, s.unks, s.head_unk, L, mk, [&](int, bool is_unk, int i, int j) {
                const int32_t id = is_unk ? (int32_t)unk : id_of(uni_look(ld, a, mk, i, j, tab_p, tab_m, marker_pos, sd));
                lane.push_back(Piece{id, (int)uni_span_start(0, mk, i), (int)uni_span_end(0, mk, j)});
            });
            if (!(lane == wide) || n_lane != n_wide || n_parts != n_wide) return 4;
        }
        printf("%zu", wide.size());
        for (const Piece& q : wide) printf(" %d:%d:%d", q.id, q.a, q.e);
        printf(" %ld %ld %ld %ld\n", wide_lookups, bound, emit_lookups, wide_loads);
    }
    return g_bad;
}
