// pretok_cl100k_harness.cpp -- the cl100k part of pretok.h on the host, as a stand-alone program (tests/test_pretok_cl100k_host.py builds
// it plain and with sanitizers).
// stdin:  "P <words per tile> <records per walk step>" sets the geometry of the model (1 .. 64 each; the device has 64 and 64);
//         batches, each "B <n>" followed by n lines of hex bytes ("-": the empty string).
// stdout: per string one line with the byte offsets at which a pre-token starts ("-": none).
// Every batch is cut twice: string by string by pt_cl100k_starts_scalar, and by a model of the device scheme over the packed batch:
//   word records (pt_cl100k_record)  ->  one record per tile (pt_rec_left / pt_rec_right over the "ballots" of the tile's words)
//   ->  per tile the walk over tile records, a step's worth at a time, backwards and forwards  ->  per word its carries from the tile's
//   and the words' records  ->  pt_cl100k_finish.
// Exit status 3 when the two disagree.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "pretok.h"
#define PRETOK_TABLE static const
#include "pretok_tables.inc"

struct HostWindow {
    uint8_t b[kPtWindow];
    uint64_t qword(int j) const {
        uint64_t v;
        memcpy(&v, b + 8 * j, 8);
        return v;
    }
    uint32_t byte(int i) const { return b[i]; }
};

static std::vector<uint8_t> unhex(const char* s) {
    std::vector<uint8_t> out;
    if (s[0] == '-') return out;
    for (; s[0] && s[1] && s[0] != '\n'; s += 2) {
        unsigned v = 0;
        sscanf(s, "%2x", &v);
        out.push_back((uint8_t)v);
    }
    return out;
}

// the nine "ballot" words of up to 64 records
static void ballots(const uint32_t* rec, int n, uint64_t* K) {
    for (int b = 0; b < kPtRecBits; ++b) K[b] = 0;
    for (int j = 0; j < n; ++j)
        for (int b = 0; b < kPtRecBits; ++b) K[b] |= (uint64_t)((rec[j] >> b) & 1u) << j;
}
static uint64_t low_bits(int n) { return n >= 64 ? ~0ull : (1ull << n) - 1ull; }

int main() {
    const PretokTables T{kPretokStage1, kPretokStage2, PRETOK_TABLE_LIMIT};
    std::vector<char> buf(1 << 22);
    int64_t wpt = 64, step = 64;
    while (fgets(buf.data(), (int)buf.size(), stdin)) {
        if (buf[0] == 'P') {
            long a = 0, b = 0;
            if (sscanf(buf.data() + 1, "%ld %ld", &a, &b) != 2 || a < 1 || a > 64 || b < 1 || b > 64) return 2;
            wpt = a;
            step = b;
            continue;
        }
        if (buf[0] != 'B') continue;
        const long n_str = atol(buf.data() + 2);
        std::vector<uint8_t> text;
        std::vector<int64_t> off{0};
        for (long s = 0; s < n_str; ++s) {
            if (!fgets(buf.data(), (int)buf.size(), stdin)) return 2;
            const std::vector<uint8_t> one = unhex(buf.data());
            text.insert(text.end(), one.begin(), one.end());
            off.push_back((int64_t)text.size());
        }
        const int64_t total = (int64_t)text.size();
        // the scalar walk, string by string (each string in an allocation of its own size: a read past it is the sanitizer's)
        std::vector<uint8_t> want((size_t)total);
        for (long s = 0; s < n_str; ++s) {
            const int64_t n = off[s + 1] - off[s];
            std::vector<uint8_t> str(text.begin() + off[s], text.begin() + off[s + 1]), cls((size_t)n), st((size_t)n);
            pt_cl100k_starts_scalar(str.data(), n, T, cls.data(), st.data());
            for (int64_t i = 0; i < n; ++i) want[(size_t)(off[s] + i)] = st[(size_t)i];
        }
        // the model of the device scheme
        std::vector<uint8_t> is_first((size_t)total + 1, 0);
        for (long s = 0; s <= n_str; ++s) is_first[(size_t)off[s]] = 1;
        const int64_t n_words = (total + kPtWord - 1) / kPtWord, n_tiles = (n_words + wpt - 1) / wpt;
        std::vector<PtCl> planes((size_t)n_words);
        std::vector<uint32_t> wrec((size_t)(n_tiles * wpt), kPtRecZero), trec((size_t)n_tiles);
        for (int64_t w = 0; w < n_words; ++w) {
            HostWindow win;
            pt_u128 B = 0;
            for (int i = 0; i < kPtWindow; ++i) {
                const int64_t p = w * kPtWord - kPtHalo + i;
                win.b[i] = p >= 0 && p < total ? text[(size_t)p] : 0;
                if (p >= 0 && p <= total && is_first[(size_t)p]) B |= (pt_u128)1 << i;
            }
            pt_cl100k_prepare(win, B, T, planes[(size_t)w]);
            wrec[(size_t)w] = pt_cl100k_record(planes[(size_t)w]);
        }
        uint64_t K[kPtRecBits];
        for (int64_t t = 0; t < n_tiles; ++t) {                  // "launch A"
            ballots(&wrec[(size_t)(t * wpt)], (int)wpt, K);
            trec[(size_t)t] = (pt_rec_left(K, low_bits((int)wpt)) & 0x7Fu) | (pt_rec_right(K, low_bits((int)wpt)) & 0x180u);
        }
        for (int64_t t = 0; t < n_tiles; ++t) {                  // "launch B"
            std::vector<uint32_t> grp((size_t)step);
            uint32_t in = kPtRecPass;
            for (int64_t base = t - step; in & 0x54u; base -= step) {      // backwards
                for (int64_t j = 0; j < step; ++j) grp[(size_t)j] = base + j >= 0 ? trec[(size_t)(base + j)] : kPtRecZero;
                ballots(grp.data(), (int)step, K);
                in = (pt_rec_then(pt_rec_left(K, low_bits((int)step)), in) & 0x7Fu) | (in & 0x180u);
            }
            for (int64_t base = t + 1; in & 0x100u; base += step) {        // forwards
                for (int64_t j = 0; j < step; ++j) grp[(size_t)j] = base + j < n_tiles ? trec[(size_t)(base + j)] : kPtRecZero;
                ballots(grp.data(), (int)step, K);
                in = (in & 0x7Fu) | (pt_rec_then(in, pt_rec_right(K, low_bits((int)step))) & 0x180u);
            }
            ballots(&wrec[(size_t)(t * wpt)], (int)wpt, K);
            for (int64_t l = 0; l < wpt && t * wpt + l < n_words; ++l) {
                const int64_t w = t * wpt + l;
                const uint32_t left = pt_rec_then(in, pt_rec_left(K, low_bits((int)l)));
                const uint32_t right = pt_rec_then(pt_rec_right(K, low_bits((int)wpt) & ~low_bits((int)l + 1)), in);
                if ((left & 0x54u) || (right & 0x100u)) {
                    fprintf(stderr, "word %lld: a carry is left unresolved (%x, %x)\n", (long long)w, left, right);
                    return 3;
                }
                const uint64_t got = pt_cl100k_finish(planes[(size_t)w], pt_carry_of((left & 0x7Fu) | (right & 0x180u)));
                for (int i = 0; i < kPtWord && w * kPtWord + i < total; ++i)
                    if (((got >> i) & 1u) != want[(size_t)(w * kPtWord + i)]) {
                        fprintf(stderr, "word %lld bit %d: the word form gives %d, the scalar walk %d\n", (long long)w, i, (int)((got >> i) & 1u),
                                (int)want[(size_t)(w * kPtWord + i)]);
                        return 3;
                    }
            }
        }
        for (long s = 0; s < n_str; ++s) {
            bool any = false;
            for (int64_t i = off[s]; i < off[s + 1]; ++i)
                if (want[(size_t)i]) {
                    printf(any ? " %lld" : "%lld", (long long)(i - off[s]));
                    any = true;
                }
            printf(any ? "\n" : "-\n");
        }
    }
    return 0;
}
