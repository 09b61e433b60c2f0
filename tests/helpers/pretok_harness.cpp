// pretok_harness.cpp -- pretok.h on the host, as a stand-alone program (tests/test_pretok_host.py builds it plain and with sanitizers).
// stdin:  batches, each "B <n>" followed by n lines of hex bytes ("-": the empty string); "C <hex code point>": the class of a scalar value.
// stdout: per string one line with the byte offsets at which a pre-token starts ("-": none); per C line the class 0 .. 3.
// Every batch is cut twice: string by string by pt_starts_scalar, and word by word over the packed batch by pt_word_starts, exactly as
// the device kernel calls it (a window of 96 bytes, bytes outside the batch read as 0, the string starts and the batch's end as bits).
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

int main() {
    const PretokTables T{kPretokStage1, kPretokStage2, PRETOK_TABLE_LIMIT};
    std::string line;
    std::vector<char> buf(1 << 22);
    while (fgets(buf.data(), (int)buf.size(), stdin)) {
        if (buf[0] == 'C') {
            printf("%d\n", pt_class_cp((uint32_t)strtoul(buf.data() + 2, nullptr, 16), T));
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
            pt_starts_scalar(str.data(), n, T, cls.data(), st.data());
            for (int64_t i = 0; i < n; ++i) want[(size_t)(off[s] + i)] = st[(size_t)i];
        }
        // the word form over the packed batch
        std::vector<uint8_t> is_first((size_t)total + 1, 0);
        for (long s = 0; s <= n_str; ++s) is_first[(size_t)off[s]] = 1;
        for (int64_t w0 = 0; w0 < total; w0 += kPtWord) {
            HostWindow win;
            pt_u128 B = 0;
            for (int i = 0; i < kPtWindow; ++i) {
                const int64_t p = w0 - kPtHalo + i;
                win.b[i] = p >= 0 && p < total ? text[(size_t)p] : 0;
                if (p >= 0 && p <= total && is_first[(size_t)p]) B |= (pt_u128)1 << i;
            }
            const uint64_t got = pt_word_starts(win, B, T);
            for (int i = 0; i < kPtWord && w0 + i < total; ++i)
                if (((got >> i) & 1u) != want[(size_t)(w0 + i)]) {
                    fprintf(stderr, "word %lld bit %d: the word form gives %d, the scalar walk %d\n", (long long)(w0 / kPtWord), i, (int)((got >> i) & 1u),
                            (int)want[(size_t)(w0 + i)]);
                    return 3;
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
