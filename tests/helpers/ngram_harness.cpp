// Host harness of latok_amd/csrc/ngram_text.h (tests/test_ngram_host.py): the streaming MurmurHash3 state and the gram compare of
// the n-gram term counts, run by g++ on tokens inside a poisoned buffer that is exactly as long as the aligned dword that holds the
// last token's last byte, so that every carry count against every alignment, the finish behind every token and the bounds of the
// aligned loads are tested without a device.
//   stdin:  poison(hex byte), then commands, one per line:
//             H <seed hex> <sep hex> <n> then n pairs <gap> <token hex>
//                     the tokens lie in the buffer in order, each behind `gap` poisoned bytes (the first gap is the start alignment);
//                     fed as token, sep, token, sep, .. with a finish behind every token
//             E <sep hex> <n> then n pairs <gap> <token hex>, then <word hex>
//                     ng_equal of the gram against the word, which lies zero-padded in a blob of exactly its own dwords at dword 0
//   stdout: per H:  n hashes (hex), one per finish;  per E:  1 or 0
//   exit 2 if a text load left the buffer, 3 if a blob load left the blob
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <iostream>
#include <string>
#include <vector>

#include "ngram_text.h"

static int g_bad = 0;

static std::vector<uint8_t> unhex(const std::string& hex) {
    std::vector<uint8_t> out;
    for (size_t i = 0; i + 1 < hex.size(); i += 2) out.push_back((uint8_t)std::stoul(hex.substr(i, 2), nullptr, 16));
    return out;
}

struct Text {
    std::vector<uint8_t> buf;
    std::vector<NgSpan> tok;
};
// n pairs <gap> <token hex> from stdin
static bool read_text(int n, unsigned poison, Text* t) {
    std::vector<uint8_t> bytes;
    for (int k = 0; k < n; ++k) {
        long gap;
        std::string hex;
        if (!(std::cin >> gap >> hex) || gap < 0) return false;
        const std::vector<uint8_t> data = unhex(hex);
        if (data.empty()) return false;   // (no token is empty)
        bytes.insert(bytes.end(), (size_t)gap, (uint8_t)poison);
        t->tok.push_back(NgSpan{(int64_t)bytes.size(), (int64_t)(bytes.size() + data.size())});
        bytes.insert(bytes.end(), data.begin(), data.end());
    }
    const size_t n_dwords = ((bytes.size() - 1) >> 2) + 1;   // up to the dword of the last byte, no further
    t->buf.assign(4 * n_dwords, (uint8_t)poison);
    memcpy(t->buf.data(), bytes.data(), bytes.size());
    return true;
}

int main() {
    unsigned poison = 0;
    std::string cmd;
    if (!(std::cin >> std::hex >> poison >> std::dec)) return 1;
    while (std::cin >> cmd) {
        unsigned seed = 0, sep = 0;
        int n = 0;
        if (cmd == "H") {
            if (!(std::cin >> std::hex >> seed >> sep >> std::dec >> n)) return 1;
        } else if (cmd == "E") {
            if (!(std::cin >> std::hex >> sep >> std::dec >> n)) return 1;
        } else {
            return 1;
        }
        Text t;
        if (n < 1 || !read_text(n, poison, &t)) return 1;
        const uint8_t* p = t.buf.data();
        const size_t n_dwords = t.buf.size() / 4;
        auto ld = [p, n_dwords](int64_t i) -> uint32_t {
            if (i < 0 || (size_t)i >= n_dwords) { g_bad |= 2; return 0xDEADBEEFu; }
            uint32_t w;
            memcpy(&w, p + 4 * i, 4);
            return w;
        };
        if (cmd == "H") {
            NgHash st = ng_hash_init(seed);
            for (int k = 0; k < n; ++k) {
                if (k > 0) ng_hash_byte(st, sep);
                ng_hash_token(st, ld, t.tok[k].a, t.tok[k].e);
                printf("%08x%c", ng_hash_finish(st), k + 1 < n ? ' ' : '\n');
            }
            continue;
        }
        std::string hex;
        if (!(std::cin >> hex)) return 1;
        const std::vector<uint8_t> word = unhex(hex);
        std::vector<uint32_t> blob((word.size() + 3) / 4 + (word.empty() ? 1 : 0), 0u);
        memcpy(blob.data(), word.data(), word.size());
        const std::vector<uint32_t>* bp = &blob;
        auto bl = [bp](uint64_t i) -> uint32_t {
            if (i >= bp->size()) { g_bad |= 3; return 0xDEADBEEFu; }
            return (*bp)[i];
        };
        const Text* tp = &t;
        printf("%d\n", ng_equal(ld, [tp](int k) { return tp->tok[k]; }, n, sep, bl, 0u, (uint32_t)word.size()) ? 1 : 0);
    }
    return g_bad;
}
