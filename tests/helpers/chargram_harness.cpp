// Host harness of latok_amd/csrc/chargram_text.h (tests/test_chargram_host.py): the character count, the gram count, the walk over a
// token's padded word with its slots and streaming hashes, and the gram compare of the character n-gram term counts, run by g++ on a
// token inside a poisoned buffer that is exactly as long as the aligned dword that holds the token's last byte.  Every text load is
// checked against the token's own dwords: none below the dword of its first byte, none behind the dword of its last.
//   stdin:  poison(hex byte), then commands, one per line:
//             W <seed hex> <pad hex> <min_n> <max_n> <gap> <token hex>
//                     the token lies behind `gap` poisoned bytes; cg_count_chars, cg_gram_count, then cg_walk
//             E <pad hex> <gap> <token hex> <gs> <ge> <front> <back> <word hex or ->
//                     cg_equal of the gram whose real characters are the token's bytes [gs, ge) (token-relative), with the pad in
//                     front / behind, against the word, which lies zero-padded in a blob of exactly its own dwords at dword 0
//   stdout: per W:  L G n_emitted, then per emitted gram  slot:hash:len:gs:ge:front:back  (gs, ge token-relative), all on one line
//           per E:  1 or 0
//   exit 2 if a text load left the token's dwords, 3 if a blob load left the blob
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <iostream>
#include <string>
#include <vector>

#include "chargram_text.h"

static int g_bad = 0;

static std::vector<uint8_t> unhex(const std::string& hex) {
    std::vector<uint8_t> out;
    if (hex == "-") return out;
    for (size_t i = 0; i + 1 < hex.size(); i += 2) out.push_back((uint8_t)std::stoul(hex.substr(i, 2), nullptr, 16));
    return out;
}

int main() {
    unsigned poison = 0;
    std::string cmd;
    if (!(std::cin >> std::hex >> poison >> std::dec)) return 1;
    while (std::cin >> cmd) {
        unsigned seed = 0, pad = 0;
        int min_n = 0, max_n = 0;
        long gap = 0;
        std::string hex;
        if (cmd == "W") {
            if (!(std::cin >> std::hex >> seed >> pad >> std::dec >> min_n >> max_n >> gap >> hex)) return 1;
        } else if (cmd == "E") {
            if (!(std::cin >> std::hex >> pad >> std::dec >> gap >> hex)) return 1;
        } else {
            return 1;
        }
        const std::vector<uint8_t> tok = unhex(hex);
        if (tok.empty() || gap < 0) return 1;
        const int64_t a = gap, e = gap + (int64_t)tok.size();
        std::vector<uint8_t> buf(4 * (size_t)(((e - 1) >> 2) + 1), (uint8_t)poison);   // up to the dword of the last byte, no further
        memcpy(buf.data() + a, tok.data(), tok.size());
        const uint8_t* p = buf.data();
        const int64_t q_lo = a >> 2, q_hi = (e - 1) >> 2;
        auto ld = [p, q_lo, q_hi](int64_t i) -> uint32_t {
            if (i < q_lo || i > q_hi) { g_bad |= 2; return 0xDEADBEEFu; }
            uint32_t w;
            memcpy(&w, p + 4 * i, 4);
            return w;
        };
        if (cmd == "W") {
            const int64_t L = cg_count_chars(ld, a, e), W = L + 2;
            std::vector<CgGram> got;
            cg_walk(ld, a, e, W, min_n, max_n, pad, seed, [&got](const CgGram& g) { got.push_back(g); });
            printf("%lld %lld %zu", (long long)L, (long long)cg_gram_count(W, min_n, max_n), got.size());
            for (const CgGram& g : got)
                printf(" %lld:%08x:%u:%lld:%lld:%d:%d", (long long)g.slot, g.hash, g.len, (long long)(g.gs - a), (long long)(g.ge - a), g.front ? 1 : 0,
                       g.back ? 1 : 0);
            printf("\n");
            continue;
        }
        long gs, ge;
        int front, back;
        std::string whex;
        if (!(std::cin >> gs >> ge >> front >> back >> whex)) return 1;
        const std::vector<uint8_t> word = unhex(whex);
        std::vector<uint32_t> blob((word.size() + 3) / 4 + (word.empty() ? 1 : 0), 0u);
        if (!word.empty()) memcpy(blob.data(), word.data(), word.size());
        const std::vector<uint32_t>* bp = &blob;
        auto bl = [bp](uint64_t i) -> uint32_t {
            if (i >= bp->size()) { g_bad |= 3; return 0xDEADBEEFu; }
            return (*bp)[i];
        };
        printf("%d\n", cg_equal(ld, a + gs, a + ge, front != 0, back != 0, pad, bl, 0u, (uint32_t)word.size()) ? 1 : 0);
    }
    return g_bad;
}
