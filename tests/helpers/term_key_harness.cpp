// Host harness of latok_amd/csrc/term_key.h (tests/test_term_key_host.py): the key of the term-count calls, run by g++, so that
// the bucket and sign arithmetic, the key layout and its order are tested without a device.
//   stdin:  lines  "h <hash hex> <n_features> <alternate_sign>"              hashed key of a hash word
//                  "t <seed hex> <n_features> <alternate_sign> <token hex>"  the same for th_hash_lane of the token's bytes
//                  "v <id>"                                                 vocabulary key of an int32 id
//                  "o"                                                      the out-of-vocabulary key
//   stdout: one line each: "<key hex> <column> <value> <oov 0/1> <hash hex>"  (column: as the form reads it back)
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "term_key.h"
#include "token_hash.h"

static void put(uint64_t key, bool vocab, uint32_t hash) {
    printf("%" PRIx64 " %d %d %d %08x\n", key, (int)(vocab ? tk_vocab_column(key) : tk_hashed_column(key)), (int)tk_value(key), (int)tk_is_oov(key), hash);
}

int main() {
    char form;
    static char hex[1 << 12];
    while (scanf(" %c", &form) == 1) {
        unsigned h = 0, seed = 0;
        long long n = 0, id = 0;
        int alt = 0;
        if (form == 'h') {
            if (scanf("%x %lld %d", &h, &n, &alt) != 3) return 1;
            put(tk_hashed_key(h, (uint32_t)n, alt != 0), false, h);
        } else if (form == 't') {
            if (scanf("%x %lld %d %4095s", &seed, &n, &alt, hex) != 4) return 1;
            const size_t len = strlen(hex) / 2;
            std::vector<uint8_t> buf(((len + 3) / 4 + 1) * 4, (uint8_t)0xA5);
            for (size_t i = 0; i < len; ++i) {
                unsigned v = 0;
                sscanf(hex + 2 * i, "%2x", &v);
                buf[i] = (uint8_t)v;
            }
            const uint8_t* p = buf.data();
            h = th_hash_lane([p](int64_t i) { uint32_t w; memcpy(&w, p + 4 * i, 4); return w; }, 0, (int64_t)len, seed);
            put(tk_hashed_key(h, (uint32_t)n, alt != 0), false, h);
        } else if (form == 'v') {
            if (scanf("%lld", &id) != 1) return 1;
            put(tk_vocab_key((int32_t)id), true, 0);
        } else if (form == 'o') {
            put(kTkOov, true, 0);
        } else {
            return 1;
        }
    }
    return 0;
}
