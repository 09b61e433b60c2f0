// Host harness of latok_amd/csrc/token_hash.h (tests/test_token_hashes_host.py): both forms of the device's hash, run by g++ on
// tokens inside a poisoned buffer, so that the arithmetic, the order of the wave fold, the masks and the bounds of the aligned
// loads are tested without a device.
//   stdin:  poison(hex byte)  then lines  "<form> <pad> <seed hex> <token bytes as hex, '-' for none>"
//           form l = th_hash_lane, w = the wave's rounds (th_wave_block per lane, th_wave_fold, th_wave_tail)
//           pad  = bytes in front of the token (its start alignment); the buffer ends with the aligned dword of its last byte
//   stdout: one hash (hex) per line; exit 2 if a load left the buffer
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "token_hash.h"

static bool g_out_of_bounds = false;

int main() {
    unsigned poison = 0;
    if (scanf("%x", &poison) != 1) return 1;
    char form;
    long pad;
    unsigned seed;
    static char hex[1 << 16];
    while (scanf(" %c %ld %x %65535s", &form, &pad, &seed, hex) == 4) {
        const size_t n = hex[0] == '-' ? 0 : strlen(hex) / 2;
        const int64_t a = pad, e = pad + (int64_t)n;
        const size_t n_dwords = e > 0 ? (size_t)((e - 1) >> 2) + 1 : 1;      // up to the dword of the last byte, no further
        std::vector<uint8_t> buf(4 * n_dwords, (uint8_t)poison);
        for (size_t i = 0; i < n; ++i) {
            unsigned v = 0;
            sscanf(hex + 2 * i, "%2x", &v);
            buf[(size_t)pad + i] = (uint8_t)v;
        }
        const uint8_t* p = buf.data();
        auto ld = [p, n_dwords](int64_t i) -> uint32_t {
            if (i < 0 || (size_t)i >= n_dwords) { g_out_of_bounds = true; return 0xDEADBEEFu; }
            uint32_t w;
            memcpy(&w, p + 4 * i, 4);
            return w;
        };
        uint32_t h;
        if (form == 'l') {
            h = th_hash_lane(ld, a, e, seed);
        } else {
            h = seed;
            const int64_t rounds = (((e - a) >> 2) + kThWaveBlocks - 1) / kThWaveBlocks;
            for (int64_t r = 0; r < rounds; ++r) {
                uint32_t k[kThWaveBlocks];
                for (int l = 0; l < kThWaveBlocks; ++l) k[l] = th_wave_block(ld, a, e, r, l);
                h = th_wave_fold(h, [&k](int l) { return k[l]; }, th_wave_count(a, e, r));
            }
            h = th_wave_tail(ld, a, e, h);
        }
        printf("%08x\n", h);
    }
    return g_out_of_bounds ? 2 : 0;
}
