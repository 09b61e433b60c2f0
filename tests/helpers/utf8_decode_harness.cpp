// Host harness of latok_amd/csrc/utf8_decode.h (tests/test_utf8_decode_host.py): the decoders the device kernels are built from, run
// by g++ on 4-byte windows, so that their values are held to the reference without a device.
//   utf8_decode_harness w <in> <out> <poison hex>
//       in:  N windows of 4 bytes {b0, b1, b2, b3}
//       out: four uint32[N] arrays one after the other --
//            the smallest and the largest of utf8_decode_at<I>, I = 0..15, with the window at bytes I..I+3 of 19 bytes that are
//            `poison` everywhere else; utf8_decode_bytes(b0, b1, b2, b3); utf8_cp_of(the window as a dword)
//   utf8_decode_harness n <in> <out>
//       in:  N dwords;  out: uint32[N] = utf8_lead_nibble of each
#define __device__
#define __forceinline__ inline
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "utf8_decode.h"

template <int I>
static uint32_t at(const uint8_t* win, uint8_t poison) {
    uint8_t b[20];
    memset(b, poison, sizeof b);
    memcpy(b + I, win, 4);
    uint32_t w[5];
    memcpy(w, b, 20);
    return latok::utf8_decode_at<I>(w);
}

template <int I>
struct Each {
    static void run(const uint8_t* win, uint8_t poison, uint32_t* lo, uint32_t* hi) {
        const uint32_t v = at<I>(win, poison);
        if (v < *lo) *lo = v;
        if (v > *hi) *hi = v;
        Each<I + 1>::run(win, poison, lo, hi);
    }
};
template <>
struct Each<16> {
    static void run(const uint8_t*, uint8_t, uint32_t*, uint32_t*) {}
};

static std::vector<uint8_t> slurp(const char* path) {
    std::vector<uint8_t> v;
    FILE* f = fopen(path, "rb");
    if (!f) return v;
    uint8_t buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

int main(int argc, char** argv) {
    if (argc < 4) return 1;
    const std::vector<uint8_t> in = slurp(argv[2]);
    if (in.empty() || in.size() % 4) return 1;
    const size_t n = in.size() / 4;
    FILE* out = fopen(argv[3], "wb");
    if (!out) return 1;
    if (argv[1][0] == 'n') {
        std::vector<uint32_t> r(n);
        for (size_t i = 0; i < n; ++i) {
            uint32_t w;
            memcpy(&w, &in[4 * i], 4);
            r[i] = latok::utf8_lead_nibble(w);
        }
        if (fwrite(r.data(), 4, n, out) != n) return 1;
    } else {
        if (argc < 5) return 1;
        const uint8_t poison = (uint8_t)strtoul(argv[4], nullptr, 16);
        std::vector<uint32_t> r(4 * n);
        for (size_t i = 0; i < n; ++i) {
            const uint8_t* win = &in[4 * i];
            uint32_t lo = 0xFFFFFFFFu, hi = 0;
            Each<0>::run(win, poison, &lo, &hi);
            uint32_t w;
            memcpy(&w, win, 4);
            r[i] = lo;
            r[n + i] = hi;
            r[2 * n + i] = latok::utf8_decode_bytes(win[0], win[1], win[2], win[3]);
            r[3 * n + i] = latok::utf8_cp_of(w);
        }
        if (fwrite(r.data(), 4, 4 * n, out) != 4 * n) return 1;
    }
    return fclose(out) == 0 ? 0 : 1;
}
