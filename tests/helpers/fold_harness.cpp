// Host harness for latok_amd/csrc/fold_map.h, built by tests/test_fold_host.py with g++ (once more with the address and
// undefined-behaviour sanitizers): the very functions the kernels of fold_kernels.hip call, on the tables of fold_tables.inc.
//   fold_harness sweep FOLD OUT        F_fold(c) for c = 0 .. 0x110000 as uint32 {n, cp0, cp1, cp2} per code point, written to OUT
//   fold_harness bytes IN OUT          IN = records {int32 fold, int32 n, n bytes}; every string is folded by fold_string at every
//                                      alignment 0 .. 15 inside a poisoned buffer, into a poisoned buffer of exactly the counted size;
//                                      guard bytes and agreement of all alignments are checked here; OUT = records {int32 n, bytes}
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "fold_map.h"
#include "fold_tables.inc"

static FoldTables tables() {
    FoldTables T;
    T.stage1 = kFoldStage1;
    T.stage2 = kFoldStage2;
    T.rec = kFoldRec;
    T.high = kFoldHigh;
    T.n_high = (int)kFoldHighN;
    return T;
}

static int die(const char* what) {
    fprintf(stderr, "fold_harness: %s\n", what);
    return 1;
}

static int sweep(int fold, const char* path) {
    const FoldTables T = tables();
    std::vector<uint32_t> out(4u * 0x110001u);
    for (uint32_t c = 0; c <= 0x110000u; ++c) {
        const FoldImage im = fold_cp(c, fold, T);
        if (im.same != (im.n == 1 && im.cp[0] == c)) return die("same flag disagrees with the image");
        out[4 * c] = (uint32_t)im.n;
        for (int j = 0; j < 3; ++j) out[4 * c + 1 + j] = j < im.n ? im.cp[j] : 0u;
    }
    FILE* f = fopen(path, "wb");
    if (!f || fwrite(out.data(), 4, out.size(), f) != out.size()) return die("cannot write");
    fclose(f);
    return 0;
}

static int bytes_mode(const char* in_path, const char* out_path) {
    const FoldTables T = tables();
    FILE* in = fopen(in_path, "rb");
    FILE* out = fopen(out_path, "wb");
    if (!in || !out) return die("cannot open");
    const int kGuard = 32;
    int32_t head[2];
    while (fread(head, 4, 2, in) == 2) {
        const int fold = head[0];
        const int32_t n = head[1];
        std::vector<uint8_t> s((size_t)n);
        if (n > 0 && fread(s.data(), 1, (size_t)n, in) != (size_t)n) return die("short record");
        std::vector<uint8_t> first;
        for (int a = 0; a < 16; ++a) {
            // exactly n bytes on the heap behind `a` poison bytes: the sanitizer build sees any read behind the string's end
            uint8_t* src = (uint8_t*)malloc((size_t)a + (size_t)n + 1);
            memset(src, 0xC3, (size_t)a);
            if (n > 0) memcpy(src + a, s.data(), (size_t)n);
            const int64_t need = fold_string(src + a, n, fold, T, nullptr);
            if (need < 0 || need > 3 * (int64_t)n) return die("size outside [0, 3 n]");
            std::vector<uint8_t> dst((size_t)need + 2 * kGuard, 0xA5);
            const int64_t got = fold_string(src + a, n, fold, T, dst.data() + kGuard);
            free(src);
            if (got != need) return die("the two walks disagree on the size");
            for (int g = 0; g < kGuard; ++g)
                if (dst[(size_t)g] != 0xA5 || dst[(size_t)kGuard + (size_t)need + (size_t)g] != 0xA5) return die("guard byte overwritten");
            std::vector<uint8_t> body(dst.begin() + kGuard, dst.begin() + kGuard + need);
            if (a == 0) first = body;
            else if (body != first) return die("result depends on the alignment");
        }
        const int32_t len = (int32_t)first.size();
        fwrite(&len, 4, 1, out);
        if (len > 0) fwrite(first.data(), 1, (size_t)len, out);
    }
    fclose(in);
    fclose(out);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "sweep")) return sweep(atoi(argv[2]), argv[3]);
    if (argc == 4 && !strcmp(argv[1], "bytes")) return bytes_mode(argv[2], argv[3]);
    return die("usage: fold_harness sweep FOLD OUT | fold_harness bytes IN OUT");
}
