// Host harness of latok_amd/csrc/tfidf_weight.h (tests/test_tfidf_host.py): the scalar rules the kernels of tfidf_kernels.hip call,
// run by g++ (once more with the address and undefined-behaviour sanitizers).  Prints one line per case, the float32 result as its bit
// pattern so that nothing is lost in text:
//   idf <df> <n_docs> <smooth> <bits>
//   tf <t> <sublinear> <bits>
//   row <norm: 0 none, 1 l1, 2 l2> <k> <bits of out[0]> .. : tw_term / tw_norm / tw_scale over the weights 1 .. k, and over k zeros
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "tfidf_weight.h"

static unsigned bits_of(float v) {
    unsigned u;
    memcpy(&u, &v, 4);
    return u;
}

static void row(int norm, int k, bool zeros) {
    float w[8], sum = 0.0f;
    for (int i = 0; i < k; ++i) {
        w[i] = zeros ? 0.0f : (float)(i + 1) * ((i & 1) ? -1.0f : 1.0f);
        if (norm) sum += tw_term(w[i], norm == 2);
    }
    const float n = norm ? tw_norm(sum, norm == 2) : 1.0f;
    printf("row %d %d %d", norm, k, zeros ? 1 : 0);
    for (int i = 0; i < k; ++i) printf(" %08x", bits_of(tw_scale(w[i], n)));
    printf("\n");
}

int main() {
    const int64_t ns[3] = {0, 1, 2147483647};
    for (int smooth = 0; smooth < 2; ++smooth)
        for (const int64_t n : ns) {
            const int64_t dfs[3] = {0, 1, n};
            for (const int64_t df : dfs)
                if (df <= n) printf("idf %lld %lld %d %08x\n", (long long)df, (long long)n, smooth, bits_of(tw_idf((int32_t)df, n, smooth != 0)));
        }
    const int32_t ts[8] = {INT32_MIN + 1, -3, -1, 0, 1, 2, (1 << 24) + 1, INT32_MAX};
    for (int sub = 0; sub < 2; ++sub)
        for (const int32_t t : ts) printf("tf %d %d %08x\n", (int)t, sub, bits_of(tw_tf(t, sub != 0)));
    for (int norm = 0; norm < 3; ++norm)
        for (int k = 1; k <= 5; k += 2) {
            row(norm, k, false);
            row(norm, k, true);
        }
    return 0;
}
