/* Minimal C caller of liblatok_hip.so: one 32-bit id per token of a few UTF-8 strings -- MurmurHash3 x86_32 of the token's bytes,
 * cut and hashed on the device -- first a size query, then the call, then every token with its id and a bucket of a 2^18 table.
 *   gcc -std=c99 -Iinclude examples/token_hashes_utf8.c -Llatok_amd -llatok_hip -Wl,-rpath,$PWD/latok_amd -o /tmp/token_hashes_utf8
 * Needs a HIP device at run time (there is no CPU fallback); compiling it only needs the header. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "latok_hip.h"

int main(void) {
    const char* texts[] = {"This is a #test! Testing, Testing, 1 2 3", "see http://a.b/c or mail me@x.org", "", "   ",
                           "camelCase \xE6\x97\xA5\xE6\x9C\xAC\xE8\xAA\x9E \xF0\x9F\xA4\x93"};
    const int64_t n = 5;
    const uint32_t seed = 0;
    int64_t off[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < n; ++i) off[i + 1] = off[i] + (int64_t)strlen(texts[i]);
    uint8_t* buf = (uint8_t*)malloc((size_t)off[n]);
    for (int i = 0; i < n; ++i) memcpy(buf + off[i], texts[i], (size_t)(off[i + 1] - off[i]));

    if (latok_init(0) != LATOK_OK) {
        fprintf(stderr, "latok_init: %s\n", latok_last_error());
        return 1;
    }
    /* size query: no output buffer, capacity 0 -- the counts are valid already, the call reports the number of tokens */
    int64_t counts[5], need = 0;
    int rc = latok_token_hashes_utf8_bytes_batch(buf, off, n, off[n], seed, counts, NULL, NULL, 0, &need, 0, NULL);
    if (rc != LATOK_OK && need == 0) {
        fprintf(stderr, "latok_token_hashes_utf8_bytes_batch: %s\n", latok_last_error());
        return 1;
    }
    uint32_t* hashes = (uint32_t*)malloc((size_t)(need + 1) * sizeof(uint32_t));
    int64_t* spans = (int64_t*)malloc((size_t)(need + 1) * 2 * sizeof(int64_t));
    int64_t got = 0;
    if (latok_token_hashes_utf8_bytes_batch(buf, off, n, off[n], seed, counts, spans, hashes, need, &got, 0, NULL) != LATOK_OK || got != need) {
        fprintf(stderr, "latok_token_hashes_utf8_bytes_batch: %s\n", latok_last_error());
        return 1;
    }
    int64_t k = 0;
    for (int i = 0; i < n; ++i) {
        printf("%d (%d tokens):", i, (int)counts[i]);
        for (int64_t j = 0; j < counts[i]; ++j, ++k)   /* the records are relative to the string's first byte */
            printf(" %.*s=%08x/%u", (int)(spans[2 * k + 1] - spans[2 * k]), (const char*)buf + off[i] + spans[2 * k], (unsigned)hashes[k],
                   (unsigned)(hashes[k] & 0x3FFFFu));
        printf("\n");
    }
    latok_shutdown();
    free(spans);
    free(hashes);
    free(buf);
    return 0;
}
