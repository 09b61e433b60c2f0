/* Minimal C caller of liblatok_hip.so: the tokenized line of a few UTF-8 strings -- each string's tokens joined by one space,
 * cut and joined on the device -- first a size query, then the call, then the rows.
 *   gcc -std=c99 -Iinclude examples/join_tokens_utf8.c -Llatok_amd -llatok_hip -Wl,-rpath,$PWD/latok_amd -o /tmp/join_tokens_utf8
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
    int64_t off[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < n; ++i) off[i + 1] = off[i] + (int64_t)strlen(texts[i]);
    uint8_t* buf = (uint8_t*)malloc((size_t)off[n]);
    for (int i = 0; i < n; ++i) memcpy(buf + off[i], texts[i], (size_t)(off[i + 1] - off[i]));

    if (latok_init(0) != LATOK_OK) {
        fprintf(stderr, "latok_init: %s\n", latok_last_error());
        return 1;
    }
    /* size query: no output buffer, capacity 0 -- the row offsets and counts are valid already, the call reports the size */
    int64_t out_off[6], counts[5], need = 0;
    int rc = latok_join_tokens_utf8_bytes_batch(buf, off, n, off[n], ' ', NULL, 0, out_off, counts, &need, 0, NULL);
    if (rc != LATOK_OK && need == 0) {
        fprintf(stderr, "latok_join_tokens_utf8_bytes_batch: %s\n", latok_last_error());
        return 1;
    }
    uint8_t* out = (uint8_t*)malloc((size_t)need + 1);
    int64_t got = 0;
    if (latok_join_tokens_utf8_bytes_batch(buf, off, n, off[n], ' ', out, need, out_off, counts, &got, 0, NULL) != LATOK_OK || got != need) {
        fprintf(stderr, "latok_join_tokens_utf8_bytes_batch: %s\n", latok_last_error());
        return 1;
    }
    for (int i = 0; i < n; ++i)
        printf("%d (%d tokens): %.*s\n", i, (int)counts[i], (int)(out_off[i + 1] - out_off[i]), (const char*)out + out_off[i]);
    latok_shutdown();
    free(out);
    free(buf);
    return 0;
}
