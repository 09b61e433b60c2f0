/* Minimal C caller of liblatok_hip.so: the id of every token of a few UTF-8 strings in a ten-word vocabulary -- cut, hashed and
 * looked up on the device, exactly (the bytes decide, not the hash) -- first a size query, then the call, then token=id.
 *   gcc -std=c99 -Iinclude examples/token_ids_utf8.c -Llatok_amd -llatok_hip -Wl,-rpath,$PWD/latok_amd -o /tmp/token_ids_utf8
 * Needs a HIP device at run time (there is no CPU fallback); compiling it only needs the header. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "latok_hip.h"

int main(void) {
    const char* vocab_words[] = {"This", "is", "a", "#test", "!", "Testing", ",", "1", "2", "\xE6\x97\xA5\xE6\x9C\xAC\xE8\xAA\x9E"};
    const char* texts[] = {"This is a #test! Testing, Testing, 1 2 3", "this is not", "", "   ",
                           "a \xE6\x97\xA5\xE6\x9C\xAC\xE8\xAA\x9E \xF0\x9F\xA4\x93"};
    const int64_t n_words = 10, n = 5;
    const int32_t unk = -1;
    char words[128];
    int64_t word_off[11] = {0}, off[6] = {0};
    for (int i = 0; i < n_words; ++i) {
        memcpy(words + word_off[i], vocab_words[i], strlen(vocab_words[i]));
        word_off[i + 1] = word_off[i] + (int64_t)strlen(vocab_words[i]);
    }
    for (int i = 0; i < n; ++i) off[i + 1] = off[i] + (int64_t)strlen(texts[i]);
    uint8_t* buf = (uint8_t*)malloc((size_t)off[n]);
    for (int i = 0; i < n; ++i) memcpy(buf + off[i], texts[i], (size_t)(off[i + 1] - off[i]));

    latok_vocab* vocab = NULL;
    if (latok_init(0) != LATOK_OK || latok_vocab_create((const uint8_t*)words, word_off, n_words, NULL, 0u, &vocab) != LATOK_OK) {
        fprintf(stderr, "latok_init / latok_vocab_create: %s\n", latok_last_error());
        return 1;
    }
    /* size query: no output buffer, capacity 0 -- the counts are valid already, the call reports the number of tokens */
    int64_t counts[5], need = 0, got = 0;
    int rc = latok_token_ids_utf8_bytes_batch(buf, off, n, off[n], vocab, unk, counts, NULL, NULL, 0, &need, 0, NULL);
    if (rc != LATOK_OK && need == 0) {
        fprintf(stderr, "latok_token_ids_utf8_bytes_batch: %s\n", latok_last_error());
        return 1;
    }
    int32_t* ids = (int32_t*)malloc((size_t)(need + 1) * sizeof(int32_t));
    int64_t* spans = (int64_t*)malloc((size_t)(need + 1) * 2 * sizeof(int64_t));
    if (latok_token_ids_utf8_bytes_batch(buf, off, n, off[n], vocab, unk, counts, spans, ids, need, &got, 0, NULL) != LATOK_OK || got != need) {
        fprintf(stderr, "latok_token_ids_utf8_bytes_batch: %s\n", latok_last_error());
        return 1;
    }
    int64_t k = 0;
    for (int i = 0; i < n; ++i) {
        printf("%d (%d tokens):", i, (int)counts[i]);
        for (int64_t j = 0; j < counts[i]; ++j, ++k)   /* the records are relative to the string's first byte */
            printf(" %.*s=%d", (int)(spans[2 * k + 1] - spans[2 * k]), (const char*)buf + off[i] + spans[2 * k], (int)ids[k]);
        printf("\n");
    }
    latok_vocab_destroy(vocab);
    latok_shutdown();
    free(spans);
    free(ids);
    free(buf);
    return 0;
}
