/* Minimal C caller of liblatok_hip.so: the vocabulary of a few UTF-8 strings -- every distinct token with its frequency, counted on
 * the device, exactly (the bytes decide, not the hash) --, read back, turned into a latok_vocab, and the ids of the same strings in
 * it: corpus -> vocabulary -> ids without a token ever being cut on the host.
 *   gcc -std=c99 -Iinclude examples/count_tokens_utf8.c -Llatok_amd -llatok_hip -Wl,-rpath,$PWD/latok_amd -o /tmp/count_tokens_utf8
 * Needs a HIP device at run time (there is no CPU fallback); compiling it only needs the header. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "latok_hip.h"

int main(void) {
    const char* texts[] = {"This is a #test! Testing, Testing, 1 2 3", "this is not a test", "", "   ",
                           "a \xE6\x97\xA5\xE6\x9C\xAC\xE8\xAA\x9E \xF0\x9F\xA4\x93 a"};
    const int64_t n = 5;
    int64_t off[6] = {0};
    for (int i = 0; i < n; ++i) off[i + 1] = off[i] + (int64_t)strlen(texts[i]);
    uint8_t* buf = (uint8_t*)malloc((size_t)off[n]);
    for (int i = 0; i < n; ++i) memcpy(buf + off[i], texts[i], (size_t)(off[i + 1] - off[i]));

    /* a counter for up to 1000 distinct words of up to 256 bytes; one update per batch, as many batches as the corpus has */
    latok_counter* counter = NULL;
    int64_t stats[5];
    if (latok_init(0) != LATOK_OK || latok_counter_create(1000, 256, 0u, &counter) != LATOK_OK ||
        latok_count_tokens_utf8_bytes_batch(buf, off, n, off[n], counter, stats, 0, NULL) != LATOK_OK) {
        fprintf(stderr, "latok_init / latok_counter_create / latok_count_tokens_utf8_bytes_batch: %s\n", latok_last_error());
        return 1;
    }
    printf("this batch: %lld tokens, %lld counted, %lld long, %lld dropped\n", (long long)stats[0], (long long)stats[1], (long long)stats[2],
           (long long)stats[3]);
    /* size query: no buffers, capacity 0 -- the call reports the number of words and of their bytes */
    int64_t n_words = 0, n_bytes = 0;
    int rc = latok_counter_read(counter, NULL, 0, NULL, NULL, 0, &n_words, &n_bytes);
    if (rc != LATOK_OK && n_words == 0) {
        fprintf(stderr, "latok_counter_read: %s\n", latok_last_error());
        return 1;
    }
    uint8_t* words = (uint8_t*)malloc((size_t)n_bytes + 1);
    int64_t* word_off = (int64_t*)malloc((size_t)(n_words + 1) * sizeof(int64_t));
    uint64_t* word_counts = (uint64_t*)malloc((size_t)(n_words + 1) * sizeof(uint64_t));
    if (latok_counter_read(counter, words, n_bytes, word_off, word_counts, n_words, &n_words, &n_bytes) != LATOK_OK) {
        fprintf(stderr, "latok_counter_read: %s\n", latok_last_error());
        return 1;
    }
    for (int64_t i = 0; i < n_words; ++i)   /* (in table order: sort by count for a ranking) */
        printf("%.*s x%llu\n", (int)(word_off[i + 1] - word_off[i]), (const char*)words + word_off[i], (unsigned long long)word_counts[i]);

    /* the words and their offsets have the layout latok_vocab_create takes: word i gets id i */
    latok_vocab* vocab = NULL;
    if (latok_vocab_create(words, word_off, n_words, NULL, 0u, &vocab) != LATOK_OK) {
        fprintf(stderr, "latok_vocab_create: %s\n", latok_last_error());
        return 1;
    }
    int64_t counts[5], got = 0;
    int32_t* ids = (int32_t*)malloc((size_t)(stats[0] + 1) * sizeof(int32_t));
    if (latok_token_ids_utf8_bytes_batch(buf, off, n, off[n], vocab, -1, counts, NULL, ids, stats[0], &got, 0, NULL) != LATOK_OK || got != stats[0]) {
        fprintf(stderr, "latok_token_ids_utf8_bytes_batch: %s\n", latok_last_error());
        return 1;
    }
    int64_t k = 0;
    for (int i = 0; i < n; ++i) {
        printf("%d (%d tokens):", i, (int)counts[i]);
        for (int64_t j = 0; j < counts[i]; ++j, ++k) printf(" %d", (int)ids[k]);   /* no -1: every token is in its own vocabulary */
        printf("\n");
    }
    latok_vocab_destroy(vocab);
    latok_counter_destroy(counter);
    latok_shutdown();
    free(ids);
    free(word_counts);
    free(word_off);
    free(words);
    free(buf);
    return 0;
}
