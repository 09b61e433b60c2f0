/* Minimal C caller of liblatok_hip.so: the byte-level BPE ids of a few UTF-8 strings against a small GPT-style vocabulary (the words
 * in rank order, lead_space = 1: a word after a space carries that space) -- first as CSR rows with the byte range of every piece (a
 * size query, then the call), then as the padded [n, 12] block with BOS / EOS -- merged and looked up on the device.
 *   gcc -std=c99 -Iinclude examples/bpe_utf8.c -Llatok_amd -llatok_hip -Wl,-rpath,$PWD/latok_amd -o /tmp/bpe_utf8
 * Needs a HIP device at run time (there is no CPU fallback); compiling it only needs the header. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "latok_hip.h"

int main(void) {
    /* ranks 0 .. 13; ids 100 + rank, and the three specials live outside the list */
    const char* vocab_words[] = {" ", "l", "o", "w", "e", "r", "s", "t", "lo", "low", " low", "er", "es", "est"};
    const char* texts[] = {"low lower lowest", "slowest  low", "", "   ", "low \xC3\xA9"};
    enum { n_words = 14, n = 5, max_length = 12, unk = 99, bos = 1, eos = 2, pad = 0 };
    char words[256];
    int64_t word_off[n_words + 1] = {0}, off[n + 1] = {0};
    int32_t word_ids[n_words];
    for (int i = 0; i < n_words; ++i) {
        memcpy(words + word_off[i], vocab_words[i], strlen(vocab_words[i]));
        word_off[i + 1] = word_off[i] + (int64_t)strlen(vocab_words[i]);
        word_ids[i] = 100 + i;
    }
    for (int i = 0; i < n; ++i) off[i + 1] = off[i] + (int64_t)strlen(texts[i]);
    uint8_t* buf = (uint8_t*)malloc((size_t)off[n] + 1);
    for (int i = 0; i < n; ++i) memcpy(buf + off[i], texts[i], (size_t)(off[i + 1] - off[i]));

    latok_bpe* bpe = NULL;
    if (latok_init(0) != LATOK_OK || latok_bpe_create((const uint8_t*)words, word_off, n_words, word_ids, 4096, 1, 0u, &bpe) != LATOK_OK) {
        fprintf(stderr, "latok_init / latok_bpe_create: %s\n", latok_last_error());
        return 1;
    }
    /* size query: no id buffer, capacity 0 -- indptr is valid already, the call reports the number of pieces */
    int64_t indptr[n + 1], need = 0, got = 0, tokens = 0;
    int rc = latok_bpe_ids_utf8_bytes_batch(buf, off, n, off[n], bpe, unk, indptr, NULL, NULL, 0, &need, &tokens, 0, NULL);
    if (rc != LATOK_OK && need == 0) {
        fprintf(stderr, "latok_bpe_ids_utf8_bytes_batch: %s\n", latok_last_error());
        return 1;
    }
    int32_t* ids = (int32_t*)malloc((size_t)(need + 1) * sizeof(int32_t));
    int64_t* spans = (int64_t*)malloc((size_t)(need + 1) * 2 * sizeof(int64_t));
    if (latok_bpe_ids_utf8_bytes_batch(buf, off, n, off[n], bpe, unk, indptr, ids, spans, need, &got, &tokens, 0, NULL) != LATOK_OK || got != need) {
        fprintf(stderr, "latok_bpe_ids_utf8_bytes_batch: %s\n", latok_last_error());
        return 1;
    }
    printf("%d tokens, %d pieces\n", (int)tokens, (int)got);
    for (int i = 0; i < n; ++i) {
        printf("  row %d:", i);
        for (int64_t k = indptr[i]; k < indptr[i + 1]; ++k)
            printf(" '%s'[%d,%d)", ids[k] == unk ? "?" : vocab_words[ids[k] - 100], (int)spans[2 * k], (int)spans[2 * k + 1]);
        printf("\n");
    }

    /* the padded form */
    int32_t block[n * max_length], lengths[n];
    if (latok_bpe_padded_utf8_bytes_batch(buf, off, n, off[n], bpe, unk, max_length, 1, bos, eos, pad, block, lengths, NULL, 0, NULL) != LATOK_OK) {
        fprintf(stderr, "latok_bpe_padded_utf8_bytes_batch: %s\n", latok_last_error());
        return 1;
    }
    for (int i = 0; i < n; ++i) {
        printf("  input_ids %d (%d used):", i, (int)lengths[i]);
        for (int j = 0; j < max_length; ++j) printf(" %d", (int)block[i * max_length + j]);
        printf("\n");
    }
    latok_bpe_destroy(bpe);
    latok_shutdown();
    free(ids);
    free(spans);
    free(buf);
    return 0;
}
