/* Minimal C caller of liblatok_hip.so: the Unigram ids of a few UTF-8 strings against a small SentencePiece-style vocabulary (words
 * with scores, the marker U+2581 in front of a word that starts a string or follows whitespace) -- first as CSR rows with the byte
 * range of every piece (a size query, then the call), then as the padded [n, 12] block with BOS / EOS -- searched on the device.
 *   gcc -std=c99 -Iinclude examples/unigram_utf8.c -Llatok_amd -llatok_hip -Wl,-rpath,$PWD/latok_amd -o /tmp/unigram_utf8
 * Needs a HIP device at run time (there is no CPU fallback); compiling it only needs the header. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "latok_hip.h"

#define MK "\xE2\x96\x81"

int main(void) {
    /* ids 100 + position; the three specials live outside the list */
    const char* vocab_words[] = {MK, "l", "o", "w", "e", "r", "s", "t", MK "low", "low", "er", "est", MK "s", ","};
    const float scores[] = {-2.0f, -5.0f, -5.0f, -5.0f, -5.0f, -5.0f, -5.0f, -5.0f, -3.0f, -3.5f, -3.0f, -3.25f, -4.0f, -2.5f};
    const char* texts[] = {"low lower lowest", "slowest,  low", "", "   ", "low \xC3\xA9"};
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

    latok_unigram* uni = NULL;
    /* unk_score = min(scores) - 10, neighbouring unknown pieces fused */
    if (latok_init(0) != LATOK_OK ||
        latok_unigram_create((const uint8_t*)words, word_off, n_words, scores, word_ids, (const uint8_t*)MK, 3, -15.0f, 1, 4096, 0u, &uni) != LATOK_OK) {
        fprintf(stderr, "latok_init / latok_unigram_create: %s\n", latok_last_error());
        return 1;
    }
    /* size query: no id buffer, capacity 0 -- indptr is valid already, the call reports the number of pieces */
    int64_t indptr[n + 1], need = 0, got = 0, tokens = 0;
    int rc = latok_unigram_ids_utf8_bytes_batch(buf, off, n, off[n], uni, unk, indptr, NULL, NULL, 0, &need, &tokens, 0, NULL);
    if (rc != LATOK_OK && need == 0) {
        fprintf(stderr, "latok_unigram_ids_utf8_bytes_batch: %s\n", latok_last_error());
        return 1;
    }
    int32_t* ids = (int32_t*)malloc((size_t)(need + 1) * sizeof(int32_t));
    int64_t* spans = (int64_t*)malloc((size_t)(need + 1) * 2 * sizeof(int64_t));
    if (latok_unigram_ids_utf8_bytes_batch(buf, off, n, off[n], uni, unk, indptr, ids, spans, need, &got, &tokens, 0, NULL) != LATOK_OK || got != need) {
        fprintf(stderr, "latok_unigram_ids_utf8_bytes_batch: %s\n", latok_last_error());
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
    if (latok_unigram_padded_utf8_bytes_batch(buf, off, n, off[n], uni, unk, max_length, 1, bos, eos, pad, block, lengths, NULL, 0, NULL) != LATOK_OK) {
        fprintf(stderr, "latok_unigram_padded_utf8_bytes_batch: %s\n", latok_last_error());
        return 1;
    }
    for (int i = 0; i < n; ++i) {
        printf("  input_ids %d (%d used):", i, (int)lengths[i]);
        for (int j = 0; j < max_length; ++j) printf(" %d", (int)block[i * max_length + j]);
        printf("\n");
    }
    latok_unigram_destroy(uni);
    latok_shutdown();
    free(ids);
    free(spans);
    free(buf);
    return 0;
}
