/* Minimal C caller of liblatok_hip.so: the WordPiece ids of a few UTF-8 strings against a small BERT-style vocabulary -- first as
 * CSR rows with the byte range of every piece (a size query, then the call), then as the padded [n, 12] block with [CLS] / [SEP] a
 * model takes -- cut and looked up on the device.
 *   gcc -std=c99 -Iinclude examples/wordpiece_utf8.c -Llatok_amd -llatok_hip -Wl,-rpath,$PWD/latok_amd -o /tmp/wordpiece_utf8
 * Needs a HIP device at run time (there is no CPU fallback); compiling it only needs the header. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "latok_hip.h"

int main(void) {
    const char* vocab_words[] = {"[PAD]", "[UNK]", "[CLS]", "[SEP]", "un", "##aff", "##able", "##ing", "test", "a", "is", "this", "!", "##s"};
    const char* texts[] = {"this is unaffable !", "tests testing unaffing", "", "   ", "a \xE6\x97\xA5\xE6\x9C\xAC\xE8\xAA\x9E a"};
    enum { n_words = 14, n = 5, max_length = 12 };
    char words[256];
    int64_t word_off[n_words + 1] = {0}, off[n + 1] = {0};
    for (int i = 0; i < n_words; ++i) {
        memcpy(words + word_off[i], vocab_words[i], strlen(vocab_words[i]));
        word_off[i + 1] = word_off[i] + (int64_t)strlen(vocab_words[i]);
    }
    for (int i = 0; i < n; ++i) off[i + 1] = off[i] + (int64_t)strlen(texts[i]);
    uint8_t* buf = (uint8_t*)malloc((size_t)off[n] + 1);
    for (int i = 0; i < n; ++i) memcpy(buf + off[i], texts[i], (size_t)(off[i + 1] - off[i]));

    latok_wordpiece* wp = NULL;
    if (latok_init(0) != LATOK_OK ||
        latok_wordpiece_create((const uint8_t*)words, word_off, n_words, NULL, (const uint8_t*)"##", 2, 100, 0u, &wp) != LATOK_OK) {
        fprintf(stderr, "latok_init / latok_wordpiece_create: %s\n", latok_last_error());
        return 1;
    }
    /* size query: no id buffer, capacity 0 -- indptr is valid already, the call reports the number of pieces */
    int64_t indptr[n + 1], need = 0, got = 0, tokens = 0;
    int rc = latok_wordpiece_ids_utf8_bytes_batch(buf, off, n, off[n], wp, 1, indptr, NULL, NULL, 0, &need, &tokens, 0, NULL);
    if (rc != LATOK_OK && need == 0) {
        fprintf(stderr, "latok_wordpiece_ids_utf8_bytes_batch: %s\n", latok_last_error());
        return 1;
    }
    int32_t* ids = (int32_t*)malloc((size_t)(need + 1) * sizeof(int32_t));
    int64_t* spans = (int64_t*)malloc((size_t)(need + 1) * 2 * sizeof(int64_t));
    if (latok_wordpiece_ids_utf8_bytes_batch(buf, off, n, off[n], wp, 1, indptr, ids, spans, need, &got, &tokens, 0, NULL) != LATOK_OK || got != need) {
        fprintf(stderr, "latok_wordpiece_ids_utf8_bytes_batch: %s\n", latok_last_error());
        return 1;
    }
    printf("%d tokens, %d pieces\n", (int)tokens, (int)got);
    for (int i = 0; i < n; ++i) {
        printf("  row %d:", i);
        for (int64_t k = indptr[i]; k < indptr[i + 1]; ++k)
            printf(" %s[%d,%d)", vocab_words[ids[k]], (int)spans[2 * k], (int)spans[2 * k + 1]);
        printf("\n");
    }

    /* the padded form: [CLS] = 2, [SEP] = 3, [PAD] = 0, unknown pieces = [UNK] = 1 */
    int32_t block[n * max_length], lengths[n];
    if (latok_wordpiece_padded_utf8_bytes_batch(buf, off, n, off[n], wp, 1, max_length, 1, 2, 3, 0, block, lengths, NULL, 0, NULL) != LATOK_OK) {
        fprintf(stderr, "latok_wordpiece_padded_utf8_bytes_batch: %s\n", latok_last_error());
        return 1;
    }
    for (int i = 0; i < n; ++i) {
        printf("  input_ids %d (%d used):", i, (int)lengths[i]);
        for (int j = 0; j < max_length; ++j) printf(" %d", (int)block[i * max_length + j]);
        printf("\n");
    }
    latok_wordpiece_destroy(wp);
    latok_shutdown();
    free(ids);
    free(spans);
    free(buf);
    return 0;
}
