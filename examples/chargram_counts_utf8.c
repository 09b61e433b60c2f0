/* Minimal C caller of liblatok_hip.so: the character trigrams inside the tokens of a few UTF-8 strings (scikit-learn's
 * analyzer="char_wb") as the CSR rows of a document-term matrix -- against a vocabulary whose words may hold the pad (" th"), and
 * hashed into 16 columns with alternating signs.  Every token is padded with one space on both sides; the grams are cut, looked up or
 * hashed, sorted and reduced on the device: first a size query, then the call.
 *   gcc -std=c99 -Iinclude examples/chargram_counts_utf8.c -Llatok_amd -llatok_hip -Wl,-rpath,$PWD/latok_amd -o /tmp/chargram_counts_utf8
 * Needs a HIP device at run time (there is no CPU fallback); compiling it only needs the header. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "latok_hip.h"

static void print_rows(const char* what, int64_t n, const int64_t* indptr, const int32_t* indices, const int32_t* data, const int64_t* oov) {
    printf("%s\n", what);
    for (int64_t i = 0; i < n; ++i) {
        printf("  row %d:", (int)i);
        for (int64_t k = indptr[i]; k < indptr[i + 1]; ++k) printf(" %d:%d", (int)indices[k], (int)data[k]);
        if (oov) printf("   (oov %d)", (int)oov[i]);
        printf("\n");
    }
}

int main(void) {
    const char* vocab_words[] = {" th", "the", "he ", " a ", "her"};
    const char* texts[] = {"the other theme", "a the", "", "there"};
    const int64_t n_words = 5, n = 4;
    const int min_n = 3, max_n = 3, pad = ' ';
    char words[128];
    int64_t word_off[6] = {0}, off[5] = {0};
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
    /* size query: no entry buffers, capacity 0 -- indptr and oov are valid already, the call reports the number of entries */
    int64_t indptr[5], oov[4], need = 0, got = 0, grams = 0;
    int rc = latok_chargram_counts_utf8_bytes_batch(buf, off, n, off[n], vocab, min_n, max_n, pad, indptr, oov, NULL, NULL, 0, &need, &grams, 0, NULL);
    if (rc != LATOK_OK && need == 0) {
        fprintf(stderr, "latok_chargram_counts_utf8_bytes_batch: %s\n", latok_last_error());
        return 1;
    }
    int32_t* indices = (int32_t*)malloc((size_t)(need + 1) * sizeof(int32_t));
    int32_t* data = (int32_t*)malloc((size_t)(need + 1) * sizeof(int32_t));
    if (latok_chargram_counts_utf8_bytes_batch(buf, off, n, off[n], vocab, min_n, max_n, pad, indptr, oov, indices, data, need, &got, &grams, 0,
                                               NULL) != LATOK_OK ||
        got != need) {
        fprintf(stderr, "latok_chargram_counts_utf8_bytes_batch: %s\n", latok_last_error());
        return 1;
    }
    printf("%d grams, %d entries\n", (int)grams, (int)got);
    print_rows("vocabulary ids (id:count)", n, indptr, indices, data, oov);
    free(indices);
    free(data);

    /* the hashed form: a gram has at most one entry, so the gram total bounds the entries */
    indices = (int32_t*)malloc((size_t)(grams + 1) * sizeof(int32_t));
    data = (int32_t*)malloc((size_t)(grams + 1) * sizeof(int32_t));
    if (latok_hashed_chargram_counts_utf8_bytes_batch(buf, off, n, off[n], 0u, 16, 1, min_n, max_n, pad, indptr, indices, data, grams, &got, NULL, 0,
                                                      NULL) != LATOK_OK) {
        fprintf(stderr, "latok_hashed_chargram_counts_utf8_bytes_batch: %s\n", latok_last_error());
        return 1;
    }
    print_rows("hashed into 16 columns, alternating signs (column:sum)", n, indptr, indices, data, NULL);
    latok_vocab_destroy(vocab);
    latok_shutdown();
    free(indices);
    free(data);
    free(buf);
    return 0;
}
