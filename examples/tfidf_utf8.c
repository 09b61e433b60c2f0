/* Minimal C caller of liblatok_hip.so: TF-IDF rows of UTF-8 strings against a small vocabulary.  A FIT pass feeds two batches to a
 * latok_idf (document frequencies, counted on the device straight from the text); a TRANSFORM pass turns a third batch into CSR rows
 * whose data is tf * idf over the row's L2 norm -- TfidfVectorizer(vocabulary=...).fit(...).transform(...) without a count leaving the
 * device: first a size query, then the call.
 *   gcc -std=c99 -Iinclude examples/tfidf_utf8.c -Llatok_amd -llatok_hip -Wl,-rpath,$PWD/latok_amd -o /tmp/tfidf_utf8
 * Needs a HIP device at run time (there is no CPU fallback); compiling it only needs the header. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "latok_hip.h"

/* strings back to back and their byte offsets; returns the total */
static int64_t pack(const char** texts, int n, uint8_t* buf, int64_t* off) {
    off[0] = 0;
    for (int i = 0; i < n; ++i) {
        memcpy(buf + off[i], texts[i], strlen(texts[i]));
        off[i + 1] = off[i] + (int64_t)strlen(texts[i]);
    }
    return off[n];
}

int main(void) {
    const char* vocab_words[] = {"the", "cat", "sat", "on", "mat", "dog"};
    const char* fit_a[] = {"the cat sat on the mat", "the dog sat"};
    const char* fit_b[] = {"the cat", "", "a dog on the mat"};
    const char* docs[] = {"the cat sat on the cat", "unknown words only", "dog"};
    const int64_t n_words = 6;
    uint8_t words[64], buf[256];
    int64_t word_off[7], off[8];
    pack(vocab_words, (int)n_words, words, word_off);

    latok_vocab* vocab = NULL;
    latok_idf* idf = NULL;
    if (latok_init(0) != LATOK_OK || latok_vocab_create(words, word_off, n_words, NULL, 0u, &vocab) != LATOK_OK ||
        latok_idf_create(n_words, &idf) != LATOK_OK) {
        fprintf(stderr, "setup: %s\n", latok_last_error());
        return 1;
    }
    /* fit: one update per batch; min_n = max_n = 1 are the plain term counts */
    int64_t total = pack(fit_a, 2, buf, off);
    int rc = latok_idf_update_utf8_bytes_batch(buf, off, 2, total, vocab, 0u, 0, 1, 1, ' ', idf, NULL, NULL, 0, NULL);
    total = pack(fit_b, 3, buf, off);
    if (rc == LATOK_OK) rc = latok_idf_update_utf8_bytes_batch(buf, off, 3, total, vocab, 0u, 0, 1, 1, ' ', idf, NULL, NULL, 0, NULL);
    int32_t df[6];
    float weights[6];
    int64_t n_docs = 0;
    if (rc != LATOK_OK || latok_idf_read(idf, df, n_words, &n_docs) != LATOK_OK || latok_idf_weights(idf, 1, weights, n_words) != LATOK_OK) {
        fprintf(stderr, "fit: %s\n", latok_last_error());
        return 1;
    }
    printf("%d documents\n", (int)n_docs);
    for (int i = 0; i < n_words; ++i) printf("  %-4s df %d idf %.6f\n", vocab_words[i], (int)df[i], weights[i]);

    /* transform: size query (indptr and oov are valid already), then the entries */
    const int opts = LATOK_TFIDF_SMOOTH_IDF | LATOK_TFIDF_NORM_L2;
    const int64_t n = 3;
    int64_t indptr[4], oov[3], need = 0, got = 0;
    total = pack(docs, (int)n, buf, off);
    rc = latok_tfidf_utf8_bytes_batch(buf, off, n, total, vocab, 1, 1, ' ', idf, opts, indptr, oov, NULL, NULL, 0, &need, 0, NULL);
    if (rc != LATOK_OK && need == 0) {
        fprintf(stderr, "latok_tfidf_utf8_bytes_batch: %s\n", latok_last_error());
        return 1;
    }
    int32_t* indices = (int32_t*)malloc((size_t)(need + 1) * sizeof(int32_t));
    float* data = (float*)malloc((size_t)(need + 1) * sizeof(float));
    if (latok_tfidf_utf8_bytes_batch(buf, off, n, total, vocab, 1, 1, ' ', idf, opts, indptr, oov, indices, data, need, &got, 0, NULL) != LATOK_OK ||
        got != need) {
        fprintf(stderr, "latok_tfidf_utf8_bytes_batch: %s\n", latok_last_error());
        return 1;
    }
    for (int64_t i = 0; i < n; ++i) {
        printf("  row %d:", (int)i);
        for (int64_t k = indptr[i]; k < indptr[i + 1]; ++k) printf(" %s:%.6f", vocab_words[indices[k]], data[k]);
        printf("   (oov %d)\n", (int)oov[i]);
    }
    free(indices);
    free(data);
    latok_idf_destroy(idf);
    latok_vocab_destroy(vocab);
    latok_shutdown();
    return 0;
}
