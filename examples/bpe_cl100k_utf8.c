/* Minimal C caller of liblatok_hip.so: the cl100k / Llama 3 pre-tokens of a few UTF-8 strings (every byte lies in one: the contraction
 * in either case, the lead space, digits in threes, the newlines behind punctuation), then their byte-level BPE ids against a small
 * vocabulary whose object carries the pre-tokenizer (latok_bpe_create_pretok with LATOK_PRETOK_CL100K; lead_space stays 0).
 *   gcc -std=c99 -Iinclude examples/bpe_cl100k_utf8.c -Llatok_amd -llatok_hip -Wl,-rpath,$PWD/latok_amd -o /tmp/bpe_cl100k_utf8
 * Needs a HIP device at run time (there is no CPU fallback); compiling it only needs the header. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "latok_hip.h"

int main(void) {
    /* ranks 0 .. 14; ids 100 + rank */
    const char* vocab_words[] = {" ", "l", "o", "w", "1", "2", "'", "T", "n", "d", "lo", "low", " low", "'T", "\n"};
    const char* texts[] = {"low  low DON'T!\n\n", "", "1212121 low", "low \xC3\xA9"};
    enum { n_words = 15, n = 4, unk = 99 };
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

    if (latok_init(0) != LATOK_OK) {
        fprintf(stderr, "latok_init: %s\n", latok_last_error());
        return 1;
    }
    /* the pre-tokens: a string of L bytes has at most L */
    int64_t counts[n], n_pre = 0;
    int64_t* pre = (int64_t*)malloc((size_t)(off[n] + 1) * 2 * sizeof(int64_t));
    if (latok_pretokens_utf8_bytes_batch(buf, off, n, off[n], LATOK_PRETOK_CL100K, counts, pre, off[n], &n_pre, 0, NULL) != LATOK_OK) {
        fprintf(stderr, "latok_pretokens_utf8_bytes_batch: %s\n", latok_last_error());
        return 1;
    }
    for (int64_t i = 0, k = 0; i < n; ++i) {
        printf("  row %d:", (int)i);
        for (int64_t j = 0; j < counts[i]; ++j, ++k) printf(" [%d,%d)", (int)pre[2 * k], (int)pre[2 * k + 1]);
        printf("\n");
    }

    latok_bpe* bpe = NULL;
    int pretok = -1;
    if (latok_bpe_create_pretok((const uint8_t*)words, word_off, n_words, word_ids, 4096, 0, LATOK_PRETOK_CL100K, 0u, &bpe) != LATOK_OK ||
        latok_bpe_pretokenizer(bpe, &pretok) != LATOK_OK || pretok != LATOK_PRETOK_CL100K) {
        fprintf(stderr, "latok_bpe_create_pretok: %s\n", latok_last_error());
        return 1;
    }
    /* size query, then the call; the calls are latok_bpe_create's: they dispatch on the object */
    int64_t indptr[n + 1], need = 0, got = 0, tokens = 0;
    int rc = latok_bpe_ids_utf8_bytes_batch(buf, off, n, off[n], bpe, unk, indptr, NULL, NULL, 0, &need, &tokens, 0, NULL);
    if (rc != LATOK_OK && need == 0) {
        fprintf(stderr, "latok_bpe_ids_utf8_bytes_batch: %s\n", latok_last_error());
        return 1;
    }
    int32_t* ids = (int32_t*)malloc((size_t)(need + 1) * sizeof(int32_t));
    if (latok_bpe_ids_utf8_bytes_batch(buf, off, n, off[n], bpe, unk, indptr, ids, NULL, need, &got, &tokens, 0, NULL) != LATOK_OK || got != need) {
        fprintf(stderr, "latok_bpe_ids_utf8_bytes_batch: %s\n", latok_last_error());
        return 1;
    }
    printf("%d pre-tokens, %d pieces\n", (int)tokens, (int)got);
    for (int i = 0; i < n; ++i) {
        printf("  row %d:", i);
        for (int64_t k = indptr[i]; k < indptr[i + 1]; ++k) printf(" %d", (int)ids[k]);
        printf("\n");
    }
    latok_bpe_destroy(bpe);
    latok_shutdown();
    free(ids);
    free(pre);
    free(buf);
    return 0;
}
