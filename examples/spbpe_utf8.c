/* Minimal C caller of liblatok_hip.so: SentencePiece's segments of a few UTF-8 strings (a lead run of spaces, then what follows up to the
 * next space; nothing is dropped), then their SentencePiece BPE ids against a small vocabulary with byte fallback (latok_bpe_create_spm):
 * characters are merged, U+2581 (E2 96 81) stands for a space, one more stands in front of every string, and a character that no word
 * covers becomes one piece per byte.
 *   gcc -std=c99 -Iinclude examples/spbpe_utf8.c -Llatok_amd -llatok_hip -Wl,-rpath,$PWD/latok_amd -o /tmp/spbpe_utf8
 * Needs a HIP device at run time (there is no CPU fallback); compiling it only needs the header. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "latok_hip.h"

#define M "\xE2\x96\x81"

int main(void) {
    /* ranks 0 .. 11; ids 300 + rank; the byte pieces are ids 3 .. 258 as in Llama 2's model */
    const char* vocab_words[] = {M "l", "lo", M "lo", M "low", M M, "l", "o", "w", M, "e", "r", "er"};
    const char* texts[] = {"low  lower", "", "   ", "low \xC3\xA9"};
    enum { n_words = 12, n = 4, unk = 0 };
    char words[256];
    int64_t word_off[n_words + 1] = {0}, off[n + 1] = {0};
    int32_t word_ids[n_words], byte_ids[256];
    for (int i = 0; i < n_words; ++i) {
        memcpy(words + word_off[i], vocab_words[i], strlen(vocab_words[i]));
        word_off[i + 1] = word_off[i] + (int64_t)strlen(vocab_words[i]);
        word_ids[i] = 300 + i;
    }
    for (int b = 0; b < 256; ++b) byte_ids[b] = 3 + b;
    for (int i = 0; i < n; ++i) off[i + 1] = off[i] + (int64_t)strlen(texts[i]);
    uint8_t* buf = (uint8_t*)malloc((size_t)off[n] + 1);
    for (int i = 0; i < n; ++i) memcpy(buf + off[i], texts[i], (size_t)(off[i + 1] - off[i]));

    if (latok_init(0) != LATOK_OK) {
        fprintf(stderr, "latok_init: %s\n", latok_last_error());
        return 1;
    }
    /* the segments: a string of L bytes has at most L */
    int64_t counts[n], n_seg = 0;
    int64_t* seg = (int64_t*)malloc((size_t)(off[n] + 1) * 2 * sizeof(int64_t));
    if (latok_pretokens_utf8_bytes_batch(buf, off, n, off[n], LATOK_PRETOK_SPM, counts, seg, off[n], &n_seg, 0, NULL) != LATOK_OK) {
        fprintf(stderr, "latok_pretokens_utf8_bytes_batch: %s\n", latok_last_error());
        return 1;
    }
    for (int64_t i = 0, k = 0; i < n; ++i) {
        printf("  row %d:", (int)i);
        for (int64_t j = 0; j < counts[i]; ++j, ++k) printf(" [%d,%d)", (int)seg[2 * k], (int)seg[2 * k + 1]);
        printf("\n");
    }

    latok_bpe* bpe = NULL;
    int pretok = -1, fallback = 0, dummy = 0, fuse = 0;
    if (latok_bpe_create_spm((const uint8_t*)words, word_off, n_words, word_ids, byte_ids, 1, 0, 4096, 0u, &bpe) != LATOK_OK ||
        latok_bpe_pretokenizer(bpe, &pretok) != LATOK_OK || pretok != LATOK_PRETOK_SPM ||
        latok_bpe_spm_info(bpe, &fallback, &dummy, &fuse) != LATOK_OK || !fallback || !dummy) {
        fprintf(stderr, "latok_bpe_create_spm: %s\n", latok_last_error());
        return 1;
    }
    /* size query, then the call; the calls are latok_bpe_create's: they dispatch on the object.  A batch of this kind may have more
     * pieces than bytes (the dummy prefix, byte fallback of a marker): always take the size from the query */
    int64_t indptr[n + 1], need = 0, got = 0, segments = 0;
    int rc = latok_bpe_ids_utf8_bytes_batch(buf, off, n, off[n], bpe, unk, indptr, NULL, NULL, 0, &need, &segments, 0, NULL);
    if (rc != LATOK_OK && need == 0) {
        fprintf(stderr, "latok_bpe_ids_utf8_bytes_batch: %s\n", latok_last_error());
        return 1;
    }
    int32_t* ids = (int32_t*)malloc((size_t)(need + 1) * sizeof(int32_t));
    int64_t* spans = (int64_t*)malloc((size_t)(need + 1) * 2 * sizeof(int64_t));
    if (latok_bpe_ids_utf8_bytes_batch(buf, off, n, off[n], bpe, unk, indptr, ids, spans, need, &got, &segments, 0, NULL) != LATOK_OK || got != need) {
        fprintf(stderr, "latok_bpe_ids_utf8_bytes_batch: %s\n", latok_last_error());
        return 1;
    }
    printf("%d segments, %d pieces\n", (int)segments, (int)got);
    for (int i = 0; i < n; ++i) {
        printf("  row %d:", i);
        for (int64_t k = indptr[i]; k < indptr[i + 1]; ++k) printf(" %d[%d,%d)", (int)ids[k], (int)spans[2 * k], (int)spans[2 * k + 1]);
        printf("\n");
    }
    latok_bpe_destroy(bpe);
    latok_shutdown();
    free(spans);
    free(ids);
    free(seg);
    free(buf);
    return 0;
}
