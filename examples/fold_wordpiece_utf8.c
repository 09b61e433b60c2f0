/* Minimal C caller of liblatok_hip.so: an UNCASED WordPiece vocabulary.  The batch is uploaded once, folded on the device
 * (latok_fold_utf8_bytes_batch: lower-cased, accents stripped) with device pointers, and the folded bytes -- they never visit the
 * host -- go straight to latok_wordpiece_padded_utf8_bytes_batch, which writes the [n, 10] block with [CLS] / [SEP] a model takes.
 *   gcc -std=c99 -Iinclude examples/fold_wordpiece_utf8.c -Llatok_amd -llatok_hip -Wl,-rpath,$PWD/latok_amd -o /tmp/fold_wordpiece_utf8
 * Needs a HIP device at run time (there is no CPU fallback); compiling it only needs the header. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "latok_hip.h"

int main(void) {
    const char* vocab_words[] = {"[PAD]", "[UNK]", "[CLS]", "[SEP]", "un", "##aff", "##able", "cafe", "is", "this", "!", "resume"};
    const char* texts[] = {"This IS Unaffable !", "CAF\xC3\x89 caf\xC3\xA9 Cafe\xCC\x81", "", "R\xC3\xA9sum\xC3\xA9 \xC3\x9CNAFFABLE"};
    enum { n_words = 12, n = 4, max_length = 10 };
    char words[256];
    int64_t word_off[n_words + 1] = {0}, off[n + 1] = {0};
    for (int i = 0; i < n_words; ++i) {
        memcpy(words + word_off[i], vocab_words[i], strlen(vocab_words[i]));
        word_off[i + 1] = word_off[i] + (int64_t)strlen(vocab_words[i]);
    }
    for (int i = 0; i < n; ++i) off[i + 1] = off[i] + (int64_t)strlen(texts[i]);
    const int64_t total = off[n];
    uint8_t* buf = (uint8_t*)malloc((size_t)total + 1);
    for (int i = 0; i < n; ++i) memcpy(buf + off[i], texts[i], (size_t)(off[i + 1] - off[i]));

    latok_wordpiece* wp = NULL;
    if (latok_init(0) != LATOK_OK ||
        latok_wordpiece_create((const uint8_t*)words, word_off, n_words, NULL, (const uint8_t*)"##", 2, 100, 0u, &wp) != LATOK_OK) {
        fprintf(stderr, "latok_init / latok_wordpiece_create: %s\n", latok_last_error());
        return 1;
    }
    /* device buffers (latok_dev_alloc returns 16-byte aligned memory): the batch, the folded batch (at most 3 x the bytes), the block */
    uint8_t* d_in = (uint8_t*)latok_dev_alloc((size_t)total + 16);
    int64_t* d_off = (int64_t*)latok_dev_alloc(sizeof off);
    uint8_t* d_fold = (uint8_t*)latok_dev_alloc((size_t)(3 * total) + 16);
    int64_t* d_fold_off = (int64_t*)latok_dev_alloc(sizeof off);
    int32_t* d_block = (int32_t*)latok_dev_alloc(sizeof(int32_t) * n * max_length);
    int32_t* d_len = (int32_t*)latok_dev_alloc(sizeof(int32_t) * n);
    if (!d_in || !d_off || !d_fold || !d_fold_off || !d_block || !d_len || latok_memcpy_h2d(d_in, buf, (size_t)total) != LATOK_OK ||
        latok_memcpy_h2d(d_off, off, sizeof off) != LATOK_OK) {
        fprintf(stderr, "device buffers: %s\n", latok_last_error());
        return 1;
    }
    int64_t folded = 0;
    if (latok_fold_utf8_bytes_batch(d_in, d_off, n, total, LATOK_FOLD_LOWER | LATOK_FOLD_STRIP_MARKS, d_fold, 3 * total, d_fold_off, &folded,
                                    LATOK_DEVICE_PTRS, NULL) != LATOK_OK) {
        fprintf(stderr, "latok_fold_utf8_bytes_batch: %s\n", latok_last_error());
        return 1;
    }
    /* the padded form on the folded bytes: [CLS] = 2, [SEP] = 3, [PAD] = 0, unknown pieces = [UNK] = 1 */
    if (latok_wordpiece_padded_utf8_bytes_batch(d_fold, d_fold_off, n, folded, wp, 1, max_length, 1, 2, 3, 0, d_block, d_len, NULL,
                                                LATOK_DEVICE_PTRS, NULL) != LATOK_OK) {
        fprintf(stderr, "latok_wordpiece_padded_utf8_bytes_batch: %s\n", latok_last_error());
        return 1;
    }
    int32_t block[n * max_length], lengths[n];
    if (latok_memcpy_d2h(block, d_block, sizeof block) != LATOK_OK || latok_memcpy_d2h(lengths, d_len, sizeof lengths) != LATOK_OK) {
        fprintf(stderr, "latok_memcpy_d2h: %s\n", latok_last_error());
        return 1;
    }
    printf("%d bytes in, %d folded\n", (int)total, (int)folded);
    for (int i = 0; i < n; ++i) {
        printf("  input_ids %d (%d used):", i, (int)lengths[i]);
        for (int j = 0; j < max_length; ++j) printf(" %d", (int)block[i * max_length + j]);
        printf("\n");
    }
    latok_dev_free(d_in);
    latok_dev_free(d_off);
    latok_dev_free(d_fold);
    latok_dev_free(d_fold_off);
    latok_dev_free(d_block);
    latok_dev_free(d_len);
    latok_wordpiece_destroy(wp);
    latok_shutdown();
    free(buf);
    return 0;
}
