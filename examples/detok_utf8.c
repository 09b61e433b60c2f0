/* Minimal C caller of liblatok_hip.so: a round trip on the device.  A few UTF-8 strings are cut into byte-level BPE ids
 * (latok_bpe_ids_utf8_bytes_batch with LATOK_DEVICE_PTRS: text in, indptr and ids out, all in device memory) and the resident ids are
 * decoded back to bytes by latok_detok_csr, again with device pointers: a size query, then the call.  No id visits the host; only the
 * decoded bytes and their row offsets are copied down for printing.
 *   gcc -std=c99 -Iinclude examples/detok_utf8.c -Llatok_amd -llatok_hip -Wl,-rpath,$PWD/latok_amd -o /tmp/detok_utf8
 * Needs a HIP device at run time (there is no CPU fallback); compiling it only needs the header. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "latok_hip.h"

static int fail(const char* what) {
    fprintf(stderr, "%s: %s\n", what, latok_last_error());
    return 1;
}

int main(void) {
    /* ranks 0 .. 13 of a small GPT-style vocabulary (lead_space = 1: a word after a space carries that space); ids 100 + rank */
    const char* vocab_words[] = {" ", "l", "o", "w", "e", "r", "s", "t", "lo", "low", " low", "er", "es", "est"};
    const char* texts[] = {"low lower lowest", "slowest low", "", "lowers"};
    enum { n_words = 14, n = 4, unk = 99 };
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
    latok_detok* detok = NULL;
    if (latok_init(0) != LATOK_OK) return fail("latok_init");
    if (latok_bpe_create((const uint8_t*)words, word_off, n_words, word_ids, 4096, 1, 0u, &bpe) != LATOK_OK) return fail("latok_bpe_create");
    if (latok_detok_create((const uint8_t*)words, word_off, n_words, word_ids, LATOK_DETOK_CONCAT, NULL, 0, 0, &detok) != LATOK_OK)
        return fail("latok_detok_create");

    /* the batch on the device; a piece has at least one byte, so off[n] ids are room enough */
    const size_t cap = (size_t)off[n];
    uint8_t* d_text = (uint8_t*)latok_dev_alloc(cap + 16);
    int64_t* d_off = (int64_t*)latok_dev_alloc(sizeof(off));
    int64_t* d_indptr = (int64_t*)latok_dev_alloc(sizeof(off));
    int32_t* d_ids = (int32_t*)latok_dev_alloc(cap * sizeof(int32_t) + 16);
    int64_t* d_out_off = (int64_t*)latok_dev_alloc(sizeof(off));
    if (!d_text || !d_off || !d_indptr || !d_ids || !d_out_off) return fail("latok_dev_alloc");
    if (latok_memcpy_h2d(d_text, buf, cap) != LATOK_OK || latok_memcpy_h2d(d_off, off, sizeof(off)) != LATOK_OK) return fail("latok_memcpy_h2d");

    int64_t n_pieces = 0;
    if (latok_bpe_ids_utf8_bytes_batch(d_text, d_off, n, off[n], bpe, unk, d_indptr, d_ids, NULL, (int64_t)cap, &n_pieces, NULL, LATOK_DEVICE_PTRS, NULL) !=
        LATOK_OK)
        return fail("latok_bpe_ids_utf8_bytes_batch");

    /* decode the resident ids: the size query (no byte buffer, capacity 0) leaves out_off valid and reports the need */
    int64_t need = 0, got = 0, unknown = 0;
    int rc = latok_detok_csr(detok, d_indptr, d_ids, n, n_pieces, NULL, 0, NULL, 0, d_out_off, &need, &unknown, LATOK_DEVICE_PTRS, NULL);
    if (rc != LATOK_OK && need == 0) return fail("latok_detok_csr");
    uint8_t* d_out = (uint8_t*)latok_dev_alloc((size_t)need + 16);
    if (!d_out) return fail("latok_dev_alloc");
    if (latok_detok_csr(detok, d_indptr, d_ids, n, n_pieces, NULL, 0, d_out, need, d_out_off, &got, &unknown, LATOK_DEVICE_PTRS, NULL) != LATOK_OK ||
        got != need)
        return fail("latok_detok_csr");

    int64_t out_off[n + 1];
    char* out = (char*)malloc((size_t)need + 1);
    if (latok_memcpy_d2h(out_off, d_out_off, sizeof(out_off)) != LATOK_OK || latok_memcpy_d2h(out, d_out, (size_t)need) != LATOK_OK)
        return fail("latok_memcpy_d2h");
    printf("%d pieces, %d bytes, %d unknown\n", (int)n_pieces, (int)got, (int)unknown);
    for (int i = 0; i < n; ++i) printf("  row %d: '%.*s'\n", i, (int)(out_off[i + 1] - out_off[i]), out + out_off[i]);

    latok_dev_free(d_out);
    latok_dev_free(d_out_off);
    latok_dev_free(d_ids);
    latok_dev_free(d_indptr);
    latok_dev_free(d_off);
    latok_dev_free(d_text);
    latok_detok_destroy(detok);
    latok_bpe_destroy(bpe);
    latok_shutdown();
    free(out);
    free(buf);
    return 0;
}
