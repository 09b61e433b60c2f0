/* UTF-8 batches through the batch flow with results in CODE-POINT units (include/latok_hip.h: latok_flow_split_offsets_utf8):
 * the positions the reference reports for the decoded str (latok/core/default_tokenizer.py:137-160 reads code points,
 * latok.c:53-55,79), from bytes that stay UTF-8 in device memory.  Two batches are submitted back to back and nothing waits
 * until latok_flow_wait; then the four result words of each are read: item total, error word, code-point total, and the
 * malformed-input flag.  The second batch holds a stray continuation byte: the flow REPORTS that (result[3] != 0, nothing of the
 * batch is valid) and the caller resubmits it through the blocking call, which has the staged decoder.
 *   gcc -std=c99 -Iinclude examples/flow_utf8_codepoints.c -Llatok_amd -llatok_hip -Wl,-rpath,$PWD/latok_amd -o /tmp/flow_utf8 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "latok_hip.h"

#define N_BATCH 2
#define MAX_STR 4
#define CHECK(call)                                                          \
    do {                                                                     \
        if ((call) != LATOK_OK) {                                            \
            fprintf(stderr, "%s: %s\n", #call, latok_last_error());          \
            return 1;                                                        \
        }                                                                    \
    } while (0)

typedef struct {
    const char* const* texts;
    int n;
    int64_t byte_off[MAX_STR + 1];
    void *d_u8, *d_off, *d_counts, *d_offsets, *d_result;
    int64_t cap;
} batch_t;

int main(void) {
    static const char* const b0[] = {"caf\xC3\xA9 \xE6\x97\xA5\xE6\x9C\xAC\xE8\xAA\x9E #tag", "", "\xF0\x9F\xA4\x93 me@x.org"};
    static const char* const b1[] = {"fine", "a\x80\x80\x80\x80 stray continuation bytes"};
    batch_t B[N_BATCH] = {{b0, 3}, {b1, 2}};
    CHECK(latok_init(0));
    for (int k = 0; k < N_BATCH; ++k) {
        batch_t* b = &B[k];
        b->byte_off[0] = 0;
        for (int i = 0; i < b->n; ++i) b->byte_off[i + 1] = b->byte_off[i] + (int64_t)strlen(b->texts[i]);
        const int64_t bytes = b->byte_off[b->n];
        char* joined = (char*)malloc((size_t)bytes + 1);
        for (int i = 0; i < b->n; ++i) memcpy(joined + b->byte_off[i], b->texts[i], strlen(b->texts[i]));
        b->cap = bytes;                                  /* a batch has at most one boundary per byte */
        b->d_u8 = latok_dev_alloc((size_t)bytes + 16);
        b->d_off = latok_dev_alloc((size_t)(b->n + 1) * 8);
        b->d_counts = latok_dev_alloc((size_t)b->n * 4 + 16);
        b->d_offsets = latok_dev_alloc((size_t)b->cap * 4 + 16);
        b->d_result = latok_dev_alloc(32);               /* int64[4] */
        if (!b->d_u8 || !b->d_off || !b->d_counts || !b->d_offsets || !b->d_result) return 1;
        CHECK(latok_memcpy_h2d(b->d_u8, joined, (size_t)bytes));
        CHECK(latok_memcpy_h2d(b->d_off, b->byte_off, (size_t)(b->n + 1) * 8));
        free(joined);
    }
    for (int k = 0; k < N_BATCH; ++k)                    /* submit both, wait once */
        CHECK(latok_flow_split_offsets_utf8((const uint8_t*)B[k].d_u8, (const int64_t*)B[k].d_off, B[k].n, B[k].byte_off[B[k].n], B[k].d_counts,
                                            B[k].d_offsets, B[k].cap, (int64_t*)B[k].d_result, LATOK_OUT_INT32));
    CHECK(latok_flow_wait());
    for (int k = 0; k < N_BATCH; ++k) {
        batch_t* b = &B[k];
        int64_t result[4], n_items = 0;
        CHECK(latok_memcpy_d2h(result, b->d_result, 32));
        if (result[1] != 0) {
            fprintf(stderr, "batch %d: error word %lld\n", k, (long long)result[1]);
            return 1;
        }
        printf("batch %d: %lld code points, %s\n", k, (long long)result[2], result[3] ? "malformed -> blocking call" : "well formed");
        if (result[3] != 0) {                            /* reported, not decoded: the blocking call decodes it */
            CHECK(latok_split_offsets_utf8_batch((const uint8_t*)b->d_u8, (const int64_t*)b->d_off, b->n, b->byte_off[b->n], (int64_t*)b->d_counts,
                                                 (int64_t*)b->d_offsets, b->cap, &n_items, LATOK_DEVICE_PTRS | LATOK_OUT_INT32, NULL));
        } else {
            n_items = result[0];
        }
        int32_t counts[MAX_STR];
        int32_t* offsets = (int32_t*)malloc((size_t)(n_items > 0 ? n_items : 1) * 4);
        CHECK(latok_memcpy_d2h(counts, b->d_counts, (size_t)b->n * 4));
        if (n_items > 0) CHECK(latok_memcpy_d2h(offsets, b->d_offsets, (size_t)n_items * 4));
        int64_t t = 0;
        for (int i = 0; i < b->n; ++i) {
            printf("%d.%d:", k, i);
            for (int c = 0; c < counts[i]; ++c, ++t) printf(" %d", (int)offsets[t]);
            printf("\n");
        }
        free(offsets);
        latok_dev_free(b->d_u8); latok_dev_free(b->d_off); latok_dev_free(b->d_counts); latok_dev_free(b->d_offsets); latok_dev_free(b->d_result);
    }
    CHECK(latok_shutdown());
    return 0;
}
