// ngram_kernels.hip -- word n-grams of a UTF-8 batch in byte space: one term key (term_key.h) per gram, the kernels behind
// latok_ngram_counts_utf8_bytes_batch and latok_hashed_ngram_counts_utf8_bytes_batch.  They work in TOKEN space, as the WordPiece
// kernels do.  SpanRecords of scatter_block (compact_kernels.hip) has left the int64 span record of every token at its rank in
// the workspace and the token count c_s of every string; the chained scan the row starts in token space (row_start[n_str + 1]).
//
//   k_ngram_rows   K_s = sum over n in [min_n, max_n] of max(0, c_s - n + 1): the grams of string s.  The chained scan of the
//                  n_str + 1 entries (the last is 0) gives the row starts in KEY space and the key total K.
//   k_ngram_keys   one lane per token t.  The lane takes its string s (lane_token of block_ops.h; the checked record load of the
//                  tokens it walks is token_bytes there) and its index j = t - row_start[s] in the row.  It walks
//                  the tokens j .. min(j + max_n, c_s) - 1 ONCE with the streaming hash of ngram_text.h -- separator, token, finish
//                  -- and behind token j + n - 1 stores the key of the gram g(n, j) if n >= min_n: tk_hashed_key of the hash, or
//                  tk_vocab_probe with ng_equal over the gram's span records (which walks the gram again, only where hash and
//                  length agree).
//   the bijection  the grams of a row lie order by order: key_start[s] + (sum over m in [min_n, n) of (c_s - m + 1)) + j holds
//                  g(n, j).  Order n has c_s - n + 1 grams, j = 0 .. c_s - n, so the orders' ranges are disjoint and fill
//                  [key_start[s], key_start[s + 1]) exactly; the reduce sorts inside the row, so the order inside it is free.
// A lane whose grams are long or whose probes collide keeps its wave busy while the others idle: accepted in this version, as in
// WordPiece; there is no whole-wave form for long tokens.  Every loop runs by its own counter: the walk at most max_n <= kNgMax
// tokens, a token's dwords, a probe at most n_slots steps.  A key is stored only inside [0, n_keys), a record read only inside
// [0, n_tok) (the walk ends with the batch's last token), the text only where a checked record says -- whatever the workspace holds;
// the string's part of the argument stands at lane_token of block_ops.h.  Table and blob are read with ordinary cached loads, the
// text as aligned dwords up to the one that holds a token's last byte.  No kernel here waits for another workgroup; all stores are
// vector stores from plain C++.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_ops.h"
#include "kernels.h"
#include "ngram_text.h"
#include "term_key.h"

namespace latok {

// grams of a string of c tokens
__device__ __forceinline__ int64_t ng_row_keys(int64_t c, int min_n, int max_n) {
    int64_t k = 0;
    for (int n = min_n; n <= max_n; ++n) k += c >= n ? c - n + 1 : 0;
    return k;
}

__global__ __launch_bounds__(256) void k_ngram_rows(const int64_t* __restrict__ tok_cnt, int64_t n_str, int min_n, int max_n,
                                                    int64_t* __restrict__ key_cnt) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s > n_str) return;
    key_cnt[s] = s < n_str ? ng_row_keys(tok_cnt[s], min_n, max_n) : 0;   // (the entry behind the last string)
}

template <bool VOCAB>
__global__ __launch_bounds__(kNgBlock) void k_ngram_keys(GramKeys P) {
    const LaneToken me = lane_token<kNgBlock>(P.t);
    const int64_t t = me.t, r = me.row, base = me.base, n_tok = P.t.n_tok;
    if (t >= n_tok) return;
    const int64_t rs = P.t.row_start[r], c = P.t.row_start[r + 1] - rs, j = t - rs;
    if (j < 0 || j >= c || base < 0) return;   // (cannot happen with row starts from the scan)
    int64_t left = c - j;                       // tokens from mine to the row's end ...
    if (left > n_tok - t) left = n_tok - t;
    const int n_walk = left < P.max_n ? (int)left : P.max_n;   // ... of which the walk takes at most max_n <= kNgMax
    const uint32_t* const text = P.t.text;
    const int64_t total = P.t.total;
    const int64_t* const tok_spans = P.t.tok_spans;
    auto ld = [text](int64_t i) { return text[i]; };
    // token k of my grams, absolute; a record that does not lie inside the text is an empty token: nothing of it is read
    auto span = [tok_spans, t, base, total](int k) {
        const TokenBytes b = token_bytes(tok_spans, t + k, base, total);
        return b.ok ? NgSpan{b.a, b.e} : NgSpan{0, 0};
    };
    const VtSlot* const slots = reinterpret_cast<const VtSlot*>(P.form.vt.slots);
    const uint32_t* const blob = P.form.vt.blob;
    const uint32_t sep = P.joiner;
    NgHash st = ng_hash_init(P.form.seed);
    int64_t at = P.rank[r] + j;   // where g(n, j) goes: the orders before n add their c - m + 1 each
    for (int n = 1; n <= n_walk; ++n) {
        if (n > 1) ng_hash_byte(st, sep);
        const NgSpan tok = span(n - 1);
        ng_hash_token(st, ld, tok.a, tok.e);
        if (n < P.min_n) continue;
        const uint32_t h = ng_hash_finish(st);
        uint64_t key;
        if (VOCAB) {
            const uint32_t len = st.s.len;
            key = tk_vocab_probe([slots](uint64_t i) { return slots[i]; }, P.form.vt.n_slots, h, len, [&](uint32_t off) {
                return ng_equal(ld, span, n, sep, [blob](uint64_t i) { return blob[i]; }, off, len);
            });
        } else {
            key = tk_hashed_key(h, P.form.n_features, P.form.alternate_sign);
        }
        if (at >= 0 && at < P.n_keys) P.keys[at] = key;
        at += c - n + 1;
    }
}

// ---- launchers -----------------------------------------------------------------------------------------------------
hipError_t launch_ngram_rows(const int64_t* tok_cnt, int64_t n_str, int min_n, int max_n, int64_t* key_cnt, hipStream_t st) {
    if (n_str <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_ngram_rows, dim3((unsigned)((n_str + 256) / 256)), dim3(256), 0, st, tok_cnt, n_str, min_n, max_n, key_cnt);
    return hipGetLastError();
}

hipError_t launch_ngram_keys(const GramKeys& P, hipStream_t st) { return launch_gram_keys(k_ngram_keys<true>, k_ngram_keys<false>, kNgBlock, P, st); }

}  // namespace latok
