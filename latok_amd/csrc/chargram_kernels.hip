// chargram_kernels.hip -- character n-grams inside tokens (scikit-learn's analyzer="char_wb") of a UTF-8 batch in byte space: one term
// key (term_key.h) per gram, the kernels behind latok_chargram_counts_utf8_bytes_batch and latok_hashed_chargram_counts_utf8_bytes_batch.
// They work in TOKEN space, one lane per token, as the WordPiece and word n-gram kernels do: SpanRecords of scatter_block
// (compact_kernels.hip) has left the int64 span record of every token at its rank in the workspace, the chained scan the row starts in
// token space (row_start[n_str + 1]).  The rules of a token's grams are chargram_text.h.
//
//   k_cgram_count  one lane per token t, plus the entry behind the last token (0).  The lane finds its string (block_rows,
//                  row_of_token, token_bytes of block_ops.h), counts the token's character starts over its checked byte range as
//                  aligned dwords (cg_count_chars: a mask of the non-continuation bytes per dword and a popcount) and stores G(W) as
//                  int64.  The chained scan of the n_tok + 1 entries gives each token's key rank and the key total K.
//   row starts     key_start[s] = rank[row_start[s]]: k_wp_rows of wordpiece_kernels.hip, in int64.
//   k_cgram_keys   one lane per token.  cg_walk goes over the padded word's start positions i = 0 .. W - 1 and feeds at most max_n
//                  characters from each through the streaming hash; the key of gram (n, i) -- tk_hashed_key of the hash, or
//                  tk_vocab_probe with cg_equal over the gram's bytes -- goes to rank[t] + (sum over m in [min_n, n) of g(m, W)) + i:
//                  order by order, a bijection onto the token's range of keys; the reduce sorts inside the row, so the order inside it
//                  is free.  The short word's one gram goes to the one slot its order has.
// A lane whose token is long keeps its wave busy while the others idle -- one lane walks a long token alone: accepted in this version,
// as in WordPiece; there is no whole-wave form for long tokens.  Every loop runs by its own counter: a token's dwords, a character's
// bytes up to the token's end, the positions, at most max_n <= kNgMax orders, a probe at most n_slots steps.  A key is stored only
// inside the token's own slots and inside [0, n_keys), a record read only inside [0, n_tok), a rank only inside [0, n_tok], the text
// only where a checked record says -- whatever the workspace holds.  Table and blob are read with ordinary cached loads, the text as
// aligned dwords up to the one that holds a token's last byte.  No kernel here waits for another workgroup; all stores are vector
// stores from plain C++.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_ops.h"
#include "chargram_text.h"
#include "kernels.h"
#include "term_key.h"

namespace latok {

// the checked byte range of token t (one lane of a workgroup whose rows are [lo, end)); false: no gram
__device__ __forceinline__ bool cg_token(const int64_t* __restrict__ row_off, int64_t n_str, int64_t total, const int64_t* __restrict__ row_start,
                                         const int64_t* __restrict__ tok_spans, int64_t lo, int64_t end, int64_t t, TokenBytes* out) {
    int64_t r = row_of_token(row_start, lo, end, t);
    r = r < 0 ? 0 : (r >= n_str ? n_str - 1 : r);
    *out = token_bytes(tok_spans, t, row_off[r], total);
    return out->ok;
}

__global__ __launch_bounds__(kCgBlock) void k_cgram_count(const uint32_t* __restrict__ text, int64_t total, const int64_t* __restrict__ row_off,
                                                          int64_t n_str, const int64_t* __restrict__ row_start,
                                                          const int64_t* __restrict__ tok_spans, int64_t n_tok, int min_n, int max_n,
                                                          int64_t* __restrict__ cnt) {
    const int64_t t0 = (int64_t)blockIdx.x * kCgBlock, t = t0 + threadIdx.x;
    int64_t lo, end;
    block_rows<kCgBlock>(row_start, n_str, t0, &lo, &end);
    if (t > n_tok) return;
    int64_t g = 0;
    TokenBytes b;
    if (t < n_tok && cg_token(row_off, n_str, total, row_start, tok_spans, lo, end, t, &b))
        g = cg_gram_count(cg_count_chars([text](int64_t i) { return text[i]; }, b.a, b.e) + 2, min_n, max_n);
    cnt[t] = g;   // (t == n_tok: the entry behind the last token)
}

struct ChargramParams {
    const uint32_t* text;
    int64_t total;
    const int64_t* row_off;
    int64_t n_str;
    const int64_t* row_start;   // token space
    const int64_t* rank;        // key space, n_tok + 1 entries
    const int64_t* tok_spans;
    int64_t n_tok, n_keys;
    int min_n, max_n;
    uint32_t pad;
    VocabTable vt;              // VOCAB
    uint32_t seed, n_features;  // hashed form
    bool alternate_sign;
    uint64_t* keys;
};

template <bool VOCAB>
__global__ __launch_bounds__(kCgBlock) void k_cgram_keys(ChargramParams P) {
    const int64_t t0 = (int64_t)blockIdx.x * kCgBlock, t = t0 + threadIdx.x;
    int64_t lo, end;
    block_rows<kCgBlock>(P.row_start, P.n_str, t0, &lo, &end);
    if (t >= P.n_tok) return;
    TokenBytes b;
    if (!cg_token(P.row_off, P.n_str, P.total, P.row_start, P.tok_spans, lo, end, t, &b)) return;
    const int64_t at = P.rank[t], mine = P.rank[t + 1] - at;   // (rank has n_tok + 1 entries)
    if (mine < 1 || at < 0 || at + mine > P.n_keys) return;
    const uint32_t* const text = P.text;
    auto ld = [text](int64_t i) { return text[i]; };
    const int64_t W = cg_count_chars(ld, b.a, b.e) + 2;
    const VtSlot* const slots = reinterpret_cast<const VtSlot*>(P.vt.slots);
    const uint32_t* const blob = P.vt.blob;
    const uint32_t pad = P.pad;
    uint64_t* const keys = P.keys;
    cg_walk(ld, b.a, b.e, W, P.min_n, P.max_n, pad, VOCAB ? P.vt.seed : P.seed, [&](const CgGram& g) {
        uint64_t key;
        if (VOCAB) {
            key = tk_vocab_probe([slots](uint64_t i) { return slots[i]; }, P.vt.n_slots, g.hash, g.len, [&](uint32_t off) {
                return cg_equal(ld, g.gs, g.ge, g.front, g.back, pad, [blob](uint64_t i) { return blob[i]; }, off, g.len);
            });
        } else {
            key = tk_hashed_key(g.hash, P.n_features, P.alternate_sign);
        }
        if (g.slot >= 0 && g.slot < mine) keys[at + g.slot] = key;
    });
}

// ---- launchers -----------------------------------------------------------------------------------------------------
hipError_t launch_cgram_count(const uint8_t* u8, int64_t total, const int64_t* row_off, int64_t n_str, const int64_t* row_start,
                              const int64_t* tok_spans, int64_t n_tok, int min_n, int max_n, int64_t* cnt, hipStream_t st) {
    if (n_str <= 0 || n_tok <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)((n_tok + 1 + kCgBlock - 1) / kCgBlock);   // (+ 1: the entry behind the last token)
    hipLaunchKernelGGL(k_cgram_count, dim3(blocks), dim3(kCgBlock), 0, st, reinterpret_cast<const uint32_t*>(u8), total, row_off, n_str, row_start,
                       tok_spans, n_tok, min_n, max_n < kNgMax ? max_n : kNgMax, cnt);
    return hipGetLastError();
}

hipError_t launch_cgram_keys(const uint8_t* u8, int64_t total, const int64_t* row_off, int64_t n_str, const int64_t* row_start,
                             const int64_t* rank, const int64_t* tok_spans, int64_t n_tok, int64_t n_keys, int min_n, int max_n, int pad,
                             const VocabTable* vt, uint32_t seed, uint32_t n_features, bool alternate_sign, uint64_t* keys, hipStream_t st) {
    if (n_str <= 0 || n_tok <= 0 || n_keys <= 0) return hipSuccess;
    ChargramParams P;
    P.text = reinterpret_cast<const uint32_t*>(u8);
    P.total = total;
    P.row_off = row_off;
    P.n_str = n_str;
    P.row_start = row_start;
    P.rank = rank;
    P.tok_spans = tok_spans;
    P.n_tok = n_tok;
    P.n_keys = n_keys;
    P.min_n = min_n;
    P.max_n = max_n < kNgMax ? max_n : kNgMax;
    P.pad = (uint32_t)pad & 0xFFu;
    P.vt = vt ? *vt : VocabTable{};
    P.seed = seed;
    P.n_features = n_features;
    P.alternate_sign = alternate_sign;
    P.keys = keys;
    const dim3 grid((unsigned)((n_tok + kCgBlock - 1) / kCgBlock)), block(kCgBlock);
    if (vt) hipLaunchKernelGGL((k_cgram_keys<true>), grid, block, 0, st, P);
    else hipLaunchKernelGGL((k_cgram_keys<false>), grid, block, 0, st, P);
    return hipGetLastError();
}

}  // namespace latok
