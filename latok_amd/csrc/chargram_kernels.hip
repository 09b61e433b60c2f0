// chargram_kernels.hip -- character n-grams inside tokens (scikit-learn's analyzer="char_wb") of a UTF-8 batch in byte space: one term
// key (term_key.h) per gram, the kernels behind latok_chargram_counts_utf8_bytes_batch and latok_hashed_chargram_counts_utf8_bytes_batch.
// They work in TOKEN space, one lane per token, as the WordPiece and word n-gram kernels do: SpanRecords of scatter_block
// (compact_kernels.hip) has left the int64 span record of every token at its rank in the workspace, the chained scan the row starts in
// token space (row_start[n_str + 1]).  The rules of a token's grams are chargram_text.h.
//
//   k_cgram_count  one lane per token t, plus the entry behind the last token (0).  The lane takes its token's checked byte range
//                  (lane_token of block_ops.h), counts the token's character starts over it as
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
// inside the token's own slots and inside [0, n_keys), a rank read only inside [0, n_tok]; records and text are read as lane_token of
// block_ops.h says, where that part of the argument stands -- whatever the workspace holds.  Table and blob are read with ordinary
// cached loads, the text as aligned dwords up to the one that holds a token's last byte.  No kernel here waits for another workgroup;
// all stores are vector stores from plain C++.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_ops.h"
#include "chargram_text.h"
#include "kernels.h"
#include "term_key.h"

namespace latok {

__global__ __launch_bounds__(kCgBlock) void k_cgram_count(TokenText T, int min_n, int max_n, int64_t* __restrict__ cnt) {
    const LaneToken k = lane_token<kCgBlock>(T);
    if (k.t > T.n_tok) return;
    const uint32_t* const text = T.text;
    cnt[k.t] = k.b.ok ? cg_gram_count(cg_count_chars([text](int64_t i) { return text[i]; }, k.b.a, k.b.e) + 2, min_n, max_n) : 0;
    // (t == n_tok: the entry behind the last token)
}

template <bool VOCAB>
__global__ __launch_bounds__(kCgBlock) void k_cgram_keys(GramKeys P) {
    const LaneToken k = lane_token<kCgBlock>(P.t);
    if (!k.b.ok) return;
    const TokenBytes b = k.b;
    const int64_t at = P.rank[k.t], mine = P.rank[k.t + 1] - at;   // (rank has n_tok + 1 entries)
    if (mine < 1 || at < 0 || at + mine > P.n_keys) return;
    const uint32_t* const text = P.t.text;
    auto ld = [text](int64_t i) { return text[i]; };
    const int64_t W = cg_count_chars(ld, b.a, b.e) + 2;
    const VtSlot* const slots = reinterpret_cast<const VtSlot*>(P.form.vt.slots);
    const uint32_t* const blob = P.form.vt.blob;
    const uint32_t pad = P.joiner;
    uint64_t* const keys = P.keys;
    cg_walk(ld, b.a, b.e, W, P.min_n, P.max_n, pad, P.form.seed, [&](const CgGram& g) {
        uint64_t key;
        if (VOCAB) {
            key = tk_vocab_probe([slots](uint64_t i) { return slots[i]; }, P.form.vt.n_slots, g.hash, g.len, [&](uint32_t off) {
                return cg_equal(ld, g.gs, g.ge, g.front, g.back, pad, [blob](uint64_t i) { return blob[i]; }, off, g.len);
            });
        } else {
            key = tk_hashed_key(g.hash, P.form.n_features, P.form.alternate_sign);
        }
        if (g.slot >= 0 && g.slot < mine) keys[at + g.slot] = key;
    });
}

// ---- launchers -----------------------------------------------------------------------------------------------------
hipError_t launch_cgram_count(const TokenText& t, int min_n, int max_n, int64_t* cnt, hipStream_t st) {
    if (t.n_str <= 0 || t.n_tok <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)((t.n_tok + 1 + kCgBlock - 1) / kCgBlock);   // (+ 1: the entry behind the last token)
    hipLaunchKernelGGL(k_cgram_count, dim3(blocks), dim3(kCgBlock), 0, st, t, min_n, max_n, cnt);
    return hipGetLastError();
}

hipError_t launch_cgram_keys(const GramKeys& P, hipStream_t st) { return launch_gram_keys(k_cgram_keys<true>, k_cgram_keys<false>, kCgBlock, P, st); }

}  // namespace latok
