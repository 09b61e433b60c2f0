// wordpiece_kernels.hip -- WordPiece ids of a UTF-8 batch in byte space: the kernels behind latok_wordpiece_ids_utf8_bytes_batch and
// latok_wordpiece_padded_utf8_bytes_batch.  They work in TOKEN space, one lane per token.  SpanRecords of scatter_block
// (compact_kernels.hip) has left the int64 span record of every token at its rank in the workspace and the token count of every
// string; the chained scan the row starts in token space (row_start[n_str + 1], row_start[n_str] = the token total).
//
//   k_wp_count   pieces of token t = wp_walk (wordpiece.h) without stores -> cnt[t]; cnt[n_tok] = 0, so that the scan of the
//                n_tok + 1 entries leaves the piece total behind the last token's rank
//   k_wp_emit    behind the scan: the same walk of the same token, by the same function, with stores: ids[rank[t] + k], and the
//                piece's string-relative byte range if asked for, only if the piece total fits the capacity.  Piece 0 is kept in
//                registers until the walk returns (a miss after hits withdraws what was found), a piece k >= 1 is stored only below
//                the count the first pass found: nothing is ever written outside the token's own range of ranks
//   k_wp_rows    indptr[s] = rank[row_start[s]], in the caller's width
//   k_wp_pad     one thread per cell (s, j) of the [n_str, max_length] block of the padded form
// A lane's token, its string and its checked byte range are lane_token of block_ops.h, where the bounds argument of that part stands:
// a token that is not ok is skipped, so no load leaves the buffer whatever the workspace holds.  Table and blob are read with
// ordinary cached loads (they are what is worth keeping in L2), the text as aligned dwords up to the one that holds the token's
// last byte.  A lane with a long or unknown token keeps its wave busy while the others idle:
// accepted in this version.  No kernel here waits for another workgroup; all stores are vector stores from plain C++.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_ops.h"
#include "kernels.h"
#include "wordpiece.h"

namespace latok {

#define LATOK_WP_VIEWS(wt)                                                                                                          \
    const VtSlot* const slots0 = reinterpret_cast<const VtSlot*>((wt).initial.slots);                                               \
    const VtSlot* const slots1 = reinterpret_cast<const VtSlot*>((wt).cont.slots);                                                  \
    const uint32_t* const blob0 = (wt).initial.blob;                                                                                \
    const uint32_t* const blob1 = (wt).cont.blob;                                                                                   \
    const auto tab0 = wp_table_view([slots0](uint64_t i) { return slots0[i]; }, [blob0](uint64_t i) { return blob0[i]; },          \
                                    (wt).initial.n_slots, (wt).max_len0);                                                           \
    const auto tab1 = wp_table_view([slots1](uint64_t i) { return slots1[i]; }, [blob1](uint64_t i) { return blob1[i]; },          \
                                    (wt).cont.n_slots, (wt).max_len1)

__global__ __launch_bounds__(kWpBlock) void k_wp_count(TokenText T, WordPieceTables wt, int64_t* __restrict__ cnt) {
    const LaneToken k = lane_token<kWpBlock>(T);
    if (k.t > T.n_tok) return;
    int64_t n = 0;
    if (k.b.ok) {
        const uint32_t* const text = T.text;
        LATOK_WP_VIEWS(wt);
        n = wp_walk([text](int64_t i) { return text[i]; }, k.b.a, k.b.e, tab0, tab1, wt.initial.seed, wt.max_chars, 0,
                    [](int, int32_t, int64_t, int64_t) {});
    }
    cnt[k.t] = n;   // (t == n_tok: the entry behind the last token)
}

template <typename OUT>
__global__ __launch_bounds__(kWpBlock) void k_wp_emit(TokenText T, WordPieceTables wt, int32_t unk, const int64_t* __restrict__ rank,
                                                      const int64_t* __restrict__ n_pieces_dev, int64_t cap, int32_t* __restrict__ ids,
                                                      OUT* __restrict__ spans) {
    if (*n_pieces_dev > cap) return;   // the caller's buffers hold `cap` pieces: nothing is written when the batch has more
    const LaneToken k = lane_token<kWpBlock>(T);
    if (!k.b.ok) return;
    const int64_t at = rank[k.t];
    const int n_mine = (int)(rank[k.t + 1] - at);   // (rank has n_tok + 1 entries)
    if (n_mine < 1 || at < 0 || at + n_mine > cap) return;
    typedef OUT out2 __attribute__((ext_vector_type(2)));
    const int64_t base = k.base;
    int32_t id0 = unk;
    int64_t a0 = k.b.a, e0 = k.b.e;
    const uint32_t* const text = T.text;
    LATOK_WP_VIEWS(wt);
    wp_walk([text](int64_t i) { return text[i]; }, k.b.a, k.b.e, tab0, tab1, wt.initial.seed, wt.max_chars, unk,
            [&id0, &a0, &e0, ids, spans, at, n_mine, base](int j, int32_t id, int64_t a, int64_t e) {
                if (j == 0) {   // kept back: a later piece 0 replaces it
                    id0 = id;
                    a0 = a;
                    e0 = e;
                } else if (j < n_mine) {
                    __builtin_nontemporal_store(id, ids + at + j);
                    if (spans) {
                        out2 v;
                        v.x = (OUT)(a - base);
                        v.y = (OUT)(e - base);
                        __builtin_nontemporal_store(v, reinterpret_cast<out2*>(spans) + at + j);
                    }
                }
            });
    __builtin_nontemporal_store(id0, ids + at);
    if (spans) {
        out2 v;
        v.x = (OUT)(a0 - base);
        v.y = (OUT)(e0 - base);
        __builtin_nontemporal_store(v, reinterpret_cast<out2*>(spans) + at);
    }
}

// the piece rank of the first token of row s (rank has n_tok + 1 entries; the index is held inside them whatever row_start holds)
__device__ __forceinline__ int64_t wp_row_rank(const int64_t* __restrict__ row_start, const int64_t* __restrict__ rank, int64_t n_tok, int64_t s) {
    const int64_t t = row_start[s];
    return rank[t < 0 ? 0 : (t > n_tok ? n_tok : t)];
}

template <typename OUT>
__global__ __launch_bounds__(256) void k_wp_rows(const int64_t* __restrict__ row_start, const int64_t* __restrict__ rank, int64_t n_str,
                                                 int64_t n_tok, OUT* __restrict__ indptr_out) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s <= n_str) indptr_out[s] = (OUT)wp_row_rank(row_start, rank, n_tok, s);
}

__global__ __launch_bounds__(256) void k_wp_pad(const int32_t* __restrict__ ids, const int64_t* __restrict__ row_start,
                                                const int64_t* __restrict__ rank, int64_t n_str, int64_t n_tok, int64_t max_length, int sp, int32_t cls_id,
                                                int32_t sep_id, int32_t pad_id, int32_t* __restrict__ input_ids, int32_t* __restrict__ lengths) {
    const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (cell >= n_str * max_length) return;
    const int64_t s = cell / max_length, j = cell - s * max_length;
    const int64_t p0 = rank ? wp_row_rank(row_start, rank, n_tok, s) : 0, p1 = rank ? wp_row_rank(row_start, rank, n_tok, s + 1) : 0;
    const int64_t body = max_length - 2 * sp;
    const int64_t used = max((int64_t)0, min(p1 - p0, body));
    int32_t v = pad_id;
    if (j < sp) v = cls_id;
    else if (j < sp + used) v = ids[p0 + j - sp];
    else if (j == sp + used && sp) v = sep_id;
    input_ids[cell] = v;
    if (j == 0) lengths[s] = (int32_t)(used + 2 * sp);
}

// ---- launchers -----------------------------------------------------------------------------------------------------
hipError_t launch_wp_count(const TokenText& t, const WordPieceTables& wt, int64_t* cnt, hipStream_t st) {
    if (t.n_str <= 0 || t.n_tok <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)((t.n_tok + 1 + kWpBlock - 1) / kWpBlock);   // (+ 1: the entry behind the last token)
    hipLaunchKernelGGL(k_wp_count, dim3(blocks), dim3(kWpBlock), 0, st, t, wt, cnt);
    return hipGetLastError();
}

hipError_t launch_wp_emit(bool out32, const TokenText& t, const WordPieceTables& wt, int32_t unk_id, const int64_t* rank,
                          const int64_t* n_pieces_dev, int64_t cap, int32_t* ids, void* spans, hipStream_t st) {
    if (t.n_str <= 0 || t.n_tok <= 0 || !ids) return hipSuccess;
    const dim3 grid((unsigned)((t.n_tok + kWpBlock - 1) / kWpBlock)), block(kWpBlock);
    if (out32) hipLaunchKernelGGL((k_wp_emit<int32_t>), grid, block, 0, st, t, wt, unk_id, rank, n_pieces_dev, cap, ids, (int32_t*)spans);
    else hipLaunchKernelGGL((k_wp_emit<int64_t>), grid, block, 0, st, t, wt, unk_id, rank, n_pieces_dev, cap, ids, (int64_t*)spans);
    return hipGetLastError();
}

hipError_t launch_wp_rows(bool out32, const int64_t* row_start, const int64_t* rank, int64_t n_str, int64_t n_tok, void* indptr_out, hipStream_t st) {
    const dim3 grid((unsigned)((n_str + 256) / 256)), block(256);
    if (out32) hipLaunchKernelGGL((k_wp_rows<int32_t>), grid, block, 0, st, row_start, rank, n_str, n_tok, (int32_t*)indptr_out);
    else hipLaunchKernelGGL((k_wp_rows<int64_t>), grid, block, 0, st, row_start, rank, n_str, n_tok, (int64_t*)indptr_out);
    return hipGetLastError();
}

hipError_t launch_wp_pad(const int32_t* ids, const int64_t* row_start, const int64_t* rank, int64_t n_str, int64_t n_tok, int64_t max_length, int add_special,
                         int32_t cls_id, int32_t sep_id, int32_t pad_id, int32_t* input_ids, int32_t* lengths, hipStream_t st) {
    if (n_str <= 0) return hipSuccess;
    const int64_t cells = n_str * max_length;
    hipLaunchKernelGGL(k_wp_pad, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, ids, row_start, rank, n_str, n_tok, max_length,
                       add_special ? 1 : 0, cls_id, sep_id, pad_id, input_ids, lengths);
    return hipGetLastError();
}

}  // namespace latok
