// block_ops.h -- what the threads of one workgroup do together, and the per-thread searches they share: the bisections of a row-start
// array, the rows that touch a workgroup's tokens, the checked load of a token's span record, the three composed into a lane's token, the
// workgroup prefix sum.  Device code
// only; beside wave_ops.h (what one wavefront does), for the same reason: a kernel calls these instead of carrying a copy.
#ifndef LATOK_BLOCK_OPS_H
#define LATOK_BLOCK_OPS_H
#include "kernels.h"
#include "wave_ops.h"

namespace latok {

// first i in [lo, hi) with v[i] >= x (hi if none) / with v[i] > x
__device__ __forceinline__ int64_t lower_bound_i64(const int64_t* __restrict__ v, int64_t lo, int64_t hi, int64_t x) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (v[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ int64_t upper_bound_i64(const int64_t* __restrict__ v, int64_t lo, int64_t hi, int64_t x) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (v[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the rows that touch the workgroup's tokens [t0, t0 + SPAN): [*lo, *end) holds the row of every one of them.  row_start = the row
// starts in token space, n_str + 1 entries.  Every thread of the workgroup calls it (a barrier inside) and gets both values.
template <int SPAN>
__device__ __forceinline__ void block_rows(const int64_t* __restrict__ row_start, int64_t n_str, int64_t t0, int64_t* lo, int64_t* end) {
    __shared__ int64_t s_lo, s_end;
    if (threadIdx.x == 0) {
        const int64_t first = lower_bound_i64(row_start, 0, n_str, t0);
        s_end = lower_bound_i64(row_start, first, n_str, t0 + SPAN);   // (rows that start on the far edge, empty ones included, are the next workgroup's)
        s_lo = first > 0 ? first - 1 : 0;                              // the row that was open when the block began
    }
    __syncthreads();
    *lo = s_lo;
    *end = s_end;
}
// the row of token t among the rows [lo, end) of block_rows: the last one that starts at or before t, whatever the number of empty
// rows at one offset (>= lo where row_start[lo] <= t, which block_rows gives with row starts from the scan)
__device__ __forceinline__ int64_t row_of_token(const int64_t* __restrict__ row_start, int64_t lo, int64_t end, int64_t t) {
    return upper_bound_i64(row_start, lo, end, t) - 1;
}

// the absolute byte range of token t, whose string begins at byte `base` of a text of `total` bytes, from its int64 span record (two
// string-relative offsets, one 16-byte load).  ok = the range lies inside the text and is not empty: with records from the scatter
// always; a caller that reads nothing of a token that is not ok leaves the text with no load, whatever the workspace holds.
struct TokenBytes {
    int64_t a, e;
    bool ok;
};
__device__ __forceinline__ TokenBytes token_bytes(const int64_t* __restrict__ tok_spans, int64_t t, int64_t base, int64_t total) {
    typedef long long ll2 __attribute__((ext_vector_type(2)));
    const ll2 rec = *reinterpret_cast<const ll2*>(tok_spans + 2 * t);
    const int64_t a = base + rec.x, e = base + rec.y;
    return TokenBytes{a, e, base >= 0 && rec.x >= 0 && a < e && e <= total};
}

// The token of this lane in a kernel that takes one token per lane, BLOCK per workgroup, of a text in token space (TokenText of
// kernels.h): t = the token, row = its string, held inside [0, n_str) whatever row_start holds, base = the string's first byte, b = the
// token's checked byte range.  b.ok is false for a lane behind the last token (nothing of it is loaded) and for a record that does not
// lie inside the text (cannot happen with records from the scatter): a caller that reads the text only where b.ok -- or where a
// token_bytes of its own says so -- leaves the buffer with no load, whatever the workspace holds; a record is read only inside
// [0, n_tok).  Every thread of the workgroup calls it before any early return: block_rows contains a barrier.
struct LaneToken {
    int64_t t, row, base;
    TokenBytes b;
};
template <int BLOCK>
__device__ __forceinline__ LaneToken lane_token(const TokenText& T) {
    const int64_t t0 = (int64_t)blockIdx.x * BLOCK, t = t0 + threadIdx.x;
    int64_t lo, end;
    block_rows<BLOCK>(T.row_start, T.n_str, t0, &lo, &end);
    LaneToken k{t, 0, 0, TokenBytes{0, 0, false}};
    if (t >= T.n_tok) return k;
    const int64_t r = row_of_token(T.row_start, lo, end, t);
    k.row = r < 0 ? 0 : (r >= T.n_str ? T.n_str - 1 : r);
    k.base = T.row_off[k.row];
    k.b = token_bytes(T.tok_spans, t, k.base, T.total);
    return k;
}

// inclusive prefix sum of one value per thread over a workgroup of WAVES wavefronts; *total = the workgroup's sum (the exclusive
// prefix is the result minus v).  lds = T[WAVES] of the caller.  The leading barrier makes a second use of the same words safe.
template <typename T, int WAVES>
__device__ __forceinline__ T block_scan_add(T v, T* lds, T* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    v = shfl_scan_add(v, lane);
    __syncthreads();   // (lds may still be read from the use before)
    if (lane == 63) lds[wave] = v;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < WAVES; ++k) {
        const T x = lds[k];
        if (k < wave) before += x;
        all += x;
    }
    *total = all;
    return v + before;
}

}  // namespace latok
#endif
