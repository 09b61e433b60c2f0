// terms_kernels.hip -- per-string term counts: the segmented sort-and-reduce behind latok_term_counts_utf8_bytes_batch and
// latok_hashed_term_counts_utf8_bytes_batch.  k_term_scatter (compact_kernels.hip, TermTokens) has left one term key (term_key.h) per
// token at its rank and the chained scan the row starts in token space (row_start[n_str + 1], row_start[n_str] = the token total).
//
//   ownership    token space is cut into tiles of kTermsTile tokens; a workgroup owns the rows that START in its tile -- found by
//                two bisections of row_start, whatever the number of empty rows at one offset.  A row of more than kTermsRowMax
//                (= kTermsTile) tokens is long: it reaches beyond its tile, so at most one starts in a tile and it is the last
//                row that does.  Without it a workgroup's tokens are one contiguous range of fewer than 2 * kTermsTile keys.
//   k_terms_tile the short rows: the range goes into LDS as (row start inside the range) << 34 | key, one bitonic sort of the
//                composites is the segmented sort (the row is the high part; out-of-vocabulary keys carry bit 33 and end up behind
//                the found keys of their row).  One block scan of packed {entry heads, found tokens, values} then gives every row
//                its distinct count and OOV count and every run of one column its sum and its rank inside the row.
//   k_terms_long the long row of a tile, one workgroup: an LSD radix sort of the row's keys, 5 bits a pass over the 34 key bits,
//                ping-pong between the key buffer and a second one -- every thread counts and scatters a contiguous share of the
//                row, so the sort is stable with LDS counters alone: O(L) a pass, seven passes, any length.  The reduce then
//                streams the sorted row 256 keys a step with carried totals.  A tile in which no row starts does nothing.
//   both write   distinct[row], oov[row] and the row's entries (column << 32 | sum) over the FIRST distinct[row] keys of the row in
//                the key buffer.  The rows' token ranges are disjoint, so no workgroup waits for or writes into another's.
//   k_terms_emit behind the scan of distinct[] (= indptr, nnz): entry j of row r from keys[row_start[r] + j] to indptr[r] + j, one
//                thread per token slot, only if nnz fits the capacity.
// No kernel here waits for another workgroup; all stores are vector stores from plain C++.  From block_ops.h: the bisections
// (lower_bound_i64, row_of_token), block_rows (k_terms_emit), block_scan_add (k_terms_tile, k_terms_long).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_ops.h"
#include "kernels.h"
#include "term_key.h"

namespace latok {

constexpr int kTermsBlock = 256;
constexpr int kTermsRange = 2 * kTermsTile;               // keys a workgroup sorts at most (the range is shorter by one at least)
constexpr int kTermsPer = kTermsRange / kTermsBlock;      // sorted positions per thread in the scan
constexpr int kTermsRowShift = kTkKeyBits;                // the row start sits above the key in a composite
static_assert(kTermsRowMax <= kTermsTile && (kTermsTile & (kTermsTile - 1)) == 0, "a short row fits a tile; tiles are a power of two");
static_assert(kTermsRowMax == kTermsTile, "at most one long row starts in a tile: the ownership below relies on it");
constexpr int kRadixBits = 5, kRadixBins = 1 << kRadixBits, kRadixPasses = 7;
static_assert(kRadixPasses * kRadixBits >= kTkKeyBits && (kRadixPasses & 1), "the passes cover the key and end in the second buffer");

// What the workgroup of tile `tile` owns: rows [first, end) start in it; their short tokens are [a, b); long_row = the long row
// that starts in it, or -1.
struct TermsOwn {
    int64_t first, end, a, b, long_row;
};
__device__ __forceinline__ TermsOwn terms_own(const int64_t* __restrict__ row_start, int64_t n_str, int64_t tile) {
    TermsOwn o;
    const int64_t t0 = tile * kTermsTile;
    o.first = lower_bound_i64(row_start, 0, n_str, t0);
    o.end = lower_bound_i64(row_start, o.first, n_str, t0 + kTermsTile);
    o.a = row_start[o.first];   // (row_start has n_str + 1 entries)
    o.b = row_start[o.end];
    o.long_row = -1;
    if (o.end > o.first) {
        const int64_t s_last = row_start[o.end - 1];
        if (o.b - s_last > kTermsRowMax) {
            o.long_row = o.end - 1;
            o.b = s_last;
        }
    }
    return o;
}

// packed scan word of a sorted position: entry heads << 48 | found tokens << 32, plus the (signed) value
__device__ __forceinline__ long long terms_pack(bool head, bool found, int v) { return ((long long)head << 48) + ((long long)found << 32) + (long long)v; }
__device__ __forceinline__ int terms_sum(long long p) { return (int)(unsigned)p; }
__device__ __forceinline__ int terms_found(long long p) { return (int)(((p - (long long)terms_sum(p)) >> 32) & 0xFFFF); }
__device__ __forceinline__ int terms_heads(long long p) { return (int)((p - (long long)terms_sum(p)) >> 48); }

__global__ __launch_bounds__(kTermsBlock) void k_terms_tile(uint64_t* __restrict__ keys, const int64_t* __restrict__ row_start, int64_t n_str,
                                                            uint32_t flip, int64_t* __restrict__ distinct, int64_t* __restrict__ oov) {
    __shared__ uint64_t comp[kTermsRange];
    __shared__ long long scan_s[kTermsRange];
    __shared__ int run0[kTermsRange];
    __shared__ long long s_wave[kTermsBlock / 64];
    __shared__ TermsOwn s_own;
    const int tid = threadIdx.x;
    if (tid == 0) s_own = terms_own(row_start, n_str, blockIdx.x);
    __syncthreads();
    const TermsOwn o = s_own;
    const int n = (int)(o.b - o.a);          // < kTermsRange: every row of the range is short and starts inside the tile
    if (n <= 0 || n >= kTermsRange) return;   // (uniform; the second half cannot happen with row starts from the scan)
    int N = 2;
    while (N < n) N <<= 1;
    for (int i = tid; i < N; i += kTermsBlock) {
        uint64_t c = ~0ull;   // padding sorts behind every key
        if (i < n) {
            const int64_t r = row_of_token(row_start, o.first, o.end, o.a + i);   // the row that holds token a + i
            c = ((uint64_t)(row_start[r] - o.a) << kTermsRowShift) | keys[o.a + i];
        }
        comp[i] = c;
    }
    __syncthreads();
    for (int k = 2; k <= N; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < (N >> 1); i += kTermsBlock) {
                const int l = 2 * i - (i & (j - 1)), r = l + j;
                const uint64_t x = comp[l], y = comp[r];
                if ((x > y) == ((l & k) == 0)) {
                    comp[l] = y;
                    comp[r] = x;
                }
            }
            __syncthreads();
        }
    }
    // the packed scan over the sorted positions, kTermsPer consecutive ones per thread
    long long mine[kTermsPer], run = 0;
#pragma unroll
    for (int e = 0; e < kTermsPer; ++e) {
        const int i = tid * kTermsPer + e;
        long long p = 0;
        if (i < n) {
            const uint64_t c = comp[i];
            const bool found = !tk_is_oov(c);
            const bool head = found && (i == 0 || (c >> 1) != (comp[i - 1] >> 1));
            p = terms_pack(head, found, found ? tk_value(c) : 0);
        }
        run += p;
        mine[e] = run;
    }
    long long total;
    const long long before = block_scan_add<long long, kTermsBlock / 64>(run, s_wave, &total) - run;
#pragma unroll
    for (int e = 0; e < kTermsPer; ++e) {
        const int i = tid * kTermsPer + e;
        if (i < n) scan_s[i] = mine[e] + before;
    }
    __syncthreads();
    // every run of one column: its head leaves the sum in front of it at the run's entry rank ...
    for (int i = tid; i < n; i += kTermsBlock) {
        const uint64_t c = comp[i];
        if (!tk_is_oov(c) && (i == 0 || (c >> 1) != (comp[i - 1] >> 1))) {
            const long long p = scan_s[i];
            run0[terms_heads(p) - 1] = terms_sum(p) - tk_value(c);
        }
    }
    __syncthreads();
    // ... its last token stores the entry; the last token of a row stores the row's two counts
    for (int i = tid; i < n; i += kTermsBlock) {
        const uint64_t c = comp[i];
        const uint64_t next = i + 1 < n ? comp[i + 1] : ~0ull;
        const int rs = (int)(c >> kTermsRowShift);
        const long long p = scan_s[i], p0 = rs > 0 ? scan_s[rs - 1] : 0ll;
        if (!tk_is_oov(c) && (c >> 1) != (next >> 1)) {
            const int rank = terms_heads(p) - 1 - terms_heads(p0);
            const int sum = terms_sum(p) - run0[terms_heads(p) - 1];
            keys[o.a + rs + rank] = ((uint64_t)((uint32_t)(c >> kTkColumnShift) ^ flip) << 32) | (uint64_t)(uint32_t)sum;
        }
        if ((next >> kTermsRowShift) != (c >> kTermsRowShift)) {
            const int64_t row = row_of_token(row_start, o.first, o.end, o.a + rs);
            distinct[row] = terms_heads(p) - terms_heads(p0);
            oov[row] = (i + 1 - rs) - (terms_found(p) - terms_found(p0));
        }
    }
}

__global__ __launch_bounds__(kTermsBlock) void k_terms_long(uint64_t* __restrict__ keys, uint64_t* __restrict__ alt, const int64_t* __restrict__ row_start,
                                                            int64_t n_str, uint32_t flip, int64_t* __restrict__ distinct, int64_t* __restrict__ oov) {
    __shared__ unsigned cnt[kRadixBins * kTermsBlock];   // counter of (digit d, thread t) at d * kTermsBlock + t: the scan order
    __shared__ long long s_wave[kTermsBlock / 64];
    __shared__ TermsOwn s_own;
    __shared__ long long s_found;
    const int tid = threadIdx.x;
    if (tid == 0) s_own = terms_own(row_start, n_str, blockIdx.x);
    __syncthreads();
    const int64_t row = s_own.long_row;
    if (row < 0) return;   // (uniform) no long row starts in this tile
    const int64_t s = row_start[row], L = row_start[row + 1] - s;
    const int64_t share = (L + kTermsBlock - 1) / kTermsBlock;
    const int64_t i0 = min(L, tid * share), i1 = min(L, i0 + share);   // my contiguous share of the row
    uint64_t* src = keys + s;
    uint64_t* dst = alt + s;
    for (int pass = 0; pass < kRadixPasses; ++pass) {
        const int shift = pass * kRadixBits;
#pragma unroll
        for (int d = 0; d < kRadixBins; ++d) cnt[d * kTermsBlock + tid] = 0u;
        for (int64_t i = i0; i < i1; ++i) ++cnt[(int)((src[i] >> shift) & (kRadixBins - 1)) * kTermsBlock + tid];
        __syncthreads();
        // exclusive scan of the counters in (digit, thread) order: kRadixBins consecutive ones per thread
        unsigned sum = 0;
        for (int e = 0; e < kRadixBins; ++e) sum += cnt[tid * kRadixBins + e];
        long long total;
        unsigned at = (unsigned)(block_scan_add<long long, kTermsBlock / 64>((long long)sum, s_wave, &total) - (long long)sum);
        for (int e = 0; e < kRadixBins; ++e) {
            const unsigned c = cnt[tid * kRadixBins + e];
            cnt[tid * kRadixBins + e] = at;
            at += c;
        }
        __syncthreads();
        for (int64_t i = i0; i < i1; ++i) {
            const uint64_t k = src[i];
            dst[cnt[(int)((k >> shift) & (kRadixBins - 1)) * kTermsBlock + tid]++] = k;   // (< L: the counters sum to L)
        }
        __threadfence_block();
        __syncthreads();
        uint64_t* const t = src;
        src = dst;
        dst = t;
    }
    // the sorted row is in src (= alt: an odd number of passes); its entries go over the row's first keys in dst (= keys)
    if (tid == 0) {   // the found keys come first
        int64_t lo = 0, hi = L;
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (tk_is_oov(src[mid])) hi = mid;
            else lo = mid + 1;
        }
        s_found = lo;
    }
    __syncthreads();
    const int64_t F = s_found;
    long long heads = 0, sum = 0;   // carried totals (uniform)
    for (int64_t base = 0; base < F; base += kTermsBlock) {
        const int64_t i = base + tid;
        const bool valid = i < F;
        const uint64_t c = valid ? src[i] : 0ull;
        const uint64_t next = i + 1 < F ? src[i + 1] : ~0ull;
        const bool head = valid && (i == 0 || (c >> 1) != (src[i - 1] >> 1));
        const int v = valid ? tk_value(c) : 0;
        long long total;
        const long long p = block_scan_add<long long, kTermsBlock / 64>(((long long)head << 32) + (long long)v, s_wave, &total);
        const int sl = (int)(unsigned)p, st = (int)(unsigned)total;
        const long long my_heads = heads + ((p - sl) >> 32), my_sum = sum + sl;
        const uint64_t col = (uint64_t)((uint32_t)(c >> kTkColumnShift) ^ flip) << 32;
        if (head) dst[my_heads - 1] = col | (uint64_t)(uint32_t)(int)(my_sum - v);   // the sum in front of the run
        __threadfence_block();
        __syncthreads();
        if (valid && (c >> 1) != (next >> 1)) dst[my_heads - 1] = col | (uint64_t)(uint32_t)(int)(my_sum - (long long)(int)(uint32_t)dst[my_heads - 1]);
        heads += (total - st) >> 32;
        sum += st;
    }
    if (tid == 0) {
        distinct[row] = heads;
        oov[row] = L - F;
    }
}

__global__ __launch_bounds__(kTermsBlock) void k_terms_emit(const uint64_t* __restrict__ keys, const int64_t* __restrict__ row_start, int64_t n_str,
                                                            int64_t n_tok, const int64_t* __restrict__ distinct, const int64_t* __restrict__ indptr,
                                                            const int64_t* __restrict__ nnz_dev, int64_t cap, int32_t* __restrict__ indices,
                                                            int32_t* __restrict__ data) {
    if (*nnz_dev > cap) return;   // the caller's buffers hold `cap` entries: nothing is written when the batch has more
    const int64_t t0 = (int64_t)blockIdx.x * kTermsTile, t1 = min(n_tok, t0 + kTermsTile);
    int64_t lo, end;
    block_rows<kTermsTile>(row_start, n_str, t0, &lo, &end);
    for (int64_t t = t0 + threadIdx.x; t < t1; t += kTermsBlock) {
        const int64_t r = row_of_token(row_start, lo, end, t);   // (>= lo: row_start[lo] <= t0)
        const int64_t j = t - row_start[r];
        if (j < distinct[r]) {
            const uint64_t e = keys[t];
            indices[indptr[r] + j] = (int32_t)(uint32_t)(e >> 32);
            data[indptr[r] + j] = (int32_t)(uint32_t)e;
        }
    }
}

template <typename OUT>
__global__ __launch_bounds__(256) void k_terms_finish(const int64_t* __restrict__ indptr, const int64_t* __restrict__ oov, int64_t n_str,
                                                      OUT* __restrict__ indptr_out, OUT* __restrict__ oov_out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i <= n_str) indptr_out[i] = (OUT)indptr[i];
    if (oov_out && i < n_str) oov_out[i] = (OUT)oov[i];
}

// ---- launchers -----------------------------------------------------------------------------------------------------
hipError_t launch_terms_reduce(uint64_t* keys, uint64_t* alt, const int64_t* row_start, int64_t n_str, int64_t n_tok, bool vocab_form,
                               int64_t* distinct, int64_t* oov, hipStream_t st) {
    if (n_str <= 0 || n_tok <= 0) return hipSuccess;
    const unsigned tiles = (unsigned)(n_tok / kTermsTile + 1);   // (+ 1: rows that start at the token total -- empty -- have an owner too)
    const uint32_t flip = vocab_form ? 0x80000000u : 0u;
    hipLaunchKernelGGL(k_terms_tile, dim3(tiles), dim3(kTermsBlock), 0, st, keys, row_start, n_str, flip, distinct, oov);
    hipLaunchKernelGGL(k_terms_long, dim3(tiles), dim3(kTermsBlock), 0, st, keys, alt, row_start, n_str, flip, distinct, oov);
    return hipGetLastError();
}

hipError_t launch_terms_emit(const uint64_t* keys, const int64_t* row_start, int64_t n_str, int64_t n_tok, const int64_t* distinct,
                             const int64_t* indptr, const int64_t* nnz_dev, int64_t cap, int32_t* indices, int32_t* data, hipStream_t st) {
    if (n_str <= 0 || n_tok <= 0) return hipSuccess;
    const unsigned tiles = (unsigned)((n_tok + kTermsTile - 1) / kTermsTile);
    hipLaunchKernelGGL(k_terms_emit, dim3(tiles), dim3(kTermsBlock), 0, st, keys, row_start, n_str, n_tok, distinct, indptr, nnz_dev, cap, indices,
                       data);
    return hipGetLastError();
}

hipError_t launch_terms_finish(bool out32, const int64_t* indptr, const int64_t* oov, int64_t n_str, void* indptr_out, void* oov_out,
                               hipStream_t st) {
    const dim3 grid((unsigned)((n_str + 256) / 256)), block(256);
    if (out32) hipLaunchKernelGGL((k_terms_finish<int32_t>), grid, block, 0, st, indptr, oov, n_str, (int32_t*)indptr_out, (int32_t*)oov_out);
    else hipLaunchKernelGGL((k_terms_finish<int64_t>), grid, block, 0, st, indptr, oov, n_str, (int64_t*)indptr_out, (int64_t*)oov_out);
    return hipGetLastError();
}

}  // namespace latok
