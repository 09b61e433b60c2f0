// tfidf_kernels.hip -- TF-IDF on a CSR in device memory: the kernels behind latok_idf_* and latok_tfidf_* (tfidf_weight.h holds the
// scalar rules).  The CSR is the caller's, or the one k_terms_emit has just written; indptr is int64 or int32 (IP).
//
//   k_csr_check    one pass over indptr and indices: indptr[0] = 0, non-decreasing, indptr[n_rows] = nnz, every column in
//                  [0, n_cols).  What fails ORs a bit into the error word; every kernel below returns at once when the word is set, so
//                  a refused call has touched neither df nor the output, and no kernel follows an indptr that was not checked.
//   k_df_add       df[c] += 1 for every stored entry: 16-byte loads of four indices, an integer atomic that returns nothing.  The
//                  cached form keeps a tagged table of kDfSlots columns per workgroup in LDS: an entry whose column owns (or wins)
//                  its slot is an LDS atomic, any other goes to memory; every occupied slot costs one global atomic at the end.
//                  Integer addition commutes: both forms give the same df whatever the order.
//   k_idf_weights  df, n_docs -> float32 idf[n_cols], in double (tw_idf)
//   k_tfidf_rows   the short rows.  A wave owns four consecutive rows, one per DPP row of 16 lanes.  A row of at most kTfidfSubMax
//                  entries is taken by its 16 lanes: lane l holds entries l, l + 16, l + 32, l + 48 in registers, adds their norm
//                  terms in that order, row16_sum_f32 adds the 16 partial sums, and the lanes scale what they hold.  A row of up to
//                  kTfidfWaveMax entries is then taken by the whole wave, one such row after the other: lane l strides over entries
//                  l, l + 64, ..; wave_sum_f32; a second pass over the weights it stored scales them.
//   k_tfidf_long   a row of more than kTfidfWaveMax entries, one workgroup (second launch): entry space is cut into tiles of
//                  kTfidfWaveMax entries, at most one long row starts in a tile, and the tile's workgroup takes it -- thread t strides
//                  over entries t, t + 256, ..; the four wave sums are added in wave order.
// Which lanes take a row, and in which order they add, follows from the row's LENGTH alone: a row's output bits do not depend on
// where it sits in the batch or on its neighbours.  No floating-point atomic; no kernel waits for another workgroup; all stores are
// vector stores from plain C++.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "kernels.h"
#include "tfidf_weight.h"
#include "wave_ops.h"

namespace latok {

constexpr int kTfidfBlock = 256;
constexpr int kTfidfGroup = 16;                                  // lanes of a short row: one DPP row
constexpr int kTfidfPer = kTfidfSubMax / kTfidfGroup;            // entries a lane of the group holds
constexpr int kTfidfRowsPerBlock = kTfidfBlock / kTfidfGroup;    // 16
static_assert(kTfidfSubMax % kTfidfGroup == 0 && kTfidfWaveMax > kTfidfSubMax, "the tiers of k_tfidf_rows");
constexpr int kDfBlock = 256;
constexpr int kDfChunk = 16384;                                  // entries a workgroup of k_df_add takes
static_assert((kDfSlots & (kDfSlots - 1)) == 0 && kDfChunk % (4 * kDfBlock) == 0, "the slot is a masked hash; chunks are whole rounds of int4 loads");

// the batch's entry count: the host's, or the scan's own word when the host has not read it yet (then nothing runs beyond `cap`
// entries, which is what the buffers hold)
__device__ __forceinline__ int64_t entries_of(int64_t nnz, const int64_t* __restrict__ nnz_dev, int64_t cap) {
    if (!nnz_dev) return nnz;
    const int64_t n = *nnz_dev;
    return n > cap ? -1 : n;
}

template <typename IP>
__global__ __launch_bounds__(256) void k_csr_check(const IP* __restrict__ indptr, const int32_t* __restrict__ indices, int64_t n_rows, int64_t nnz,
                                                   const int64_t* __restrict__ nnz_dev, int64_t cap, int64_t n_cols, int* __restrict__ err) {
    const int64_t n = entries_of(nnz, nnz_dev, cap);
    if (n < 0) return;
    const int64_t span = indptr ? max(n_rows + 1, n) : n;
    int bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < span; i += (int64_t)gridDim.x * 256) {
        if (indptr && i <= n_rows) {
            const int64_t p = (int64_t)indptr[i];
            if (i == 0 && p != 0) bad |= kCsrBadStart;
            if (i < n_rows && (int64_t)indptr[i + 1] < p) bad |= kCsrBadOrder;
            if (i == n_rows && p != n) bad |= kCsrBadTotal;
        }
        if (n_cols > 0 && i < n && (uint64_t)(int64_t)indices[i] >= (uint64_t)n_cols) bad |= kCsrBadColumn;
    }
    if (bad) atomicOr(err, bad);
}

__device__ __forceinline__ void df_add_global(int32_t* __restrict__ df, int c) { (void)atomicAdd(df + c, 1); }

// the entries [lo, hi) of the workgroup, four at a time where the address allows it
template <class F>
__device__ __forceinline__ void df_for_each(const int32_t* __restrict__ indices, int64_t lo, int64_t hi, F f) {
    const int64_t head = min(hi, lo + (int64_t)(((16 - ((uintptr_t)(indices + lo) & 15)) & 15) >> 2));   // up to the first 16-byte boundary
    const int64_t quads = (hi - head) >> 2, tail = head + 4 * quads;
    for (int64_t i = lo + threadIdx.x; i < head; i += kDfBlock) f(indices[i]);
    const int4* __restrict__ v = (const int4*)(indices + head);
    for (int64_t q = threadIdx.x; q < quads; q += kDfBlock) {
        const int4 x = v[q];
        f(x.x);
        f(x.y);
        f(x.z);
        f(x.w);
    }
    for (int64_t i = tail + threadIdx.x; i < hi; i += kDfBlock) f(indices[i]);
}

__global__ __launch_bounds__(kDfBlock) void k_df_add_plain(const int32_t* __restrict__ indices, int64_t nnz, const int64_t* __restrict__ nnz_dev,
                                                           int64_t cap, const int* __restrict__ err, int32_t* __restrict__ df) {
    const int64_t n = entries_of(nnz, nnz_dev, cap);
    if (n < 0 || *err) return;
    const int64_t lo = (int64_t)blockIdx.x * kDfChunk, hi = min(n, lo + kDfChunk);
    if (lo >= hi) return;
    df_for_each(indices, lo, hi, [&](int c) { df_add_global(df, c); });
}

__global__ __launch_bounds__(kDfBlock) void k_df_add(const int32_t* __restrict__ indices, int64_t nnz, const int64_t* __restrict__ nnz_dev, int64_t cap,
                                                     const int* __restrict__ err, int32_t* __restrict__ df) {
    __shared__ int tag[kDfSlots];
    __shared__ int cnt[kDfSlots];
    const int64_t n = entries_of(nnz, nnz_dev, cap);
    if (n < 0 || *err) return;   // (uniform)
    const int64_t lo = (int64_t)blockIdx.x * kDfChunk, hi = min(n, lo + kDfChunk);
    if (lo >= hi) return;        // (uniform)
    for (int s = threadIdx.x; s < kDfSlots; s += kDfBlock) {
        tag[s] = -1;   // (a checked column is >= 0)
        cnt[s] = 0;
    }
    __syncthreads();
    df_for_each(indices, lo, hi, [&](int c) {
        const int s = (int)(((uint32_t)c * 2654435761u) >> 16) & (kDfSlots - 1);
        int owner = __hip_atomic_load(&tag[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (owner == -1) {
            owner = atomicCAS(&tag[s], -1, c);
            if (owner == -1) owner = c;
        }
        if (owner == c) (void)atomicAdd(&cnt[s], 1);
        else df_add_global(df, c);
    });
    __syncthreads();
    for (int s = threadIdx.x; s < kDfSlots; s += kDfBlock) {
        const int c = tag[s], k = cnt[s];
        if (c >= 0 && k > 0) (void)atomicAdd(df + c, k);
    }
}

__global__ __launch_bounds__(256) void k_idf_weights(const int32_t* __restrict__ df, int64_t n_cols, int64_t n_docs, int smooth, float* __restrict__ idf) {
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < n_cols; c += (int64_t)gridDim.x * 256) idf[c] = tw_idf(df[c], n_docs, smooth != 0);
}

// the weight of entry j before the norm
__device__ __forceinline__ float tfidf_w(const int32_t* __restrict__ indices, const int32_t* data, const float* __restrict__ idf, int64_t j, bool sub) {
    const float tf = tw_tf(data[j], sub);
    return idf ? tw_weight(tf, idf[indices[j]]) : tf;
}

// One row [s, e) by the G lanes that hold lane numbers l = 0 .. G - 1, G = 64 (the wave) or 256 (the workgroup, through `s_part`):
// the weights go to out[] in the first pass and are scaled in the second; every lane reads back only what it stored itself.
template <int G>
__device__ __forceinline__ void tfidf_row_strided(const int32_t* __restrict__ indices, const int32_t* data, const float* __restrict__ idf, int64_t s,
                                                  int64_t e, int l, int opts, float* out, float* s_part) {
    const bool sub = (opts & kTwSublinearTf) != 0, l2 = (opts & kTwNormL2) != 0, normed = (opts & (kTwNormL1 | kTwNormL2)) != 0;
    float acc = 0.0f;
    for (int64_t j = s + l; j < e; j += G) {
        const float w = tfidf_w(indices, data, idf, j, sub);
        if (!normed) out[j] = tw_scale(w, 1.0f);
        else {
            out[j] = w;
            acc += tw_term(w, l2);
        }
    }
    if (!normed) return;   // (uniform)
    float sum = wave_sum_f32(acc);
    if (G > 64) {
        const int wave = threadIdx.x >> 6;
        __syncthreads();   // (s_part may still be read from the row before)
        if ((threadIdx.x & 63) == 0) s_part[wave] = sum;
        __syncthreads();
        sum = (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
    }
    const float norm = tw_norm(sum, l2);
    for (int64_t j = s + l; j < e; j += G) out[j] = tw_scale(out[j], norm);
}

template <typename IP>
__global__ __launch_bounds__(kTfidfBlock) void k_tfidf_rows(const IP* __restrict__ indptr, const int32_t* __restrict__ indices, const int32_t* data,
                                                            int64_t n_rows, int64_t nnz, const int64_t* __restrict__ nnz_dev, int64_t cap,
                                                            const float* __restrict__ idf, int opts, const int* __restrict__ err, float* out) {
    if (entries_of(nnz, nnz_dev, cap) < 0 || (err && *err)) return;   // (uniform)
    const bool sub = (opts & kTwSublinearTf) != 0, l2 = (opts & kTwNormL2) != 0, normed = (opts & (kTwNormL1 | kTwNormL2)) != 0;
    const int lane = threadIdx.x & 63, l = lane & (kTfidfGroup - 1);
    const int64_t row = (int64_t)blockIdx.x * kTfidfRowsPerBlock + (threadIdx.x >> 4);
    // every lane stays active to the end: the DPP sums read all 16 lanes of a row, the wave sums all 64
    int64_t s = 0, e = 0;
    if (row < n_rows) {
        s = (int64_t)indptr[row];
        e = (int64_t)indptr[row + 1];
    }
    const int64_t len = e - s;
    const bool mine = len <= kTfidfSubMax;
    float w[kTfidfPer], acc = 0.0f;
#pragma unroll
    for (int k = 0; k < kTfidfPer; ++k) {
        const int64_t j = s + l + k * kTfidfGroup;
        w[k] = 0.0f;
        if (mine && j < e) {
            w[k] = tfidf_w(indices, data, idf, j, sub);
            acc += tw_term(w[k], l2);
        }
    }
    const float norm = normed ? tw_norm(row16_sum_f32(acc), l2) : 1.0f;
#pragma unroll
    for (int k = 0; k < kTfidfPer; ++k) {
        const int64_t j = s + l + k * kTfidfGroup;
        if (mine && j < e) out[j] = tw_scale(w[k], norm);
    }
    // the wave's rows of kTfidfSubMax + 1 .. kTfidfWaveMax entries, one after the other on all 64 lanes
#pragma unroll
    for (int q = 0; q < 64 / kTfidfGroup; ++q) {
        const int64_t qs = lane_read64(s, q * kTfidfGroup), qe = lane_read64(e, q * kTfidfGroup);
        if (qe - qs > kTfidfSubMax && qe - qs <= kTfidfWaveMax) tfidf_row_strided<64>(indices, data, idf, qs, qe, lane, opts, out, nullptr);
    }
}

template <typename IP>
__global__ __launch_bounds__(kTfidfBlock) void k_tfidf_long(const IP* __restrict__ indptr, const int32_t* __restrict__ indices, const int32_t* data,
                                                            int64_t n_rows, int64_t nnz, const int64_t* __restrict__ nnz_dev, int64_t cap,
                                                            const float* __restrict__ idf, int opts, const int* __restrict__ err, float* out) {
    __shared__ float s_part[kTfidfBlock / 64];
    __shared__ int64_t s_row;
    const int64_t n = entries_of(nnz, nnz_dev, cap);
    if (n < 0 || (err && *err)) return;   // (uniform)
    const int64_t t0 = (int64_t)blockIdx.x * kTfidfWaveMax;
    if (t0 >= n) return;
    if (threadIdx.x == 0) {   // the last row that starts below the tile's end: the only one that can start in the tile and be long
        int64_t lo = 0, hi = n_rows;
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if ((int64_t)indptr[mid] < t0 + kTfidfWaveMax) lo = mid + 1;
            else hi = mid;
        }
        const int64_t r = lo - 1;
        s_row = (r >= 0 && (int64_t)indptr[r] >= t0 && (int64_t)indptr[r + 1] - (int64_t)indptr[r] > kTfidfWaveMax) ? r : -1;
    }
    __syncthreads();
    const int64_t r = s_row;
    if (r < 0) return;   // (uniform)
    tfidf_row_strided<kTfidfBlock>(indices, data, idf, (int64_t)indptr[r], (int64_t)indptr[r + 1], threadIdx.x, opts, out, s_part);
}

// ---- launchers -----------------------------------------------------------------------------------------------------
static unsigned stride_grid(int64_t items) { return (unsigned)std::min<int64_t>(std::max<int64_t>((items + 255) / 256, 1), 2048); }

hipError_t launch_csr_check(bool ip32, const void* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int64_t* nnz_dev, int64_t cap,
                            int64_t n_cols, int* err, hipStream_t st) {
    const int64_t bound = nnz_dev ? cap : nnz;
    const unsigned grid = stride_grid(std::max(indptr ? n_rows + 1 : 0, bound));
    if (ip32) hipLaunchKernelGGL((k_csr_check<int32_t>), dim3(grid), dim3(256), 0, st, (const int32_t*)indptr, indices, n_rows, nnz, nnz_dev, cap, n_cols, err);
    else hipLaunchKernelGGL((k_csr_check<int64_t>), dim3(grid), dim3(256), 0, st, (const int64_t*)indptr, indices, n_rows, nnz, nnz_dev, cap, n_cols, err);
    return hipGetLastError();
}

hipError_t launch_df_add(bool cached, const int32_t* indices, int64_t nnz, const int64_t* nnz_dev, int64_t cap, const int* err, int32_t* df,
                         hipStream_t st) {
    const int64_t bound = nnz_dev ? cap : nnz;
    if (bound <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((bound + kDfChunk - 1) / kDfChunk);
    if (cached) hipLaunchKernelGGL(k_df_add, dim3(grid), dim3(kDfBlock), 0, st, indices, nnz, nnz_dev, cap, err, df);
    else hipLaunchKernelGGL(k_df_add_plain, dim3(grid), dim3(kDfBlock), 0, st, indices, nnz, nnz_dev, cap, err, df);
    return hipGetLastError();
}

hipError_t launch_idf_weights(const int32_t* df, int64_t n_cols, int64_t n_docs, bool smooth, float* idf, hipStream_t st) {
    hipLaunchKernelGGL(k_idf_weights, dim3(stride_grid(n_cols)), dim3(256), 0, st, df, n_cols, n_docs, smooth ? 1 : 0, idf);
    return hipGetLastError();
}

hipError_t launch_tfidf_rows(bool ip32, const void* indptr, const int32_t* indices, const int32_t* data, int64_t n_rows, int64_t nnz,
                             const int64_t* nnz_dev, int64_t cap, const float* idf, int opts, const int* err, float* out, hipStream_t st) {
    const int64_t bound = nnz_dev ? cap : nnz;
    if (n_rows <= 0 || bound <= 0) return hipSuccess;
    const dim3 rows((unsigned)((n_rows + kTfidfRowsPerBlock - 1) / kTfidfRowsPerBlock)), tiles((unsigned)((bound + kTfidfWaveMax - 1) / kTfidfWaveMax));
    if (ip32) {
        hipLaunchKernelGGL((k_tfidf_rows<int32_t>), rows, dim3(kTfidfBlock), 0, st, (const int32_t*)indptr, indices, data, n_rows, nnz, nnz_dev, cap, idf, opts, err, out);
        if (bound > kTfidfWaveMax)
            hipLaunchKernelGGL((k_tfidf_long<int32_t>), tiles, dim3(kTfidfBlock), 0, st, (const int32_t*)indptr, indices, data, n_rows, nnz, nnz_dev, cap, idf, opts, err, out);
    } else {
        hipLaunchKernelGGL((k_tfidf_rows<int64_t>), rows, dim3(kTfidfBlock), 0, st, (const int64_t*)indptr, indices, data, n_rows, nnz, nnz_dev, cap, idf, opts, err, out);
        if (bound > kTfidfWaveMax)
            hipLaunchKernelGGL((k_tfidf_long<int64_t>), tiles, dim3(kTfidfBlock), 0, st, (const int64_t*)indptr, indices, data, n_rows, nnz, nnz_dev, cap, idf, opts, err, out);
    }
    return hipGetLastError();
}

}  // namespace latok
