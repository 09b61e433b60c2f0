// detok_kernels.hip -- decoding on the device: ids back to UTF-8 bytes (latok_detok_csr / latok_detok_padded, include/latok_hip.h; the
// object, the lookup and the per-piece rule: detok.h).  PIECE SPACE is the ids of a CSR, or the cells of the padded [n_rows, L] block
// (a cell at or behind its row's length is a dropped piece).  One stream:
//   k_detok_lengths  padded form with lengths: a length outside [0, L] ORs kDetokBadLength into the error word (the CSR form's word is
//                    k_csr_check's); every kernel below returns at once when the word is set
//   k_detok_widen    CSR form with an int32 indptr: the row starts as int64, what block_rows reads
//   k_detok_count    one thread per piece, kDetokBlock pieces per workgroup: the piece's row (block_rows / row_of_token, or a
//                    division), the id lookup, the rule and the look-back of detok.h; the piece's output bytes (uint32), the
//                    workgroup's sum, the unknown ids (one atomic per workgroup that met any)
//   k_scan_chained   the workgroup sums -> each workgroup's first output byte; THE byte total (launch_tile_scan, unchanged)
//   k_detok_write    the same workgroups.  Always: out_off[s] of every row that starts among the workgroup's pieces = its first byte +
//                    the prefix of the row's first piece (block_scan_add); the last workgroup also gives the rows that start behind
//                    the last piece, out_off[n_rows] among them, the total.  If total <= capacity: the workgroup's pieces own one
//                    contiguous output range; it is assembled in an LDS window of kDetokWin bytes whose byte j lies 16-byte-congruent
//                    to its address, window by window for a longer range, and every window leaves as aligned 16-byte stores with
//                    dword and byte stores on its ragged ends only -- one writer per byte, whatever the neighbours do.  A piece puts at
//                    most kDetokLaneBytes bytes into a window by its own lane; a longer stretch is queued in LDS and copied by the
//                    whole workgroup, byte j by thread j mod kDetokBlock.
// The window: kDetokBlock pieces of running text are 1 .. 1.5 KiB of output, so 4 KiB holds a workgroup's range in one round up to an
// average of 16 bytes per piece; with the row prefixes (2 KiB), the queue (1.5 KiB) and the scan's words a workgroup keeps under 8 KiB
// of LDS, and eight workgroups -- 32 waves, the CU's limit -- fit beside each other.  Lanes write consecutive bytes of consecutive
// pieces and the store phase reads 16 consecutive bytes per lane: neither has a bank conflict by construction of the addresses.
// No kernel waits for another workgroup beyond the scan's own protocol; all stores are vector stores from plain C++.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_ops.h"
#include "detok.h"
#include "kernels.h"

namespace latok {

constexpr int kDetokWaves = kDetokBlock / 64;
constexpr int kDetokQueue = kDetokWin / kDetokLaneBytes;   // stretches of more than kDetokLaneBytes bytes that fit one window

__global__ __launch_bounds__(256) void k_detok_lengths(const int32_t* __restrict__ lengths, int64_t n_rows, int64_t max_length, int* __restrict__ err) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s < n_rows && (lengths[s] < 0 || (int64_t)lengths[s] > max_length)) atomicOr(err, kDetokBadLength);
}
__global__ __launch_bounds__(256) void k_detok_widen(const int32_t* __restrict__ indptr, int64_t n, int64_t* __restrict__ row_start) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s < n) row_start[s] = indptr[s];
}

// The piece of this lane: t, whether it is a cell of its row (real), and the first piece of its row.  Every thread of the workgroup
// calls it before any divergent return (block_rows holds a barrier).
struct DetokLane {
    int64_t t, row_first;
    bool real;
};
template <bool PADDED>
__device__ __forceinline__ DetokLane detok_lane(const DetokRows& R) {
    const int64_t t0 = (int64_t)blockIdx.x * kDetokBlock, t = t0 + threadIdx.x;
    DetokLane k{t, 0, false};
    if (PADDED) {
        if (t >= R.n_cells) return k;
        const int64_t r = t / R.max_length;
        int64_t len = R.lengths ? (int64_t)R.lengths[r] : R.max_length;
        len = len < 0 ? 0 : (len > R.max_length ? R.max_length : len);
        k.row_first = r * R.max_length;
        k.real = t - k.row_first < len;
        return k;
    }
    int64_t lo, end;
    block_rows<kDetokBlock>(R.row_start, R.n_rows, t0, &lo, &end);
    if (t >= R.n_cells) return k;
    int64_t r = row_of_token(R.row_start, lo, end, t);
    r = r < 0 ? 0 : (r >= R.n_rows ? R.n_rows - 1 : r);
    const int64_t first = R.row_start[r];
    k.row_first = first < 0 ? 0 : (first > t ? t : first);   // (a checked CSR gives 0 <= first <= t)
    k.real = true;
    return k;
}
__device__ __forceinline__ int32_t detok_entry(const DetokTable& T, const DetokSkip& S, int32_t id, bool* unknown) {
    *unknown = false;
    if (dt_skipped(S.id, S.n, id)) return -1;
    const int32_t* keys = T.keys;
    const int32_t* vals = T.vals;
    const int32_t e = dt_lookup(T.map, [keys](int64_t i) { return keys[i]; }, [vals](int64_t i) { return vals[i]; }, id);
    *unknown = e < 0;
    return e;
}

template <bool PADDED>
__global__ __launch_bounds__(kDetokBlock) void k_detok_count(DetokTable T, DetokRows R, const int32_t* __restrict__ ids, DetokSkip S,
                                                             const int* __restrict__ err, uint32_t* __restrict__ cnt,
                                                             int64_t* __restrict__ wg_sum, unsigned long long* __restrict__ n_unknown) {
    __shared__ long long s_scan[kDetokWaves];
    if (*err) {   // (uniform) the rows were refused: nothing is read through them
        if (threadIdx.x == 0) wg_sum[blockIdx.x] = 0;
        return;
    }
    const DetokLane k = detok_lane<PADDED>(R);
    uint32_t c = 0;
    bool unknown = false;
    if (k.real) {
        const int32_t e = detok_entry(T, S, ids[k.t], &unknown);
        if (e >= 0) {
            const DtEntry rec = reinterpret_cast<const DtEntry*>(T.entries)[e];
            bool has_prev = false;
            if (dt_needs_prev(rec, T.mode))
                has_prev = dt_has_prev(k.t, k.row_first, [&](int64_t u) {
                    bool unk;
                    return detok_entry(T, S, ids[u], &unk) >= 0;
                });
            c = dt_piece_bytes(dt_piece(rec, T.mode, has_prev));
        }
    }
    if (k.t < R.n_cells) cnt[k.t] = c;
    long long total;
    (void)block_scan_add<long long, kDetokWaves>((long long)c, s_scan, &total);
    const int n_unk = __syncthreads_count(unknown ? 1 : 0);
    if (threadIdx.x == 0) {
        wg_sum[blockIdx.x] = total;
        if (n_unk > 0) atomicAdd(n_unknown, (unsigned long long)n_unk);
    }
}

struct DetokStretch {   // a queued copy: output bytes [k0, k1) of piece p go to window bytes j0 ..
    DtPiece p;
    uint32_t k0, k1;   // (a piece's byte count is a uint32; a stretch lies inside one window)
    int j0;
};

template <bool PADDED>
__global__ __launch_bounds__(kDetokBlock) void k_detok_write(DetokTable T, DetokRows R, const int32_t* __restrict__ ids, DetokSkip S,
                                                             const int* __restrict__ err, const uint32_t* __restrict__ cnt,
                                                             const int64_t* __restrict__ wg_rank, const int64_t* __restrict__ total_dev,
                                                             uint8_t* __restrict__ out, int64_t cap, int64_t* __restrict__ out_off) {
    __shared__ long long s_scan[kDetokWaves];
    __shared__ long long s_pref[kDetokBlock];
    __shared__ __attribute__((aligned(16))) uint8_t s_win[kDetokWin];
    __shared__ DetokStretch s_q[kDetokQueue];
    __shared__ int s_qn;
    if (*err) return;   // (uniform)
    const int tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * kDetokBlock, t = t0 + tid;
    const int64_t n_total = *total_dev, g0 = wg_rank[blockIdx.x];
    const uint32_t c = t < R.n_cells ? cnt[t] : 0u;
    long long wg_total;
    const long long excl = block_scan_add<long long, kDetokWaves>((long long)c, s_scan, &wg_total) - (long long)c;
    s_pref[tid] = excl;   // (a thread behind the last piece holds the workgroup's total)
    if (tid == 0) s_qn = 0;
    __syncthreads();
    // ---- the rows that start among this workgroup's pieces
    const bool last = blockIdx.x == gridDim.x - 1;
    if (PADDED) {
        for (int64_t r = (t0 + R.max_length - 1) / R.max_length + tid; r < R.n_rows && r * R.max_length < t0 + kDetokBlock; r += kDetokBlock)
            out_off[r] = g0 + s_pref[r * R.max_length - t0];
        if (last && tid == 0) out_off[R.n_rows] = n_total;
    } else {
        int64_t lo, end;
        block_rows<kDetokBlock>(R.row_start, R.n_rows, t0, &lo, &end);
        for (int64_t r = lo + tid; r < end; r += kDetokBlock) {
            const int64_t p = R.row_start[r];
            if (p >= t0 && p < t0 + kDetokBlock) out_off[r] = g0 + s_pref[p - t0];
        }
        if (last)
            for (int64_t r = end + tid; r <= R.n_rows; r += kDetokBlock) out_off[r] = n_total;
    }
    // ---- the bytes.  The caller's buffer holds `cap` bytes; when the batch needs more, nothing is written.
    if (!out || n_total > cap || wg_total <= 0) return;   // (uniform)
    uint8_t* dst = out + g0;
    const int a = (int)((uintptr_t)dst & 15u);   // x = a + (byte of the workgroup's range): window byte x mod kDetokWin <-> dst - a + x
    uint8_t* base = dst - a;
    const long long x0 = a + excl, x1 = x0 + (long long)c, x_end = a + wg_total;
    DtPiece p{0u, 0u, 0u};
    if (c > 0u) {
        bool unk;
        const int32_t e = detok_entry(T, S, ids[t], &unk);
        if (e >= 0) p = dt_piece_of_count(reinterpret_cast<const DtEntry*>(T.entries)[e], c);
    }
    const long long x_mine = x0 + (long long)dt_piece_bytes(p);   // (== x1 unless the ids changed between the passes)
    const long long x_hi = x_mine < x1 ? x_mine : x1;
    const uint32_t* blob = T.blob;
    auto ld = [blob](uint64_t i) { return blob[i]; };
    for (long long w0 = 0; w0 < x_end; w0 += kDetokWin) {   // (uniform)
        const long long w1 = w0 + kDetokWin < x_end ? w0 + kDetokWin : x_end;
        const long long lo_i = x0 > w0 ? x0 : w0, hi_i = x_hi < w1 ? x_hi : w1;
        if (lo_i < hi_i) {
            const uint64_t k0 = (uint64_t)(lo_i - x0), k1 = (uint64_t)(hi_i - x0);
            const int j0 = (int)(lo_i - w0);
            if (hi_i - lo_i <= kDetokLaneBytes) {
                dt_copy(p, T.sep, ld, k0, k1, [&](uint64_t k, uint32_t b) { s_win[j0 + (int)(k - k0)] = (uint8_t)b; });
            } else {
                const int q = atomicAdd(&s_qn, 1);   // (< kDetokQueue: the stretches are disjoint, each longer than kDetokLaneBytes)
                if (q < kDetokQueue) s_q[q] = DetokStretch{p, (uint32_t)k0, (uint32_t)k1, j0};
            }
        }
        __syncthreads();
        const int nq = s_qn < kDetokQueue ? s_qn : kDetokQueue;
        for (int q = 0; q < nq; ++q) {   // (uniform)
            const DetokStretch s = s_q[q];
            const uint64_t k0 = s.k0;
            const int n = (int)(s.k1 - s.k0);
            for (int j = tid; j < n; j += kDetokBlock)
                dt_copy(s.p, T.sep, ld, k0 + (uint64_t)j, k0 + (uint64_t)j + 1u, [&](uint64_t, uint32_t b) { s_win[s.j0 + j] = (uint8_t)b; });
        }
        __syncthreads();
        if (tid == 0) s_qn = 0;
        // window bytes [lo, hi) -> base + w0 + [lo, hi): 16-byte groups, dwords and bytes on the ragged ends
        const int lo = w0 == 0 ? a : 0, hi = (int)(w1 - w0);
        uint8_t* g = base + w0;
        const int d0 = (lo + 3) & ~3, d1 = hi & ~3;
        if (d0 >= d1) {
            for (int j = lo + tid; j < hi; j += kDetokBlock) g[j] = s_win[j];
        } else {
            const int q0 = (d0 + 15) & ~15, q1 = d1 & ~15;
            for (int j = lo + tid; j < d0; j += kDetokBlock) g[j] = s_win[j];
            for (int j = d1 + tid; j < hi; j += kDetokBlock) g[j] = s_win[j];
            if (q0 < q1) {
                for (int j = d0 + 4 * tid; j < q0; j += 4 * kDetokBlock) *reinterpret_cast<uint32_t*>(g + j) = *reinterpret_cast<const uint32_t*>(s_win + j);
                for (int j = q0 + 16 * tid; j < q1; j += 16 * kDetokBlock) *reinterpret_cast<uint4*>(g + j) = *reinterpret_cast<const uint4*>(s_win + j);
                for (int j = q1 + 4 * tid; j < d1; j += 4 * kDetokBlock) *reinterpret_cast<uint32_t*>(g + j) = *reinterpret_cast<const uint32_t*>(s_win + j);
            } else {
                for (int j = d0 + 4 * tid; j < d1; j += 4 * kDetokBlock) *reinterpret_cast<uint32_t*>(g + j) = *reinterpret_cast<const uint32_t*>(s_win + j);
            }
        }
        __syncthreads();   // (the window and the queue counter are free again)
    }
}

int64_t detok_groups(int64_t n_cells) { return n_cells > 0 ? (n_cells + kDetokBlock - 1) / kDetokBlock : 0; }

hipError_t launch_detok_lengths(const int32_t* lengths, int64_t n_rows, int64_t max_length, int* err, hipStream_t st) {
    if (!lengths || n_rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_detok_lengths, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, st, lengths, n_rows, max_length, err);
    return hipGetLastError();
}
hipError_t launch_detok_widen(const int32_t* indptr, int64_t n, int64_t* row_start, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_detok_widen, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, indptr, n, row_start);
    return hipGetLastError();
}
hipError_t launch_detok_count(const DetokTable& T, const DetokRows& R, const int32_t* ids, const DetokSkip& S, const int* err, uint32_t* cnt,
                              int64_t* wg_sum, unsigned long long* n_unknown, hipStream_t st) {
    const int64_t nb = detok_groups(R.n_cells);
    if (nb <= 0) return hipSuccess;
    if (R.row_start) hipLaunchKernelGGL((k_detok_count<false>), dim3((unsigned)nb), dim3(kDetokBlock), 0, st, T, R, ids, S, err, cnt, wg_sum, n_unknown);
    else hipLaunchKernelGGL((k_detok_count<true>), dim3((unsigned)nb), dim3(kDetokBlock), 0, st, T, R, ids, S, err, cnt, wg_sum, n_unknown);
    return hipGetLastError();
}
hipError_t launch_detok_write(const DetokTable& T, const DetokRows& R, const int32_t* ids, const DetokSkip& S, const int* err, const uint32_t* cnt,
                              const int64_t* wg_rank, const int64_t* total_dev, uint8_t* out, int64_t cap, int64_t* out_off, hipStream_t st) {
    const int64_t nb = detok_groups(R.n_cells);
    if (nb <= 0) return hipSuccess;
    if (R.row_start) hipLaunchKernelGGL((k_detok_write<false>), dim3((unsigned)nb), dim3(kDetokBlock), 0, st, T, R, ids, S, err, cnt, wg_rank, total_dev, out, cap, out_off);
    else hipLaunchKernelGGL((k_detok_write<true>), dim3((unsigned)nb), dim3(kDetokBlock), 0, st, T, R, ids, S, err, cnt, wg_rank, total_dev, out, cap, out_off);
    return hipGetLastError();
}

}  // namespace latok
