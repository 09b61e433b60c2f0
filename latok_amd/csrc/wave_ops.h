// wave_ops.h -- what the 64 lanes of one wavefront do with each other: the LDS-only wave fence, moves and reductions on
// DPP / readlane, the __shfl_up scans of the counting kernels, a 64-ary search by ballot.  Device code only; shared by every
// kernel source so that a kernel calls these instead of carrying a copy.
#ifndef LATOK_WAVE_OPS_H
#define LATOK_WAVE_OPS_H
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace latok {

__device__ __forceinline__ void wave_lds_sync() {
    // LDS traffic of one wave is executed in issue order; this only stops the compiler from reordering across it
    // fences restricted to the LDS address space: a plain wavefront fence makes hipcc drain vmcnt(0) as well, i.e.
    // wait for this tile's output store (and any load in flight) before the next tile's loads can be issued
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
}

// ---- cross-lane helpers on DPP / readlane (no LDS round trip, unlike ds_bpermute-based __shfl) -----------------
// update_dpp(old, src, ctrl, row_mask, bank_mask, bound_ctrl=false): lanes without a valid source keep `old`.
constexpr int kDppRowShr1 = 0x111, kDppRowShr2 = 0x112, kDppRowShr4 = 0x114, kDppRowShr8 = 0x118;
constexpr int kDppRowBcast15 = 0x142, kDppRowBcast31 = 0x143, kDppWaveShl1 = 0x130, kDppWaveShr1 = 0x138;

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_mov(int old, int src) {
    return __builtin_amdgcn_update_dpp(old, src, CTRL, ROW_MASK, 0xF, false);
}
__device__ __forceinline__ int lane_read(int v, int uniform_lane) { return __builtin_amdgcn_readlane(v, uniform_lane); }
// values that are wave-uniform by construction but live in VGPRs: move them to SGPRs
__device__ __forceinline__ int to_scalar(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int64_t to_scalar64(int64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ int64_t lane_read64(int64_t v, int uniform_lane) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, uniform_lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), uniform_lane);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ int wave_sum(int v) {
    v += dpp_mov<kDppRowShr1, 0xF>(0, v);
    v += dpp_mov<kDppRowShr2, 0xF>(0, v);
    v += dpp_mov<kDppRowShr4, 0xF>(0, v);
    v += dpp_mov<kDppRowShr8, 0xF>(0, v);   // lane 15 of every row now holds its row's sum
    return lane_read(v, 15) + lane_read(v, 31) + lane_read(v, 47) + lane_read(v, 63);
}

// float32 sum over every DPP row (16 lanes) of the wave, in every lane of the row: a butterfly of mirrors, so that each step adds
// the same two values in both lanes of a pair (a + b = b + a bit for bit) and all 16 lanes end with the same bits.  The order of the
// additions is fixed by the lane numbers inside the row alone.
constexpr int kDppRowMirror = 0x140, kDppRowHalfMirror = 0x141, kDppQuadMirror = 0x1B, kDppQuadSwap = 0xB1;
template <int CTRL>
__device__ __forceinline__ float dpp_movf(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float row16_sum_f32(float v) {
    v += dpp_movf<kDppRowMirror>(v);       // lane i with lane 15 - i
    v += dpp_movf<kDppRowHalfMirror>(v);   // lane i with lane 7 - i of its half
    v += dpp_movf<kDppQuadMirror>(v);      // lane i with lane 3 - i of its quad
    v += dpp_movf<kDppQuadSwap>(v);        // lanes 0 <-> 1, 2 <-> 3
    return v;
}
// ... and over the whole wave, wave-uniform: the four row sums in the fixed order (r0 + r1) + (r2 + r3)
__device__ __forceinline__ float wave_sum_f32(float v) {
    const int r = __float_as_int(row16_sum_f32(v));
    return (__int_as_float(lane_read(r, 0)) + __int_as_float(lane_read(r, 16))) + (__int_as_float(lane_read(r, 32)) + __int_as_float(lane_read(r, 48)));
}

// inclusive prefix maximum over the 64 lanes of values >= `floor` (six DPP steps; the __shfl_up form is six dependent
// ds_bpermute round trips through the LDS pipe, ~0.7 us per call at the occupancy of the featurize kernel)
__device__ __forceinline__ int wave_scan_max(int v, int floor) {
    v = max(v, dpp_mov<kDppRowShr1, 0xF>(floor, v));
    v = max(v, dpp_mov<kDppRowShr2, 0xF>(floor, v));
    v = max(v, dpp_mov<kDppRowShr4, 0xF>(floor, v));
    v = max(v, dpp_mov<kDppRowShr8, 0xF>(floor, v));
    v = max(v, dpp_mov<kDppRowBcast15, 0xA>(floor, v));
    v = max(v, dpp_mov<kDppRowBcast31, 0xC>(floor, v));
    return v;
}
// maximum over the wave, in every lane (wave-uniform)
__device__ __forceinline__ int wave_max(int v, int floor) { return lane_read(wave_scan_max(v, floor), 63); }

// unsigned minimum over the wave, in every lane (wave-uniform): the same six DPP steps; a lane without a source takes 0xFFFFFFFF
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
    v = min(v, (uint32_t)dpp_mov<kDppRowShr1, 0xF>(-1, (int)v));
    v = min(v, (uint32_t)dpp_mov<kDppRowShr2, 0xF>(-1, (int)v));
    v = min(v, (uint32_t)dpp_mov<kDppRowShr4, 0xF>(-1, (int)v));
    v = min(v, (uint32_t)dpp_mov<kDppRowShr8, 0xF>(-1, (int)v));
    v = min(v, (uint32_t)dpp_mov<kDppRowBcast15, 0xA>(-1, (int)v));
    v = min(v, (uint32_t)dpp_mov<kDppRowBcast31, 0xC>(-1, (int)v));
    return (uint32_t)lane_read((int)v, 63);
}

// ---- scans on __shfl_up (ds_bpermute: one LDS round trip per step; kept where the kernels were measured with them) -------
// inclusive prefix sum over the 64 lanes (int or long long); lane 63 holds the wave's total.  Not wave_sum: that one is a
// total on DPP, this one a scan.  (Two sites keep the loop written out -- k_lead_compress's look-back, k_small_batch: hipcc
// schedules those kernels differently around the call, and this header came in without changing a kernel.)
template <typename T>
__device__ __forceinline__ T shfl_scan_add(T inc, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    return inc;
}

// Bw = the string-start bits of my word (lane = word of a 4096-char tile).  Returns the tile-relative position of the last
// string start in the words BEFORE mine (prefix max over the lanes, shifted by one lane), -1 if there is none.
__device__ __forceinline__ int last_start_before(uint64_t Bw, int lane) {
    int carry = Bw ? 64 * lane + 63 - __builtin_clzll(Bw) : -1;     // tile-relative position of my word's last string start
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(carry, d);
        if (lane >= d && o > carry) carry = o;
    }
    carry = __shfl_up(carry, 1);
    if (lane == 0) carry = -1;
    return carry;
}

// Which boundaries (x) of a word start a token with a non-SPACE char (nn), for all boundaries of the word at once: on the
// bit-reversed word a boundary is the TOP of its token, so "some non-SPACE below me in my token" is a carry chain -- one add.
//   generate = non-SPACE chars that are not boundaries, propagate = non-boundaries, carry-in (cin) = the token that
//   continues into the next word(s) has a non-SPACE char there
__device__ __forceinline__ uint64_t kept_boundaries(uint64_t x, uint64_t nn, bool cin) {
    const uint64_t xr = __builtin_bitreverse64(x), nr = __builtin_bitreverse64(nn);
    const uint64_t g = nr & ~xr, pr = ~xr;
    const uint64_t a = pr | g;
    const uint64_t carries = (a + g + (cin ? 1ull : 0ull)) ^ a ^ g;      // carry INTO every position
    return __builtin_bitreverse64(xr & (nr | carries));
}

// lower_bound over the row offsets: smallest s in [0, n_entries] with row_off[s] >= c (n_entries if none).  64-ary
// search by one wave: every lane probes one pivot, the ballot picks the sub-range
// (the resolve stage's rare recomputations; the scatter kernels when no tile index was published).
__device__ __forceinline__ int64_t wave_lower_bound(const int64_t* __restrict__ row_off, int64_t n_entries, int64_t c,
                                                    int lane) {
    int64_t lo = 0, hi = n_entries;
    while (hi > lo) {
        const int64_t len = hi - lo;
        const int64_t step = (len + 63) / 64;
        const int64_t p = lo + (int64_t)lane * step;
        const bool pred = p < hi && row_off[p] >= c;
        const uint64_t m = __ballot(pred);
        if (!m) {
            const int64_t n_valid = (len + step - 1) / step;
            lo = min(lo + (n_valid - 1) * step + 1, hi);
        } else {
            const int f = __builtin_ctzll(m);
            hi = lo + (int64_t)f * step;
            if (f > 0) lo = lo + (int64_t)(f - 1) * step + 1;
        }
    }
    return lo;
}

}  // namespace latok
#endif
