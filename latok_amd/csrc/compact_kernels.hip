// compact_kernels.hip -- everything tokenize() / featurize() do AFTER the split mask, on the device and parallel over
// the packed buffer (not over strings, so one 1 M-char document is as parallel as 8 000 tweets):
//
//   boundary offsets   np.nonzero(splits)[0] per string                      reference default_tokenizer.py:148
//   token spans        slice between consecutive boundaries, strip, drop ''   reference default_tokenizer.py:149-158
//   token features     per-token sums of the 25 matrix columns (featurize)    reference default_tokenizer.py:163-191
//   joined token text  the tokens themselves, sep.join per string, UTF-8 out  reference default_tokenizer.py:149-160   (below: "joined token text")
//   token hashes       MurmurHash3 x86_32 of every token's UTF-8 bytes        reference default_tokenizer.py:149-160   (HashTokens, k_hash_scatter)
//
// Inputs are the two bitmasks the tile kernel writes (boundary bits, SPACE bits; bit i = packed char i) and row_off.
// Because strings are contiguous and ordered in the packed buffer, "all offsets of string 0, then string 1, ..." is
// simply position order, so the output index of an item is the global rank of its bit.  Three launches:
//   k_word_counts        one wave per 4096-char tile: items per word (uint16 prefix inside the tile), items per tile
//   k_scan_chained       exclusive scan of the tile counts over the whole batch in one launch (single-pass chained scan
//                        with look-back over workgroup totals): every tile's rank and, for the host, the item total
//   k_counts_scatter     workgroups split into two roles: one thread per string: count = rank(end) - rank(start), O(1);
//                        one wave per tile: scatter its items at tile rank + position inside the tile
// A token is kept iff it contains a non-SPACE char; its extent needs the next boundary bit, which normally sits in the
// same or the next word (a lane follows the mask forward only for its own items).  Counts and records are written as
// int64 or, on request (LATOK_OUT_INT32), as int32: the records are most of the traffic of these paths.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "bitscan.h"
#include "block_ops.h"
#include "count_table.h"
#include "kernels.h"
#include "lane_math.h"
#include "term_key.h"
#include "token_hash.h"
#include "vocab_table.h"

namespace latok {

// ---- pass 1 --------------------------------------------------------------------------------------------------------
// SPANS = false: items = boundary bits.  SPANS = true: items = boundaries whose token is kept; the kept-mask word is
// stored for the later passes.  A token is kept iff it holds a non-SPACE char; for all but the last boundary of a
// word that is a mask test inside the word, the last one looks ahead until the next boundary (normally the next word).
// One wave per 4096-char tile, lane = word: the tile's item count and every word's exclusive prefix inside its tile
// (uint16); rank(word) = tile_rank[tile] + word_pref[word], tile_rank = exclusive scan of the tile counts (k_scan_chained).
template <bool SPANS>
__device__ __forceinline__ void word_counts_tile(const uint64_t* __restrict__ bits, const uint64_t* __restrict__ space,
                                                 int64_t n_words, int64_t total, uint64_t* __restrict__ kept_out,
                                                 int64_t* __restrict__ tile_cnt, uint16_t* __restrict__ word_pref, int64_t t, int lane) {
    const int64_t w = t * 64 + lane;
    if (t * 64 >= n_words) return;   // whole wave
    int cnt = 0;
    const uint64_t x = w < n_words ? bits[w] : 0ull;
    if (!SPANS) {
        cnt = __popcll(x);
    } else {
        const uint64_t nn = w < n_words ? (~space[w] & valid_mask(w, total)) : 0ull;   // non-SPACE chars of the word
        // the next word's masks from the neighbour lane (lane 63: from memory): the word's last token normally ends there
        uint64_t x1 = __shfl_down(x, 1), nn1 = __shfl_down(nn, 1);
        if (lane == 63) {
            const bool has = w + 1 < n_words;
            x1 = has ? bits[w + 1] : 0ull;
            nn1 = has ? (~space[w + 1] & valid_mask(w + 1, total)) : 0ull;
        }
        // which boundaries start a token with a non-SPACE char (kept_boundaries, wave_ops.h); carry-in = the token that
        // continues into the next word(s) has a non-SPACE char there
        bool cin;
        if (x1) cin = (nn1 & ((x1 & (~x1 + 1ull)) - 1ull)) != 0;
        else cin = nn1 != 0 || (x != 0 && w + 1 < n_words && tail_has_nonspace(bits, space, w + 1, n_words, total));
        const uint64_t kept = kept_boundaries(x, nn, cin);
        if (w < n_words) kept_out[w] = kept;
        cnt = __popcll(kept);
    }
    const int inc = shfl_scan_add(cnt, lane);
    if (w < n_words) word_pref[w] = (uint16_t)(inc - cnt);
    if (lane == 63) tile_cnt[t] = inc;
}

template <bool SPANS>
__global__ __launch_bounds__(256) void k_word_counts(const uint64_t* __restrict__ bits, const uint64_t* __restrict__ space,
                                                     int64_t n_words, int64_t total, uint64_t* __restrict__ kept_out,
                                                     int64_t* __restrict__ tile_cnt, uint16_t* __restrict__ word_pref,
                                                     const int64_t* __restrict__ total_dev) {
    // total_dev (or NULL): the batch's size is a word in device memory that an earlier launch of the stream wrote; the grid was
    // sized for an upper bound (n_words), and tiles behind the real size do nothing (DeviceTotal, kernels.h)
    if (total_dev) {
        total = device_total(total_dev, total);
        n_words = (total + 63) >> 6;
    }
    word_counts_tile<SPANS>(bits, space, n_words, total, kept_out, tile_cnt, word_pref,
                            ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, threadIdx.x & 63);
}

// Exclusive scan of the tile counts over the whole batch in ONE launch (it used to be three: local scans, scan of the
// block totals, fix-up): single-pass chained scan.  A workgroup takes a ticket -- its position in the scan order is the
// order in which workgroups START, so a workgroup only ever waits for workgroups that are already running --, scans its
// chunk of 4096 counts, publishes the chunk total, and looks back over its predecessors' published words, 64 at a time
// (one per lane), summing totals until it meets a predecessor that already knows its inclusive prefix.  The words carry
// the launch's epoch, so nothing has to be cleared between launches (api.cpp: next_scan_epoch).
constexpr int kChainBlock = 1024, kChainItems = 4, kChainChunk = kChainBlock * kChainItems;
constexpr int kChainValueBits = 44, kChainFlagShift = 44, kChainEpochShift = 46;
constexpr unsigned long long kChainValueMask = (1ull << kChainValueBits) - 1ull;
constexpr unsigned kChainAggregate = 1u, kChainPrefix = 2u;

__device__ __forceinline__ void chain_publish(unsigned long long* slot, unsigned epoch, unsigned flag, long long value) {
    const unsigned long long w = ((unsigned long long)epoch << kChainEpochShift) | ((unsigned long long)flag << kChainFlagShift) |
                                 ((unsigned long long)value & kChainValueMask);
    // relaxed, agent scope: the word IS the message (value + flag + epoch in one 64-bit store), nothing else has to be
    // visible with it -- a release here writes back the whole L2 of the XCD for every workgroup (measured: 10x slower)
    __hip_atomic_store(slot, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kChainBlock) void k_scan_chained(const int64_t* __restrict__ in, int64_t n, int64_t* __restrict__ out,
                                                              unsigned long long* __restrict__ chain, unsigned* __restrict__ ticket,
                                                              unsigned epoch, unsigned n_blocks, int64_t* __restrict__ total_out,
                                                              int64_t* __restrict__ total_host, int* __restrict__ err,
                                                              const int64_t* __restrict__ units_dev) {
    // units_dev (or NULL): the number of counts is not known to the host -- it is ceil(*units_dev / kTile), at most the `n` the
    // grid was sized for.  The chain terminates for every such size, 0 and exact multiples of kChainChunk included, because
    // the size only decides what a workgroup READS, never whether it takes part: all n_blocks launched workgroups take a
    // ticket, publish their aggregate BEFORE they wait for anything (a workgroup whose chunk lies behind the real size
    // publishes 0), and look back only at smaller tickets, whose holders are therefore running or done.  No workgroup leaves
    // without publishing and none waits for one that was not launched; the holder of ticket n_blocks - 1 -- n_blocks is the
    // launched grid, not a function of the size -- writes the total (0 for an empty batch) and re-arms the ticket counter.
    if (units_dev) n = min(n, (device_total(units_dev, n * kTile) + kTile - 1) / kTile);
    __shared__ unsigned s_ticket;
    __shared__ long long s_wave_tot[kChainBlock / 64];
    __shared__ long long s_prefix;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_ticket = atomicAdd(ticket, 1u);
    __syncthreads();
    const unsigned b = s_ticket;
    const int64_t base = (int64_t)b * kChainChunk + (int64_t)threadIdx.x * kChainItems;
    long long v[kChainItems], sum = 0;
#pragma unroll
    for (int j = 0; j < kChainItems; ++j) {
        v[j] = base + j < n ? in[base + j] : 0;
        sum += v[j];
    }
    const long long inc = shfl_scan_add(sum, lane);   // (block_scan_add of block_ops.h written out: no barrier in front of the first use)
    if (lane == 63) s_wave_tot[wave] = inc;
    __syncthreads();
    long long wave_excl = 0, agg = 0;
#pragma unroll
    for (int k = 0; k < kChainBlock / 64; ++k) {
        const long long x = s_wave_tot[k];
        if (k < wave) wave_excl += x;
        agg += x;
    }
    if (wave == 0) {
        if (lane == 0) chain_publish(&chain[b], epoch, b == 0 ? kChainPrefix : kChainAggregate, agg);
        long long prefix = 0;
        for (long long j0 = (long long)b - 1; j0 >= 0; j0 -= 64) {   // wave-uniform
            const long long j = j0 - lane;
            unsigned long long sv = 0;
            if (j >= 0) {
                // (bounded: every predecessor holds a ticket, i.e. is running, and publishes before it waits for anything,
                // so this never spins for long; should the state ever be corrupt, the launch ends with an error flag
                // instead of hanging the device)
                int spins = 0;
                do {
                    sv = __hip_atomic_load(&chain[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                } while (((unsigned)(sv >> kChainEpochShift) != epoch || ((sv >> kChainFlagShift) & 3ull) == 0ull) && ++spins < (1 << 22));
                if (spins >= (1 << 22)) {
                    *err = 2;
                    sv = ((unsigned long long)epoch << kChainEpochShift) | ((unsigned long long)kChainPrefix << kChainFlagShift);
                }
            }
            const bool is_prefix = j < 0 || ((sv >> kChainFlagShift) & 3ull) == kChainPrefix;   // before workgroup 0: prefix 0
            const long long val = j >= 0 ? (long long)(sv & kChainValueMask) : 0;
            const unsigned long long pm = __ballot(is_prefix);
            const int first = pm ? __builtin_ctzll(pm) : 64;      // the nearest predecessor that knows its inclusive prefix
            long long part = lane <= first ? val : 0;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor(part, d);
            prefix += part;
            if (pm) break;
        }
        if (lane == 0) {
            s_prefix = prefix;
            if (b > 0) chain_publish(&chain[b], epoch, kChainPrefix, prefix + agg);
            if (b == n_blocks - 1) {          // the last ticket: every workgroup has taken its own by now
                *total_out = prefix + agg;
                if (total_host) *total_host = prefix + agg;   // pinned, device-mapped: read by the host after the stream drains
                *ticket = 0u;
            }
        }
    }
    __syncthreads();
    long long run = s_prefix + wave_excl + inc - sum;
#pragma unroll
    for (int j = 0; j < kChainItems; ++j) {
        if (base + j < n) out[base + j] = run;
        run += v[j];
    }
}

// ---- pass 2: items per string = rank(row_off[s+1]) - rank(row_off[s]) ------------------------------------------------
__device__ __forceinline__ int64_t rank_at(const uint64_t* __restrict__ mask, const int64_t* __restrict__ tile_rank,
                                           const uint16_t* __restrict__ word_pref, int64_t x, int64_t total, int64_t n_items) {
    if (x >= total) return n_items;
    const int64_t w = x >> 6;
    return tile_rank[w >> 6] + word_pref[w] + __popcll(mask[w] & low_mask((int)(x & 63)));
}
// OUT = int64_t or int32_t.  A string of 2^31 chars or more cannot be reported in int32: *err is raised (the host turns
// it into LATOK_ERR_INVALID).
template <typename OUT>
__device__ __forceinline__ void string_counts_role(int64_t s, const uint64_t* __restrict__ mask, const int64_t* __restrict__ tile_rank,
                                                   const uint16_t* __restrict__ word_pref, const int64_t* __restrict__ row_off,
                                                   int64_t n_str, int64_t total, int64_t n, OUT* __restrict__ counts,
                                                   int* __restrict__ err) {
    if (s >= n_str) return;
    const int64_t r0 = row_off[s], r1 = row_off[s + 1];
    if (sizeof(OUT) == 4 && r1 - r0 > 0x7FFFFFFFll) *err = 1;   // (plain store: the flag may live in pinned host memory)
    counts[s] = (OUT)(rank_at(mask, tile_rank, word_pref, r1, total, n) - rank_at(mask, tile_rank, word_pref, r0, total, n));
}
template <typename OUT>
__global__ __launch_bounds__(256) void k_string_counts(const uint64_t* __restrict__ mask, const int64_t* __restrict__ tile_rank,
                                                       const uint16_t* __restrict__ word_pref, const int64_t* __restrict__ row_off,
                                                       int64_t n_str, int64_t total, const int64_t* __restrict__ n_items,
                                                       OUT* __restrict__ counts, int* __restrict__ err,
                                                       const int64_t* __restrict__ total_dev) {
    if (total_dev) total = device_total(total_dev, total);
    string_counts_role<OUT>((int64_t)blockIdx.x * blockDim.x + threadIdx.x, mask, tile_rank, word_pref, row_off, n_str, total, *n_items,
                            counts, err);
}

// ---- pass 3 --------------------------------------------------------------------------------------------------------
// One wave per 64 consecutive words (4096 chars).  The wave
//   (a) finds where the owning string of every position begins: the string starts inside the tile become bits in LDS,
//       the last start before each word is a prefix max over the lanes, and the string that was open when the tile began
//       comes from the per-tile string index the tile kernel publishes (tile_string_starts);
//   (b) lane = word: walks the items of its word (all mask arithmetic inside the word; only a token that runs past the
//       word's end follows the masks further) and puts the records into an LDS window at their rank inside the wave;
//   (c) streams the window to the output: consecutive lanes write consecutive 8-byte words.
// Offsets (offsets[k] = p - start of its string) take (b) and (c) word-major (offsets_walk).  Every other form takes them
// token-major (token_walk) and hands each token to its consumer, below: SpanRecords, HashTokens, IdTokens, CountTokens, TermTokens.
constexpr int kScatterWaves = 4;      // waves per workgroup of every scatter kernel; both block roles use its 256 threads
constexpr int kScatterCodes = 1024;   // items per round
constexpr int kScatterRowsEnd = kScatterCodes * 2 + 64 * 48;   // token-major LDS: the item codes (2 B each), then the 48-byte mask rows of the 64 words
struct HashArgs {
    const uint32_t* text = nullptr;   // the batch's bytes as aligned dwords (the buffer is 16-byte aligned)
    uint32_t* hashes = nullptr;
    uint32_t seed = 0;
};
struct VocabArgs {                    // (the text and the seed travel in HashArgs)
    const VtSlot* slots = nullptr;
    const uint32_t* blob = nullptr;
    uint64_t n_slots = 0;             // a power of two
    int32_t* ids = nullptr;
    int32_t unk = 0;
};
struct CountArgs {                    // (the text and the seed travel in HashArgs)
    uint64_t* slots = nullptr;        // one 8-byte word per slot (count_table.h), 0 = empty
    unsigned long long* counts = nullptr;
    const uint32_t* blob = nullptr;   // the resident words, stored by earlier launches
    uint64_t n_slots = 0;             // a power of two, <= 2^31
    unsigned long long* tally = nullptr;   // this call's {counted, long, dropped}
    int max_word_bytes = 0;           // 1 .. kHashWaveBytes
};
struct TermArgs {                     // (the text and the seed travel in HashArgs, the table in VocabArgs)
    uint64_t* keys = nullptr;         // one term_key.h key per token, at its rank
    uint32_t n_features = 0;          // 0: the vocabulary form
    bool alternate_sign = false;
};
struct CtDeviceAtomics {              // count_table.h's policy: relaxed, agent scope -- the slot word is the whole message
    static __device__ __forceinline__ uint64_t load(const uint64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __device__ __forceinline__ uint64_t cas(uint64_t* p, uint64_t expect, uint64_t v) {
        __hip_atomic_compare_exchange_strong(p, &expect, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return expect;
    }
};

// ---- the consumers of the token-major walk ---------------------------------------------------------------------------
// A consumer says what is done with the stripped token [a2, e2) of rank `rank`: short_token in the lane that holds it (p, e: the raw
// extent; lo: the start of its string), long_token -- kWaveTokens: a token of more than kHashWaveBytes bytes, taken by the whole wave
// behind the round with its hash h already formed; `mine`: this lane held it -- and flush once the tile is done.  begin gets the
// kLdsBytes of LDS a consumer asked for.  The consumers that hash read `text` and `seed` from their HashArgs.
template <class T>
struct ArrayOf {   // the loaders of token_hash.h / vocab_table.h / count_table.h over the text, a blob or the slots: ordinary cached loads
    const T* p;
    template <class I>
    __device__ __forceinline__ T operator()(I i) const { return p[i]; }
};
using DwordsOf = ArrayOf<uint32_t>;
// A long token's hash is wave-uniform, so the wave probes in step: every lane asks for the same slot -- one request -- ...
struct WaveSlotsOf {
    const VtSlot* p;
    __device__ __forceinline__ VtSlot operator()(uint64_t i) const {
        const VtSlot v = p[i];
        return VtSlot{(uint32_t)__builtin_amdgcn_readfirstlane((int)v.hash), __builtin_amdgcn_readfirstlane(v.id),
                      (uint32_t)__builtin_amdgcn_readfirstlane((int)v.off), (uint32_t)__builtin_amdgcn_readfirstlane((int)v.len)};
    }
};
// ... and compares a candidate 64 dwords per step with coalesced loads; a ballot decides.
struct WaveEqual {
    DwordsOf text;
    int64_t a, e;
    DwordsOf blob;
    int lane;
    __device__ __forceinline__ bool operator()(uint32_t off) const {
        const int64_t rounds_c = vt_wave_rounds(a, e);
        for (int64_t r = 0; r < rounds_c; ++r)
            if (__ballot(vt_wave_differs(text, a, e, blob, off, r, lane))) return false;
        return true;
    }
};
struct TokenConsumer {   // what a consumer leaves out
    static constexpr bool kWordMajor = false, kWaveTokens = false;
    static constexpr int kLdsBytes = 0;
    __device__ __forceinline__ void begin(uint8_t*, int) {}
    __device__ __forceinline__ void flush(int) {}
};
// the stripped extent of a token, string relative, as one record of two fields at its rank
template <typename OUT>
__device__ __forceinline__ void store_span(OUT* out, int64_t rank, int64_t a2, int64_t e2, int64_t lo) {
    typedef OUT out2 __attribute__((ext_vector_type(2)));
    out2 v;
    v.x = (OUT)(a2 - lo);
    v.y = (OUT)(e2 - lo);
    __builtin_nontemporal_store(v, reinterpret_cast<out2*>(out) + rank);
}
// Span records (k_counts_scatter).  FIELDS = 2 (kind 1): spans[2k..] = stripped extent.  FIELDS = 4 (kind 2): spans4[4k..] = {raw start,
// raw end, stripped start, stripped end}: featurize's span record, for UTF-8 in BYTE space -- the sums of the same tokens are formed in
// code-point space by k_features_tiles, which then writes no records (a token has the same rank in both spaces).  The other forms of
// featurize get their records from k_features_tiles, together with the sums.
template <typename OUT, int FIELDS>
struct SpanRecords : TokenConsumer {
    OUT* out;
    __device__ __forceinline__ void short_token(int64_t rank, int64_t p, int64_t e, int64_t a2, int64_t e2, int64_t lo) {
        if (FIELDS == 2) {
            store_span(out, rank, a2, e2, lo);
        } else if (sizeof(OUT) == 4) {                    // the record is 16 or 32 bytes: aligned 16-byte stores
            typedef OUT out4 __attribute__((ext_vector_type(4)));
            out4 r;
            r.x = (OUT)(p - lo);
            r.y = (OUT)(e - lo);
            r.z = (OUT)(a2 - lo);
            r.w = (OUT)(e2 - lo);
            __builtin_nontemporal_store(r, reinterpret_cast<out4*>(out) + rank);
        } else {
            store_span(out, 2 * rank, p, e, lo);
            store_span(out, 2 * rank + 1, a2, e2, lo);
        }
    }
};
// Token hashes (k_hash_scatter): SpanRecords<OUT, 2>'s records (out may be NULL: none) and hashes[k] = MurmurHash3 x86_32 of the stripped
// token's bytes (token_hash.h).  In the token-major loop lane j holds token j's byte range: it walks its own token -- neighbouring lanes
// hold neighbouring tokens, their aligned dword loads share cache lines --, unless the token is longer than kHashWaveBytes: those
// the wave takes one at a time behind the round, 256 bytes per step with coalesced loads, every lane mixing its own block and
// the h chain folded in lane order, so a long token costs its length once, with the whole wave at work.
template <typename OUT>
struct HashTokens : TokenConsumer {
    static constexpr bool kWaveTokens = true;
    HashArgs h;
    OUT* out;
    __device__ __forceinline__ void short_token(int64_t rank, int64_t, int64_t, int64_t a2, int64_t e2, int64_t lo) {
        if (out) store_span(out, rank, a2, e2, lo);
        if (e2 - a2 <= kHashWaveBytes) __builtin_nontemporal_store(th_hash_lane(DwordsOf{h.text}, a2, e2, h.seed), h.hashes + rank);
    }
    __device__ __forceinline__ void long_token(int64_t rank, int64_t, int64_t, uint32_t hash, int, bool mine) {
        if (mine) __builtin_nontemporal_store(hash, h.hashes + rank);
    }
};
// Token ids (k_vocab_scatter): HashTokens with the hash kept in its lane instead of stored: the lane that hashed a short token probes the
// vocabulary table with it (vocab_table.h: one 16-byte slot per step, at most n_slots steps), compares the bytes where hash and
// length agree and stores ids[k] = the word's id or unk.  A long token is probed and compared by the wave in step (WaveSlotsOf,
// WaveEqual).  The table and the blob are read with ordinary cached loads (they are what is worth keeping in L2); no hash goes
// through memory.
template <typename OUT>
struct IdTokens : TokenConsumer {
    static constexpr bool kWaveTokens = true;
    HashArgs h;
    VocabArgs v;
    OUT* out;
    __device__ __forceinline__ void short_token(int64_t rank, int64_t, int64_t, int64_t a2, int64_t e2, int64_t lo) {
        if (out) store_span(out, rank, a2, e2, lo);
        if (e2 - a2 > kHashWaveBytes) return;
        const DwordsOf text{h.text};
        const int32_t id = vt_lookup_lane(text, a2, e2, th_hash_lane(text, a2, e2, h.seed), ArrayOf<VtSlot>{v.slots}, DwordsOf{v.blob}, v.n_slots, v.unk);
        __builtin_nontemporal_store(id, v.ids + rank);
    }
    __device__ __forceinline__ void long_token(int64_t rank, int64_t a, int64_t e, uint32_t hash, int lane, bool mine) {
        const uint32_t hu = (uint32_t)__builtin_amdgcn_readfirstlane((int)hash);
        const int32_t id = vt_probe(WaveSlotsOf{v.slots}, v.n_slots, hu, (uint32_t)(e - a), WaveEqual{{h.text}, a, e, {v.blob}, lane}, v.unk);
        if (mine) __builtin_nontemporal_store(id, v.ids + rank);
    }
};
// Token counts (k_count_scatter): IdTokens' lane path with a counting table in the vocabulary's place (count_table.h): the lane finds its
// token's slot or claims an empty one with one CAS -- nothing waits for another thread --, and the hit is counted in a per-wave
// accumulator in LDS, a direct-mapped {slot + 1, count} array of kCountAccEntries entries: the tag is claimed with an LDS CAS, a
// hit is an LDS add, a conflicting entry adds to the global count directly.  Behind the tile's last round the wave flushes its
// entries with no-return atomic adds, so a hot word costs one global atomic per tile, not one per token.  It writes no records.
// A token of more than max_word_bytes bytes is tallied as long and never entered: there is no whole-wave form.  The three
// tallies (counted, long, dropped) are reduced over the wave: one atomic each per tile.
struct CountTokens : TokenConsumer {
    static constexpr int kLdsBytes = 8 * kCountAccEntries;
    HashArgs h;
    CountArgs c;
    uint32_t* acc = nullptr;   // the wave's accumulator: tags (slot + 1, 0 = free) in the first half, counts in the second
    unsigned n_counted = 0, n_long = 0, n_dropped = 0;   // my tallies
    __device__ __forceinline__ void begin(uint8_t* lds, int lane) {
        acc = reinterpret_cast<uint32_t*>(lds);
        for (int i = lane; i < 2 * kCountAccEntries; i += 64) acc[i] = 0u;   // (visible behind the round's first wave barrier)
    }
    __device__ __forceinline__ void short_token(int64_t, int64_t, int64_t, int64_t a2, int64_t e2, int64_t) {
        if (e2 - a2 > c.max_word_bytes) {
            ++n_long;
            return;
        }
        const DwordsOf text{h.text};
        const int64_t s = ct_find_or_insert<CtDeviceAtomics>(text, a2, e2, th_hash_lane(text, a2, e2, h.seed), c.slots, DwordsOf{c.blob}, c.n_slots,
                                                             (uint32_t)kCountProbeMax);
        if (s == kCtDropped) {
            ++n_dropped;
            return;
        }
        ++n_counted;
        const uint32_t tag = (uint32_t)s + 1u, at = (uint32_t)s & (uint32_t)(kCountAccEntries - 1);
        const uint32_t was = atomicCAS(&acc[at], 0u, tag);
        if (was == 0u || was == tag) atomicAdd(&acc[kCountAccEntries + at], 1u);
        else (void)__hip_atomic_fetch_add(c.counts + s, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ void flush(int lane) {   // the tile is done: the accumulator (no-return adds) and the three tallies
        for (int i = lane; i < kCountAccEntries; i += 64) {
            const uint32_t tag = acc[i];
            if (tag) (void)__hip_atomic_fetch_add(c.counts + (tag - 1u), (unsigned long long)acc[kCountAccEntries + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            n_counted += __shfl_xor(n_counted, d);
            n_long += __shfl_xor(n_long, d);
            n_dropped += __shfl_xor(n_dropped, d);
        }
        if (lane == 0) {
            if (n_counted) (void)__hip_atomic_fetch_add(c.tally + 0, (unsigned long long)n_counted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (n_long) (void)__hip_atomic_fetch_add(c.tally + 1, (unsigned long long)n_long, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (n_dropped) (void)__hip_atomic_fetch_add(c.tally + 2, (unsigned long long)n_dropped, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
};
// Term keys (k_term_scatter): IdTokens' two paths with a term key (term_key.h) stored at the token's rank in the workspace instead of an
// id in caller memory: the id with a found bit of its own, or -- with no table, n_features > 0 -- the hash bucket and the sign.
// terms_kernels.hip sorts and reduces the keys inside every string.  It writes no records.
struct TermTokens : TokenConsumer {
    static constexpr bool kWaveTokens = true;
    HashArgs h;
    VocabArgs v;
    TermArgs t;
    __device__ __forceinline__ void short_token(int64_t rank, int64_t, int64_t, int64_t a2, int64_t e2, int64_t) {
        if (e2 - a2 > kHashWaveBytes) return;
        const DwordsOf text{h.text}, blob{v.blob};
        const uint32_t hash = th_hash_lane(text, a2, e2, h.seed);
        t.keys[rank] = t.n_features ? tk_hashed_key(hash, t.n_features, t.alternate_sign)
                                    : tk_vocab_probe(ArrayOf<VtSlot>{v.slots}, v.n_slots, hash, (uint32_t)(e2 - a2),
                                                     [text, a2, e2, blob](uint32_t off) { return vt_equal_lane(text, a2, e2, blob, off); });
    }
    __device__ __forceinline__ void long_token(int64_t rank, int64_t a, int64_t e, uint32_t hash, int lane, bool mine) {
        const uint32_t hu = (uint32_t)__builtin_amdgcn_readfirstlane((int)hash);
        const uint64_t key = t.n_features ? tk_hashed_key(hu, t.n_features, t.alternate_sign)
                                          : tk_vocab_probe(WaveSlotsOf{v.slots}, v.n_slots, hu, (uint32_t)(e - a), WaveEqual{{h.text}, a, e, {v.blob}, lane});
        if (mine) t.keys[rank] = key;
    }
};
// Offsets (k_counts_scatter, kind 0): no tokens, the word-major walk.
template <typename OUT>
struct Offsets : TokenConsumer {
    static constexpr bool kWordMajor = true;
    OUT* out;
};

// (a) where the string that owns a position begins: string-start bits of the tile in LDS (one atomicOr per string
//     that starts in it), per lane the last start before its word (prefix max), and for everything before the first
//     start the string that was open when the tile began.  No per-item loads: a lane that had to fetch row_off at
//     every string change stalled the whole wave on every step of its item loop.
// bw: 64 words of the wave's LDS.  *Bw = the string starts of my word, *lo_in = the start of the string open at its bit 0.
__device__ __forceinline__ void tile_string_starts(const TokenPlanes& p, int64_t w0, int lane, unsigned long long* bw, uint64_t* Bw, int64_t* lo_in) {
    const int64_t t0 = w0 << 6;
    // first string starting at or after t0: published by the tile kernel (one wave = one tile), else searched
    int64_t idx0 = p.tile_first ? p.tile_first[w0 >> 6] : wave_lower_bound(p.row_off, p.n_str, t0, lane);
    idx0 = idx0 < 0 ? 0 : idx0;
    if (idx0 > p.n_str) idx0 = p.n_str;
    const int64_t start_before = idx0 > 0 ? p.row_off[idx0 - 1] : 0;
    bw[lane] = 0ull;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int64_t i0 = idx0; i0 < p.n_str; i0 += 64) {
        const int64_t sidx = i0 + lane;
        const int64_t ro = sidx < p.n_str ? p.row_off[sidx] : INT64_MAX;
        const int64_t rel = ro - t0;
        if (rel >= 0 && rel < 4096) atomicOr(&bw[rel >> 6], 1ull << (rel & 63));
        if (__shfl(ro, 63) >= t0 + 4096) break;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    *Bw = bw[lane];
    const int carry = last_start_before(*Bw, lane);
    *lo_in = carry >= 0 ? t0 + carry : start_before;
}

// (b) + (c) of the offsets, window by window: offsets are one subtraction per item, and here the word-major loop through an LDS
// window (win: kScatterCodes values) is the faster form.  rest = the items of my word w, k = the wave rank of its first, n_wave = the
// tile's items, base_out = the tile's rank in out.
// Every string start is itself a boundary (splits[0] = 1), so the walk over a word's items meets the string starts
// in passing: `cur` = offset of the word's bit 0 relative to the string the walk is in -- base - lo_in on entry,
// -b once the item at bit b is a string start.  32-bit halves: no 64-bit shifts, masks or clz in the loop (the
// former form -- mask the string starts below the item, clz -- was 3x the instructions).
template <typename OUT>
__device__ __forceinline__ void offsets_walk(uint64_t rest, int k, int n_wave, int64_t w, uint64_t Bw, int64_t lo_in, OUT* win, OUT* out, int64_t base_out, int lane) {
    constexpr int kCodes = kScatterCodes;
    const int64_t base = w << 6;
    uint32_t r0 = (uint32_t)rest, r1 = (uint32_t)(rest >> 32);
    const uint32_t B0 = (uint32_t)Bw, B1 = (uint32_t)(Bw >> 32);
    OUT cur = (OUT)(base - lo_in);
    for (int win0 = 0; win0 < n_wave; win0 += kCodes) {
        const int lim = win0 + kCodes;
        while (r0 && k < lim) {
            const int b = __builtin_ctz(r0);
            r0 &= r0 - 1u;
            if ((B0 >> b) & 1u) cur = (OUT)(-b);
            win[k - win0] = (OUT)(cur + b);
            ++k;
        }
        while (!r0 && r1 && k < lim) {
            const int b = __builtin_ctz(r1);
            r1 &= r1 - 1u;
            if ((B1 >> b) & 1u) cur = (OUT)(-(32 + b));
            win[k - win0] = (OUT)(cur + 32 + b);
            ++k;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // stream the window out: single elements up to the first 16-byte boundary of the output, then 16-byte stores
        const int n_val = min(kCodes, n_wave - win0);
        OUT* dst = out + base_out + win0;
        constexpr int kPer = 16 / (int)sizeof(OUT);                   // elements per 16-byte store
        const int head = min(n_val, (int)(((16u - ((uintptr_t)dst & 15u)) & 15u) / sizeof(OUT)));
        if (lane < head) __builtin_nontemporal_store(win[lane], dst + lane);
        const int n_vec = (n_val - head) / kPer;
        typedef OUT vec_t __attribute__((ext_vector_type(16 / sizeof(OUT))));
        for (int i = lane; i < n_vec; i += 64) {
            vec_t v;
#pragma unroll
            for (int e = 0; e < kPer; ++e) v[e] = win[head + kPer * i + e];
            __builtin_nontemporal_store(v, reinterpret_cast<vec_t*>(dst + head) + i);
        }
        const int tail0 = head + kPer * n_vec;
        if (lane < n_val - tail0) __builtin_nontemporal_store(win[tail0 + lane], dst + tail0 + lane);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
}

// (b) + (c) of every other form.  (b) token spans: every lane lists its items as (lane, bit) codes at their rank inside the wave ...
// (c) ... and the wave then takes the items in rank order, lane j the j-th: the owner word's masks arrive through
//     LDS rows, so all 64 lanes are busy whatever the spread of items over the words is (a word-major loop runs as
//     long as the fullest word, typically 2x the mean), and the records go straight to consecutive addresses.
// buf: the wave's LDS (codes, rows, the consumer's bytes).  rest = the items of my word w0 + lane, k = the wave rank of its first,
// n_wave = the tile's items, base_out = the tile's rank; Bw / lo_in from tile_string_starts.
template <class C>
__device__ __forceinline__ void token_walk(const TokenPlanes& p, C& c, uint8_t* buf, uint64_t rest, int k, int n_wave, int64_t w0, int64_t base_out,
                                           uint64_t Bw, int64_t lo_in, int lane) {
    constexpr int kCodes = kScatterCodes;
    const int64_t w = w0 + lane, n_words = p.n_words, total = p.total;
    const uint64_t xb = w < n_words ? p.bits[w] : 0ull;              // all boundaries of the word (item_mask is a subset)
    const uint64_t nn = w < n_words ? (~p.space[w] & valid_mask(w, total)) : 0ull;
    // the next word's masks (a token that crosses the word's end normally ends there): from the neighbour lane
    uint64_t xb1 = __shfl_down(xb, 1), nn1 = __shfl_down(nn, 1);
    if (lane == 63) {
        const bool has = w + 1 < n_words;
        xb1 = has ? p.bits[w + 1] : 0ull;
        nn1 = has ? (~p.space[w + 1] & valid_mask(w + 1, total)) : 0ull;
    }
    // the lanes' masks as 48-byte rows in LDS (behind the codes): in the token-major loop lane j reads the row of the
    // word that owns its item with three 16-byte reads (six 64-bit shuffles = twelve ds_bpermute before)
    uint16_t* codes = reinterpret_cast<uint16_t*>(buf);
    uint64_t* rows = reinterpret_cast<uint64_t*>(buf + kCodes * 2);            // codes take kCodes * 2 bytes
    {
        uint64_t* r = rows + 6 * lane;
        r[0] = xb; r[1] = nn; r[2] = xb1; r[3] = nn1; r[4] = Bw; r[5] = (uint64_t)lo_in;
    }
    c.begin(buf + kScatterRowsEnd, lane);
    for (int win0 = 0; win0 < n_wave; win0 += kCodes) {
        while (rest && k < win0 + kCodes) {
            const int b = __builtin_ctzll(rest);
            rest &= rest - 1;
            codes[k - win0] = (uint16_t)((lane << 6) | b);
            ++k;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int n_here = min(kCodes, n_wave - win0);
        for (int j0 = 0; j0 < n_here; j0 += 64) {
            const int j = j0 + lane;
            const bool active = j < n_here;
            const int code = active ? (int)codes[j] : 0;
            const int owner = code >> 6, b = code & 63;
            const uint64_t* orow = rows + 6 * owner;
            const uint64_t o_xb = orow[0], o_nn = orow[1], o_xb1 = orow[2], o_nn1 = orow[3], o_Bw = orow[4];
            const int64_t o_lo_in = (int64_t)orow[5];
            int64_t h_a = 0, h_e = 0;                                 // (kWaveTokens) my token's absolute byte range
            if (active) {
                const int64_t obase = (w0 + owner) << 6;
                const uint64_t bl = o_Bw & ((2ull << b) - 1ull);      // string starts at or before the item (b = 63: all)
                const int64_t lo = bl ? obase + 63 - __builtin_clzll(bl) : o_lo_in;
                // token [p, e): e = next boundary; stripped extent [a2, e2).  The 64 positions from the item on, taken out
                // of the 128-bit pair (owner word, next word): one form whether the token ends in its own word or in the
                // next one (two divergent branches before, and some lane of 64 nearly always crosses a word)
                const uint64_t X = (o_xb >> b) | ((o_xb1 << 1) << (63 - b));     // boundaries at p, p+1, ..
                const uint64_t N = (o_nn >> b) | ((o_nn1 << 1) << (63 - b));     // non-SPACE chars at p, p+1, ..
                const uint64_t after = X & ~1ull;
                const int64_t pos = obase + b;
                int64_t e, a2, e2;                              // (e: the raw end, 4-field records only)
                if (after) {                                    // the token ends within 64 chars (kept => seg != 0)
                    const uint64_t seg = N & (((after & (~after + 1ull)) - 1ull));
                    e = pos + __builtin_ctzll(after);
                    a2 = pos + __builtin_ctzll(seg);
                    e2 = pos + 64 - __builtin_clzll(seg);
                } else if (o_xb1 & ~((1ull << b) - 1ull)) {     // (rare) longer: ends at a boundary of the next word beyond p + 63
                    const int eb = __builtin_ctzll(o_xb1 & ~((1ull << b) - 1ull));
                    const uint64_t seg0 = o_nn & (~0ull << b);
                    const uint64_t seg1 = o_nn1 & ((1ull << eb) - 1ull);
                    e = obase + 64 + eb;
                    a2 = seg0 ? obase + __builtin_ctzll(seg0) : obase + 64 + __builtin_ctzll(seg1);
                    e2 = seg1 ? obase + 128 - __builtin_clzll(seg1) : obase + 64 - __builtin_clzll(seg0);
                } else {                                        // (rare) no boundary up to the end of the next word
                    e = next_set_bit(p.bits, obase + 128, total);
                    const uint64_t seg = o_nn & (~0ull << b);
                    a2 = seg ? obase + __builtin_ctzll(seg) : (o_nn1 ? obase + 64 + __builtin_ctzll(o_nn1) : next_zero_bit(p.space, obase + 128, e));
                    e2 = prev_zero_end(p.space, a2, e);
                }
                c.short_token(base_out + win0 + j, pos, e, a2, e2, lo);
                h_a = a2;
                h_e = e2;
            }
            if constexpr (C::kWaveTokens) {
                // the long tokens of the round, one at a time by the whole wave (wave-uniform loop: `todo` is a ballot)
                const DwordsOf ld{c.h.text};
                for (uint64_t todo = __ballot(h_e - h_a > kHashWaveBytes); todo; todo &= todo - 1ull) {
                    const int src = __builtin_ctzll(todo);
                    const int64_t a = __shfl(h_a, src), e = __shfl(h_e, src);
                    const int64_t rounds = (((e - a) >> 2) + kThWaveBlocks - 1) / kThWaveBlocks;
                    uint32_t h = c.h.seed;
                    uint32_t mk = th_wave_block(ld, a, e, 0, lane);
                    for (int64_t r = 0; r < rounds; ++r) {
                        const uint32_t cur = mk;
                        if (r + 1 < rounds) mk = th_wave_block(ld, a, e, r + 1, lane);   // (the next round's loads fly during the fold)
                        h = th_wave_fold(h, [cur](int l) { return (uint32_t)__builtin_amdgcn_readlane((int)cur, l); }, th_wave_count(a, e, r));
                    }
                    c.long_token(base_out + win0 + j, a, e, th_wave_tail(ld, a, e, h), lane, lane == src);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    c.flush(lane);
}

// The body of every scatter kernel.  c: the kernel's consumer (Offsets: the word-major form); counts (or NULL): the per-string item
// counts; cap: the items the caller's buffers hold; vb: the (virtual) workgroup index.
template <typename OUT, class C>
__device__ __forceinline__ void scatter_block(const TokenPlanes& p, C& c, OUT* counts, int64_t cap, unsigned n_scatter_blocks, int* err, unsigned vb) {
    if (vb >= n_scatter_blocks) {   // role 2: one thread per string
        if (counts)
            string_counts_role<OUT>((int64_t)(vb - n_scatter_blocks) * (kScatterWaves * 64) + threadIdx.x, p.item_mask, p.tile_rank, p.word_pref,
                                    p.row_off, p.n_str, p.total, *p.n_items, counts, err);
        return;
    }
    // role 1: one wave per tile.  The caller's buffer holds `cap` items; when the batch has more, nothing is written
    // (the host reports the needed size) -- the launch does not have to wait for the host to learn the total.
    if (*p.n_items > cap) return;
    // Offsets: window of values (OUT); token-major: the item codes + the mask rows.  Sized for
    // what the form needs (it was 8 KB per wave for every form: 4 workgroups per CU).  Measured on C2, same box: int32 offsets
    // 0.174 -> 0.165 ms and int32 spans 0.233 -> 0.222 at 7 - 8 workgroups per CU, but int64 spans 0.247 -> 0.256 (twice
    // the store stream per token): that form keeps the footprint that holds it at 4.
    constexpr int kSpan64Buf = 6656;   // int64 spans: 5 workgroups per CU (4: C3 +2.5 %; 7: C2 +4 %)
    constexpr int kBufBytes = C::kWordMajor ? kScatterCodes * (int)sizeof(OUT)
                                            : (sizeof(OUT) == 8 ? kSpan64Buf : kScatterRowsEnd) + C::kLdsBytes;   // (a consumer's own bytes lie behind the rows)
    __shared__ __attribute__((aligned(16))) uint8_t buf_s[kScatterWaves][kBufBytes];
    __shared__ long long smax_s[kScatterWaves][65];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t w0 = ((int64_t)vb * kScatterWaves + wave) * 64;
    if (w0 >= p.n_words) return;                                    // whole wave (no block-wide barrier is used below)
    const int64_t w = w0 + lane;
    const int n_wave = (int)p.tile_cnt[w0 >> 6];
    if (n_wave == 0) return;
    const uint64_t x = w < p.n_words ? p.item_mask[w] : 0ull;
    const int off = w < p.n_words ? (int)p.word_pref[w] : 0;        // rank of my first item inside the wave
    const int64_t base_out = p.tile_rank[w0 >> 6];
    uint8_t* buf = buf_s[wave];
    uint64_t Bw;
    int64_t lo_in;
    tile_string_starts(p, w0, lane, reinterpret_cast<unsigned long long*>(smax_s[wave]), &Bw, &lo_in);
    if constexpr (C::kWordMajor) {
        offsets_walk<OUT>(x, off, n_wave, w, Bw, lo_in, reinterpret_cast<OUT*>(buf), c.out, base_out, lane);
    } else {
        static_assert(C::kLdsBytes == 0 || sizeof(OUT) == 4, "a consumer with LDS of its own is instantiated for int32 only");
        token_walk(p, c, buf, x, off, n_wave, w0, base_out, Bw, lo_in, lane);
    }
}

template <int KIND, typename OUT>
__global__ __launch_bounds__(kScatterWaves * 64) void k_counts_scatter(
    const uint64_t* __restrict__ bits, const uint64_t* __restrict__ space, const uint64_t* __restrict__ item_mask,
    const int64_t* __restrict__ tile_rank, const int64_t* __restrict__ tile_cnt, const uint16_t* __restrict__ word_pref,
    int64_t n_words, int64_t total, const int64_t* __restrict__ row_off, int64_t n_str,
    const int64_t* __restrict__ tile_first, OUT* __restrict__ out, const int64_t* __restrict__ n_items_dev, int64_t cap,
    OUT* __restrict__ counts, unsigned n_scatter_blocks, int* __restrict__ err, DoneSignal done, DeviceTotal dt) {
    TokenPlanes p{bits, space, item_mask, tile_rank, tile_cnt, word_pref, n_words, total, row_off, n_str, tile_first, n_items_dev};
    if (dt.total) {   // (uniform) the size from device memory; the records are not written for a batch reported as malformed
        p.total = device_total(dt.total, total);
        p.n_words = (p.total + 63) >> 6;
    }
    if (!(dt.gate && *dt.gate != 0 && blockIdx.x < n_scatter_blocks)) {   // (the counts role still runs: counts may be written)
        std::conditional_t<KIND == 0, Offsets<OUT>, SpanRecords<OUT, KIND == 2 ? 4 : 2>> c{{}, out};
        scatter_block<OUT>(p, c, counts, cap, n_scatter_blocks, err, blockIdx.x);
    }
    signal_block_done(done);   // (pinned outputs of a small host batch: the host polls the completion word)
}

// Token hashes and token ids in kernels of their own (k_counts_scatter keeps its arguments and its code).
template <typename OUT>
__global__ __launch_bounds__(kScatterWaves * 64) void k_hash_scatter(
    const uint64_t* __restrict__ bits, const uint64_t* __restrict__ space, const uint64_t* __restrict__ item_mask,
    const int64_t* __restrict__ tile_rank, const int64_t* __restrict__ tile_cnt, const uint16_t* __restrict__ word_pref,
    int64_t n_words, int64_t total, const int64_t* __restrict__ row_off, int64_t n_str,
    const int64_t* __restrict__ tile_first, OUT* __restrict__ out, const int64_t* __restrict__ n_items_dev, int64_t cap,
    OUT* __restrict__ counts, unsigned n_scatter_blocks, int* __restrict__ err, HashArgs ha) {
    const TokenPlanes p{bits, space, item_mask, tile_rank, tile_cnt, word_pref, n_words, total, row_off, n_str, tile_first, n_items_dev};
    HashTokens<OUT> c{{}, ha, out};
    scatter_block<OUT>(p, c, counts, cap, n_scatter_blocks, err, blockIdx.x);
}
template <typename OUT>
__global__ __launch_bounds__(kScatterWaves * 64) void k_vocab_scatter(
    const uint64_t* __restrict__ bits, const uint64_t* __restrict__ space, const uint64_t* __restrict__ item_mask,
    const int64_t* __restrict__ tile_rank, const int64_t* __restrict__ tile_cnt, const uint16_t* __restrict__ word_pref,
    int64_t n_words, int64_t total, const int64_t* __restrict__ row_off, int64_t n_str,
    const int64_t* __restrict__ tile_first, OUT* __restrict__ out, const int64_t* __restrict__ n_items_dev, int64_t cap,
    OUT* __restrict__ counts, unsigned n_scatter_blocks, int* __restrict__ err, HashArgs ha, VocabArgs va) {
    const TokenPlanes p{bits, space, item_mask, tile_rank, tile_cnt, word_pref, n_words, total, row_off, n_str, tile_first, n_items_dev};
    IdTokens<OUT> c{{}, ha, va, out};
    scatter_block<OUT>(p, c, counts, cap, n_scatter_blocks, err, blockIdx.x);
}

// Token counts and term keys: the planes and the consumer's state as one argument.  Neither writes records nor is gated by a
// capacity.  Token counts have no per-string counts; those of the term keys are int64 (they feed the row scan of the term-count calls).
struct CountScatterArgs {
    TokenPlanes p;
    unsigned n_scatter_blocks; int* err;
    HashArgs ha; CountArgs ca;
};
__global__ __launch_bounds__(kScatterWaves * 64) void k_count_scatter(CountScatterArgs a) {
    CountTokens c{{}, a.ha, a.ca};
    scatter_block<int32_t>(a.p, c, (int32_t*)nullptr, INT64_MAX, a.n_scatter_blocks, a.err, blockIdx.x);
}
struct TermScatterArgs {
    TokenPlanes p;
    int64_t* counts;
    unsigned n_scatter_blocks; int* err;
    HashArgs ha; VocabArgs va; TermArgs ta;
};
__global__ __launch_bounds__(kScatterWaves * 64) void k_term_scatter(TermScatterArgs a) {
    TermTokens c{{}, a.ha, a.va, a.ta};
    scatter_block<int64_t>(a.p, c, a.counts, INT64_MAX, a.n_scatter_blocks, a.err, blockIdx.x);
}

// The commit behind k_count_scatter: two launches over the slots, one thread per slot, that make the table independent of the
// caller's text.  (a) k_count_commit_sum: the padded dwords of the fresh slots, reduced per workgroup, one atomic each -> ctl[0];
// the host reads it and grows the blob if it has to.  (b) k_count_commit_copy: every workgroup takes its share of the blob with
// one atomic add on the cursor ctl[1], its fresh slots copy their <= 256 bytes from the text (ct_commit_word) and store their
// resident word; ctl[2] (distinct) advances by the workgroup's fresh slots.  A share that would leave the blob is not written and
// raises ctl[3] (the host sized the blob from (a), so this does not happen; the host then fails the counter).  The workgroup sums
// and prefixes are block_scan_add (block_ops.h).
constexpr int kCommitBlock = 256;
__global__ __launch_bounds__(kCommitBlock) void k_count_commit_sum(const uint64_t* __restrict__ slots, uint64_t n_slots,
                                                                   unsigned long long* __restrict__ ctl) {
    const uint64_t i = (uint64_t)blockIdx.x * kCommitBlock + threadIdx.x;
    const uint64_t v = i < n_slots ? slots[i] : kCtEmpty;
    __shared__ unsigned s_wave[kCommitBlock / 64];
    unsigned total;
    (void)block_scan_add<unsigned, kCommitBlock / 64>(ct_is_fresh(v) ? ct_padded_dwords(v) : 0u, s_wave, &total);
    if (threadIdx.x == 0 && total) (void)__hip_atomic_fetch_add(ctl + 0, (unsigned long long)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__global__ __launch_bounds__(kCommitBlock) void k_count_commit_copy(uint64_t* __restrict__ slots, uint64_t n_slots,
                                                                    const uint32_t* __restrict__ text, uint32_t* __restrict__ blob,
                                                                    uint64_t blob_dwords, unsigned long long* __restrict__ ctl) {
    __shared__ unsigned long long s_base;
    __shared__ unsigned s_wave[kCommitBlock / 64];
    const uint64_t i = (uint64_t)blockIdx.x * kCommitBlock + threadIdx.x;
    const uint64_t v = i < n_slots ? slots[i] : kCtEmpty;
    const bool fresh = ct_is_fresh(v);
    const unsigned dwords = fresh ? ct_padded_dwords(v) : 0u;
    unsigned total, n_fresh;
    const unsigned before = block_scan_add<unsigned, kCommitBlock / 64>(dwords, s_wave, &total) - dwords;
    (void)block_scan_add<unsigned, kCommitBlock / 64>(fresh ? 1u : 0u, s_wave, &n_fresh);
    if (total == 0) return;                            // (uniform)
    if (threadIdx.x == 0) {
        s_base = __hip_atomic_fetch_add(ctl + 1, (unsigned long long)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (void)__hip_atomic_fetch_add(ctl + 2, (unsigned long long)n_fresh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (!fresh) return;
    const uint64_t at = s_base + before;
    if (at + ct_padded_dwords(v) > blob_dwords) {      // never with a blob sized from k_count_commit_sum
        ctl[3] = 1ull;
        return;
    }
    slots[i] = ct_commit_word([text](int64_t k) { return text[k]; }, v, at, [blob](uint64_t k, uint32_t w) { blob[k] = w; });
}

// ---- code-point results of a UTF-8 batch from its BYTE-space results ------------------------------------------------------
// The reference reads a str as code points (latok.c:53-55,79) and reports boundaries as code-point indices.  A UTF-8 batch in
// code-point units used to be decoded into a UTF-32 copy first (1 B read + 4 B written + 4 B read again per char); instead the
// byte-space tile kernel runs on the bytes themselves and leaves two bitmasks over the BYTES -- boundaries (set at lead bytes)
// and lead bytes -- plus, per 64-byte word, the number of leads of its tile before it and the leads per tile.  Code point k of
// the batch is the k-th lead byte, so
//   cp mask        = the boundary bits at the lead positions, packed: per word pext(boundaries, leads), appended at the word's
//                    rank = leads before it (tile_rank from k_scan_chained over the tile counts + the word's prefix);
//   cp_row_off[s]  = number of leads before byte_off[s].
// One workgroup per 16 tiles of 64 words; the packed chunks of its words meet in one LDS window (a chunk straddles at most two
// output words) and leave as whole words.  Every output word is written exactly once, by the workgroup that holds the lead of
// its LAST bit (the batch's final, partial word: by the last workgroup with a lead): the bits of a workgroup's first word that
// belong to earlier ones are recomputed by its first wave from the words in front of it.  No atomics on global memory, no
// cleared output (two global atomics per tile cost 40 of 110 us on C3); the kernel is bound by the pext: through a 256-byte table
// of 4-bit pexts in LDS (~100 VALU per word; the five-round arithmetic compress: ~256, 80 us on C3; one wave per tile with a
// look-back pext of its own: 106 us).  Role 2 (the workgroups behind): one thread
// per row offset.
// *odd is raised when the byte-space model and the decoder's model of MALFORMED input differ: a continuation byte with no lead
// byte within the 3 bytes before it, or at the start of a string (the host then takes the staged decoder instead).
// kCompressWaves (kernels.h): tiles per workgroup
constexpr int kCompressWords = kCompressWaves * 64;        // input words per workgroup = output words it can own (+ 1)
template <bool TWO>   // TWO: a second byte-space mask (the SPACE plane, for token spans) is packed the same way into out_mask2
__global__ __launch_bounds__(kCompressWaves * 64) void k_lead_compress(
    const uint64_t* __restrict__ bmask, const uint64_t* __restrict__ bmask2, uint64_t* __restrict__ out_mask2,
    const uint64_t* __restrict__ lead, const int64_t* __restrict__ tile_rank, const int64_t* __restrict__ tile_cnt,
    const uint16_t* __restrict__ word_pref, int64_t n_words, int64_t total_bytes, const int64_t* __restrict__ byte_off, int64_t n_str,
    const int64_t* __restrict__ total_cps_dev, uint64_t* __restrict__ out_mask, int64_t cap_words, int64_t* __restrict__ cp_row_off,
    int* __restrict__ odd, unsigned n_tile_blocks) {
    if (blockIdx.x >= n_tile_blocks) {   // role 2: code-point offset of every string (and of the end of the batch)
        const int64_t total_cps = *total_cps_dev;
        const int64_t s = (int64_t)(blockIdx.x - n_tile_blocks) * (kCompressWaves * 64) + threadIdx.x;
        if (s > n_str) return;
        const int64_t b = byte_off[s];
        if (b >= total_bytes) { cp_row_off[s] = total_cps; return; }
        const int64_t bw = b >> 6;
        const uint64_t mw = lead[bw];
        cp_row_off[s] = tile_rank[bw >> 6] + word_pref[bw] + __popcll(mw & low_mask((int)(b & 63)));
        if (s < n_str && byte_off[s + 1] > b && !((mw >> (b & 63)) & 1ull)) *odd = 1;   // a string begins with a continuation byte
        return;
    }
    // The workgroup takes kCompressWaves consecutive tiles; their packed chunks meet in ONE window in LDS, so only the
    // workgroup's first output word needs bits from in front of it (and only its last, partial one is left to the next).
    __shared__ unsigned long long win_s[TWO ? 2 : 1][kCompressWords + 2];
    __shared__ __attribute__((aligned(16))) uint8_t pext_tab[256];       // lk_pext4_entry: 4-bit pexts (lane_math.h)
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < 256) pext_tab[tid] = lk_pext4_entry((uint32_t)tid);
    const int64_t n_tiles = (n_words + 63) >> 6;
    const int64_t T0 = (int64_t)blockIdx.x * kCompressWaves;
    const int64_t T1 = min(T0 + kCompressWaves, n_tiles) - 1;      // the workgroup's last tile
    const int64_t t = min(T0 + (tid >> 6), T1);
    const int64_t w = T0 * 64 + tid;
    const bool in = w < n_words;
    // everything the thread needs from memory is requested here, in one round trip, by unconditional loads at clamped addresses
    // (a predicated load is a branch, and hipcc waits for everything in flight at it)
    const int64_t total_cps = *total_cps_dev;
    const int64_t wc = in ? w : n_words - 1;
    lk_u64 m = lead[wc];
    lk_u64 x = bmask[wc];
    lk_u64 x2 = TWO ? bmask2[wc] : 0ull;
    const uint64_t m_before = lead[wc > 0 ? wc - 1 : 0];           // (the word before mine: every thread loads its own, coalesced)
    const int64_t my_pos0 = tile_rank[t];                          // code-point index of my tile's first lead
    const int pref = (int)word_pref[wc];
    const int64_t pos0 = tile_rank[T0];                            // ... of the workgroup's
    const int64_t end = tile_rank[T1] + tile_cnt[T1];              // one past the workgroup's last code point
    // the look-back (first wave): lane k takes the k-th word in front of the workgroup
    const int64_t wk = T0 * 64 - 1 - lane > 0 ? T0 * 64 - 1 - lane : 0;
    lk_u64 mb = 0, xb = 0, xb2 = 0;
    if (tid < 64) { mb = lead[wk]; xb = bmask[wk]; xb2 = TWO ? bmask2[wk] : 0ull; }
    unsigned long long* win = win_s[0];
    unsigned long long* win2 = win_s[TWO ? 1 : 0];
    win[tid] = 0ull;
    if (tid < 2) win[kCompressWords + tid] = 0ull;
    if (TWO) {
        win2[tid] = 0ull;
        if (tid < 2) win2[kCompressWords + tid] = 0ull;
    }
    if (!in) { m = 0ull; x = 0ull; x2 = 0ull; }
    // continuation bytes without a lead byte in the 3 bytes before them (malformed input)
    {
        const uint64_t C = in ? (~m & valid_mask(w, total_bytes)) : 0ull;
        const uint64_t Cp = w > 0 ? ~m_before : 0ull;
        const uint64_t run = C & ((C << 1) | (Cp >> 63)) & ((C << 2) | (Cp >> 62)) & ((C << 3) | (Cp >> 61));
        if (run) *odd = 1;
    }
    if ((total_cps + 63) / 64 > cap_words) return;                 // the caller's mask is too small: nothing is written (uniform)
    const int64_t ow0 = pos0 >> 6;                                 // first output word the workgroup has bits in
    // words the workgroup owns: those whose last bit is its own, + the batch's final partial word if its last lead is
    const int64_t own_end = end == total_cps ? (end + 63) >> 6 : end >> 6;
    if (end == pos0 || own_end <= ow0) return;                     // no lead at all / all bits lie in a word a later one owns (uniform)
    // Every byte of the workgroup's tiles is a lead (ASCII text) and its first code point opens an output word: code point k of the
    // range IS byte k, the packed words are the input words (uniform; nothing to pack, nothing shared with a neighbour).
    {
        const int64_t b0 = T0 * kTile, b1 = min((T1 + 1) * (int64_t)kTile, total_bytes);
        if ((pos0 & 63) == 0 && end - pos0 == b1 - b0) {
            if (in) {
                out_mask[ow0 + tid] = x;
                if (TWO) out_mask2[ow0 + tid] = x2;
            }
            return;
        }
    }
    __syncthreads();
    {
        const int64_t pos = my_pos0 + pref;
        const int rel = (int)((pos >> 6) - ow0), sh = (int)(pos & 63);
        if (TWO) {
            if (x | x2) {
                lk_pext64_lut<true>(&x, &x2, m, pext_tab);
                if (x) {
                    atomicOr(&win[rel], x << sh);
                    if (sh && (x >> (64 - sh))) atomicOr(&win[rel + 1], x >> (64 - sh));
                }
                if (x2) {
                    atomicOr(&win2[rel], x2 << sh);
                    if (sh && (x2 >> (64 - sh))) atomicOr(&win2[rel + 1], x2 >> (64 - sh));
                }
            }
        } else if (x) {                                            // (a word without boundaries adds nothing)
            lk_u64 c = x, unused = 0;
            lk_pext64_lut<false>(&c, &unused, m, pext_tab);
            atomicOr(&win[rel], c << sh);
            if (sh && (c >> (64 - sh))) atomicOr(&win[rel + 1], c >> (64 - sh));
        }
    }
    if (tid < 64) {
        // the bits of the first word that belong to earlier workgroups: the `need` leads in front of this one, nearest word first
        // (the 63 leads before a tile lie in its previous 4 words in well-formed text; the look-back goes on for as long as
        // malformed input makes it)
        int need = (int)(pos0 & 63);
        for (int64_t back = 0; need > 0; back += 64) {             // wave-uniform; one round unless the input is malformed
            const int64_t wj = T0 * 64 - 1 - back - lane;
            if (back > 0) {
                mb = wj >= 0 ? lead[wj] : 0ull;
                xb = wj >= 0 ? bmask[wj] : 0ull;
                xb2 = (TWO && wj >= 0) ? bmask2[wj] : 0ull;
            } else if (wj < 0) {
                mb = 0ull; xb = 0ull; xb2 = 0ull;
            }
            const int cnt = __popcll(mb);
            int inc = cnt;   // (written out: shfl_scan_add here reorders the kernel's instructions)
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int o = __shfl_up(inc, d);
                if (lane >= d) inc += o;
            }
            const int before = inc - cnt;                           // leads between my word and the workgroup's first
            if (cnt > 0 && before < need) {
                const int take = min(cnt, need - before);           // my top `take` leads
                lk_u64 c = xb, c2 = xb2;
                lk_pext64_lut<TWO>(&c, &c2, mb, pext_tab);
                c >>= (cnt - take);
                if (c) atomicOr(&win[0], c << (need - before - take));
                if (TWO) {
                    c2 >>= (cnt - take);
                    if (c2) atomicOr(&win2[0], c2 << (need - before - take));
                }
            }
            need -= __shfl(inc, 63);
            if (T0 * 64 - 1 - back - 63 <= 0) break;                // the batch begins here (cannot happen with need > 0: ranks are exact)
        }
    }
    __syncthreads();
    const int n_out = (int)(own_end - ow0);                         // 1 .. kCompressWords + 1
    for (int j = tid; j < n_out; j += kCompressWaves * 64) {
        out_mask[ow0 + j] = win[j];
        if (TWO) out_mask2[ow0 + j] = win2[j];
    }
}

hipError_t launch_lead_compress(const uint64_t* bmask, const uint64_t* bmask2, const uint64_t* lead, const int64_t* tile_rank,
                                const int64_t* tile_cnt, const uint16_t* word_pref, int64_t n_words, int64_t total_bytes,
                                const int64_t* byte_off, int64_t n_str, const int64_t* total_cps_dev, uint64_t* out_mask,
                                uint64_t* out_mask2, int64_t cap_words, int64_t* cp_row_off, int* odd, hipStream_t st) {
    const int64_t n_tiles = (n_words + 63) / 64;
    const unsigned nb_tiles = (unsigned)((n_tiles + kCompressWaves - 1) / kCompressWaves);
    const unsigned nb_rows = (unsigned)((n_str + 1 + kCompressWaves * 64 - 1) / (kCompressWaves * 64));
    const dim3 grid(nb_tiles + nb_rows), block(kCompressWaves * 64);
    if (bmask2)
        hipLaunchKernelGGL(k_lead_compress<true>, grid, block, 0, st, bmask, bmask2, out_mask2, lead, tile_rank, tile_cnt, word_pref, n_words,
                           total_bytes, byte_off, n_str, total_cps_dev, out_mask, cap_words, cp_row_off, odd, nb_tiles);
    else
        hipLaunchKernelGGL(k_lead_compress<false>, grid, block, 0, st, bmask, bmask2, out_mask2, lead, tile_rank, tile_cnt, word_pref, n_words,
                           total_bytes, byte_off, n_str, total_cps_dev, out_mask, cap_words, cp_row_off, odd, nb_tiles);
    return hipGetLastError();
}

// ---- rule code of every char from byte space (featurize of UTF-8 in code-point units) --------------------------------------
// k_features_tiles reads the rule code of every char (FeatParams::codes, 1 B/char), which the UTF-32 tile kernel leaves as it
// classifies.  A UTF-8 batch in code-point units has no UTF-32 copy: after the byte-space pipeline (lead-byte mask, leads per
// word and per tile) and k_scan_chained (tile ranks), this kernel stores, for every lead byte, the rule code of its char at the
// char's code-point index tile_rank[t] + word_pref[w] + (leads below it in the word).  It classifies as bytes_phase1 does: the
// byte-space rule-code table (kernels.h: kB6*), an ASCII byte by one lookup, a multi-byte char through lk_lead_entry_of /
// lk_lead_index in at most two decode slots per dword (more only in malformed input: a wave-uniform loop), U+FFFD for a sequence
// that is cut short -- so the codes are what the UTF-32 tile kernel writes for the decoded char.
// A group = kCompressWaves tiles (k_lead_compress's geometry), one thread per 64-byte word; a workgroup walks groups (the class
// table is copied to LDS once per workgroup).  The codes of a group are one contiguous range [tile_rank[T0], tile_rank[T1] +
// tile_cnt[T1]).  Per dword a thread packs its lead bytes' codes with one v_perm (selector by the dword's lead nibble) and
// appends them to a 64-bit accumulator, which ORs every full dword into a zeroed LDS window over the range (4 pad bytes per 64:
// an all-lead wave writes without bank conflicts; the dwords a thread shares with its neighbours merge by the OR).  The window
// goes out with dword stores, byte stores at its two ends.  Ranges of different groups never overlap: no global atomics.
constexpr int kLeadCodesWin = kCompressWaves * kTile + 8;                         // the range + its offset in its first dword
constexpr int kLeadCodesLds = kLeadCodesWin + 4 * ((kLeadCodesWin + 63) / 64);
__device__ __forceinline__ int lead_codes_slot(int i) { return i + ((i >> 6) << 2); }   // LDS byte of window byte i (i % 4 == 0)

// one decode slot of a dword: the multi-byte lead that `s` marks (bit 7 of its byte; s == 0: byte 3, whatever it is) -> its code
// ORed into `out` at its byte (a slot without a lead adds 0 or its dword's lead's own code again, bytes_phase1's argument)
__device__ __forceinline__ void lead_codes_slot_decode(uint32_t lo, uint32_t hi, uint32_t s, const uint2* ltab, const uint8_t* t1b,
                                                       const uint8_t* t2b, uint32_t code_fffd, uint32_t& out) {
    const uint32_t r8 = (uint32_t)__builtin_ctz(s | 0x80000000u) & 24u;
    const uint32_t W = __builtin_amdgcn_alignbit(hi, lo, r8);   // the 4 bytes from the slot's byte on (lo = dword Q, hi = Q + 1)
    const uint2 q = ltab[W & 0xFFu];
    lk_lead_entry e;
    e.sel = q.x;
    e.hi0 = q.y;
    uint32_t off2, R;
    const bool bad = lk_lead_index(e, W, &off2, &R);
    off2 = min(off2, 2u * (uint32_t)(kB6Stage1Len - 1));
    const uint32_t blk = *reinterpret_cast<const uint16_t*>(t1b + off2);
    const uint32_t code = t2b[blk | (R & 0x3Fu)];
    out = bad ? ((out & ~(0xFFu << r8)) | (code_fffd << r8)) : (out | (code << r8));
}

__global__ __launch_bounds__(kCompressWaves * 64) void k_lead_codes(
    const uint8_t* __restrict__ u8, int64_t total_bytes, const uint64_t* __restrict__ lead, const int64_t* __restrict__ tile_rank,
    const int64_t* __restrict__ tile_cnt, const uint16_t* __restrict__ word_pref, int64_t n_words, const uint8_t* __restrict__ tb6rule,
    uint8_t* __restrict__ codes) {
    __shared__ __attribute__((aligned(16))) uint8_t tab_s[kB6TablesBytes];
    __shared__ __attribute__((aligned(16))) uint8_t win_s[kLeadCodesLds];
    __shared__ uint2 ltab_s[256];                                  // lk_lead_entry_of of every byte value
    __shared__ uint8_t ctab_s[256];                                // code of a byte taken as a char (0 from 0x80 on)
    __shared__ uint32_t sel_s[16];                                 // v_perm selector that packs the lead bytes of a dword
    const int tid = threadIdx.x;
    constexpr int NT = kCompressWaves * 64;
    for (int i = tid; i < kB6TablesBytes / 16; i += NT)
        reinterpret_cast<uint4*>(tab_s)[i] = reinterpret_cast<const uint4*>(tb6rule)[i];
    if (tid < 256) {
        const lk_lead_entry e = lk_lead_entry_of((uint32_t)tid);
        ltab_s[tid] = make_uint2(e.sel, e.hi0);
        ctab_s[tid] = tid < 0x80 ? tb6rule[kB6Stage1Bytes + tid] : (uint8_t)0;   // (ASCII = stage 2's first two blocks)
    }
    if (tid < 16) {
        uint32_t sel = 0x04040404u;                                // byte 4 of {0, x}: 0
        int j = 0;
        for (int k = 0; k < 4; ++k)
            if ((tid >> k) & 1) { sel = (sel & ~(0xFFu << (8 * j))) | ((uint32_t)k << (8 * j)); ++j; }
        sel_s[tid] = sel;
    }
    const uint8_t* t1b = tab_s;
    const uint8_t* t2b = tab_s + kB6Stage1Bytes;
    uint32_t* win32 = reinterpret_cast<uint32_t*>(win_s);
    const int64_t n_tiles = (n_words + 63) >> 6;
    const int64_t n_groups = (n_tiles + kCompressWaves - 1) / kCompressWaves;
    for (int64_t G = blockIdx.x; G < n_groups; G += gridDim.x) {
        const int64_t T0 = G * kCompressWaves;
        const int64_t T1 = min(T0 + kCompressWaves, n_tiles) - 1;
        const int64_t pos0 = tile_rank[T0];
        const int64_t end = tile_rank[T1] + tile_cnt[T1];
        // no lead byte at all; or ranks that cannot be (the scan failed: the host sees its flag and drops the batch) -- uniform
        if (end == pos0 || pos0 < 0 || end < pos0 || end - pos0 > (int64_t)kCompressWaves * kTile || end > total_bytes) continue;
        const int64_t t = min(T0 + (tid >> 6), T1);
        const int64_t w = T0 * 64 + tid;
        const bool in = w < n_words;
        const int64_t wc = in ? w : n_words - 1;
        uint64_t m = in ? lead[wc] : 0ull;
        const int64_t pos = tile_rank[t] + word_pref[wc];          // code-point index of my word's first lead
        if (pos < pos0 || pos + __popcll(m) > end) m = 0ull;       // (the same: every store stays inside the range)
        // my 64 bytes (0 past the end of the batch) and the 4 after them (the next lane's first dword; lane 63: from memory)
        uint32_t d[17];
        const int64_t b = w * 64;
        if (in && b + 64 <= total_bytes) {
            const uint4* src = reinterpret_cast<const uint4*>(u8 + b);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint4 v = src[k];
                d[4 * k] = v.x; d[4 * k + 1] = v.y; d[4 * k + 2] = v.z; d[4 * k + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                uint32_t x = 0;
                for (int j = 0; j < 4; ++j)
                    if (b + 4 * q + j < total_bytes) x |= (uint32_t)u8[b + 4 * q + j] << (8 * j);
                d[q] = x;
            }
        }
        d[16] = (uint32_t)__shfl_down((int)d[0], 1);
        if ((tid & 63) == 63) {
            uint32_t x = 0;
            for (int j = 0; j < 4; ++j)
                if (b + 64 + j < total_bytes) x |= (uint32_t)u8[b + 64 + j] << (8 * j);
            d[16] = x;
        }
        const int64_t wb = pos0 & ~(int64_t)3;                     // window byte 0 = the first byte of the range's first dword
        const int n_win = (int)((end - wb + 3) >> 2);              // window dwords
        for (int i = tid; i < n_win + (n_win >> 4) + 1; i += NT) win32[i] = 0u;
        __syncthreads();                                           // (also: the tables, for the first group)
        const uint32_t code_fffd = t2b[*reinterpret_cast<const uint16_t*>(t1b + 2u * (0xFFFDu >> 6)) | (0xFFFDu & 63u)];
        const int o = (int)(pos - wb);
        int e = o >> 2, cnt = o & 3;                               // next window dword, bytes in the accumulator (the first
        uint64_t acc = 0;                                          // `cnt` are a neighbour's: 0, merged by the OR)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const uint32_t x = d[q];
            uint32_t out = (uint32_t)ctab_s[x & 0xFFu] | ((uint32_t)ctab_s[(x >> 8) & 0xFFu] << 8) |
                           ((uint32_t)ctab_s[(x >> 16) & 0xFFu] << 16) | ((uint32_t)ctab_s[x >> 24] << 24);
            const uint32_t hi = x & 0x80808080u;
            const uint32_t m1 = hi & (x << 1);                     // multi-byte leads (11xxxxxx), "bit 7 of the byte" form
            if (__any(m1 != 0u)) {                                 // (wave-uniform)
                const uint32_t m2 = m1 & (m1 - 1u);
                lead_codes_slot_decode(x, d[q + 1], m1, ltab_s, t1b, t2b, code_fffd, out);
                if (__any(m2 != 0u)) {
                    lead_codes_slot_decode(x, d[q + 1], m2, ltab_s, t1b, t2b, code_fffd, out);
                    uint32_t rest = m2 & (m2 - 1u);                // leads beyond two per dword (malformed input)
                    while (__any(rest != 0u)) {
                        if (rest) lead_codes_slot_decode(x, d[q + 1], rest, ltab_s, t1b, t2b, code_fffd, out);
                        rest &= rest - 1u;
                    }
                }
            }
            const uint32_t L = (uint32_t)(m >> (4 * q)) & 15u;
            const uint32_t packed = __builtin_amdgcn_perm(0u, out, sel_s[L]);
            acc |= (uint64_t)packed << (8 * cnt);
            cnt += __popc(L);
            const bool full = cnt >= 4;
            atomicOr(&win32[e + (e >> 4)], full ? (uint32_t)acc : 0u);
            e += full ? 1 : 0;
            acc = full ? acc >> 32 : acc;
            cnt -= full ? 4 : 0;
        }
        if (cnt > 0) atomicOr(&win32[e + (e >> 4)], (uint32_t)acc);
        __syncthreads();
        // out: every dword of the range, whole where the range covers it, else byte by byte (the range's first and last dword)
        const int64_t q0 = pos0 >> 2, q1 = (end + 3) >> 2;
        for (int64_t q = q0 + tid; q < q1; q += NT) {
            const int i = (int)(q - q0);
            const uint32_t v = win32[i + (i >> 4)];
            if (4 * q >= pos0 && 4 * q + 4 <= end) {
                *reinterpret_cast<uint32_t*>(codes + 4 * q) = v;
            } else {
                for (int j = 0; j < 4; ++j)
                    if (4 * q + j >= pos0 && 4 * q + j < end) codes[4 * q + j] = (uint8_t)(v >> (8 * j));
            }
        }
        __syncthreads();                                           // (the window is zeroed again for the next group)
    }
}

hipError_t launch_lead_codes(const uint8_t* u8, int64_t total_bytes, const uint64_t* lead, const int64_t* tile_rank, const int64_t* tile_cnt,
                             const uint16_t* word_pref, int64_t n_words, const uint8_t* tb6rule, uint8_t* codes, int n_cu, hipStream_t st) {
    const int64_t n_tiles = (n_words + 63) / 64;
    if (n_tiles <= 0) return hipSuccess;
    const int64_t n_groups = (n_tiles + kCompressWaves - 1) / kCompressWaves;
    const unsigned nb = (unsigned)min(n_groups, (int64_t)max(n_cu, 1));   // one workgroup per CU (LDS), each walks its groups
    hipLaunchKernelGGL(k_lead_codes, dim3(nb), dim3(kCompressWaves * 64), 0, st, u8, total_bytes, lead, tile_rank, tile_cnt, word_pref,
                       n_words, tb6rule, codes);
    return hipGetLastError();
}

// The zero padding k_features_tiles reads behind the last rule code (one tile + 256 B), for a batch whose code-point total only
// the device knows: written at codes[*total_dev ..) by this launch instead of a memset the host would have to place.
__global__ __launch_bounds__(256) void k_pad_codes(uint8_t* __restrict__ codes, const int64_t* __restrict__ total_dev, int64_t bound,
                                                   int n_pad) {
    const int64_t total = device_total(total_dev, bound);
    for (int i = threadIdx.x; i < n_pad; i += 256) codes[total + i] = 0;
}
hipError_t launch_pad_codes(uint8_t* codes, const int64_t* total_dev, int64_t bound, hipStream_t st) {
    hipLaunchKernelGGL(k_pad_codes, dim3(1), dim3(256), 0, st, codes, total_dev, bound, kTile + 256);
    return hipGetLastError();
}

// ---- joined token text: sep.join(tokenize(text)) of every string, UTF-8 out (reference default_tokenizer.py:149-160) ------
// The tokens as text instead of positions: for every string its stripped, non-empty tokens (exactly the byte ranges
// k_counts_scatter<1> reports) joined by one separator byte, all rows back to back in one buffer plus out_off[n_str + 1].
// Mask-driven and parallel over the packed buffer; span records are never formed.  Two planes per 64-byte word (lane_math.h:
// lk_join_planes): body = the byte is copied, head = a separator goes in front of it.  An output item is a body bit or a head
// bit; the output position of body byte i is (body bits before i) + (head bits at or before i), its separator one before.
//   k_join_counts    one wave per 4096-byte tile, lane = word: the two planes, items per word (uint16 prefix) and per tile
//   k_scan_chained   tile ranks and the byte total (unchanged: at most 8192 items per tile, the uint16 word prefix holds them)
//   k_join_scatter   one wave per tile: the tile's bytes, compacted with their separators into an LDS window, leave as one
//                    contiguous run; behind them one thread per string: out_off[s] = rank of byte_off[s], O(1)
// A token (or a string's leading whitespace) that reaches beyond the tile needs three carries into it: "a non-SPACE byte
// earlier in my token", "... later in my token", "... earlier in my string".  Inside a tile they are carry chains over the
// ballots of the words' summaries; from outside, the wave reads the neighbouring tiles' masks 64 words per step until the
// question is settled -- one step in ordinary text, one step per 4096 bytes for a token or a whitespace prefix that long
// (every step is one coalesced load per plane by the whole wave, never a per-string or per-token serial walk).
constexpr int kJoinWaves = 4;
constexpr int kJoinWin = 2 * kTile + 16;   // items of a tile (every byte a one-byte token with its separator: 2 per byte) + the run's offset inside its first dword

__global__ __launch_bounds__(kJoinWaves * 64) void k_join_counts(
    const uint64_t* __restrict__ bits, const uint64_t* __restrict__ space, int64_t n_words, int64_t total,
    const int64_t* __restrict__ row_off, int64_t n_str, const int64_t* __restrict__ tile_first, uint64_t* __restrict__ body_out,
    uint64_t* __restrict__ head_out, int64_t* __restrict__ tile_cnt, uint16_t* __restrict__ word_pref) {
    __shared__ unsigned long long bw_s[kJoinWaves][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t t = (int64_t)blockIdx.x * kJoinWaves + wave;
    const int64_t w0 = t * 64;
    if (w0 >= n_words) return;                                      // whole wave (no block-wide barrier is used below)
    const int64_t n_tiles = (n_words + 63) >> 6;
    const int64_t w = w0 + lane;
    const bool in = w < n_words;
    const uint64_t x = in ? bits[w] : 0ull;
    const uint64_t nn = in ? (~space[w] & valid_mask(w, total)) : 0ull;
    // string starts of the tile as bits (k_counts_scatter's step (a)) and the start of the string that is open at its first byte
    const int64_t t0 = w0 << 6;
    int64_t idx0 = tile_first[t];
    idx0 = idx0 < 0 ? 0 : (idx0 > n_str ? n_str : idx0);
    const int64_t start_before = idx0 > 0 ? row_off[idx0 - 1] : 0;
    const bool starts_here = row_off[idx0] == t0;                   // (row_off has n_str + 1 entries)
    unsigned long long* bw = bw_s[wave];
    bw[lane] = 0ull;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int64_t i0 = idx0; i0 < n_str; i0 += 64) {
        const int64_t sidx = i0 + lane;
        const int64_t ro = sidx < n_str ? row_off[sidx] : INT64_MAX;
        const int64_t rel = ro - t0;
        if (rel >= 0 && rel < 4096) atomicOr(&bw[rel >> 6], 1ull << (rel & 63));
        if (__shfl(ro, 63) >= t0 + 4096) break;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const uint64_t r = bw[lane];
    // carries from the tiles in front: the open token has a non-SPACE byte there (f_in), the open string has one (q_in)
    int f_in = 0, q_in = 0, b_in = 0;
    bool f_open = true, q_open = !starts_here && t0 > start_before;   // (wave-uniform)
    for (int64_t k = t - 1; k >= 0 && (f_open || q_open); --k) {
        const int64_t v = k * 64 + lane;                            // (a tile in front of mine lies inside the batch entirely)
        const uint64_t xv = bits[v], nv = ~space[v];
        if (f_open) {
            const lk_join_sum s = lk_join_summary(xv, nv, 0ull);
            const uint64_t G = __ballot(s.gen_f), P = __ballot(s.prop_x);
            if (lk_seg_out(G, ~P, lk_seg_carries(G, ~P, 0))) { f_in = 1; f_open = false; }
            else if (P != ~0ull) f_open = false;                    // a boundary with nothing but SPACE behind it
        }
        if (q_open) {
            const int64_t base = v << 6;
            uint64_t m = nv;
            if (base + 64 <= start_before) m = 0ull;
            else if (base < start_before) m &= ~0ull << (start_before - base);
            if (__ballot(m != 0ull)) { q_in = 1; q_open = false; }
            else if (k * (int64_t)kTile <= start_before) q_open = false;
        }
    }
    // ... and from the tiles behind: the token that is open at my last byte has a non-SPACE byte there (b_in)
    for (int64_t k = t + 1; k < n_tiles; ++k) {
        const int64_t v = k * 64 + lane;
        const bool vin = v < n_words;
        const uint64_t xv = vin ? bits[v] : 0ull;
        const uint64_t nv = vin ? (~space[v] & valid_mask(v, total)) : 0ull;
        const lk_join_sum s = lk_join_summary(xv, nv, 0ull);
        const uint64_t Gr = lk_rev(__ballot(s.gen_b)), P = __ballot(s.prop_x);
        const uint64_t Sr = lk_rev(~P);
        if (lk_seg_out(Gr, Sr, lk_seg_carries(Gr, Sr, 0))) { b_in = 1; break; }
        if (P != ~0ull) break;
    }
    // the chains over the tile's 64 words (bit = word), then inside the word
    const lk_join_sum s = lk_join_summary(x, nn, r);
    const uint64_t Gf = __ballot(s.gen_f), Gb = __ballot(s.gen_b), Gq = __ballot(s.gen_q);
    const uint64_t Sx = ~__ballot(s.prop_x), Sr = ~__ballot(s.prop_r);
    const int cf = (int)((lk_seg_carries(Gf, Sx, f_in) >> lane) & 1ull);
    const int cb = (int)((lk_seg_carries(lk_rev(Gb), lk_rev(Sx), b_in) >> (63 - lane)) & 1ull);
    const int cq = (int)((lk_seg_carries(Gq, Sr, q_in) >> lane) & 1ull);
    const lk_join_planes_t o = lk_join_planes(x, nn, r, cf, cb, cq);
    if (in) {
        body_out[w] = o.body;
        head_out[w] = o.head;
    }
    const int cnt = __popcll(o.body) + __popcll(o.head);
    const int inc = shfl_scan_add(cnt, lane);
    if (in) word_pref[w] = (uint16_t)(inc - cnt);
    if (lane == 63) tile_cnt[t] = inc;
}

__global__ __launch_bounds__(kJoinWaves * 64) void k_join_scatter(
    const uint8_t* __restrict__ u8, int64_t total, const uint64_t* __restrict__ body, const uint64_t* __restrict__ head,
    const int64_t* __restrict__ tile_rank, const int64_t* __restrict__ tile_cnt, const uint16_t* __restrict__ word_pref,
    int64_t n_words, const int64_t* __restrict__ row_off, int64_t n_str, int sep, uint8_t* __restrict__ out, int64_t cap,
    const int64_t* __restrict__ n_items_dev, int64_t* __restrict__ out_off, int* __restrict__ err, unsigned n_tile_blocks) {
    if (blockIdx.x >= n_tile_blocks) {   // role 2: one thread per row offset (and the end of the batch)
        const int64_t s = (int64_t)(blockIdx.x - n_tile_blocks) * (kJoinWaves * 64) + threadIdx.x;
        if (s > n_str) return;
        const int64_t n = *n_items_dev;
        const int64_t p = row_off[s];
        int64_t rank = n;
        if (p < total) {
            const int64_t w = p >> 6;
            const uint64_t lm = low_mask((int)(p & 63));
            rank = tile_rank[w >> 6] + word_pref[w] + __popcll(body[w] & lm) + __popcll(head[w] & lm);
        }
        out_off[s] = rank;
        if (s == 0 && n > cap) *err = *err | 4;   // (plain stores: the flag may live in pinned host memory)
        return;
    }
    // role 1: one wave per tile.  The caller's buffer holds `cap` bytes; when the batch needs more, nothing is written.
    if (*n_items_dev > cap) return;
    __shared__ __attribute__((aligned(16))) uint8_t win_s[kJoinWaves][kJoinWin];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t t = (int64_t)blockIdx.x * kJoinWaves + wave;
    const int64_t w0 = t * 64;
    if (w0 >= n_words) return;                                      // whole wave
    const int n_wave = (int)tile_cnt[t];
    if (n_wave == 0) return;
    const int64_t w = w0 + lane;
    const bool in = w < n_words;
    const uint64_t bodyw = in ? body[w] : 0ull, headw = in ? head[w] : 0ull;
    const int pref = in ? (int)word_pref[w] : 0;
    uint8_t* dst = out + tile_rank[t];
    const int a = (int)((uintptr_t)dst & 3u);                       // window byte j <-> dst - a + j: dwords of the two coincide
    uint8_t* win = win_s[wave];
    const int64_t t0 = w0 << 6;
    const int sh = (lane & 15) * 4;
    const uint64_t below = low_mask(sh);
    // 256 bytes per round, one dword per lane: coalesced loads; the owner word's planes and prefix arrive through shuffles
    for (int rd = 0; rd < 16; ++rd) {
        const int src = 4 * rd + (lane >> 4);
        const uint64_t bq = __shfl(bodyw, src), hq = __shfl(headw, src);
        const int pq = __shfl(pref, src);
        const unsigned bn = (unsigned)(bq >> sh) & 15u, hn = (unsigned)(hq >> sh) & 15u;   // (head bits are body bits)
        if (__ballot(bn != 0u) == 0ull) continue;                   // (wave-uniform) 256 bytes of whitespace
        if (bn != 0u) {
            const int64_t p = t0 + 256 * rd + 4 * lane;
            uint32_t d = 0;
            if (p + 4 <= total) {
                d = *reinterpret_cast<const uint32_t*>(u8 + p);
            } else {
                for (int k = 0; k < 4; ++k)
                    if (p + k < total) d |= (uint32_t)u8[p + k] << (8 * k);
            }
            int pos = a + pq + __popcll(bq & below) + __popcll(hq & below);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if ((hn >> k) & 1u) win[pos++] = (uint8_t)sep;
                if ((bn >> k) & 1u) win[pos++] = (uint8_t)(d >> (8 * k));
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // the run [a, a + n_wave) of the window: whole dwords, the ragged <= 3 bytes at each end as bytes -- one writer per byte
    const int lo = a, hi = a + n_wave;
    uint8_t* base = dst - a;
    const int d0 = (lo + 3) & ~3, d1 = hi & ~3;
    if (d0 >= d1) {
        if (lo + lane < hi) base[lo + lane] = win[lo + lane];
    } else {
        if (lo + lane < d0) base[lo + lane] = win[lo + lane];
        for (int j = d0 + 4 * lane; j < d1; j += 256)
            __builtin_nontemporal_store(*reinterpret_cast<const uint32_t*>(win + j), reinterpret_cast<uint32_t*>(base + j));
        if (d1 + lane < hi) base[d1 + lane] = win[d1 + lane];
    }
}

hipError_t launch_join_counts(const uint64_t* bits, const uint64_t* space, int64_t n_words, int64_t total, const int64_t* row_off,
                              int64_t n_str, const int64_t* tile_first, uint64_t* body, uint64_t* head, int64_t* tile_cnt,
                              uint16_t* word_pref, hipStream_t st) {
    if (n_words <= 0) return hipSuccess;
    const int64_t n_tiles = (n_words + 63) / 64;
    hipLaunchKernelGGL(k_join_counts, dim3((unsigned)((n_tiles + kJoinWaves - 1) / kJoinWaves)), dim3(kJoinWaves * 64), 0, st, bits, space,
                       n_words, total, row_off, n_str, tile_first, body, head, tile_cnt, word_pref);
    return hipGetLastError();
}

// out == NULL: the row offsets only (a size query)
hipError_t launch_join_scatter(const uint8_t* u8, int64_t total, const uint64_t* body, const uint64_t* head, const int64_t* tile_rank,
                               const int64_t* tile_cnt, const uint16_t* word_pref, int64_t n_words, const int64_t* row_off,
                               int64_t n_str, int sep, uint8_t* out, int64_t cap, const int64_t* n_items_dev, int64_t* out_off,
                               int* err, hipStream_t st) {
    if (n_words <= 0) return hipSuccess;
    const int64_t n_tiles = (n_words + 63) / 64;
    const unsigned nb_tiles = out ? (unsigned)((n_tiles + kJoinWaves - 1) / kJoinWaves) : 0u;
    const unsigned nb_rows = (unsigned)((n_str + 1 + kJoinWaves * 64 - 1) / (kJoinWaves * 64));
    hipLaunchKernelGGL(k_join_scatter, dim3(nb_tiles + nb_rows), dim3(kJoinWaves * 64), 0, st, u8, total, body, head, tile_rank, tile_cnt,
                       word_pref, n_words, row_off, n_str, sep, out, cap, n_items_dev, out_off, err, nb_tiles);
    return hipGetLastError();
}

// ---- launchers -----------------------------------------------------------------------------------------------------
int64_t scan_chunk() { return kChainChunk; }
int chain_lookback() { return 64; }   // one predecessor per lane of the look-back wave
int chain_value_bits() { return kChainValueBits; }
int chain_epoch_bits() { return 64 - kChainEpochShift; }
int64_t count_blocks(int64_t n_words) { return n_words > 0 ? ((n_words + 63) / 64 + kChainChunk - 1) / kChainChunk : 0; }

// exclusive scan of per-tile counts that some other kernel left (the byte-space tile kernel: leads per tile): k_scan_chained alone
hipError_t launch_tile_scan(const int64_t* tile_cnt, int64_t n_tiles, int64_t* tile_rank, const ChainState& c, int64_t* total_dev,
                            int64_t* total_host, int* err, hipStream_t st, const int64_t* units_dev) {
    if (n_tiles <= 0) return hipSuccess;
    const unsigned n_blocks = (unsigned)((n_tiles + kChainChunk - 1) / kChainChunk);
    hipLaunchKernelGGL(k_scan_chained, dim3(n_blocks), dim3(kChainBlock), 0, st, tile_cnt, n_tiles, tile_rank, c.chain, c.ticket, c.epoch,
                       n_blocks, total_dev, total_host, err, units_dev);
    return hipGetLastError();
}

// the planes' one writer: p's item mask (spans: the kept mask), tile counts, word prefixes, tile ranks and *p.n_items are its outputs
hipError_t launch_word_counts_scan(bool spans, const TokenPlanes& p, const ChainState& c, int64_t* total_host, int* err, hipStream_t st,
                                   DeviceTotal dt) {
    if (p.n_words <= 0) return hipSuccess;
    const int64_t n_tiles = (p.n_words + 63) / 64;
    const dim3 grid((unsigned)((n_tiles + 3) / 4)), block(256);
    uint64_t* kept = spans ? const_cast<uint64_t*>(p.item_mask) : nullptr;
    int64_t* tile_cnt = const_cast<int64_t*>(p.tile_cnt);
    uint16_t* word_pref = const_cast<uint16_t*>(p.word_pref);
    if (spans) hipLaunchKernelGGL((k_word_counts<true>), grid, block, 0, st, p.bits, p.space, p.n_words, p.total, kept, tile_cnt, word_pref, dt.total);
    else hipLaunchKernelGGL((k_word_counts<false>), grid, block, 0, st, p.bits, p.space, p.n_words, p.total, kept, tile_cnt, word_pref, dt.total);
    const unsigned n_blocks = (unsigned)count_blocks(p.n_words);
    hipLaunchKernelGGL(k_scan_chained, dim3(n_blocks), dim3(kChainBlock), 0, st, p.tile_cnt, n_tiles, const_cast<int64_t*>(p.tile_rank), c.chain,
                       c.ticket, c.epoch, n_blocks, const_cast<int64_t*>(p.n_items), total_host, err, dt.total);
    return hipGetLastError();
}

hipError_t launch_string_counts(bool out32, const TokenPlanes& p, void* counts, int* err, hipStream_t st, DeviceTotal dt) {
    if (p.n_str <= 0) return hipSuccess;
    const dim3 grid((unsigned)((p.n_str + 255) / 256)), block(256);
    if (out32)
        hipLaunchKernelGGL((k_string_counts<int32_t>), grid, block, 0, st, p.item_mask, p.tile_rank, p.word_pref, p.row_off, p.n_str, p.total,
                           p.n_items, (int32_t*)counts, err, dt.total);
    else
        hipLaunchKernelGGL((k_string_counts<int64_t>), grid, block, 0, st, p.item_mask, p.tile_rank, p.word_pref, p.row_off, p.n_str, p.total,
                           p.n_items, (int64_t*)counts, err, dt.total);
    return hipGetLastError();
}

// The grid of every scatter launch, two block roles: one wave per tile only if there is a payload to write, then one thread per string
// only if counts are asked for; nothing is launched for neither.  launch(OUT{}, grid, block, nb_scatter) enqueues the kernel for
// records and counts of type OUT.
template <class Launch>
static hipError_t launch_scatter(bool out32, const TokenPlanes& p, bool payload, bool counts, Launch launch) {
    if (p.n_words <= 0) return hipSuccess;
    constexpr int kThreads = kScatterWaves * 64;
    const unsigned nb_scatter = payload ? (unsigned)((p.n_words + kThreads - 1) / kThreads) : 0u;
    const unsigned nb_counts = counts ? (unsigned)((p.n_str + kThreads - 1) / kThreads) : 0u;
    if (nb_scatter + nb_counts == 0) return hipSuccess;
    const dim3 grid(nb_scatter + nb_counts), block(kThreads);
    if (out32) launch(int32_t{}, grid, block, nb_scatter);
    else launch(int64_t{}, grid, block, nb_scatter);
    return hipGetLastError();
}
// the positional arguments that k_counts_scatter, k_hash_scatter and k_vocab_scatter share, then each kernel's own
template <class Kernel, typename OUT, class... Own>
static void launch_positional(Kernel kernel, dim3 grid, dim3 block, hipStream_t st, const TokenPlanes& p, OUT* out, int64_t cap, OUT* counts,
                              unsigned nb_scatter, int* err, Own... own) {
    hipLaunchKernelGGL(kernel, grid, block, 0, st, p.bits, p.space, p.item_mask, p.tile_rank, p.tile_cnt, p.word_pref, p.n_words, p.total, p.row_off,
                       p.n_str, p.tile_first, out, p.n_items, cap, counts, nb_scatter, err, own...);
}

// counts (may be NULL: already written) and / or items (out may be NULL: counts only) in one launch
hipError_t launch_counts_scatter(int kind, bool out32, const TokenPlanes& p, void* out, int64_t cap, void* counts, int* err, hipStream_t st,
                                 DoneSignal done, DeviceTotal dt) {
    return launch_scatter(out32, p, out, counts, [&](auto t, dim3 grid, dim3 block, unsigned nb) {
        using OUT = decltype(t);
        const auto kernel = kind == 0 ? k_counts_scatter<0, OUT> : kind == 2 ? k_counts_scatter<2, OUT> : k_counts_scatter<1, OUT>;
        launch_positional(kernel, grid, block, st, p, (OUT*)out, cap, (OUT*)counts, nb, err, done, dt);
    });
}

// token hashes (+ the span records if out != NULL, + the counts if counts != NULL); hashes == NULL: counts only (a size query)
hipError_t launch_hash_scatter(bool out32, const TokenPlanes& p, const uint8_t* u8, uint32_t seed, void* out, uint32_t* hashes, int64_t cap,
                               void* counts, int* err, hipStream_t st) {
    HashArgs ha;
    ha.text = reinterpret_cast<const uint32_t*>(u8);
    ha.hashes = hashes;
    ha.seed = seed;
    return launch_scatter(out32, p, hashes, counts, [&](auto t, dim3 grid, dim3 block, unsigned nb) {
        using OUT = decltype(t);
        launch_positional(k_hash_scatter<OUT>, grid, block, st, p, (OUT*)out, cap, (OUT*)counts, nb, err, ha);
    });
}

static VocabArgs vocab_args(const VocabTable& vt, int32_t* ids, int32_t unk_id) {
    VocabArgs va;
    va.slots = reinterpret_cast<const VtSlot*>(vt.slots);
    va.blob = vt.blob;
    va.n_slots = vt.n_slots;
    va.ids = ids;
    va.unk = unk_id;
    return va;
}
// token ids (+ the span records if out != NULL, + the counts if counts != NULL); ids == NULL: counts only (a size query)
hipError_t launch_vocab_scatter(bool out32, const TokenPlanes& p, const uint8_t* u8, const VocabTable& vt, int32_t unk_id, void* out,
                                int32_t* ids, int64_t cap, void* counts, int* err, hipStream_t st) {
    HashArgs ha;
    ha.text = reinterpret_cast<const uint32_t*>(u8);
    ha.seed = vt.seed;
    const VocabArgs va = vocab_args(vt, ids, unk_id);
    return launch_scatter(out32, p, ids, counts, [&](auto t, dim3 grid, dim3 block, unsigned nb) {
        using OUT = decltype(t);
        launch_positional(k_vocab_scatter<OUT>, grid, block, st, p, (OUT*)out, cap, (OUT*)counts, nb, err, ha, va);
    });
}

// token counts: every token of the batch found or entered in the counting table and counted; no output but the table
hipError_t launch_count_scatter(const TokenPlanes& p, const uint8_t* u8, const CountTable& ct, int* err, hipStream_t st) {
    CountScatterArgs a{};
    a.p = p;
    a.err = err;
    a.ha.text = reinterpret_cast<const uint32_t*>(u8);
    a.ha.seed = ct.seed;
    a.ca.slots = ct.slots;
    a.ca.counts = ct.counts;
    a.ca.blob = ct.blob;
    a.ca.n_slots = ct.n_slots;
    a.ca.tally = ct.tally;
    a.ca.max_word_bytes = ct.max_word_bytes;
    return launch_scatter(true, p, true, false, [&](auto, dim3 grid, dim3 block, unsigned nb) {
        a.n_scatter_blocks = nb;
        hipLaunchKernelGGL(k_count_scatter, grid, block, 0, st, a);
    });
}
// term keys: keys[rank] of every token and the int64 token count of every string
hipError_t launch_term_scatter(const TokenPlanes& p, const uint8_t* u8, const TermKeyForm& form, uint64_t* keys, int64_t* counts, int* err,
                               hipStream_t st) {
    TermScatterArgs a{};
    a.p = p;
    a.counts = counts;
    a.err = err;
    a.ha.text = reinterpret_cast<const uint32_t*>(u8);
    a.ha.seed = form.seed;
    if (form.vocab) a.va = vocab_args(form.vt, nullptr, 0);
    a.ta.keys = keys;
    a.ta.n_features = form.n_features;
    a.ta.alternate_sign = form.alternate_sign;
    return launch_scatter(false, p, true, counts, [&](auto, dim3 grid, dim3 block, unsigned nb) {
        a.n_scatter_blocks = nb;
        hipLaunchKernelGGL(k_term_scatter, grid, block, 0, st, a);
    });
}

hipError_t launch_count_commit_sum(const CountTable& ct, hipStream_t st) {
    hipLaunchKernelGGL(k_count_commit_sum, dim3((unsigned)((ct.n_slots + kCommitBlock - 1) / kCommitBlock)), dim3(kCommitBlock), 0, st, ct.slots,
                       ct.n_slots, ct.ctl);
    return hipGetLastError();
}
hipError_t launch_count_commit_copy(const uint8_t* u8, const CountTable& ct, hipStream_t st) {
    hipLaunchKernelGGL(k_count_commit_copy, dim3((unsigned)((ct.n_slots + kCommitBlock - 1) / kCommitBlock)), dim3(kCommitBlock), 0, st, ct.slots,
                       ct.n_slots, reinterpret_cast<const uint32_t*>(u8), ct.blob, ct.blob_dwords, ct.ctl);
    return hipGetLastError();
}

}  // namespace latok
