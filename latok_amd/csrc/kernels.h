// kernels.h -- constants, parameter blocks and launcher prototypes shared by the .hip kernel files and api.cpp.
#ifndef LATOK_KERNELS_H
#define LATOK_KERNELS_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "detok.h"
#include "fold_map.h"
#include "split_code.h"

namespace latok {

// ---- geometry ------------------------------------------------------------------------------------------------
constexpr int kTile = 4096;              // chars per tile = 64 lanes x 64-bit words (== LATOK_TILE_CHARS)
constexpr int kTblShift = 7;             // stage-2 block = 128 code points
constexpr int kStage1Len = 8705;         // 0x110000 >> 7, + 1 entry for cp >= 0x110000
constexpr int kStage1Pad = 8720;         // padded to 16 B
constexpr int kStage2Len = 255 * 128;    // 32640, multiple of 16
constexpr int kTablesLdsBytes = kStage1Pad + kStage2Len;   // 41360
// byte space (kModeBytes): [stage 1: uint16 block offsets, by cp >> 6 | stage 2: 64-entry blocks] (split_code.h: LK_B6_*)
constexpr int kB6Stage1Len = LK_B6_STAGE1_LEN;                       // 17409
constexpr int kB6Stage1Bytes = (kB6Stage1Len * 2 + 1023) / 1024 * 1024;   // 35840: whole 1 KiB pieces (one wave instruction of the on-demand copy each)
constexpr int kB6MaxBlocks = 400;                                    // distinct 64-char blocks: 354 (split codes) / 394 (rule codes)
constexpr int kB6Stage2Bytes = kB6MaxBlocks * 64;                    // 25600, whole 1 KiB pieces as well
constexpr int kB6TablesBytes = kB6Stage1Bytes + kB6Stage2Bytes;
static_assert(kB6Stage1Bytes % 1024 == 0 && kB6Stage2Bytes % 1024 == 0 && kB6Stage1Bytes <= kTablesLdsBytes, "byte space keeps its stage 1 where the other modes keep both stages");
constexpr int kStageBytes = 64 * 80;     // 64 rows of 64 code bytes + 16 B pad (conflict-free ds_read_b128)
constexpr int kWaveLdsBytes = kStageBytes + 16 + 65 * 8 + 8;  // staging + halo + string-start words = 5664

constexpr int kModeBits = 0;
constexpr int kModeValues = 1;
constexpr int kModeBlockMask = 2;        // compat _gen_block_mask: planes from caller byte arrays, byte mask out
constexpr int kModeRules = 3;            // kModeBits with caller-supplied C_SPLIT / C_MASK / C_SYM (SplitParams::rules)
constexpr int kModeBytes = 4;            // kModeBits in BYTE space: input = UTF-8 bytes (SplitParams::u8), row_off = byte
                                         // offsets, bit i of the mask = byte i (set at the lead byte of a boundary char)
constexpr int kModeLatin1 = 5;           // kModeBits on PEP 393 kind-1 input: SplitParams::u8 = one BYTE per char (U+0000..U+00FF)
constexpr int kModeUcs2 = 6;             // kModeBits on PEP 393 kind-2 input: SplitParams::u8 = one uint16 per char
// modes whose input is SplitParams::u8 and whose tiles use the byte-space LDS layout (pads, 16-byte halo)
// the same four input forms / outputs with caller-supplied C_SPLIT / C_MASK / C_SYM (SplitParams::rules; t2 = rule codes):
// kModeRules is kModeBits + tables; these are the others
constexpr int kModeBytesRules = 7;       // kModeBytes + run-time rule tables
constexpr int kModeLatin1Rules = 8;      // kModeLatin1 + run-time rule tables
constexpr int kModeUcs2Rules = 9;        // kModeUcs2 + run-time rule tables
constexpr int kModeValuesRules = 10;     // kModeValues + run-time rule tables: what gen_split_mask returns for any tables
                                         // (default_tokenizer.py:121-132): rows(C_SPLIT) * mask + rows(C_SYM), string start = 1
// input / output form of a mode, and whether the rules are interpreted at run time
constexpr int mode_base(int mode) {
    return mode == kModeRules ? kModeBits : mode == kModeBytesRules ? kModeBytes : mode == kModeLatin1Rules ? kModeLatin1
         : mode == kModeUcs2Rules ? kModeUcs2 : mode == kModeValuesRules ? kModeValues : mode;
}
constexpr bool mode_rules(int mode) { return mode != mode_base(mode); }
constexpr int mode_with_rules(int base) {
    return base == kModeBits ? kModeRules : base == kModeBytes ? kModeBytesRules : base == kModeLatin1 ? kModeLatin1Rules
         : base == kModeUcs2 ? kModeUcs2Rules : base == kModeValues ? kModeValuesRules : base;
}
constexpr bool mode_is_bytes(int mode) { return mode_base(mode) == kModeBytes || mode_base(mode) == kModeLatin1 || mode_base(mode) == kModeUcs2; }
constexpr bool mode_is_units(int mode) { return mode_base(mode) == kModeLatin1 || mode_base(mode) == kModeUcs2; }
constexpr bool mode_writes_bits(int mode) { return mode_base(mode) == kModeBits || mode_is_bytes(mode); }

constexpr long long kNegInf64 = -(1ll << 60);
constexpr int kWPB = 12;                 // waves per workgroup: 768 threads -> 168 VGPRs per lane, one workgroup per CU
constexpr int kSegMax = kWPB * 64;       // tiles per segment = threads of the block-wide scans
// k_tiles_main<.., HOLD> (UTF-32 bitmask modes): a segment of at most kSegHoldTiles tiles (kSegHoldRounds tiles per wave) stores its mask
// words as one contiguous run at its end; the words of a wave's first kSegHoldLdsRounds tiles wait in LDS, the others in its
// registers (split_kernels.hip: run_segment).  latok_debug_tile_limits reports them.
constexpr int kSegHoldRounds = 12;
constexpr int kSegHoldTiles = kSegHoldRounds * kWPB;   // 144
constexpr int kSegHoldLdsRounds = 4;

struct Fn64 {        // q transfer function of a run of tiles: f(q) = max(q + a, b); a <= kNegInf64 means constant b
    long long a, b;
};
struct Hd64 {        // head descriptor of a run of tiles: starts before its first closing event, and whether it has one
    long long h;
    int c;
};

// Completion word of a multi-workgroup launch whose outputs land in pinned host memory (small / mid-size host batches): every
// workgroup drains its stores to system scope and counts itself in; the last one stores `seq` into `word` (which the host
// polls instead of waiting for the stream) and resets the counter.  word == NULL: off.
struct DoneSignal {
    unsigned long long* word;
    unsigned long long seq;
    unsigned* counter;     // device memory, 0 between launches
};
#if defined(__HIPCC__)
__device__ __forceinline__ void signal_block_done(const DoneSignal& d) {
    if (!d.word) return;
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned n = gridDim.x;
        // acq_rel at agent scope: the last workgroup's increment synchronises with every earlier workgroup's, so their
        // (system-fenced) output stores happen-before the word store below -- not only by posted-write ordering
        if (__hip_atomic_fetch_add(d.counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == n - 1u) {
            *d.counter = 0u;
            __threadfence_system();
            __hip_atomic_store(d.word, d.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}
#endif

struct SplitParams {
    const uint32_t* cps;        // packed UTF-32 code points (16-byte aligned)
    const uint8_t* u8;          // kModeBytes: packed UTF-8 bytes instead (16-byte aligned); kModeLatin1 / kModeUcs2: the code units; cps is unused
    const int64_t* row_off;     // [n_str + 1]
    int64_t n_str, total, n_tiles;
    int seg_tiles;              // tiles per segment (kWPB..kSegMax, see plan_segments)
    int64_t n_segs;             // ceil(n_tiles / seg_tiles)
    const uint8_t* t1;          // stage-1 table in global memory (kStage1Pad bytes; kModeBytes: kB6Stage1Bytes of uint16 block offsets)
    const uint8_t* t2;          // stage-2 split codes in global memory (kStage2Len bytes; kModeBytes: kB6Stage2Bytes), behind t1
    uint64_t* bits_out;         // kModeBits
    uint8_t* values_out;        // kModeValues / kModeBlockMask
    uint64_t* space_out;        // optional (kModeBits): SPACE plane as a bitmask, same layout as bits_out (token spans)
    uint64_t* lead_out;         // optional (kModeBytes): bit i = byte i is a LEAD byte (not 10xxxxxx), same layout as bits_out
                                // (code-point results from the byte-space mask: compact_kernels.hip, k_lead_compress)
    uint16_t* lead_pref_out;    // with lead_out: [words] leads of the tile before each word, and
    int64_t* lead_cnt_out;      //                [n_tiles] leads per tile (what k_word_counts would compute from lead_out)
    uint8_t* codes_out;         // optional (kModeBits / kModeRules on UTF-32 input, t2 = rule codes): the code byte of every char
                                // (featurize: k_features_tiles reads 1 B/char instead of classifying 4 B/char again)
    int64_t* tile_first;        // [n_tiles]: first string that starts at or after each tile's first char (k_tile_index; also read by the compaction passes)
    int4* summ;                 // [n_tiles] {a, b, head_starts, has_closing | edge-block geometry}
    Fn64* seg_fn;               // [n_segs] segment aggregates
    Hd64* seg_hd;               // [n_segs]
    int64_t* fix_count;         // [1] statistics: tiles recomputed by the resolve stage
    // kModeBlockMask only
    const int8_t* bm_a1;        // "starts" bytes [total]
    const int8_t* bm_a2;        // "spaces" bytes [total]
    const int* bm_flags;        // {any(a1), any(a2)}
    DoneSignal done;            // last launch of a host-pointer call on pinned memory (k_one_segment / k_resolve_fix): completion word
    // kModeRules only (t2 then points at the rule-code table)
    lk_rule_tables rules;
};


// A batch whose size only the device knows when its launches are enqueued (code-point results of a UTF-8 batch in a flow: the
// code-point total is the result of the lead-byte scan).  total: the word that holds it, written earlier on the same stream; the
// launch's own size arguments are then an UPPER BOUND (a batch has at most one char per byte) that sizes grids and buffers, and
// tiles, words and strings behind the real size do no work.  gate: a word that is nonzero when the batch was found malformed --
// the records and feature sums of such a batch are not written.  {NULL, NULL}: the host's size is the size.
struct DeviceTotal {
    const int64_t* total;
    const int* gate;
};
#if defined(__HIPCC__)
// the size a kernel works with: the device's word, held inside [0, bound] -- the buffers were sized by the bound, so whatever the
// word holds (a scan that ended with its error flag raised leaves anything) no access leaves them
__device__ __forceinline__ int64_t device_total(const int64_t* p, int64_t bound) {
    const int64_t t = *p;
    return t < 0 ? 0 : (t > bound ? bound : t);
}
#endif

// The read view of a scanned batch: the two bitmasks of the tile kernel and what k_word_counts + k_scan_chained leave over them.
// Every consumer of the token scatter and k_string_counts read a batch through this record (k_features_tiles: through FeatParams,
// which the host fills from it); launch_word_counts_scan is its one writer (the item mask where it is the kept mask, the tile counts,
// the word prefixes, the tile ranks and *n_items).
// The field order is the kernel-argument layout of k_count_scatter and k_term_scatter.
struct TokenPlanes {
    const uint64_t* bits;         // final boundary bitmask (bit i = packed unit i)
    const uint64_t* space;        // SPACE bitmask (NULL: offsets); only walked for tokens that span more than two words
    const uint64_t* item_mask;    // the items: every boundary (offsets) or the boundaries whose token is kept (k_word_counts<true>)
    const int64_t* tile_rank;     // index of a tile's first item (exclusive scan of the per-tile item counts)
    const int64_t* tile_cnt;      // items per tile
    const uint16_t* word_pref;    // items of the tile before each word
    int64_t n_words, total;       // 64-bit words of one plane, units of the batch (an upper bound under a DeviceTotal)
    const int64_t* row_off;       // [n_str + 1]
    int64_t n_str;
    const int64_t* tile_first;    // per tile: first string that starts at or after its first unit (NULL: searched)
    const int64_t* n_items;       // device: the item total of the batch (k_scan_chained)
};
// The state of one chained scan (k_scan_chained): the published words, the ticket counter and the launch's epoch.
struct ChainState {
    unsigned long long* chain;
    unsigned* ticket;
    unsigned epoch;
};

// featurize on the tile grid (feature_kernels.hip: k_features_tiles)
struct FeatParams {
    const uint8_t* codes;         // rule code of every char (SplitParams::codes_out of the tile kernel), padded by one tile + 256 B
    const int64_t* row_off;
    int64_t n_str, total, n_tiles;
    const uint64_t* bits;         // final boundary bitmask
    const uint64_t* kept;         // boundaries whose token is kept (k_word_counts<true>)
    const int64_t* tile_rank;     // index of a tile's first token (exclusive scan of the per-tile token counts)
    const int64_t* tile_cnt;      // tokens per tile
    const uint16_t* word_pref;    // tokens of the tile before each word
    const int64_t* tile_first;    // per tile: first string that starts at or after its first char
    const uint64_t* space;        // SPACE bitmask (only walked for tokens that span more than two words)
    int8_t* features;             // [n_tokens][25]
    void* spans4;                 // [n_tokens][4] = {raw start, raw end, stripped start, stripped end}, string relative; int64 or int32
                                  // NULL: no span records, only the sums (UTF-8 in byte space: launch_counts_scatter kind 2 writes them)
    bool out32;                   // spans4 holds int32
    const int64_t* n_tokens_dev;  // device: total tokens of the batch (k_word_counts_scan) ...
    int64_t cap;                  // ... nothing is written when it exceeds the caller's capacity
    DoneSignal done;
    DeviceTotal dt;               // total / n_tiles above are an upper bound when dt.total is set
};
hipError_t launch_features_tiles(const FeatParams& P, int n_cu, hipStream_t st);

void plan_segments(int64_t n_tiles, int n_cu, int* seg_tiles, int64_t* n_segs);
// the three stages in one launch of one workgroup: batches of at most kOneSegTiles tiles planned as ONE segment
// (P.n_segs = 1, P.seg_tiles >= P.n_tiles), UTF-32 bitmask modes (kModeBits / kModeRules)
constexpr int64_t kOneSegTiles = 24;
constexpr int64_t kFastTailTiles = 256;   // k_tiles_main<.., FAST_TAIL>: batches of at most ~1 M chars (beyond, one tile's latency is noise)
constexpr int kNarrowWPB = 16;            // Latin-1 / UCS-2 tile kernels: 4 waves per SIMD (<= 128 VGPRs)
constexpr int kCpsPrefetchRows = 2;       // rows (1 KiB) of the wave's next UTF-32 tile requested before phase 2 of the current one
constexpr int kCpsPrefetchRowsFlow = 6;   // the same in a batch of a flow (tile_core.h)
// What the tile pipeline launches for a batch: the segment plan and the kernel variants.  plan_launch is the only place
// that decides it; run_pipeline launches what it says and the test hooks (latok_debug_plan / _last_plan) report it.
struct LaunchPlan {
    int n_cu_eff;        // CUs the segments are planned for (a batch of a flow: its share of the chip)
    int seg_tiles;
    int64_t n_segs;
    int64_t rounds;      // segments the busiest workgroup walks
    int grid;            // workgroups of k_tiles_main and k_resolve_fix (k_one_segment: 1)
    int fast_tail;       // k_tiles_main<MODE, FAST_TAIL = true>
    int pf;              // rows of the next UTF-32 tile prefetched (k_tiles_main's PF)
    int wpb;             // waves per workgroup of the tile kernel
    int nw;              // waves per workgroup of the resolve stage: nw * 64 >= seg_tiles
    int one_launch;      // k_one_segment: the three stages in one launch
    int hold;            // k_tiles_main<.., HOLD>: a segment's mask words leave as one run (UTF-32 bitmask modes, seg_tiles <= kSegHoldTiles)
};
// test hook (latok_debug_set_tile_plan): what plan_launch decides by itself unless told otherwise -- the segment length (0 = the
// plan's own; a forced length also rules the one-launch path out), the most workgroups (0 = the plan's own) and whether short
// segments are held (-1 = the plan's own, 0 = never)
struct PlanForce {
    int seg_tiles = 0, grid = 0, hold = -1;
};
// n_cu: CUs of the device (or the context's test cap); one_launch_ok: the call may take k_one_segment (all three stages,
// no timing events between them)
void plan_launch(int64_t n_tiles, int n_cu, bool in_flow, int mode, bool one_launch_ok, LaunchPlan* L, const PlanForce* force = nullptr);
hipError_t launch_tile_index(const SplitParams& P, hipStream_t st);   // stage 0: P.tile_first (must be set)
hipError_t launch_split_tiles(const SplitParams& P, int mode, const LaunchPlan& L, hipStream_t st);
hipError_t launch_resolve_fix(const SplitParams& P, int mode, const LaunchPlan& L, hipStream_t st);
hipError_t launch_one_segment(const SplitParams& P, int mode, hipStream_t st);
// batches of at most one tile, everything in one launch (split_kernels.hip: k_small_batch); P.t1 / P.t2 / P.rules / P.cps /
// P.row_off / P.n_str / P.total must be set, kind 0 = offsets, 1 = token spans.  done (or NULL): a pinned host word that
// receives seq once every output is visible to the host.
// kind 2 = featurize: items = [n_items][4] span records, features = [n_items][25] sums
hipError_t launch_small_batch(const SplitParams& P, bool rules, int kind, bool out32, void* counts, void* items, int8_t* features,
                              int64_t* n_items, unsigned long long* done, unsigned long long seq, hipStream_t st);
hipError_t launch_any_nonzero(const int8_t* a1, const int8_t* a2, int64_t n, int* flags, hipStream_t st);

// aux_kernels.hip
hipError_t launch_parse_matrix(const uint32_t* cps, int64_t n, const uint8_t* t1, const uint8_t* t2cls,
                               const uint16_t* cw, int8_t* out, hipStream_t st);
// one string of at most kSmallMatrixChars chars in pinned memory: one workgroup; done (or NULL) receives seq after the last store
constexpr int kSmallMatrixChars = 4096;
hipError_t launch_parse_matrix_small(const uint32_t* cps, int n, const uint8_t* t1, const uint8_t* t2cls, const uint16_t* cw,
                                     int8_t* out, unsigned long long* done, unsigned long long seq, hipStream_t st);
// done != NULL: one workgroup, which stores seq into *done after its last output (small arrays in pinned memory)
hipError_t launch_combine_rows(const uint8_t* m, int64_t stride_r, int64_t stride_c, int64_t cols, const int8_t* idx,
                               int idx_ndim, int irows, int icols, int8_t* out, hipStream_t st,
                               unsigned long long* done = nullptr, unsigned long long seq = 0);
// _gen_block_mask of one array pair of at most kTile elements (P.bm_a1 / bm_a2 / values_out / row_off = {0, n} in pinned
// memory, P.total = n): one single-wave launch
hipError_t launch_small_block_mask(const SplitParams& P, unsigned long long* done, unsigned long long seq, hipStream_t st);
hipError_t launch_rebase_rows(int64_t* row, int64_t n, int64_t base, hipStream_t st);
int64_t scan_blocks(int64_t n);   // entries the caller must provide in `block_tot`
hipError_t launch_exclusive_scan(const int64_t* in, int64_t n, int64_t* out, int64_t* total, int64_t* block_tot,
                                 hipStream_t st, int64_t* total_host = nullptr);
// compact_kernels.hip: word-parallel compaction (offsets / token spans / featurize spans)
int64_t count_blocks(int64_t n_words);   // workgroups of launch_word_counts_scan = entries of its `chain` state
int64_t scan_chunk();                  // kChainChunk: entries one workgroup of the chained scan takes (latok_debug_wordpiece_limits)
// the chained scan's other constants (latok_debug_scan_limits): predecessors one look-back round reads, bits of a published word's
// value field (a scan's total must stay below 2^bits: the field wraps silently) and bits of its launch epoch
int chain_lookback();
int chain_value_bits();
int chain_epoch_bits();
hipError_t launch_word_counts_scan(bool spans, const TokenPlanes& p, const ChainState& c, int64_t* total_host, int* err, hipStream_t st,
                                   DeviceTotal dt = DeviceTotal{nullptr, nullptr});
hipError_t launch_string_counts(bool out32, const TokenPlanes& p, void* counts, int* err, hipStream_t st,
                                DeviceTotal dt = DeviceTotal{nullptr, nullptr});
// kind 0 = offsets, 1 = stripped token spans, 2 = featurize's 4-field span records {raw start, raw end, stripped start, stripped end}
hipError_t launch_counts_scatter(int kind, bool out32, const TokenPlanes& p, void* out, int64_t cap, void* counts, int* err, hipStream_t st,
                                 DoneSignal done = DoneSignal{nullptr, 0, nullptr}, DeviceTotal dt = DeviceTotal{nullptr, nullptr});
// k_features_tiles (feature_kernels.hip, where the measurements behind these values are told); latok_debug_limits reports them
constexpr int kFeatWaves = 7;                                         // (6 -> 7: C2 -4.5 %, C3 -6 %; 8 would need rounds of < 800 tokens: two rounds per C2 tile)
constexpr int kFeatRound = 896;                                       // tokens per round (word-major form)
constexpr int kFeatRec = 25;                                          // packed records in the window, as in the output
constexpr int kFeatRoundTm = 768;                                     // token-major form: records + 2-byte (lane, bit) codes share the window
constexpr int kFeatWinBytes = kFeatRound * kFeatRec + 16;             // (+ 16: the records start at record_shift(dst); token-major rounds cost nothing extra)
constexpr int kFeatFormThresh = 5;                                    // token-major when maxc * 2 * wm_rounds > ceil(n / 64) * kFeatFormThresh
constexpr int kCompressWaves = 16;   // k_lead_compress: tiles (= waves) per workgroup
// code-point boundary mask + code-point row offsets from the byte-space mask and the lead-byte mask of a UTF-8 batch
// (bmask2 / out_mask2: optionally a second mask -- the SPACE plane -- packed the same way, for token spans in code-point units)
hipError_t launch_lead_compress(const uint64_t* bmask, const uint64_t* bmask2, const uint64_t* lead, const int64_t* tile_rank,
                                const int64_t* tile_cnt, const uint16_t* word_pref, int64_t n_words, int64_t total_bytes,
                                const int64_t* byte_off, int64_t n_str, const int64_t* total_cps_dev, uint64_t* out_mask,
                                uint64_t* out_mask2, int64_t cap_words, int64_t* cp_row_off, int* odd, hipStream_t st);
// the rule code of every char of a UTF-8 batch at its code-point index (codes[tile_rank[t] + word_pref[w] + leads below it]), from
// the bytes, the lead-byte mask and the lead ranks of the byte-space pipeline; tb6rule = the byte-space rule-code table (featurize)
hipError_t launch_lead_codes(const uint8_t* u8, int64_t total_bytes, const uint64_t* lead, const int64_t* tile_rank, const int64_t* tile_cnt,
                             const uint16_t* word_pref, int64_t n_words, const uint8_t* tb6rule, uint8_t* codes, int n_cu, hipStream_t st);
// units_dev (or NULL): the kernel's device-sized form -- ceil(*units_dev / kTile) counts, at most the n_tiles the grid is sized for
hipError_t launch_tile_scan(const int64_t* tile_cnt, int64_t n_tiles, int64_t* tile_rank, const ChainState& c, int64_t* total_dev,
                            int64_t* total_host, int* err, hipStream_t st, const int64_t* units_dev = nullptr);
// joined token text of a UTF-8 batch in byte space (compact_kernels.hip: "joined token text"): the body / head planes with the
// items (output bytes) per word and per tile; then, behind a scan of the tile counts, the output bytes (only if the total
// fits cap; out may be NULL) and out_off[n_str + 1].  *err gets bit 2 (value 4) when the total exceeds cap.
hipError_t launch_join_counts(const uint64_t* bits, const uint64_t* space, int64_t n_words, int64_t total, const int64_t* row_off,
                              int64_t n_str, const int64_t* tile_first, uint64_t* body, uint64_t* head, int64_t* tile_cnt,
                              uint16_t* word_pref, hipStream_t st);
hipError_t launch_join_scatter(const uint8_t* u8, int64_t total, const uint64_t* body, const uint64_t* head, const int64_t* tile_rank,
                               const int64_t* tile_cnt, const uint16_t* word_pref, int64_t n_words, const int64_t* row_off,
                               int64_t n_str, int sep, uint8_t* out, int64_t cap, const int64_t* n_items_dev, int64_t* out_off,
                               int* err, hipStream_t st);
// token hashes of a UTF-8 batch in byte space (compact_kernels.hip: HashTokens): behind k_word_counts<true> + k_scan_chained, the
// per-string counts (counts may be NULL), the two-field span records (out may be NULL) and one MurmurHash3 x86_32 word per token
// at its rank, the last two only if the total fits cap.  A token of more than kHashWaveBytes bytes is hashed by its whole wave.
constexpr int kHashWaveBytes = 256;
hipError_t launch_hash_scatter(bool out32, const TokenPlanes& p, const uint8_t* u8, uint32_t seed, void* out, uint32_t* hashes, int64_t cap,
                               void* counts, int* err, hipStream_t st);
// token ids of a UTF-8 batch in byte space (compact_kernels.hip: IdTokens): launch_hash_scatter's launch with the hash kept in its
// lane and looked up in a vocabulary table (vocab_table.h) -- exact: the hash finds the slot, the bytes decide.  ids[rank] = the
// word's id or unk_id.  The table is device memory, read only.
struct VocabTable {
    const void* slots = nullptr;      // VtSlot[n_slots]
    const uint32_t* blob = nullptr;   // the padded words
    uint64_t n_slots = 0;             // a power of two
    uint32_t seed = 0;
};
hipError_t launch_vocab_scatter(bool out32, const TokenPlanes& p, const uint8_t* u8, const VocabTable& vt, int32_t unk_id, void* out,
                                int32_t* ids, int64_t cap, void* counts, int* err, hipStream_t st);
// token counts of a UTF-8 batch in byte space (compact_kernels.hip: CountTokens): launch_vocab_scatter's launch without outputs; every
// token of at most max_word_bytes bytes is found or entered in a counting table (count_table.h) and counted, exactly.
// kCountProbeMax bounds a probe whatever the table holds: at load <= 0.5 a run of 128 occupied slots has probability about
// 0.82^128 ~ 1e-11 per slot, so the bound never fires on a table sized as documented and keeps a full one from costing n_slots
// loads per token.  kCountAccEntries: entries of a wave's direct-mapped {slot, count} accumulator in LDS (8 bytes each: 4 KiB per
// wave, 38 944 B per workgroup -> 4 workgroups = 16 waves per CU).  A 4096-byte tile holds ~700 tokens of English text, fewer
// than 512 of them distinct, so most of a tile's words own an entry; what conflicts adds to global memory directly.  The cost of
// the flush atomics and the right size are unmeasured.
constexpr int kCountProbeMax = 128;
constexpr int kCountAccEntries = 512;   // a power of two
struct CountTable {
    uint64_t* slots = nullptr;              // uint64[n_slots], 0 = empty
    unsigned long long* counts = nullptr;   // uint64[n_slots]
    uint32_t* blob = nullptr;               // the resident words; dword 0 is reserved
    uint64_t blob_dwords = 0;               // capacity of the blob
    uint64_t n_slots = 0;                   // a power of two, <= 2^31
    uint32_t seed = 0;
    int max_word_bytes = 0;
    unsigned long long* tally = nullptr;    // this call's {counted, long, dropped}
    unsigned long long* ctl = nullptr;      // {fresh dwords of this call, blob cursor, distinct, overflow flag}
};
hipError_t launch_count_scatter(const TokenPlanes& p, const uint8_t* u8, const CountTable& ct, int* err, hipStream_t st);
// the key form of the term family (term_key.h): the lookup in a vocabulary table, or the hashed form (bucket = |h| mod n_features, sign)
struct TermKeyForm {
    bool vocab = false;
    VocabTable vt;                // vocab
    uint32_t seed = 0;            // of the hash: the table's own in the vocabulary form
    uint32_t n_features = 0;      // hashed form (0 in the vocabulary form)
    bool alternate_sign = false;
};
// term keys of a UTF-8 batch in byte space (compact_kernels.hip: TermTokens): launch_vocab_scatter's launch with one term key
// per token at its rank in `keys` and the int64 token count of every string in `counts`.  No records, no capacity.
hipError_t launch_term_scatter(const TokenPlanes& p, const uint8_t* u8, const TermKeyForm& form, uint64_t* keys, int64_t* counts, int* err,
                               hipStream_t st);
// per-string term counts (terms_kernels.hip): the segmented sort-and-reduce of the term keys.  A workgroup owns the rows that start
// in its tile of kTermsTile tokens; a row of more than kTermsRowMax tokens is sorted by a workgroup of its own through `alt`
// (as large as `keys`).  row_start[n_str + 1] = the exclusive scan of the per-string token counts.  launch_terms_reduce leaves
// distinct[row], oov[row] and the row's entries over the row's first keys; launch_terms_emit, behind the scan of distinct[] into
// indptr[] and *nnz_dev, stores indices / data if nnz fits cap; launch_terms_finish types indptr[n_str + 1] and oov[n_str] (may be
// NULL) for the caller.  latok_debug_terms_limits reports the two constants.
constexpr int kTermsTile = 1024;
constexpr int kTermsRowMax = 1024;
hipError_t launch_terms_reduce(uint64_t* keys, uint64_t* alt, const int64_t* row_start, int64_t n_str, int64_t n_tok, bool vocab_form,
                               int64_t* distinct, int64_t* oov, hipStream_t st);
hipError_t launch_terms_emit(const uint64_t* keys, const int64_t* row_start, int64_t n_str, int64_t n_tok, const int64_t* distinct,
                             const int64_t* indptr, const int64_t* nnz_dev, int64_t cap, int32_t* indices, int32_t* data, hipStream_t st);
hipError_t launch_terms_finish(bool out32, const int64_t* indptr, const int64_t* oov, int64_t n_str, void* indptr_out, void* oov_out,
                               hipStream_t st);
// The text of a batch in TOKEN space, what the kernels with one lane per token read (lane_token of block_ops.h): behind kind 1 of
// launch_counts_scatter (the int64 span record of every token at its rank, the int64 token count of every string) and the scan of
// those counts.  Device memory, read only; the host builds it once per call.
struct TokenText {
    const uint32_t* text;       // the UTF-8 bytes as aligned dwords
    int64_t total;              // in bytes
    const int64_t* row_off;     // first byte of every string
    int64_t n_str;
    const int64_t* row_start;   // token space, n_str + 1 entries (row_start[n_str] = the token total)
    const int64_t* tok_spans;   // two string-relative byte offsets per token
    int64_t n_tok;
};
// WordPiece ids (wordpiece_kernels.hip).  launch_wp_count leaves the pieces of every token in cnt[0 .. n_tok) and 0 in cnt[n_tok]; the
// caller scans the n_tok + 1 entries into rank[] (rank[n_tok] = the piece total); launch_wp_emit walks every token again and stores
// ids, and string-relative spans if asked for, at the piece rank, only if the total fits cap; launch_wp_rows types indptr[s] =
// rank[row_start[s]], s = 0 .. n_str.  launch_wp_pad fills an [n_str, max_length] int32 block from the ids: cls (if add_special),
// the first max_length - 2 add_special pieces of the row, sep (if add_special), pad; lengths[s] = cells used.  rank == NULL there:
// a batch without a token, every row is empty.  The tables are device memory, read only.
constexpr int kWpBlock = 256;   // tokens per workgroup of k_wp_count / k_wp_emit (latok_debug_wordpiece_limits)
struct WordPieceTables {
    VocabTable initial, cont;         // (the seed is the same in both)
    uint32_t max_len0 = 0, max_len1 = 0;
    int max_chars = 0;
};
hipError_t launch_wp_count(const TokenText& t, const WordPieceTables& wt, int64_t* cnt, hipStream_t st);
hipError_t launch_wp_emit(bool out32, const TokenText& t, const WordPieceTables& wt, int32_t unk_id, const int64_t* rank,
                          const int64_t* n_pieces_dev, int64_t cap, int32_t* ids, void* spans, hipStream_t st);
hipError_t launch_wp_rows(bool out32, const int64_t* row_start, const int64_t* rank, int64_t n_str, int64_t n_tok, void* indptr_out, hipStream_t st);
hipError_t launch_wp_pad(const int32_t* ids, const int64_t* row_start, const int64_t* rank, int64_t n_str, int64_t n_tok, int64_t max_length, int add_special,
                         int32_t cls_id, int32_t sep_id, int32_t pad_id, int32_t* input_ids, int32_t* lengths, hipStream_t st);
// byte-level BPE ids (bpe_kernels.hip, bpe.h).  launch_bpe_count leaves the pieces of every token in cnt[0 .. n_tok) and 0 in
// cnt[n_tok], and the final part-start mask of every token of at most 64 bytes in masks[0 .. n_tok); the caller scans the n_tok + 1
// entries into rank[]; launch_bpe_emit stores ids (through rank_id) and string-relative spans if asked for at the piece rank, only
// if the total fits cap.  Row pointers and the padded block are launch_wp_rows / launch_wp_pad.  Device memory, read only.
constexpr int kBpeBlock = 256;   // tokens per workgroup of k_bpe_count / k_bpe_emit (latok_debug_bpe_limits)
struct BpeTable {
    VocabTable table;                   // id slot = the word's rank
    const int32_t* rank_id = nullptr;   // [max(n_words, 1)]
    int64_t n_words = 0;
    uint32_t max_len = 0;               // bytes of the longest word
    int max_bytes = 0;                  // 1 .. 4096
    int lead_space = 0;
};
hipError_t launch_bpe_count(const TokenText& t, const BpeTable& bt, int64_t* cnt, uint64_t* masks, hipStream_t st);
hipError_t launch_bpe_emit(bool out32, const TokenText& t, const BpeTable& bt, int32_t unk_id, const int64_t* rank, const uint64_t* masks,
                           const int64_t* n_pieces_dev, int64_t cap, int32_t* ids, void* spans, hipStream_t st);
// GPT-2's pre-tokenizer as a token front (pretok_kernels.hip, pretok.h): one launch, one wave per tile of kTile bytes, leaves the planes a
// token call reads -- bits = a bit at every byte where a pre-token starts, space = all zero (every pre-token is kept, nothing is
// stripped), both n_words = ceil(total / 64) words with zero bits behind the batch's end -- and tile_first[tile], as k_tile_index does.
// u8 is 16-byte aligned; nothing outside [0, total) is read.  latok_debug_pretok_limits reports the constants.
constexpr int kPretokWaves = 4;   // tiles per workgroup of k_pretok_planes
hipError_t launch_pretok_planes(const uint8_t* u8, int64_t total, const int64_t* row_off, int64_t n_str, uint64_t* bits, uint64_t* space,
                                int64_t* tile_first, hipStream_t st);
// The cl100k / Llama 3 pre-tokenizer as a token front: the same planes and tile index by the same geometry, in two launches --
// k_pretok_cl100k_records leaves one 4-byte carry record per tile in tile_rec[ceil(total / kTile)], k_pretok_cl100k_planes walks them
// (kPretokWalk = 64 records per step) and writes the planes.  latok_debug_pretok_cl100k_limits reports the constants.
constexpr int kPretokWalk = 64;   // tile records per walk step: one per lane
hipError_t launch_pretok_cl100k_planes(const uint8_t* u8, int64_t total, const int64_t* row_off, int64_t n_str, uint32_t* tile_rec, uint64_t* bits,
                                       uint64_t* space, int64_t* tile_first, hipStream_t st);
// SentencePiece's segments as a token front (pretok_kernels.hip, spbpe.h): launch_pretok_planes' contract with another rule -- a bit at every
// byte where a segment starts.  No table is read.
hipError_t launch_pretok_spm_planes(const uint8_t* u8, int64_t total, const int64_t* row_off, int64_t n_str, uint64_t* bits, uint64_t* space,
                                    int64_t* tile_first, hipStream_t st);
// SentencePiece BPE ids (spbpe_kernels.hip, spbpe.h): launch_bpe_count / launch_bpe_emit's contract for an object of latok_bpe_create_spm.  The
// tokens are the segments of the front above; the lookups read every segment's virtual text; a segment may have more pieces than bytes
// (byte fallback of a marker: three pieces for one space, three for the dummy), at most 3 * (bytes + strings) in a batch.
struct SpBpeTable {
    BpeTable bt;                         // (lead_space is not read)
    const int32_t* byte_ids = nullptr;   // [256], or NULL: no byte fallback
    int add_dummy_prefix = 0;
    int fuse_unk = 0;
};
hipError_t launch_spbpe_count(const TokenText& t, const SpBpeTable& sp, int64_t* cnt, uint64_t* masks, hipStream_t st);
hipError_t launch_spbpe_emit(bool out32, const TokenText& t, const SpBpeTable& sp, int32_t unk_id, const int64_t* rank, const uint64_t* masks,
                             const int64_t* n_pieces_dev, int64_t cap, int32_t* ids, void* spans, hipStream_t st);
// Unigram (Viterbi) ids (unigram_kernels.hip, unigram.h).  launch_uni_count leaves the pieces of every token in cnt[0 .. n_tok) and 0
// in cnt[n_tok], and three words per token of at most 64 bytes in marks[] (three arrays of n_tok words: the piece starts, which of them
// are unknown, whether the marker's piece is); the caller scans the n_tok + 1 entries into rank[]; launch_uni_emit stores ids (through
// pos_id) and string-relative spans if asked for at the piece rank, only if the total fits cap.  Row pointers and the padded block are
// launch_wp_rows / launch_wp_pad.  Device memory, read only.
constexpr int kUniBlock = 128;   // tokens per workgroup of k_uni_count / k_uni_emit (latok_debug_unigram_limits)
struct UniTable {
    VocabTable plain, marked;           // id slot = the word's position in the list (the seed is the same in both)
    const int32_t* pos_id = nullptr;    // [max(n_words, 1)]
    const float* pos_score = nullptr;   // [max(n_words, 1)]
    int64_t n_words = 0;
    uint32_t max_len_plain = 0, max_len_marked = 0;   // bytes of the longest word of either table
    int32_t marker_pos = -1;            // the word that is the marker alone
    int marker_len = 0;                 // 0: no token is marked
    float unk_score = 0.0f;
    int fuse_unk = 0;
    int max_bytes = 0;                  // 1 .. 4096
};
hipError_t launch_uni_count(const TokenText& t, const UniTable& ut, int64_t* cnt, uint64_t* marks, hipStream_t st);
hipError_t launch_uni_emit(bool out32, const TokenText& t, const UniTable& ut, int32_t unk_id, const int64_t* rank, const uint64_t* marks,
                           const int64_t* n_pieces_dev, int64_t cap, int32_t* ids, void* spans, hipStream_t st);
// The gram keys of the term family: one term key per gram of the orders min_n .. max_n, each inside its own range of `keys`, which
// holds n_keys keys; the lookup spells a gram with `joiner` between its tokens (word grams) or around the word (character grams).
// launch_terms_reduce / _emit / _finish then take keys and the key-space row starts as they take the token keys and the token rows.
struct GramKeys {
    TokenText t;
    const int64_t* rank;   // key space, from the caller's scan: per ROW for word grams (n_str + 1 entries, where the row's keys start),
                           // per TOKEN for character grams (n_tok + 1 entries); the last entry = n_keys
    int64_t n_keys;
    int min_n, max_n;      // 1 <= min_n <= max_n <= kNgMax of ngram_text.h (the caller holds max_n there)
    uint32_t joiner;       // one byte: sep / pad
    TermKeyForm form;
    uint64_t* keys;
};
// one lane per token in workgroups of `block`, the kernel of the key form
template <typename K>
inline hipError_t launch_gram_keys(K* vocab, K* hashed, int block, const GramKeys& P, hipStream_t st) {
    if (P.t.n_str <= 0 || P.t.n_tok <= 0 || P.n_keys <= 0) return hipSuccess;
    hipLaunchKernelGGL(P.form.vocab ? vocab : hashed, dim3((unsigned)((P.t.n_tok + block - 1) / block)), dim3(block), 0, st, P);
    return hipGetLastError();
}
// word n-grams (ngram_kernels.hip).  launch_ngram_rows leaves the grams of every string in key_cnt[0 .. n_str) and 0 in
// key_cnt[n_str]; the caller scans the n_str + 1 entries into the rows' key ranks.
constexpr int kNgBlock = 256;   // tokens per workgroup of k_ngram_keys (latok_debug_ngram_limits)
hipError_t launch_ngram_rows(const int64_t* tok_cnt, int64_t n_str, int min_n, int max_n, int64_t* key_cnt, hipStream_t st);
hipError_t launch_ngram_keys(const GramKeys& P, hipStream_t st);
// character n-grams inside tokens (chargram_kernels.hip, chargram_text.h).  launch_cgram_count leaves the grams G(W) of every token in
// cnt[0 .. n_tok) and 0 in cnt[n_tok]; the caller scans the n_tok + 1 entries into the tokens' key ranks and takes the row starts in
// key space from launch_wp_rows.
constexpr int kCgBlock = 256;   // tokens per workgroup of k_cgram_count / k_cgram_keys (latok_debug_chargram_limits)
hipError_t launch_cgram_count(const TokenText& t, int min_n, int max_n, int64_t* cnt, hipStream_t st);
hipError_t launch_cgram_keys(const GramKeys& P, hipStream_t st);
// tfidf_kernels.hip: TF-IDF on a CSR in device memory (tfidf_weight.h).  indptr is int32 (ip32) or int64; nnz_dev != NULL: the entry
// count is the scan's own word, not yet read by the host -- the kernels then do nothing when it exceeds `cap`, what the buffers hold
// (launch_terms_emit's rule), and `nnz` is ignored.  launch_csr_check ORs kCsrBad* bits into *err (indptr == NULL: the columns alone;
// n_cols == 0: the indptr alone); the launches behind it return at once when *err is set.  launch_df_add: df[c] += 1 per entry, with the
// workgroup's LDS table of kDfSlots hot columns (cached) or one global atomic per entry.  launch_tfidf_rows: out[j] = the weight of
// entry j over its row's norm (idf == NULL: no idf; err == NULL: nothing was checked); out may be `data` itself.  A row of at most
// kTfidfSubMax entries is taken by 16 lanes, one of at most kTfidfWaveMax by a wave, a longer one by a workgroup of a second launch
// (latok_debug_tfidf_limits).
constexpr int kTfidfSubMax = 64, kTfidfWaveMax = 1024, kDfSlots = 1024;
constexpr int kCsrBadStart = 1, kCsrBadOrder = 2, kCsrBadTotal = 4, kCsrBadColumn = 8;
hipError_t launch_csr_check(bool ip32, const void* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int64_t* nnz_dev, int64_t cap,
                            int64_t n_cols, int* err, hipStream_t st);
hipError_t launch_df_add(bool cached, const int32_t* indices, int64_t nnz, const int64_t* nnz_dev, int64_t cap, const int* err, int32_t* df,
                         hipStream_t st);
hipError_t launch_idf_weights(const int32_t* df, int64_t n_cols, int64_t n_docs, bool smooth, float* idf, hipStream_t st);
hipError_t launch_tfidf_rows(bool ip32, const void* indptr, const int32_t* indices, const int32_t* data, int64_t n_rows, int64_t nnz,
                             const int64_t* nnz_dev, int64_t cap, const float* idf, int opts, const int* err, float* out, hipStream_t st);
// the commit behind it: (a) the padded dwords of the fresh slots -> ctl[0]; (b) their bytes into the blob, resident words stored
hipError_t launch_count_commit_sum(const CountTable& ct, hipStream_t st);
hipError_t launch_count_commit_copy(const uint8_t* u8, const CountTable& ct, hipStream_t st);
// zeros at codes[t .. t + kTile + 256), t = *total_dev held inside [0, bound]
hipError_t launch_pad_codes(uint8_t* codes, const int64_t* total_dev, int64_t bound, hipStream_t st);
int64_t utf8_blocks(int64_t total_bytes);   // 4 KiB blocks of the chunk-parallel UTF-8 decoder
int64_t utf8_block_bytes();                 // kU8Block: bytes per block of that decoder (latok_debug_limits)
int64_t scan_small_max();                   // kScanSmallMax: entries above which launch_exclusive_scan takes three launches
int64_t scan_local_chunk();                 // kScanChunk: entries per workgroup of k_scan_local / k_scan_add (latok_debug_scan_limits)
int64_t scan_block_threads();               // kScanBlock: threads of every kernel of launch_exclusive_scan
hipError_t launch_utf8_block_counts(const uint8_t* u8, int64_t total, int64_t* block_cnt, hipStream_t st);
hipError_t launch_utf8_decode(const uint8_t* u8, int64_t total, const int64_t* byte_off, int64_t n_str,
                              const int64_t* block_base, uint16_t* chunk_pref, int64_t total_cps, uint32_t* cps,
                              int64_t* cp_off, hipStream_t st);
hipError_t launch_widen_units(const void* units, int kind, int64_t n, uint32_t* cps, hipStream_t st);   // kind 1 / 2 -> UTF-32
hipError_t launch_corpus_fill(uint64_t seed, int model, uint64_t sid0, int64_t n_str, const int64_t* row_off,
                              uint32_t* cps, hipStream_t st);
hipError_t launch_stream_read(const void* src, int64_t bytes, uint32_t* sink, int n_cu, hipStream_t st);
hipError_t launch_utf8_bytes(const uint32_t* cps, int64_t n, unsigned long long* total, hipStream_t st);
// fold_kernels.hip: case folding and accent stripping of a UTF-8 batch (fold_map.h).  start32 = fold_start_words(total) dwords,
// group_pref = fold_groups(total) entries, tile_cnt / tile_rank = fold_tiles(total) entries, scanned by launch_tile_scan between the
// two passes.  launch_fold_write stores the bytes only if the total fits cap (out may be NULL) and out_off[n_str + 1] always.
constexpr int kFoldTile = 4096;   // bytes per wave of k_fold_counts / k_fold_write (latok_debug_fold_limits)
int64_t fold_start_words(int64_t total);
int64_t fold_groups(int64_t total);
int64_t fold_tiles(int64_t total);
hipError_t launch_fold_starts(const int64_t* byte_off, int64_t n_str, int64_t total, uint32_t* start32, hipStream_t st);
hipError_t launch_fold_counts(const uint8_t* u8, int64_t total, const uint32_t* start32, int fold, const FoldTables& T, uint16_t* group_pref,
                              int64_t* tile_cnt, hipStream_t st);
hipError_t launch_fold_write(const uint8_t* u8, int64_t total, const uint32_t* start32, int fold, const FoldTables& T, const uint16_t* group_pref,
                             const int64_t* tile_rank, const int64_t* tile_cnt, const int64_t* row_off, int64_t n_str, uint8_t* out, int64_t cap,
                             const int64_t* n_items_dev, int64_t* out_off, hipStream_t st);
// detok_kernels.hip: decoding, ids back to bytes (detok.h).  The pieces are the ids of a CSR (row_start: its int64 row starts, n_cells =
// the id count) or the cells of a padded [n_rows, max_length] block (row_start == NULL; lengths may be NULL: every cell counts).
// launch_detok_count leaves the output bytes of every piece in cnt[0 .. n_cells) and the sum of every workgroup of kDetokBlock pieces in
// wg_sum[0 .. detok_groups(n_cells)), and adds the unknown ids to *n_unknown; the caller scans the sums into wg_rank (launch_tile_scan);
// launch_detok_write stores out_off[n_rows + 1] always and the bytes only if the total fits cap (out may be NULL).  *err: the error word
// of launch_csr_check / launch_detok_lengths in front of them; the launches return at once when it is set.  latok_debug_detok_limits
// reports the three constants.
constexpr int kDetokBlock = 256;       // pieces per workgroup of k_detok_count / k_detok_write
constexpr int kDetokWin = 4096;        // bytes of the LDS window of k_detok_write, a multiple of 16
constexpr int kDetokLaneBytes = 64;    // bytes a piece puts into a window by its own lane at most
constexpr int kDetokBadLength = 16;    // beside kCsrBad*: a length of the padded form lies outside [0, max_length]
struct DetokTable {
    const uint32_t* blob = nullptr;
    const void* entries = nullptr;     // DtEntry[n_words]
    const int32_t* keys = nullptr;     // sorted form: the distinct ids
    const int32_t* vals = nullptr;     // the entry by id - min_id (dense) or beside keys[i]
    DtMap map{0, 0, 0};
    int mode = 0;
    uint32_t sep = 0;
};
struct DetokSkip {
    int32_t id[kDtMaxSkip];
    int n;
};
struct DetokRows {
    const int64_t* row_start;
    const int32_t* lengths;
    int64_t n_rows, max_length, n_cells;
};
int64_t detok_groups(int64_t n_cells);
hipError_t launch_detok_lengths(const int32_t* lengths, int64_t n_rows, int64_t max_length, int* err, hipStream_t st);
hipError_t launch_detok_widen(const int32_t* indptr, int64_t n, int64_t* row_start, hipStream_t st);
hipError_t launch_detok_count(const DetokTable& T, const DetokRows& R, const int32_t* ids, const DetokSkip& S, const int* err, uint32_t* cnt,
                              int64_t* wg_sum, unsigned long long* n_unknown, hipStream_t st);
hipError_t launch_detok_write(const DetokTable& T, const DetokRows& R, const int32_t* ids, const DetokSkip& S, const int* err, const uint32_t* cnt,
                              const int64_t* wg_rank, const int64_t* total_dev, uint8_t* out, int64_t cap, int64_t* out_off, hipStream_t st);

}  // namespace latok
#endif
