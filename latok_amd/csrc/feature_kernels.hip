// feature_kernels.hip -- featurize on the tile grid: k_features_tiles and its launcher.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bitscan.h"
#include "feat_records.h"
#include "kernels.h"
#include "tile_core.h"

namespace latok {

// ---------------------------------------------------------------------------------------------------------------
// featurize: per-token sums of the 25 feature columns (reference default_tokenizer.py:163-191), one wave
// per tile like the split kernel.  The tile's chars are classified into rule codes and bit-sliced exactly as above,
// all 25 feature planes of a word are built in registers (lk_feature_planes), and the sum of column c over a token is
// popcount(plane_c & token_span): the work per word is proportional to its tokens, not its chars, and the n x 25
// matrix never exists.  A token that runs past its word takes the "head" sums (chars before the first boundary) of the
// following words from the neighbour lanes; one that runs past the tile is finished char by char (rare).  The 25
// bytes of a token are packed in 7 dwords (byte-wise wrap-around adds = the reference's uint8 arithmetic) and leave
// through the wave's staging buffer as one contiguous stream.
// ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t swar_add_u8(uint32_t a, uint32_t b) {
    return ((a & 0x7F7F7F7Fu) + (b & 0x7F7F7F7Fu)) ^ ((a ^ b) & 0x80808080u);
}
__device__ __forceinline__ FeatSums feat_popc(const lk_planes& F, lk_u64 m) {
    FeatSums r;
#pragma unroll
    for (int j = 0; j < 7; ++j) r.v[j] = 0;
#pragma unroll
    for (int c = 0; c < LK_N_FEATURES; ++c)
        r.v[c >> 2] |= (uint32_t)__popcll(LK_PLANE_GET(F, c) & m) << (8 * (c & 3));   // <= 64: no byte overflow
    return r;
}
// the same over one 32-bit half of the word (HI = 0: chars 0..31, 1: chars 32..63): a token of a few chars lies in one half,
// so its 25 sums cost one and + one popcount per column instead of two
template <int HI>
__device__ __forceinline__ FeatSums feat_popc_half(const lk_planes& F, uint32_t m) {
    FeatSums r;
#pragma unroll
    for (int j = 0; j < 7; ++j) r.v[j] = 0;
#pragma unroll
    for (int c = 0; c < LK_N_FEATURES; ++c)
        r.v[c >> 2] |= (uint32_t)__popc(LK_PLANE_HALF(F, c, HI) & m) << (8 * (c & 3));   // <= 32: no byte overflow
    return r;
}
__device__ __forceinline__ uint32_t feat_row_bits1(uint32_t w, uint32_t p, uint32_t x, uint32_t y, bool first, bool last) {
    // 25 columns of one char from base words (aux_kernels.hip:feature_row_bits, same bit layout)
    uint32_t r = w & 0xFFFu;
    r |= ((p >> 0) & 1u) << 12; r |= ((x >> 0) & 1u) << 13; r |= ((p >> 1) & 1u) << 14; r |= ((x >> 1) & 1u) << 15;
    r |= ((p >> 3) & 1u) << 16; r |= ((x >> 3) & 1u) << 17;
    r |= (first ? 1u : (p >> 5) & 1u) << 18; r |= (last ? 1u : (x >> 5) & 1u) << 19;
    r |= ((p >> 6) & 1u) << 20; r |= ((x >> 8) & 1u) << 21; r |= ((x >> 10) & 1u) << 22;
    r |= ((y >> 0) & 1u) << 23; r |= ((y >> 10) & 1u) << 24;
    return r;
}

// Lane = word while the sums are computed, but the output is token-major (all tokens of lane 0, then lane 1, ...), so
// a tile's records have to meet in LDS before they can leave as a stream.  A window that only holds part of a tile
// forces rounds in which most lanes idle (192-token rounds: 5x the instructions); writing the 25-byte records straight
// to global memory costs +0.4 ms in scattered stores.  So this kernel trades waves for LDS: kFeatWaves waves per CU,
// each with a window for kFeatRound tokens (a 4096-char tile of word-soup text has ~830), which doubles as the
// code-byte staging buffer before the planes are built.
// kFeatWaves, kFeatRound, kFeatRec, kFeatRoundTm, kFeatWinBytes and kFeatFormThresh: kernels.h (latok_debug_limits reports them)
static_assert(kFeatRoundTm * (kFeatRec + 2) + 16 <= kFeatWinBytes, "token-major round fits the window");
constexpr int kFeatWaveLds = kFeatWinBytes + 16 + 66 * 8;             // window | (unused) | string-start words
constexpr int kFeatLdsTotal = kFeatWaves * kFeatWaveLds;
static_assert(kFeatLdsTotal <= 160 * 1024, "LDS budget of one CU");
static_assert(kFeatWinBytes % 16 == 0 && kFeatWaveLds % 16 == 0, "alignment");

// span records (4 x OUT per token) go through the same window in rounds of what fits
template <typename OUT>
constexpr int span_round() { return kFeatWinBytes / (4 * (int)sizeof(OUT)) < kFeatRound ? kFeatWinBytes / (4 * (int)sizeof(OUT)) : kFeatRound; }

// 64 rule codes of one word (16-byte aligned) -> d[16]
__device__ __forceinline__ void load_codes64(const uint8_t* __restrict__ p, uint32_t (&d)[16]) {
    const u32x4* q = reinterpret_cast<const u32x4*>(p);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const u32x4 v = q[k];
        d[4 * k + 0] = v.x; d[4 * k + 1] = v.y; d[4 * k + 2] = v.z; d[4 * k + 3] = v.w;
    }
}

template <typename OUT>
__device__ __forceinline__ void feature_tile(const FeatParams& P, const TileLds& L, int64_t t, int lane) {
    OUT* const spans4 = reinterpret_cast<OUT*>(P.spans4);   // int64 or int32 records (LATOK_OUT_INT32)
    const int64_t t0 = t * kTile;
    const int64_t total = P.total;
    const int64_t n_words = (total + 63) >> 6;
    const int64_t w = t * 64 + lane;
    const int n_wave = (int)P.tile_cnt[t];
    if (n_wave == 0) return;
    const lk_u64 x = w < n_words ? P.kept[w] : 0ull;          // kept tokens that start in my word
    const int off = w < n_words ? (int)P.word_pref[w] : 0;
    const int64_t base_out = P.tile_rank[t];
    const lk_u64 xb = w < n_words ? P.bits[w] : 0ull;         // all boundaries of my word

    // ---- string starts of the tile (+ the two words behind it) as bits in LDS, from the per-tile string index --------
    int64_t idx0 = P.tile_first[t];
    idx0 = idx0 < 0 ? 0 : (idx0 > P.n_str ? P.n_str : idx0);
    // start of the string that is open when the tile begins (spans are string relative)
    const int64_t start_before = idx0 > 0 ? P.row_off[idx0 - 1] : 0;
    int64_t ro = idx0 + lane <= P.n_str ? P.row_off[idx0 + lane] : INT64_MAX;
    // ---- my word: 64 rule codes (1 B/char, left by the tile kernel: P.codes; padded behind `total`), the three
    //      neighbour codes from the neighbour lanes, and the 25 planes ------------------------------------------------
    const int64_t base = t0 + 64 * (int64_t)lane;
    const int64_t remain = total - base;
    const lk_u64 valid = remain >= 64 ? ~0ull : (remain <= 0 ? 0ull : ((1ull << remain) - 1ull));
    uint32_t d[16];
    load_codes64(P.codes + base, d);
    uint32_t edge = 0;                                    // lane 0: code of char t0-1; lane 63: codes of t0+4096, t0+4097
    if (lane == 0 && t0 > 0) edge = P.codes[t0 - 1];
    if (lane == 63) {
        if (t0 + kTile < total) edge = P.codes[t0 + kTile];
        if (t0 + kTile + 1 < total) edge |= (uint32_t)P.codes[t0 + kTile + 1] << 8;
    }
    L.bw[lane] = 0;
    if (lane < 2) L.bw[64 + lane] = 0;   // one word more than the split kernel: the first word of the next tile is needed
    wave_lds_sync();
    for (;;) {
        const int64_t rel = ro - t0;
        if (rel >= 0 && rel < kTile + 128) atomicOr(&L.bw[rel >> 6], 1ull << (rel & 63));
        const int64_t last = lane_read64(ro, 63);
        if (last >= t0 + kTile + 128) break;
        idx0 += 64;
        ro = idx0 + lane <= P.n_str ? P.row_off[idx0 + lane] : INT64_MAX;
    }
    wave_lds_sync();
    const lk_u64 B = L.bw[lane];
    const lk_u64 Bn = L.bw[lane + 1] & 3ull;
    lk_planes F;
    {
        lk_halo h;
        const uint32_t up = (uint32_t)dpp_mov<kDppWaveShr1, 0xF>(0, (int)(d[15] >> 24));      // from lane - 1
        const uint32_t dn = (uint32_t)dpp_mov<kDppWaveShl1, 0xF>(0, (int)(d[0] & 0xFFFFu));   // from lane + 1
        h.prev = lane > 0 ? up : edge;
        h.next0 = lane < 63 ? (dn & 0xFFu) : (edge & 0xFFu);
        h.next1 = lane < 63 ? (dn >> 8) : (edge >> 8);
        lk_u64 plane[8];
        lk_bitslice64(d, plane);
        lk_feature_planes(plane, h, B, Bn, F);
    }
    const uint32_t prev65 = (uint32_t)lane_read((int)(d[15] >> 24), 63);   // code of the tile's last char

    // ---- what a token that leaves my word collects from the following words -----------------------------------------
    const lk_u64 head_mask = (xb ? ((xb & (~xb + 1ull)) - 1ull) : ~0ull) & valid;
    const FeatSums H = feat_popc(F, head_mask);
    const int full = xb == 0;
    const int top = xb ? 63 - __builtin_clzll(xb) : 0;
    const bool need_tail = xb != 0 && ((x >> top) & 1ull);     // my last boundary starts a kept token: it continues
    FeatSums C;
#pragma unroll
    for (int j = 0; j < 7; ++j) C.v[j] = 0;
    bool open = need_tail;                                     // still collecting
    lk_u64 xb_next_tile = 0, nn_next_tile = 0;                 // boundary / non-SPACE masks of the next tile's first word
    FeatSums Hs = H;                                           // H / full of lane + d: one more DPP shift per step
    int fs = full;
    for (int d = 1; d < 64; ++d) {
        if (!__ballot(open && lane + d < 64)) break;
#pragma unroll
        for (int j = 0; j < 7; ++j) Hs.v[j] = (uint32_t)dpp_mov<kDppWaveShl1, 0xF>(0, (int)Hs.v[j]);
        fs = dpp_mov<kDppWaveShl1, 0xF>(0, fs);
        if (open && lane + d < 64) {
#pragma unroll
            for (int j = 0; j < 7; ++j) C.v[j] = swar_add_u8(C.v[j], Hs.v[j]);
            open = fs != 0;
        }
    }
    if (__ballot(open)) {
        // A token runs past the tile (the usual case for its last token): every lane builds the planes of the next tile's
        // first word (the same 64 codes, a broadcast load) and the open lanes take its head sums.
        const int64_t q0 = t0 + kTile;
        uint32_t d65[16];
        load_codes64(P.codes + q0, d65);
        lk_halo h65;
        h65.prev = prev65;                         // code of the tile's last char
        h65.next0 = q0 + 64 < total ? (uint32_t)P.codes[q0 + 64] : 0u;
        h65.next1 = q0 + 65 < total ? (uint32_t)P.codes[q0 + 65] : 0u;
        lk_u64 plane65[8];
        lk_bitslice64(d65, plane65);
        lk_planes F65;
        const lk_u64 B65 = L.bw[64], Bn65 = L.bw[65] & 3ull;
        lk_feature_planes(plane65, h65, B65, Bn65, F65);
        const int64_t rem65 = total - q0;
        const lk_u64 valid65 = rem65 >= 64 ? ~0ull : (rem65 <= 0 ? 0ull : ((1ull << rem65) - 1ull));
        const lk_u64 xb65 = (q0 >> 6) < n_words ? P.bits[q0 >> 6] : 0ull;
        const lk_u64 hm65 = (xb65 ? ((xb65 & (~xb65 + 1ull)) - 1ull) : ~0ull) & valid65;
        const FeatSums H65 = feat_popc(F65, hm65);
        xb_next_tile = xb65;
        nn_next_tile = ~LK_PLANE_GET(F65, 5) & valid65;
        if (open) {
#pragma unroll
            for (int j = 0; j < 7; ++j) C.v[j] = swar_add_u8(C.v[j], H65.v[j]);
            open = xb65 == 0 && q0 + 64 < total;
        }
    }
    const lk_u64 open_m = __ballot(open);
    if (open_m) {
        // Still open after the next tile's first word: a token of more than 64 chars that leaves the tile (at most one
        // lane: the owner of the tile's last kept token -- a masked URL, a long run of letters; a 1 M-char document
        // without whitespace is ONE such token).  The whole wave continues it, 64 words per step, lane = word: the same
        // planes + popcount as above, until the word that holds the next boundary; the partial sums meet in a
        // butterfly and go to the owner.  (The token lies inside one string: the only string start that matters is
        // the string's end.)
        const int owner = lk_ctz(open_m);
        const int64_t from = t0 + kTile + 64;
        // the string that holds the token ends at the first row offset > from - 1 (tokens never cross strings)
        int64_t lo_s = 0, hi_s = P.n_str;
        while (hi_s - lo_s > 1) {
            const int64_t mid = (lo_s + hi_s) >> 1;
            if (P.row_off[mid] <= from - 1) lo_s = mid; else hi_s = mid;
        }
        const int64_t s_end = P.row_off[lo_s + 1];
        FeatSums acc;
#pragma unroll
        for (int j = 0; j < 7; ++j) acc.v[j] = 0;
        for (int64_t c0 = from; c0 < total; c0 += kTile) {
            const int64_t wb = c0 + 64 * (int64_t)lane;
            const lk_u64 xbw = (wb >> 6) < n_words ? P.bits[wb >> 6] : 0ull;
            const lk_u64 hasb = __ballot(xbw != 0ull);
            const int fl = hasb ? lk_ctz(hasb) : 64;                  // lane of the word that holds the next boundary
            uint32_t dw[16];
            load_codes64(P.codes + wb, dw);                            // (in bounds: the code array is padded by a tile)
            uint32_t e2 = 0;
            if (lane == 0) e2 = P.codes[c0 - 1];
            if (lane == 63) {
                if (c0 + kTile < total) e2 = P.codes[c0 + kTile];
                if (c0 + kTile + 1 < total) e2 |= (uint32_t)P.codes[c0 + kTile + 1] << 8;
            }
            const uint32_t up = (uint32_t)__shfl_up((int)(dw[15] >> 24), 1);
            const uint32_t dn = (uint32_t)__shfl_down((int)(dw[0] & 0xFFFFu), 1);
            lk_halo hw;
            hw.prev = lane > 0 ? up : e2;
            hw.next0 = lane < 63 ? (dn & 0xFFu) : (e2 & 0xFFu);
            hw.next1 = lane < 63 ? (dn >> 8) : (e2 >> 8);
            const int64_t rel = s_end - wb;                            // the string's end as a "string start" bit
            const lk_u64 Bw = (rel >= 0 && rel < 64) ? (1ull << rel) : 0ull;
            const lk_u64 Bnw = (rel == 64) ? 1ull : (rel == 65 ? 2ull : 0ull);
            lk_u64 pw[8];
            lk_bitslice64(dw, pw);
            lk_planes Fw;
            lk_feature_planes(pw, hw, Bw, Bnw, Fw);
            const int64_t remw = total - wb;
            const lk_u64 validw = remw >= 64 ? ~0ull : (remw <= 0 ? 0ull : ((1ull << remw) - 1ull));
            lk_u64 m = 0ull;
            if (lane < fl) m = validw;
            else if (lane == fl) m = ((xbw & (~xbw + 1ull)) - 1ull) & validw;
            const FeatSums part = feat_popc(Fw, m);
#pragma unroll
            for (int j = 0; j < 7; ++j) acc.v[j] = swar_add_u8(acc.v[j], part.v[j]);
            if (hasb) break;
        }
#pragma unroll
        for (int sh = 32; sh >= 1; sh >>= 1) {
#pragma unroll
            for (int j = 0; j < 7; ++j) acc.v[j] = swar_add_u8(acc.v[j], (uint32_t)__shfl_xor((int)acc.v[j], sh));
        }
        if (lane == owner) {
#pragma unroll
            for (int j = 0; j < 7; ++j) C.v[j] = swar_add_u8(C.v[j], acc.v[j]);
        }
    }

    // ---- per-word values both forms below need --------------------------------------------------------------------
    const lk_u64 nn = ~LK_PLANE_GET(F, 5) & valid;             // non-SPACE chars of my word
    // the next word's masks (from lane + 1)
    lk_u64 xb1 = (lk_u64)(uint32_t)dpp_mov<kDppWaveShl1, 0xF>(0, (int)(uint32_t)xb) |
                 ((lk_u64)(uint32_t)dpp_mov<kDppWaveShl1, 0xF>(0, (int)(uint32_t)(xb >> 32)) << 32);
    lk_u64 nn1 = (lk_u64)(uint32_t)dpp_mov<kDppWaveShl1, 0xF>(0, (int)(uint32_t)nn) |
                 ((lk_u64)(uint32_t)dpp_mov<kDppWaveShl1, 0xF>(0, (int)(uint32_t)(nn >> 32)) << 32);
    if (lane == 63) { xb1 = xb_next_tile; nn1 = nn_next_tile; }
    // start of the string that is open at my word's first char: the last string start before my word inside the tile,
    // else the one that was open when the tile began
    int last_b = B ? 64 * lane + 63 - __builtin_clzll(B) : -1;  // tile-relative position of my word's last string start
    const int carry = dpp_mov<kDppWaveShr1, 0xF>(-1, wave_scan_max(last_b, -1));   // exclusive: lane 0 gets -1
    const int64_t lo_in = carry >= 0 ? t0 + carry : start_before;

    // ---- skewed tiles (some word holds many more tokens than the mean, e.g. CJK text where every char is a token):
    // token-major form.  Every lane lists its tokens as (lane, bit) codes at their rank inside the tile, then lane j
    // takes the j-th token and pulls the owner word's 25 planes (and masks) through shuffles, so all lanes stay busy.
    // ~70 64-bit shuffles per token make it the slower form for evenly filled tiles, hence the choice per tile.
    const int maxc = wave_max(lk_popc(x), 0);
    // threshold swept on C2 (word-major 9 % faster) and C3 (token-major 15 % faster): fullest word > 1.5 x steps of 64 tokens
    // The word-major walk below runs as long as the fullest word (maxc steps of ~160 instructions with the span records), once
    // per window round; the token-major form takes ceil(n_wave / 64) steps of ~300 whatever the spread.
    const int wm_rounds = (n_wave + kFeatRound - 1) / kFeatRound;
    if (maxc * 2 * wm_rounds > ((n_wave + 63) >> 6) * kFeatFormThresh) {
        uint8_t* fwin = L.stage;
        uint16_t* codes = reinterpret_cast<uint16_t*>(L.stage + kFeatRoundTm * kFeatRec + 16);   // behind the feature records
        lk_u64 trest = x;
        int tk = off;
        for (int win0 = 0; win0 < n_wave; win0 += kFeatRoundTm) {
            uint8_t* const fdst = reinterpret_cast<uint8_t*>(P.features) + (base_out + win0) * 25;
            const int shift = record_shift(fdst);
            while (trest && tk < win0 + kFeatRoundTm) {
                const int b = lk_ctz(trest);
                trest &= trest - 1;
                codes[tk - win0] = (uint16_t)((lane << 6) | b);
                ++tk;
            }
            wave_lds_sync();
            const int n_here = min(kFeatRoundTm, n_wave - win0);
            for (int j0 = 0; j0 < n_here; j0 += 64) {
                const int j = j0 + lane;
                const bool active = j < n_here;
                const int code = active ? (int)codes[j] : 0;
                const int owner = code >> 6, b = code & 63;
                const int64_t obase = t0 + 64 * (int64_t)owner;
                const int64_t orem = total - obase;
                const lk_u64 ovalid = orem >= 64 ? ~0ull : (orem <= 0 ? 0ull : ((1ull << orem) - 1ull));
                const lk_u64 o_xb = (lk_u64)__shfl((long long)xb, owner), o_xb1 = (lk_u64)__shfl((long long)xb1, owner),
                             o_nn1 = (lk_u64)__shfl((long long)nn1, owner), o_B = (lk_u64)__shfl((long long)B, owner);
                const int64_t o_lo_in = __shfl((long long)lo_in, owner);
                const lk_u64 above = o_xb & (~1ull << b);
                lk_u64 seg = (~0ull << b) & ovalid;
                if (above) seg &= (above & (~above + 1ull)) - 1ull;
                FeatSums sum;
#pragma unroll
                for (int q = 0; q < 7; ++q) sum.v[q] = 0;
                lk_u64 o_S = 0;
#pragma unroll
                for (int c = 0; c < LK_N_FEATURES; ++c) {
                    const lk_u64 pc = (lk_u64)__shfl((long long)LK_PLANE_GET(F, c), owner);
                    if (c == 5) o_S = pc;
                    sum.v[c >> 2] |= (uint32_t)__popcll(pc & seg) << (8 * (c & 3));
                }
#pragma unroll
                for (int q = 0; q < 7; ++q) {
                    const uint32_t cq = (uint32_t)__shfl((int)C.v[q], owner);
                    if (!above) sum.v[q] = swar_add_u8(sum.v[q], cq);
                }
                if (active) put_record(fwin + shift, j, sum);
                if (active && spans4) {   // (spans4 == NULL: the records come from another kernel, see below)
                    const lk_u64 o_nn = ~o_S & ovalid;
                    const int64_t p = obase + b;
                    const lk_u64 bl = o_B & ((2ull << b) - 1ull);
                    const int64_t lo = bl ? obase + 63 - __builtin_clzll(bl) : o_lo_in;
                    int64_t e, a2, e2;
                    if (above) {
                        const int eb = lk_ctz(above);
                        const lk_u64 sg = o_nn & (~0ull << b) & ((1ull << eb) - 1ull);
                        e = obase + eb;
                        a2 = obase + lk_ctz(sg);
                        e2 = obase + 64 - __builtin_clzll(sg);
                    } else if (o_xb1) {
                        const int eb = lk_ctz(o_xb1);
                        const lk_u64 sg0 = o_nn & (~0ull << b);
                        const lk_u64 sg1 = o_nn1 & ((1ull << eb) - 1ull);
                        e = obase + 64 + eb;
                        a2 = sg0 ? obase + lk_ctz(sg0) : obase + 64 + lk_ctz(sg1);
                        e2 = sg1 ? obase + 128 - __builtin_clzll(sg1) : obase + 64 - __builtin_clzll(sg0);
                    } else {
                        e = next_set_bit(P.bits, obase + 64, total);
                        const lk_u64 sg = o_nn & (~0ull << b);
                        a2 = sg ? obase + lk_ctz(sg) : next_zero_bit(P.space, obase + 64, e);
                        e2 = prev_zero_end(P.space, a2, e);
                    }
                    typedef OUT out2 __attribute__((ext_vector_type(2)));
                    out2* sp = reinterpret_cast<out2*>(spans4 + (base_out + win0 + j) * 4);
                    out2 v0, v1;
                    v0.x = (OUT)(p - lo);
                    v0.y = (OUT)(e - lo);
                    v1.x = (OUT)(a2 - lo);
                    v1.y = (OUT)(e2 - lo);
                    __builtin_nontemporal_store(v0, sp);
                    __builtin_nontemporal_store(v1, sp + 1);
                }
            }
            wave_lds_sync();
            flush_records(fwin, n_here, fdst, lane);
            wave_lds_sync();
        }
        return;
    }

    // ---- tokens of my word, round by round through the staging buffer -------------------------------------------------
    // The walk is split by 32-bit halves: first the tokens that start in chars 0..31 (popcounts on the low halves of the
    // planes only), then the part of the one token that may reach from the low half into the high half, then the tokens that
    // start in chars 32..63 (high halves only).  Ranks grow in that order, so the records land at consecutive slots.
    uint8_t* win = L.stage;
    uint32_t rest_lo = (uint32_t)x, rest_hi = (uint32_t)(x >> 32);
    const uint32_t xb_lo = (uint32_t)xb, xb_hi = (uint32_t)(xb >> 32);
    const uint32_t valid_lo = (uint32_t)valid, valid_hi = (uint32_t)(valid >> 32);
    FeatSums S_str;                       // low-half sums of the straddling token
#pragma unroll
    for (int j = 0; j < 7; ++j) S_str.v[j] = 0;
    int str_slot = -1;                    // its slot (>= 0: the upper part is still to be added)
    int k = off;
    for (int win0 = 0; win0 < n_wave; win0 += kFeatRound) {
        const int lim = win0 + kFeatRound;
        uint8_t* const fdst = reinterpret_cast<uint8_t*>(P.features) + (base_out + win0) * 25;
        uint8_t* const rwin = win + record_shift(fdst);   // where this round's records go (flush_records)
        while (rest_lo && k < lim) {
            const int b = __builtin_ctz(rest_lo);
            rest_lo &= rest_lo - 1u;
            const uint32_t above = xb_lo & (~1u << b);
            uint32_t seg = (~0u << b) & valid_lo;
            if (above) seg &= (above & (0u - above)) - 1u;
            const FeatSums sum = feat_popc_half<0>(F, seg);
            if (above) {
                put_record(rwin, k - win0, sum);
            } else {                      // no boundary up to char 31: the token goes on in the high half (the last low token)
                S_str = sum;
                str_slot = k;
            }
            ++k;
        }
        if (__ballot(str_slot >= 0 && rest_lo == 0u)) {
            if (str_slot >= 0 && rest_lo == 0u) {
                uint32_t seg = valid_hi;
                if (xb_hi) seg &= (xb_hi & (0u - xb_hi)) - 1u;          // chars 32.. up to the first boundary there
                const FeatSums s2 = feat_popc_half<1>(F, seg);
#pragma unroll
                for (int j = 0; j < 7; ++j) S_str.v[j] = swar_add_u8(S_str.v[j], s2.v[j]);
                if (!xb_hi) {                                             // ... and on into the following words
#pragma unroll
                    for (int j = 0; j < 7; ++j) S_str.v[j] = swar_add_u8(S_str.v[j], C.v[j]);
                }
                put_record(rwin, str_slot - win0, S_str);
                str_slot = -1;
            }
        }
        while (rest_lo == 0u && rest_hi && k < lim) {
            const int b = __builtin_ctz(rest_hi);
            rest_hi &= rest_hi - 1u;
            const uint32_t above = xb_hi & (~1u << b);
            uint32_t seg = (~0u << b) & valid_hi;
            if (above) seg &= (above & (0u - above)) - 1u;
            FeatSums sum = feat_popc_half<1>(F, seg);
            if (!above) {
#pragma unroll
                for (int j = 0; j < 7; ++j) sum.v[j] = swar_add_u8(sum.v[j], C.v[j]);
            }
            put_record(rwin, k - win0, sum);
            ++k;
        }
        wave_lds_sync();
        flush_records(win, min(kFeatRound, n_wave - win0), fdst, lane);
        wave_lds_sync();
    }

    // ---- the span records of the same tokens: {raw start, raw end, stripped start, stripped end}, string relative --------
    // (reference featurize: LaToken.start_idx / end_idx = the raw span, .text = text[stripped]; default_tokenizer.py:173-191)
    // spans4 == NULL (uniform): UTF-8 in byte space -- these positions are code points, the caller wants bytes: the records of the
    // same tokens, at the same ranks, are written by k_counts_scatter<2> from the byte-space masks (compact_kernels.hip)
    if (!spans4) return;
    OUT* swin = reinterpret_cast<OUT*>(L.stage);
    constexpr int kSpanRound = span_round<OUT>();
    lk_u64 rest = x;
    k = off;
    for (int win0 = 0; win0 < n_wave; win0 += kSpanRound) {
        while (rest && k < win0 + kSpanRound) {
            const int b = lk_ctz(rest);
            rest &= rest - 1;
            const int64_t p = base + b;
            const lk_u64 bl = B & ((2ull << b) - 1ull);         // string starts at or before the token (b = 63: all)
            const int64_t lo = bl ? base + 63 - __builtin_clzll(bl) : lo_in;
            const lk_u64 above = xb & (~1ull << b);
            int64_t e, a2, e2;
            if (above) {
                const int eb = lk_ctz(above);
                const lk_u64 seg = nn & (~0ull << b) & ((1ull << eb) - 1ull);
                e = base + eb;
                a2 = base + lk_ctz(seg);
                e2 = base + 64 - __builtin_clzll(seg);
            } else if (xb1) {
                const int eb = lk_ctz(xb1);
                const lk_u64 seg0 = nn & (~0ull << b);
                const lk_u64 seg1 = nn1 & ((1ull << eb) - 1ull);
                e = base + 64 + eb;
                a2 = seg0 ? base + lk_ctz(seg0) : base + 64 + lk_ctz(seg1);
                e2 = seg1 ? base + 128 - __builtin_clzll(seg1) : base + 64 - __builtin_clzll(seg0);
            } else {
                e = next_set_bit(P.bits, base + 64, total);
                const lk_u64 seg = nn & (~0ull << b);
                a2 = seg ? base + lk_ctz(seg) : next_zero_bit(P.space, base + 64, e);
                e2 = prev_zero_end(P.space, a2, e);
            }
            OUT* rec = swin + (k - win0) * 4;
            rec[0] = (OUT)(p - lo);
            rec[1] = (OUT)(e - lo);
            rec[2] = (OUT)(a2 - lo);
            rec[3] = (OUT)(e2 - lo);
            ++k;
        }
        wave_lds_sync();
        {
            // 16-byte stores: two (int64) or four (int32) values each; a record is 32 or 16 bytes, so the stream is aligned
            constexpr int kPer = 16 / (int)sizeof(OUT);
            typedef OUT vec_t __attribute__((ext_vector_type(16 / sizeof(OUT))));
            const int n_vec = min(kSpanRound, n_wave - win0) * 4 / kPer;
            vec_t* dst = reinterpret_cast<vec_t*>(spans4 + (base_out + win0) * 4);
            for (int i = lane; i < n_vec; i += 64) {
                vec_t v;
#pragma unroll
                for (int e = 0; e < kPer; ++e) v[e] = swin[kPer * i + e];
                __builtin_nontemporal_store(v, dst + i);
            }
        }
        wave_lds_sync();
    }
}

template <typename OUT>
__global__ __launch_bounds__(kFeatWaves * 64) void k_features_tiles(FeatParams P) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kFeatLdsTotal];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    bool gated = false;
    if (P.dt.total) {   // (uniform) the batch's size from device memory (kernels.h: DeviceTotal); a malformed batch writes nothing
        P.total = device_total(P.dt.total, P.total);
        P.n_tiles = (P.total + kTile - 1) / kTile;
        gated = P.dt.gate && *P.dt.gate != 0;
    }
    // (the caller's buffers are too small: nothing is written)
    if (!gated && !(P.n_tokens_dev && *P.n_tokens_dev > P.cap)) {
        TileLds L;
        L.small_bits = L.small_space = nullptr;
        L.t1 = L.t2 = L.lut = L.ctab = L.ltab = L.t1b = L.t2b = nullptr; L.tables = nullptr; L.ctl = nullptr;   // nothing is classified here: the tile kernel left the rule codes (P.codes)
        uint8_t* mine = lds + wave * kFeatWaveLds;
        L.stage = mine;
        L.halo = mine + kFeatWinBytes;
        L.bw = reinterpret_cast<lk_u64*>(mine + kFeatWinBytes + 16);
        for (int64_t t = (int64_t)blockIdx.x * kFeatWaves + wave; t < P.n_tiles; t += (int64_t)gridDim.x * kFeatWaves)
            feature_tile<OUT>(P, L, t, lane);
    }
    signal_block_done(P.done);   // (pinned outputs of a small host batch: the host polls the completion word)
}

hipError_t launch_features_tiles(const FeatParams& P, int n_cu, hipStream_t st) {
    if (P.n_tiles <= 0) return hipSuccess;
    int64_t blocks = (P.n_tiles + kFeatWaves - 1) / kFeatWaves;
    if (blocks > n_cu) blocks = n_cu;
    if (P.out32) hipLaunchKernelGGL((k_features_tiles<int32_t>), dim3((unsigned)blocks), dim3(kFeatWaves * 64), 0, st, P);
    else hipLaunchKernelGGL((k_features_tiles<int64_t>), dim3((unsigned)blocks), dim3(kFeatWaves * 64), 0, st, P);
    return hipGetLastError();
}

}  // namespace latok
