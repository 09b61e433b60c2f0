// Host harness for the body / head lane math of the joined token text (latok_amd/csrc/lane_math.h: lk_join_summary,
// lk_seg_carries, lk_join_planes), built by tests/test_join_tokens_host.py with g++.  It links the words the way k_join_counts
// does: 64 words form a tile whose summaries become 64-bit "ballots" and one carry chain per question; the carries into a tile
// come from the tiles around it, one tile per step.
//
// stdin:  n_words f_in b_in q_in          (what lies in front of word 0 / behind the last word)
//         n_words lines "x nn r" (hex)    boundary bits, non-SPACE bits, string-start bits
// stdout: n_words lines "body head" (hex)
#include <cstdio>
#include <vector>

#include "lane_math.h"

struct TileSum {
    lk_u64 Gf = 0, Gb = 0, Gq = 0, Sx = 0, Sr = 0;   // generate ballots, segment (= not propagate) ballots
};

int main() {
    long long n = 0;
    int f_end = 0, b_end = 0, q_end = 0;
    if (scanf("%lld %d %d %d", &n, &f_end, &b_end, &q_end) != 4 || n < 0) return 2;
    std::vector<lk_u64> x(n), nn(n), r(n);
    for (long long i = 0; i < n; ++i)
        if (scanf("%llx %llx %llx", &x[i], &nn[i], &r[i]) != 3) return 2;
    const long long n_tiles = (n + 63) / 64;
    std::vector<TileSum> ts(n_tiles);
    for (long long t = 0; t < n_tiles; ++t)
        for (int l = 0; l < 64; ++l) {
            const long long w = t * 64 + l;
            const lk_join_sum s = w < n ? lk_join_summary(x[w], nn[w], r[w]) : lk_join_summary(0, 0, 0);
            ts[t].Gf |= (lk_u64)s.gen_f << l;
            ts[t].Gb |= (lk_u64)s.gen_b << l;
            ts[t].Gq |= (lk_u64)s.gen_q << l;
            ts[t].Sx |= (lk_u64)!s.prop_x << l;
            ts[t].Sr |= (lk_u64)!s.prop_r << l;
        }
    for (long long t = 0; t < n_tiles; ++t) {
        // carries into the tile: walk the tiles in front / behind until one settles the question, else what lies beyond the ends
        int f_in = f_end, q_in = q_end, b_in = b_end;
        for (long long k = t - 1; k >= 0; --k) {
            if (lk_seg_out(ts[k].Gf, ts[k].Sx, lk_seg_carries(ts[k].Gf, ts[k].Sx, 0))) { f_in = 1; break; }
            if (ts[k].Sx) { f_in = 0; break; }
        }
        for (long long k = t - 1; k >= 0; --k) {
            if (lk_seg_out(ts[k].Gq, ts[k].Sr, lk_seg_carries(ts[k].Gq, ts[k].Sr, 0))) { q_in = 1; break; }
            if (ts[k].Sr) { q_in = 0; break; }
        }
        for (long long k = t + 1; k < n_tiles; ++k) {
            const lk_u64 Gr = lk_rev(ts[k].Gb), Sr = lk_rev(ts[k].Sx);
            if (lk_seg_out(Gr, Sr, lk_seg_carries(Gr, Sr, 0))) { b_in = 1; break; }
            if (Sr) { b_in = 0; break; }
        }
        const lk_u64 Cf = lk_seg_carries(ts[t].Gf, ts[t].Sx, f_in);
        const lk_u64 Cb = lk_seg_carries(lk_rev(ts[t].Gb), lk_rev(ts[t].Sx), b_in);
        const lk_u64 Cq = lk_seg_carries(ts[t].Gq, ts[t].Sr, q_in);
        for (int l = 0; l < 64 && t * 64 + l < n; ++l) {
            const long long w = t * 64 + l;
            const lk_join_planes_t o = lk_join_planes(x[w], nn[w], r[w], (int)((Cf >> l) & 1), (int)((Cb >> (63 - l)) & 1), (int)((Cq >> l) & 1));
            printf("%llx %llx\n", o.body, o.head);
        }
    }
    return 0;
}
