// Host harness of latok_amd/csrc/count_table.h (tests/test_count_table_host.py): find-or-insert, both compares and the commit of the
// device's counting table, run by g++ with __atomic_* builtins on tokens laid into a poisoned text buffer -- single-threaded and
// with several threads on one table --, so that the slot layout, the wrap of the probe, its bound, the masks, the bounds of the
// aligned loads and the claim protocol are tested without a device.  The hash is token_hash.h's, as in the kernel.
//   stdin:  commands, one per line:
//             T <seed hex> <max_words> <probe_max>    a new, empty table of ct_slot_count(max_words) slots
//             B <threads> <poison hex> <n>            a batch of n tokens; n lines follow:  <phase 0..3> <token as hex>
//                                                     the tokens lie in one text buffer in this order, each after 0..3 poison
//                                                     bytes so that its first byte has the given phase; the buffer ends with the
//                                                     aligned dword of the last token's last byte.  threads = 1: the tokens are
//                                                     entered in order; threads > 1: every thread t enters ALL tokens, starting at
//                                                     token t * n / threads and wrapping.  Then the batch is committed.
//             D                                       dump the table
//             E                                       check that no occupied slot word equals the empty word
//   stdout: per T:  "slots <n_slots>"
//           per B:  threads = 1: per token "<slot or -1> <slot loads>"; then "batch counted <c> dropped <d> fresh <f> blob <dwords>"
//           per D:  per occupied slot "<slot> <word as hex> <count>", then "end"
//           per E:  "ok"
//   exit 2 if a text load left the buffer, 3 if a blob access left the blob, 4 if a slot is still fresh after a commit
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <thread>
#include <vector>

#include "count_table.h"
#include "token_hash.h"

static int g_bad = 0;
static thread_local long tl_loads = 0;

struct HostAtomics {
    static uint64_t load(const uint64_t* p) {
        ++tl_loads;
        return __atomic_load_n(p, __ATOMIC_RELAXED);
    }
    static uint64_t cas(uint64_t* p, uint64_t expect, uint64_t v) {
        __atomic_compare_exchange_n(p, &expect, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
        return expect;
    }
};

static std::vector<uint8_t> unhex(const char* hex) {
    std::vector<uint8_t> out;
    const size_t n = strlen(hex) / 2;
    for (size_t i = 0; i < n; ++i) {
        unsigned v = 0;
        sscanf(hex + 2 * i, "%2x", &v);
        out.push_back((uint8_t)v);
    }
    return out;
}

int main() {
    static char tok[1 << 12], hex[1 << 12];
    std::vector<uint64_t> slots, counts;
    std::vector<uint32_t> blob{0u};   // dword 0 is reserved
    uint32_t seed = 0, probe_max = 0;
    while (scanf(" %4095s", tok) == 1) {
        if (tok[0] == 'T') {
            long max_words;
            if (scanf("%x %ld %u", &seed, &max_words, &probe_max) != 3) return 1;
            slots.assign(ct_slot_count(max_words), kCtEmpty);
            counts.assign(slots.size(), 0);
            blob.assign(1, 0u);
            printf("slots %zu\n", slots.size());
            continue;
        }
        if (tok[0] == 'E') {
            for (uint32_t len = 1; len <= (uint32_t)kCtMaxWordBytes; ++len)
                for (uint32_t h : {0u, 0xFFFFu, 0x10000u, 0xFFFFFFFFu}) {
                    const uint64_t f = ct_fresh_word(len, h, 0);
                    if (f == kCtEmpty || ct_resident_word(f, 1) == kCtEmpty || ct_len(f) != len || ct_len(ct_resident_word(f, 1)) != len) return 1;
                    if (!ct_is_fresh(f) || ct_is_fresh(ct_resident_word(f, 1)) || ct_pos(ct_resident_word(f, 77)) != 77) return 1;
                    if (ct_pos(ct_fresh_word(len, h, kCtMaxTextBytes - 1)) != (uint64_t)(kCtMaxTextBytes - 1)) return 1;
                }
            printf("ok\n");
            continue;
        }
        if (tok[0] == 'D') {
            for (size_t s = 0; s < slots.size(); ++s) {
                const uint64_t v = slots[s];
                if (v == kCtEmpty) continue;
                if (ct_is_fresh(v)) return 4;
                if (ct_pos(v) + ct_padded_dwords(v) > blob.size()) return 3;
                const uint8_t* p = reinterpret_cast<const uint8_t*>(blob.data() + ct_pos(v));
                printf("%zu ", s);
                for (uint32_t b = 0; b < ct_len(v); ++b) printf("%02x", p[b]);
                // (the padding behind the word is zero)
                for (uint32_t b = ct_len(v); b < 4 * ct_padded_dwords(v); ++b)
                    if (p[b] != 0) return 3;
                printf(" %llu\n", (unsigned long long)counts[s]);
            }
            printf("end\n");
            continue;
        }
        if (tok[0] != 'B') return 1;
        int threads;
        unsigned poison;
        long n;
        if (scanf("%d %x %ld", &threads, &poison, &n) != 3) return 1;
        std::vector<uint8_t> text;
        std::vector<int64_t> ta, te;
        for (long i = 0; i < n; ++i) {
            int phase;
            if (scanf("%d %4095s", &phase, hex) != 2) return 1;
            const std::vector<uint8_t> w = unhex(hex);
            if (w.empty() || w.size() > (size_t)kCtMaxWordBytes) return 1;
            while ((int)(text.size() & 3) != phase) text.push_back((uint8_t)poison);
            ta.push_back((int64_t)text.size());
            text.insert(text.end(), w.begin(), w.end());
            te.push_back((int64_t)text.size());
        }
        const size_t n_dwords = (text.size() + 3) / 4;           // up to the dword of the last byte, no further
        std::vector<uint32_t> dwords(n_dwords, 0x01010101u * poison);
        memcpy(dwords.data(), text.data(), text.size());
        const uint32_t* tp = dwords.data();
        auto ld = [tp, n_dwords](int64_t i) -> uint32_t {
            if (i < 0 || (size_t)i >= n_dwords) { __atomic_store_n(&g_bad, 2, __ATOMIC_RELAXED); return 0xDEADBEEFu; }
            return tp[i];
        };
        const uint32_t* bp = blob.data();
        const size_t blob_n = blob.size();
        auto bl = [bp, blob_n](uint64_t i) -> uint32_t {
            if (i >= blob_n) { __atomic_store_n(&g_bad, 3, __ATOMIC_RELAXED); return 0xDEADBEEFu; }
            return bp[i];
        };
        uint64_t* sp = slots.data();
        uint64_t* cp = counts.data();
        const uint64_t n_slots = slots.size();
        std::vector<int64_t> got((size_t)n, -2);
        std::vector<long> loads((size_t)n, 0);
        long counted = 0, dropped = 0;
        auto enter = [&](long i, bool note) {
            const uint32_t h = th_hash_lane(ld, ta[i], te[i], seed);
            tl_loads = 0;
            const int64_t s = ct_find_or_insert<HostAtomics>(ld, ta[i], te[i], h, sp, bl, n_slots, probe_max);
            if (note) { got[i] = s; loads[i] = tl_loads; }
            if (s == kCtDropped) __atomic_fetch_add(&dropped, 1, __ATOMIC_RELAXED);
            else {
                __atomic_fetch_add(&counted, 1, __ATOMIC_RELAXED);
                __atomic_fetch_add(cp + s, 1ull, __ATOMIC_RELAXED);
            }
        };
        if (threads <= 1) {
            for (long i = 0; i < n; ++i) enter(i, true);
            for (long i = 0; i < n; ++i) printf("%lld %ld\n", (long long)got[i], loads[i]);
        } else {
            std::vector<std::thread> pool;
            for (int t = 0; t < threads; ++t)
                pool.emplace_back([&, t] {
                    const long first = (long)t * n / threads;
                    for (long k = 0; k < n; ++k) enter((first + k) % n, false);
                });
            for (std::thread& th : pool) th.join();
        }
        // the commit: (a) the padded dwords of the fresh slots, (b) their bytes into the blob, resident words stored
        uint64_t need = 0, fresh = 0;
        for (const uint64_t v : slots)
            if (ct_is_fresh(v)) { need += ct_padded_dwords(v); ++fresh; }
        uint64_t at = blob.size();
        blob.resize(blob.size() + need, 0xDEADBEEFu);
        uint32_t* bw = blob.data();
        const size_t blob_new = blob.size();
        for (uint64_t& v : slots)
            if (ct_is_fresh(v)) {
                const uint32_t nd = ct_padded_dwords(v);
                v = ct_commit_word(ld, v, at, [bw, blob_new](uint64_t i, uint32_t w) {
                    if (i >= blob_new) { g_bad = 3; return; }
                    bw[i] = w;
                });
                at += nd;
            }
        printf("batch counted %ld dropped %ld fresh %llu blob %zu\n", counted, dropped, (unsigned long long)fresh, blob.size());
    }
    return g_bad;
}
