// api.cpp -- host side of liblatok_hip.so: the C ABI declared in include/latok_hip.h.
//
// Thin by design: argument checks, workspace management, H2D/D2H staging for host-pointer calls, and the launch
// sequence of the pipeline (tile index -> tiles -> resolve/repair).  No compute happens on the
// host and there is no CPU fallback: without a HIP device every compute entry point fails.
#include <hip/hip_runtime.h>
#include <errno.h>
#include <fcntl.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <array>
#include <atomic>
#include <chrono>
#include <initializer_list>
#include <mutex>
#include <new>
#include <optional>
#include <string>
#include <thread>
#include <vector>

#include "../../include/latok_hip.h"
#include "corpus_gen.h"
#include "flow_hazards.h"
#include "kernels.h"
#include "unicode_tables.inc"
#include "vocab_table.h"
#include "chargram_text.h"
#include "ngram_text.h"
#include "count_table.h"
#include "wordpiece.h"
#include "bpe.h"
#include "unigram.h"
#include "pretok.h"
#include "spbpe.h"
#include "fold_map.h"
#include "fold_tables.inc"
#include "tfidf_weight.h"

static_assert(LATOK_TBL_SHIFT == latok::kTblShift, "table shift");
static_assert(LATOK_TBL_STAGE1_LEN == latok::kStage1Len, "stage-1 length");
static_assert(LATOK_TBL_NBLOCKS * (1 << LATOK_TBL_SHIFT) == latok::kStage2Len, "stage-2 length");
static_assert(LATOK_TILE_CHARS == latok::kTile, "tile size");
static_assert(LATOK_PRETOK_LATOK == kPretokLatok && LATOK_PRETOK_GPT2 == kPretokGpt2 && LATOK_PRETOK_CL100K == kPretokCl100k && LATOK_PRETOK_SPM == kPretokSpm,
              "pre-tokenizer constants");

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
#define HIP_TRY(expr)                                                                                     \
    do {                                                                                                  \
        hipError_t e_ = (expr);                                                                           \
        if (e_ != hipSuccess) return fail(LATOK_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    unsigned gen = 0;   // counts (re)allocations: fresh memory holds anything
    int ensure(size_t bytes) {
        if (bytes <= cap) return LATOK_OK;
        ++gen;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            p = nullptr;
            return fail(LATOK_ERR_NOMEM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
        }
        cap = want;
        return LATOK_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
};

// an exact-size device allocation with one owner, freed with it: what the long-lived objects (vocab, WordPiece, idf, counter) hold
struct DevMem {
    void* p = nullptr;
    DevMem() = default;
    DevMem(DevMem&& o) noexcept : p(std::exchange(o.p, nullptr)) {}
    DevMem& operator=(DevMem&& o) noexcept {
        if (p && p != o.p) (void)hipFree(p);
        p = std::exchange(o.p, nullptr);
        return *this;
    }
    ~DevMem() {
        if (p) (void)hipFree(p);
    }
    hipError_t alloc(size_t bytes) {   // of an empty one
        const hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) p = nullptr;
        return e;
    }
    template <class T>
    T* as() const {
        return static_cast<T*>(p);
    }
};

// slots + padded words of one vocab_table.h table on the device
struct DevTable {
    DevMem slots, blob;   // VtSlot[n_slots], the padded words
    uint64_t n_slots = 0;
    // allocates, then enqueues the two copies on `st`: the caller waits for `st` before `t` dies
    int upload(const VtTable& t, hipStream_t st) {
        const size_t slot_bytes = t.slots.size() * sizeof(VtSlot), blob_bytes = t.blob.size() * 4;
        n_slots = t.slots.size();
        hipError_t e = slots.alloc(slot_bytes);
        if (e == hipSuccess) e = blob.alloc(blob_bytes);
        if (e != hipSuccess) return fail(LATOK_ERR_NOMEM, "hipMalloc(%zu) failed: %s", slot_bytes + blob_bytes, hipGetErrorString(e));
        e = hipMemcpyAsync(slots.p, t.slots.data(), slot_bytes, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(blob.p, t.blob.data(), blob_bytes, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return fail(LATOK_ERR_HIP, "uploading the vocabulary failed: %s", hipGetErrorString(e));
        return LATOK_OK;
    }
    latok::VocabTable view(uint32_t seed) const { return latok::VocabTable{slots.p, blob.as<const uint32_t>(), n_slots, seed}; }
};

// pinned, device-mapped host memory: small host-pointer calls stage their inputs here and have the kernels read and
// write it in place over the bus, so that a call costs launches + ONE synchronisation instead of five blocking copies
struct PinBuf {
    void* h = nullptr;   // host address
    void* d = nullptr;   // the same memory as the device sees it
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return LATOK_OK;
        release();
        const size_t want = bytes + bytes / 4 + 4096;
        hipError_t e = hipHostMalloc(&h, want, hipHostMallocMapped);
        if (e == hipSuccess) e = hipHostGetDevicePointer(&d, h, 0);
        if (e != hipSuccess) {
            release();
            return fail(LATOK_ERR_NOMEM, "hipHostMalloc(%zu) failed: %s", want, hipGetErrorString(e));
        }
        memset(h, 0, want);
        cap = want;
        return LATOK_OK;
    }
    void release() {
        if (h) (void)hipHostFree(h);
        h = d = nullptr;
        cap = 0;
    }
};

// Small-batch completion: the kernel stores a sequence number into pinned memory after its last output and the host
// polls that word -- the end-of-kernel signal takes ~10 us longer to come back through the runtime than the data does.
// Bounded: after kPollNs without the word (first launch of a code object, a busy stream, a faulted kernel) the caller
// falls back to hipStreamSynchronize, which also surfaces errors.  LATOK_SMALL_POLL=0 turns polling off.
constexpr long long kPollNs = 200000;
static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    __asm__ __volatile__("yield");
#else
    __asm__ __volatile__("" ::: "memory");
#endif
}
static bool poll_completion() {
    static const bool on = [] { const char* e = getenv("LATOK_SMALL_POLL"); return !(e && e[0] == '0'); }();
    return on;
}
static bool wait_completion_word(const unsigned long long* word, unsigned long long seq) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        for (int i = 0; i < 256; ++i) {
            if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == seq) return true;
            cpu_relax();
        }
        if (std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count() > kPollNs) return false;
    }
}

static inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

// host-pointer calls up to this size take the pinned zero-copy path: the arrays are copied into pinned mapped memory by
// the host and the kernels read / write them over the bus, including the binary searches over row_off.  Measured against
// the staged-copy path (tools/batch_size_sweep.py, offsets of strings of ~105 chars, us per call): 16 K chars 70 / 112,
// 54 K 60 / 120, 108 K 75 / 137; the two meet near 1 M chars, where the host's own memcpy into the pinned area is what
// the call costs either way.
constexpr int64_t kSmallChars = 262144;
constexpr int64_t kSmallStrings = 16384;

// The input form of a batch as the tile kernel reads it: UTF-32 code points, PEP 393 kind 1 / 2 code units (positions are
// chars) or UTF-8 bytes (positions are bytes).  Code-point positions of a UTF-8 batch are not a kernel form: the blocking calls
// (cp_units_route, latok_split_mask_utf8_batch) reach them through byte space (enqueue_lead_front) or the decoder, flow_submit_utf8
// through byte space alone.
enum class Form { Utf32, Latin1, Ucs2, Utf8 };
struct Input {
    const void* p = nullptr;
    Form form = Form::Utf32;
    size_t width() const { return form == Form::Utf32 ? 4 : form == Form::Ucs2 ? 2 : 1; }   // bytes per unit
    bool narrow() const { return form == Form::Latin1 || form == Form::Ucs2; }
};
// the public PEP 393 kind (1 / 2 / 4, checked by the caller) or the flow's 0 (UTF-8 bytes)
static Form form_of_kind(int kind) { return kind == 4 ? Form::Utf32 : kind == 2 ? Form::Ucs2 : kind == 1 ? Form::Latin1 : Form::Utf8; }
// a CSR batch: units, row offsets [n_str + 1] and the total, both counted in units
struct Batch {
    Input in;
    const int64_t* row = nullptr;
    int64_t n_str = 0, total = 0;
};

// The device buffers of one batch in flight and the state of its chained scan: the context's own calls share one set, every
// flow slot has another.
struct Workspace {
    DevBuf summ, seg_agg, fix_count, tile_first;   // tile stage (run_pipeline)
    DevBuf bits, space, kept, wcnt, wpref, bases, scalar, chain, chain_ctl;   // compaction passes (enqueue_compaction_dev)
    DevBuf codes, widened;                          // featurize: rule code of every char, PEP 393 units widened to UTF-32
    // code-point results of a UTF-8 batch from byte space (enqueue_lead_front, blocking calls and flow alike): lead-byte mask and
    // SPACE plane over the bytes, the packed code-point masks, the code-point row offsets
    DevBuf lead, bspace, cpbits, cpspace, cprow;
    DevBuf jbody, jhead;   // joined token text: the body / head planes over the bytes (k_join_counts)
    DevBuf tkeys, tkeys2, trows;   // term counts: one key per token, the long rows' second buffer, five int64 arrays over the rows
    DevBuf wpspans, wpcnt, wprank, wpids;   // WordPiece: per token its span record, piece count and piece rank; the padded form's ids
    DevBuf bpemask;   // BPE (which uses the WordPiece buffers as well): per token of at most 64 bytes its final part-start mask
    DevBuf unimarks;   // Unigram (which uses the WordPiece buffers as well): per token of at most 64 bytes three words of the count pass
    DevBuf ngrows;   // word n-grams: gram counts and row starts in key space (the span records share wpspans, the keys tkeys / tkeys2)
    DevBuf tfptr, tfidx, tfval, tfctl;   // TF-IDF: a host caller's CSR on the device (indptr, indices, data) and the error word of k_csr_check
    // decoding (which stages a host caller's rows and ids in tfptr / tfidx and keeps its error word and unknown tally in tfctl): output
    // bytes per piece, the sum and the first output byte of every workgroup of pieces, the int64 row starts of an int32 indptr
    DevBuf dtcnt, dtsum, dtrank, dtrows;
    // the single-pass scan of k_word_counts_scan keeps its look-back state (chain: per workgroup, chain_ctl: {ticket
    // counter}) between launches: entries carry an epoch, so the array is cleared only when it is (re)allocated or when the
    // 18-bit epoch wraps (next_scan_epoch); *_seen = DevBuf::gen of the allocations it was last cleared in
    unsigned scan_epoch = 0, chain_seen = 0, chain_ctl_seen = 0;
    bool chain_ready = false;
    void release() {
        for (DevBuf* b : {&summ, &seg_agg, &fix_count, &tile_first, &bits, &space, &kept, &wcnt, &wpref, &bases, &scalar, &chain,
                          &chain_ctl, &codes, &widened, &lead, &bspace, &cpbits, &cpspace, &cprow, &jbody, &jhead, &tkeys,
                          &tkeys2, &trows, &wpspans, &wpcnt, &wprank, &wpids, &bpemask, &unimarks, &ngrows, &tfptr, &tfidx, &tfval, &tfctl, &dtcnt, &dtsum, &dtrank, &dtrows})
            b->release();
        scan_epoch = chain_seen = chain_ctl_seen = 0;
        chain_ready = false;
    }
};
struct WsNeed {
    DevBuf* buf;
    size_t bytes;   // 0: the batch does not use the buffer
};
constexpr int kTileNeeds = 4;   // the first entries of ws_needs: the tile stage
constexpr int kWsNeeds = 40;
// What a batch asks of its workspace beyond the tile stage.  token spans (spans) add the SPACE and kept planes, featurize (feats)
// the code bytes, and narrow units read by featurize (widen) a UTF-32 copy.  cp_rows > 0: the units are UTF-8 bytes whose results
// are reported in code points (cp_rows = n_str + 1): every buffer is sized by the byte count, which bounds the code-point count.
// join: the two planes of the joined token text (UTF-8 bytes, with spans).  term_rows > 0 (= n_str + 1): term counts -- the row
// arrays and a scan state that also serves a scan over the rows; term_tokens: the batch's token total, which the term-count call
// waits for before it sizes the two key buffers.  wp_tokens: the token total again, for the WordPiece calls (which use the first two
// row arrays of term_rows): 16 bytes of span record, 8 of piece count and 8 of piece rank per token, one entry more in the last two,
// and a scan state for that many entries; wp_pieces: the piece total, which the padded form waits for before it sizes its ids.
// bpe_tokens: the token total once more, for the BPE calls (which set wp_tokens too): 8 bytes of part-start mask per token.
// uni_tokens: the same for the Unigram calls: 24 bytes per token (the piece starts, the unknown pieces, the marker piece's flag).
// Word n-grams (which use the row arrays of term_rows as well): ng_tokens, the token total: 16 bytes of span record per token, in the
// buffer the WordPiece calls keep theirs in; ng_rows > 0 (= n_str + 1): the gram counts and the row starts in key space; ng_keys:
// the key total, which the n-gram call waits for before it sizes the two key buffers -- the term counts' own, one key per gram.
// TF-IDF: tf_ctl, the error word of the CSR check; tf_ptr_bytes / tf_entries: the staging of a host caller's CSR (latok_idf_update_csr,
// latok_tfidf_csr) -- its indptr in the caller's width, one int32 index and one 4-byte value per entry.
// Decoding (latok_detok_csr / _padded, which set the TF-IDF fields for their own staging): dt_cells, the pieces -- 4 bytes of count per
// piece, 8 + 8 bytes per workgroup of kDetokBlock pieces and a scan state for that many sums; dt_rows > 0 (= n_rows + 1): the int64 row
// starts of an int32 indptr.
constexpr int kTermRowArrays = 5;   // token counts, row starts, distinct counts, indptr, OOV counts
struct WsShape {
    bool spans = false, feats = false, widen = false, join = false;
    int64_t cp_rows = 0;
    int64_t term_rows = 0, term_tokens = 0;
    int64_t wp_tokens = 0, wp_pieces = 0;
    int64_t bpe_tokens = 0;
    int64_t uni_tokens = 0;
    int64_t ng_tokens = 0, ng_rows = 0, ng_keys = 0;
    bool tf_ctl = false;
    int64_t tf_ptr_bytes = 0, tf_entries = 0;
    int64_t dt_cells = 0, dt_rows = 0;
};
// The one sizing rule of a workspace: every buffer a batch of `units` positions uses and its byte size.
static std::array<WsNeed, kWsNeeds> ws_needs(Workspace& w, int64_t units, const WsShape& shape) {
    const bool spans = shape.spans, feats = shape.feats, widen = shape.widen, join = shape.join;
    const int64_t cp_rows = shape.cp_rows;
    const size_t t = (size_t)std::max<int64_t>((units + latok::kTile - 1) / latok::kTile, 1);
    const size_t words = (size_t)((units + 63) / 64), c_tiles = (words + 63) / 64;
    return {{{&w.summ, t * 16},   // (also the cl100k front's carry records, 4 bytes per tile: that front never runs the tile stage)
             // one Fn64 + Hd64 pair per segment; plan_segments never makes a segment shorter than kWPB tiles (unless it is the
             // only one), so n_segs <= t / kWPB + 1
             {&w.seg_agg, (t / latok::kWPB + 2) * (sizeof(latok::Fn64) + sizeof(latok::Hd64))},
             {&w.fix_count, 8},
             {&w.tile_first, t * 8 + 8},   // per-tile string index (stage 0)
             {&w.bits, words * 8 + 8},
             {&w.space, spans ? words * 8 + 8 : 0},
             {&w.kept, spans ? words * 8 + 8 : 0},
             {&w.wcnt, c_tiles * 8 + 8},    // items per tile
             {&w.wpref, words * 2 + 8},     // items of the tile before each word
             {&w.bases, c_tiles * 8 + 8},   // rank of each tile's first item
             {&w.scalar, 64},
             {&w.chain, (size_t)std::max({latok::count_blocks((int64_t)words), latok::count_blocks(shape.term_rows * 64),
                                            latok::count_blocks(shape.wp_tokens > 0 ? (shape.wp_tokens + 1) * 64 : 0),
                                            latok::count_blocks(latok::detok_groups(shape.dt_cells) * 64)}) * 8 + 64},
             {&w.chain_ctl, 64},
             {&w.codes, feats ? (size_t)units + latok::kTile + 256 : 0},   // read (never used) up to a tile behind the last char
             {&w.widened, widen ? (size_t)units * 4 + 16 : 0},
             {&w.lead, cp_rows > 0 ? words * 8 + 8 : 0},
             {&w.bspace, cp_rows > 0 && spans ? words * 8 + 8 : 0},
             {&w.cpbits, cp_rows > 0 ? words * 8 + 8 : 0},
             {&w.cpspace, cp_rows > 0 && spans ? words * 8 + 8 : 0},
             {&w.cprow, cp_rows > 0 ? (size_t)cp_rows * 8 : 0},
             {&w.jbody, join ? words * 8 + 8 : 0},
             {&w.jhead, join ? words * 8 + 8 : 0},
             {&w.tkeys, (size_t)std::max<int64_t>({shape.term_tokens, shape.ng_keys, 0}) * 8},
             {&w.tkeys2, (size_t)std::max<int64_t>({shape.term_tokens, shape.ng_keys, 0}) * 8},
             {&w.trows, shape.term_rows > 0 ? (size_t)shape.term_rows * 8 * kTermRowArrays : 0},
             {&w.wpspans, (size_t)std::max<int64_t>({shape.wp_tokens, shape.ng_tokens, 0}) * 16},
             {&w.ngrows, shape.ng_rows > 0 ? (size_t)shape.ng_rows * 8 * 2 : 0},
             {&w.wpcnt, shape.wp_tokens > 0 ? (size_t)(shape.wp_tokens + 1) * 8 : 0},
             {&w.wprank, shape.wp_tokens > 0 ? (size_t)(shape.wp_tokens + 1) * 8 : 0},
             {&w.wpids, shape.wp_pieces > 0 ? (size_t)shape.wp_pieces * 4 : 0},
             {&w.bpemask, shape.bpe_tokens > 0 ? (size_t)shape.bpe_tokens * 8 : 0},
             {&w.unimarks, shape.uni_tokens > 0 ? (size_t)shape.uni_tokens * 24 : 0},
             {&w.tfptr, (size_t)shape.tf_ptr_bytes},
             {&w.tfidx, shape.tf_entries > 0 ? (size_t)shape.tf_entries * 4 + 16 : 0},
             {&w.tfval, shape.tf_entries > 0 ? (size_t)shape.tf_entries * 4 + 16 : 0},
             {&w.tfctl, shape.tf_ctl ? (size_t)64 : 0},
             {&w.dtcnt, shape.dt_cells > 0 ? (size_t)shape.dt_cells * 4 + 16 : 0},
             {&w.dtsum, shape.dt_cells > 0 ? (size_t)latok::detok_groups(shape.dt_cells) * 8 + 16 : 0},
             {&w.dtrank, shape.dt_cells > 0 ? (size_t)latok::detok_groups(shape.dt_cells) * 8 + 16 : 0},
             {&w.dtrows, shape.dt_rows > 0 ? (size_t)shape.dt_rows * 8 : 0}}};
}
static int ws_ensure(const WsNeed* needs, int n) {
    for (int i = 0; i < n; ++i) {
        const int rc = needs[i].buf->ensure(needs[i].bytes);
        if (rc) return rc;
    }
    return LATOK_OK;
}

// One context = one device, one stream, one set of tables / workspaces / staging buffers, one rule-table state and one
// lock.  Calls on the same context are serialised by its lock; calls on different contexts (other devices, or the same
// device twice) share nothing and run concurrently.  Every entry point works on the calling thread's CURRENT context
// (latok_ctx_set_current; default: the process-wide one that latok_init creates) -- the same model as hipSetDevice.
struct Ctx {
    std::mutex mu;
    bool inited = false;
    int device = -1, n_cu = 0;
    hipStream_t stream = nullptr;
    // tables
    DevBuf t1, t1rule, t2code, t2cls, cw;
    DevBuf tb6, tb6rule;   // byte space: its own class table, split codes / rule codes (build_byte_tables)
    // case folding (latok_fold_utf8_bytes_batch): the tables of fold_map.h, uploaded by the context's first fold call; the string-end
    // bitmap and the group prefixes of the batch in hand
    DevBuf fold_tab, fold_start, fold_pref;
    FoldTables fold_t;
    bool fold_ready = false;
    // runtime rule tables (latok_set_rules); off = the built-in default_tokenizer.py tables
    bool rules_on = false;
    lk_rule_tables rules;
    Workspace ws;                  // the workspace of the context's own calls
    DevBuf& h_cps = ws.widened;    // UTF-32 staging of host-pointer calls: the same memory as the workspace's widened units
    // staging for host-pointer calls and for the offsets API
    DevBuf h_row, h_out, counts, scan_tot, h_aux;
    PinBuf pin, pin_tot;   // pin_tot: 64 bytes the scans drop their grand totals into (read after a stream sync, no copy)
    unsigned long long small_seq = 0;   // completion word of the single-launch small-batch path (pin_tot word 2)
    DevBuf done_ctr;                    // workgroup counter of latok::DoneSignal (0 between launches)
    std::vector<uint32_t> hd_cps;       // host decode of small UTF-8 batches (host_decode_small)
    std::vector<int64_t> hd_row, hd_pos;
    unsigned done_ctr_seen = 0;
    DevBuf u_bytes, u_boff, u_cnt, u_row, u_pref;   // UTF-8 ingest: uploaded bytes / byte offsets, per-string cp counts, cp offsets
    // chunked host pipeline (compact_host_pipelined): copy streams, events and double buffers
    hipStream_t s_h2d = nullptr, s_d2h = nullptr;
    hipEvent_t ev_in_ready[2] = {nullptr, nullptr}, ev_k_done[2] = {nullptr, nullptr}, ev_d2h_done[2] = {nullptr, nullptr};
    DevBuf pipe_in[2], pipe_row[2], pipe_counts[2], pipe_items[2], pipe_feat[2];
    PinBuf pipe_tot;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    // batch flow (latok_flow_*): up to kFlowSlots device-resident batches in flight, each with its own stream and workspace
    struct FlowSlot {
        Workspace ws;
        hipStream_t st = nullptr;
    };
    static constexpr int kFlowSlots = 4;
    FlowSlot flow[kFlowSlots];
    int flow_slots = 2;                  // slots in use
    bool flow_ready = false;
    unsigned long long flow_seq = 0;     // batches submitted so far
    latok::FlowHazards flow_held;        // memory ranges of the batches in flight, per slot (flow_hazards.h)
    const uint32_t* bench_cps_b = nullptr;   // latok_bench_set_second_input: what the odd steps of the flow measurements read
    const int64_t* bench_row_b = nullptr;
    hipEvent_t turn_event = nullptr;     // recorded behind the last kernel of every call (StreamTurn)
    hipStream_t turn_stream = nullptr;
    bool turn_stream_valid = false;
    // test hooks: latok_debug_set_plan_cus (0 = the device's own CU count), what the last run_pipeline launched and the route the
    // last compaction call took (latok_debug_last_route)
    int plan_cus = 0;
    latok::PlanForce plan_force;         // latok_debug_set_tile_plan
    int last_route = 0;
    struct LastPlan {
        latok::LaunchPlan plan{};
        int64_t n_tiles = 0;
        int mode = 0;
        bool small = false, valid = false;
        const int64_t* fix_count = nullptr;
        hipStream_t st = nullptr;
    } last;
};
Ctx g_default;                       // latok_init / latok_shutdown
thread_local Ctx* tl_ctx = nullptr;  // latok_ctx_set_current; nullptr = g_default
Ctx* current_ctx() { return tl_ctx ? tl_ctx : &g_default; }

// HIP's current device is per host thread: whatever thread a call arrives on, allocations, events and launches of a
// context must happen with ITS device current (a worker thread starts on device 0).  Restores the caller's device.
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(const Ctx& c) {
        if (c.inited && hipGetDevice(&prev) == hipSuccess && prev != c.device) switched = hipSetDevice(c.device) == hipSuccess;
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
};
#define LATOK_ENTER()                        \
    Ctx& g = *current_ctx();                 \
    std::lock_guard<std::mutex> lk(g.mu);    \
    DeviceGuard device_guard_(g)


int need_init(const Ctx& g) {
    if (!g.inited) return fail(LATOK_ERR_NOT_INIT, "latok_init() has not been called (no CPU fallback exists)");
    return LATOK_OK;
}

// The workspaces (tile summaries, bitmasks, ranks, staging) are shared by all calls of a context.  Host calls are serialised by its lock,
// but with caller streams the kernels of two calls could still overlap on the device: a call that runs on another
// stream than the previous one first waits (on the device) for that call's last kernel.
struct StreamTurn {
    Ctx& g;
    hipStream_t st;
    StreamTurn(Ctx& ctx, void* stream) : g(ctx), st(stream ? (hipStream_t)stream : ctx.stream) {
        if (g.inited && g.turn_event && g.turn_stream_valid && g.turn_stream != st)
            (void)hipStreamWaitEvent(st, g.turn_event, 0);
    }
    ~StreamTurn() {
        if (g.inited && g.turn_event) {
            (void)hipEventRecord(g.turn_event, st);
            g.turn_stream = st;
            g.turn_stream_valid = true;
        }
    }
};

// LATOK_ONE_SEGMENT=0 in the environment: small batches take the three-launch pipeline too (A/B, tests)
static bool one_segment_enabled() {
    static const bool on = [] { const char* e = getenv("LATOK_ONE_SEGMENT"); return !(e && e[0] == '0'); }();
    return on;
}

// One launch sequence of the tile pipeline on device-resident data.  Every field but the batch and the stream is optional.
struct Pipe {
    Batch b;                          // (the block mask has no units: its planes are bm_a1 / bm_a2)
    int mode = latok::kModeBits;      // kModeBits / kModeValues / kModeBlockMask; the form of a non-UTF-32 batch picks the bitmask variant
    uint64_t* bits = nullptr;
    uint8_t* values = nullptr;
    uint64_t* space = nullptr;        // also the SPACE plane (token spans)
    uint64_t* lead = nullptr;         // byte space: also the lead-byte mask, the leads of a tile before each word and the leads
    uint16_t* lead_pref = nullptr;    // per tile (code-point results, enqueue_lead_front)
    int64_t* lead_cnt = nullptr;
    uint8_t* codes = nullptr;         // also the rule code of every char (featurize)
    const int8_t* bm_a1 = nullptr;    // kModeBlockMask: the two planes and {any(a1), any(a2)}
    const int8_t* bm_a2 = nullptr;
    const int* bm_flags = nullptr;
    int stages = 7;                   // 1 = tile index, 2 = tiles, 4 = resolve
    latok::DoneSignal done{nullptr, 0, nullptr};   // completion word stored by the last launch
    hipEvent_t tiles_begin = nullptr, tiles_end = nullptr;
    hipStream_t st = nullptr;
};

// enqueue the pipeline on workspace `w` (the context's own, or a flow slot's: flow_reserve sized it before anything was enqueued)
int run_pipeline(Ctx& g, Workspace& w, const Pipe& a) {
    const int64_t n_str = a.b.n_str, total = a.b.total;
    if (total <= 0 || n_str <= 0) return LATOK_OK;
    const Input& in = a.b.in;
    int mode = a.mode;
    if (in.form != Form::Utf32) {   // byte space: UTF-8 bytes in, positions are bytes; or PEP 393 code units, positions are chars
        if (mode != latok::kModeBits) return fail(LATOK_ERR_INVALID, "byte-space input supports the bitmask outputs only");
        if (((uintptr_t)in.p & 15) != 0)
            return fail(LATOK_ERR_INVALID, in.narrow() ? "device code-unit pointer must be 16-byte aligned" : "device UTF-8 pointer must be 16-byte aligned");
        mode = in.form == Form::Latin1 ? latok::kModeLatin1 : (in.form == Form::Ucs2 ? latok::kModeUcs2 : latok::kModeBytes);
    }
    // run-time rule tables (latok_set_rules): the same input form, rules interpreted from the kernel arguments
    if (g.rules_on && mode != latok::kModeBlockMask) mode = latok::mode_with_rules(mode);
    const int64_t n_tiles = (total + latok::kTile - 1) / latok::kTile;
    int rc = ws_ensure(ws_needs(w, total, WsShape{}).data(), kTileNeeds);
    if (rc) return rc;
    latok::SplitParams P;
    P.cps = in.form == Form::Utf32 ? (const uint32_t*)in.p : nullptr;
    P.u8 = in.form == Form::Utf32 ? nullptr : (const uint8_t*)in.p;
    P.row_off = a.b.row;
    P.n_str = n_str;
    P.total = total;
    P.n_tiles = n_tiles;
    // (the CU share of a batch of a flow, the segment plan and the kernel variants: latok::plan_launch)
    const int n_cu = g.plan_cus > 0 ? g.plan_cus : g.n_cu;   // latok_debug_set_plan_cus: plan and launch as if the chip had n_cu CUs
    const bool one_launch_ok = a.stages == 7 && in.form == Form::Utf32 && !a.tiles_begin && !a.tiles_end && one_segment_enabled();
    latok::LaunchPlan L;
    latok::plan_launch(n_tiles, n_cu, &w != &g.ws, mode, one_launch_ok, &L, &g.plan_force);
    P.seg_tiles = L.seg_tiles;
    P.n_segs = L.n_segs;
    const bool one_launch = L.one_launch != 0;
    if ((size_t)P.n_segs * (sizeof(latok::Fn64) + sizeof(latok::Hd64)) > w.seg_agg.cap || (size_t)n_tiles * 16 > w.summ.cap)
        return fail(LATOK_ERR_INVALID, "internal: workspace too small for %lld segments / %lld tiles", (long long)P.n_segs, (long long)n_tiles);
    if (a.codes && mode != latok::kModeBits && mode != latok::kModeRules)
        return fail(LATOK_ERR_INVALID, "internal: code bytes are written by the UTF-32 bitmask modes only");
    // rule codes (split code + NUM) when the rules are interpreted at run time or the code bytes are kept for featurize
    const uint8_t* tables = (const uint8_t*)((latok::mode_rules(mode) || a.codes) ? g.t1rule.p : g.t1.p);
    P.t1 = tables;
    P.t2 = tables + latok::kStage1Pad;
    if (latok::mode_base(mode) == latok::kModeBytes) {   // (byte space classifies through its own table, cut at 6 bits)
        P.t1 = (const uint8_t*)(latok::mode_rules(mode) ? g.tb6rule.p : g.tb6.p);
        P.t2 = P.t1 + latok::kB6Stage1Bytes;
    }
    if (latok::mode_rules(mode)) P.rules = g.rules;
    else memset(&P.rules, 0, sizeof(P.rules));
    P.bits_out = a.bits;
    P.values_out = a.values;
    P.space_out = a.space;
    P.lead_out = a.lead;
    P.lead_pref_out = a.lead_pref;
    P.lead_cnt_out = a.lead_cnt;
    P.codes_out = a.codes;
    P.tile_first = (int64_t*)w.tile_first.p;   // the per-tile string index lives in the workspace
    P.summ = (int4*)w.summ.p;
    P.seg_fn = (latok::Fn64*)w.seg_agg.p;
    P.seg_hd = (latok::Hd64*)((char*)w.seg_agg.p + (size_t)P.n_segs * sizeof(latok::Fn64));
    P.fix_count = (int64_t*)w.fix_count.p;
    P.bm_a1 = a.bm_a1;
    P.bm_a2 = a.bm_a2;
    P.bm_flags = a.bm_flags;
    P.done = (a.stages & 4) ? a.done : latok::DoneSignal{nullptr, 0, nullptr};
    // what is launched, for latok_debug_last_plan (a few stores)
    g.last.plan = L;
    g.last.n_tiles = n_tiles;
    g.last.mode = mode;
    g.last.small = g.pin.d && in.p == g.pin.d;
    g.last.fix_count = (const int64_t*)w.fix_count.p;
    g.last.st = a.st;
    g.last.valid = true;
    const hipStream_t st = a.st;
    if (one_launch) {
        HIP_TRY(latok::launch_one_segment(P, mode, st));
        return LATOK_OK;
    }
    if (a.stages & 1) HIP_TRY(latok::launch_tile_index(P, st));   // (the kernel-timing loop of latok_bench_split_mask launches stage 1 alone)
    if (a.tiles_begin) HIP_TRY(hipEventRecord(a.tiles_begin, st));
    if (a.stages & 2) HIP_TRY(latok::launch_split_tiles(P, mode, L, st));
    if (a.tiles_end) HIP_TRY(hipEventRecord(a.tiles_end, st));
    if (a.stages & 4) HIP_TRY(latok::launch_resolve_fix(P, mode, L, st));
    return LATOK_OK;
}

int check_csr_host(const int64_t* row_off, int64_t n_str, int64_t* total_io) {
    if (n_str < 0) return fail(LATOK_ERR_INVALID, "n_str must be >= 0");
    if (n_str == 0) { *total_io = 0; return LATOK_OK; }
    if (!row_off) return fail(LATOK_ERR_INVALID, "row_off is NULL");
    if (row_off[0] != 0) return fail(LATOK_ERR_INVALID, "row_off[0] must be 0");
    for (int64_t s = 0; s < n_str; ++s)
        if (row_off[s + 1] < row_off[s]) return fail(LATOK_ERR_INVALID, "row_off must be non-decreasing");
    if (*total_io >= 0 && *total_io != row_off[n_str])
        return fail(LATOK_ERR_INVALID, "total_chars does not match row_off[n_str]");
    *total_io = row_off[n_str];
    return LATOK_OK;
}

int resolve_total_device(const int64_t* d_row, int64_t n_str, int64_t* total_io, hipStream_t st) {
    if (n_str < 0) return fail(LATOK_ERR_INVALID, "n_str must be >= 0");
    if (n_str == 0) { *total_io = 0; return LATOK_OK; }
    if (*total_io < 0) {
        HIP_TRY(hipMemcpyAsync(total_io, d_row + n_str, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return LATOK_OK;
}

// the total of a call's batch, once per call: read from device row offsets when the caller passed total < 0 (one blocking
// 8-byte read), checked against host row offsets
int resolve_total(const int64_t* row_off, int64_t n_str, int64_t* total_io, bool dev, hipStream_t st) {
    return dev ? resolve_total_device(row_off, n_str, total_io, st) : check_csr_host(row_off, n_str, total_io);
}

// Completion word of the pinned small path: the last launch stores done->seq into pin_tot word 2, which the host polls
// (wait_done) instead of waiting for the stream.  done->word stays NULL when polling is off.
int arm_done(Ctx& g, hipStream_t st, latok::DoneSignal* done) {
    *done = latok::DoneSignal{nullptr, 0, nullptr};
    if (!poll_completion()) return LATOK_OK;
    int rc;
    if ((rc = g.pin_tot.ensure(64)) || (rc = g.done_ctr.ensure(64))) return rc;
    if (g.done_ctr.gen != g.done_ctr_seen) {
        g.done_ctr_seen = g.done_ctr.gen;
        HIP_TRY(hipMemsetAsync(g.done_ctr.p, 0, 64, st));
    }
    *done = latok::DoneSignal{(unsigned long long*)g.pin_tot.d + 2, ++g.small_seq, (unsigned*)g.done_ctr.p};
    return LATOK_OK;
}
int wait_done(Ctx& g, const latok::DoneSignal& done, hipStream_t st) {
    if (!(done.word && wait_completion_word((const unsigned long long*)g.pin_tot.h + 2, done.seq))) HIP_TRY(hipStreamSynchronize(st));
    return LATOK_OK;
}

// the batch on the device: the caller's device pointers as they are, or a host batch of narrow units / UTF-8 bytes copied
// into u_bytes / u_boff
int units_on_device(Ctx& g, const Batch& b, bool dev, hipStream_t st, Batch* d) {
    *d = b;
    if (dev) return LATOK_OK;
    int rc;
    const size_t bytes = (size_t)b.total * b.in.width();
    if ((rc = g.u_bytes.ensure(bytes + 16))) return rc;
    if ((rc = g.u_boff.ensure((size_t)(b.n_str + 1) * 8))) return rc;
    if (bytes > 0) HIP_TRY(hipMemcpyAsync(g.u_bytes.p, b.in.p, bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(g.u_boff.p, b.row, (size_t)(b.n_str + 1) * 8, hipMemcpyHostToDevice, st));
    d->in.p = g.u_bytes.p;
    d->row = (const int64_t*)g.u_boff.p;
    return LATOK_OK;
}

// A batch without a unit has no item: all its counts (or row offsets) are zero.  Host memory is cleared in place, device memory
// on the call's stream -- waited for when the caller returns straight away (sync).  Nothing behind a NULL pointer.
int zero_counts(bool dev, void* p, size_t bytes, hipStream_t st, bool sync = false) {
    if (!p || bytes == 0) return LATOK_OK;
    if (!dev) memset(p, 0, bytes);
    else HIP_TRY(hipMemsetAsync(p, 0, bytes, st));
    if (dev && sync) HIP_TRY(hipStreamSynchronize(st));
    return LATOK_OK;
}
int refuse_too_long() { return fail(LATOK_ERR_INVALID, "a string is too long for LATOK_OUT_INT32; use the 64-bit form"); }
// The pinned pair of a blocking call after its one synchronisation: h[0] = the total, h[1] = the scan's own flag (high half) and
// the int32-overflow flag (the bits `o32_mask` of the low half: all of them on the compaction routes, bit 0 for join and hashes,
// whose low half also carries the capacity flag).  A scan that met corrupt look-back state has its state cleared by the next call.
int finish_totals(Workspace& w, const volatile int64_t* h, int64_t o32_mask, int64_t* total_out) {
    if (h[1] >> 32) { w.chain_ready = false; return fail(LATOK_ERR_HIP, "internal: the scan's look-back state was corrupt (the call is safe to repeat)"); }
    if (h[1] & o32_mask) return refuse_too_long();
    *total_out = h[0];
    return LATOK_OK;
}

// The end of a blocking compaction call (offsets, token spans, featurize), behind its totals: `n_items` items were counted.  The
// counts are delivered even when the records do not fit; the records and the feature sums (src_feat NULL: there are none) only
// when they do; the capacity is refused after the copies and their wait.  src_*: where the kernels left them -- pinned memory that the
// host reads (`pinned`: the small path), device staging that is copied down and waited for, or NULL: the caller's device buffers.
int refuse_no_room(int64_t n_items, int64_t items_cap, const void* items_out) {
    if (n_items > items_cap) return fail(LATOK_ERR_INVALID, "output capacity too small: need %lld", (long long)n_items);
    if (n_items > 0 && !items_out) return fail(LATOK_ERR_INVALID, "output buffer is NULL");
    return LATOK_OK;
}
int deliver_records(bool pinned, const void* src_counts, const void* src_items, const void* src_feat, void* counts_out, void* items_out,
                    int8_t* features_out, int64_t n_str, size_t elt, size_t item_bytes, int64_t n_items, int64_t items_cap, hipStream_t st) {
    const bool fits = n_items <= items_cap && (n_items == 0 || items_out);
    const size_t n = fits ? (size_t)n_items : 0;
    if (src_counts && pinned) {
        memcpy(counts_out, src_counts, (size_t)n_str * elt);
        if (n > 0) {
            memcpy(items_out, src_items, n * item_bytes);
            if (src_feat) memcpy(features_out, src_feat, n * LATOK_FEATURE_COUNT);
        }
    } else if (src_counts) {
        HIP_TRY(hipMemcpyAsync(counts_out, src_counts, (size_t)n_str * elt, hipMemcpyDeviceToHost, st));
        if (n > 0) {
            HIP_TRY(hipMemcpyAsync(items_out, src_items, n * item_bytes, hipMemcpyDeviceToHost, st));
            if (src_feat) HIP_TRY(hipMemcpyAsync(features_out, src_feat, n * LATOK_FEATURE_COUNT, hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(hipStreamSynchronize(st));
    }
    return refuse_no_room(n_items, items_cap, items_out);
}

// The frame of a blocking byte-space call on a UTF-8 batch, in two steps with the entry's own checks between them.  The entry keeps
// its flag check, need_init and argument checks ahead of open(), answers the empty batch itself and checks its outputs' alignment
// ahead of stage().  The StreamTurn lives as long as the frame: declare it behind every lock the call takes.
struct BytesCall {
    bool dev = false, o32 = false;
    size_t elt = 8;                       // width of the outputs that follow LATOK_OUT_INT32
    std::optional<StreamTurn> turn;
    hipStream_t st = nullptr;
    int64_t total = 0;                    // the batch's bytes, resolved
    bool empty = true;                    // no string or no byte: nothing is launched
    Batch b;                              // the caller's batch ...
    Batch d;                              // ... and the same on the device (stage)
    volatile int64_t* h_tot = nullptr;    // the context's pinned words as the host sees them (stage) ...
    int64_t* p_tot = nullptr;             // ... and the device
    // host row offsets are checked before the call takes its turn on the stream, device row offsets resolved on it
    int open(Ctx& g, const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes, int flags, void* stream) {
        int rc;
        const bool dev_ptrs = (flags & LATOK_DEVICE_PTRS) != 0;
        if (!dev_ptrs && (rc = check_csr_host(byte_off, n_str, &total_bytes))) return rc;
        turn.emplace(g, stream);
        if (dev_ptrs && (rc = resolve_total_device(byte_off, n_str, &total_bytes, turn->st))) return rc;
        if (total_bytes > 0 && !utf8) return fail(LATOK_ERR_INVALID, "NULL buffer");
        adopt(Batch{Input{utf8, Form::Utf8}, byte_off, n_str, total_bytes}, dev_ptrs, (flags & LATOK_OUT_INT32) != 0, turn->st);
        return LATOK_OK;
    }
    // a batch that was checked and resolved elsewhere (compact_common), on that call's turn
    void adopt(const Batch& batch, bool dev_ptrs, bool out32, hipStream_t stream) {
        dev = dev_ptrs;
        o32 = out32;
        elt = o32 ? 4 : 8;
        st = stream;
        b = batch;
        total = batch.total;
        empty = batch.n_str == 0 || batch.total == 0;
    }
    // a batch that launches: the batch on the device, the context's workspace sized for `shape`, the pinned words of `clear_mask` zero
    int stage(Ctx& g, int route, const WsShape& shape, unsigned clear_mask) {
        int rc;
        if (dev && ((uintptr_t)b.in.p & 15) != 0) return fail(LATOK_ERR_INVALID, "device UTF-8 pointer must be 16-byte aligned");
        g.last_route = route;
        if ((rc = units_on_device(g, b, dev, st, &d))) return rc;
        if ((rc = ws_ensure(ws_needs(g.ws, total, shape).data(), kWsNeeds)) || (rc = g.pin_tot.ensure(64))) return rc;
        h_tot = (volatile int64_t*)g.pin_tot.h;
        p_tot = (int64_t*)g.pin_tot.d;
        for (int i = 0; i < 8; ++i)
            if (clear_mask >> i & 1) h_tot[i] = 0;
        return LATOK_OK;
    }
    // the call's wait for its kernels, then the pinned pair (finish_totals)
    int wait_totals(Ctx& g, int64_t o32_mask, int64_t* total_out) {
        HIP_TRY(hipStreamSynchronize(st));
        return finish_totals(g.ws, h_tot, o32_mask, total_out);
    }
};
constexpr unsigned kClearPair = 0x3, kClearSized = 0xB, kClearBytesFeats = 0x1B;   // pinned words {0, 1}, {0, 1, 3}, {0, 1, 3, 4}
constexpr unsigned kClearNgrams = 0x2B;                                               // {0, 1, 3, 5}
constexpr unsigned kClearTfidfErr = 0x80;                                             // word 7: the error word of the TF-IDF tail

// The end of a call whose payload has a size known only now (`n` items, read behind wait_totals): more than the caller's capacity
// is refused with `need_fmt`; host pointers then get `n` items of every array (a NULL dst was not asked for) and a last wait.
struct SizedCopy {
    void* dst;
    const void* src;
    size_t width;   // bytes per item
};
int deliver_sized(const BytesCall& c, int64_t n, int64_t cap, const char* need_fmt, std::initializer_list<SizedCopy> copies) {
    if (n > cap) return fail(LATOK_ERR_INVALID, need_fmt, (long long)n);
    if (c.dev || n == 0) return LATOK_OK;
    for (const SizedCopy& k : copies)
        if (k.dst) HIP_TRY(hipMemcpyAsync(k.dst, k.src, (size_t)n * k.width, hipMemcpyDeviceToHost, c.st));
    HIP_TRY(hipStreamSynchronize(c.st));
    return LATOK_OK;
}

// the shared object of a call (`noun`: vocabulary, idf, counter) lives on the device of the context that runs the call; a counter
// passes `failed`, and is refused when an update of it did not finish
int check_device(const Ctx& g, const char* noun, int device, bool failed = false) {
    if (device != g.device) return fail(LATOK_ERR_INVALID, "the %s lives on device %d, the current context on device %d", noun, device, g.device);
    if (failed) return fail(LATOK_ERR_INVALID, "the %s is in the failed state (an update did not finish): latok_%s_clear it", noun, noun);
    return LATOK_OK;
}
// the vocabulary (or WordPiece object) of a call: there is one, and it passes check_device
template <class Obj, class Handle>
int check_object(const Ctx& g, const Handle* handle, const char* null_msg, const Obj** v) {
    *v = reinterpret_cast<const Obj*>(handle);
    if (!*v) return fail(LATOK_ERR_INVALID, "%s", null_msg);
    return check_device(g, "vocabulary", (*v)->device);
}
// the word list of latok_vocab_create, latok_wordpiece_create and latok_bpe_create; needs no device
int check_word_list(const uint8_t* words, const int64_t* word_off, int64_t n_words) {
    if (n_words < 0 || n_words >= (1ll << 31)) return fail(LATOK_ERR_INVALID, "n_words must be in 0 .. 2^31 - 1");
    if (!word_off) return fail(LATOK_ERR_INVALID, "word_off is NULL");
    if (word_off[0] != 0) return fail(LATOK_ERR_INVALID, "word_off must start at 0");
    uint64_t padded = 0;
    for (int64_t i = 0; i < n_words; ++i) {
        if (word_off[i + 1] < word_off[i]) return fail(LATOK_ERR_INVALID, "word_off must be non-decreasing (word %lld)", (long long)i);
        padded += ((uint64_t)(word_off[i + 1] - word_off[i]) + 3u) & ~3ull;
        if (padded >= (1ull << 32)) return fail(LATOK_ERR_INVALID, "the padded words take 2^32 bytes or more");
    }
    if (word_off[n_words] > 0 && !words) return fail(LATOK_ERR_INVALID, "words is NULL");
    return LATOK_OK;
}

// Shared body of the mask entry points: UTF-32 bits or values, PEP 393 units or UTF-8 bytes (bits).  Small UTF-32 host batches
// run in place on pinned memory; the other host batches are staged on the device.
int mask_common(Ctx& g, Input in, const int64_t* row_off, int64_t n_str, int64_t total, void* out, int mode, int flags, void* stream) {
    int rc = need_init(g);
    if (rc) return rc;
    StreamTurn turn(g, stream);
    hipStream_t st = turn.st;
    const bool dev = (flags & LATOK_DEVICE_PTRS) != 0;
    if ((rc = resolve_total(row_off, n_str, &total, dev, st))) return rc;
    if (total == 0) return LATOK_OK;
    if (!in.p || !out) return fail(LATOK_ERR_INVALID, "NULL buffer");
    Pipe a;
    a.b = Batch{in, row_off, n_str, total};
    a.mode = mode;
    a.st = st;
    auto set_out = [&](void* o) {
        if (mode == latok::kModeBits) a.bits = (uint64_t*)o;
        else a.values = (uint8_t*)o;
    };
    if (dev) {
        if (in.form == Form::Utf32 && ((uintptr_t)in.p & 15) != 0) return fail(LATOK_ERR_INVALID, "device cps pointer must be 16-byte aligned");
        set_out(out);
        return run_pipeline(g, g.ws, a);
    }
    const size_t out_bytes = mode == latok::kModeBits ? (size_t)((total + 63) / 64) * 8 : (size_t)total;
    if (in.form == Form::Utf32 && total <= kSmallChars && n_str <= kSmallStrings) {
        // small batch: stage in pinned mapped memory, kernels work on it in place, one synchronisation
        const size_t o_row = align16((size_t)total * 4), o_out = o_row + (size_t)(n_str + 1) * 8;
        if ((rc = g.pin.ensure(o_out + align16(out_bytes)))) return rc;
        memcpy(g.pin.h, in.p, (size_t)total * 4);
        memcpy((char*)g.pin.h + o_row, row_off, (size_t)(n_str + 1) * 8);
        a.b.in.p = g.pin.d;
        a.b.row = (const int64_t*)((char*)g.pin.d + o_row);
        set_out((char*)g.pin.d + o_out);
        if ((rc = arm_done(g, st, &a.done)) || (rc = run_pipeline(g, g.ws, a)) || (rc = wait_done(g, a.done, st))) return rc;
        memcpy(out, (char*)g.pin.h + o_out, out_bytes);
        return LATOK_OK;
    }
    if (in.form == Form::Utf32) {
        if ((rc = g.h_cps.ensure((size_t)total * 4))) return rc;
        if ((rc = g.h_row.ensure((size_t)(n_str + 1) * 8))) return rc;
        if ((rc = g.h_out.ensure(out_bytes))) return rc;
        HIP_TRY(hipMemcpyAsync(g.h_cps.p, in.p, (size_t)total * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(g.h_row.p, row_off, (size_t)(n_str + 1) * 8, hipMemcpyHostToDevice, st));
        a.b.in.p = g.h_cps.p;
        a.b.row = (const int64_t*)g.h_row.p;
    } else if ((rc = g.h_out.ensure(out_bytes)) || (rc = units_on_device(g, a.b, false, st, &a.b))) {
        return rc;
    }
    set_out(g.h_out.p);
    if ((rc = run_pipeline(g, g.ws, a))) return rc;
    HIP_TRY(hipMemcpyAsync(out, g.h_out.p, out_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return LATOK_OK;
}

}  // namespace

extern "C" {

int latok_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* latok_last_error(void) { return g_err.c_str(); }
const char* latok_version(void) { return "latok_hip 0.1 (gfx950)"; }

// ---- context lifecycle ---------------------------------------------------------------------------------------------
static void ctx_release(Ctx& g) {   // caller holds g.mu (or owns g exclusively)
    if (g.stream) (void)hipStreamSynchronize(g.stream);
    g.pin.release();
    g.pin_tot.release();
    g.done_ctr.release();
    g.rules_on = false;
    g.plan_cus = 0;
    g.last = Ctx::LastPlan{};
    for (DevBuf* b : {&g.t1, &g.t1rule, &g.tb6, &g.tb6rule, &g.t2code, &g.t2cls, &g.cw, &g.h_row, &g.h_out, &g.counts, &g.scan_tot, &g.u_bytes,
                      &g.u_boff, &g.u_cnt, &g.u_row, &g.u_pref, &g.h_aux, &g.fold_tab, &g.fold_start, &g.fold_pref})
        b->release();
    g.fold_ready = false;
    g.fold_t = FoldTables{};
    g.ws.release();
    for (auto& e : g.ev) {
        if (e) (void)hipEventDestroy(e);
        e = nullptr;
    }
    if (g.turn_event) (void)hipEventDestroy(g.turn_event);
    g.turn_event = nullptr;
    g.turn_stream_valid = false;
    for (int i = 0; i < 2; ++i) {
        for (DevBuf* b : {&g.pipe_in[i], &g.pipe_row[i], &g.pipe_counts[i], &g.pipe_items[i], &g.pipe_feat[i]}) b->release();
        for (hipEvent_t* e : {&g.ev_in_ready[i], &g.ev_k_done[i], &g.ev_d2h_done[i]}) {
            if (*e) (void)hipEventDestroy(*e);
            *e = nullptr;
        }
    }
    g.pipe_tot.release();
    for (auto& f : g.flow) {
        if (f.st) {
            (void)hipStreamSynchronize(f.st);
            (void)hipStreamDestroy(f.st);
        }
        f.st = nullptr;
        f.ws.release();
    }
    g.flow_held.clear();
    g.bench_cps_b = nullptr;
    g.bench_row_b = nullptr;
    g.flow_ready = false;
    g.flow_seq = 0;
    if (g.s_h2d) (void)hipStreamDestroy(g.s_h2d);
    if (g.s_d2h) (void)hipStreamDestroy(g.s_d2h);
    g.s_h2d = g.s_d2h = nullptr;
    if (g.stream) (void)hipStreamDestroy(g.stream);
    g.stream = nullptr;
    g.inited = false;
    g.device = -1;
}

// Byte space's class table (split_code.h: LK_B6_*): the generated two-stage table (blocks of 128 code points, uint8 block ids) cut
// again at 64 code points -- stage 1 by cp >> 6 = every UTF-8 byte of the char but the last, as the uint16 OFFSET of a 64-entry
// stage-2 block, which the last byte's payload indexes.  blob = [stage 1, kB6Stage1Bytes | stage 2, kB6Stage2Bytes]; code[] =
// kClassCode or kClassRuleCode.  What the kernel relies on beyond the lookup itself is checked here: ASCII is blocks 0 and 1,
// back to back (its bytes are looked up without stage 1), and the last stage-1 entry (cp >= 0x110000) is a block of zeros.
static int build_byte_tables(const unsigned char* code, std::vector<uint8_t>& blob) {
    blob.assign(latok::kB6TablesBytes, 0);
    uint16_t* s1 = reinterpret_cast<uint16_t*>(blob.data());
    uint8_t* s2 = blob.data() + latok::kB6Stage1Bytes;
    int n_blocks = 0;
    for (int hi = 0; hi < latok::kB6Stage1Len; ++hi) {
        uint8_t v[64];
        const uint32_t cp0 = (uint32_t)hi << LK_B6_SHIFT;
        const uint32_t b7 = kStage1[cp0 >= 0x110000u ? LATOK_TBL_STAGE1_LEN - 1 : (cp0 >> LATOK_TBL_SHIFT)];
        for (int j = 0; j < 64; ++j) {
            const uint32_t in = cp0 >= 0x110000u ? 0u : ((cp0 + j) & ((1u << LATOK_TBL_SHIFT) - 1u));
            v[j] = code[kStage2[(b7 << LATOK_TBL_SHIFT) | in]];
        }
        int b = 0;
        while (b < n_blocks && memcmp(s2 + 64 * b, v, 64) != 0) ++b;
        if (b == n_blocks) {
            if (n_blocks == latok::kB6MaxBlocks) return fail(LATOK_ERR_INVALID, "internal: more than %d distinct 64-char class blocks", latok::kB6MaxBlocks);
            memcpy(s2 + 64 * n_blocks++, v, 64);
        }
        s1[hi] = (uint16_t)(64 * b);
    }
    bool last_zero = true;
    for (int j = 0; j < 64; ++j) last_zero = last_zero && s2[s1[latok::kB6Stage1Len - 1] + j] == 0;
    if (s1[0] != 0 || s1[1] != 64 || !last_zero) return fail(LATOK_ERR_INVALID, "internal: byte-space class table layout");
    return LATOK_OK;
}

/* test hook (not part of the ABI; needs no device): the byte-space class table as the kernels get it -- rule_codes 0: split
 * codes, 1: rule codes.  Writes kB6TablesBytes into out (cap_bytes >= that) and returns the offset of stage 2 inside it. */
extern "C" int latok_debug_byte_tables(int rule_codes, void* out, int64_t cap_bytes) {
    std::vector<uint8_t> blob;
    const int rc = build_byte_tables(rule_codes ? kClassRuleCode : kClassCode, blob);
    if (rc) return rc;
    if (!out || cap_bytes < (int64_t)blob.size()) return fail(LATOK_ERR_INVALID, "need %zu bytes", blob.size());
    memcpy(out, blob.data(), blob.size());
    return latok::kB6Stage1Bytes;
}

static int ctx_init_body(Ctx& g, int device) {
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    g.n_cu = prop.multiProcessorCount;
    HIP_TRY(hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking));
    for (auto& e : g.ev) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipEventCreateWithFlags(&g.turn_event, hipEventDisableTiming));
    g.turn_stream_valid = false;

    // tables: stage-1 (padded), stage-2 as split codes (fused path) and as class ids + class words (parse matrix)
    std::vector<uint8_t> t1(latok::kStage1Pad, kStage1[LATOK_TBL_STAGE1_LEN - 1]);
    memcpy(t1.data(), kStage1, LATOK_TBL_STAGE1_LEN);
    std::vector<uint8_t> t2code(latok::kStage2Len);
    for (int i = 0; i < latok::kStage2Len; ++i) t2code[i] = kClassCode[kStage2[i]];
    int rc;
    std::vector<uint8_t> t2rule(latok::kStage2Len);
    for (int i = 0; i < latok::kStage2Len; ++i) t2rule[i] = kClassRuleCode[kStage2[i]];
    if ((rc = g.t1.ensure(t1.size() + t2code.size()))) return rc;   // [stage1 | stage2 codes], contiguous like in LDS
    if ((rc = g.t1rule.ensure(t1.size() + t2rule.size()))) return rc;   // same with rule codes (runtime rule tables)
    HIP_TRY(hipMemcpy(g.t1rule.p, t1.data(), t1.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy((char*)g.t1rule.p + t1.size(), t2rule.data(), t2rule.size(), hipMemcpyHostToDevice));
    {
        std::vector<uint8_t> blob;
        if ((rc = build_byte_tables(kClassCode, blob))) return rc;
        if ((rc = g.tb6.ensure(blob.size()))) return rc;
        HIP_TRY(hipMemcpy(g.tb6.p, blob.data(), blob.size(), hipMemcpyHostToDevice));
        if ((rc = build_byte_tables(kClassRuleCode, blob))) return rc;
        if ((rc = g.tb6rule.ensure(blob.size()))) return rc;
        HIP_TRY(hipMemcpy(g.tb6rule.p, blob.data(), blob.size(), hipMemcpyHostToDevice));
    }
    if ((rc = g.t2cls.ensure(sizeof(kStage2)))) return rc;
    if ((rc = g.cw.ensure(sizeof(kClassWord)))) return rc;
    if ((rc = g.ws.scalar.ensure(64))) return rc;
    HIP_TRY(hipMemcpy(g.t1.p, t1.data(), t1.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy((char*)g.t1.p + t1.size(), t2code.data(), t2code.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(g.t2cls.p, kStage2, sizeof(kStage2), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(g.cw.p, kClassWord, sizeof(kClassWord), hipMemcpyHostToDevice));
    g.device = device;
    g.inited = true;
    return LATOK_OK;
}

// bind a context to `device`: stream, events, Unicode tables.  The caller's current HIP device is left as it was.
static int ctx_init(Ctx& g, int device) {   // caller holds g.mu
    int n = latok_device_count();
    if (n <= 0) return fail(LATOK_ERR_HIP, "no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= n) return fail(LATOK_ERR_INVALID, "device %d out of range (0..%d)", device, n - 1);
    int prev = -1;
    (void)hipGetDevice(&prev);
    const int rc = ctx_init_body(g, device);
    if (rc) {   // a partly built context leaks nothing
        const std::string msg = g_err;
        ctx_release(g);
        g_err = msg;
    }
    if (prev >= 0 && prev != device) (void)hipSetDevice(prev);
    return rc;
}

int latok_init(int device) {
    Ctx& g = g_default;
    std::lock_guard<std::mutex> lk(g.mu);
    if (g.inited) {
        if (g.device == device) return LATOK_OK;
        return fail(LATOK_ERR_INVALID, "the default context is already on device %d; use latok_ctx_create for other devices", g.device);
    }
    return ctx_init(g, device);
}

int latok_shutdown(void) {
    Ctx& g = g_default;
    std::lock_guard<std::mutex> lk(g.mu);
    if (!g.inited) return LATOK_OK;
    DeviceGuard dg(g);
    ctx_release(g);
    return LATOK_OK;
}

int latok_ctx_create(int device, latok_ctx** ctx_out) {
    if (!ctx_out) return fail(LATOK_ERR_INVALID, "ctx_out is NULL");
    *ctx_out = nullptr;
    Ctx* c = new (std::nothrow) Ctx();
    if (!c) return fail(LATOK_ERR_NOMEM, "out of host memory");
    int rc;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        rc = ctx_init(*c, device);
    }
    if (rc) {
        delete c;
        return rc;
    }
    *ctx_out = reinterpret_cast<latok_ctx*>(c);
    return LATOK_OK;
}

int latok_ctx_destroy(latok_ctx* ctx) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) return LATOK_OK;
    if (c == &g_default) return fail(LATOK_ERR_INVALID, "the default context is destroyed by latok_shutdown()");
    if (tl_ctx == c) tl_ctx = nullptr;
    {
        std::lock_guard<std::mutex> lk(c->mu);   // waits for a call that is still running on it
        DeviceGuard dg(*c);
        ctx_release(*c);
    }
    delete c;
    return LATOK_OK;
}

int latok_ctx_set_current(latok_ctx* ctx) {
    tl_ctx = reinterpret_cast<Ctx*>(ctx);   // NULL = the default context
    if (tl_ctx == &g_default) tl_ctx = nullptr;
    return LATOK_OK;
}

latok_ctx* latok_ctx_get_current(void) { return reinterpret_cast<latok_ctx*>(tl_ctx); }

int latok_ctx_device(latok_ctx* ctx) {
    const Ctx* c = ctx ? reinterpret_cast<const Ctx*>(ctx) : &g_default;
    return c->inited ? c->device : -1;
}

int latok_reserve(int64_t max_chars, int64_t max_strings) {
    LATOK_ENTER();
    int rc = need_init(g);
    if (rc) return rc;
    if (max_chars < 0 || max_strings < 0) return fail(LATOK_ERR_INVALID, "negative size");
    return ws_ensure(ws_needs(g.ws, max_chars, WsShape{}).data(), kTileNeeds);
}

// one rule table: row-major int8 [rows x cols] as build_combo_matrix returns it -> per-row column sets
static int pack_rule_table(const char* name, const int8_t* idx, int rows, int cols, uint32_t* row_sets) {
    if (rows < 0 || rows > LK_MAX_RULE_ROWS)
        return fail(LATOK_ERR_INVALID, "%s: %d rows (0..%d supported)", name, rows, LK_MAX_RULE_ROWS);
    if (rows > 0 && (!idx || cols < 1)) return fail(LATOK_ERR_INVALID, "%s: NULL table or no columns", name);
    for (int r = 0; r < rows; ++r) {
        uint32_t set = 0;
        for (int c = 0; c < cols; ++c) {
            const int v = idx[r * cols + c];
            if (v == -1) {
                // the reference seeds a row's product from its FIRST entry (latok.c:329-338); a row that starts with
                // the -1 pad would multiply into the previous row's product there -- refuse instead of guessing
                if (c == 0) return fail(LATOK_ERR_INVALID, "%s: row %d starts with -1", name, r);
                continue;
            }
            if (v < 0 || v >= LK_N_FEATURES)
                return fail(LATOK_ERR_INVALID, "%s: feature id %d in row %d is outside 0..%d", name, v, r, LK_N_FEATURES - 1);
            set |= 1u << v;
        }
        row_sets[r] = set;
    }
    return LATOK_OK;
}

int latok_set_rules(const int8_t* c_split, int split_rows, int split_cols, const int8_t* c_mask, int mask_rows,
                    int mask_cols, const int8_t* c_sym, int sym_rows, int sym_cols) {
    LATOK_ENTER();
    int rc = need_init(g);
    if (rc) return rc;
    lk_rule_tables R;
    memset(&R, 0, sizeof(R));
    if ((rc = pack_rule_table("C_SPLIT", c_split, split_rows, split_cols, R.row[0]))) return rc;
    if ((rc = pack_rule_table("C_MASK", c_mask, mask_rows, mask_cols, R.row[1]))) return rc;
    if ((rc = pack_rule_table("C_SYM", c_sym, sym_rows, sym_cols, R.row[2]))) return rc;
    R.n_rows[0] = split_rows;
    R.n_rows[1] = mask_rows;
    R.n_rows[2] = sym_rows;
    g.rules = R;
    g.rules_on = true;
    return LATOK_OK;
}

int latok_reset_rules(void) {
    LATOK_ENTER();
    g.rules_on = false;
    return LATOK_OK;
}

int latok_rules_active(void) {
    LATOK_ENTER();
    return g.rules_on ? 1 : 0;
}

int latok_split_mask_batch(const uint32_t* cps, const int64_t* row_off, int64_t n_str, int64_t total_chars,
                           uint64_t* mask_bits_out, int flags, void* stream) {
    LATOK_ENTER();
    return mask_common(g, Input{cps, Form::Utf32}, row_off, n_str, total_chars, mask_bits_out, latok::kModeBits, flags, stream);
}

int latok_split_values_batch(const uint32_t* cps, const int64_t* row_off, int64_t n_str, int64_t total_chars,
                             uint8_t* values_out, int flags, void* stream) {
    LATOK_ENTER();
    return mask_common(g, Input{cps, Form::Utf32}, row_off, n_str, total_chars, values_out, latok::kModeValues, flags, stream);
}

// UTF-8 ingest: decode a CSR batch of UTF-8 strings (b: total resolved by the caller) into the library's device buffers
// (g.h_cps = packed code points, g.u_row = code-point row offsets).  Inputs are host or device pointers per `dev`.  One
// blocking 8-byte read.  With `bytes_route`: when the batch has no continuation byte at all (pure ASCII, the common case)
// byte positions ARE code-point positions, so nothing is decoded; *bytes_route = the batch on the device for the byte-space
// tile kernel, whose results are then valid in code-point units as they are (bytes_route->in.p = NULL: decoded).
static int decode_utf8_to_workspace(Ctx& g, const Batch& b, bool dev, hipStream_t st, int64_t* total_cps_out, Batch* bytes_route = nullptr) {
    int rc;
    *total_cps_out = 0;
    if (bytes_route) *bytes_route = Batch();
    const int64_t n_str = b.n_str, total_bytes = b.total;
    if (n_str == 0) return LATOK_OK;
    if (total_bytes > 0 && !b.in.p) return fail(LATOK_ERR_INVALID, "utf8 buffer is NULL");
    Batch d;
    if ((rc = units_on_device(g, b, dev, st, &d))) return rc;
    const uint8_t* d_u8 = (const uint8_t*)d.in.p;
    const int64_t n_blocks = latok::utf8_blocks(total_bytes);
    if ((rc = g.u_cnt.ensure((size_t)n_blocks * 16 + 16))) return rc;               // block counts | block bases
    if ((rc = g.u_row.ensure((size_t)(n_str + 1) * 8))) return rc;
    if ((rc = g.u_pref.ensure((size_t)(n_blocks * 256) * 2 + 16))) return rc;       // u16 prefix per 16-byte chunk
    if ((rc = g.scan_tot.ensure((size_t)latok::scan_blocks(n_blocks) * 8))) return rc;
    int64_t* d_cnt = (int64_t*)g.u_cnt.p;
    int64_t* d_base = d_cnt + n_blocks;
    HIP_TRY(latok::launch_utf8_block_counts(d_u8, total_bytes, d_cnt, st));
    if ((rc = g.pin_tot.ensure(64))) return rc;
    HIP_TRY(latok::launch_exclusive_scan(d_cnt, n_blocks, d_base, (int64_t*)g.ws.scalar.p, (int64_t*)g.scan_tot.p, st,
                                         (int64_t*)g.pin_tot.d));
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t total_cps = *(volatile const int64_t*)g.pin_tot.h;
    if (bytes_route && total_cps == total_bytes && ((uintptr_t)d_u8 & 15) == 0) {
        *bytes_route = d;
        *total_cps_out = total_cps;
        return LATOK_OK;
    }
    if ((rc = g.h_cps.ensure((size_t)total_cps * 4 + 16))) return rc;
    HIP_TRY(latok::launch_utf8_decode(d_u8, total_bytes, d.row, n_str, d_base, (uint16_t*)g.u_pref.p, total_cps,
                                      (uint32_t*)g.h_cps.p, (int64_t*)g.u_row.p, st));
    *total_cps_out = total_cps;
    return LATOK_OK;
}

// featurize: per-token column sums on the tile grid (split_kernels.hip: k_features_tiles) over the kept tokens of `p`
static int enqueue_features(Ctx& g, const uint8_t* d_codes, const latok::TokenPlanes& p, void* d_spans4, int8_t* d_feat, bool out32, int64_t cap,
                            hipStream_t st, latok::DoneSignal done, latok::DeviceTotal dt) {
    latok::FeatParams F;
    F.codes = d_codes;
    F.row_off = p.row_off;
    F.n_str = p.n_str;
    F.total = p.total;
    F.n_tiles = (p.total + latok::kTile - 1) / latok::kTile;
    F.bits = p.bits;
    F.kept = p.item_mask;
    F.tile_rank = p.tile_rank;
    F.tile_cnt = p.tile_cnt;
    F.word_pref = p.word_pref;
    F.tile_first = p.tile_first;
    F.space = p.space;
    F.features = d_feat;
    F.spans4 = d_spans4;
    F.out32 = out32;
    F.n_tokens_dev = p.n_items;
    F.cap = cap;
    F.done = done;
    F.dt = dt;
    HIP_TRY(latok::launch_features_tiles(F, g.n_cu, st));
    return LATOK_OK;
}

// the chained scan's state in workspace `w` (sized by ws_needs) on its next epoch; the state is cleared when it is new
static int next_scan_epoch(Workspace& w, hipStream_t st, latok::ChainState* out) {
    w.scan_epoch = (w.scan_epoch + 1) & 0x3FFFFu;
    // (the state array may have been re-allocated by this call or by an earlier reserve: fresh memory holds anything)
    if (w.chain.gen != w.chain_seen || w.chain_ctl.gen != w.chain_ctl_seen || w.scan_epoch == 0 || !w.chain_ready) {
        w.chain_seen = w.chain.gen;
        w.chain_ctl_seen = w.chain_ctl.gen;
        HIP_TRY(hipMemsetAsync(w.chain.p, 0, w.chain.cap, st));
        HIP_TRY(hipMemsetAsync(w.chain_ctl.p, 0, 64, st));
        w.scan_epoch = 1;
        w.chain_ready = true;
    }
    *out = latok::ChainState{(unsigned long long*)w.chain.p, (unsigned*)w.chain_ctl.p, w.scan_epoch};
    return LATOK_OK;
}
// The planes of a scanned batch in workspace `w` (kernels.h: TokenPlanes): `total` units in n_str rows; spans = false: offsets (every
// boundary is an item, no SPACE plane).  bits / space: the two bitmasks where they are not the workspace's own (masks packed before
// the call; the byte-space and the code-point pair of featurize in byte space).  The item total is the workspace's scalar word 0.
static latok::TokenPlanes token_planes(const Workspace& w, const int64_t* row, int64_t n_str, int64_t total, bool spans = true,
                                       const uint64_t* bits = nullptr, const uint64_t* space = nullptr) {
    latok::TokenPlanes p;
    p.bits = bits ? bits : (const uint64_t*)w.bits.p;
    p.space = !spans ? nullptr : bits ? space : (const uint64_t*)w.space.p;
    p.item_mask = spans ? (const uint64_t*)w.kept.p : p.bits;
    p.tile_rank = (const int64_t*)w.bases.p;
    p.tile_cnt = (const int64_t*)w.wcnt.p;
    p.word_pref = (const uint16_t*)w.wpref.p;
    p.n_words = (total + 63) / 64;
    p.total = total;
    p.row_off = row;
    p.n_str = n_str;
    p.tile_first = (const int64_t*)w.tile_first.p;
    p.n_items = (const int64_t*)w.scalar.p;
    return p;
}
// one chained scan of the sized calls' rows, on its own epoch: dst = the exclusive scan of src[0 .. n), the total -> *d_total and, if
// asked for, the pinned word r_total; d_flag: the scan's own error flag
static int enqueue_row_scan(Workspace& w, const int64_t* src, int64_t n, int64_t* dst, int64_t* d_total, int64_t* r_total, int* d_flag, hipStream_t st) {
    int rc;
    latok::ChainState chain;
    if ((rc = next_scan_epoch(w, st, &chain))) return rc;
    HIP_TRY(latok::launch_tile_scan(src, n, dst, chain, d_total, r_total, d_flag, st));
    return LATOK_OK;
}

// One device-resident (chunk of a) batch for enqueue_compaction_dev
struct Compaction {
    Batch b;
    bool spans = false, feats = false, o32 = false;   // offsets, token spans, or token spans + feature sums
    void* counts = nullptr;           // per-string counts, then the records and feature sums: written only if the total fits `cap`
    void* items = nullptr;
    int8_t* feat = nullptr;
    int64_t cap = 0;
    int64_t* p_tot = nullptr;         // the total and the int32-overflow flag, as the device sees them ...
    volatile int64_t* h_tot = nullptr;   // ... and the host (the context's pinned pair; NULL: a flow's result words)
    latok::DoneSignal done{nullptr, 0, nullptr};
    const uint64_t* pre_bits = nullptr;    // the two bitmasks are already there (code-point masks packed from byte space:
    const uint64_t* pre_space = nullptr;   // enqueue_lead_front): only the string index is launched
    const uint8_t* pre_codes = nullptr;    // featurize: the rule codes too (k_lead_codes), padded to one tile + 256 B behind `total`
    // a code-point batch of a flow (flow_submit_utf8): b.total is the BYTE count, an upper bound; the code-point total is the word
    // dt.total, which the lead-byte scan writes on the same stream, and dt.gate its malformed-input flag.  The batch's result words
    // (p_tot[0..3]) were cleared by the caller.
    latok::DeviceTotal dt{nullptr, nullptr};
    hipStream_t st = nullptr;
};

// Device-side core of the compaction entry points, on one device-resident (chunk of a) batch: per-string boundary
// offsets (spans = false), token spans, or token spans + feature sums (feats).  Launch sequence:
//   tile index -> tiles -> resolve            the two bitmasks (boundaries, SPACE)
//   k_word_counts, k_scan_chained             items per word / tile, tile ranks and the total
//   k_counts_scatter (or k_string_counts + k_features_tiles)     per-string counts + the records, written only if the
//                                             total fits `cap`
// Nothing is synchronised here: the total and the int32-overflow flag land in the pinned pair p_tot[0..1] (h_tot = the
// host's view of the same two words) when the stream gets there.
static int enqueue_compaction_dev(Ctx& g, Workspace& w, const Compaction& c) {
    int rc;
    const int64_t total = c.b.total;
    const hipStream_t st = c.st;
    const bool widen = c.feats && c.b.in.narrow();   // featurize re-reads the code points: widen once, on the device
    if (widen && ((uintptr_t)c.b.in.p & (c.b.in.width() - 1)) != 0) return fail(LATOK_ERR_INVALID, "misaligned code units");
    if ((rc = ws_ensure(ws_needs(w, total, WsShape{.spans = c.spans, .feats = c.feats, .widen = widen}).data(), kWsNeeds))) return rc;
    Pipe a;
    a.b = c.b;
    a.st = st;
    if (widen) {
        HIP_TRY(latok::launch_widen_units(c.b.in.p, (int)c.b.in.width(), total, (uint32_t*)w.widened.p, st));
        a.b.in = Input{w.widened.p, Form::Utf32};
    }
    latok::ChainState chain;
    if ((rc = next_scan_epoch(w, st, &chain))) return rc;
    const latok::TokenPlanes p = token_planes(w, c.b.row, c.b.n_str, total, c.spans, c.pre_bits, c.pre_space);
    uint8_t* d_codes = nullptr;
    if (c.feats && c.pre_codes) {   // packed before (every char's code is there already): only the padding behind the last char
        d_codes = const_cast<uint8_t*>(c.pre_codes);
        if (c.dt.total) HIP_TRY(latok::launch_pad_codes(d_codes, c.dt.total, total, st));   // (behind a total the host does not know)
        else HIP_TRY(hipMemsetAsync(d_codes + total, 0, (size_t)latok::kTile + 256, st));
    } else if (c.feats) {   // the tile kernel leaves the rule code of every char: 1 B/char for k_features_tiles instead of 4 B/char + tables
        d_codes = (uint8_t*)w.codes.p;
        const size_t tail0 = (size_t)total & ~(size_t)(latok::kTile - 1);
        HIP_TRY(hipMemsetAsync(d_codes + tail0, 0, (size_t)total + latok::kTile + 256 - tail0, st));
    }
    a.bits = const_cast<uint64_t*>(p.bits);   // (masks packed before the call are not written: stages = 1)
    a.space = const_cast<uint64_t*>(p.space);
    a.codes = c.pre_codes ? nullptr : d_codes;
    a.stages = c.pre_bits ? 1 : 7;
    if ((rc = run_pipeline(g, w, a))) return rc;
    if (c.h_tot) {   // pinned pair of the context's own calls: cleared by the host
        c.h_tot[0] = 0;
        c.h_tot[1] = 0;
    } else if (!c.dt.total) {   // a flow's result words live wherever the caller put them: cleared on the stream
        HIP_TRY(hipMemsetAsync(c.p_tot, 0, 16, st));
    }
    int* d_err = (int*)(c.p_tot + 1);
    HIP_TRY(latok::launch_word_counts_scan(c.spans, p, chain, c.p_tot, d_err + 1, st, c.dt));   // (the scan's own flag: the upper half of the pinned word)
    if (c.feats) {   // spans and sums come from one kernel
        HIP_TRY(latok::launch_string_counts(c.o32, p, c.counts, d_err, st, c.dt));
        return enqueue_features(g, d_codes, p, c.items, c.feat, c.o32, c.cap, st, c.done, c.dt);
    }
    HIP_TRY(latok::launch_counts_scatter(c.spans ? 1 : 0, c.o32, p, c.items, c.cap, c.counts, d_err, st, c.done, c.dt));
    return LATOK_OK;
}

// Large host-pointer batches: a chunked pipeline over three streams.  The batch is cut into chunks of whole strings
// (~8 M chars); chunk c + 1 is on its way up the bus (copy stream) while chunk c runs its kernels (the context's stream)
// and the records of chunk c - 1 go down (second copy stream); inputs and outputs are double-buffered on the device, a
// chunk's records land in a buffer sized for the worst case (one item per char), so nothing waits for a total before it
// is enqueued.  Per chunk the host waits once (for its total) before it can place the chunk's records behind the
// previous ones in the caller's arrays.  With pinned host arrays (latok_host_alloc) both copy directions run at bus
// speed concurrently; pageable arrays work too (the runtime stages them).
// (test hook: LATOK_PIPE_CHUNK_CHARS in the environment shrinks the chunks, so that a test can push hundreds of chunks
// through the double buffers with batches the oracle checks in seconds)
static int64_t pipe_chunk_chars() {
    static const int64_t v = [] {
        const char* e = getenv("LATOK_PIPE_CHUNK_CHARS");
        const long long x = e ? atoll(e) : 0;
        return (int64_t)(x >= 64 ? x : (8ll << 20));
    }();
    return v;
}
#define kPipeChunkChars (pipe_chunk_chars())
#define kPipeMinChars (2 * pipe_chunk_chars())

static int ensure_pipe(Ctx& g) {
    if (g.s_h2d) return LATOK_OK;
    HIP_TRY(hipStreamCreateWithFlags(&g.s_h2d, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&g.s_d2h, hipStreamNonBlocking));
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(hipEventCreateWithFlags(&g.ev_in_ready[i], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&g.ev_k_done[i], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&g.ev_d2h_done[i], hipEventDisableTiming));
    }
    return LATOK_OK;
}

static int compact_host_pipelined_body(Ctx& g, bool spans, bool feats, bool o32, const Batch& h, void* counts_out, void* items_out,
                                       int64_t items_cap, int64_t* n_items_out, int8_t* features_out, hipStream_t st) {
    int rc;
    if ((rc = ensure_pipe(g))) return rc;
    const int64_t* row_off = h.row;
    const int64_t n_str = h.n_str;
    const size_t unit_bytes = h.in.width();
    const size_t elt = o32 ? 4 : 8;
    const size_t item_bytes = (feats ? 4 : (spans ? 2 : 1)) * elt;
    // chunk boundaries (string ids): cut where the cumulative char count passes multiples of the chunk size
    std::vector<int64_t> cut(1, 0);
    int64_t max_chars = 0, max_strs = 0;
    while (cut.back() < n_str) {
        const int64_t s0 = cut.back();
        const int64_t* e = std::upper_bound(row_off + s0 + 1, row_off + n_str + 1, row_off[s0] + kPipeChunkChars);
        int64_t s1 = (e - row_off) - 1;            // last string that still ends within the chunk size
        if (s1 <= s0) s1 = s0 + 1;                 // a single string longer than a chunk is a chunk of its own
        cut.push_back(s1);
        max_chars = std::max(max_chars, row_off[s1] - row_off[s0]);
        max_strs = std::max(max_strs, s1 - s0);
    }
    const int n_chunks = (int)cut.size() - 1;
    for (int i = 0; i < 2; ++i) {
        if ((rc = g.pipe_in[i].ensure((size_t)max_chars * unit_bytes + 64))) return rc;
        if ((rc = g.pipe_row[i].ensure((size_t)(max_strs + 1) * 8))) return rc;
        if ((rc = g.pipe_counts[i].ensure((size_t)max_strs * elt + 16))) return rc;
        if ((rc = g.pipe_items[i].ensure((size_t)max_chars * item_bytes + 64))) return rc;      // at most one item per char
        if (feats && (rc = g.pipe_feat[i].ensure((size_t)max_chars * LATOK_FEATURE_COUNT + 64))) return rc;
    }
    if ((rc = g.pipe_tot.ensure(8 * 16))) return rc;
    // size the workspace for the largest chunk now: growing a buffer later would free it under a chunk that is still running
    if ((rc = ws_ensure(ws_needs(g.ws, max_chars, WsShape{.spans = spans, .feats = feats, .widen = feats && h.in.narrow()}).data(), kWsNeeds))) return rc;
    int64_t running = 0;
    bool overflow = false, too_long = false;
    std::vector<int64_t> n_of(n_chunks, 0);
    auto finish = [&](int c) -> int {   // chunk c's kernels are enqueued: wait for its total, send its records down
        const int slot = c & 1;
        HIP_TRY(hipEventSynchronize(g.ev_k_done[slot]));
        volatile int64_t* h = (volatile int64_t*)g.pipe_tot.h + 2 * (c & 7);
        int64_t n = 0;
        // (mask 0: a chunk that overflows int32 does not end the call while later chunks are in flight: refused once, at the end)
        if ((rc = finish_totals(g.ws, h, 0, &n))) return rc;
        if (h[1] & 0xFFFFFFFFll) too_long = true;
        n_of[c] = n;
        const int64_t s0 = cut[c], ns = cut[c + 1] - cut[c];
        HIP_TRY(hipStreamWaitEvent(g.s_d2h, g.ev_k_done[slot], 0));
        HIP_TRY(hipMemcpyAsync((char*)counts_out + (size_t)s0 * elt, g.pipe_counts[slot].p, (size_t)ns * elt, hipMemcpyDeviceToHost, g.s_d2h));
        if (running + n > items_cap || (n > 0 && !items_out)) overflow = true;
        if (!overflow && n > 0) {
            HIP_TRY(hipMemcpyAsync((char*)items_out + (size_t)running * item_bytes, g.pipe_items[slot].p, (size_t)n * item_bytes,
                                   hipMemcpyDeviceToHost, g.s_d2h));
            if (feats)
                HIP_TRY(hipMemcpyAsync(features_out + (size_t)running * LATOK_FEATURE_COUNT, g.pipe_feat[slot].p,
                                       (size_t)n * LATOK_FEATURE_COUNT, hipMemcpyDeviceToHost, g.s_d2h));
        }
        HIP_TRY(hipEventRecord(g.ev_d2h_done[slot], g.s_d2h));
        running += n;
        return LATOK_OK;
    };
    auto upload = [&](int c) -> int {   // chunk c's code units and row offsets (its device buffers are free once chunk c - 2 is computed)
        const int slot = c & 1;
        const int64_t s0 = cut[c], ns = cut[c + 1] - s0, c0 = row_off[s0], nc = row_off[cut[c + 1]] - c0;
        if (c >= 2) HIP_TRY(hipStreamWaitEvent(g.s_h2d, g.ev_k_done[slot], 0));
        if (nc > 0)
            HIP_TRY(hipMemcpyAsync(g.pipe_in[slot].p, (const char*)h.in.p + (size_t)c0 * unit_bytes, (size_t)nc * unit_bytes,
                                   hipMemcpyHostToDevice, g.s_h2d));
        HIP_TRY(hipMemcpyAsync(g.pipe_row[slot].p, row_off + s0, (size_t)(ns + 1) * 8, hipMemcpyHostToDevice, g.s_h2d));
        HIP_TRY(hipEventRecord(g.ev_in_ready[slot], g.s_h2d));
        return LATOK_OK;
    };
    if ((rc = upload(0))) return rc;
    for (int c = 0; c < n_chunks; ++c) {
        const int slot = c & 1;
        const int64_t s0 = cut[c], ns = cut[c + 1] - s0, c0 = row_off[s0], nc = row_off[cut[c + 1]] - c0;
        // compute: behind the upload, and behind the download of chunk c - 2 (it read the same output buffers)
        HIP_TRY(hipStreamWaitEvent(st, g.ev_in_ready[slot], 0));
        if (c >= 2) HIP_TRY(hipStreamWaitEvent(st, g.ev_d2h_done[slot], 0));
        HIP_TRY(latok::launch_rebase_rows((int64_t*)g.pipe_row[slot].p, ns + 1, c0, st));
        volatile int64_t* h_tot = (volatile int64_t*)g.pipe_tot.h + 2 * (c & 7);
        if (nc > 0) {
            Compaction k;
            k.b = Batch{Input{g.pipe_in[slot].p, h.in.form}, (const int64_t*)g.pipe_row[slot].p, ns, nc};
            k.spans = spans;
            k.feats = feats;
            k.o32 = o32;
            k.counts = g.pipe_counts[slot].p;
            k.items = g.pipe_items[slot].p;
            k.feat = (int8_t*)g.pipe_feat[slot].p;
            k.cap = nc;
            k.p_tot = (int64_t*)g.pipe_tot.d + 2 * (c & 7);
            k.h_tot = h_tot;
            k.st = st;
            if ((rc = enqueue_compaction_dev(g, g.ws, k))) return rc;
        } else {   // only empty strings in this chunk
            h_tot[0] = 0;
            h_tot[1] = 0;
            HIP_TRY(hipMemsetAsync(g.pipe_counts[slot].p, 0, (size_t)ns * elt, st));
        }
        HIP_TRY(hipEventRecord(g.ev_k_done[slot], st));
        // the next upload is queued before the host waits for anything: the copy stream never runs dry
        // (chunk c + 1 shares its buffers with chunk c - 1, whose kernels were enqueued an iteration ago)
        if (c + 1 < n_chunks && (rc = upload(c + 1))) return rc;
        if (c >= 1 && (rc = finish(c - 1))) return rc;
    }
    if ((rc = finish(n_chunks - 1))) return rc;
    HIP_TRY(hipStreamSynchronize(g.s_d2h));
    HIP_TRY(hipStreamSynchronize(st));
    *n_items_out = running;
    if (too_long) return refuse_too_long();
    return refuse_no_room(running, items_cap, items_out);
}

// h: a host batch of at least kPipeMinChars units, checked
static int compact_host_pipelined(Ctx& g, bool spans, bool feats, bool o32, const Batch& h, void* counts_out, void* items_out,
                                  int64_t items_cap, int64_t* n_items_out, int8_t* features_out, hipStream_t st) {
    const int rc = compact_host_pipelined_body(g, spans, feats, o32, h, counts_out, items_out, items_cap, n_items_out, features_out, st);
    if (rc != LATOK_OK && g.s_h2d) {
        // a failure in the middle leaves copies in flight that read and write the CALLER's arrays: drain them before the
        // error is returned (the message of the failure is kept)
        const std::string msg = g_err;
        (void)hipStreamSynchronize(g.s_h2d);
        (void)hipStreamSynchronize(st);
        (void)hipStreamSynchronize(g.s_d2h);
        g_err = msg;
    }
    return rc;
}

// Host decode of a small UTF-8 batch (compact_common) with the device decoder's rule -- one code point per lead byte, as
// many continuation bytes as the lead announces (utf8_decode.h) -- into UTF-32.  Only when every string is structurally
// well-formed (each lead followed by exactly its continuation bytes inside the string, no stray continuation byte): the two
// device paths define what malformed input means, and they keep doing so.  cps / cp_row / bytepos: code points, code-point
// row offsets, byte position of every char (+ one entry for the end).
static bool host_decode_small(const uint8_t* u8, const int64_t* boff, int64_t n_str, std::vector<uint32_t>& cps,
                              std::vector<int64_t>& cp_row, std::vector<int64_t>& bytepos) {
    const int64_t total = boff[n_str];
    cps.clear(); bytepos.clear();
    cps.reserve((size_t)total); bytepos.reserve((size_t)total + 1);
    cp_row.assign((size_t)n_str + 1, 0);
    for (int64_t s = 0; s < n_str; ++s) {
        const int64_t end = boff[s + 1];
        for (int64_t i = boff[s]; i < end;) {
            const uint32_t b0 = u8[i];
            int extra = 0;
            uint32_t cp = b0;
            if (b0 >= 0x80u) {
                if (b0 < 0xC0u) return false;                       // stray continuation byte
                if (b0 >= 0xF0u) { cp = b0 & 0x07u; extra = 3; }
                else if (b0 >= 0xE0u) { cp = b0 & 0x0Fu; extra = 2; }
                else { cp = b0 & 0x1Fu; extra = 1; }
                if (i + extra >= end) return false;                 // truncated at the string's end
                for (int j = 1; j <= extra; ++j) {
                    const uint32_t b = u8[i + j];
                    if ((b & 0xC0u) != 0x80u) return false;         // truncated sequence
                    cp = (cp << 6) | (b & 0x3Fu);
                }
            }
            cps.push_back(cp);
            bytepos.push_back(i);
            i += 1 + extra;
        }
        cp_row[(size_t)s + 1] = (int64_t)cps.size();
    }
    bytepos.push_back(total);
    return true;
}

// Code-point results of a UTF-8 batch WITHOUT a UTF-32 copy of it (the reference reads code points, latok.c:53-55,79; a UTF-8
// caller has bytes): the byte-space tile kernel on the bytes, which also leaves the lead-byte mask and the lead counts per word
// and per tile; one scan of the tile counts (k_scan_chained); then k_lead_compress packs the boundary bits at lead bytes (and,
// for token spans, the SPACE plane) and turns the byte offsets into code-point offsets.  HBM traffic: the bytes once + ~5 bits per
// byte of masks and ranks, against 1 + 4 + 4 bytes per char through the staged decoder.
// This front is the same for the blocking calls (cp_masks_via_bytes), the flow (flow_submit_utf8) and featurize in byte space
// (enqueue_utf8_bytes_features).  One stream, nothing waits for the host:
//   tile index -> byte-space tiles -> resolve       boundary mask, SPACE plane, lead mask + lead counts over the BYTES
//   k_scan_chained (lead counts)                    lead ranks; the code-point total -> scalar word 1 (word 0 is the item total of the
//                                                   scan that follows), r_cps; the scan's own flag -> the high half of r_err
//   k_lead_compress                                 packed code-point masks, code-point row offsets; malformed -> r_odd
//   k_lead_codes (codes)                            the rule code of every char at its code-point position, as the UTF-32 tile kernel
//                                                   would leave it
// `w` was sized by ws_needs at the byte count (which bounds the code-point count) with a shape that has cp_rows = n_str + 1, .spans
// if `space` and .feats if `codes`.  What comes back are the planes, for the launches that follow.
struct LeadFront {
    Batch b;                       // UTF-8 bytes on the device (16-byte aligned), byte offsets, total in bytes (> 0), n_str > 0
    bool space = false, codes = false;   // also the SPACE plane (token spans) / the rule codes (featurize)
    uint64_t* cpbits = nullptr;    // where the packed code-point mask goes: a caller's buffer of cap_words words (a smaller mask is
    int64_t cap_words = 0;         // not written), or NULL: the workspace's cpbits, a whole plane
    int64_t* cp_row = nullptr;     // the code-point row offsets [n_str + 1]: a caller's buffer, or NULL: the workspace's cprow
    int64_t* r_cps = nullptr;      // the three result words as the device sees them (cleared by the caller): code-point total,
    int* r_err = nullptr;          // the call's error word,
    int* r_odd = nullptr;          // malformed-input flag
    hipStream_t st = nullptr;
};
struct LeadPlanes {
    uint64_t *bmask = nullptr, *bspace = nullptr, *lead = nullptr;   // over the bytes
    uint64_t *cpbits = nullptr, *cpspace = nullptr;                  // packed at the lead bytes
    int64_t* cp_row = nullptr;
    uint8_t* codes = nullptr;
    int64_t* total_cps = nullptr;                                    // the device word that holds the code-point total
};
static int enqueue_lead_front(Ctx& g, Workspace& w, const LeadFront& a, LeadPlanes* out) {
    int rc;
    const int64_t total_bytes = a.b.total, words_b = (total_bytes + 63) / 64, c_tiles = (words_b + 63) / 64;
    LeadPlanes& t = *out;   // (a plane that was not asked for: NULL)
    t.bmask = (uint64_t*)w.bits.p;
    t.bspace = a.space ? (uint64_t*)w.bspace.p : nullptr;
    t.lead = (uint64_t*)w.lead.p;
    t.cpbits = a.cpbits ? a.cpbits : (uint64_t*)w.cpbits.p;
    t.cpspace = a.space ? (uint64_t*)w.cpspace.p : nullptr;
    t.cp_row = a.cp_row ? a.cp_row : (int64_t*)w.cprow.p;
    t.codes = a.codes ? (uint8_t*)w.codes.p : nullptr;
    t.total_cps = (int64_t*)w.scalar.p + 1;
    int64_t* d_rank = (int64_t*)w.bases.p;
    int64_t* d_tcnt = (int64_t*)w.wcnt.p;
    uint16_t* d_pref = (uint16_t*)w.wpref.p;
    latok::ChainState chain;
    if ((rc = next_scan_epoch(w, a.st, &chain))) return rc;
    Pipe p;
    p.b = a.b;
    p.bits = t.bmask;
    p.space = t.bspace;
    p.lead = t.lead;
    p.lead_pref = d_pref;
    p.lead_cnt = d_tcnt;
    p.st = a.st;
    if ((rc = run_pipeline(g, w, p))) return rc;
    HIP_TRY(latok::launch_tile_scan(d_tcnt, c_tiles, d_rank, chain, t.total_cps, a.r_cps, a.r_err + 1, a.st));
    HIP_TRY(latok::launch_lead_compress(t.bmask, t.bspace, t.lead, d_rank, d_tcnt, d_pref, words_b, total_bytes, a.b.row, a.b.n_str, t.total_cps,
                                        t.cpbits, t.cpspace, a.cpbits ? a.cap_words : words_b, t.cp_row, a.r_odd, a.st));
    if (a.codes)
        HIP_TRY(latok::launch_lead_codes((const uint8_t*)a.b.in.p, total_bytes, t.lead, d_rank, d_tcnt, d_pref, words_b, (const uint8_t*)g.tb6rule.p,
                                         t.codes, g.n_cu, a.st));
    return LATOK_OK;
}

// The front on the context's own workspace, for the blocking calls (a: everything but the result words, which are the pinned words
// 0, 1 and 3): the code-point total and the malformed-input flag are read after one synchronisation.  *fallback_out = 1: the batch
// holds a continuation byte that the byte-space model and the decoder treat differently (malformed UTF-8): the caller takes the decoder.
static int cp_masks_via_bytes(Ctx& g, LeadFront a, LeadPlanes* planes, int64_t* total_cps_out, int* fallback_out) {
    int rc;
    *fallback_out = 0;
    Workspace& w = g.ws;
    // DevBuf::ensure frees on growth, and the planes of this front stay live through the compaction that follows: the workspace is
    // sized here, once, with everything that compaction will ask for, at the byte count.  enqueue_compaction_dev's own ws_ensure (a
    // sub-shape at the code-point count, which is no larger) then finds nothing to grow.  flow_reserve does the same for a slot.
    if ((rc = ws_ensure(ws_needs(w, a.b.total, WsShape{.spans = a.space, .feats = a.codes, .cp_rows = a.b.n_str + 1}).data(), kWsNeeds)) ||
        (rc = g.pin_tot.ensure(64)))
        return rc;
    volatile int64_t* h_tot = (volatile int64_t*)g.pin_tot.h;
    int64_t* p_tot = (int64_t*)g.pin_tot.d;
    h_tot[0] = 0;
    h_tot[1] = 0;
    h_tot[3] = 0;
    a.r_cps = p_tot;
    a.r_err = (int*)(p_tot + 1);
    a.r_odd = (int*)(p_tot + 3);
    if ((rc = enqueue_lead_front(g, w, a, planes))) return rc;
    HIP_TRY(hipStreamSynchronize(a.st));
    if (h_tot[1] != 0) { w.chain_ready = false; return fail(LATOK_ERR_HIP, "internal: the chained scan did not complete (flag %lld)", (long long)h_tot[1]); }
    if (h_tot[3] != 0) { *fallback_out = 1; return LATOK_OK; }
    *total_cps_out = h_tot[0];
    return LATOK_OK;
}

// featurize of a UTF-8 batch in BYTE space (latok_token_features_utf8_bytes_batch and its flow form): span records in byte
// positions, feature sums per CHAR.  A token has the same rank in byte space and in code-point space, so two writers share one
// record index: k_counts_scatter<2> puts the four byte positions from the byte-space masks, k_features_tiles (without span records)
// the sums from the packed code-point masks and the rule codes.  One stream, nothing waits for the host:
//   enqueue_lead_front (SPACE plane, codes)         byte-space masks, packed code-point masks, code-point row offsets, rule codes;
//                                                   code-point total -> r_cps and the workspace's scalar word 1; malformed -> r_odd
//   k_word_counts + k_scan_chained (byte masks)     kept mask / item ranks in byte space; THE token total -> scalar word 0, r_items
//   k_counts_scatter<2>                             counts + byte records        (gates: total <= cap, *r_odd == 0)
//   tile index (code-point rows), k_word_counts + k_scan_chained (code-point masks)    item ranks in code-point space
//   k_features_tiles                                the sums                     (the same two gates)
// The three scans share the workspace's rank arrays (bases / wcnt / wpref) and kept mask: every consumer of one scan has been
// enqueued before the next scan overwrites them, and the stream orders them.  The token total is written once, by the byte-space
// scan (the code-point scan's own total goes to scalar word 2 and to no result word), and gates both writers.  Sizes behind the
// lead scan are the byte count, an upper bound (DeviceTotal).  `w` was sized by ws_needs with WsShape{.spans = true, .feats = true, .cp_rows = n_str + 1}.
struct Utf8BytesFeats {
    Batch b;                      // UTF-8 bytes on the device, byte offsets, total in bytes (> 0), n_str > 0
    bool o32 = false;
    void* counts = nullptr;
    void* items = nullptr;
    int8_t* feat = nullptr;
    int64_t cap = 0;
    int64_t* r_items = nullptr;   // the four result words as the device sees them (cleared by the caller): token total,
    int64_t* r_err = nullptr;     // int32-overflow flag (low half) | scan flag (high half),
    int64_t* r_cps = nullptr;     // code-point total,
    int64_t* r_odd = nullptr;     // malformed-input flag
    hipStream_t st = nullptr;
};
static int enqueue_utf8_bytes_features(Ctx& g, Workspace& w, const Utf8BytesFeats& a) {
    int rc;
    const hipStream_t st = a.st;
    const int64_t n_str = a.b.n_str, total_bytes = a.b.total;
    int* d_err = (int*)a.r_err;
    const int* d_odd = (const int*)a.r_odd;
    const LeadFront f{.b = a.b, .space = true, .codes = true, .r_cps = a.r_cps, .r_err = d_err, .r_odd = (int*)a.r_odd, .st = st};
    LeadPlanes t;
    if ((rc = enqueue_lead_front(g, w, f, &t))) return rc;
    HIP_TRY(latok::launch_pad_codes(t.codes, t.total_cps, total_bytes, st));
    latok::ChainState chain;
    // byte space: kept tokens, their ranks, the total (scalar word 0); counts and the four byte positions of every token (the lead ranks are spent)
    const latok::TokenPlanes pb = token_planes(w, a.b.row, n_str, total_bytes, true, t.bmask, t.bspace);
    if ((rc = next_scan_epoch(w, st, &chain))) return rc;
    HIP_TRY(latok::launch_word_counts_scan(true, pb, chain, a.r_items, d_err + 1, st));
    HIP_TRY(latok::launch_counts_scatter(2, a.o32, pb, a.items, a.cap, a.counts, d_err, st, latok::DoneSignal{nullptr, 0, nullptr},
                                         latok::DeviceTotal{nullptr, d_odd}));
    // code-point space: the same tokens on the packed masks (the byte-space ranks and kept mask are spent); sums only
    const latok::DeviceTotal dt{t.total_cps, d_odd};
    Pipe q;
    q.b = Batch{Input{}, t.cp_row, n_str, total_bytes};
    q.stages = 1;
    q.st = st;
    if ((rc = run_pipeline(g, w, q))) return rc;
    latok::TokenPlanes pc = token_planes(w, t.cp_row, n_str, total_bytes, true, t.cpbits, t.cpspace);
    pc.n_items += 2;   // (this scan's own total goes to scalar word 2 and to no result word ...
    if ((rc = next_scan_epoch(w, st, &chain))) return rc;
    HIP_TRY(latok::launch_word_counts_scan(true, pc, chain, nullptr, d_err + 1, st, dt));
    pc.n_items = pb.n_items;   // ... THE token total, the byte-space scan's, gates the sums as it gates the records)
    return enqueue_features(g, t.codes, pc, nullptr, a.feat, a.o32, a.cap, st, latok::DoneSignal{nullptr, 0, nullptr}, dt);
}

// Joined token text of a UTF-8 batch in BYTE space (latok_join_tokens_utf8_bytes_batch and its flow form): for every string its
// stripped, non-empty tokens joined by one separator byte (sep.join(tokenize(text)), reference default_tokenizer.py:149-160).
// One stream, nothing waits for the host:
//   tile index -> byte-space tiles -> resolve          boundary mask, smeared SPACE plane over the BYTES
//   [k_word_counts + k_scan_chained, k_counts_scatter  kept mask and token ranks, per-string token counts -- only when counts are asked for]
//   k_join_counts                                      body / head planes, output bytes per word and per tile
//   k_scan_chained                                     tile ranks; THE byte total -> scalar word 0, r_bytes
//   k_join_scatter                                     the bytes (gate: total <= cap), out_off; bit 2 of the error word if the total exceeds cap
// Every batch size takes this route: there is no one-launch form and no host decode, so a batch gives the same bytes at every size.
// `w` was sized by ws_needs with WsShape{.spans = true, .join = true}.
struct JoinTokens {
    Batch b;                      // UTF-8 bytes on the device, byte offsets, total in bytes (> 0), n_str > 0
    int sep = ' ';
    uint8_t* out = nullptr;       // NULL: a size query
    int64_t cap = 0;
    int64_t* out_off = nullptr;   // int64[n_str + 1]
    void* counts = nullptr;       // NULL: not asked for
    bool o32 = false;             // width of the counts
    int64_t* r_bytes = nullptr;   // the two result words as the device sees them (cleared by the caller): output bytes,
    int64_t* r_err = nullptr;     // int32-overflow flag (bit 0) | capacity flag (bit 2) in the low half, scan flag in the high half
    hipStream_t st = nullptr;
};
static int enqueue_join_tokens(Ctx& g, Workspace& w, const JoinTokens& a) {
    int rc;
    const hipStream_t st = a.st;
    const int64_t n_str = a.b.n_str, total = a.b.total;
    latok::TokenPlanes t = token_planes(w, a.b.row, n_str, total);
    const int64_t words = t.n_words, c_tiles = (words + 63) / 64;
    int64_t* d_rank = (int64_t*)w.bases.p;
    int64_t* d_tcnt = (int64_t*)w.wcnt.p;
    uint16_t* d_pref = (uint16_t*)w.wpref.p;
    int64_t* d_total = (int64_t*)w.scalar.p;        // word 0: the byte total (word 2: the token total of the counts)
    int* d_err = (int*)a.r_err;
    latok::ChainState chain;
    Pipe p;
    p.b = a.b;
    p.bits = (uint64_t*)w.bits.p;
    p.space = (uint64_t*)w.space.p;
    p.st = st;
    if ((rc = run_pipeline(g, w, p))) return rc;
    if (a.counts) {   // the token counts of the spans call, by its own kernels (the ranks are spent once the counts are written)
        t.n_items = d_total + 2;
        if ((rc = next_scan_epoch(w, st, &chain))) return rc;
        HIP_TRY(latok::launch_word_counts_scan(true, t, chain, nullptr, d_err + 1, st));
        HIP_TRY(latok::launch_counts_scatter(1, a.o32, t, nullptr, 0, a.counts, d_err, st));
    }
    uint64_t* d_body = (uint64_t*)w.jbody.p;
    uint64_t* d_head = (uint64_t*)w.jhead.p;
    if ((rc = next_scan_epoch(w, st, &chain))) return rc;
    HIP_TRY(latok::launch_join_counts(t.bits, t.space, words, total, a.b.row, n_str, t.tile_first, d_body, d_head, d_tcnt, d_pref, st));
    HIP_TRY(latok::launch_tile_scan(d_tcnt, c_tiles, d_rank, chain, d_total, a.r_bytes, d_err + 1, st));
    HIP_TRY(latok::launch_join_scatter((const uint8_t*)a.b.in.p, total, d_body, d_head, d_rank, d_tcnt, d_pref, words, a.b.row, n_str, a.sep, a.out,
                                       a.cap, d_total, a.out_off, d_err, st));
    return LATOK_OK;
}

// The front of the byte-space token calls (hashes and ids, term counts, WordPiece, counting): the two bitmasks over the BYTES, then the
// kept tokens, their ranks and their total.  One stream, nothing waits for the host:
//   tile index -> byte-space tiles -> resolve     boundary mask, smeared SPACE plane over the BYTES
//   k_word_counts + k_scan_chained                kept mask, token ranks; THE token total -> scalar word 0, r_tokens
// d_err = the call's error word; the scan's own flag goes to its high half.  `w` was sized by ws_needs with a shape that has
// .spans = true.  What comes back are the workspace's planes, for the launches that follow.
// pretok = LATOK_PRETOK_GPT2: the first line is ONE launch instead, k_pretok_planes (pretok_kernels.hip): a bit at every byte where a
// pre-token of GPT-2's pattern starts, an all-zero SPACE plane (every pre-token is kept, nothing is stripped) and the per-tile string
// index, in the same buffers.  The context's rule tables play no part in it.
// pretok = LATOK_PRETOK_CL100K: TWO launches instead (k_pretok_cl100k_records, k_pretok_cl100k_planes), which leave the same three for
// the cl100k / Llama 3 pattern; the carry records of the tiles between the two live in w.summ.
// pretok = LATOK_PRETOK_SPM: ONE launch, k_pretok_spm_planes: SentencePiece's segments (spbpe.h) by k_pretok_planes' geometry.
static int enqueue_token_front(Ctx& g, Workspace& w, const Batch& b, int64_t* r_tokens, int* d_err, hipStream_t st, latok::TokenPlanes* out,
                               int pretok = kPretokLatok) {
    int rc;
    *out = token_planes(w, b.row, b.n_str, b.total);
    latok::ChainState chain;
    if (pretok == kPretokGpt2) {
        HIP_TRY(latok::launch_pretok_planes((const uint8_t*)b.in.p, b.total, b.row, b.n_str, (uint64_t*)w.bits.p, (uint64_t*)w.space.p,
                                            (int64_t*)w.tile_first.p, st));
    } else if (pretok == kPretokSpm) {
        HIP_TRY(latok::launch_pretok_spm_planes((const uint8_t*)b.in.p, b.total, b.row, b.n_str, (uint64_t*)w.bits.p, (uint64_t*)w.space.p,
                                                (int64_t*)w.tile_first.p, st));
    } else if (pretok == kPretokCl100k) {
        HIP_TRY(latok::launch_pretok_cl100k_planes((const uint8_t*)b.in.p, b.total, b.row, b.n_str, (uint32_t*)w.summ.p, (uint64_t*)w.bits.p,
                                                   (uint64_t*)w.space.p, (int64_t*)w.tile_first.p, st));
    } else {
        Pipe p;
        p.b = b;
        p.bits = (uint64_t*)w.bits.p;
        p.space = (uint64_t*)w.space.p;
        p.st = st;
        if ((rc = run_pipeline(g, w, p))) return rc;
    }
    if ((rc = next_scan_epoch(w, st, &chain))) return rc;
    HIP_TRY(latok::launch_word_counts_scan(true, *out, chain, r_tokens, d_err + 1, st));
    return LATOK_OK;
}
// The front of the sized calls (term counts, n-grams, WordPiece), which need the token total on the host: enqueue_token_front with the
// pinned words (p_tot / h_tot: word 0 tokens, word 1 the error word), wait 1, then the refusal of 2^31 tokens or more in the caller's
// words (`too_many`, one %lld).  The caller sizes its buffers by *n_tok.
static int sized_token_front(Ctx& g, Workspace& w, const Batch& b, int64_t* p_tot, const volatile int64_t* h_tot, hipStream_t st,
                             const char* too_many, latok::TokenPlanes* t, int64_t* n_tok, int pretok = kPretokLatok) {
    int rc;
    if ((rc = enqueue_token_front(g, w, b, p_tot, (int*)(p_tot + 1), st, t, pretok))) return rc;
    HIP_TRY(hipStreamSynchronize(st));   // wait 1: the token total decides whether the call goes on and what its buffers take
    if ((rc = finish_totals(w, h_tot, 0, n_tok))) return rc;
    if (*n_tok >= (1ll << 31)) return fail(LATOK_ERR_INVALID, too_many, (long long)*n_tok);
    return LATOK_OK;
}
// The token rows of the n-gram and WordPiece calls, behind sized_token_front (n_tok > 0, w.wpspans sized for it): the span record of
// every token at its rank (k_counts_scatter, kind 1, int64) into w.wpspans, the token count of every string into d_cnt (n_str + 1,
// cleared by the caller) and the row starts in token space into d_start (k_scan_chained; the total -> scalar word 4).  *text = the
// batch in token space, for the kernels that take one token per lane.
static int enqueue_token_rows(Workspace& w, const Batch& b, const latok::TokenPlanes& t, int64_t n_tok, int64_t* d_cnt, int64_t* d_start, int* d_err,
                              hipStream_t st, latok::TokenText* text) {
    HIP_TRY(latok::launch_counts_scatter(1, false, t, (int64_t*)w.wpspans.p, n_tok, d_cnt, d_err, st));
    *text = {(const uint32_t*)b.in.p, b.total, b.row, b.n_str, d_start, (const int64_t*)w.wpspans.p, n_tok};
    return enqueue_row_scan(w, d_cnt, b.n_str + 1, d_start, (int64_t*)w.scalar.p + 4, nullptr, d_err + 1, st);
}
// "Wait 2" of a sized call whose second total sizes buffers: the wait, the scan's own flag, then the total that the stream left in
// pinned word `word`; 2^31 or more is refused in the caller's words (`too_many`, one %lld; NULL: the caller refuses it itself).
static int second_sized_total(Workspace& w, const volatile int64_t* h_tot, int word, hipStream_t st, const char* too_many, int64_t* out) {
    int rc;
    HIP_TRY(hipStreamSynchronize(st));   // the total decides whether the call goes on and what its buffers take
    if ((rc = finish_totals(w, h_tot, 0, out))) return rc;   // (leaves the token total again, which wait 1 has delivered)
    *out = h_tot[word];
    if (too_many && *out >= (1ll << 31)) return fail(LATOK_ERR_INVALID, too_many, (long long)*out);
    return LATOK_OK;
}

// Token hashes and token ids of a UTF-8 batch in BYTE space (latok_token_hashes_utf8_bytes_batch, latok_token_ids_utf8_bytes_batch and
// their flow forms): one 32-bit word per stripped, non-empty token (the tokens of default_tokenizer.py:149-160, as
// latok_token_spans_utf8_bytes_batch cuts them), at the token's rank.  The hashed form stores the token's MurmurHash3 x86_32; the ids
// form keeps the hash in its lane and finds the token's slot in the vocabulary table, the bytes decide.  One stream, nothing waits
// for the host:
//   enqueue_token_front                           kept mask, token ranks; THE token total -> scalar word 0, r_tokens
//   k_hash_scatter / k_vocab_scatter              counts, the span records (if asked for) and the words (gate: total <= cap)
// Every batch size takes this route: there is no one-launch form and no host decode, so a batch gives the same words at every size.
// `w` was sized by ws_needs with WsShape{.spans = true}.
struct Vocab {                     // latok_vocab: immutable once created
    int device = -1;
    int64_t n_words = 0;
    uint32_t seed = 0;
    DevTable table;
};
struct TokenWords {
    Batch b;                       // UTF-8 bytes on the device (16-byte aligned), byte offsets, total in bytes (> 0), n_str > 0
    const Vocab* vocab = nullptr;  // NULL: the hashed form
    uint32_t seed = 0;             // of the hashed form (the ids form hashes with its vocabulary's)
    int32_t unk = -1;              // ids form: the id of a token that is not in the vocabulary
    void* counts = nullptr;        // NULL: not asked for
    void* spans = nullptr;         // NULL: not asked for
    void* words = nullptr;         // uint32 hashes / int32 ids; NULL: a size query
    int64_t cap = 0;               // in tokens
    bool o32 = false;              // width of the counts and records
    int64_t* r_tokens = nullptr;   // the two result words as the device sees them (cleared by the caller): tokens,
    int64_t* r_err = nullptr;      // int32-overflow flag (bit 0) in the low half, scan flag in the high half
    hipStream_t st = nullptr;
};
static int enqueue_token_words(Ctx& g, Workspace& w, const TokenWords& a) {
    int rc;
    int* d_err = (int*)a.r_err;
    latok::TokenPlanes t;
    if ((rc = enqueue_token_front(g, w, a.b, a.r_tokens, d_err, a.st, &t))) return rc;
    const uint8_t* u8 = (const uint8_t*)a.b.in.p;
    void* spans = a.words ? a.spans : nullptr;   // the records are written only when the words are
    if (!a.vocab) {
        HIP_TRY(latok::launch_hash_scatter(a.o32, t, u8, a.seed, spans, (uint32_t*)a.words, a.cap, a.counts, d_err, a.st));
        return LATOK_OK;
    }
    const latok::VocabTable vt = a.vocab->table.view(a.vocab->seed);
    HIP_TRY(latok::launch_vocab_scatter(a.o32, t, u8, vt, a.unk, spans, (int32_t*)a.words, a.cap, a.counts, d_err, a.st));
    return LATOK_OK;
}
// The blocking call behind compact_common's checks: b = the caller's UTF-8 batch (total resolved, n_str > 0, total > 0).  Every
// batch that the host did not decode takes this route, whatever its size.  One synchronisation.
static int features_utf8_bytes_route(Ctx& g, const Batch& b, bool dev, bool o32, void* counts_out, void* items_out, int8_t* features_out,
                                     int64_t items_cap, int64_t* n_items_out, hipStream_t st) {
    int rc;
    const int64_t n_str = b.n_str, total_bytes = b.total;
    BytesCall c;
    c.adopt(b, dev, o32, st);
    // pinned result words: 0 = tokens, 1 = flags, 3 = malformed, 4 = code points (2 is the small path's completion word)
    if ((rc = c.stage(g, 4, WsShape{.spans = true, .feats = true, .cp_rows = n_str + 1}, kClearBytesFeats))) return rc;
    Utf8BytesFeats a;
    a.b = c.d;
    a.o32 = o32;
    a.counts = counts_out;
    a.items = items_out;
    a.feat = features_out;
    // (a batch has at most one token per byte: a larger capacity gates nothing, and the staging below is sized by it)
    a.cap = items_out ? std::min(items_cap, total_bytes) : 0;
    if (!dev) {
        if ((rc = g.counts.ensure((size_t)n_str * 8)) || (rc = g.h_out.ensure((size_t)a.cap * 4 * c.elt + 16)) ||
            (rc = g.h_aux.ensure((size_t)a.cap * LATOK_FEATURE_COUNT + 16)))
            return rc;
        a.counts = g.counts.p;
        a.items = g.h_out.p;
        a.feat = (int8_t*)g.h_aux.p;
    }
    a.r_items = c.p_tot;
    a.r_err = c.p_tot + 1;
    a.r_odd = c.p_tot + 3;
    a.r_cps = c.p_tot + 4;
    a.st = st;
    if ((rc = enqueue_utf8_bytes_features(g, g.ws, a))) return rc;
    int64_t n_items = 0;
    // (mask 0: malformed input is refused before an int32 overflow, so the overflow flag is read behind that check)
    if ((rc = c.wait_totals(g, 0, &n_items))) return rc;
    if (c.h_tot[3] != 0)
        return fail(LATOK_ERR_INVALID, "malformed UTF-8 (a continuation byte without a lead byte): no feature sums in byte space; "
                                       "latok_token_features_utf8_batch reads such input through the decoder");
    if (c.h_tot[1] & 0xFFFFFFFFll) return refuse_too_long();
    *n_items_out = n_items;
    return deliver_records(false, dev ? nullptr : g.counts.p, g.h_out.p, g.h_aux.p, counts_out, items_out, features_out, n_str, c.elt, 4 * c.elt,
                           n_items, items_cap, st);
}

// Code-point results of a UTF-8 batch in a blocking compaction call (b: n_str > 0, total resolved): what the kernels read instead of
// the bytes, in k->b and k->pre_*, and the route in g.last_route.  Route 3, large batches: the byte-space kernel + the masks packed at
// the lead bytes (no UTF-32 copy of the batch); the compaction then runs on the code-point masks (featurize: and on the rule codes
// k_lead_codes stores at the code-point positions), sized by the code-point total the host has read.  Route 2, small batches and
// malformed input: the decoder first -- or, with no multi-byte char in the batch, the bytes themselves: byte space == code-point space.
static int cp_units_route(Ctx& g, const Batch& b, bool dev, bool spans, bool feats, hipStream_t st, Compaction* k) {
    int rc;
    int64_t total_cps = 0;
    if (b.total > kSmallChars && (!dev || ((uintptr_t)b.in.p & 15) == 0)) {
        Batch bytes;
        int fallback = 0;
        LeadPlanes t;
        if ((rc = units_on_device(g, b, dev, st, &bytes)) ||
            (rc = cp_masks_via_bytes(g, LeadFront{.b = bytes, .space = spans, .codes = feats, .st = st}, &t, &total_cps, &fallback)))
            return rc;
        if (!fallback) {
            g.last_route = 3;
            k->b = Batch{Input{}, t.cp_row, b.n_str, total_cps};
            k->pre_bits = t.cpbits;
            k->pre_space = t.cpspace;
            k->pre_codes = t.codes;
            return LATOK_OK;
        }
    }
    g.last_route = 2;
    Batch ascii;   // (featurize needs the rule codes of the UTF-32 tile kernel: it always decodes)
    if ((rc = decode_utf8_to_workspace(g, b, dev, st, &total_cps, feats ? nullptr : &ascii))) return rc;
    k->b = ascii.in.p ? ascii : Batch{Input{g.h_cps.p, Form::Utf32}, (const int64_t*)g.u_row.p, b.n_str, total_cps};
    return LATOK_OK;
}

// Shared body of the compaction entry points: argument checks, staging of host-pointer batches, one synchronisation.
// cp_units: a UTF-8 batch (b.row = byte offsets, b.total = bytes) whose results are in code-point units.
static int compact_common(Ctx& g, bool spans, bool feats, Batch b, bool cp_units, void* counts_out, void* items_out, int8_t* features_out,
                          int64_t items_cap, int64_t* n_items_out, int flags, void* stream) {
    const bool o32 = (flags & LATOK_OUT_INT32) != 0;
    int rc = need_init(g);
    if (rc) return rc;
    if (!n_items_out) return fail(LATOK_ERR_INVALID, "the total-count output pointer is NULL");
    *n_items_out = 0;
    if (items_cap < 0) return fail(LATOK_ERR_INVALID, "negative capacity");
    const bool dev = (flags & LATOK_DEVICE_PTRS) != 0;
    const int64_t* row_off = b.row;
    const int64_t n_str = b.n_str;
    if (o32 && !dev && row_off && n_str > 0) {   // before anything is staged (device-resident row offsets: the kernel checks)
        for (int64_t s = 0; s < n_str; ++s)
            if (row_off[s + 1] - row_off[s] > 0x7FFFFFFFll)
                return fail(LATOK_ERR_INVALID, "string %lld is too long for LATOK_OUT_INT32; use the 64-bit form", (long long)s);
    }
    if (!dev && (rc = check_csr_host(row_off, n_str, &b.total))) return rc;   // (device row offsets: below, on the call's stream)
    // Small well-formed UTF-8 host batches (one string per call is the usual C caller) are decoded by the host
    // (host_decode_small) and take the pinned small-batch path of the code-point form; byte-space results are mapped back:
    // a char position becomes the byte position of that char, relative to its string.
    g.last_route = 0;
    if (!dev && b.in.form == Form::Utf8 && b.in.p && counts_out && n_str <= kSmallStrings && b.total > 0 && b.total <= kSmallChars &&
        host_decode_small((const uint8_t*)b.in.p, row_off, n_str, g.hd_cps, g.hd_row, g.hd_pos)) {
        const Batch cps{Input{g.hd_cps.data(), Form::Utf32}, g.hd_row.data(), n_str, (int64_t)g.hd_cps.size()};
        rc = compact_common(g, spans, feats, cps, false, counts_out, items_out, features_out, items_cap, n_items_out, flags, stream);
        g.last_route = 1;
        if (rc != LATOK_OK || cp_units || !items_out) return rc;
        const int64_t per = feats ? 4 : (spans ? 2 : 1);
        int64_t k = 0;
        for (int64_t s = 0; s < n_str; ++s) {
            const int64_t n = o32 ? (int64_t)((const int32_t*)counts_out)[s] : ((const int64_t*)counts_out)[s];
            const int64_t c0 = g.hd_row[(size_t)s], b0 = row_off[s];
            for (int64_t j = 0; j < n * per; ++j, ++k) {
                if (o32) { int32_t* v = (int32_t*)items_out + k; *v = (int32_t)(g.hd_pos[(size_t)(c0 + *v)] - b0); }
                else { int64_t* v = (int64_t*)items_out + k; *v = g.hd_pos[(size_t)(c0 + *v)] - b0; }
            }
        }
        return LATOK_OK;
    }
    StreamTurn turn(g, stream);
    hipStream_t st = turn.st;
    if (dev) {
        if ((rc = resolve_total_device(row_off, n_str, &b.total, st))) return rc;
        if (b.in.form == Form::Utf32 && b.total > 0 && ((uintptr_t)b.in.p & 15) != 0)
            return fail(LATOK_ERR_INVALID, "device cps pointer must be 16-byte aligned");
    }
    if (n_str == 0) return LATOK_OK;
    if (!counts_out) return fail(LATOK_ERR_INVALID, "counts_out is NULL");
    if (b.total > 0 && !b.in.p) return fail(LATOK_ERR_INVALID, "NULL buffer");
    const size_t elt = o32 ? 4 : 8;                                   // width of counts and of every record field
    const size_t item_bytes = (feats ? 4 : (spans ? 2 : 1)) * elt;
    if (feats && b.in.form == Form::Utf8 && !cp_units) {   // featurize in byte space: a route of its own
        if (b.total == 0) return zero_counts(dev, counts_out, (size_t)n_str * elt, st);
        return features_utf8_bytes_route(g, b, dev, o32, counts_out, items_out, features_out, items_cap, n_items_out, st);
    }
    if (!dev && !cp_units && b.total >= kPipeMinChars)
        return compact_host_pipelined(g, spans, feats, o32, b, counts_out, items_out, items_cap, n_items_out, features_out, st);
    Compaction k;
    k.b = b;
    if (cp_units && (rc = cp_units_route(g, b, dev, spans, feats, st, &k))) return rc;
    Batch& d = k.b;   // the batch as the kernels read it (UTF-8 in code-point units: the route's, with its masks and codes in k.pre_*)
    const int64_t total = d.total;
    if (total == 0) return zero_counts(dev, counts_out, (size_t)n_str * elt, st);   // only empty strings
    // small host batch: inputs and every output live in pinned mapped memory; nothing is copied by the runtime and the
    // call synchronises once (a string of ~100 chars: ~110 us of blocking copies otherwise)
    const bool small = !dev && (b.in.form == Form::Utf32 || b.in.narrow()) && total <= kSmallChars && n_str <= kSmallStrings;
    size_t po_row = 0, po_counts = 0, po_items = 0, po_feat = 0;
    if (small) {
        po_row = align16((size_t)total * 4);
        po_counts = po_row + align16((size_t)(n_str + 1) * 8);
        po_items = po_counts + align16((size_t)n_str * elt);
        po_feat = po_items + (size_t)total * item_bytes;      // at most one item per char
        if ((rc = g.pin.ensure(po_feat + (feats ? (size_t)total * LATOK_FEATURE_COUNT : 0) + 64))) return rc;
        // Narrow units (the C-extension caller of INTEGRATION.md section C hands over ONE str per call in its PEP 393 kind)
        // are widened to UTF-32 by the host straight into the pinned area: positions are chars either way, so the results
        // are the same, and the call costs one launch instead of staged copies (kind 1, one 105-char string: 110 -> 17 us).
        uint32_t* w = (uint32_t*)g.pin.h;
        if (b.in.form == Form::Utf32) {
            memcpy(w, b.in.p, (size_t)total * 4);
        } else if (b.in.form == Form::Ucs2) {
            for (int64_t i = 0; i < total; ++i) { uint16_t u; memcpy(&u, (const char*)b.in.p + 2 * i, 2); w[i] = u; }
        } else {
            for (int64_t i = 0; i < total; ++i) w[i] = ((const uint8_t*)b.in.p)[i];
        }
        memcpy((char*)g.pin.h + po_row, row_off, (size_t)(n_str + 1) * 8);
        d.in = Input{g.pin.d, Form::Utf32};
        d.row = (const int64_t*)((char*)g.pin.d + po_row);
    } else if (!dev && b.in.form == Form::Utf32) {
        if ((rc = g.h_cps.ensure((size_t)total * 4 + 16))) return rc;
        if ((rc = g.h_row.ensure((size_t)(n_str + 1) * 8))) return rc;
        HIP_TRY(hipMemcpyAsync(g.h_cps.p, b.in.p, (size_t)total * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(g.h_row.p, row_off, (size_t)(n_str + 1) * 8, hipMemcpyHostToDevice, st));
        d.in.p = g.h_cps.p;
        d.row = (const int64_t*)g.h_row.p;
    } else if (!dev && !cp_units && (rc = units_on_device(g, b, false, st, &d))) {   // narrow units, UTF-8 in byte space
        return rc;
    }
    if ((rc = g.pin_tot.ensure(64))) return rc;
    volatile int64_t* h_tot = (volatile int64_t*)g.pin_tot.h;
    int64_t* p_tot = (int64_t*)g.pin_tot.d;
    // where the records go: the caller's device buffers, the pinned area, or (host pointers, mid-size batch) device staging
    // sized for the worst case of one item per char
    k.spans = spans;
    k.feats = feats;
    k.o32 = o32;
    k.counts = counts_out;
    k.items = items_out;
    k.feat = features_out;
    k.cap = items_out ? items_cap : 0;
    if (small) {
        k.counts = (char*)g.pin.d + po_counts;
        k.items = (char*)g.pin.d + po_items;
        k.feat = (int8_t*)((char*)g.pin.d + po_feat);
        k.cap = total;
    } else if (!dev) {
        if ((rc = g.counts.ensure((size_t)n_str * 8))) return rc;
        if ((rc = g.h_out.ensure((size_t)total * item_bytes))) return rc;
        if (feats && (rc = g.h_aux.ensure((size_t)total * LATOK_FEATURE_COUNT))) return rc;
        k.counts = g.counts.p;
        k.items = g.h_out.p;
        k.feat = (int8_t*)g.h_aux.p;
        k.cap = total;
    }
    latok::DoneSignal done{nullptr, 0, nullptr};
    if (small && total <= latok::kTile) {
        // at most one tile (tokenize(text) / featurize(text): one string per call): one single-wave launch does everything
        // and stores a completion word the host polls
        latok::SplitParams P;
        memset(&P, 0, sizeof(P));
        P.cps = (const uint32_t*)d.in.p;
        P.row_off = d.row;
        P.n_str = n_str;
        P.total = total;
        P.n_tiles = 1;
        const uint8_t* tables = (const uint8_t*)((g.rules_on || feats) ? g.t1rule.p : g.t1.p);   // featurize needs rule codes
        P.t1 = tables;
        P.t2 = tables + latok::kStage1Pad;
        if (g.rules_on) P.rules = g.rules;
        h_tot[0] = 0;
        h_tot[1] = 0;
        done = latok::DoneSignal{poll_completion() ? (unsigned long long*)(p_tot + 2) : nullptr, ++g.small_seq, nullptr};
        HIP_TRY(latok::launch_small_batch(P, g.rules_on, feats ? 2 : (spans ? 1 : 0), o32, k.counts, k.items, k.feat, p_tot, done.word,
                                          done.seq, st));
    } else {
        // several tiles in pinned memory: the last kernel's workgroups count themselves in and the last one stores the
        // completion word (latok::DoneSignal)
        if (small && (rc = arm_done(g, st, &k.done))) return rc;
        k.p_tot = p_tot;
        k.h_tot = h_tot;
        k.st = st;
        if ((rc = enqueue_compaction_dev(g, g.ws, k))) return rc;
        done = k.done;
    }
    // the one synchronisation: total and flag are in pinned memory now (a polled small batch has seen its completion
    // word, which the kernel stores after everything else; the launch itself retires on the stream a moment later)
    if ((rc = wait_done(g, done, st))) return rc;
    int64_t n_items = *n_items_out = h_tot[0];   // (the total is reported whatever the flags say)
    if ((rc = finish_totals(g.ws, h_tot, 0xFFFFFFFFll, &n_items))) return rc;
    const char* pin = (const char*)g.pin.h;
    if (small) return deliver_records(true, pin + po_counts, pin + po_items, feats ? pin + po_feat : nullptr, counts_out, items_out, features_out,
                                      n_str, elt, item_bytes, n_items, items_cap, st);
    return deliver_records(false, dev ? nullptr : g.counts.p, g.h_out.p, feats ? g.h_aux.p : nullptr, counts_out, items_out, features_out, n_str,
                           elt, item_bytes, n_items, items_cap, st);
}

int latok_split_offsets_batch(const uint32_t* cps, const int64_t* row_off, int64_t n_str, int64_t total,
                              int64_t* counts_out, int64_t* offsets_out, int64_t offsets_cap, int64_t* n_offsets_out,
                              int flags, void* stream) {
    LATOK_ENTER();
    return compact_common(g, false, false, Batch{Input{cps, Form::Utf32}, row_off, n_str, total}, false, counts_out, offsets_out, nullptr,
                          offsets_cap, n_offsets_out, flags, stream);
}

int latok_token_spans_batch(const uint32_t* cps, const int64_t* row_off, int64_t n_str, int64_t total,
                            int64_t* counts_out, int64_t* spans_out, int64_t spans_cap, int64_t* n_tokens_out, int flags,
                            void* stream) {
    LATOK_ENTER();
    return compact_common(g, true, false, Batch{Input{cps, Form::Utf32}, row_off, n_str, total}, false, counts_out, spans_out, nullptr,
                          spans_cap, n_tokens_out, flags, stream);
}

int latok_utf8_decode_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes,
                            uint32_t* cps_out, int64_t cps_cap, int64_t* cp_row_off_out, int64_t* total_cps_out, int flags,
                            void* stream) {
    LATOK_ENTER();
    int rc = need_init(g);
    if (rc) return rc;
    if (!total_cps_out) return fail(LATOK_ERR_INVALID, "total_cps_out is NULL");
    StreamTurn turn(g, stream);
    hipStream_t st = turn.st;
    const bool dev = (flags & LATOK_DEVICE_PTRS) != 0;
    int64_t total_cps = 0;
    if ((rc = resolve_total(byte_off, n_str, &total_bytes, dev, st))) return rc;
    if ((rc = decode_utf8_to_workspace(g, Batch{Input{utf8, Form::Utf8}, byte_off, n_str, total_bytes}, dev, st, &total_cps))) return rc;
    *total_cps_out = total_cps;
    if (n_str == 0) return LATOK_OK;
    if (total_cps > cps_cap) return fail(LATOK_ERR_INVALID, "cps_cap too small: need %lld", (long long)total_cps);
    if (!cp_row_off_out || (total_cps > 0 && !cps_out)) return fail(LATOK_ERR_INVALID, "NULL output buffer");
    const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (total_cps > 0) HIP_TRY(hipMemcpyAsync(cps_out, g.h_cps.p, (size_t)total_cps * 4, kind, st));
    HIP_TRY(hipMemcpyAsync(cp_row_off_out, g.u_row.p, (size_t)(n_str + 1) * 8, kind, st));
    HIP_TRY(hipStreamSynchronize(st));
    return LATOK_OK;
}

// b: the caller's UTF-8 batch, total resolved
static int mask_utf8_via_bytes(Ctx& g, const Batch& b, bool dev, uint64_t* mask_bits_out, int64_t mask_cap_words, int64_t* cp_row_off_out,
                               int64_t* total_cps_out, hipStream_t st, int* fallback_out) {
    int rc;
    Batch d;
    if ((rc = units_on_device(g, b, dev, st, &d))) return rc;
    const int64_t words_b = (b.total + 63) / 64;
    const int64_t out_words = mask_cap_words < words_b ? mask_cap_words : words_b;   // (a batch has at most one char per byte)
    uint64_t* d_out = mask_bits_out;
    if (!dev) {   // (the row offsets of a host call: the workspace's)
        if ((rc = g.h_out.ensure((size_t)out_words * 8 + 8))) return rc;
        d_out = (uint64_t*)g.h_out.p;
    }
    int64_t total_cps = 0;
    LeadPlanes t;
    const LeadFront a{.b = d, .cpbits = d_out, .cap_words = out_words, .cp_row = dev ? cp_row_off_out : nullptr, .st = st};
    if ((rc = cp_masks_via_bytes(g, a, &t, &total_cps, fallback_out))) return rc;
    if (*fallback_out) return LATOK_OK;
    *total_cps_out = total_cps;
    const int64_t words = (total_cps + 63) / 64;
    if (words > mask_cap_words) return fail(LATOK_ERR_INVALID, "mask_cap_words too small: need %lld", (long long)words);
    if (!dev) {
        if (words > 0) HIP_TRY(hipMemcpyAsync(mask_bits_out, d_out, (size_t)words * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(cp_row_off_out, t.cp_row, (size_t)(b.n_str + 1) * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return LATOK_OK;
}

int latok_split_mask_utf8_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes,
                                uint64_t* mask_bits_out, int64_t mask_cap_words, int64_t* cp_row_off_out,
                                int64_t* total_cps_out, int flags, void* stream) {
    LATOK_ENTER();
    int rc = need_init(g);
    if (rc) return rc;
    if (!total_cps_out) return fail(LATOK_ERR_INVALID, "total_cps_out is NULL");
    StreamTurn turn(g, stream);
    hipStream_t st = turn.st;
    const bool dev = (flags & LATOK_DEVICE_PTRS) != 0;
    if ((rc = resolve_total(byte_off, n_str, &total_bytes, dev, st))) return rc;
    const Batch b{Input{utf8, Form::Utf8}, byte_off, n_str, total_bytes};
    // large batches: byte space + compaction of the mask (no UTF-32 copy)
    if (n_str > 0 && total_bytes > kSmallChars && utf8 && cp_row_off_out && mask_bits_out && mask_cap_words >= 0 &&
        (!dev || ((uintptr_t)utf8 & 15) == 0)) {
        int fallback = 0;
        rc = mask_utf8_via_bytes(g, b, dev, mask_bits_out, mask_cap_words, cp_row_off_out, total_cps_out, st, &fallback);
        if (rc || !fallback) return rc;
    }
    int64_t total = 0;
    Batch bytes;
    if ((rc = decode_utf8_to_workspace(g, b, dev, st, &total, &bytes))) return rc;
    *total_cps_out = total;
    if (n_str == 0) return LATOK_OK;
    const int64_t words = (total + 63) / 64;
    if (words > mask_cap_words) return fail(LATOK_ERR_INVALID, "mask_cap_words too small: need %lld", (long long)words);
    if (!cp_row_off_out || (words > 0 && !mask_bits_out)) return fail(LATOK_ERR_INVALID, "NULL output buffer");
    Pipe a;
    // no multi-byte char: the byte-space kernel on the bytes, code-point offsets = byte offsets
    a.b = bytes.in.p ? bytes : Batch{Input{g.h_cps.p, Form::Utf32}, (const int64_t*)g.u_row.p, n_str, total};
    a.bits = mask_bits_out;
    a.st = st;
    if (!dev) {
        if ((rc = g.h_out.ensure((size_t)words * 8 + 8))) return rc;
        a.bits = (uint64_t*)g.h_out.p;
    }
    if ((rc = run_pipeline(g, g.ws, a))) return rc;
    const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (!dev && words > 0) HIP_TRY(hipMemcpyAsync(mask_bits_out, a.bits, (size_t)words * 8, kind, st));
    HIP_TRY(hipMemcpyAsync(cp_row_off_out, a.b.row, (size_t)(n_str + 1) * 8, kind, st));
    HIP_TRY(hipStreamSynchronize(st));
    return LATOK_OK;
}

int latok_split_offsets_utf8_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes,
                                   int64_t* counts_out, int64_t* offsets_out, int64_t offsets_cap,
                                   int64_t* n_offsets_out, int flags, void* stream) {
    LATOK_ENTER();
    return compact_common(g, false, false, Batch{Input{utf8, Form::Utf8}, byte_off, n_str, total_bytes}, true, counts_out, offsets_out,
                          nullptr, offsets_cap, n_offsets_out, flags, stream);
}

int latok_token_spans_utf8_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes,
                                 int64_t* counts_out, int64_t* spans_out, int64_t spans_cap, int64_t* n_tokens_out,
                                 int flags, void* stream) {
    LATOK_ENTER();
    return compact_common(g, true, false, Batch{Input{utf8, Form::Utf8}, byte_off, n_str, total_bytes}, true, counts_out, spans_out,
                          nullptr, spans_cap, n_tokens_out, flags, stream);
}

int latok_token_features_utf8_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes,
                                    int64_t* counts_out, int64_t* spans4_out, int8_t* features_out, int64_t cap,
                                    int64_t* n_tokens_out, int flags, void* stream) {
    LATOK_ENTER();
    if (!features_out && cap > 0) return fail(LATOK_ERR_INVALID, "features_out is NULL");
    return compact_common(g, true, true, Batch{Input{utf8, Form::Utf8}, byte_off, n_str, total_bytes}, true, counts_out, spans4_out,
                          features_out, cap, n_tokens_out, flags, stream);
}

/* byte-space UTF-8 entry points: the tile kernel reads the bytes (1 B/char for ASCII), all positions are byte offsets */
int latok_split_mask_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes,
                                      uint64_t* mask_bits_out, int flags, void* stream) {
    LATOK_ENTER();
    return mask_common(g, Input{utf8, Form::Utf8}, byte_off, n_str, total_bytes, mask_bits_out, latok::kModeBits, flags, stream);
}

int latok_split_offsets_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes,
                                         int64_t* counts_out, int64_t* offsets_out, int64_t offsets_cap,
                                         int64_t* n_offsets_out, int flags, void* stream) {
    LATOK_ENTER();
    return compact_common(g, false, false, Batch{Input{utf8, Form::Utf8}, byte_off, n_str, total_bytes}, false, counts_out, offsets_out,
                          nullptr, offsets_cap, n_offsets_out, flags, stream);
}

int latok_token_spans_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes,
                                       int64_t* counts_out, int64_t* spans_out, int64_t spans_cap, int64_t* n_tokens_out,
                                       int flags, void* stream) {
    LATOK_ENTER();
    return compact_common(g, true, false, Batch{Input{utf8, Form::Utf8}, byte_off, n_str, total_bytes}, false, counts_out, spans_out,
                          nullptr, spans_cap, n_tokens_out, flags, stream);
}

/* featurize in byte space: byte positions in the span records, feature sums per char (enqueue_utf8_bytes_features) */
int latok_token_features_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes,
                                          int64_t* counts_out, int64_t* spans4_out, int8_t* features_out, int64_t cap,
                                          int64_t* n_tokens_out, int flags, void* stream) {
    LATOK_ENTER();
    if (!features_out && cap > 0) return fail(LATOK_ERR_INVALID, "features_out is NULL");
    return compact_common(g, true, true, Batch{Input{utf8, Form::Utf8}, byte_off, n_str, total_bytes}, false, counts_out, spans4_out,
                          features_out, cap, n_tokens_out, flags, stream);
}

/* joined token text in byte space: every string's tokens joined by one separator byte (enqueue_join_tokens) */
int latok_join_tokens_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes, int sep,
                                       uint8_t* out_bytes, int64_t out_cap, int64_t* out_off, void* counts_out, int64_t* n_out_bytes,
                                       int flags, void* stream) {
    LATOK_ENTER();
    if (sep < 0 || sep > 255) return fail(LATOK_ERR_INVALID, "sep must be one byte (0..255), got %d", sep);
    int rc = need_init(g);
    if (rc) return rc;
    if (!n_out_bytes) return fail(LATOK_ERR_INVALID, "the total-size output pointer is NULL");
    *n_out_bytes = 0;
    if (out_cap < 0) return fail(LATOK_ERR_INVALID, "negative capacity");
    if (!out_bytes && out_cap > 0) return fail(LATOK_ERR_INVALID, "out_bytes is NULL but out_cap > 0 (a size query passes out_cap = 0)");
    if (flags & ~(LATOK_OUT_INT32 | LATOK_DEVICE_PTRS)) return fail(LATOK_ERR_INVALID, "unknown flag");
    BytesCall c;   // (elt: the width of the counts; out_off is int64 in every mode)
    if ((rc = c.open(g, utf8, byte_off, n_str, total_bytes, flags, stream))) return rc;
    const bool dev = c.dev;
    const hipStream_t st = c.st;
    if (n_str > 0 && !out_off) return fail(LATOK_ERR_INVALID, "out_off is NULL");
    if (c.empty) {   // no byte, no token: empty rows (device pointers: one wait, whatever was cleared)
        if ((rc = zero_counts(dev, out_off, (size_t)(n_str + 1) * 8, st)) || (rc = zero_counts(dev, counts_out, (size_t)n_str * c.elt, st))) return rc;
        if (dev) HIP_TRY(hipStreamSynchronize(st));
        return LATOK_OK;
    }
    if (dev && (((uintptr_t)out_off & 7) != 0 || ((uintptr_t)counts_out & (c.elt - 1)) != 0)) return fail(LATOK_ERR_INVALID, "misaligned output buffer");
    if ((rc = c.stage(g, 5, WsShape{.spans = true, .join = true}, kClearPair))) return rc;
    JoinTokens a;
    a.b = c.d;
    a.sep = sep;
    a.out = out_bytes;
    // (a kept token has at least one byte and brings at most one separator: a larger capacity gates nothing, and the staging is sized by it)
    a.cap = out_bytes ? std::min(out_cap, 2 * c.total) : 0;
    a.out_off = out_off;
    a.counts = counts_out;
    a.o32 = c.o32;
    if (!dev) {
        if ((rc = g.h_out.ensure((size_t)a.cap + 16)) || (rc = g.h_aux.ensure((size_t)(n_str + 1) * 8)) || (rc = g.counts.ensure((size_t)n_str * 8)))
            return rc;
        if (out_bytes) a.out = (uint8_t*)g.h_out.p;
        a.out_off = (int64_t*)g.h_aux.p;
        if (counts_out) a.counts = g.counts.p;
    }
    a.r_bytes = c.p_tot;
    a.r_err = c.p_tot + 1;
    a.st = st;
    if ((rc = enqueue_join_tokens(g, g.ws, a))) return rc;
    if (!dev) {   // row offsets and counts are valid whatever the capacity
        HIP_TRY(hipMemcpyAsync(out_off, a.out_off, (size_t)(n_str + 1) * 8, hipMemcpyDeviceToHost, st));
        if (counts_out) HIP_TRY(hipMemcpyAsync(counts_out, a.counts, (size_t)n_str * c.elt, hipMemcpyDeviceToHost, st));
    }
    int64_t n = 0;
    if ((rc = c.wait_totals(g, 1, &n))) return rc;
    *n_out_bytes = n;
    return deliver_sized(c, n, out_cap, "output capacity too small: need %lld bytes", {{out_bytes, a.out, 1}});
}

/* case folding and accent stripping in byte space: UTF-8 in, folded UTF-8 out (fold_kernels.hip; the map: fold_map.h).  One stream:
 *   k_fold_starts     the string-end bitmap over the bytes
 *   k_fold_counts     output bytes per 16-byte group (prefix inside its tile) and per tile
 *   k_scan_chained    tile ranks; THE byte total -> scalar word 0 and the pinned pair
 *   k_fold_write      the bytes (gate: total <= cap), out_off
 * The tables reach the device with the context's first fold call. */
static int ensure_fold_tables(Ctx& g, hipStream_t st) {
    if (g.fold_ready) return LATOK_OK;
    int rc;
    const size_t b1 = align16(sizeof(kFoldStage1)), b2 = align16(sizeof(kFoldStage2)), b3 = align16(sizeof(kFoldRec)), b4 = align16(sizeof(kFoldHigh));
    if ((rc = g.fold_tab.ensure(b1 + b2 + b3 + b4))) return rc;
    uint8_t* p = (uint8_t*)g.fold_tab.p;
    HIP_TRY(hipMemcpyAsync(p, kFoldStage1, sizeof(kFoldStage1), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(p + b1, kFoldStage2, sizeof(kFoldStage2), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(p + b1 + b2, kFoldRec, sizeof(kFoldRec), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(p + b1 + b2 + b3, kFoldHigh, sizeof(kFoldHigh), hipMemcpyHostToDevice, st));
    g.fold_t.stage1 = (const uint16_t*)p;
    g.fold_t.stage2 = (const uint16_t*)(p + b1);
    g.fold_t.rec = (const uint32_t*)(p + b1 + b2);
    g.fold_t.high = (const uint32_t*)(p + b1 + b2 + b3);
    g.fold_t.n_high = (int)kFoldHighN;
    g.fold_ready = true;
    return LATOK_OK;
}
int latok_fold_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes, int fold,
                                uint8_t* out_bytes, int64_t out_cap, int64_t* out_off, int64_t* n_out_bytes, int flags, void* stream) {
    LATOK_ENTER();
    if (fold & ~(LATOK_FOLD_LOWER | LATOK_FOLD_STRIP_MARKS | LATOK_FOLD_CLEAN | LATOK_FOLD_CJK_SPACE))
        return fail(LATOK_ERR_INVALID, "unknown fold bit in %d", fold);
    if (flags & ~LATOK_DEVICE_PTRS) return fail(LATOK_ERR_INVALID, "unknown flag");
    if (!n_out_bytes) return fail(LATOK_ERR_INVALID, "the total-size output pointer is NULL");
    *n_out_bytes = 0;
    if (out_cap < 0) return fail(LATOK_ERR_INVALID, "negative capacity");
    if (!out_bytes && out_cap > 0) return fail(LATOK_ERR_INVALID, "out_bytes is NULL but out_cap > 0 (a size query passes out_cap = 0)");
    if (n_str > 0 && !out_off) return fail(LATOK_ERR_INVALID, "out_off is NULL");
    int rc = need_init(g);
    if (rc) return rc;
    BytesCall c;
    if ((rc = c.open(g, utf8, byte_off, n_str, total_bytes, flags, stream))) return rc;
    const bool dev = c.dev;
    const hipStream_t st = c.st;
    if (c.empty) {   // no byte: empty rows (device pointers: one wait, whatever was cleared)
        if ((rc = zero_counts(dev, out_off, (size_t)(n_str + 1) * 8, st))) return rc;
        if (dev) HIP_TRY(hipStreamSynchronize(st));
        return LATOK_OK;
    }
    if (dev && ((uintptr_t)out_off & 7) != 0) return fail(LATOK_ERR_INVALID, "misaligned output buffer");
    if ((rc = c.stage(g, 13, WsShape{}, kClearPair))) return rc;
    const int64_t total = c.total;
    if ((rc = ensure_fold_tables(g, st)) || (rc = g.fold_start.ensure((size_t)latok::fold_start_words(total) * 4)) ||
        (rc = g.fold_pref.ensure((size_t)latok::fold_groups(total) * 2)))
        return rc;
    // (an image has at most three times the bytes of its sequence: a larger capacity gates nothing, and the staging is sized by it)
    const int64_t cap = out_bytes ? std::min(out_cap, 3 * total) : 0;
    uint8_t* d_out = out_bytes;
    int64_t* d_out_off = out_off;
    if (!dev) {
        if ((rc = g.h_out.ensure((size_t)cap + 16)) || (rc = g.h_aux.ensure((size_t)(n_str + 1) * 8))) return rc;
        if (out_bytes) d_out = (uint8_t*)g.h_out.p;
        d_out_off = (int64_t*)g.h_aux.p;
    }
    Workspace& w = g.ws;
    uint32_t* d_start = (uint32_t*)g.fold_start.p;
    uint16_t* d_pref = (uint16_t*)g.fold_pref.p;
    int64_t* d_tcnt = (int64_t*)w.wcnt.p;
    int64_t* d_rank = (int64_t*)w.bases.p;
    int64_t* d_total = (int64_t*)w.scalar.p;
    const uint8_t* d_u8 = (const uint8_t*)c.d.in.p;
    latok::ChainState chain;
    if ((rc = next_scan_epoch(w, st, &chain))) return rc;
    HIP_TRY(latok::launch_fold_starts(c.d.row, n_str, total, d_start, st));
    HIP_TRY(latok::launch_fold_counts(d_u8, total, d_start, fold, g.fold_t, d_pref, d_tcnt, st));
    HIP_TRY(latok::launch_tile_scan(d_tcnt, latok::fold_tiles(total), d_rank, chain, d_total, c.p_tot, (int*)(c.p_tot + 1) + 1, st));
    HIP_TRY(latok::launch_fold_write(d_u8, total, d_start, fold, g.fold_t, d_pref, d_rank, d_tcnt, c.d.row, n_str, d_out, cap, d_total, d_out_off, st));
    if (!dev) HIP_TRY(hipMemcpyAsync(out_off, d_out_off, (size_t)(n_str + 1) * 8, hipMemcpyDeviceToHost, st));   // valid whatever the capacity
    int64_t n = 0;
    if ((rc = c.wait_totals(g, 0, &n))) return rc;
    *n_out_bytes = n;
    return deliver_sized(c, n, out_cap, "output capacity too small: need %lld bytes", {{out_bytes, d_out, 1}});
}

/* token hashes and token ids in byte space: one MurmurHash3 x86_32 word per token, or its id in a vocabulary, rank-aligned with the
 * span records (enqueue_token_words).  The two blocking entry points' shared body: ids = the call takes a vocabulary. */
static int token_words_common(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes, bool ids, const latok_vocab* vocab,
                              uint32_t seed, int32_t unk_id, void* counts_out, void* spans_out, void* words_out, int64_t cap,
                              int64_t* n_tokens_out, int flags, void* stream) {
    LATOK_ENTER();
    if (flags & ~(LATOK_OUT_INT32 | LATOK_DEVICE_PTRS)) return fail(LATOK_ERR_INVALID, "unknown flag");
    int rc = need_init(g);
    if (rc) return rc;
    if (!n_tokens_out) return fail(LATOK_ERR_INVALID, "the total-size output pointer is NULL");
    *n_tokens_out = 0;
    if (cap < 0) return fail(LATOK_ERR_INVALID, "negative capacity");
    if (!words_out && cap > 0) return fail(LATOK_ERR_INVALID, "%s_out is NULL but cap > 0 (a size query passes cap = 0)", ids ? "ids" : "hashes");
    const Vocab* v = nullptr;
    if (ids && (rc = check_object(g, vocab, "vocab is NULL", &v))) return rc;
    BytesCall c;   // (elt: the width of a count and of one field of a record; a hash or an id is 4 bytes in every mode)
    if ((rc = c.open(g, utf8, byte_off, n_str, total_bytes, flags, stream))) return rc;
    const bool dev = c.dev;
    const size_t elt = c.elt;
    if (c.empty) return zero_counts(dev, counts_out, (size_t)n_str * elt, c.st, true);   // no byte, no token
    if (dev && (((uintptr_t)spans_out & (2 * elt - 1)) != 0 || ((uintptr_t)counts_out & (elt - 1)) != 0 || ((uintptr_t)words_out & 3) != 0))
        return fail(LATOK_ERR_INVALID, "misaligned output buffer");
    if ((rc = c.stage(g, ids ? 7 : 6, WsShape{.spans = true}, kClearPair))) return rc;
    TokenWords a;
    a.b = c.d;
    a.vocab = v;
    a.seed = seed;
    a.unk = unk_id;
    a.counts = counts_out;
    a.spans = spans_out;
    a.words = words_out;
    a.cap = words_out ? std::min(cap, c.total) : 0;   // (a token has at least one byte: a larger capacity gates nothing, and the staging is sized by it)
    a.o32 = c.o32;
    if (!dev) {
        if ((rc = g.h_aux.ensure((size_t)a.cap * 4 + 16)) || (rc = g.h_out.ensure((size_t)a.cap * 2 * elt + 16)) || (rc = g.counts.ensure((size_t)n_str * 8)))
            return rc;
        if (words_out) a.words = g.h_aux.p;
        if (spans_out) a.spans = g.h_out.p;
        if (counts_out) a.counts = g.counts.p;
    }
    a.r_tokens = c.p_tot;
    a.r_err = c.p_tot + 1;
    a.st = c.st;
    if ((rc = enqueue_token_words(g, g.ws, a))) return rc;
    if (!dev && counts_out) HIP_TRY(hipMemcpyAsync(counts_out, a.counts, (size_t)n_str * elt, hipMemcpyDeviceToHost, c.st));   // valid whatever the capacity
    int64_t n = 0;
    if ((rc = c.wait_totals(g, 1, &n))) return rc;   // the call's one wait for the kernels
    *n_tokens_out = n;
    return deliver_sized(c, n, cap, "capacity too small: need %lld tokens", {{words_out, a.words, 4}, {spans_out, a.spans, 2 * elt}});
}
int latok_token_hashes_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes, uint32_t seed,
                                        int64_t* counts_out, int64_t* spans_out, uint32_t* hashes_out, int64_t cap, int64_t* n_tokens_out,
                                        int flags, void* stream) {
    return token_words_common(utf8, byte_off, n_str, total_bytes, false, nullptr, seed, -1, counts_out, spans_out, hashes_out, cap, n_tokens_out, flags,
                              stream);
}

/* Pre-tokens in byte space (latok_pretokens_utf8_bytes_batch): the span call of a pre-tokenizer.  LATOK_PRETOK_LATOK is
 * latok_token_spans_utf8_bytes_batch itself.  LATOK_PRETOK_GPT2, one stream, every batch size the same kernels:
 *   enqueue_token_front (GPT2)     k_pretok_planes: start plane, zero SPACE plane, tile index; k_word_counts + k_scan_chained: ranks, THE total
 *   k_counts_scatter (kind 1)      per-string counts and the [start, end) records (gate: total <= capacity)
 * One wait; host pointers: the copies and a second wait.  Route 26 of latok_debug_last_route.
 * LATOK_PRETOK_CL100K: the same call with the cl100k front (two launches in place of k_pretok_planes), route 29.
 * LATOK_PRETOK_SPM: the same call with SentencePiece's segments (k_pretok_spm_planes in place of k_pretok_planes), route 32. */
static int pretokens_planes(int pretok, const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes, void* counts_out, void* spans_out,
                            int64_t spans_cap, int64_t* n_tokens_out, int flags, void* stream) {
    LATOK_ENTER();
    int rc = need_init(g);
    if (rc) return rc;
    if (!n_tokens_out) return fail(LATOK_ERR_INVALID, "the total-count output pointer is NULL");
    *n_tokens_out = 0;
    if (spans_cap < 0) return fail(LATOK_ERR_INVALID, "negative capacity");
    const bool o32 = (flags & LATOK_OUT_INT32) != 0;
    if (o32 && !(flags & LATOK_DEVICE_PTRS) && byte_off && n_str > 0) {   // before anything is staged (device-resident offsets: the kernel checks)
        for (int64_t s = 0; s < n_str; ++s)
            if (byte_off[s + 1] - byte_off[s] > 0x7FFFFFFFll)
                return fail(LATOK_ERR_INVALID, "string %lld is too long for LATOK_OUT_INT32; use the 64-bit form", (long long)s);
    }
    BytesCall c;
    if ((rc = c.open(g, utf8, byte_off, n_str, total_bytes, flags, stream))) return rc;
    const bool dev = c.dev;
    const size_t elt = c.elt;
    if (n_str == 0) return LATOK_OK;
    if (!counts_out) return fail(LATOK_ERR_INVALID, "counts_out is NULL");
    if (c.empty) return zero_counts(dev, counts_out, (size_t)n_str * elt, c.st, true);   // only empty strings
    if (dev && (((uintptr_t)spans_out & (2 * elt - 1)) != 0 || ((uintptr_t)counts_out & (elt - 1)) != 0)) return fail(LATOK_ERR_INVALID, "misaligned output buffer");
    if ((rc = c.stage(g, pretok == kPretokCl100k ? 29 : pretok == kPretokSpm ? 32 : 26, WsShape{.spans = true}, kClearPair))) return rc;
    void* d_counts = counts_out;
    void* d_spans = spans_out;
    int64_t cap = spans_out ? spans_cap : 0;
    if (!dev) {   // device staging sized for the worst case of one pre-token per byte
        if ((rc = g.counts.ensure((size_t)n_str * 8)) || (rc = g.h_out.ensure((size_t)c.total * 2 * elt))) return rc;
        d_counts = g.counts.p;
        d_spans = g.h_out.p;
        cap = c.total;
    }
    int* d_err = (int*)(c.p_tot + 1);
    latok::TokenPlanes t;
    if ((rc = enqueue_token_front(g, g.ws, c.d, c.p_tot, d_err, c.st, &t, pretok))) return rc;
    HIP_TRY(latok::launch_counts_scatter(1, o32, t, d_spans, cap, d_counts, d_err, c.st));
    HIP_TRY(hipStreamSynchronize(c.st));
    int64_t n = *n_tokens_out = c.h_tot[0];   // (the total is reported whatever the flags say)
    if ((rc = finish_totals(g.ws, c.h_tot, 0xFFFFFFFFll, &n))) return rc;
    return deliver_records(false, dev ? nullptr : g.counts.p, g.h_out.p, nullptr, counts_out, spans_out, nullptr, n_str, elt, 2 * elt, n, spans_cap, c.st);
}
int latok_pretokens_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes, int pretok, int64_t* counts_out,
                                     int64_t* spans_out, int64_t spans_cap, int64_t* n_tokens_out, int flags, void* stream) {
    // what needs no device is refused first
    if (pretok != LATOK_PRETOK_LATOK && pretok != LATOK_PRETOK_GPT2 && pretok != LATOK_PRETOK_CL100K && pretok != LATOK_PRETOK_SPM)
        return fail(LATOK_ERR_INVALID, "unknown pretok %d (LATOK_PRETOK_LATOK, LATOK_PRETOK_GPT2, LATOK_PRETOK_CL100K or LATOK_PRETOK_SPM)", pretok);
    if (flags & ~(LATOK_OUT_INT32 | LATOK_DEVICE_PTRS)) return fail(LATOK_ERR_INVALID, "unknown flag");
    if (pretok == LATOK_PRETOK_LATOK)
        return latok_token_spans_utf8_bytes_batch(utf8, byte_off, n_str, total_bytes, counts_out, spans_out, spans_cap, n_tokens_out, flags, stream);
    return pretokens_planes(pretok, utf8, byte_off, n_str, total_bytes, counts_out, spans_out, spans_cap, n_tokens_out, flags, stream);
}

/* vocabularies: built on the host (vocab_table.h), uploaded once, read only afterwards */
static int flow_drain(Ctx& g);   // batch flow (below): its three streams
// The end of a shared object (latok_vocab, latok_wordpiece, latok_bpe, latok_idf, latok_counter; `mu`: the lock of a mutable one).  The current
// context's own work on it is waited for first: its stream and its flow; whatever they report, the object is freed.
extern "C++" template <class Obj>
static int destroy_object(Ctx& g, Obj* obj, std::mutex Obj::*mu = nullptr) {
    if (!obj) return LATOK_OK;
    int rc = LATOK_OK;
    if (g.inited) {
        const hipError_t e = hipStreamSynchronize(g.stream);
        rc = flow_drain(g);
        if (e != hipSuccess) rc = fail(LATOK_ERR_HIP, "hipStreamSynchronize failed: %s", hipGetErrorString(e));
    }
    if (mu) { std::lock_guard<std::mutex> ol(obj->*mu); }   // (a call of another context that still holds it has returned)
    delete obj;
    return rc;
}

int latok_vocab_create(const uint8_t* words, const int64_t* word_off, int64_t n_words, const int32_t* word_ids, uint32_t seed,
                       latok_vocab** vocab_out) {
    LATOK_ENTER();
    // what needs no device is refused first
    if (!vocab_out) return fail(LATOK_ERR_INVALID, "vocab_out is NULL");
    *vocab_out = nullptr;
    int rc = check_word_list(words, word_off, n_words);
    if (rc || (rc = need_init(g))) return rc;
    VtTable t;
    Vocab* v = nullptr;
    try {
        vt_build(words, word_off, n_words, word_ids, seed, &t);
        v = new Vocab();
    } catch (const std::bad_alloc&) {
        return fail(LATOK_ERR_NOMEM, "out of host memory");
    }
    v->device = g.device;
    v->n_words = n_words;
    v->seed = seed;
    rc = v->table.upload(t, g.stream);
    const hipError_t e = hipStreamSynchronize(g.stream);   // (the host table dies with this call, and every context may use the object at once)
    if (!rc && e != hipSuccess) rc = fail(LATOK_ERR_HIP, "uploading the vocabulary failed: %s", hipGetErrorString(e));
    if (rc) {
        delete v;
        return rc;
    }
    *vocab_out = reinterpret_cast<latok_vocab*>(v);
    return LATOK_OK;
}

int latok_vocab_destroy(latok_vocab* vocab) {
    LATOK_ENTER();
    return destroy_object(g, reinterpret_cast<Vocab*>(vocab));
}

int latok_vocab_info(const latok_vocab* vocab, int64_t* n_words, int64_t* n_slots, uint32_t* seed, int* device) {
    const Vocab* v = reinterpret_cast<const Vocab*>(vocab);
    if (!v) return fail(LATOK_ERR_INVALID, "vocab is NULL");
    if (n_words) *n_words = v->n_words;
    if (n_slots) *n_slots = (int64_t)v->table.n_slots;
    if (seed) *seed = v->seed;
    if (device) *device = v->device;
    return LATOK_OK;
}

/* token ids in byte space: the id of every token in a vocabulary, rank-aligned with the span records (token_words_common) */
int latok_token_ids_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes, const latok_vocab* vocab,
                                     int32_t unk_id, int64_t* counts_out, int64_t* spans_out, int32_t* ids_out, int64_t cap,
                                     int64_t* n_tokens_out, int flags, void* stream) {
    return token_words_common(utf8, byte_off, n_str, total_bytes, true, vocab, 0, unk_id, counts_out, spans_out, ids_out, cap, n_tokens_out, flags, stream);
}

/* TF-IDF (latok_idf_*, latok_tfidf_*; tfidf_kernels.hip, tfidf_weight.h).  The object: df and n_docs, and per smoothing mode the float32
 * idf vector, computed by the first call that asks (k_idf_weights) and dropped by every update, load and clear.  A consumer on another
 * stream than the one that computed the vector waits for its event on the device. */
struct Idf {                       // latok_idf: mutable; calls on it are serialised by its own lock
    std::mutex mu;
    int device = -1;
    int64_t n_cols = 0;            // (never changes)
    int64_t n_docs = 0;
    DevMem df;                     // int32[n_cols]
    DevMem idf[2];                 // [smooth]: float[n_cols], allocated on first use
    bool idf_valid[2] = {false, false};
    hipEvent_t idf_ready[2] = {nullptr, nullptr};
    ~Idf() {
        for (hipEvent_t e : idf_ready)
            if (e) (void)hipEventDestroy(e);
    }
};
static void idf_drop_weights(Idf& f) { f.idf_valid[0] = f.idf_valid[1] = false; }
// the idf vector of one smoothing mode, valid on `st` (caller holds f.mu)
static int idf_weights_on(Idf& f, bool smooth, hipStream_t st, const float** out) {
    const int m = smooth ? 1 : 0;
    if (!f.idf[m].p) {
        const hipError_t e = f.idf[m].alloc((size_t)f.n_cols * 4);
        if (e != hipSuccess) return fail(LATOK_ERR_NOMEM, "hipMalloc of %lld idf weights failed: %s", (long long)f.n_cols, hipGetErrorString(e));
    }
    if (!f.idf_ready[m]) HIP_TRY(hipEventCreateWithFlags(&f.idf_ready[m], hipEventDisableTiming));
    if (!f.idf_valid[m]) {
        HIP_TRY(latok::launch_idf_weights(f.df.as<int32_t>(), f.n_cols, f.n_docs, smooth, f.idf[m].as<float>(), st));
        HIP_TRY(hipEventRecord(f.idf_ready[m], st));
        f.idf_valid[m] = true;
    } else {
        HIP_TRY(hipStreamWaitEvent(st, f.idf_ready[m], 0));
    }
    *out = f.idf[m].as<float>();
    return LATOK_OK;
}
static int tfidf_check_opts(int opts) {
    if (opts & ~kTwAllOpts) return fail(LATOK_ERR_INVALID, "unknown opts bit");
    if ((opts & kTwNormL1) && (opts & kTwNormL2)) return fail(LATOK_ERR_INVALID, "LATOK_TFIDF_NORM_L1 and LATOK_TFIDF_NORM_L2 exclude each other");
    return LATOK_OK;
}
static int csr_refusal(int err) {
    if (err & latok::kCsrBadStart) return fail(LATOK_ERR_INVALID, "indptr[0] must be 0");
    if (err & latok::kCsrBadOrder) return fail(LATOK_ERR_INVALID, "indptr must be non-decreasing");
    if (err & latok::kCsrBadTotal) return fail(LATOK_ERR_INVALID, "indptr[n_rows] does not match nnz");
    if (err & latok::kCsrBadColumn) return fail(LATOK_ERR_INVALID, "a column index lies outside [0, n_cols) of the idf");
    return LATOK_OK;
}
static int g_df_add_cached = 1;   // latok_debug_set_df_add: 0 = the plain k_df_add_plain (tools/path_bench.py measures both)

/* The term family: per-string counts of a UTF-8 batch in BYTE space, the CSR rows of a document-term matrix, with one key per token
 * (latok_term_counts_*, latok_hashed_term_counts_*), per word n-gram (latok_ngram_counts_*, latok_hashed_ngram_counts_*) or per character
 * n-gram inside a token (latok_chargram_counts_*, latok_hashed_chargram_counts_*), and the TF-IDF calls over text behind them.  One core,
 * enqueue_term_keys, which lists what each kind launches. */
enum class TermKind { Tokens, WordGrams, CharGrams };   // one key per token / per word n-gram / per character n-gram inside a token
struct TermsCall {                 // one blocking call of the term family: what its entry point received ...
    const uint8_t* utf8;
    const int64_t* byte_off;
    int64_t n_str, total_bytes;
    const latok_vocab* vocab = nullptr;   // the vocabulary form, or the hashed one with its parameters
    bool hashed = false;
    uint32_t seed = 0;
    int64_t n_features = 0;
    int alternate_sign = 0;
    TermKind kind = TermKind::Tokens;   // what a key stands for; the two gram kinds: the orders, pinned word 5 = the key total K
    int min_n = 1, max_n = 1;
    int sep = 0x20, pad = 0x20;    // the byte between the tokens of a word gram / around the word of a character gram
    bool tfidf = false, update = false;   // the TF-IDF tail behind the counts: the weighting of the rows, or (update) the update of idf
    Idf* idf = nullptr;            // may be NULL (weighting without idf)
    int opts = 0;
    void *indptr_out = nullptr, *oov_out = nullptr;
    int32_t *indices_out = nullptr, *data_out = nullptr;   // (data: float32 in the TF-IDF calls, weighted in place)
    int64_t cap = 0;               // in entries
    int64_t *nnz_out = nullptr, *n_tokens_out = nullptr, *n_grams_out = nullptr;
    int flags = 0;
    void* stream = nullptr;
    // ... and what terms_stage_outputs made of it for the enqueue cores
    Batch b;                       // UTF-8 bytes on the device (16-byte aligned), byte offsets, total in bytes (> 0), n_str > 0
    const Vocab* v = nullptr;      // NULL: the hashed form
    void *indptr = nullptr, *oov = nullptr;        // [n_str + 1], [n_str] or NULL: the caller's device buffers or the context's own
    int32_t *indices = nullptr, *data = nullptr;   // NULL (both): a size query
    int64_t fill_cap = 0;          // in entries: what the kernels may write
    bool o32 = false;              // width of indptr and oov
    int64_t* p_tot = nullptr;      // the pinned words as the device sees them (cleared by stage): 0 tokens, 1 flags, 3 nnz
    volatile int64_t* h_tot = nullptr;
    int64_t n_tokens = 0, n_grams = 0;   // (out) the token total; the key total K of the n-gram route
    hipStream_t st = nullptr;
};
// the five arrays of w.trows (kTermRowArrays), n_str + 1 int64 each
struct TermRows {
    int64_t *cnt, *start, *distinct, *indptr, *oov;   // token counts and row starts in token space, distinct counts, indptr, OOV counts
    size_t bytes;
    TermRows(const Workspace& w, int64_t n_str)
        : cnt((int64_t*)w.trows.p), start(cnt + (n_str + 1)), distinct(cnt + 2 * (n_str + 1)), indptr(cnt + 3 * (n_str + 1)),
          oov(cnt + 4 * (n_str + 1)), bytes((size_t)(n_str + 1) * 8 * kTermRowArrays) {}
};
constexpr const char* kTooManyTermTokens = "the batch has %lld tokens: term counts are int32 (fewer than 2^31 tokens a call)";
// The CSR tail of the term and n-gram counts: the `n_keys` keys of w.tkeys, whose rows start at d_starts (token space or key space),
// are sorted and reduced inside every string, the distinct counts scanned into indptr (nnz -> scalar word 5, pinned word 3) and, when
// the caller gave buffers, the entries emitted.  launch_terms_finish follows at the call site, keys or none.
static int enqueue_csr_tail(Workspace& w, const TermsCall& a, const TermRows& r, const int64_t* d_starts, int64_t n_keys) {
    int rc;
    const int64_t n_str = a.b.n_str;
    uint64_t* d_keys = (uint64_t*)w.tkeys.p;
    int64_t* d_nnz = (int64_t*)w.scalar.p + 5;
    HIP_TRY(latok::launch_terms_reduce(d_keys, (uint64_t*)w.tkeys2.p, d_starts, n_str, n_keys, a.v != nullptr, r.distinct, r.oov, a.st));
    if ((rc = enqueue_row_scan(w, r.distinct, n_str + 1, r.indptr, d_nnz, a.p_tot + 3, (int*)(a.p_tot + 1) + 1, a.st))) return rc;
    if (a.indices) HIP_TRY(latok::launch_terms_emit(d_keys, d_starts, n_str, n_keys, r.distinct, r.indptr, d_nnz, a.fill_cap, a.indices, a.data, a.st));
    return LATOK_OK;
}
// the key form of a call: the vocabulary's table and seed, or the hashed form's parameters
static latok::TermKeyForm term_key_form(const TermsCall& a) {
    latok::TermKeyForm f;
    f.vocab = a.v != nullptr;
    if (a.v) f.vt = a.v->table.view(a.v->seed);
    f.seed = a.v ? a.v->seed : a.seed;
    f.n_features = a.v ? 0u : (uint32_t)a.n_features;
    f.alternate_sign = a.alternate_sign != 0;
    return f;
}
/* The core of the term family.  One stream, every batch size the same kernels: the head (wait 1: the token total, pinned word 0, sizes
 * the per-token buffers), the keys of the call's kind with their row starts, then the term counts' own sort and reduce inside every
 * string (enqueue_csr_tail) and the rows in the caller's width (k_terms_finish, keys or none).  The two gram kinds work in token space
 * and wait a second time (second_sized_total), for the key total K that sizes the two key buffers; their rows then lie in KEY space.
 * `w` was sized by ws_needs with WsShape{.spans = true, .term_rows = n_str + 1} and, for the gram kinds, .ng_rows = n_str + 1; the call
 * sizes the rest.  The gram kinds use the buffers the WordPiece calls keep: span records, per-token count and rank. */
static int enqueue_term_keys(Ctx& g, Workspace& w, TermsCall& a) {
    int rc;
    const hipStream_t st = a.st;
    const int64_t total = a.b.total, n_str = a.b.n_str;
    const bool words = a.kind == TermKind::WordGrams, chars = a.kind == TermKind::CharGrams;
    int* d_err = (int*)(a.p_tot + 1);
    latok::TokenPlanes t;
    if ((rc = sized_token_front(g, w, a.b, a.p_tot, a.h_tot, st, kTooManyTermTokens, &t, &a.n_tokens))) return rc;
    const int64_t n_tok = a.n_tokens;
    WsShape shape{.spans = true, .term_rows = n_str + 1};
    (chars ? shape.wp_tokens : words ? shape.ng_tokens : shape.term_tokens) = n_tok;
    if (chars || words) shape.ng_rows = n_str + 1;
    if (n_tok > 0 && (rc = ws_ensure(ws_needs(w, total, shape).data(), kWsNeeds))) return rc;
    const TermRows r(w, n_str);                       // token space: counts, row starts
    HIP_TRY(hipMemsetAsync(r.cnt, 0, r.bytes, st));   // (no key: every row is empty, nnz = 0)
    const latok::TermKeyForm form = term_key_form(a);
    const int64_t* d_starts = r.start;                // the rows of the keys: token space, or key space for the gram kinds
    int64_t n_keys = n_tok;
    if (n_tok > 0 && a.kind == TermKind::Tokens) {
        /*   sized_token_front (wait 1)                    kept mask, token ranks; the host reads THE token total (pinned word 0): the key buffers are sized
         *   k_term_scatter                                one term key per token at its rank (term_key.h), int64 token count per string
         *   k_scan_chained                                the row starts in token space
         *   enqueue_csr_tail: k_terms_tile, k_terms_long  sort and reduce inside every string: distinct and OOV counts, the entries
         *     k_scan_chained, k_terms_emit                indptr, nnz -> pinned word 3; indices / data if nnz fits the capacity
         *   k_terms_finish                                indptr / oov in the caller's width
         *   (wait 2)                                      nnz; host pointers then copy nnz entries (wait 3) */
        HIP_TRY(latok::launch_term_scatter(t, (const uint8_t*)a.b.in.p, form, (uint64_t*)w.tkeys.p, r.cnt, d_err, st));
        if ((rc = enqueue_row_scan(w, r.cnt, n_str + 1, r.start, (int64_t*)w.scalar.p + 4, nullptr, d_err + 1, st))) return rc;
    } else if (n_tok > 0) {
        latok::TokenText text;
        if ((rc = enqueue_token_rows(w, a.b, t, n_tok, r.cnt, r.start, d_err, st, &text))) return rc;
        int64_t* d_kcnt = (int64_t*)w.ngrows.p;       // key space: counts per row (word grams only), row starts
        int64_t* d_kstart = d_kcnt + (n_str + 1);
        int64_t* d_gcnt = (int64_t*)w.wpcnt.p;        // per token (character grams only): grams, key rank (n_tok + 1 entries)
        int64_t* d_grank = (int64_t*)w.wprank.p;
        int64_t* d_ktotal = (int64_t*)w.scalar.p + 6;
        const int max_n = std::min(a.max_n, kNgMax);  // (terms_refusals has refused more; the kernels' walks rest on it)
        if (words) {
            /*   sized_token_front (wait 1)                    kept mask, token ranks; the host reads THE token total (pinned word 0): the span records are sized
             *   enqueue_token_rows                            the span record of every token at its rank in the workspace, the row starts in token space
             *   k_ngram_rows + k_scan_chained                 grams per string, the row starts in key space; the key total K -> pinned word 5
             *   (wait 2)                                      the host reads K: 2^31 or more is refused, the two key buffers are sized
             *   k_ngram_keys                                  one term key per gram inside its row's range of keys
             *   enqueue_csr_tail, k_terms_finish              as the token kind, with the key rows and K in the place of the token rows
             *   (wait 3)                                      nnz; host pointers then copy nnz entries (wait 4) */
            HIP_TRY(latok::launch_ngram_rows(r.cnt, n_str, a.min_n, max_n, d_kcnt, st));
            if ((rc = enqueue_row_scan(w, d_kcnt, n_str + 1, d_kstart, d_ktotal, a.p_tot + 5, d_err + 1, st))) return rc;
        } else {
            /*   sized_token_front (wait 1)                    kept mask, token ranks; the host reads THE token total (pinned word 0): the per-token buffers are sized
             *   enqueue_token_rows                            the span record of every token at its rank in the workspace, the row starts in token space
             *   k_cgram_count + k_scan_chained                grams per token (chargram_text.h), each token's key rank; the key total K -> pinned word 5
             *   k_wp_rows                                     the row starts in key space: the key rank of every string's first token
             *   (wait 2)                                      the host reads K: 2^31 or more is refused, the two key buffers are sized
             *   k_cgram_keys                                  one term key per gram inside its token's range of keys
             *   enqueue_csr_tail, k_terms_finish              as the token kind, with the key rows and K in the place of the token rows
             *   (wait 3)                                      nnz; host pointers then copy nnz entries (wait 4) */
            HIP_TRY(latok::launch_cgram_count(text, a.min_n, max_n, d_gcnt, st));
            if ((rc = enqueue_row_scan(w, d_gcnt, n_tok + 1, d_grank, d_ktotal, a.p_tot + 5, d_err + 1, st))) return rc;
            HIP_TRY(latok::launch_wp_rows(false, r.start, d_grank, n_str, n_tok, d_kstart, st));
        }
        const char* too_many = words ? "the batch has %lld n-grams: term counts are int32 (fewer than 2^31 grams a call)"
                                     : "the batch has %lld character n-grams: term counts are int32 (fewer than 2^31 grams a call)";
        if ((rc = second_sized_total(w, a.h_tot, 5, st, too_many, &a.n_grams))) return rc;   // wait 2
        n_keys = a.n_grams;
        d_starts = d_kstart;
        if (n_keys > 0) {
            shape.ng_keys = n_keys;
            if ((rc = ws_ensure(ws_needs(w, total, shape).data(), kWsNeeds))) return rc;   // (only the key buffers grow)
            const latok::GramKeys keys{text, words ? d_kstart : d_grank, n_keys, a.min_n, max_n, (uint32_t)(words ? a.sep : a.pad) & 0xFFu,
                                       form, (uint64_t*)w.tkeys.p};
            HIP_TRY(words ? latok::launch_ngram_keys(keys, st) : latok::launch_cgram_keys(keys, st));
        }
    }
    if (n_keys > 0 && (rc = enqueue_csr_tail(w, a, r, d_starts, n_keys))) return rc;
    HIP_TRY(latok::launch_terms_finish(a.o32, r.indptr, r.oov, n_str, a.indptr, a.oov, st));
    return LATOK_OK;
}

// The argument refusals, none of which touches the device: first those that write nothing, then, behind need_init and with the
// out-pointers zeroed, the checks of the ids call and the capacity protocol in entries.
static int terms_refusals(const Ctx& g, TermsCall& a) {
    int rc;
    if (a.flags & ~(LATOK_OUT_INT32 | LATOK_DEVICE_PTRS)) return fail(LATOK_ERR_INVALID, "unknown flag");
    if (a.tfidf) {
        if (a.update && (a.flags & LATOK_OUT_INT32)) return fail(LATOK_ERR_INVALID, "unknown flag");
        if ((rc = tfidf_check_opts(a.opts))) return rc;
        if (a.update && !a.idf) return fail(LATOK_ERR_INVALID, "idf is NULL");
        if (a.idf && a.hashed && a.n_features != a.idf->n_cols)
            return fail(LATOK_ERR_INVALID, "n_features is %lld, the idf has %lld columns", (long long)a.n_features, (long long)a.idf->n_cols);
    }
    if (a.kind != TermKind::Tokens) {
        if (a.min_n < 1) return fail(LATOK_ERR_INVALID, "min_n must be at least 1");
        if (a.max_n < a.min_n) return fail(LATOK_ERR_INVALID, "max_n must not be below min_n");
        if (a.max_n > kNgMax) return fail(LATOK_ERR_INVALID, "max_n must not exceed %d", kNgMax);
        if (a.kind == TermKind::WordGrams && (a.sep < 0 || a.sep > 255)) return fail(LATOK_ERR_INVALID, "sep must be one byte: 0 .. 255");
        if (a.kind == TermKind::CharGrams && (a.pad < 0 || a.pad > 255)) return fail(LATOK_ERR_INVALID, "pad must be one byte: 0 .. 255");
    }
    if ((rc = need_init(g))) return rc;
    if (!a.nnz_out) return fail(LATOK_ERR_INVALID, "the total-size output pointer is NULL");
    *a.nnz_out = 0;
    if (a.n_tokens_out) *a.n_tokens_out = 0;
    if (a.n_grams_out) *a.n_grams_out = 0;
    if (!a.indptr_out && !a.update) return fail(LATOK_ERR_INVALID, "indptr_out is NULL");
    if (a.cap < 0) return fail(LATOK_ERR_INVALID, "negative capacity");
    if ((a.indices_out == nullptr) != (a.data_out == nullptr)) return fail(LATOK_ERR_INVALID, "indices_out and data_out go together: one of them is NULL");
    if (!a.indices_out && a.cap > 0) return fail(LATOK_ERR_INVALID, "indices_out and data_out are NULL but cap > 0 (a size query passes cap = 0)");
    if (a.hashed && (a.n_features < 1 || a.n_features > 0x7FFFFFFFll)) return fail(LATOK_ERR_INVALID, "n_features must be in 1 .. 2^31 - 1");
    if (!a.hashed) return check_object(g, a.vocab, "vocab is NULL", &a.v);
    return LATOK_OK;
}
// the enqueue cores' part of a staged call
static int terms_stage_outputs(Ctx& g, TermsCall& a, const BytesCall& c) {
    int rc;
    const int64_t n_str = c.d.n_str;
    a.b = c.d;
    // (an entry has at least one token, a token one byte: the staging is sized by it; a token starts one gram of every order at most;
    // a token of b >= 1 bytes has at most b + 2 <= 3 b padded characters, each of which starts one character gram of every order at most)
    const int64_t most = c.total * (a.kind == TermKind::Tokens ? 1 : a.max_n - a.min_n + 1) * (a.kind == TermKind::CharGrams ? 3 : 1);
    a.fill_cap = a.update ? most : a.indices_out ? std::min(a.cap, most) : 0;
    a.o32 = c.o32;
    const bool own = !c.dev || a.update;   // a host call's outputs, and every update's, land in the context's own buffers
    if (own && ((rc = g.h_aux.ensure((size_t)a.fill_cap * 4 + 16)) || (rc = g.h_out.ensure((size_t)a.fill_cap * 4 + 16)) ||
                (rc = g.counts.ensure((size_t)(2 * n_str + 2) * 8))))
        return rc;
    const bool own_entries = own && (a.indices_out || a.update);
    a.indptr = own ? g.counts.p : a.indptr_out;
    a.oov = own && a.oov_out ? (uint8_t*)g.counts.p + (size_t)(n_str + 1) * 8 : a.oov_out;
    a.indices = own_entries ? (int32_t*)g.h_aux.p : a.indices_out;
    a.data = own_entries ? (int32_t*)g.h_out.p : a.data_out;
    a.p_tot = c.p_tot;
    a.h_tot = c.h_tot;
    a.st = c.st;
    return LATOK_OK;
}
// The TF-IDF entry points' tail, behind the entries that launch_terms_emit wrote: the column check (vocabulary form with an idf), then
// the update of df from the context's own buffers (update) or the weighting of data in place; the error word travels to pinned word 7
// on the stream and is read behind the counts' own wait.  The caller holds the idf's lock.
static int enqueue_tfidf_tail(Ctx& g, const TermsCall& a) {
    int rc;
    Idf* const f = a.idf;
    const int64_t n_str = a.b.n_str;
    const int64_t* d_nnz = (const int64_t*)g.ws.scalar.p + 5;   // the scan's own rows and total, as the enqueue left them
    int* d_err = (int*)g.ws.tfctl.p;
    HIP_TRY(hipMemsetAsync(d_err, 0, 4, a.st));
    if (f && !a.hashed) HIP_TRY(latok::launch_csr_check(false, nullptr, a.indices, n_str, 0, d_nnz, a.fill_cap, f->n_cols, d_err, a.st));
    if (a.update) {
        HIP_TRY(latok::launch_df_add(g_df_add_cached != 0, a.indices, 0, d_nnz, a.fill_cap, d_err, f->df.as<int32_t>(), a.st));
    } else {
        const float* weights = nullptr;
        if (f && (rc = idf_weights_on(*f, (a.opts & kTwSmoothIdf) != 0, a.st, &weights))) return rc;
        HIP_TRY(latok::launch_tfidf_rows(false, TermRows(g.ws, n_str).indptr, a.indices, a.data, n_str, 0, d_nnz, a.fill_cap, weights, a.opts, d_err,
                                         (float*)a.data, a.st));
    }
    HIP_TRY(hipMemcpyAsync((void*)(a.h_tot + 7), d_err, 4, hipMemcpyDeviceToHost, a.st));
    return LATOK_OK;
}
// indptr and oov of a host call (valid whatever the capacity), wait 2, the totals, the tail's refusal, then the update's documents or the entries
static int terms_deliver(Ctx& g, const TermsCall& a, BytesCall& c) {
    int rc;
    const int64_t n_str = a.b.n_str;
    if (!c.dev && !a.update) {
        HIP_TRY(hipMemcpyAsync(a.indptr_out, a.indptr, (size_t)(n_str + 1) * c.elt, hipMemcpyDeviceToHost, c.st));
        if (a.oov_out) HIP_TRY(hipMemcpyAsync(a.oov_out, a.oov, (size_t)n_str * c.elt, hipMemcpyDeviceToHost, c.st));
    }
    int64_t n_tok = 0;
    if ((rc = c.wait_totals(g, 0, &n_tok))) return rc;   // wait 2
    if (a.n_tokens_out) *a.n_tokens_out = n_tok;
    if (a.n_grams_out) *a.n_grams_out = a.n_grams;
    const int64_t nnz = c.h_tot[3];
    *a.nnz_out = nnz;
    if (a.tfidf && c.h_tot[7]) return csr_refusal((int)c.h_tot[7]);
    if (!a.update) return deliver_sized(c, nnz, a.cap, "capacity too small: need %lld entries", {{a.indices_out, a.indices, 4}, {a.data_out, a.data, 4}});   // (wait 3)
    a.idf->n_docs += n_str;
    idf_drop_weights(*a.idf);
    return LATOK_OK;
}
// the blocking entry points' shared body, step by step; the idf's lock is taken before the call's turn on the stream
static int term_counts_common(TermsCall a) {
    LATOK_ENTER();
    int rc;
    if ((rc = terms_refusals(g, a))) return rc;
    Idf* const f = a.idf;
    const int64_t n_str = a.n_str;
    std::unique_lock<std::mutex> idf_lock;
    if (f) {
        idf_lock = std::unique_lock<std::mutex>(f->mu);
        if ((rc = check_device(g, "idf", f->device))) return rc;
        if (a.update && f->n_docs + std::max<int64_t>(n_str, 0) >= (1ll << 31))
            return fail(LATOK_ERR_INVALID, "the idf would hold %lld documents: df is int32 (fewer than 2^31)", (long long)(f->n_docs + n_str));
    }
    BytesCall c;   // (elt: the width of indptr and oov; an index and a count are 4 bytes in every mode)
    if ((rc = c.open(g, a.utf8, a.byte_off, n_str, a.total_bytes, a.flags, a.stream))) return rc;
    if (c.dev && ((uintptr_t)a.indptr_out & (c.elt - 1)) != 0) return fail(LATOK_ERR_INVALID, "misaligned output buffer");
    if (c.empty && a.update) {   // rows without an entry: documents all the same
        f->n_docs += n_str;
        if (n_str > 0) idf_drop_weights(*f);
        return LATOK_OK;
    }
    if (c.empty) {   // no byte, no token: every row is empty
        if ((rc = zero_counts(c.dev, a.indptr_out, (size_t)(n_str + 1) * c.elt, c.st))) return rc;
        return zero_counts(c.dev, a.oov_out, (size_t)n_str * c.elt, c.st, true);
    }
    if (c.dev && (((uintptr_t)a.oov_out & (c.elt - 1)) != 0 || ((uintptr_t)a.indices_out & 3) != 0 || ((uintptr_t)a.data_out & 3) != 0))
        return fail(LATOK_ERR_INVALID, "misaligned output buffer");
    const bool grams = a.kind != TermKind::Tokens;   // the kinds whose rows lie in key space
    const int route = (a.kind == TermKind::CharGrams ? 16 : a.kind == TermKind::WordGrams ? 14 : 9) + (a.hashed ? 1 : 0);
    const WsShape shape{.spans = true, .term_rows = n_str + 1, .ng_rows = grams ? n_str + 1 : 0, .tf_ctl = a.tfidf};
    if ((rc = c.stage(g, route, shape, (grams ? kClearNgrams : kClearSized) | (a.tfidf ? kClearTfidfErr : 0u)))) return rc;
    if ((rc = terms_stage_outputs(g, a, c))) return rc;
    if ((rc = enqueue_term_keys(g, g.ws, a))) return rc;
    // (no key: the scan did not run and nnz = 0)
    if (a.tfidf && a.indices && (grams ? a.n_grams : a.n_tokens) > 0 && (rc = enqueue_tfidf_tail(g, a))) return rc;
    return terms_deliver(g, a, c);
}
int latok_ngram_counts_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes, const latok_vocab* vocab,
                                        int min_n, int max_n, int sep, int64_t* indptr_out, int64_t* oov_out, int32_t* indices_out,
                                        int32_t* data_out, int64_t cap, int64_t* nnz_out, int64_t* n_grams_out, int flags, void* stream) {
    return term_counts_common({.utf8 = utf8, .byte_off = byte_off, .n_str = n_str, .total_bytes = total_bytes, .vocab = vocab, .kind = TermKind::WordGrams,
                               .min_n = min_n, .max_n = max_n, .sep = sep, .indptr_out = indptr_out, .oov_out = oov_out, .indices_out = indices_out,
                               .data_out = data_out, .cap = cap, .nnz_out = nnz_out, .n_grams_out = n_grams_out, .flags = flags, .stream = stream});
}
int latok_hashed_ngram_counts_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes, uint32_t seed,
                                               int64_t n_features, int alternate_sign, int min_n, int max_n, int sep, int64_t* indptr_out,
                                               int32_t* indices_out, int32_t* data_out, int64_t cap, int64_t* nnz_out, int64_t* n_grams_out,
                                               int flags, void* stream) {
    return term_counts_common({.utf8 = utf8, .byte_off = byte_off, .n_str = n_str, .total_bytes = total_bytes, .hashed = true, .seed = seed,
                               .n_features = n_features, .alternate_sign = alternate_sign, .kind = TermKind::WordGrams, .min_n = min_n, .max_n = max_n, .sep = sep,
                               .indptr_out = indptr_out, .indices_out = indices_out, .data_out = data_out, .cap = cap, .nnz_out = nnz_out,
                               .n_grams_out = n_grams_out, .flags = flags, .stream = stream});
}
int latok_chargram_counts_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes, const latok_vocab* vocab,
                                           int min_n, int max_n, int pad, int64_t* indptr_out, int64_t* oov_out, int32_t* indices_out,
                                           int32_t* data_out, int64_t cap, int64_t* nnz_out, int64_t* n_grams_out, int flags, void* stream) {
    return term_counts_common({.utf8 = utf8, .byte_off = byte_off, .n_str = n_str, .total_bytes = total_bytes, .vocab = vocab, .kind = TermKind::CharGrams,
                               .min_n = min_n, .max_n = max_n, .pad = pad, .indptr_out = indptr_out, .oov_out = oov_out,
                               .indices_out = indices_out, .data_out = data_out, .cap = cap, .nnz_out = nnz_out, .n_grams_out = n_grams_out,
                               .flags = flags, .stream = stream});
}
int latok_hashed_chargram_counts_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes, uint32_t seed,
                                                  int64_t n_features, int alternate_sign, int min_n, int max_n, int pad, int64_t* indptr_out,
                                                  int32_t* indices_out, int32_t* data_out, int64_t cap, int64_t* nnz_out, int64_t* n_grams_out,
                                                  int flags, void* stream) {
    return term_counts_common({.utf8 = utf8, .byte_off = byte_off, .n_str = n_str, .total_bytes = total_bytes, .hashed = true, .seed = seed,
                               .n_features = n_features, .alternate_sign = alternate_sign, .kind = TermKind::CharGrams, .min_n = min_n, .max_n = max_n,
                               .pad = pad, .indptr_out = indptr_out, .indices_out = indices_out, .data_out = data_out, .cap = cap,
                               .nnz_out = nnz_out, .n_grams_out = n_grams_out, .flags = flags, .stream = stream});
}
int latok_term_counts_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes, const latok_vocab* vocab,
                                       int64_t* indptr_out, int64_t* oov_out, int32_t* indices_out, int32_t* data_out, int64_t cap,
                                       int64_t* nnz_out, int64_t* n_tokens_out, int flags, void* stream) {
    return term_counts_common({.utf8 = utf8, .byte_off = byte_off, .n_str = n_str, .total_bytes = total_bytes, .vocab = vocab,
                               .indptr_out = indptr_out, .oov_out = oov_out, .indices_out = indices_out, .data_out = data_out, .cap = cap,
                               .nnz_out = nnz_out, .n_tokens_out = n_tokens_out, .flags = flags, .stream = stream});
}
int latok_hashed_term_counts_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes, uint32_t seed,
                                              int64_t n_features, int alternate_sign, int64_t* indptr_out, int32_t* indices_out,
                                              int32_t* data_out, int64_t cap, int64_t* nnz_out, int64_t* n_tokens_out, int flags, void* stream) {
    return term_counts_common({.utf8 = utf8, .byte_off = byte_off, .n_str = n_str, .total_bytes = total_bytes, .hashed = true, .seed = seed,
                               .n_features = n_features, .alternate_sign = alternate_sign, .indptr_out = indptr_out, .indices_out = indices_out,
                               .data_out = data_out, .cap = cap, .nnz_out = nnz_out, .n_tokens_out = n_tokens_out, .flags = flags, .stream = stream});
}

/* the TF-IDF entry points over text: term_counts_common with a tail; min_n = max_n = 1 with a one-byte sep takes the plain term counts'
 * kernels (the n-gram route checks its arguments itself) */
static TermKind tfidf_kind(int min_n, int max_n, int sep) {
    return min_n == 1 && max_n == 1 && sep >= 0 && sep <= 255 ? TermKind::Tokens : TermKind::WordGrams;
}
int latok_tfidf_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes, const latok_vocab* vocab, int min_n,
                                 int max_n, int sep, const latok_idf* idf, int opts, int64_t* indptr_out, int64_t* oov_out, int32_t* indices_out,
                                 float* data_out, int64_t cap, int64_t* nnz_out, int flags, void* stream) {
    return term_counts_common({.utf8 = utf8, .byte_off = byte_off, .n_str = n_str, .total_bytes = total_bytes, .vocab = vocab,
                               .kind = tfidf_kind(min_n, max_n, sep), .min_n = min_n, .max_n = max_n, .sep = sep, .tfidf = true,
                               .idf = const_cast<Idf*>(reinterpret_cast<const Idf*>(idf)), .opts = opts, .indptr_out = indptr_out, .oov_out = oov_out,
                               .indices_out = indices_out, .data_out = (int32_t*)data_out, .cap = cap, .nnz_out = nnz_out, .flags = flags, .stream = stream});
}
int latok_hashed_tfidf_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes, uint32_t seed,
                                        int64_t n_features, int alternate_sign, int min_n, int max_n, int sep, const latok_idf* idf, int opts,
                                        int64_t* indptr_out, int32_t* indices_out, float* data_out, int64_t cap, int64_t* nnz_out, int flags,
                                        void* stream) {
    return term_counts_common({.utf8 = utf8, .byte_off = byte_off, .n_str = n_str, .total_bytes = total_bytes, .hashed = true, .seed = seed,
                               .n_features = n_features, .alternate_sign = alternate_sign, .kind = tfidf_kind(min_n, max_n, sep), .min_n = min_n,
                               .max_n = max_n, .sep = sep, .tfidf = true, .idf = const_cast<Idf*>(reinterpret_cast<const Idf*>(idf)), .opts = opts,
                               .indptr_out = indptr_out, .indices_out = indices_out, .data_out = (int32_t*)data_out, .cap = cap, .nnz_out = nnz_out,
                               .flags = flags, .stream = stream});
}
int latok_idf_update_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes, const latok_vocab* vocab,
                                      uint32_t seed, int64_t n_features, int min_n, int max_n, int sep, latok_idf* idf, int64_t* nnz_out,
                                      int64_t* n_tokens_out, int flags, void* stream) {
    int64_t nnz = 0;
    return term_counts_common({.utf8 = utf8, .byte_off = byte_off, .n_str = n_str, .total_bytes = total_bytes, .vocab = vocab,
                               .hashed = vocab == nullptr, .seed = seed, .n_features = n_features, .kind = tfidf_kind(min_n, max_n, sep),
                               .min_n = min_n, .max_n = max_n, .sep = sep, .tfidf = true, .update = true, .idf = reinterpret_cast<Idf*>(idf),
                               .nnz_out = nnz_out ? nnz_out : &nnz, .n_tokens_out = n_tokens_out, .flags = flags, .stream = stream});
}

int latok_idf_create(int64_t n_cols, latok_idf** out) {
    LATOK_ENTER();
    if (!out) return fail(LATOK_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (n_cols < 1 || n_cols > (1ll << 28)) return fail(LATOK_ERR_INVALID, "n_cols must be in 1 .. 2^28");
    int rc = need_init(g);
    if (rc) return rc;
    Idf* f = nullptr;
    try {
        f = new Idf();
    } catch (const std::bad_alloc&) {
        return fail(LATOK_ERR_NOMEM, "out of host memory");
    }
    f->device = g.device;
    f->n_cols = n_cols;
    hipError_t e = f->df.alloc((size_t)n_cols * 4);
    if (e != hipSuccess) {
        delete f;
        return fail(LATOK_ERR_NOMEM, "hipMalloc of %lld document frequencies failed: %s", (long long)n_cols, hipGetErrorString(e));
    }
    e = hipMemsetAsync(f->df.p, 0, (size_t)n_cols * 4, g.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g.stream);
    if (e != hipSuccess) {
        delete f;
        return fail(LATOK_ERR_HIP, "clearing the document frequencies failed: %s", hipGetErrorString(e));
    }
    *out = reinterpret_cast<latok_idf*>(f);
    return LATOK_OK;
}

int latok_idf_destroy(latok_idf* idf) {
    LATOK_ENTER();
    return destroy_object(g, reinterpret_cast<Idf*>(idf), &Idf::mu);
}

int latok_idf_clear(latok_idf* idf) {
    LATOK_ENTER();
    Idf* f = reinterpret_cast<Idf*>(idf);
    if (!f) return fail(LATOK_ERR_INVALID, "idf is NULL");
    int rc = need_init(g);
    if (rc) return rc;
    std::lock_guard<std::mutex> il(f->mu);
    if ((rc = check_device(g, "idf", f->device))) return rc;
    HIP_TRY(hipMemsetAsync(f->df.p, 0, (size_t)f->n_cols * 4, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    f->n_docs = 0;
    idf_drop_weights(*f);
    return LATOK_OK;
}

int latok_idf_info(const latok_idf* idf, int64_t* n_cols, int64_t* n_docs, int* device) {
    Idf* f = const_cast<Idf*>(reinterpret_cast<const Idf*>(idf));
    if (!f) return fail(LATOK_ERR_INVALID, "idf is NULL");
    std::lock_guard<std::mutex> il(f->mu);
    if (n_cols) *n_cols = f->n_cols;
    if (n_docs) *n_docs = f->n_docs;
    if (device) *device = f->device;
    return LATOK_OK;
}

int latok_idf_read(const latok_idf* idf, int32_t* df_out, int64_t cap, int64_t* n_docs_out) {
    LATOK_ENTER();
    Idf* f = const_cast<Idf*>(reinterpret_cast<const Idf*>(idf));
    if (!f) return fail(LATOK_ERR_INVALID, "idf is NULL");
    if (n_docs_out) *n_docs_out = 0;
    if (cap < 0) return fail(LATOK_ERR_INVALID, "negative capacity");
    if (cap > 0 && !df_out) return fail(LATOK_ERR_INVALID, "df_out is NULL but cap > 0 (a size query passes cap = 0)");
    int rc = need_init(g);
    if (rc) return rc;
    std::lock_guard<std::mutex> il(f->mu);
    if ((rc = check_device(g, "idf", f->device))) return rc;
    if (n_docs_out) *n_docs_out = f->n_docs;
    if (cap == 0 && !df_out) return LATOK_OK;
    if (cap < f->n_cols) return fail(LATOK_ERR_INVALID, "capacity too small: need %lld columns", (long long)f->n_cols);
    HIP_TRY(hipMemcpyAsync(df_out, f->df.p, (size_t)f->n_cols * 4, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    return LATOK_OK;
}

int latok_idf_load(latok_idf* idf, const int32_t* df, int64_t n_docs) {
    LATOK_ENTER();
    Idf* f = reinterpret_cast<Idf*>(idf);
    if (!f) return fail(LATOK_ERR_INVALID, "idf is NULL");
    if (!df) return fail(LATOK_ERR_INVALID, "df is NULL");
    if (n_docs < 0 || n_docs >= (1ll << 31)) return fail(LATOK_ERR_INVALID, "n_docs must be in 0 .. 2^31 - 1");
    int rc = need_init(g);
    if (rc) return rc;
    std::lock_guard<std::mutex> il(f->mu);
    if ((rc = check_device(g, "idf", f->device))) return rc;
    for (int64_t c = 0; c < f->n_cols; ++c)
        if (df[c] < 0 || (int64_t)df[c] > n_docs) return fail(LATOK_ERR_INVALID, "df[%lld] = %d lies outside [0, n_docs]", (long long)c, (int)df[c]);
    HIP_TRY(hipMemcpyAsync(f->df.p, df, (size_t)f->n_cols * 4, hipMemcpyHostToDevice, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    f->n_docs = n_docs;
    idf_drop_weights(*f);
    return LATOK_OK;
}

int latok_idf_weights(const latok_idf* idf, int smooth, float* out, int64_t cap) {
    LATOK_ENTER();
    Idf* f = const_cast<Idf*>(reinterpret_cast<const Idf*>(idf));
    if (!f) return fail(LATOK_ERR_INVALID, "idf is NULL");
    if (!out) return fail(LATOK_ERR_INVALID, "out is NULL");
    int rc = need_init(g);
    if (rc) return rc;
    std::lock_guard<std::mutex> il(f->mu);
    if ((rc = check_device(g, "idf", f->device))) return rc;
    if (cap < f->n_cols) return fail(LATOK_ERR_INVALID, "capacity too small: need %lld columns", (long long)f->n_cols);
    const float* w = nullptr;
    if ((rc = idf_weights_on(*f, smooth != 0, g.stream, &w))) return rc;
    HIP_TRY(hipMemcpyAsync(out, w, (size_t)f->n_cols * 4, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    return LATOK_OK;
}

// A caller's CSR for the device: device pointers as they are, host arrays copied into the workspace; then the check.  finish() waits
// for the call's kernels and turns the error word into the refusal.
struct CsrCall {
    bool dev = false, o32 = false;
    std::optional<StreamTurn> turn;
    hipStream_t st = nullptr;
    const void* indptr = nullptr;
    const int32_t* indices = nullptr;
    int32_t* data = nullptr;       // host callers: the staged copy, which the weighting overwrites in place
    int* d_err = nullptr;
    int open(Ctx& g, const void* indptr_in, const int32_t* indices_in, const int32_t* data_in, int64_t n_rows, int64_t nnz, int64_t n_cols, int flags,
             void* stream) {
        int rc;
        dev = (flags & LATOK_DEVICE_PTRS) != 0;
        o32 = (flags & LATOK_OUT_INT32) != 0;
        const size_t elt = o32 ? 4 : 8;
        if (dev && (((uintptr_t)indptr_in & (elt - 1)) != 0 || ((uintptr_t)indices_in & 3) != 0 || ((uintptr_t)data_in & 3) != 0))
            return fail(LATOK_ERR_INVALID, "misaligned buffer");
        turn.emplace(g, stream);
        st = turn->st;
        WsShape shape;
        shape.tf_ctl = true;
        if (!dev) {
            shape.tf_ptr_bytes = (int64_t)((size_t)(n_rows + 1) * elt);
            shape.tf_entries = nnz;
        }
        if ((rc = ws_ensure(ws_needs(g.ws, 0, shape).data(), kWsNeeds)) || (rc = g.pin_tot.ensure(64))) return rc;
        indptr = indptr_in;
        indices = indices_in;
        data = const_cast<int32_t*>(data_in);
        if (!dev) {
            HIP_TRY(hipMemcpyAsync(g.ws.tfptr.p, indptr_in, (size_t)(n_rows + 1) * elt, hipMemcpyHostToDevice, st));
            indptr = g.ws.tfptr.p;
            if (nnz > 0) HIP_TRY(hipMemcpyAsync(g.ws.tfidx.p, indices_in, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
            indices = (const int32_t*)g.ws.tfidx.p;
            if (data_in && nnz > 0) HIP_TRY(hipMemcpyAsync(g.ws.tfval.p, data_in, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
            data = (int32_t*)g.ws.tfval.p;
        }
        d_err = (int*)g.ws.tfctl.p;
        HIP_TRY(hipMemsetAsync(d_err, 0, 4, st));
        HIP_TRY(latok::launch_csr_check(o32, indptr, indices, n_rows, nnz, nullptr, 0, n_cols, d_err, st));
        return LATOK_OK;
    }
    int finish(Ctx& g) {
        volatile int64_t* h = (volatile int64_t*)g.pin_tot.h;
        h[7] = 0;
        HIP_TRY(hipMemcpyAsync((void*)(h + 7), d_err, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return csr_refusal((int)h[7]);
    }
};
static int csr_args(const void* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, int flags) {
    if (flags & ~(LATOK_OUT_INT32 | LATOK_DEVICE_PTRS)) return fail(LATOK_ERR_INVALID, "unknown flag");
    if (n_rows < 0) return fail(LATOK_ERR_INVALID, "n_rows must be >= 0");
    if (nnz < 0) return fail(LATOK_ERR_INVALID, "nnz must be >= 0");
    if ((flags & LATOK_OUT_INT32) && (nnz > 0x7FFFFFFFll || n_rows >= 0x7FFFFFFFll)) return fail(LATOK_ERR_INVALID, "nnz does not fit an int32 indptr");
    if (n_rows == 0 && nnz != 0) return fail(LATOK_ERR_INVALID, "indptr[n_rows] does not match nnz");
    if (n_rows > 0 && !indptr) return fail(LATOK_ERR_INVALID, "indptr is NULL");
    if (nnz > 0 && !indices) return fail(LATOK_ERR_INVALID, "indices is NULL");
    return LATOK_OK;
}

int latok_idf_update_csr(latok_idf* idf, const void* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, int flags, void* stream) {
    LATOK_ENTER();
    Idf* f = reinterpret_cast<Idf*>(idf);
    if (!f) return fail(LATOK_ERR_INVALID, "idf is NULL");
    int rc = csr_args(indptr, indices, n_rows, nnz, flags);
    if (rc || (rc = need_init(g))) return rc;
    std::lock_guard<std::mutex> il(f->mu);
    if ((rc = check_device(g, "idf", f->device))) return rc;
    if (f->n_docs + n_rows >= (1ll << 31))
        return fail(LATOK_ERR_INVALID, "the idf would hold %lld documents: df is int32 (fewer than 2^31)", (long long)(f->n_docs + n_rows));
    if (n_rows == 0) return LATOK_OK;
    CsrCall c;
    if ((rc = c.open(g, indptr, indices, nullptr, n_rows, nnz, f->n_cols, flags, stream))) return rc;
    HIP_TRY(latok::launch_df_add(g_df_add_cached != 0, c.indices, nnz, nullptr, 0, c.d_err, f->df.as<int32_t>(), c.st));
    if ((rc = c.finish(g))) return rc;
    f->n_docs += n_rows;
    idf_drop_weights(*f);
    return LATOK_OK;
}

int latok_tfidf_csr(const void* indptr, const int32_t* indices, const int32_t* data, int64_t n_rows, int64_t nnz, const latok_idf* idf, int opts,
                    float* data_out, int flags, void* stream) {
    LATOK_ENTER();
    Idf* f = const_cast<Idf*>(reinterpret_cast<const Idf*>(idf));
    int rc = csr_args(indptr, indices, n_rows, nnz, flags);
    if (rc || (rc = tfidf_check_opts(opts))) return rc;
    if (nnz > 0 && (!data || !data_out)) return fail(LATOK_ERR_INVALID, "data or data_out is NULL");
    if ((rc = need_init(g))) return rc;
    std::unique_lock<std::mutex> il;
    if (f) {
        il = std::unique_lock<std::mutex>(f->mu);
        if ((rc = check_device(g, "idf", f->device))) return rc;
    }
    if (n_rows == 0) return LATOK_OK;
    CsrCall c;
    if ((flags & LATOK_DEVICE_PTRS) && ((uintptr_t)data_out & 3) != 0) return fail(LATOK_ERR_INVALID, "misaligned buffer");
    if ((rc = c.open(g, indptr, indices, data, n_rows, nnz, f ? f->n_cols : 0, flags, stream))) return rc;
    const float* weights = nullptr;
    if (f && (rc = idf_weights_on(*f, (opts & kTwSmoothIdf) != 0, c.st, &weights))) return rc;
    float* out = c.dev ? data_out : (float*)c.data;
    HIP_TRY(latok::launch_tfidf_rows(c.o32, c.indptr, c.indices, c.data, n_rows, nnz, nullptr, 0, weights, opts, c.d_err, out, c.st));
    if ((rc = c.finish(g))) return rc;
    if (!c.dev && nnz > 0) {
        HIP_TRY(hipMemcpyAsync(data_out, out, (size_t)nnz * 4, hipMemcpyDeviceToHost, c.st));
        HIP_TRY(hipStreamSynchronize(c.st));
    }
    return LATOK_OK;
}

/* test hooks (not part of the ABI in include/latok_hip.h).  latok_debug_tfidf_limits: out[0] = kTfidfSubMax, the longest row that 16
 * lanes take; out[1] = kTfidfWaveMax, the longest row that a wave takes (a longer one gets a workgroup of the second launch); out[2] =
 * kDfSlots, the columns a workgroup of k_df_add caches.  latok_debug_set_df_add: 1 = k_df_add with its LDS table (the default), 0 = the
 * plain form; returns the mode that was set before. */
extern "C" int latok_debug_tfidf_limits(int64_t* out, int n) {
    const int64_t v[3] = {latok::kTfidfSubMax, latok::kTfidfWaveMax, latok::kDfSlots};
    for (int i = 0; i < n && i < 3; ++i) out[i] = v[i];
    return 3;
}
extern "C" int latok_debug_set_df_add(int cached) {
    const int before = g_df_add_cached;
    g_df_add_cached = cached ? 1 : 0;
    return before;
}

/* WordPiece in byte space (latok_wordpiece_ids_utf8_bytes_batch, latok_wordpiece_padded_utf8_bytes_batch): the subword ids of every
 * token.  The vocabulary object holds two vocab_table.h tables (wordpiece.h: initial and continuation), built on the host, uploaded
 * once, read only afterwards.  One stream, every batch size the same kernels:
 *   sized_token_front (wait 1)                    kept mask, token ranks; the host reads THE token total (pinned word 0): the token buffers are sized
 *   enqueue_token_rows                            the span record of every token at its rank in the workspace, the row starts in token space
 *   k_wp_count                                    pieces per token
 *   k_scan_chained                                piece ranks; the piece total -> scalar word 5, pinned word 3
 *   (padded form: wait 2)                         the piece total sizes the ids of the workspace
 *   k_wp_emit                                     ids (and spans) at the piece rank, if the total fits the capacity
 *   k_wp_rows / k_wp_pad                          indptr in the caller's width / the padded block and the lengths
 *   (last wait)                                   the piece total; host pointers then copy that many pieces (one wait more)
 * `w` was sized by ws_needs with WsShape{.spans = true, .term_rows = n_str + 1}; the call sizes the token buffers itself. */
struct WordPiece {                 // latok_wordpiece: immutable once created
    int device = -1;
    int64_t n_words = 0;
    uint32_t max_len0 = 0, max_len1 = 0;
    uint8_t prefix[kWpMaxPrefix] = {0};
    int prefix_len = 0, max_chars = 0;
    uint32_t seed = 0;
    DevTable initial, cont;
};
int latok_wordpiece_create(const uint8_t* words, const int64_t* word_off, int64_t n_words, const int32_t* word_ids, const uint8_t* prefix,
                           int prefix_len, int max_chars, uint32_t seed, latok_wordpiece** wp_out) {
    LATOK_ENTER();
    // what needs no device is refused first
    if (!wp_out) return fail(LATOK_ERR_INVALID, "wp_out is NULL");
    *wp_out = nullptr;
    if (prefix_len < 0 || prefix_len > kWpMaxPrefix) return fail(LATOK_ERR_INVALID, "prefix_len must be in 0 .. %d", kWpMaxPrefix);
    if (prefix_len > 0 && !prefix) return fail(LATOK_ERR_INVALID, "prefix is NULL");
    if (max_chars < 1 || max_chars > kWpMaxChars) return fail(LATOK_ERR_INVALID, "max_chars must be in 1 .. %d", kWpMaxChars);
    int rc = check_word_list(words, word_off, n_words);
    if (rc || (rc = need_init(g))) return rc;
    WpTables t;
    WordPiece* v = nullptr;
    try {
        wp_build(words, word_off, n_words, word_ids, prefix, prefix_len, seed, &t);
        v = new WordPiece();
    } catch (const std::bad_alloc&) {
        return fail(LATOK_ERR_NOMEM, "out of host memory");
    }
    v->device = g.device;
    v->n_words = n_words;
    v->max_len0 = t.max_len0;
    v->max_len1 = t.max_len1;
    for (int i = 0; i < prefix_len; ++i) v->prefix[i] = prefix[i];
    v->prefix_len = prefix_len;
    v->max_chars = max_chars;
    v->seed = seed;
    if ((rc = v->initial.upload(t.initial, g.stream)) == LATOK_OK) rc = v->cont.upload(t.cont, g.stream);
    const hipError_t e = hipStreamSynchronize(g.stream);   // (the host tables die with this call, and every context may use the object at once)
    if (!rc && e != hipSuccess) rc = fail(LATOK_ERR_HIP, "uploading the vocabulary failed: %s", hipGetErrorString(e));
    if (rc) {
        delete v;
        return rc;
    }
    *wp_out = reinterpret_cast<latok_wordpiece*>(v);
    return LATOK_OK;
}

int latok_wordpiece_destroy(latok_wordpiece* wp) {
    LATOK_ENTER();
    return destroy_object(g, reinterpret_cast<WordPiece*>(wp));
}

int latok_wordpiece_info(const latok_wordpiece* wp, int64_t* n_words, int64_t* n_slots_initial, int64_t* n_slots_cont, int64_t* max_len_initial,
                         int64_t* max_len_cont, uint8_t* prefix_out, int* prefix_len, int* max_chars, uint32_t* seed, int* device) {
    const WordPiece* v = reinterpret_cast<const WordPiece*>(wp);
    if (!v) return fail(LATOK_ERR_INVALID, "wp is NULL");
    if (n_words) *n_words = v->n_words;
    if (n_slots_initial) *n_slots_initial = (int64_t)v->initial.n_slots;
    if (n_slots_cont) *n_slots_cont = (int64_t)v->cont.n_slots;
    if (max_len_initial) *max_len_initial = v->max_len0;
    if (max_len_cont) *max_len_cont = v->max_len1;
    if (prefix_out) memcpy(prefix_out, v->prefix, kWpMaxPrefix);
    if (prefix_len) *prefix_len = v->prefix_len;
    if (max_chars) *max_chars = v->max_chars;
    if (seed) *seed = v->seed;
    if (device) *device = v->device;
    return LATOK_OK;
}

/* Byte-level BPE in byte space (latok_bpe_ids_utf8_bytes_batch, latok_bpe_padded_utf8_bytes_batch): the calls of the WordPiece pair with
 * another cut.  The object holds one vocab_table.h table whose id slot is the word's rank, the rank -> id array and the longest word
 * (bpe.h), built on the host, uploaded once, read only afterwards.  The stream is enqueue_wordpiece's, with k_bpe_count / k_bpe_emit
 * (bpe_kernels.hip) in place of k_wp_count / k_wp_emit and 8 bytes of part-start mask per token between the two. */
struct Bpe {                       // latok_bpe: immutable once created
    int device = -1;
    int64_t n_words = 0;
    uint32_t max_len = 0;
    int max_bytes = 0, lead_space = 0;
    int pretok = kPretokLatok;     // what cuts the text into the tokens that are merged (LATOK_PRETOK_*)
    uint32_t seed = 0;
    DevTable table;
    DevMem rank_id;
    // an object of latok_bpe_create_spm (pretok == kPretokSpm): SentencePiece BPE (spbpe.h)
    int add_dummy_prefix = 0, fuse_unk = 0;
    bool byte_fallback = false;
    DevMem byte_ids;               // [256] int32 when byte_fallback
};
// the body of latok_bpe_create_pretok and latok_bpe_create_spm, behind their own refusals
static int bpe_create_object(const uint8_t* words, const int64_t* word_off, int64_t n_words, const int32_t* word_ids, int max_bytes, int lead_space,
                             int pretok, const int32_t* byte_ids, int add_dummy_prefix, int fuse_unk, uint32_t seed, latok_bpe** bpe_out);
int latok_bpe_create_pretok(const uint8_t* words, const int64_t* word_off, int64_t n_words, const int32_t* word_ids, int max_bytes, int lead_space,
                            int pretok, uint32_t seed, latok_bpe** bpe_out) {
    // what needs no device is refused first
    if (!bpe_out) return fail(LATOK_ERR_INVALID, "bpe_out is NULL");
    *bpe_out = nullptr;
    if (max_bytes < 1 || max_bytes > kBpeMaxBytes) return fail(LATOK_ERR_INVALID, "max_bytes must be in 1 .. %d", kBpeMaxBytes);
    if (lead_space != 0 && lead_space != 1) return fail(LATOK_ERR_INVALID, "lead_space must be 0 or 1");
    if (pretok == kPretokSpm)
        return fail(LATOK_ERR_INVALID, "LATOK_PRETOK_SPM takes latok_bpe_create_spm: byte merges over SentencePiece's segments mean nothing");
    if (pretok != kPretokLatok && pretok != kPretokGpt2 && pretok != kPretokCl100k)
        return fail(LATOK_ERR_INVALID, "unknown pretok %d (LATOK_PRETOK_LATOK, LATOK_PRETOK_GPT2 or LATOK_PRETOK_CL100K)", pretok);
    if (pretok != kPretokLatok && lead_space)
        return fail(LATOK_ERR_INVALID, "lead_space must be 0 with %s: the space is already in the pre-token", pretok == kPretokGpt2 ? "LATOK_PRETOK_GPT2" : "LATOK_PRETOK_CL100K");
    return bpe_create_object(words, word_off, n_words, word_ids, max_bytes, lead_space, pretok, nullptr, 0, 0, seed, bpe_out);
}
int latok_bpe_create_spm(const uint8_t* words, const int64_t* word_off, int64_t n_words, const int32_t* word_ids, const int32_t* byte_ids,
                         int add_dummy_prefix, int fuse_unk, int max_bytes, uint32_t seed, latok_bpe** bpe_out) {
    // what needs no device is refused first
    if (!bpe_out) return fail(LATOK_ERR_INVALID, "bpe_out is NULL");
    *bpe_out = nullptr;
    if (max_bytes < 1 || max_bytes > kBpeMaxBytes) return fail(LATOK_ERR_INVALID, "max_bytes must be in 1 .. %d", kBpeMaxBytes);
    if (add_dummy_prefix != 0 && add_dummy_prefix != 1) return fail(LATOK_ERR_INVALID, "add_dummy_prefix must be 0 or 1");
    if (fuse_unk != 0 && fuse_unk != 1) return fail(LATOK_ERR_INVALID, "fuse_unk must be 0 or 1");
    const int rc = check_word_list(words, word_off, n_words);
    if (rc) return rc;
    const int64_t bad = sp_first_bad_word(words, word_off, n_words);
    if (bad >= 0)
        return fail(LATOK_ERR_INVALID, "word %lld holds E2 96 81 behind another character: segments would not be independent", (long long)bad);
    return bpe_create_object(words, word_off, n_words, word_ids, max_bytes, 0, kPretokSpm, byte_ids, add_dummy_prefix, fuse_unk, seed, bpe_out);
}
static int bpe_create_object(const uint8_t* words, const int64_t* word_off, int64_t n_words, const int32_t* word_ids, int max_bytes, int lead_space,
                             int pretok, const int32_t* byte_ids, int add_dummy_prefix, int fuse_unk, uint32_t seed, latok_bpe** bpe_out) {
    LATOK_ENTER();
    int rc = check_word_list(words, word_off, n_words);
    if (rc || (rc = need_init(g))) return rc;
    BpeTables t;
    Bpe* v = nullptr;
    try {
        bpe_build(words, word_off, n_words, word_ids, seed, &t);
        v = new Bpe();
    } catch (const std::bad_alloc&) {
        return fail(LATOK_ERR_NOMEM, "out of host memory");
    }
    v->device = g.device;
    v->n_words = n_words;
    v->max_len = t.max_len;
    v->max_bytes = max_bytes;
    v->lead_space = lead_space;
    v->pretok = pretok;
    v->seed = seed;
    v->add_dummy_prefix = add_dummy_prefix;
    v->fuse_unk = fuse_unk;
    v->byte_fallback = byte_ids != nullptr;
    if ((rc = v->table.upload(t.table, g.stream)) == LATOK_OK) {
        const size_t bytes = t.rank_id.size() * 4;
        hipError_t e = v->rank_id.alloc(bytes);
        if (e != hipSuccess) rc = fail(LATOK_ERR_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        else if ((e = hipMemcpyAsync(v->rank_id.p, t.rank_id.data(), bytes, hipMemcpyHostToDevice, g.stream)) != hipSuccess)
            rc = fail(LATOK_ERR_HIP, "uploading the vocabulary failed: %s", hipGetErrorString(e));
    }
    if (!rc && byte_ids) {   // (pageable host memory: the copy has read it when the call returns)
        hipError_t e = v->byte_ids.alloc(256 * 4);
        if (e != hipSuccess) rc = fail(LATOK_ERR_NOMEM, "hipMalloc(%zu) failed: %s", (size_t)1024, hipGetErrorString(e));
        else if ((e = hipMemcpyAsync(v->byte_ids.p, byte_ids, 256 * 4, hipMemcpyHostToDevice, g.stream)) != hipSuccess)
            rc = fail(LATOK_ERR_HIP, "uploading the vocabulary failed: %s", hipGetErrorString(e));
    }
    const hipError_t e = hipStreamSynchronize(g.stream);   // (the host tables die with this call, and every context may use the object at once)
    if (!rc && e != hipSuccess) rc = fail(LATOK_ERR_HIP, "uploading the vocabulary failed: %s", hipGetErrorString(e));
    if (rc) {
        delete v;
        return rc;
    }
    *bpe_out = reinterpret_cast<latok_bpe*>(v);
    return LATOK_OK;
}

int latok_bpe_create(const uint8_t* words, const int64_t* word_off, int64_t n_words, const int32_t* word_ids, int max_bytes, int lead_space,
                     uint32_t seed, latok_bpe** bpe_out) {
    return latok_bpe_create_pretok(words, word_off, n_words, word_ids, max_bytes, lead_space, LATOK_PRETOK_LATOK, seed, bpe_out);
}

int latok_bpe_pretokenizer(const latok_bpe* bpe, int* pretok) {
    const Bpe* v = reinterpret_cast<const Bpe*>(bpe);
    if (!v) return fail(LATOK_ERR_INVALID, "bpe is NULL");
    if (!pretok) return fail(LATOK_ERR_INVALID, "pretok is NULL");
    *pretok = v->pretok;
    return LATOK_OK;
}

int latok_bpe_spm_info(const latok_bpe* bpe, int* byte_fallback, int* add_dummy_prefix, int* fuse_unk) {
    const Bpe* v = reinterpret_cast<const Bpe*>(bpe);
    if (!v) return fail(LATOK_ERR_INVALID, "bpe is NULL");
    if (v->pretok != kPretokSpm) return fail(LATOK_ERR_INVALID, "bpe is not an object of latok_bpe_create_spm");
    if (byte_fallback) *byte_fallback = v->byte_fallback ? 1 : 0;
    if (add_dummy_prefix) *add_dummy_prefix = v->add_dummy_prefix;
    if (fuse_unk) *fuse_unk = v->fuse_unk;
    return LATOK_OK;
}

int latok_bpe_destroy(latok_bpe* bpe) {
    LATOK_ENTER();
    return destroy_object(g, reinterpret_cast<Bpe*>(bpe));
}

int latok_bpe_info(const latok_bpe* bpe, int64_t* n_words, int64_t* n_slots, int64_t* max_len, int* max_bytes, int* lead_space, uint32_t* seed,
                   int* device) {
    const Bpe* v = reinterpret_cast<const Bpe*>(bpe);
    if (!v) return fail(LATOK_ERR_INVALID, "bpe is NULL");
    if (n_words) *n_words = v->n_words;
    if (n_slots) *n_slots = (int64_t)v->table.n_slots;
    if (max_len) *max_len = v->max_len;
    if (max_bytes) *max_bytes = v->max_bytes;
    if (lead_space) *lead_space = v->lead_space;
    if (seed) *seed = v->seed;
    if (device) *device = v->device;
    return LATOK_OK;
}

/* Unigram in byte space (latok_unigram_ids_utf8_bytes_batch, latok_unigram_padded_utf8_bytes_batch): the calls of the WordPiece and BPE
 * pairs with a third cut.  The object holds two vocab_table.h tables whose id slot is the word's position in the list (every word; the
 * words behind the marker), the position -> id and position -> score arrays, the longest word of either table and the marker-alone
 * word (unigram.h), built on the host, uploaded once, read only afterwards.  The stream is enqueue_wordpiece's, with k_uni_count /
 * k_uni_emit (unigram_kernels.hip) in place of k_wp_count / k_wp_emit and 24 bytes per token between the two. */
struct Unigram {                   // latok_unigram: immutable once created
    int device = -1;
    int64_t n_words = 0;
    uint32_t max_len_plain = 0, max_len_marked = 0;
    int32_t marker_pos = -1;
    uint8_t marker[kUniMaxMarker] = {0};
    int marker_len = 0;
    float unk_score = 0.0f;
    int fuse_unk = 0, max_bytes = 0;
    uint32_t seed = 0;
    DevTable plain, marked;
    DevMem pos_id, pos_score;
};
int latok_unigram_create(const uint8_t* words, const int64_t* word_off, int64_t n_words, const float* scores, const int32_t* word_ids,
                         const uint8_t* marker, int marker_len, float unk_score, int fuse_unk, int max_bytes, uint32_t seed, latok_unigram** uni_out) {
    LATOK_ENTER();
    // what needs no device is refused first
    if (!uni_out) return fail(LATOK_ERR_INVALID, "uni_out is NULL");
    *uni_out = nullptr;
    if (max_bytes < 1 || max_bytes > kUniMaxBytes) return fail(LATOK_ERR_INVALID, "max_bytes must be in 1 .. %d", kUniMaxBytes);
    if (fuse_unk != 0 && fuse_unk != 1) return fail(LATOK_ERR_INVALID, "fuse_unk must be 0 or 1");
    if (marker_len < 0 || marker_len > kUniMaxMarker) return fail(LATOK_ERR_INVALID, "marker_len must be in 0 .. %d", kUniMaxMarker);
    if (marker_len > 0 && !marker) return fail(LATOK_ERR_INVALID, "marker is NULL");
    if (!uni_marker_ok(marker, marker_len)) return fail(LATOK_ERR_INVALID, "the marker must be exactly one character");
    if (!std::isfinite(unk_score)) return fail(LATOK_ERR_INVALID, "unk_score must be finite");
    int rc = check_word_list(words, word_off, n_words);
    if (rc) return rc;
    if (n_words > 0 && !scores) return fail(LATOK_ERR_INVALID, "scores is NULL");
    for (int64_t i = 0; i < n_words; ++i)
        if (!std::isfinite(scores[i])) return fail(LATOK_ERR_INVALID, "scores[%lld] is not finite", (long long)i);
    if ((rc = need_init(g))) return rc;
    UniTables t;
    Unigram* v = nullptr;
    try {
        uni_build(words, word_off, n_words, scores, word_ids, marker, marker_len, seed, &t);
        v = new Unigram();
    } catch (const std::bad_alloc&) {
        return fail(LATOK_ERR_NOMEM, "out of host memory");
    }
    v->device = g.device;
    v->n_words = n_words;
    v->max_len_plain = t.max_len_plain;
    v->max_len_marked = t.max_len_marked;
    v->marker_pos = t.marker_pos;
    for (int i = 0; i < marker_len; ++i) v->marker[i] = marker[i];
    v->marker_len = marker_len;
    v->unk_score = unk_score;
    v->fuse_unk = fuse_unk;
    v->max_bytes = max_bytes;
    v->seed = seed;
    if ((rc = v->plain.upload(t.plain, g.stream)) == LATOK_OK && (rc = v->marked.upload(t.marked, g.stream)) == LATOK_OK) {
        const size_t bytes = t.pos_id.size() * 4;
        hipError_t e = v->pos_id.alloc(bytes);
        if (e == hipSuccess) e = v->pos_score.alloc(bytes);
        if (e != hipSuccess) rc = fail(LATOK_ERR_NOMEM, "hipMalloc(%zu) failed: %s", 2 * bytes, hipGetErrorString(e));
        else if ((e = hipMemcpyAsync(v->pos_id.p, t.pos_id.data(), bytes, hipMemcpyHostToDevice, g.stream)) != hipSuccess ||
                 (e = hipMemcpyAsync(v->pos_score.p, t.pos_score.data(), bytes, hipMemcpyHostToDevice, g.stream)) != hipSuccess)
            rc = fail(LATOK_ERR_HIP, "uploading the vocabulary failed: %s", hipGetErrorString(e));
    }
    const hipError_t e = hipStreamSynchronize(g.stream);   // (the host tables die with this call, and every context may use the object at once)
    if (!rc && e != hipSuccess) rc = fail(LATOK_ERR_HIP, "uploading the vocabulary failed: %s", hipGetErrorString(e));
    if (rc) {
        delete v;
        return rc;
    }
    *uni_out = reinterpret_cast<latok_unigram*>(v);
    return LATOK_OK;
}

int latok_unigram_destroy(latok_unigram* uni) {
    LATOK_ENTER();
    return destroy_object(g, reinterpret_cast<Unigram*>(uni));
}

int latok_unigram_info(const latok_unigram* uni, int64_t* n_words, int64_t* n_slots_plain, int64_t* n_slots_marked, int64_t* max_len,
                       int64_t* marker_word, uint8_t* marker_out, int* marker_len, float* unk_score, int* fuse_unk, int* max_bytes, uint32_t* seed,
                       int* device) {
    const Unigram* v = reinterpret_cast<const Unigram*>(uni);
    if (!v) return fail(LATOK_ERR_INVALID, "uni is NULL");
    if (n_words) *n_words = v->n_words;
    if (n_slots_plain) *n_slots_plain = (int64_t)v->plain.n_slots;
    if (n_slots_marked) *n_slots_marked = (int64_t)v->marked.n_slots;
    if (max_len) *max_len = std::max(v->max_len_plain, v->max_len_marked);
    if (marker_word) *marker_word = v->marker_pos;
    if (marker_out) memcpy(marker_out, v->marker, kUniMaxMarker);
    if (marker_len) *marker_len = v->marker_len;
    if (unk_score) *unk_score = v->unk_score;
    if (fuse_unk) *fuse_unk = v->fuse_unk;
    if (max_bytes) *max_bytes = v->max_bytes;
    if (seed) *seed = v->seed;
    if (device) *device = v->device;
    return LATOK_OK;
}

// the object of a piece call: a WordPiece vocabulary, a BPE one or a Unigram one (exactly one is set), and the route numbers of its two forms
struct PieceCut {
    const WordPiece* wp = nullptr;
    const Bpe* bpe = nullptr;
    const Unigram* uni = nullptr;
    int route_ids = 11, route_padded = 12;
    // the front of the call: a BPE object made with LATOK_PRETOK_GPT2 brings its own, and its two routes
    int pretok() const { return bpe ? bpe->pretok : kPretokLatok; }
    void route_by_front() {
        if (pretok() == kPretokGpt2) { route_ids = 24; route_padded = 25; }
        if (pretok() == kPretokCl100k) { route_ids = 27; route_padded = 28; }
        if (pretok() == kPretokSpm) { route_ids = 30; route_padded = 31; }
    }
};

struct WordPieceCall {
    Batch b;                       // UTF-8 bytes on the device (16-byte aligned), byte offsets, total in bytes (> 0), n_str > 0
    PieceCut cut;
    int32_t unk = 0;
    void* indptr = nullptr;        // [n_str + 1]; NULL: the padded form
    int32_t* ids = nullptr;        // NULL: a size query (ids form)
    void* spans = nullptr;         // NULL: not asked for
    int64_t cap = 0;               // in pieces
    bool o32 = false;              // width of indptr and spans
    bool padded = false;           // the padded form: the ids go to the workspace, then k_wp_pad
    int64_t max_length = 0;
    int add_special = 0;
    int32_t cls_id = 0, sep_id = 0, pad_id = 0;
    int32_t* input_ids = nullptr;  // [n_str * max_length]
    int32_t* lengths = nullptr;    // [n_str]
    int64_t* p_tot = nullptr;      // the pinned words as the device sees them (cleared by the caller): 0 tokens, 1 flags, 3 pieces
    volatile int64_t* h_tot = nullptr;
    int64_t n_tokens = 0;          // (out) the token total
    hipStream_t st = nullptr;
};
static int enqueue_wordpiece(Ctx& g, Workspace& w, WordPieceCall& a) {
    int rc;
    const hipStream_t st = a.st;
    const int64_t total = a.b.total, n_str = a.b.n_str;
    int* d_err = (int*)(a.p_tot + 1);
    latok::TokenPlanes t;
    if ((rc = sized_token_front(g, w, a.b, a.p_tot, a.h_tot, st, "the batch has %lld tokens: a call takes fewer than 2^31 pieces", &t, &a.n_tokens,
                                a.cut.pretok())))
        return rc;
    int64_t* d_total = (int64_t*)w.scalar.p;
    const int64_t n_tok = a.n_tokens;
    if (n_tok > 0 && (rc = ws_ensure(ws_needs(w, total, WsShape{.spans = true, .term_rows = n_str + 1, .wp_tokens = n_tok, .bpe_tokens = a.cut.bpe ? n_tok : 0,
                                                                 .uni_tokens = a.cut.uni ? n_tok : 0}).data(),
                                    kWsNeeds)))
        return rc;
    int64_t* d_cnt = (int64_t*)w.trows.p;       // token count of every string, one zero entry behind them
    int64_t* d_start = d_cnt + (n_str + 1);     // their exclusive scan: d_start[n_str] = the token total
    int64_t* d_pcnt = (int64_t*)w.wpcnt.p;
    int64_t* d_prank = (int64_t*)w.wprank.p;
    const int32_t* d_ids = a.ids;
    if (n_tok > 0) {
        HIP_TRY(hipMemsetAsync(d_cnt, 0, (size_t)(n_str + 1) * 8, st));
        latok::TokenText text;
        if ((rc = enqueue_token_rows(w, a.b, t, n_tok, d_cnt, d_start, d_err, st, &text))) return rc;
        latok::WordPieceTables wt;
        latok::BpeTable bt;
        latok::SpBpeTable spt;
        const bool spm = a.cut.pretok() == kPretokSpm;
        uint64_t* d_mask = (uint64_t*)w.bpemask.p;
        latok::UniTable ut;
        uint64_t* d_marks = (uint64_t*)w.unimarks.p;
        if (const Bpe* b = a.cut.bpe) {
            bt.table = b->table.view(b->seed);
            bt.rank_id = b->rank_id.as<const int32_t>();
            bt.n_words = b->n_words;
            bt.max_len = b->max_len;
            bt.max_bytes = b->max_bytes;
            bt.lead_space = b->lead_space;
            if (spm) {
                spt.bt = bt;
                spt.byte_ids = b->byte_fallback ? b->byte_ids.as<const int32_t>() : nullptr;
                spt.add_dummy_prefix = b->add_dummy_prefix;
                spt.fuse_unk = b->fuse_unk;
                HIP_TRY(latok::launch_spbpe_count(text, spt, d_pcnt, d_mask, st));
            } else {
                HIP_TRY(latok::launch_bpe_count(text, bt, d_pcnt, d_mask, st));
            }
        } else if (const Unigram* u = a.cut.uni) {
            ut.plain = u->plain.view(u->seed);
            ut.marked = u->marked.view(u->seed);
            ut.pos_id = u->pos_id.as<const int32_t>();
            ut.pos_score = u->pos_score.as<const float>();
            ut.n_words = u->n_words;
            ut.max_len_plain = u->max_len_plain;
            ut.max_len_marked = u->max_len_marked;
            ut.marker_pos = u->marker_pos;
            ut.marker_len = u->marker_len;
            ut.unk_score = u->unk_score;
            ut.fuse_unk = u->fuse_unk;
            ut.max_bytes = u->max_bytes;
            HIP_TRY(latok::launch_uni_count(text, ut, d_pcnt, d_marks, st));
        } else {
            const WordPiece* v = a.cut.wp;
            wt.initial = v->initial.view(v->seed);
            wt.cont = v->cont.view(v->seed);
            wt.max_len0 = v->max_len0;
            wt.max_len1 = v->max_len1;
            wt.max_chars = v->max_chars;
            HIP_TRY(latok::launch_wp_count(text, wt, d_pcnt, st));
        }
        if ((rc = enqueue_row_scan(w, d_pcnt, n_tok + 1, d_prank, d_total + 5, a.p_tot + 3, d_err + 1, st))) return rc;
        int32_t* ids = a.ids;
        int64_t cap = a.cap;
        if (a.padded) {
            if ((rc = second_sized_total(w, a.h_tot, 3, st, nullptr, &cap))) return rc;   // wait 2 (padded form): the piece total sizes the ids
            if (cap >= (1ll << 31)) return LATOK_OK;   // (the caller refuses it)
            if ((rc = ws_ensure(ws_needs(w, total, WsShape{.spans = true, .term_rows = n_str + 1, .wp_tokens = n_tok, .wp_pieces = cap,
                                                              .bpe_tokens = a.cut.bpe ? n_tok : 0, .uni_tokens = a.cut.uni ? n_tok : 0}).data(),
                                kWsNeeds)))
                return rc;
            ids = (int32_t*)w.wpids.p;
            d_ids = ids;
        }
        if (ids && spm) HIP_TRY(latok::launch_spbpe_emit(a.o32, text, spt, a.unk, d_prank, d_mask, d_total + 5, cap, ids, a.spans, st));
        else if (ids && a.cut.bpe) HIP_TRY(latok::launch_bpe_emit(a.o32, text, bt, a.unk, d_prank, d_mask, d_total + 5, cap, ids, a.spans, st));
        else if (ids && a.cut.uni) HIP_TRY(latok::launch_uni_emit(a.o32, text, ut, a.unk, d_prank, d_marks, d_total + 5, cap, ids, a.spans, st));
        else if (ids) HIP_TRY(latok::launch_wp_emit(a.o32, text, wt, a.unk, d_prank, d_total + 5, cap, ids, a.spans, st));
        if (a.indptr) HIP_TRY(latok::launch_wp_rows(a.o32, d_start, d_prank, n_str, n_tok, a.indptr, st));
    } else if (a.indptr) {
        HIP_TRY(hipMemsetAsync(a.indptr, 0, (size_t)(n_str + 1) * (a.o32 ? 4 : 8), st));   // (no token: every row is empty)
    }
    if (a.padded)
        HIP_TRY(latok::launch_wp_pad(d_ids, d_start, n_tok > 0 ? d_prank : nullptr, n_str, n_tok, a.max_length, a.add_special, a.cls_id, a.sep_id, a.pad_id,
                                     a.input_ids, a.lengths, st));
    return LATOK_OK;
}
// the body of latok_wordpiece_ids_utf8_bytes_batch and latok_bpe_ids_utf8_bytes_batch; Handle / Obj: the object's two types
extern "C++" template <class Obj, class Handle>
static int piece_ids_call(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes, const Handle* handle,
                          const char* null_msg, PieceCut cut, const Obj* PieceCut::*slot, int32_t unk_id, int64_t* indptr_out, int32_t* ids_out,
                          int64_t* spans_out, int64_t cap, int64_t* n_pieces_out, int64_t* n_tokens_out, int flags, void* stream) {
    LATOK_ENTER();
    if (flags & ~(LATOK_OUT_INT32 | LATOK_DEVICE_PTRS)) return fail(LATOK_ERR_INVALID, "unknown flag");
    int rc = need_init(g);
    if (rc) return rc;
    if (!n_pieces_out) return fail(LATOK_ERR_INVALID, "the total-size output pointer is NULL");
    *n_pieces_out = 0;
    if (n_tokens_out) *n_tokens_out = 0;
    if (!indptr_out) return fail(LATOK_ERR_INVALID, "indptr_out is NULL");
    if (cap < 0) return fail(LATOK_ERR_INVALID, "negative capacity");
    if (!ids_out && cap > 0) return fail(LATOK_ERR_INVALID, "ids_out is NULL but cap > 0 (a size query passes cap = 0)");
    const Obj* v = nullptr;
    if ((rc = check_object(g, handle, null_msg, &v))) return rc;
    cut.*slot = v;
    cut.route_by_front();
    BytesCall c;   // (elt: the width of indptr and of one field of a span; an id is 4 bytes in every mode)
    if ((rc = c.open(g, utf8, byte_off, n_str, total_bytes, flags, stream))) return rc;
    const bool dev = c.dev;
    const size_t elt = c.elt;
    if (dev && ((uintptr_t)indptr_out & (elt - 1)) != 0) return fail(LATOK_ERR_INVALID, "misaligned output buffer");
    if (c.empty) return zero_counts(dev, indptr_out, (size_t)(n_str + 1) * elt, c.st, true);   // no byte, no piece
    if (dev && (((uintptr_t)spans_out & (2 * elt - 1)) != 0 || ((uintptr_t)ids_out & 3) != 0)) return fail(LATOK_ERR_INVALID, "misaligned output buffer");
    if ((rc = c.stage(g, cut.route_ids, WsShape{.spans = true, .term_rows = n_str + 1}, kClearSized))) return rc;
    WordPieceCall a;
    a.b = c.d;
    a.cut = cut;
    a.unk = unk_id;
    a.indptr = indptr_out;
    a.ids = ids_out;
    a.spans = ids_out ? spans_out : nullptr;
    // (a piece has at least one byte -- but for the marker-alone piece of a Unigram token, one per token at most: a larger capacity
    // gates nothing, and the staging is sized by it; 2^31 pieces or more are refused)
    // (SentencePiece BPE: byte fallback of a marker gives three pieces for one space and three for the dummy)
    const int64_t most = cut.pretok() == kPretokSpm ? 3 * (c.total + n_str) : cut.uni ? 2 * c.total : c.total;
    a.cap = ids_out ? std::min({cap, most, (int64_t)0x7FFFFFFF}) : 0;
    a.o32 = c.o32;
    if (!dev) {
        if ((rc = g.h_aux.ensure((size_t)a.cap * 4 + 16)) || (rc = g.h_out.ensure((size_t)a.cap * 2 * elt + 16)) || (rc = g.counts.ensure((size_t)(n_str + 1) * 8)))
            return rc;
        if (ids_out) a.ids = (int32_t*)g.h_aux.p;
        if (a.spans) a.spans = g.h_out.p;
        a.indptr = g.counts.p;
    }
    a.p_tot = c.p_tot;
    a.h_tot = c.h_tot;
    a.st = c.st;
    if ((rc = enqueue_wordpiece(g, g.ws, a))) return rc;
    if (!dev) HIP_TRY(hipMemcpyAsync(indptr_out, a.indptr, (size_t)(n_str + 1) * elt, hipMemcpyDeviceToHost, c.st));   // valid whatever the capacity
    int64_t n_tok = 0;
    if ((rc = c.wait_totals(g, 0, &n_tok))) return rc;   // wait 2
    if (n_tokens_out) *n_tokens_out = n_tok;
    const int64_t n = c.h_tot[3];
    *n_pieces_out = n;
    if (n >= (1ll << 31)) return fail(LATOK_ERR_INVALID, "the batch has %lld pieces: a call takes fewer than 2^31", (long long)n);
    return deliver_sized(c, n, cap, "capacity too small: need %lld pieces", {{ids_out, a.ids, 4}, {spans_out, a.spans, 2 * elt}});   // (wait 3)
}
int latok_wordpiece_ids_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes,
                                         const latok_wordpiece* wp, int32_t unk_id, int64_t* indptr_out, int32_t* ids_out, int64_t* spans_out,
                                         int64_t cap, int64_t* n_pieces_out, int64_t* n_tokens_out, int flags, void* stream) {
    return piece_ids_call(utf8, byte_off, n_str, total_bytes, wp, "wp is NULL", PieceCut{}, &PieceCut::wp, unk_id, indptr_out, ids_out, spans_out, cap,
                          n_pieces_out, n_tokens_out, flags, stream);
}
int latok_bpe_ids_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes, const latok_bpe* bpe,
                                   int32_t unk_id, int64_t* indptr_out, int32_t* ids_out, int64_t* spans_out, int64_t cap, int64_t* n_pieces_out,
                                   int64_t* n_tokens_out, int flags, void* stream) {
    return piece_ids_call(utf8, byte_off, n_str, total_bytes, bpe, "bpe is NULL", PieceCut{.route_ids = 18, .route_padded = 19}, &PieceCut::bpe, unk_id, indptr_out,
                          ids_out, spans_out, cap, n_pieces_out, n_tokens_out, flags, stream);
}
int latok_unigram_ids_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes, const latok_unigram* uni,
                                       int32_t unk_id, int64_t* indptr_out, int32_t* ids_out, int64_t* spans_out, int64_t cap, int64_t* n_pieces_out,
                                       int64_t* n_tokens_out, int flags, void* stream) {
    return piece_ids_call(utf8, byte_off, n_str, total_bytes, uni, "uni is NULL", PieceCut{.route_ids = 22, .route_padded = 23}, &PieceCut::uni, unk_id, indptr_out,
                          ids_out, spans_out, cap, n_pieces_out, n_tokens_out, flags, stream);
}

// the body of the two padded forms; cls_id / sep_id: BOS / EOS of the BPE call
extern "C++" template <class Obj, class Handle>
static int piece_padded_call(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes, const Handle* handle,
                             const char* null_msg, PieceCut cut, const Obj* PieceCut::*slot, int32_t unk_id, int64_t max_length, int add_special,
                             int32_t cls_id, int32_t sep_id, int32_t pad_id, int32_t* input_ids_out, int32_t* lengths_out, int64_t* n_pieces_out,
                             int flags, void* stream) {
    LATOK_ENTER();
    if (flags & ~(LATOK_OUT_INT32 | LATOK_DEVICE_PTRS)) return fail(LATOK_ERR_INVALID, "unknown flag");
    int rc = need_init(g);
    if (rc) return rc;
    if (n_pieces_out) *n_pieces_out = 0;
    const int sp = add_special ? 1 : 0;
    if (max_length < 1 + 2 * sp || max_length > 0x7FFFFFFF) return fail(LATOK_ERR_INVALID, "max_length must be in %d .. 2^31 - 1", 1 + 2 * sp);
    const Obj* v = nullptr;
    if ((rc = check_object(g, handle, null_msg, &v))) return rc;
    cut.*slot = v;
    cut.route_by_front();
    BytesCall c;
    if ((rc = c.open(g, utf8, byte_off, n_str, total_bytes, flags, stream))) return rc;
    const bool dev = c.dev;
    const hipStream_t st = c.st;
    if (n_str == 0) return LATOK_OK;
    if (n_str > (1ll << 40) / max_length) return fail(LATOK_ERR_INVALID, "n_str * max_length must not exceed 2^40");
    if (!input_ids_out || !lengths_out) return fail(LATOK_ERR_INVALID, "NULL buffer");
    if (dev && ((((uintptr_t)input_ids_out | (uintptr_t)lengths_out) & 3) != 0)) return fail(LATOK_ERR_INVALID, "misaligned output buffer");
    const size_t cells = (size_t)n_str * (size_t)max_length;
    int32_t* d_block = input_ids_out;
    int32_t* d_len = lengths_out;
    if (!dev) {
        if ((rc = g.h_out.ensure(cells * 4 + 16)) || (rc = g.counts.ensure((size_t)(n_str + 1) * 8))) return rc;
        d_block = (int32_t*)g.h_out.p;
        d_len = (int32_t*)g.counts.p;
    }
    if (c.empty) {   // no byte, no piece: every row is its specials and padding
        g.last_route = cut.route_padded;
        HIP_TRY(latok::launch_wp_pad(nullptr, nullptr, nullptr, n_str, 0, max_length, sp, cls_id, sep_id, pad_id, d_block, d_len, st));
    } else {
        if ((rc = c.stage(g, cut.route_padded, WsShape{.spans = true, .term_rows = n_str + 1}, kClearSized))) return rc;
        WordPieceCall a;
        a.b = c.d;
        a.cut = cut;
        a.unk = unk_id;
        a.padded = true;
        a.max_length = max_length;
        a.add_special = sp;
        a.cls_id = cls_id;
        a.sep_id = sep_id;
        a.pad_id = pad_id;
        a.input_ids = d_block;
        a.lengths = d_len;
        a.p_tot = c.p_tot;
        a.h_tot = c.h_tot;
        a.st = st;
        if ((rc = enqueue_wordpiece(g, g.ws, a))) return rc;
        const int64_t n = c.h_tot[3];   // (read behind wait 2 of the padded form; 0 when the batch has no token)
        if (n_pieces_out) *n_pieces_out = n;
        if (n >= (1ll << 31)) return fail(LATOK_ERR_INVALID, "the batch has %lld pieces: a call takes fewer than 2^31", (long long)n);
    }
    if (!dev) {
        HIP_TRY(hipMemcpyAsync(input_ids_out, d_block, cells * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(lengths_out, d_len, (size_t)n_str * 4, hipMemcpyDeviceToHost, st));
    }
    int64_t n_tok = 0;
    if (!c.empty) return c.wait_totals(g, 0, &n_tok);   // the last wait
    HIP_TRY(hipStreamSynchronize(st));
    return LATOK_OK;
}
int latok_wordpiece_padded_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes,
                                            const latok_wordpiece* wp, int32_t unk_id, int64_t max_length, int add_special, int32_t cls_id,
                                            int32_t sep_id, int32_t pad_id, int32_t* input_ids_out, int32_t* lengths_out, int64_t* n_pieces_out,
                                            int flags, void* stream) {
    return piece_padded_call(utf8, byte_off, n_str, total_bytes, wp, "wp is NULL", PieceCut{}, &PieceCut::wp, unk_id, max_length, add_special, cls_id,
                             sep_id, pad_id, input_ids_out, lengths_out, n_pieces_out, flags, stream);
}
int latok_bpe_padded_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes, const latok_bpe* bpe,
                                      int32_t unk_id, int64_t max_length, int add_special, int32_t bos_id, int32_t eos_id, int32_t pad_id,
                                      int32_t* input_ids_out, int32_t* lengths_out, int64_t* n_pieces_out, int flags, void* stream) {
    return piece_padded_call(utf8, byte_off, n_str, total_bytes, bpe, "bpe is NULL", PieceCut{.route_ids = 18, .route_padded = 19}, &PieceCut::bpe, unk_id, max_length,
                             add_special, bos_id, eos_id, pad_id, input_ids_out, lengths_out, n_pieces_out, flags, stream);
}
int latok_unigram_padded_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes, const latok_unigram* uni,
                                          int32_t unk_id, int64_t max_length, int add_special, int32_t bos_id, int32_t eos_id, int32_t pad_id,
                                          int32_t* input_ids_out, int32_t* lengths_out, int64_t* n_pieces_out, int flags, void* stream) {
    return piece_padded_call(utf8, byte_off, n_str, total_bytes, uni, "uni is NULL", PieceCut{.route_ids = 22, .route_padded = 23}, &PieceCut::uni, unk_id, max_length,
                             add_special, bos_id, eos_id, pad_id, input_ids_out, lengths_out, n_pieces_out, flags, stream);
}

/* Decoding (latok_detok_create / _destroy / _info, latok_detok_csr, latok_detok_padded; detok_kernels.hip, detok.h): ids back to bytes.
 * The object holds the blob, the entry records and the id map of detok.h, built on the host, uploaded once, read only afterwards.  One
 * stream, every batch size the same kernels:
 *   k_csr_check / k_detok_lengths    the caller's rows; what fails sets the error word, and every kernel behind it returns at once
 *   k_detok_widen                    an int32 indptr as int64 row starts
 *   k_detok_count                    output bytes per piece, per workgroup of pieces; the unknown ids
 *   k_scan_chained                   each workgroup's first output byte; THE byte total -> scalar word 0, pinned word 0
 *   device pointers:  k_detok_write (gate: total <= capacity), then the call's one wait: total, error word, unknown tally
 *   host pointers:    the wait for the same three words, which sizes the staging; k_detok_write into it; the copies and a second wait
 * `w` is sized by ws_needs with WsShape{.tf_ctl, .tf_ptr_bytes, .tf_entries (host staging), .dt_cells, .dt_rows}. */
struct Detok {                     // latok_detok: immutable once created
    int device = -1;
    int64_t n_words = 0, n_ids = 0;
    uint64_t blob_bytes = 0;
    uint32_t max_len = 0;
    int mode = 0;
    uint32_t sep = 0;
    DtMap map{0, 0, 0};
    DevMem blob, entries, keys, vals;
    latok::DetokTable view() const {
        latok::DetokTable t;
        t.blob = blob.as<const uint32_t>();
        t.entries = entries.p;
        t.keys = keys.as<const int32_t>();
        t.vals = vals.as<const int32_t>();
        t.map = map;
        t.mode = mode;
        t.sep = sep;
        return t;
    }
};
int latok_detok_create(const uint8_t* words, const int64_t* word_off, int64_t n_words, const int32_t* word_ids, int mode, const uint8_t* prefix,
                       int prefix_len, int sep, latok_detok** out) {
    LATOK_ENTER();
    // what needs no device is refused first
    if (!out) return fail(LATOK_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (mode != LATOK_DETOK_CONCAT && mode != LATOK_DETOK_WORDPIECE) return fail(LATOK_ERR_INVALID, "mode must be LATOK_DETOK_CONCAT or LATOK_DETOK_WORDPIECE");
    if (prefix_len < 0 || prefix_len > kDtMaxPrefix) return fail(LATOK_ERR_INVALID, "prefix_len must be in 0 .. %d", kDtMaxPrefix);
    if (prefix_len > 0 && !prefix) return fail(LATOK_ERR_INVALID, "prefix is NULL");
    if (sep < 0 || sep > 255) return fail(LATOK_ERR_INVALID, "sep must be one byte (0 .. 255)");
    if (mode == LATOK_DETOK_CONCAT && (prefix_len != 0 || sep != 0)) return fail(LATOK_ERR_INVALID, "LATOK_DETOK_CONCAT takes prefix_len = 0 and sep = 0");
    int rc = check_word_list(words, word_off, n_words);
    if (rc || (rc = need_init(g))) return rc;
    DtTable t;
    Detok* v = nullptr;
    try {
        dt_build(words, word_off, n_words, word_ids, mode, prefix, prefix_len, &t);
        v = new Detok();
    } catch (const std::bad_alloc&) {
        return fail(LATOK_ERR_NOMEM, "out of host memory");
    }
    v->device = g.device;
    v->n_words = n_words;
    v->n_ids = t.n_ids;
    v->blob_bytes = t.blob_bytes;
    v->max_len = t.max_len;
    v->mode = mode;
    v->sep = (uint32_t)sep;
    v->map = t.map;
    const size_t bytes[4] = {t.blob.size() * 4, t.entries.size() * sizeof(DtEntry), t.keys.size() * 4, t.vals.size() * 4};
    const void* src[4] = {t.blob.data(), t.entries.data(), t.keys.data(), t.vals.data()};
    DevMem* dst[4] = {&v->blob, &v->entries, &v->keys, &v->vals};
    for (int i = 0; i < 4 && !rc; ++i) {
        hipError_t e = dst[i]->alloc(bytes[i]);
        if (e != hipSuccess) rc = fail(LATOK_ERR_NOMEM, "hipMalloc(%zu) failed: %s", bytes[i], hipGetErrorString(e));
        else if ((e = hipMemcpyAsync(dst[i]->p, src[i], bytes[i], hipMemcpyHostToDevice, g.stream)) != hipSuccess)
            rc = fail(LATOK_ERR_HIP, "uploading the decoder failed: %s", hipGetErrorString(e));
    }
    const hipError_t e = hipStreamSynchronize(g.stream);   // (the host table dies with this call, and every context may use the object at once)
    if (!rc && e != hipSuccess) rc = fail(LATOK_ERR_HIP, "uploading the decoder failed: %s", hipGetErrorString(e));
    if (rc) {
        delete v;
        return rc;
    }
    *out = reinterpret_cast<latok_detok*>(v);
    return LATOK_OK;
}
int latok_detok_destroy(latok_detok* d) {
    LATOK_ENTER();
    return destroy_object(g, reinterpret_cast<Detok*>(d));
}
int latok_detok_info(const latok_detok* d, int64_t* n_words, int64_t* n_ids, int64_t* blob_bytes, int64_t* max_len, int* mode, int* dense, int* device) {
    const Detok* v = reinterpret_cast<const Detok*>(d);
    if (!v) return fail(LATOK_ERR_INVALID, "detok is NULL");
    if (n_words) *n_words = v->n_words;
    if (n_ids) *n_ids = v->n_ids;
    if (blob_bytes) *blob_bytes = (int64_t)v->blob_bytes;
    if (max_len) *max_len = v->max_len;
    if (mode) *mode = v->mode;
    if (dense) *dense = v->map.dense;
    if (device) *device = v->device;
    return LATOK_OK;
}

struct DetokCall {                 // what an entry point of the pair received
    const latok_detok* handle = nullptr;
    bool padded = false;
    const void* rows = nullptr;    // CSR: indptr; padded: lengths (may be NULL)
    const int32_t* ids = nullptr;
    int64_t n_rows = 0, n_pieces = 0, max_length = 0;
    const int32_t* skip = nullptr;
    int n_skip = 0;
    uint8_t* out = nullptr;
    int64_t cap = 0;
    int64_t* out_off = nullptr;
    int64_t* n_out = nullptr;
    int64_t* n_unknown = nullptr;
    int flags = 0;
    void* stream = nullptr;
};
static int detok_refusal(int err) {
    if (err & latok::kDetokBadLength) return fail(LATOK_ERR_INVALID, "a length lies outside [0, max_length]");
    return csr_refusal(err);
}
static int detok_common(const DetokCall& a) {
    LATOK_ENTER();
    int rc;
    if (a.flags & ~(LATOK_OUT_INT32 | LATOK_DEVICE_PTRS)) return fail(LATOK_ERR_INVALID, "unknown flag");
    if (!a.n_out) return fail(LATOK_ERR_INVALID, "the total-size output pointer is NULL");
    *a.n_out = 0;
    if (a.n_unknown) *a.n_unknown = 0;
    if (a.n_skip < 0 || a.n_skip > kDtMaxSkip) return fail(LATOK_ERR_INVALID, "n_skip must be in 0 .. %d", kDtMaxSkip);
    if (a.n_skip > 0 && !a.skip) return fail(LATOK_ERR_INVALID, "skip_ids is NULL");
    if (a.cap < 0) return fail(LATOK_ERR_INVALID, "negative capacity");
    if (!a.out && a.cap > 0) return fail(LATOK_ERR_INVALID, "out_bytes is NULL but out_cap > 0 (a size query passes out_cap = 0)");
    int64_t n_cells = a.n_pieces;
    if (a.padded) {
        if (a.n_rows < 0) return fail(LATOK_ERR_INVALID, "n_rows must be >= 0");
        if (a.max_length < 0) return fail(LATOK_ERR_INVALID, "max_length must be >= 0");
        if (a.max_length > 0 && a.n_rows > (int64_t)((1ull << 62) / (uint64_t)a.max_length)) return fail(LATOK_ERR_INVALID, "n_rows * max_length is too large");
        n_cells = a.n_rows * a.max_length;
        if (n_cells > 0 && !a.ids) return fail(LATOK_ERR_INVALID, "input_ids is NULL");
    } else if ((rc = csr_args(a.rows, a.ids, a.n_rows, a.n_pieces, a.flags))) {
        return rc;
    }
    if (a.n_rows > 0 && !a.out_off) return fail(LATOK_ERR_INVALID, "out_off is NULL");
    if ((rc = need_init(g))) return rc;
    const Detok* v = nullptr;
    if ((rc = check_object(g, a.handle, "detok is NULL", &v))) return rc;
    const bool dev = (a.flags & LATOK_DEVICE_PTRS) != 0, o32 = !a.padded && (a.flags & LATOK_OUT_INT32) != 0;
    const size_t elt = a.padded || o32 ? 4 : 8;   // width of one entry of `rows`
    if (dev && (((uintptr_t)a.rows & (elt - 1)) != 0 || ((uintptr_t)a.ids & 3) != 0 || ((uintptr_t)a.out_off & 7) != 0))
        return fail(LATOK_ERR_INVALID, "misaligned buffer");
    StreamTurn turn(g, a.stream);
    const hipStream_t st = turn.st;
    if (a.n_rows == 0) return zero_counts(dev, a.out_off, 8, st, true);   // no row: the one offset, if the caller has room for it
    Workspace& w = g.ws;
    const int64_t n_rows = a.n_rows;
    const size_t rows_bytes = a.rows ? (size_t)(a.padded ? n_rows : n_rows + 1) * elt : 0;
    WsShape shape;
    shape.tf_ctl = true;
    shape.dt_cells = n_cells;
    shape.dt_rows = o32 ? n_rows + 1 : 0;
    if (!dev) {
        shape.tf_ptr_bytes = (int64_t)rows_bytes;
        shape.tf_entries = n_cells;
    }
    if ((rc = ws_ensure(ws_needs(w, 0, shape).data(), kWsNeeds)) || (rc = g.pin_tot.ensure(64))) return rc;
    g.last_route = a.padded ? 21 : 20;
    const void* d_rows = a.rows;
    const int32_t* d_ids = a.ids;
    if (!dev) {
        if (rows_bytes > 0) {
            HIP_TRY(hipMemcpyAsync(w.tfptr.p, a.rows, rows_bytes, hipMemcpyHostToDevice, st));
            d_rows = w.tfptr.p;
        }
        if (n_cells > 0) {
            HIP_TRY(hipMemcpyAsync(w.tfidx.p, a.ids, (size_t)n_cells * 4, hipMemcpyHostToDevice, st));
            d_ids = (const int32_t*)w.tfidx.p;
        }
    }
    // the control words: the error word of the row checks, the unknown tally; copied into the pinned words 5 and 6 in front of the wait
    int* d_err = (int*)w.tfctl.p;
    unsigned long long* d_unk = (unsigned long long*)w.tfctl.p + 1;
    HIP_TRY(hipMemsetAsync(d_err, 0, 16, st));
    volatile int64_t* h_tot = (volatile int64_t*)g.pin_tot.h;
    int64_t* p_tot = (int64_t*)g.pin_tot.d;
    h_tot[0] = h_tot[1] = h_tot[5] = h_tot[6] = 0;
    latok::DetokRows R{nullptr, nullptr, n_rows, a.max_length, n_cells};
    if (a.padded) {
        R.lengths = (const int32_t*)d_rows;
        HIP_TRY(latok::launch_detok_lengths(R.lengths, n_rows, a.max_length, d_err, st));
    } else {
        HIP_TRY(latok::launch_csr_check(o32, d_rows, d_ids, n_rows, n_cells, nullptr, 0, 0, d_err, st));
        R.row_start = (const int64_t*)d_rows;
        if (o32) {
            HIP_TRY(latok::launch_detok_widen((const int32_t*)d_rows, n_rows + 1, (int64_t*)w.dtrows.p, st));
            R.row_start = (const int64_t*)w.dtrows.p;
        }
    }
    latok::DetokSkip S;
    for (int i = 0; i < kDtMaxSkip; ++i) S.id[i] = i < a.n_skip ? a.skip[i] : 0;
    S.n = a.n_skip;
    const latok::DetokTable T = v->view();
    uint32_t* d_cnt = (uint32_t*)w.dtcnt.p;
    int64_t* d_sum = (int64_t*)w.dtsum.p;
    int64_t* d_rank = (int64_t*)w.dtrank.p;
    int64_t* d_total = (int64_t*)w.scalar.p;
    if (n_cells > 0) {
        latok::ChainState chain;
        if ((rc = next_scan_epoch(w, st, &chain))) return rc;
        HIP_TRY(latok::launch_detok_count(T, R, d_ids, S, d_err, d_cnt, d_sum, d_unk, st));
        HIP_TRY(latok::launch_tile_scan(d_sum, latok::detok_groups(n_cells), d_rank, chain, d_total, p_tot, (int*)(p_tot + 1) + 1, st));
        if (dev) HIP_TRY(latok::launch_detok_write(T, R, d_ids, S, d_err, d_cnt, d_rank, d_total, a.out, a.cap, a.out_off, st));
    }
    HIP_TRY(hipMemcpyAsync((void*)(h_tot + 5), d_err, 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));   // the call's wait for the totals
    if ((rc = detok_refusal((int)h_tot[5]))) return rc;   // (a refused call has written nothing: the kernels behind the check returned at once)
    int64_t n = 0;
    if ((rc = finish_totals(w, h_tot, 0, &n))) return rc;
    *a.n_out = n;
    if (a.n_unknown) *a.n_unknown = h_tot[6];
    if (n_cells == 0) return zero_counts(dev, a.out_off, (size_t)(n_rows + 1) * 8, st, true);   // no piece: empty rows
    if (!dev) {   // the staging is sized by the total; out_off is valid whatever the capacity
        const bool fits = a.out && n <= a.cap;
        if ((rc = g.h_aux.ensure((size_t)(n_rows + 1) * 8)) || (fits && (rc = g.h_out.ensure((size_t)n + 16)))) return rc;
        uint8_t* d_out = fits ? (uint8_t*)g.h_out.p : nullptr;
        HIP_TRY(latok::launch_detok_write(T, R, d_ids, S, d_err, d_cnt, d_rank, d_total, d_out, n, (int64_t*)g.h_aux.p, st));
        HIP_TRY(hipMemcpyAsync(a.out_off, g.h_aux.p, (size_t)(n_rows + 1) * 8, hipMemcpyDeviceToHost, st));
        if (fits && n > 0) HIP_TRY(hipMemcpyAsync(a.out, d_out, (size_t)n, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    if (n > a.cap) return fail(LATOK_ERR_INVALID, "output capacity too small: need %lld bytes", (long long)n);
    return LATOK_OK;
}
int latok_detok_csr(const latok_detok* d, const void* indptr, const int32_t* ids, int64_t n_rows, int64_t n_pieces, const int32_t* skip_ids, int n_skip,
                    uint8_t* out_bytes, int64_t out_cap, int64_t* out_off, int64_t* n_out_bytes, int64_t* n_unknown_out, int flags, void* stream) {
    DetokCall a;
    a.handle = d;
    a.rows = indptr;
    a.ids = ids;
    a.n_rows = n_rows;
    a.n_pieces = n_pieces;
    a.skip = skip_ids;
    a.n_skip = n_skip;
    a.out = out_bytes;
    a.cap = out_cap;
    a.out_off = out_off;
    a.n_out = n_out_bytes;
    a.n_unknown = n_unknown_out;
    a.flags = flags;
    a.stream = stream;
    return detok_common(a);
}
int latok_detok_padded(const latok_detok* d, const int32_t* input_ids, const int32_t* lengths, int64_t n_rows, int64_t max_length,
                       const int32_t* skip_ids, int n_skip, uint8_t* out_bytes, int64_t out_cap, int64_t* out_off, int64_t* n_out_bytes,
                       int64_t* n_unknown_out, int flags, void* stream) {
    DetokCall a;
    a.handle = d;
    a.padded = true;
    a.rows = lengths;
    a.ids = input_ids;
    a.n_rows = n_rows;
    a.max_length = max_length;
    a.skip = skip_ids;
    a.n_skip = n_skip;
    a.out = out_bytes;
    a.cap = out_cap;
    a.out_off = out_off;
    a.n_out = n_out_bytes;
    a.n_unknown = n_unknown_out;
    a.flags = flags;
    a.stream = stream;
    return detok_common(a);
}
/* test hook (not part of the ABI; needs no device): the constants of the decode calls: out[0] = kDetokBlock (pieces per workgroup of
 * k_detok_count / k_detok_write), out[1] = kDetokWin (bytes of the LDS window), out[2] = kDtDenseSpread (the map is dense when the id
 * range is at most this many times the word count), out[3] = entries per workgroup of the chained scan over the workgroup sums, out[4] =
 * kDetokLaneBytes (the longest stretch a lane copies into a window itself).  Returns the number of values written. */
extern "C" int latok_debug_detok_limits(int64_t* out, int n) {
    const int64_t v[5] = {latok::kDetokBlock, latok::kDetokWin, kDtDenseSpread, latok::scan_chunk(), latok::kDetokLaneBytes};
    if (!out || n < 0) return fail(LATOK_ERR_INVALID, "NULL output");
    const int k = n < 5 ? n : 5;
    for (int i = 0; i < k; ++i) out[i] = v[i];
    return k;
}

/* token counting in byte space: a mutable, exact counting table on the device (count_table.h), filled by k_count_scatter and made
 * independent of the caller's text by the two commit launches before the call returns.  One stream:
 *   tile index -> byte-space tiles -> resolve     boundary mask, smeared SPACE plane over the BYTES
 *   k_word_counts + k_scan_chained                kept mask, token ranks; THE token total -> scalar word 0, pinned word 0
 *   k_count_scatter                               every token found or entered (fresh slots point into the text), counted
 *   k_count_commit_sum                            padded dwords of the fresh slots; the host waits, reads, grows the blob if needed
 *   k_count_commit_copy                           fresh words into the blob, resident slot words
 * `w` is sized by ws_needs with WsShape{.spans = true}: the spans shape, no buffer beyond it. */
struct Counter {                   // latok_counter: mutable; calls on it are serialised by its own lock
    std::mutex mu;
    int device = -1;
    int64_t max_words = 0;
    uint64_t n_slots = 0;
    int max_word_bytes = 0;
    uint32_t seed = 0;
    DevMem slots;                  // uint64[n_slots]
    DevMem counts;                 // uint64[n_slots]
    DevMem blob;                   // uint32[blob_dwords]; dword 0 is reserved
    uint64_t blob_dwords = 0;
    uint64_t cursor = 1;           // dwords of the blob in use
    DevMem ctl;                    // uint64[8]: {counted, long, dropped, -, fresh dwords, cursor, distinct, overflow}
    int64_t totals[4] = {0, 0, 0, 0};   // tokens, counted, long, dropped over all updates
    int64_t distinct = 0;
    int64_t grown = 0;             // times the blob was reallocated (latok_debug_counter_state)
    bool failed = false;           // a call ended between k_count_scatter and the end of its commit: fresh slots may remain
};
static latok::CountTable count_table_of(const Counter& c) {
    latok::CountTable t;
    t.slots = c.slots.as<uint64_t>();
    t.counts = c.counts.as<unsigned long long>();
    t.blob = c.blob.as<uint32_t>();
    t.blob_dwords = c.blob_dwords;
    t.n_slots = c.n_slots;
    t.seed = c.seed;
    t.max_word_bytes = c.max_word_bytes;
    t.tally = c.ctl.as<unsigned long long>();
    t.ctl = c.ctl.as<unsigned long long>() + 4;
    return t;
}
// empty table, empty blob, zero totals (the device part on `st`, waited for)
static int counter_reset(Counter& c, hipStream_t st) {
    const uint64_t ctl[8] = {0, 0, 0, 0, 0, 1, 0, 0};
    HIP_TRY(hipMemsetAsync(c.slots.p, 0, c.n_slots * 8, st));
    HIP_TRY(hipMemsetAsync(c.counts.p, 0, c.n_slots * 8, st));
    HIP_TRY(hipMemsetAsync(c.blob.p, 0, 4, st));
    HIP_TRY(hipMemcpyAsync(c.ctl.p, ctl, sizeof(ctl), hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    c.cursor = 1;
    c.distinct = 0;
    for (int64_t& t : c.totals) t = 0;
    c.failed = false;
    return LATOK_OK;
}

int latok_counter_create(int64_t max_words, int max_word_bytes, uint32_t seed, latok_counter** out) {
    LATOK_ENTER();
    // what needs no device is refused first
    if (!out) return fail(LATOK_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (max_words < 1 || max_words > (1ll << 30)) return fail(LATOK_ERR_INVALID, "max_words must be in 1 .. 2^30");
    if (max_word_bytes < 1 || max_word_bytes > latok::kHashWaveBytes)
        return fail(LATOK_ERR_INVALID, "max_word_bytes must be in 1 .. %d", latok::kHashWaveBytes);
    static_assert(latok::kHashWaveBytes <= kCtMaxWordBytes, "a slot word holds length - 1 in 8 bits");
    int rc = need_init(g);
    if (rc) return rc;
    Counter* c = nullptr;
    try {
        c = new Counter();
    } catch (const std::bad_alloc&) {
        return fail(LATOK_ERR_NOMEM, "out of host memory");
    }
    c->device = g.device;
    c->max_words = max_words;
    c->n_slots = ct_slot_count(max_words);
    c->max_word_bytes = max_word_bytes;
    c->seed = seed;
    // the blob starts at 8 bytes per word and grows by need (every commit knows its need before it copies)
    c->blob_dwords = std::max<uint64_t>(64, 2 * (uint64_t)max_words);
    hipError_t e = c->slots.alloc(c->n_slots * 8);
    if (e == hipSuccess) e = c->counts.alloc(c->n_slots * 8);
    if (e == hipSuccess) e = c->blob.alloc(c->blob_dwords * 4);
    if (e == hipSuccess) e = c->ctl.alloc(64);
    if (e != hipSuccess) {
        delete c;
        return fail(LATOK_ERR_NOMEM, "hipMalloc of a counter of %lld slots failed: %s", (long long)ct_slot_count(max_words), hipGetErrorString(e));
    }
    if ((rc = counter_reset(*c, g.stream))) {
        delete c;
        return rc;
    }
    *out = reinterpret_cast<latok_counter*>(c);
    return LATOK_OK;
}

int latok_counter_destroy(latok_counter* counter) {
    LATOK_ENTER();
    return destroy_object(g, reinterpret_cast<Counter*>(counter), &Counter::mu);
}

int latok_counter_clear(latok_counter* counter) {
    LATOK_ENTER();
    Counter* c = reinterpret_cast<Counter*>(counter);
    if (!c) return fail(LATOK_ERR_INVALID, "counter is NULL");
    int rc = need_init(g);
    if (rc) return rc;
    std::lock_guard<std::mutex> cl(c->mu);
    if ((rc = check_device(g, "counter", c->device))) return rc;
    return counter_reset(*c, g.stream);
}

int latok_counter_info(const latok_counter* counter, int64_t* max_words, int64_t* n_slots, int* max_word_bytes, uint32_t* seed, int* device,
                       int64_t* stats5) {
    Counter* c = const_cast<Counter*>(reinterpret_cast<const Counter*>(counter));
    if (!c) return fail(LATOK_ERR_INVALID, "counter is NULL");
    std::lock_guard<std::mutex> cl(c->mu);
    if (max_words) *max_words = c->max_words;
    if (n_slots) *n_slots = (int64_t)c->n_slots;
    if (max_word_bytes) *max_word_bytes = c->max_word_bytes;
    if (seed) *seed = c->seed;
    if (device) *device = c->device;
    if (stats5) {
        for (int i = 0; i < 4; ++i) stats5[i] = c->totals[i];
        stats5[4] = c->distinct;
    }
    return LATOK_OK;
}

// everything of an update from k_count_scatter on: a failure in here leaves the counter failed (the caller sets the flag)
static int count_scatter_and_commit(Ctx& g, Workspace& w, Counter& c, const Batch& d, const latok::TokenPlanes& tp, int64_t* p_tot,
                                    const volatile int64_t* h_tot, int64_t* stats4, hipStream_t st) {
    uint64_t ctl[8];
    latok::CountTable t = count_table_of(c);
    HIP_TRY(latok::launch_count_scatter(tp, (const uint8_t*)d.in.p, t, (int*)(p_tot + 1), st));
    HIP_TRY(latok::launch_count_commit_sum(t, st));
    HIP_TRY(hipMemcpyAsync(ctl, c.ctl.p, sizeof(ctl), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));   // the first of the call's two waits: the commit's need is known
    int rc;
    int64_t n = 0;
    if ((rc = finish_totals(w, h_tot, 0, &n))) return rc;
    const uint64_t need = c.cursor + ctl[4];
    if (need >= (1ull << 32)) return fail(LATOK_ERR_NOMEM, "the counter's words would take 2^34 bytes or more");
    if (need > c.blob_dwords) {          // grow: new allocation, device copy, free
        const uint64_t want = std::min<uint64_t>(std::max<uint64_t>(need, 2 * c.blob_dwords), (1ull << 32) - 1);
        DevMem grown;
        hipError_t e = grown.alloc(want * 4);
        if (e != hipSuccess) return fail(LATOK_ERR_NOMEM, "hipMalloc(%llu) failed: %s", (unsigned long long)(want * 4), hipGetErrorString(e));
        e = hipMemcpyAsync(grown.p, c.blob.p, c.cursor * 4, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return fail(LATOK_ERR_HIP, "copying the counter's words failed: %s", hipGetErrorString(e));
        c.blob = std::move(grown);
        c.blob_dwords = want;
        ++c.grown;
        t = count_table_of(c);
    }
    if (ctl[4] > 0) {                    // (no fresh slot: nothing to copy, the table is resident already)
        HIP_TRY(latok::launch_count_commit_copy((const uint8_t*)d.in.p, t, st));
        HIP_TRY(hipMemcpyAsync(ctl, c.ctl.p, sizeof(ctl), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (ctl[7] != 0 || ctl[5] != need) return fail(LATOK_ERR_HIP, "internal: the commit of the counter's words did not add up");
    }
    c.cursor = need;
    c.distinct = (int64_t)ctl[6];
    stats4[0] = n;
    stats4[1] = (int64_t)ctl[0];
    stats4[2] = (int64_t)ctl[1];
    stats4[3] = (int64_t)ctl[2];
    for (int i = 0; i < 4; ++i) c.totals[i] += stats4[i];
    return LATOK_OK;
}

int latok_count_tokens_utf8_bytes_batch(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, int64_t total_bytes, latok_counter* counter,
                                        int64_t* stats4_out, int flags, void* stream) {
    LATOK_ENTER();
    if (flags & ~LATOK_DEVICE_PTRS) return fail(LATOK_ERR_INVALID, "unknown flag (the counting call takes LATOK_DEVICE_PTRS only)");
    Counter* c = reinterpret_cast<Counter*>(counter);
    if (!c) return fail(LATOK_ERR_INVALID, "counter is NULL");
    int rc = need_init(g);
    if (rc) return rc;
    std::lock_guard<std::mutex> cl(c->mu);
    if ((rc = check_device(g, "counter", c->device, c->failed))) return rc;
    BytesCall call;
    if ((rc = call.open(g, utf8, byte_off, n_str, total_bytes, flags, stream))) return rc;
    const hipStream_t st = call.st;
    if (call.total >= kCtMaxTextBytes) return fail(LATOK_ERR_INVALID, "a counting batch must be shorter than 2^39 bytes");
    int64_t stats4[4] = {0, 0, 0, 0};
    if (stats4_out) memcpy(stats4_out, stats4, sizeof(stats4));
    if (call.empty) return LATOK_OK;   // no byte, no token: the counter is untouched
    if ((rc = call.stage(g, 8, WsShape{.spans = true}, kClearPair))) return rc;
    const Batch& d = call.d;
    int64_t* p_tot = call.p_tot;
    Workspace& w = g.ws;
    HIP_TRY(hipMemsetAsync(c->ctl.p, 0, 40, st));                    // this call's tallies and fresh dwords
    HIP_TRY(hipMemsetAsync(c->ctl.as<uint64_t>() + 7, 0, 8, st));      // ... and the overflow flag
    latok::TokenPlanes t;
    if ((rc = enqueue_token_front(g, w, d, p_tot, (int*)(p_tot + 1), st, &t))) return rc;
    // from here to the end of the commit the table may hold slots that point into the caller's text
    if ((rc = count_scatter_and_commit(g, w, *c, d, t, p_tot, call.h_tot, stats4, st))) {
        c->failed = true;
        (void)hipStreamSynchronize(st);   // (nothing of this call is still running when the caller gets its text back)
        return rc;
    }
    if (stats4_out) memcpy(stats4_out, stats4, sizeof(stats4));
    return LATOK_OK;
}

int latok_counter_read(const latok_counter* counter, uint8_t* words_out, int64_t bytes_cap, int64_t* word_off_out, uint64_t* counts_out,
                       int64_t cap, int64_t* n_words_out, int64_t* n_bytes_out) {
    LATOK_ENTER();
    Counter* c = const_cast<Counter*>(reinterpret_cast<const Counter*>(counter));
    if (!c) return fail(LATOK_ERR_INVALID, "counter is NULL");
    if (!n_words_out || !n_bytes_out) return fail(LATOK_ERR_INVALID, "the total-size output pointers are NULL");
    *n_words_out = *n_bytes_out = 0;
    if (cap < 0 || bytes_cap < 0) return fail(LATOK_ERR_INVALID, "negative capacity");
    if (cap > 0 && (!word_off_out || !counts_out)) return fail(LATOK_ERR_INVALID, "word_off_out or counts_out is NULL but cap > 0 (a size query passes cap = 0)");
    if (bytes_cap > 0 && !words_out) return fail(LATOK_ERR_INVALID, "words_out is NULL but bytes_cap > 0");
    int rc = need_init(g);
    if (rc) return rc;
    std::lock_guard<std::mutex> cl(c->mu);
    if ((rc = check_device(g, "counter", c->device, c->failed))) return rc;
    // not a hot path: slots, counts and blob come to the host and are compacted here, in slot order
    std::vector<uint64_t> slots, counts;
    std::vector<uint32_t> blob;
    try {
        slots.resize(c->n_slots);
    } catch (const std::bad_alloc&) {
        return fail(LATOK_ERR_NOMEM, "out of host memory");
    }
    HIP_TRY(hipMemcpyAsync(slots.data(), c->slots.p, c->n_slots * 8, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    int64_t n_words = 0, n_bytes = 0;
    for (const uint64_t v : slots) {
        if (v == kCtEmpty) continue;
        if (ct_is_fresh(v) || ct_pos(v) + ct_padded_dwords(v) > c->cursor) return fail(LATOK_ERR_HIP, "internal: a slot of the counter is not resident");
        ++n_words;
        n_bytes += ct_len(v);
    }
    *n_words_out = n_words;
    *n_bytes_out = n_bytes;
    if (n_words > cap || n_bytes > bytes_cap)
        return fail(LATOK_ERR_INVALID, "capacity too small: need %lld words and %lld bytes", (long long)n_words, (long long)n_bytes);
    if (word_off_out) word_off_out[0] = 0;
    if (n_words == 0) return LATOK_OK;
    try {
        counts.resize(c->n_slots);
        blob.resize(c->cursor);
    } catch (const std::bad_alloc&) {
        return fail(LATOK_ERR_NOMEM, "out of host memory");
    }
    HIP_TRY(hipMemcpyAsync(counts.data(), c->counts.p, c->n_slots * 8, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipMemcpyAsync(blob.data(), c->blob.p, c->cursor * 4, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    int64_t k = 0, at = 0;
    for (uint64_t i = 0; i < c->n_slots; ++i) {
        const uint64_t v = slots[i];
        if (v == kCtEmpty) continue;
        const int64_t len = ct_len(v);
        memcpy(words_out + at, reinterpret_cast<const uint8_t*>(blob.data() + ct_pos(v)), (size_t)len);
        at += len;
        counts_out[k] = counts[i];
        word_off_out[++k] = at;
    }
    return LATOK_OK;
}

/* test hooks (not part of the ABI in include/latok_hip.h): out[0..3] = capacity of the counter's blob in dwords, dwords in use,
 * times the blob was reallocated, 1 if the counter is in the failed state; and: put the counter into the failed state, as an
 * update that did not finish its commit would */
extern "C" int latok_debug_counter_state(const latok_counter* counter, int64_t* out4) {
    Counter* c = const_cast<Counter*>(reinterpret_cast<const Counter*>(counter));
    if (!c || !out4) return fail(LATOK_ERR_INVALID, "NULL argument");
    std::lock_guard<std::mutex> cl(c->mu);
    out4[0] = (int64_t)c->blob_dwords;
    out4[1] = (int64_t)c->cursor;
    out4[2] = c->grown;
    out4[3] = c->failed ? 1 : 0;
    return LATOK_OK;
}
extern "C" int latok_debug_counter_fail(latok_counter* counter) {
    Counter* c = reinterpret_cast<Counter*>(counter);
    if (!c) return fail(LATOK_ERR_INVALID, "counter is NULL");
    std::lock_guard<std::mutex> cl(c->mu);
    c->failed = true;
    return LATOK_OK;
}

/* PEP 393 buffers (the reference's own input, latok.c:53-55,79): fixed-width code units of 1, 2 or 4 bytes */
static int check_kind(int kind) {
    if (kind != 1 && kind != 2 && kind != 4) return fail(LATOK_ERR_INVALID, "kind must be 1 (Latin-1), 2 (UCS-2) or 4 (UCS-4), got %d", kind);
    return LATOK_OK;
}

int latok_split_mask_kind_batch(const void* units, int kind, const int64_t* row_off, int64_t n_str, int64_t total_chars,
                                uint64_t* mask_bits_out, int flags, void* stream) {
    LATOK_ENTER();
    const int rc = check_kind(kind);
    if (rc) return rc;
    return mask_common(g, Input{units, form_of_kind(kind)}, row_off, n_str, total_chars, mask_bits_out, latok::kModeBits, flags, stream);
}

int latok_split_offsets_kind_batch(const void* units, int kind, const int64_t* row_off, int64_t n_str, int64_t total_chars,
                                   int64_t* counts_out, int64_t* offsets_out, int64_t offsets_cap, int64_t* n_offsets_out,
                                   int flags, void* stream) {
    LATOK_ENTER();
    const int rc = check_kind(kind);
    if (rc) return rc;
    return compact_common(g, false, false, Batch{Input{units, form_of_kind(kind)}, row_off, n_str, total_chars}, false, counts_out,
                          offsets_out, nullptr, offsets_cap, n_offsets_out, flags, stream);
}

int latok_token_spans_kind_batch(const void* units, int kind, const int64_t* row_off, int64_t n_str, int64_t total_chars,
                                 int64_t* counts_out, int64_t* spans_out, int64_t spans_cap, int64_t* n_tokens_out,
                                 int flags, void* stream) {
    LATOK_ENTER();
    const int rc = check_kind(kind);
    if (rc) return rc;
    return compact_common(g, true, false, Batch{Input{units, form_of_kind(kind)}, row_off, n_str, total_chars}, false, counts_out,
                          spans_out, nullptr, spans_cap, n_tokens_out, flags, stream);
}

int latok_token_features_kind_batch(const void* units, int kind, const int64_t* row_off, int64_t n_str, int64_t total_chars,
                                    int64_t* counts_out, int64_t* spans4_out, int8_t* features_out, int64_t cap,
                                    int64_t* n_tokens_out, int flags, void* stream) {
    LATOK_ENTER();
    const int rc = check_kind(kind);
    if (rc) return rc;
    if (!features_out && cap > 0) return fail(LATOK_ERR_INVALID, "features_out is NULL");
    return compact_common(g, true, true, Batch{Input{units, form_of_kind(kind)}, row_off, n_str, total_chars}, false, counts_out,
                          spans4_out, features_out, cap, n_tokens_out, flags, stream);
}

int latok_token_features_batch(const uint32_t* cps, const int64_t* row_off, int64_t n_str, int64_t total,
                               int64_t* counts_out, int64_t* spans4_out, int8_t* features_out, int64_t cap,
                               int64_t* n_tokens_out, int flags, void* stream) {
    LATOK_ENTER();
    if (!features_out && cap > 0) return fail(LATOK_ERR_INVALID, "features_out is NULL");
    return compact_common(g, true, true, Batch{Input{cps, Form::Utf32}, row_off, n_str, total}, false, counts_out, spans4_out, features_out,
                          cap, n_tokens_out, flags, stream);
}

int latok_parse_matrix(const uint32_t* cps, int64_t n, int8_t* matrix_out, int flags, void* stream) {
    LATOK_ENTER();
    int rc = need_init(g);
    if (rc) return rc;
    if (n < 0) return fail(LATOK_ERR_INVALID, "n must be >= 0");
    if (n == 0) return LATOK_OK;
    if (!cps || !matrix_out) return fail(LATOK_ERR_INVALID, "NULL buffer");
    StreamTurn turn(g, stream);
    hipStream_t st = turn.st;
    const uint8_t* t1 = (const uint8_t*)g.t1.p;
    const uint8_t* t2 = (const uint8_t*)g.t2cls.p;
    const uint16_t* cw = (const uint16_t*)g.cw.p;
    if (flags & LATOK_DEVICE_PTRS) {
        HIP_TRY(latok::launch_parse_matrix(cps, n, t1, t2, cw, matrix_out, st));
        return LATOK_OK;
    }
    if (n <= latok::kSmallMatrixChars) {
        // one string per call (the reference's pattern): chars and matrix pass through pinned memory, one workgroup, and the
        // call returns when it has seen the kernel's completion word
        const size_t po_out = align16((size_t)n * 4);
        if ((rc = g.pin.ensure(po_out + (size_t)n * LATOK_FEATURE_COUNT + 64))) return rc;
        if ((rc = g.pin_tot.ensure(64))) return rc;
        memcpy(g.pin.h, cps, (size_t)n * 4);
        const unsigned long long seq = ++g.small_seq;
        unsigned long long* d_done = poll_completion() ? (unsigned long long*)g.pin_tot.d + 2 : nullptr;
        HIP_TRY(latok::launch_parse_matrix_small((const uint32_t*)g.pin.d, (int)n, t1, t2, cw, (int8_t*)((char*)g.pin.d + po_out), d_done,
                                                 seq, st));
        if (!(d_done && wait_completion_word((const unsigned long long*)g.pin_tot.h + 2, seq))) HIP_TRY(hipStreamSynchronize(st));
        memcpy(matrix_out, (char*)g.pin.h + po_out, (size_t)n * LATOK_FEATURE_COUNT);
        return LATOK_OK;
    }
    if ((rc = g.h_cps.ensure((size_t)n * 4))) return rc;
    if ((rc = g.h_out.ensure((size_t)n * LATOK_FEATURE_COUNT))) return rc;
    HIP_TRY(hipMemcpyAsync(g.h_cps.p, cps, (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(latok::launch_parse_matrix((const uint32_t*)g.h_cps.p, n, t1, t2, cw, (int8_t*)g.h_out.p, st));
    HIP_TRY(hipMemcpyAsync(matrix_out, g.h_out.p, (size_t)n * LATOK_FEATURE_COUNT, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return LATOK_OK;
}

int latok_combine_matrix_rows(const int8_t* m, int64_t rows, int64_t cols, int64_t stride_r, int64_t stride_c,
                              const int8_t* idx, int idx_ndim, int irows, int icols, int8_t* out, int flags,
                              void* stream) {
    LATOK_ENTER();
    int rc = need_init(g);
    if (rc) return rc;
    if (idx_ndim != 1 && idx_ndim != 2) return fail(LATOK_ERR_INVALID, "must specify 2d numpy array args");
    if (rows < 0 || cols < 0 || irows < 0 || icols < 0) return fail(LATOK_ERR_INVALID, "negative shape");
    if (cols == 0) return LATOK_OK;
    if (!m || !idx || !out) return fail(LATOK_ERR_INVALID, "NULL buffer");
    const int n_idx = idx_ndim == 2 ? irows * icols : icols;
    StreamTurn turn(g, stream);
    hipStream_t st = turn.st;
    if (flags & LATOK_DEVICE_PTRS) {
        HIP_TRY(latok::launch_combine_rows((const uint8_t*)m, stride_r, stride_c, cols, idx, idx_ndim, irows, icols, out, st));
        return LATOK_OK;
    }
    // the reference does not bounds-check idx (latok.c:324-327); we refuse out-of-range rows instead of reading wild
    for (int i = 0; i < n_idx; ++i) {
        const uint8_t r = (uint8_t)idx[i];
        if (r != 255 && (int64_t)r >= rows) return fail(LATOK_ERR_INVALID, "idx value %d out of range for %lld rows", (int)r, (long long)rows);
    }
    if (cols <= latok::kSmallMatrixChars && rows <= 64) {
        // the matrix of one string: gathered straight into pinned memory, one workgroup, completion word (see latok_parse_matrix)
        const size_t n_m = (size_t)rows * (size_t)cols;
        const size_t po_idx = align16(n_m), po_out = po_idx + align16((size_t)n_idx);
        if ((rc = g.pin.ensure(po_out + (size_t)cols + 64))) return rc;
        if ((rc = g.pin_tot.ensure(64))) return rc;
        int8_t* hm = (int8_t*)g.pin.h;
        for (int64_t r = 0; r < rows; ++r)
            for (int64_t c = 0; c < cols; ++c) hm[(size_t)(r * cols + c)] = m[r * stride_r + c * stride_c];
        if (n_idx) memcpy((char*)g.pin.h + po_idx, idx, (size_t)n_idx);
        const unsigned long long seq = ++g.small_seq;
        unsigned long long* d_done = poll_completion() ? (unsigned long long*)g.pin_tot.d + 2 : nullptr;
        HIP_TRY(latok::launch_combine_rows((const uint8_t*)g.pin.d, cols, 1, cols, (const int8_t*)((char*)g.pin.d + po_idx), idx_ndim,
                                           irows, icols, (int8_t*)((char*)g.pin.d + po_out), st, d_done, seq));
        if (!(d_done && wait_completion_word((const unsigned long long*)g.pin_tot.h + 2, seq))) HIP_TRY(hipStreamSynchronize(st));
        memcpy(out, (char*)g.pin.h + po_out, (size_t)cols);
        return LATOK_OK;
    }
    // host: gather the (possibly strided) matrix into a dense rows x cols copy, upload, run, download
    std::vector<int8_t> dense((size_t)rows * (size_t)cols);
    for (int64_t r = 0; r < rows; ++r)
        for (int64_t c = 0; c < cols; ++c) dense[(size_t)(r * cols + c)] = m[r * stride_r + c * stride_c];
    if ((rc = g.h_cps.ensure(dense.size() + 16))) return rc;
    if ((rc = g.h_aux.ensure((size_t)n_idx + 16))) return rc;
    if ((rc = g.h_out.ensure((size_t)cols))) return rc;
    if (!dense.empty()) HIP_TRY(hipMemcpyAsync(g.h_cps.p, dense.data(), dense.size(), hipMemcpyHostToDevice, st));
    if (n_idx) HIP_TRY(hipMemcpyAsync(g.h_aux.p, idx, (size_t)n_idx, hipMemcpyHostToDevice, st));
    HIP_TRY(latok::launch_combine_rows((const uint8_t*)g.h_cps.p, cols, 1, cols, (const int8_t*)g.h_aux.p, idx_ndim,
                                       irows, icols, (int8_t*)g.h_out.p, st));
    HIP_TRY(hipMemcpyAsync(out, g.h_out.p, (size_t)cols, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return LATOK_OK;
}

int latok_block_mask(const int8_t* a1, const int8_t* a2, int64_t n, int8_t* out, int flags, void* stream) {
    LATOK_ENTER();
    int rc = need_init(g);
    if (rc) return rc;
    if (n < 0) return fail(LATOK_ERR_INVALID, "n must be >= 0");
    if (n == 0) return LATOK_OK;
    if (!a1 || !a2 || !out) return fail(LATOK_ERR_INVALID, "must specify two aligning 1d numpy array args");
    StreamTurn turn(g, stream);
    hipStream_t st = turn.st;
    const bool dev = (flags & LATOK_DEVICE_PTRS) != 0;
    // the block mask of ONE array pair is the batch pipeline over a single "string" [0, n) whose planes are a1 / a2
    const int64_t row[2] = {0, n};
    if (!dev && n <= latok::kTile) {
        // at most one tile: one single-wave launch on pinned memory, completion word (see compact_common)
        const size_t an = align16((size_t)n);
        if ((rc = g.pin.ensure(3 * an + 16 + 64))) return rc;
        if ((rc = g.pin_tot.ensure(64))) return rc;
        memcpy(g.pin.h, a1, (size_t)n);
        memcpy((char*)g.pin.h + an, a2, (size_t)n);
        memcpy((char*)g.pin.h + 3 * an, row, 16);
        latok::SplitParams P;
        memset(&P, 0, sizeof(P));
        P.row_off = (const int64_t*)((char*)g.pin.d + 3 * an);
        P.n_str = 1;
        P.total = n;
        P.n_tiles = 1;
        P.bm_a1 = (const int8_t*)g.pin.d;
        P.bm_a2 = (const int8_t*)((char*)g.pin.d + an);
        P.values_out = (uint8_t*)((char*)g.pin.d + 2 * an);
        const unsigned long long seq = ++g.small_seq;
        unsigned long long* d_done = poll_completion() ? (unsigned long long*)g.pin_tot.d + 2 : nullptr;
        HIP_TRY(latok::launch_small_block_mask(P, d_done, seq, st));
        if (!(d_done && wait_completion_word((const unsigned long long*)g.pin_tot.h + 2, seq))) HIP_TRY(hipStreamSynchronize(st));
        memcpy(out, (char*)g.pin.h + 2 * an, (size_t)n);
        return LATOK_OK;
    }
    if ((rc = g.h_row.ensure(16))) return rc;
    HIP_TRY(hipMemcpyAsync(g.h_row.p, row, 16, hipMemcpyHostToDevice, st));
    const int8_t *d1 = a1, *d2 = a2;
    int8_t* dout = out;
    if (dev) {
        if ((((uintptr_t)a1 | (uintptr_t)a2 | (uintptr_t)out) & 3) != 0)
            return fail(LATOK_ERR_INVALID, "device pointers must be 4-byte aligned");
    } else {
        if ((rc = g.h_cps.ensure((size_t)n + 16))) return rc;
        if ((rc = g.h_aux.ensure((size_t)n + 16))) return rc;
        if ((rc = g.h_out.ensure((size_t)n + 16))) return rc;
        HIP_TRY(hipMemcpyAsync(g.h_cps.p, a1, (size_t)n, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(g.h_aux.p, a2, (size_t)n, hipMemcpyHostToDevice, st));
        d1 = (const int8_t*)g.h_cps.p;
        d2 = (const int8_t*)g.h_aux.p;
        dout = (int8_t*)g.h_out.p;
    }
    int* d_flags = (int*)((char*)g.ws.scalar.p + 16);
    HIP_TRY(latok::launch_any_nonzero(d1, d2, n, d_flags, st));
    Pipe a;
    a.b = Batch{Input{}, (const int64_t*)g.h_row.p, 1, n};
    a.mode = latok::kModeBlockMask;
    a.values = (uint8_t*)dout;
    a.bm_a1 = d1;
    a.bm_a2 = d2;
    a.bm_flags = d_flags;
    a.st = st;
    if ((rc = run_pipeline(g, g.ws, a))) return rc;
    if (!dev) {
        HIP_TRY(hipMemcpyAsync(out, dout, (size_t)n, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return LATOK_OK;
}

void* latok_dev_alloc(size_t bytes) {
    LATOK_ENTER();
    void* p = nullptr;
    if (!g.inited) { fail(LATOK_ERR_NOT_INIT, "latok_init() has not been called"); return nullptr; }
    hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
    if (e != hipSuccess) { fail(LATOK_ERR_NOMEM, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e)); return nullptr; }
    return p;
}
int latok_dev_free(void* p) {
    LATOK_ENTER();
    if (p) HIP_TRY(hipFree(p));
    return LATOK_OK;
}
void* latok_host_alloc(size_t bytes) {
    LATOK_ENTER();
    void* p = nullptr;
    if (!g.inited) { fail(LATOK_ERR_NOT_INIT, "latok_init() has not been called"); return nullptr; }
    hipError_t e = hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault);
    if (e != hipSuccess) { fail(LATOK_ERR_NOMEM, "hipHostMalloc(%zu): %s", bytes, hipGetErrorString(e)); return nullptr; }
    return p;
}
int latok_host_free(void* p) {
    LATOK_ENTER();
    if (p) HIP_TRY(hipHostFree(p));
    return LATOK_OK;
}
int latok_memcpy_h2d(void* d, const void* s, size_t n) {
    LATOK_ENTER();
    int rc = need_init(g);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(d, s, n, hipMemcpyHostToDevice, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    return LATOK_OK;
}
int latok_memcpy_d2h(void* d, const void* s, size_t n) {
    LATOK_ENTER();
    int rc = need_init(g);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(d, s, n, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    return LATOK_OK;
}
int latok_memset_dev(void* d, int v, size_t n) {
    LATOK_ENTER();
    int rc = need_init(g);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(d, v, n, g.stream));
    return LATOK_OK;
}
int latok_sync(void) {
    LATOK_ENTER();
    int rc = need_init(g);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(g.stream));
    return flow_drain(g);
}
int latok_device_props(int* n_cu, int64_t* hbm_bytes, char* name_out, int name_cap) {
    LATOK_ENTER();
    int rc = need_init(g);
    if (rc) return rc;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, g.device));
    if (n_cu) *n_cu = prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (int64_t)prop.totalGlobalMem;
    if (name_out && name_cap > 0) snprintf(name_out, (size_t)name_cap, "%s (%s)", prop.name, prop.gcnArchName);
    return LATOK_OK;
}

int latok_corpus_offsets(uint64_t seed, uint64_t sid0, int64_t n_str, int64_t len_lo, int64_t len_hi,
                         int64_t* row_off_out) {
    if (n_str < 0 || len_lo < 0 || len_hi < len_lo || !row_off_out) return fail(LATOK_ERR_INVALID, "bad corpus shape");
    int64_t acc = 0;
    row_off_out[0] = 0;
    for (int64_t s = 0; s < n_str; ++s) {
        acc += latok_corpus_length(seed, sid0 + (uint64_t)s, len_lo, len_hi);
        row_off_out[s + 1] = acc;
    }
    return LATOK_OK;
}
int latok_corpus_fill_host(uint64_t seed, int model, uint64_t sid0, int64_t n_str, const int64_t* row_off,
                           uint32_t* cps_out) {
    if (n_str < 0 || !row_off || (!cps_out && n_str > 0 && row_off[n_str] > 0)) return fail(LATOK_ERR_INVALID, "bad corpus args");
    for (int64_t s = 0; s < n_str; ++s)
        latok_corpus_string(seed, model, sid0 + (uint64_t)s, cps_out + row_off[s], row_off[s + 1] - row_off[s]);
    return LATOK_OK;
}
int latok_corpus_fill_device(uint64_t seed, int model, uint64_t sid0, int64_t n_str, const int64_t* row_off_dev,
                             uint32_t* cps_out_dev, void* stream) {
    LATOK_ENTER();
    int rc = need_init(g);
    if (rc) return rc;
    HIP_TRY(latok::launch_corpus_fill(seed, model, sid0, n_str, row_off_dev, cps_out_dev,
                                      stream ? (hipStream_t)stream : g.stream));
    return LATOK_OK;
}
int latok_utf8_bytes(const uint32_t* cps, int64_t n, int64_t* bytes_out, int flags) {
    if (!bytes_out || n < 0) return fail(LATOK_ERR_INVALID, "bad args");
    if (!(flags & LATOK_DEVICE_PTRS)) {
        int64_t t = 0;
        for (int64_t i = 0; i < n; ++i) t += latok_utf8_len(cps[i]);
        *bytes_out = t;
        return LATOK_OK;
    }
    LATOK_ENTER();
    int rc = need_init(g);
    if (rc) return rc;
    HIP_TRY(latok::launch_utf8_bytes(cps, n, (unsigned long long*)g.ws.scalar.p, g.stream));
    unsigned long long t = 0;
    HIP_TRY(hipMemcpyAsync(&t, g.ws.scalar.p, 8, hipMemcpyDeviceToHost, g.stream));
    HIP_TRY(hipStreamSynchronize(g.stream));
    *bytes_out = (int64_t)t;
    return LATOK_OK;
}

/* test hook (not part of the ABI in include/latok_hip.h): set the scan epoch of the current context, so that the wrap of
 * the 18-bit epoch of k_word_counts_scan's state can be exercised without 262 144 calls */
int latok_debug_set_scan_epoch(unsigned epoch) {
    LATOK_ENTER();
    g.ws.scan_epoch = epoch & 0x3FFFFu;
    return LATOK_OK;
}

/* test hook (not part of the ABI; needs no device): the constants that decide the tile pipeline's plans and host paths, so that
 * tests take their thresholds from the library: out[0..8] = kTile, kWPB, kNarrowWPB, kSegMax, kOneSegTiles, kFastTailTiles,
 * kSmallChars, kSmallStrings, tiles per workgroup of k_lead_compress; out[9..13] = kFeatWaves, kFeatRound, kFeatRoundTm,
 * kFeatFormThresh, kFeatWinBytes of k_features_tiles; out[14] = kHashWaveBytes (a longer token is hashed by its whole wave);
 * out[15..16] = kScanSmallMax (more entries: the exclusive scan takes three launches), kU8Block (bytes per block of the staged
 * UTF-8 decoder, one scan entry each); out[17..18] = kCountProbeMax (steps after which a probe of a counting table gives up),
 * kCountAccEntries (entries of a wave's count accumulator in k_count_scatter).  Returns the number of values written.  The list is
 * closed at these 19 entries (tests/test_count_table_host.py pins the count); later constants have hooks of their own. */
extern "C" int latok_debug_limits(int64_t* out, int n) {
    const int64_t v[19] = {latok::kTile, latok::kWPB, latok::kNarrowWPB, latok::kSegMax, latok::kOneSegTiles, latok::kFastTailTiles,
                           kSmallChars, kSmallStrings, latok::kCompressWaves, latok::kFeatWaves, latok::kFeatRound, latok::kFeatRoundTm,
                           latok::kFeatFormThresh, latok::kFeatWinBytes, latok::kHashWaveBytes, latok::scan_small_max(),
                           latok::utf8_block_bytes(), latok::kCountProbeMax, latok::kCountAccEntries};
    if (!out || n < 0) return fail(LATOK_ERR_INVALID, "NULL output");
    const int k = n < 19 ? n : 19;
    for (int i = 0; i < k; ++i) out[i] = v[i];
    return k;
}

/* test hook (not part of the ABI; needs no device): the constants of the term-count kernels (terms_kernels.hip): out[0] = kTermsTile
 * (tokens per tile: a workgroup owns the rows that start in its tile), out[1] = kTermsRowMax (a row of more tokens is sorted by a
 * workgroup of its own).  Returns the number of values written. */
extern "C" int latok_debug_terms_limits(int64_t* out, int n) {
    const int64_t v[2] = {latok::kTermsTile, latok::kTermsRowMax};
    if (!out || n < 0) return fail(LATOK_ERR_INVALID, "NULL output");
    const int k = n < 2 ? n : 2;
    for (int i = 0; i < k; ++i) out[i] = v[i];
    return k;
}

/* test hook (not part of the ABI; needs no device): the constants of the character n-gram calls: out[0] = kCgBlock (tokens per
 * workgroup of k_cgram_count / k_cgram_keys), out[1] = kNgMax (the highest order).  Returns the number of values written. */
extern "C" int latok_debug_chargram_limits(int64_t* out, int n) {
    const int64_t v[2] = {latok::kCgBlock, kNgMax};
    if (!out || n < 0) return fail(LATOK_ERR_INVALID, "NULL output");
    const int k = n < 2 ? n : 2;
    for (int i = 0; i < k; ++i) out[i] = v[i];
    return k;
}
/* test hook (not part of the ABI; needs no device): the constants of the n-gram calls: out[0] = kNgBlock (tokens per workgroup of
 * k_ngram_keys), out[1] = kNgMax (the highest order).  Returns the number of values written. */
extern "C" int latok_debug_ngram_limits(int64_t* out, int n) {
    const int64_t v[2] = {latok::kNgBlock, kNgMax};
    if (!out || n < 0) return fail(LATOK_ERR_INVALID, "NULL output");
    const int k = n < 2 ? n : 2;
    for (int i = 0; i < k; ++i) out[i] = v[i];
    return k;
}

/* test hook (not part of the ABI; needs no device): the constants of the fold call: out[0] = kFoldTile (bytes per wave of
 * k_fold_counts / k_fold_write), out[1] = bytes per lane and load (16), out[2] = the largest growth in bytes (3) */
extern "C" int latok_debug_fold_limits(int64_t* out, int n) {
    const int64_t v[3] = {latok::kFoldTile, 16, 3};
    if (!out || n < 0) return fail(LATOK_ERR_INVALID, "NULL output");
    const int k = n < 3 ? n : 3;
    for (int i = 0; i < k; ++i) out[i] = v[i];
    return k;
}

/* test hook (not part of the ABI; needs no device): the constants of the WordPiece calls: out[0] = kWpBlock (tokens per workgroup of
 * k_wp_count / k_wp_emit), out[1] = entries per workgroup of the chained scan over the piece counts (one scan block), out[2] =
 * kWpMaxPrefix, out[3] = kWpMaxChars.  Returns the number of values written. */
extern "C" int latok_debug_wordpiece_limits(int64_t* out, int n) {
    const int64_t v[4] = {latok::kWpBlock, latok::scan_chunk(), kWpMaxPrefix, kWpMaxChars};
    if (!out || n < 0) return fail(LATOK_ERR_INVALID, "NULL output");
    const int k = n < 4 ? n : 4;
    for (int i = 0; i < k; ++i) out[i] = v[i];
    return k;
}

/* test hook (not part of the ABI; needs no device): the constants of the BPE calls: out[0] = kBpeBlock (tokens per workgroup of
 * k_bpe_count / k_bpe_emit), out[1] = entries per workgroup of the chained scan over the piece counts (one scan block), out[2] =
 * kBpeLaneBytes (the longest token of the lane form), out[3] = kBpeMaxBytes (the ceiling of max_bytes).  Returns the number of values
 * written. */
extern "C" int latok_debug_bpe_limits(int64_t* out, int n) {
    const int64_t v[4] = {latok::kBpeBlock, latok::scan_chunk(), kBpeLaneBytes, kBpeMaxBytes};
    if (!out || n < 0) return fail(LATOK_ERR_INVALID, "NULL output");
    const int k = n < 4 ? n : 4;
    for (int i = 0; i < k; ++i) out[i] = v[i];
    return k;
}

/* test hook (not part of the ABI; needs no device): the constants of the SentencePiece BPE calls: out[0] = kBpeBlock (segments per
 * workgroup of k_spbpe_count / k_spbpe_emit), out[1] = kSpLaneBytes (the longest virtual text of the lane form), out[2] = kBpeMaxBytes
 * (the ceiling of max_bytes).  Returns the number of values written. */
extern "C" int latok_debug_spbpe_limits(int64_t* out, int n) {
    const int64_t v[3] = {latok::kBpeBlock, kSpLaneBytes, kBpeMaxBytes};
    if (!out || n < 0) return fail(LATOK_ERR_INVALID, "NULL output");
    const int k = n < 3 ? n : 3;
    for (int i = 0; i < k; ++i) out[i] = v[i];
    return k;
}

/* test hook (not part of the ABI; needs no device): the constants of the GPT-2 pre-tokenizer's front (k_pretok_planes): out[0] = bytes per
 * word (one lane), out[1] = bytes per tile (one wave), out[2] = threads per workgroup, out[3] = kPtHalo (the bytes a word's window holds
 * on either side of the word).  Returns the number of values written. */
extern "C" int latok_debug_pretok_limits(int64_t* out, int n) {
    const int64_t v[4] = {kPtWord, latok::kTile, latok::kPretokWaves * 64, kPtHalo};
    if (!out || n < 0) return fail(LATOK_ERR_INVALID, "NULL output");
    const int k = n < 4 ? n : 4;
    for (int i = 0; i < k; ++i) out[i] = v[i];
    return k;
}

/* test hook (not part of the ABI; needs no device): the constants of the cl100k pre-tokenizer's front (k_pretok_cl100k_records,
 * k_pretok_cl100k_planes): out[0] .. out[3] as latok_debug_pretok_limits, out[4] = tile records per step of the walk.  Returns the
 * number of values written. */
extern "C" int latok_debug_pretok_cl100k_limits(int64_t* out, int n) {
    const int64_t v[5] = {kPtWord, latok::kTile, latok::kPretokWaves * 64, kPtHalo, latok::kPretokWalk};
    if (!out || n < 0) return fail(LATOK_ERR_INVALID, "NULL output");
    const int k = n < 5 ? n : 5;
    for (int i = 0; i < k; ++i) out[i] = v[i];
    return k;
}

/* test hook (not part of the ABI; needs no device): the constants of the Unigram calls: out[0] = kUniBlock (tokens per workgroup of
 * k_uni_count / k_uni_emit), out[1] = entries per workgroup of the chained scan over the piece counts, out[2] = kUniLaneBytes (the
 * longest token of the lane form), out[3] = kUniMaxBytes (the ceiling of max_bytes).  Returns the number of values written. */
extern "C" int latok_debug_unigram_limits(int64_t* out, int n) {
    const int64_t v[4] = {latok::kUniBlock, latok::scan_chunk(), kUniLaneBytes, kUniMaxBytes};
    if (!out || n < 0) return fail(LATOK_ERR_INVALID, "NULL output");
    const int k = n < 4 ? n : 4;
    for (int i = 0; i < k; ++i) out[i] = v[i];
    return k;
}

/* test hook (not part of the ABI; needs no device): the constants of the two device-wide int64 scans: out[0] = kChainChunk (entries per
 * workgroup of k_scan_chained), out[1] = predecessors one look-back round reads (64), out[2] = kChainValueBits, out[3] = bits of the
 * launch epoch (18), out[4] = kScanSmallMax, out[5] = kScanChunk (entries per workgroup of k_scan_local), out[6] = kScanBlock.  Returns
 * the number of values written. */
extern "C" int latok_debug_scan_limits(int64_t* out, int n) {
    const int64_t v[7] = {latok::scan_chunk(), latok::chain_lookback(), latok::chain_value_bits(), latok::chain_epoch_bits(),
                          latok::scan_small_max(), latok::scan_local_chunk(), latok::scan_block_threads()};
    if (!out || n < 0) return fail(LATOK_ERR_INVALID, "NULL output");
    const int k = n < 7 ? n : 7;
    for (int i = 0; i < k; ++i) out[i] = v[i];
    return k;
}

/* test hook (not part of the ABI): one device-wide exclusive scan of d_in[0 .. n) into d_out (device pointers), exactly as the calls
 * run it, on the current context and its stream; blocking.  which = 0: the chained scan as enqueue_row_scan runs it -- next_scan_epoch
 * on the context's workspace, whose chain array ws_needs sizes as for a call of n rows, then launch_tile_scan; d_units (or NULL): the
 * device word of the kernel's device-sized form (ceil(*d_units / kTile) entries are real, the grid is sized for n).  which = 1:
 * launch_exclusive_scan with the context's own block totals and total words, as decode_utf8_to_workspace calls it.  *total_out = the
 * total the device wrote (the device word and the pinned word must agree), *flag_out = the scan's own error flag.
 * THE BOUND: a chained scan's total must stay below 2^kChainValueBits (2^44) -- the value field of a published word holds no more and
 * wraps silently; every count the calls scan (rows, tokens, pieces, bytes of a batch) is far below it. */
extern "C" int latok_debug_scan(int which, const int64_t* d_in, int64_t n, int64_t* d_out, const int64_t* d_units, int64_t* total_out,
                                int* flag_out) {
    LATOK_ENTER();
    int rc = need_init(g);
    if (rc) return rc;
    if (n < 1) return fail(LATOK_ERR_INVALID, "n must be >= 1");
    if ((which != 0 && which != 1) || !d_in || !d_out || !total_out || !flag_out || (which == 1 && d_units)) return fail(LATOK_ERR_INVALID, "bad args");
    StreamTurn turn(g, nullptr);
    const hipStream_t st = turn.st;
    Workspace& w = g.ws;
    if ((rc = g.pin_tot.ensure(64))) return rc;
    volatile int64_t* h = (volatile int64_t*)g.pin_tot.h;
    int64_t* p = (int64_t*)g.pin_tot.d;
    h[0] = -1;
    h[1] = 0;
    int64_t* d_total = nullptr;
    if (which == 0) {
        for (const WsNeed& need : ws_needs(w, 0, WsShape{.term_rows = n}))
            if ((need.buf == &w.chain || need.buf == &w.chain_ctl || need.buf == &w.scalar) && (rc = need.buf->ensure(need.bytes))) return rc;
        d_total = (int64_t*)w.scalar.p + 4;
        latok::ChainState chain;
        if ((rc = next_scan_epoch(w, st, &chain))) return rc;
        HIP_TRY(latok::launch_tile_scan(d_in, n, d_out, chain, d_total, p, (int*)(p + 1) + 1, st, d_units));
    } else {
        if ((rc = w.scalar.ensure(64)) || (rc = g.scan_tot.ensure((size_t)latok::scan_blocks(n) * 8))) return rc;
        d_total = (int64_t*)w.scalar.p;
        HIP_TRY(latok::launch_exclusive_scan(d_in, n, d_out, d_total, (int64_t*)g.scan_tot.p, st, p));
    }
    int64_t dev_total = -2;
    HIP_TRY(hipMemcpyAsync(&dev_total, d_total, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *flag_out = (int)(h[1] >> 32);
    *total_out = h[0];
    if (*flag_out) w.chain_ready = false;   // (as finish_totals: the next scan clears the state)
    else if (dev_total != h[0]) return fail(LATOK_ERR_HIP, "the scan's device total %lld and pinned total %lld differ", (long long)dev_total, (long long)h[0]);
    return LATOK_OK;
}

// LaunchPlan as the hooks report it: out[0..11] = n_cu_eff, seg_tiles, n_segs, rounds, grid of k_tiles_main, grid of
// k_resolve_fix, fast_tail, pf, wpb, nw, one_launch, n_tiles
static int put_plan(const latok::LaunchPlan& L, int64_t n_tiles, int64_t* out, int n) {
    const int64_t v[12] = {L.n_cu_eff, L.seg_tiles, L.n_segs, L.rounds, L.grid, L.one_launch ? 0 : L.grid, L.fast_tail, L.pf, L.wpb, L.nw,
                           L.one_launch, n_tiles};
    const int k = n < 12 ? n : 12;
    for (int i = 0; i < k; ++i) out[i] = v[i];
    return k;
}

/* test hook (not part of the ABI; needs no device): what run_pipeline would launch for a batch of n_tiles tiles on n_cu CUs,
 * in_flow = a batch of a flow, mode = latok::kMode* after the rules (the one-launch path as a blocking UTF-32 call would take
 * it).  Fills out as put_plan, returns the number of values written. */
extern "C" int latok_debug_plan(int64_t n_tiles, int n_cu, int in_flow, int mode, int64_t* out, int n) {
    if (!out || n < 0 || n_tiles < 1 || n_cu < 1 || mode < latok::kModeBits || mode > latok::kModeValuesRules)
        return fail(LATOK_ERR_INVALID, "n_tiles >= 1, n_cu >= 1, mode 0..%d", latok::kModeValuesRules);
    latok::LaunchPlan L;
    latok::plan_launch(n_tiles, n_cu, in_flow != 0, mode, one_segment_enabled(), &L);
    return put_plan(L, n_tiles, out, n);
}

/* test hook (not part of the ABI): the tile pipeline of the current context (k_tile_index / k_tiles_main / k_resolve_fix /
 * k_one_segment) plans and launches as if the device had n_cu CUs; 0 = the device's own count.  The pipeline's workgroups
 * never wait for one another (they share data between launches only), so a smaller grid only makes each persistent
 * workgroup walk more segments.  Compaction, featurize and the other kernels keep their grids. */
extern "C" int latok_debug_set_plan_cus(int n_cu) {
    LATOK_ENTER();
    int rc = need_init(g);
    if (rc) return rc;
    if (n_cu != 0 && (n_cu < 8 || n_cu > g.n_cu)) return fail(LATOK_ERR_INVALID, "plan CUs must be 0 or 8..%d", g.n_cu);
    g.plan_cus = n_cu;
    return LATOK_OK;
}

/* test hook (not part of the ABI; needs no device): the constants of the tile kernel's held segments (kernels.h): out[0] =
 * kSegHoldTiles (a segment of at most that many tiles of a UTF-32 bitmask batch stores its mask words as one run at its end),
 * out[1] = kSegHoldLdsRounds (tiles per wave whose words wait in LDS; the others wait in registers).  Returns the number of values
 * written. */
extern "C" int latok_debug_tile_limits(int64_t* out, int n) {
    const int64_t v[2] = {latok::kSegHoldTiles, latok::kSegHoldLdsRounds};
    if (!out || n < 0) return fail(LATOK_ERR_INVALID, "NULL output");
    const int k = n < 2 ? n : 2;
    for (int i = 0; i < k; ++i) out[i] = v[i];
    return k;
}

/* test hook (not part of the ABI): the tile pipeline of the current context plans with a segment length of seg_tiles tiles (0 = the
 * plan's own; kWPB .. kSegMax, and the one-launch path is then not taken), launches at most `grid` workgroups (0 = the plan's own: a
 * smaller grid makes each persistent workgroup walk more segments) and, with hold = 0, never holds a segment's mask words for the
 * write-out at its end (-1 = the plan's own: segments of at most kSegHoldTiles tiles are held).  (0, 0, -1) restores the plan. */
extern "C" int latok_debug_set_tile_plan(int seg_tiles, int grid, int hold) {
    LATOK_ENTER();
    int rc = need_init(g);
    if (rc) return rc;
    if (seg_tiles != 0 && (seg_tiles < latok::kWPB || seg_tiles > latok::kSegMax))
        return fail(LATOK_ERR_INVALID, "segment length must be 0 or %d..%d", latok::kWPB, latok::kSegMax);
    if (grid < 0 || (hold != 0 && hold != -1)) return fail(LATOK_ERR_INVALID, "grid >= 0, hold 0 or -1");
    g.plan_force.seg_tiles = seg_tiles;
    g.plan_force.grid = grid;
    g.plan_force.hold = hold;
    return LATOK_OK;
}

/* test hook (not part of the ABI): what the last run_pipeline of the current context launched.  out[0] = mode (after the
 * rules), out[1] = 1 if a host batch ran in place on pinned memory (small-batch path), out[2] = tiles recomputed by the
 * resolve stage (read after a synchronisation of the call's stream), out[3..14] = the plan as latok_debug_plan reports it,
 * out[15] = 1 if the tile kernel held its segments' mask words for one write-out per segment (LaunchPlan::hold).
 * Returns the number of values written, 0 when nothing has run. */
extern "C" int latok_debug_last_plan(int64_t* out, int n) {
    LATOK_ENTER();
    int rc = need_init(g);
    if (rc) return rc;
    if (!out || n < 0) return fail(LATOK_ERR_INVALID, "NULL output");
    if (!g.last.valid) return 0;
    int64_t fix = 0;
    HIP_TRY(hipStreamSynchronize(g.last.st));
    HIP_TRY(hipMemcpy(&fix, g.last.fix_count, 8, hipMemcpyDeviceToHost));
    const int64_t head[3] = {g.last.mode, g.last.small ? 1 : 0, fix};
    int k = 0;
    for (; k < 3 && k < n; ++k) out[k] = head[k];
    if (n > 3) k += put_plan(g.last.plan, g.last.n_tiles, out + 3, n - 3);
    if (n > 15 && k == 15) out[k++] = g.last.plan.hold;   // out[15] = the tile kernel held its segments' mask words (latok_debug_set_tile_plan)
    return k;
}

/* test hook (not part of the ABI): the route the last compaction call (offsets / spans / featurize) of the current context took --
 * 0: the batch's own units (UTF-32, PEP 393 units, UTF-8 in byte space), 1: a small UTF-8 host batch decoded by the host,
 * 2: UTF-8 through the staged device decoder, 3: UTF-8 through byte space and the packed code-point masks (and codes),
 * 4: featurize of UTF-8 in byte space (byte records from the byte-space masks, sums from the packed code-point masks),
 * 5: joined token text of UTF-8 in byte space (every batch size; there is no small-batch route),
 * 6: token hashes of UTF-8 in byte space (every batch size as well); 7: token ids of UTF-8 in byte space (likewise);
 * 9 / 10: term counts of UTF-8 in byte space, vocabulary form / hashed form (likewise);
 * 11 / 12: WordPiece ids of UTF-8 in byte space, CSR form / padded form (likewise);
 * 13: case folding of UTF-8 in byte space (likewise); 14 / 15: word n-gram counts, vocabulary form / hashed form (likewise);
 * 16 / 17: character n-gram counts inside tokens, vocabulary form / hashed form (likewise);
 * 18 / 19: byte-level BPE ids of UTF-8 in byte space, CSR form / padded form (likewise);
 * 20 / 21: decoding, ids back to bytes, CSR form / padded form (likewise);
 * 22 / 23: Unigram ids of UTF-8 in byte space, CSR form / padded form (likewise);
 * 24 / 25: byte-level BPE ids behind GPT-2's pre-tokenizer (an object of latok_bpe_create_pretok), CSR form / padded form (likewise);
 * 26: pre-token spans of GPT-2's pre-tokenizer (latok_pretokens_utf8_bytes_batch; LATOK_PRETOK_LATOK reports the span call's routes);
 * 27 / 28: byte-level BPE ids behind the cl100k pre-tokenizer, CSR form / padded form; 29: pre-token spans of the cl100k pre-tokenizer;
 * 30 / 31: SentencePiece BPE ids (an object of latok_bpe_create_spm), CSR form / padded form; 32: the segments of LATOK_PRETOK_SPM */
extern "C" int latok_debug_last_route(void) {
    LATOK_ENTER();
    return g.last_route;
}

/* test hook (not part of the ABI; needs no device): the flow's routing of batches to slots (flow_hazards.h) driven without a
 * GPU.  One call = one batch touching n ranges (lo[i], bytes[i], is_write[i]); returns the slot it is enqueued on, *drained_out = 1
 * when the flow had to be drained first.  n < 0: forget everything (= latok_flow_wait).  State of the calling thread. */
extern "C" int latok_debug_flow_route(int n_slots, const uint64_t* lo, const uint64_t* bytes, const int* is_write, int n, int* drained_out) {
    static thread_local latok::FlowHazards held;
    static thread_local unsigned long long seq = 0;
    if (drained_out) *drained_out = 0;
    if (n < 0) { held.clear(); seq = 0; return 0; }
    if (n_slots < 1 || n_slots > latok::FlowHazards::kMaxSlots || n > 16) return fail(LATOK_ERR_INVALID, "1..4 slots, <= 16 ranges");
    latok::FlowRange r[16];
    for (int i = 0; i < n; ++i) r[i] = latok::flow_range((const void*)(uintptr_t)lo[i], (size_t)bytes[i], is_write[i] != 0);
    const int turn = (int)(seq % (unsigned)n_slots);
    int s = held.route(n_slots, turn, r, n);
    if (s == latok::FlowHazards::kDrainFirst) {
        held.clear();
        if (drained_out) *drained_out = 1;
        s = turn;
    }
    held.note(s, r, n);
    ++seq;
    return s;
}

/* test hook (not part of the ABI; needs no device): the host decoder of small UTF-8 batches (host_decode_small).  Returns 1 and
 * fills cps_out[<= total bytes], cp_row_out[n_str + 1], bytepos_out[<= total bytes + 1] when every string is well formed,
 * 0 when the batch is left to the device paths, < 0 on a bad argument. */
extern "C" int latok_debug_host_decode_utf8(const uint8_t* utf8, const int64_t* byte_off, int64_t n_str, uint32_t* cps_out,
                                            int64_t* cp_row_out, int64_t* bytepos_out, int64_t* n_cps_out) {
    int64_t total = -1;
    if (!byte_off || n_str <= 0 || check_csr_host(byte_off, n_str, &total) != LATOK_OK) return LATOK_ERR_INVALID;
    std::vector<uint32_t> cps;
    std::vector<int64_t> row, pos;
    if (!host_decode_small(utf8, byte_off, n_str, cps, row, pos)) return 0;
    memcpy(cps_out, cps.data(), cps.size() * 4);
    memcpy(cp_row_out, row.data(), row.size() * 8);
    memcpy(bytepos_out, pos.data(), pos.size() * 8);
    *n_cps_out = (int64_t)cps.size();
    return 1;
}


// ---- batch flow: several device-resident batches in flight on one context --------------------------------------------
// A batch is three dependent launches (string index, tiles, resolve) and only the tile kernel fills the chip; back to back on
// one stream the two latency-bound launches and the three kernel boundaries cost 11-14 us of a 108 us step on C2.  A flow
// gives every batch in flight its own stream and workspace (two slots, used in turn) and NO dependency between the streams:
// the tile kernel of batch i+1 takes over the CUs as the workgroups of batch i retire, and the small launches of one stream
// run in the shadow of the other stream's tile kernel.  (Measured first: one stream per STAGE with events between them, so that
// the tile kernels stay strictly back to back -- 115-120 us per step, slower than serial: an inter-queue event wait costs more
// than the launch it hides.)
static int flow_setup(Ctx& g) {
    if (g.flow_ready) return LATOK_OK;
    g.flow_slots = 2;   // (3 and 4 slots measured: nothing over 2, profiles/r03_ab_flow_slots.txt)
    for (int i = 0; i < g.flow_slots; ++i) {
        Ctx::FlowSlot& f = g.flow[i];
        if (!f.st) HIP_TRY(hipStreamCreateWithFlags(&f.st, hipStreamNonBlocking));
    }
    g.flow_ready = true;
    return LATOK_OK;
}
static int flow_drain(Ctx& g) {
    if (!g.flow_ready) return LATOK_OK;
    // The streams are POLLED for up to 2 ms before the call blocks on them: a blocking wait comes back ~15 us after the last
    // kernel has ended (the runtime's wake-up), which is 1.5 % of a 20-batch flow on C2 (same-box A/B, K = 20: 89.1-90.7 ->
    // 86.1-88.7 us per batch).
    constexpr bool drain_poll = true;
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < g.flow_slots; ++i) {
        bool done = false;
        if (drain_poll) {
            for (unsigned spins = 0;; ++spins) {
                const hipError_t q = hipStreamQuery(g.flow[i].st);
                if (q == hipSuccess) { done = true; break; }
                if (q != hipErrorNotReady) return fail(LATOK_ERR_HIP, "hipStreamQuery failed: %s", hipGetErrorString(q));
                cpu_relax();
                if ((spins & 63) == 63 &&
                    std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() > 2000)
                    break;
            }
        }
        if (!done) HIP_TRY(hipStreamSynchronize(g.flow[i].st));
    }
    g.flow_held.clear();   // nothing in flight: no buffer is being read or written
    return LATOK_OK;
}
// Reserve what a batch needs in a slot.  A buffer that has to grow is reallocated only once nothing in flight can still use it.
static int flow_reserve(Ctx& g, const WsNeed* needs, int n) {
    bool grow = false;
    for (int i = 0; i < n; ++i) grow = grow || needs[i].buf->cap < needs[i].bytes;
    if (!grow) return LATOK_OK;
    const int rc = flow_drain(g);
    return rc ? rc : ws_ensure(needs, n);
}
// Slots are used in turn -- except that a batch which touches memory a batch still in flight writes (or writes memory one
// reads) goes to THAT batch's slot, whose stream orders the two; when batches of several slots are in its way the flow is
// drained first (flow_hazards.h; callers that alternate buffers never hit either; an event per batch to order such pairs
// across streams would cost every batch ~3 us).  *slot_out = the slot to enqueue on; the caller notes the batch's ranges.
static int flow_pick(Ctx& g, const latok::FlowRange* r, int n, int* slot_out) {
    const int turn = (int)(g.flow_seq % (unsigned)g.flow_slots);
    int s = g.flow_held.route(g.flow_slots, turn, r, n);
    if (s == latok::FlowHazards::kDrainFirst) {
        const int rc = flow_drain(g);
        if (rc) return rc;
        s = turn;
    }
    // a caller that never waits and never repeats a buffer: forget what an idle slot held; bound the list of a busy one
    if (g.flow_held.held(s) >= latok::FlowHazards::kPruneAt) {
        const hipError_t q = hipStreamQuery(g.flow[s].st);
        if (q == hipSuccess) g.flow_held.clear_slot(s);
        else if (q != hipErrorNotReady) return fail(LATOK_ERR_HIP, "hipStreamQuery failed: %s", hipGetErrorString(q));
        else if (g.flow_held.held(s) >= 4 * latok::FlowHazards::kPruneAt) {
            HIP_TRY(hipStreamSynchronize(g.flow[s].st));
            g.flow_held.clear_slot(s);
        }
    }
    *slot_out = s;
    return LATOK_OK;
}
// The prologue of a flow batch, the same for every submitter: what it touches, what is cleared for it, what its slot must hold.
struct FlowZero {
    void* p;
    size_t bytes;
};
struct FlowOpen {
    const latok::FlowRange* r = nullptr;   // every range of caller memory the batch touches, outputs first (the *_flow_ranges)
    int n_r = 0;
    bool empty = false;                    // no string or no unit: nothing is launched
    FlowZero result = {};                  // result words cleared on the slot's stream before the batch: 32 bytes (code-point UTF-8),
                                           // 16 (join, hashes), none (there are none, or the enqueue core clears its own)
    FlowZero zero[2] = {};                 // an empty batch: the buffers it zeroes (NULL / 0 entries are skipped)
    int64_t units = 0;                     // a batch that launches: the slot's workspace is sized by ws_needs(units, shape),
    WsShape shape;                         // of which the first n_needs entries are reserved (kTileNeeds: the mask alone)
    int n_needs = kWsNeeds;
};
// Picks the slot, reserves its workspace and notes the ranges before anything is enqueued: a launch that fails midway cannot
// leave work on the caller's buffers that the routing does not know of (over-noting only costs overlap).  Then the clears, on
// the slot's stream.  Only a batch that launches counts in flow_seq, by which the slots take turns.
static int flow_open(Ctx& g, const FlowOpen& o, int* slot_out) {
    int rc, s = 0;
    if ((rc = flow_setup(g)) || (rc = flow_pick(g, o.r, o.n_r, &s))) return rc;
    Ctx::FlowSlot& f = g.flow[s];
    if (!o.empty && (rc = flow_reserve(g, ws_needs(f.ws, o.units, o.shape).data(), o.n_needs))) return rc;
    g.flow_held.note(s, o.r, o.n_r);
    if (!o.empty) ++g.flow_seq;
    if (o.result.bytes) HIP_TRY(hipMemsetAsync(o.result.p, 0, o.result.bytes, f.st));
    if (o.empty)
        for (const FlowZero& z : o.zero)
            if (z.p && z.bytes) HIP_TRY(hipMemsetAsync(z.p, 0, z.bytes, f.st));
    *slot_out = s;
    return LATOK_OK;
}
constexpr int kMaskFlowRanges = 3, kCompactFlowRanges = 6;
// every range of caller memory a mask batch (b: n_str > 0, total > 0) touches, outputs first; returns their number
static int mask_flow_ranges(const Batch& b, uint64_t* mask, latok::FlowRange* r) {
    r[0] = latok::flow_range(mask, (size_t)((b.total + 63) / 64) * 8, true);
    r[1] = latok::flow_range(b.in.p, (size_t)b.total * b.in.width(), false);
    r[2] = latok::flow_range(b.row, (size_t)(b.n_str + 1) * 8, false);
    return kMaskFlowRanges;
}
// ... and a compaction batch: records, counts, result words, feature sums, then its inputs.  An empty batch (cap unchecked) touches
// its result words and counts alone.
static int compact_flow_ranges(bool spans, bool feats, const Batch& b, bool empty, void* counts, void* items, int8_t* feat, int64_t cap,
                               int64_t* result, size_t rec, latok::FlowRange* r) {
    const size_t n_str = (size_t)std::max<int64_t>(b.n_str, 0), n_items = empty ? 0 : (size_t)cap, fields = feats ? 4 : (spans ? 2 : 1);
    r[0] = latok::flow_range(items, n_items * fields * rec, true);
    r[1] = latok::flow_range(counts, n_str * rec, true);
    r[2] = latok::flow_range(result, 16, true);
    r[3] = latok::flow_range(feat, feats ? n_items * LATOK_FEATURE_COUNT : 0, true);
    r[4] = latok::flow_range(b.in.p, empty ? 0 : (size_t)b.total * b.in.width(), false);
    r[5] = latok::flow_range(b.row, empty ? 0 : (n_str + 1) * 8, false);
    return kCompactFlowRanges;
}
static int flow_submit(Ctx& g, const Batch& b, uint64_t* mask, int* slot_used = nullptr) {
    if (b.n_str <= 0 || b.total <= 0) return LATOK_OK;   // an empty mask batch touches nothing
    if (!b.in.p || !b.row || !mask) return fail(LATOK_ERR_INVALID, "NULL buffer");
    if (((uintptr_t)b.in.p & 15) != 0) return fail(LATOK_ERR_INVALID, "device input pointer must be 16-byte aligned");
    latok::FlowRange r[kMaskFlowRanges];
    const FlowOpen o{.r = r, .n_r = mask_flow_ranges(b, mask, r), .units = b.total, .n_needs = kTileNeeds};
    int rc, slot = 0;
    if ((rc = flow_open(g, o, &slot))) return rc;
    if (slot_used) *slot_used = slot;
    Ctx::FlowSlot& f = g.flow[slot];
    Pipe a;
    a.b = b;
    a.bits = mask;
    a.st = f.st;
    return run_pipeline(g, f.ws, a);
}
// offsets (spans = false), token spans or token spans + feature sums (feats) of one batch: everything the blocking calls
// launch, on the slot's stream and workspace; the item total and the error flags land in result[0..1] when the stream gets there
static int flow_submit_compact(Ctx& g, bool spans, bool feats, const Batch& b, void* counts, void* items, int8_t* feat, int64_t cap,
                               int64_t* result, int flags) {
    if (!result) return fail(LATOK_ERR_INVALID, "NULL result pointer");
    if (((uintptr_t)result & 7) != 0) return fail(LATOK_ERR_INVALID, "result pointer must be 8-byte aligned");
    const int64_t n_str = b.n_str;
    const bool o32 = (flags & LATOK_OUT_INT32) != 0, empty = n_str <= 0 || b.total <= 0;
    const size_t rec = o32 ? 4 : 8;   // bytes of a count / of one field of a record
    if (!empty) {
        if (!b.in.p || !b.row || !counts || ((!items || (feats && !feat)) && cap > 0)) return fail(LATOK_ERR_INVALID, "NULL buffer");
        if (cap < 0) return fail(LATOK_ERR_INVALID, "capacity must be >= 0");
        if (feats && b.in.form == Form::Utf8)
            return fail(LATOK_ERR_INVALID, "featurize of UTF-8 bytes has calls of its own (latok_flow_token_features_utf8 / _utf8_bytes)");
        if (((uintptr_t)b.in.p & 15) != 0) return fail(LATOK_ERR_INVALID, "device input pointer must be 16-byte aligned");
        if (((uintptr_t)items & 15) != 0 || ((uintptr_t)counts & (rec - 1)) != 0) return fail(LATOK_ERR_INVALID, "misaligned output buffer");
    }
    latok::FlowRange r[kCompactFlowRanges];
    // an empty batch: counts of empty strings are zero, no items; one that launches: enqueue_compaction_dev clears its result words
    const FlowOpen o{.r = r, .n_r = compact_flow_ranges(spans, feats, b, empty, counts, items, feat, cap, result, rec, r), .empty = empty,
                     .zero = {{result, 16}, {counts, n_str > 0 ? (size_t)n_str * rec : 0}}, .units = b.total,
                     .shape = {.spans = spans, .feats = feats, .widen = feats && b.in.narrow()}};
    int rc, slot = 0;
    if ((rc = flow_open(g, o, &slot)) || empty) return rc;
    Ctx::FlowSlot& f = g.flow[slot];
    Compaction k;
    k.b = b;
    k.spans = spans;
    k.feats = feats;
    k.o32 = o32;
    k.counts = counts;
    k.items = items;
    k.feat = feat;
    k.cap = cap;
    k.p_tot = result;
    k.st = f.st;
    return enqueue_compaction_dev(g, f.ws, k);
}

int latok_flow_split_mask(const uint32_t* cps_dev, const int64_t* row_off_dev, int64_t n_str, int64_t total_chars,
                          uint64_t* mask_dev) {
    LATOK_ENTER();
    int rc = need_init(g);
    if (rc) return rc;
    if (total_chars < 0) {
        if ((rc = resolve_total_device(row_off_dev, n_str, &total_chars, g.stream))) return rc;
    }
    return flow_submit(g, Batch{Input{cps_dev, Form::Utf32}, row_off_dev, n_str, total_chars}, mask_dev);
}
int latok_flow_split_mask_kind(const void* units_dev, int kind, const int64_t* row_off_dev, int64_t n_str, int64_t total_chars,
                               uint64_t* mask_dev) {
    LATOK_ENTER();
    int rc = check_kind(kind);
    if (rc) return rc;
    if ((rc = need_init(g))) return rc;
    if (total_chars < 0) {
        if ((rc = resolve_total_device(row_off_dev, n_str, &total_chars, g.stream))) return rc;
    }
    return flow_submit(g, Batch{Input{units_dev, form_of_kind(kind)}, row_off_dev, n_str, total_chars}, mask_dev);
}
int latok_flow_split_mask_utf8_bytes(const uint8_t* utf8_dev, const int64_t* byte_off_dev, int64_t n_str, int64_t total_bytes,
                                     uint64_t* mask_dev) {
    LATOK_ENTER();
    int rc = need_init(g);
    if (rc) return rc;
    if (total_bytes < 0) {
        if ((rc = resolve_total_device(byte_off_dev, n_str, &total_bytes, g.stream))) return rc;
    }
    return flow_submit(g, Batch{Input{utf8_dev, Form::Utf8}, byte_off_dev, n_str, total_bytes}, mask_dev);
}
static int flow_compact_entry(bool spans, bool feats, const void* units_dev, int kind, const int64_t* row_off_dev, int64_t n_str,
                              int64_t total_units, void* counts_dev, void* items_dev, int8_t* features_dev, int64_t cap, int64_t* result_dev,
                              int flags) {
    LATOK_ENTER();
    int rc = need_init(g);
    if (rc) return rc;
    if ((kind != 0 || feats) && (rc = check_kind(kind))) return rc;
    if (flags & ~(LATOK_OUT_INT32 | LATOK_DEVICE_PTRS)) return fail(LATOK_ERR_INVALID, "unknown flag");
    if (total_units < 0) {
        if ((rc = resolve_total_device(row_off_dev, n_str, &total_units, g.stream))) return rc;
    }
    return flow_submit_compact(g, spans, feats, Batch{Input{units_dev, form_of_kind(kind)}, row_off_dev, n_str, total_units}, counts_dev,
                               items_dev, features_dev, cap, result_dev, flags);
}
int latok_flow_split_offsets(const void* units_dev, int kind, const int64_t* row_off_dev, int64_t n_str, int64_t total_units,
                             void* counts_dev, void* offsets_dev, int64_t offsets_cap, int64_t* result_dev, int flags) {
    return flow_compact_entry(false, false, units_dev, kind, row_off_dev, n_str, total_units, counts_dev, offsets_dev, nullptr, offsets_cap,
                              result_dev, flags);
}
int latok_flow_token_spans(const void* units_dev, int kind, const int64_t* row_off_dev, int64_t n_str, int64_t total_units,
                           void* counts_dev, void* spans_dev, int64_t spans_cap, int64_t* result_dev, int flags) {
    return flow_compact_entry(true, false, units_dev, kind, row_off_dev, n_str, total_units, counts_dev, spans_dev, nullptr, spans_cap,
                              result_dev, flags);
}
int latok_flow_token_features(const void* units_dev, int kind, const int64_t* row_off_dev, int64_t n_str, int64_t total_chars,
                              void* counts_dev, void* spans4_dev, int8_t* features_dev, int64_t cap, int64_t* result_dev, int flags) {
    return flow_compact_entry(true, true, units_dev, kind, row_off_dev, n_str, total_chars, counts_dev, spans4_dev, features_dev, cap,
                              result_dev, flags);
}
// ---- code-point results of UTF-8 batches in a flow ---------------------------------------------------------------------------
// The blocking calls (cp_masks_via_bytes) wait for the host after the lead-byte scan: the host reads the code-point total and
// the malformed-input flag and sizes everything downstream by value.  A flow batch may not wait, so here (shape 1 of DESIGN.md
// section 7, "device-resident total") the launches behind the scan are sized by the BYTE count -- a batch has at most one char
// per byte -- and read the code-point total from the word the scan wrote (latok::DeviceTotal); the malformed-input flag lands in
// result[3], gates the records and feature sums on the device and is read by the caller after latok_flow_wait.  The lead-byte
// mask, the byte-space SPACE plane, the packed code-point masks, the code-point row offsets and the rule codes are buffers of
// the slot's workspace.
enum { kU8Mask = 0, kU8Offsets = 1, kU8Spans = 2, kU8Feats = 3, kU8BytesFeats = 4 };   // (4: records in BYTE positions)
struct Utf8Flow {
    int what = kU8Mask;
    const uint8_t* u8 = nullptr;
    const int64_t* boff = nullptr;
    int64_t n_str = 0, total_bytes = 0;
    uint64_t* mask = nullptr;     // kU8Mask
    int64_t mask_cap = 0;
    int64_t* cp_row = nullptr;
    void* counts = nullptr;       // the others
    void* items = nullptr;
    int8_t* feat = nullptr;
    int64_t cap = 0;
    int64_t* result = nullptr;
    bool o32 = false;
};
constexpr int kU8FlowRanges = 8;
// the debug hooks' view of a batch's ranges, in the form latok_debug_flow_route takes them; returns n, < 0 if n_max is too small
static int export_flow_ranges(const latok::FlowRange* r, int n, uint64_t* lo, uint64_t* bytes, int* is_write, int n_max) {
    if (n > n_max) return fail(LATOK_ERR_INVALID, "need room for %d ranges", n);
    for (int i = 0; i < n; ++i) {
        lo[i] = (uint64_t)r[i].lo;
        bytes[i] = (uint64_t)(r[i].hi - r[i].lo);
        is_write[i] = r[i].write ? 1 : 0;
    }
    return n;
}
// every range of caller memory the batch touches, outputs first (what flow_hazards.h orders it by); returns their number
static int utf8_flow_ranges(const Utf8Flow& a, latok::FlowRange* r) {
    const size_t rec = a.o32 ? 4 : 8, fields = a.what >= kU8Feats ? 4 : (a.what == kU8Spans ? 2 : 1);
    const size_t n_str = (size_t)std::max<int64_t>(a.n_str, 0), bytes = (size_t)std::max<int64_t>(a.total_bytes, 0);
    // (a batch has at most one item per byte: no more of the record buffers can be written, and a huge "unbounded" capacity
    // cannot wrap the tracked length into an empty range)
    const size_t cap = std::min((size_t)std::max<int64_t>(a.cap, 0), bytes);
    int n = 0;
    r[n++] = latok::flow_range(a.result, 32, true);
    if (a.what == kU8Mask) {
        const int64_t words_b = (int64_t)((bytes + 63) / 64);
        r[n++] = latok::flow_range(a.mask, (size_t)std::max<int64_t>(std::min(a.mask_cap, words_b), 0) * 8, true);
        r[n++] = latok::flow_range(a.cp_row, n_str ? (n_str + 1) * 8 : 0, true);
    } else {
        r[n++] = latok::flow_range(a.counts, n_str * rec, true);
        r[n++] = latok::flow_range(a.items, bytes ? cap * fields * rec : 0, true);
        if (a.what >= kU8Feats) r[n++] = latok::flow_range(a.feat, bytes ? cap * LATOK_FEATURE_COUNT : 0, true);
    }
    r[n++] = latok::flow_range(a.u8, bytes, false);
    r[n++] = latok::flow_range(a.boff, n_str ? (n_str + 1) * 8 : 0, false);
    return n;
}

/* test hook (not part of the ABI; needs no device): the ranges a code-point UTF-8 flow batch notes, in the form
 * latok_debug_flow_route takes them.  what: 0 mask, 1 offsets, 2 token spans, 3 featurize, 4 featurize in byte space; addr[8] = {utf8, byte_off, mask or
 * counts, cp_row_off or records, features, result, 0, 0}; cap = mask_cap_words or the record capacity.  Returns the number of
 * ranges written to lo / bytes / is_write (at most n_max), < 0 on a bad argument. */
extern "C" int latok_debug_flow_utf8_ranges(int what, const uint64_t* addr, int64_t n_str, int64_t total_bytes, int64_t cap, int flags,
                                            uint64_t* lo, uint64_t* bytes, int* is_write, int n_max) {
    if (what < kU8Mask || what > kU8BytesFeats || !addr || !lo || !bytes || !is_write) return fail(LATOK_ERR_INVALID, "bad argument");
    Utf8Flow a;
    a.what = what;
    a.u8 = (const uint8_t*)(uintptr_t)addr[0];
    a.boff = (const int64_t*)(uintptr_t)addr[1];
    a.n_str = n_str;
    a.total_bytes = total_bytes;
    if (what == kU8Mask) {
        a.mask = (uint64_t*)(uintptr_t)addr[2];
        a.cp_row = (int64_t*)(uintptr_t)addr[3];
        a.mask_cap = cap;
    } else {
        a.counts = (void*)(uintptr_t)addr[2];
        a.items = (void*)(uintptr_t)addr[3];
        a.feat = (int8_t*)(uintptr_t)addr[4];
        a.cap = cap;
    }
    a.result = (int64_t*)(uintptr_t)addr[5];
    a.o32 = (flags & LATOK_OUT_INT32) != 0;
    latok::FlowRange r[kU8FlowRanges];
    return export_flow_ranges(r, utf8_flow_ranges(a, r), lo, bytes, is_write, n_max);
}

static int flow_submit_utf8(Ctx& g, const Utf8Flow& a) {
    if (!a.result) return fail(LATOK_ERR_INVALID, "NULL result pointer");
    if (((uintptr_t)a.result & 7) != 0) return fail(LATOK_ERR_INVALID, "result pointer must be 8-byte aligned");
    if (a.n_str < 0) return fail(LATOK_ERR_INVALID, "n_str must be >= 0");
    if (a.cap < 0 || a.mask_cap < 0) return fail(LATOK_ERR_INVALID, "capacity must be >= 0");
    const bool mask = a.what == kU8Mask, spans = a.what >= kU8Spans, feats = a.what >= kU8Feats;
    const int64_t n_str = a.n_str, total_bytes = a.total_bytes;
    const size_t rec = a.o32 ? 4 : 8;
    const bool empty = n_str == 0 || total_bytes <= 0;   // no item, no char; counts and row offsets of empty strings are zero
    if (empty) {
        if (n_str > 0 && (mask ? !a.cp_row : !a.counts)) return fail(LATOK_ERR_INVALID, "NULL buffer");
    } else {
        if (!a.u8 || !a.boff) return fail(LATOK_ERR_INVALID, "NULL buffer");
        if (((uintptr_t)a.u8 & 15) != 0) return fail(LATOK_ERR_INVALID, "device UTF-8 pointer must be 16-byte aligned");
        if (mask) {
            if (!a.cp_row || (!a.mask && a.mask_cap > 0)) return fail(LATOK_ERR_INVALID, "NULL buffer");
            if (((uintptr_t)a.mask & 7) != 0 || ((uintptr_t)a.cp_row & 7) != 0) return fail(LATOK_ERR_INVALID, "misaligned output buffer");
        } else {
            if (!a.counts || ((!a.items || (feats && !a.feat)) && a.cap > 0)) return fail(LATOK_ERR_INVALID, "NULL buffer");
            if (((uintptr_t)a.items & 15) != 0 || ((uintptr_t)a.counts & (rec - 1)) != 0) return fail(LATOK_ERR_INVALID, "misaligned output buffer");
        }
    }
    latok::FlowRange r[kU8FlowRanges];
    const FlowZero rows = mask ? FlowZero{a.cp_row, (size_t)(n_str + 1) * 8} : FlowZero{a.counts, (size_t)n_str * rec};
    const FlowOpen o{.r = r, .n_r = utf8_flow_ranges(a, r), .empty = empty, .result = {a.result, 32},
                     .zero = {n_str > 0 ? rows : FlowZero{}}, .units = total_bytes, .shape = {.spans = spans, .feats = feats, .cp_rows = n_str + 1}};
    int rc, slot = 0;
    if ((rc = flow_open(g, o, &slot)) || empty) return rc;
    Ctx::FlowSlot& f = g.flow[slot];
    Workspace& w = f.ws;
    const hipStream_t st = f.st;
    const int64_t words_b = (total_bytes + 63) / 64;
    if (a.what == kU8BytesFeats) {   // records in byte positions: the sequence the blocking call enqueues, on the slot
        Utf8BytesFeats k;
        k.b = Batch{Input{a.u8, Form::Utf8}, a.boff, n_str, total_bytes};
        k.o32 = a.o32;
        k.counts = a.counts;
        k.items = a.items;
        k.feat = a.feat;
        k.cap = a.cap;
        k.r_items = a.result;
        k.r_err = a.result + 1;
        k.r_cps = a.result + 2;
        k.r_odd = a.result + 3;
        k.st = st;
        return enqueue_utf8_bytes_features(g, w, k);
    }
    // the code-point total: word 1 of the workspace's scalars (word 0 is the item total of the second scan) and result[2]
    LeadFront p{.b = Batch{Input{a.u8, Form::Utf8}, a.boff, n_str, total_bytes}, .space = spans, .codes = feats, .r_cps = a.result + 2,
                .r_err = (int*)(a.result + 1), .r_odd = (int*)(a.result + 3), .st = st};
    if (mask) {   // straight into the caller's buffers (no mask buffer, capacity 0: the workspace's plane takes it)
        p.cpbits = a.mask;
        p.cap_words = std::min(a.mask_cap, words_b);
        p.cp_row = a.cp_row;
    }
    LeadPlanes t;
    if ((rc = enqueue_lead_front(g, w, p, &t)) || mask) return rc;
    Compaction k;
    k.b = Batch{Input{}, t.cp_row, n_str, total_bytes};   // (total: the upper bound; the stages read k.dt.total)
    k.spans = spans;
    k.feats = feats;
    k.o32 = a.o32;
    k.counts = a.counts;
    k.items = a.items;
    k.feat = a.feat;
    k.cap = a.cap;
    k.p_tot = a.result;
    k.pre_bits = t.cpbits;
    k.pre_space = t.cpspace;
    k.pre_codes = t.codes;
    k.dt = latok::DeviceTotal{t.total_cps, p.r_odd};
    k.st = st;
    return enqueue_compaction_dev(g, w, k);
}
static int flow_utf8_entry(Utf8Flow a, int flags) {
    LATOK_ENTER();
    int rc = need_init(g);
    if (rc) return rc;
    if (flags & ~(LATOK_OUT_INT32 | LATOK_DEVICE_PTRS)) return fail(LATOK_ERR_INVALID, "unknown flag");
    a.o32 = (flags & LATOK_OUT_INT32) != 0;
    if (a.total_bytes < 0 && (rc = resolve_total_device(a.boff, a.n_str, &a.total_bytes, g.stream))) return rc;
    return flow_submit_utf8(g, a);
}
int latok_flow_split_mask_utf8(const uint8_t* utf8_dev, const int64_t* byte_off_dev, int64_t n_str, int64_t total_bytes,
                               uint64_t* mask_dev, int64_t mask_cap_words, int64_t* cp_row_off_dev, int64_t* result_dev) {
    Utf8Flow a;
    a.what = kU8Mask; a.u8 = utf8_dev; a.boff = byte_off_dev; a.n_str = n_str; a.total_bytes = total_bytes;
    a.mask = mask_dev; a.mask_cap = mask_cap_words; a.cp_row = cp_row_off_dev; a.result = result_dev;
    return flow_utf8_entry(a, 0);
}
static int flow_utf8_compact_entry(int what, const uint8_t* utf8_dev, const int64_t* byte_off_dev, int64_t n_str, int64_t total_bytes,
                                   void* counts_dev, void* items_dev, int8_t* features_dev, int64_t cap, int64_t* result_dev, int flags) {
    Utf8Flow a;
    a.what = what; a.u8 = utf8_dev; a.boff = byte_off_dev; a.n_str = n_str; a.total_bytes = total_bytes;
    a.counts = counts_dev; a.items = items_dev; a.feat = features_dev; a.cap = cap; a.result = result_dev;
    return flow_utf8_entry(a, flags);
}
int latok_flow_split_offsets_utf8(const uint8_t* utf8_dev, const int64_t* byte_off_dev, int64_t n_str, int64_t total_bytes,
                                  void* counts_dev, void* offsets_dev, int64_t offsets_cap, int64_t* result_dev, int flags) {
    return flow_utf8_compact_entry(kU8Offsets, utf8_dev, byte_off_dev, n_str, total_bytes, counts_dev, offsets_dev, nullptr, offsets_cap,
                                   result_dev, flags);
}
int latok_flow_token_spans_utf8(const uint8_t* utf8_dev, const int64_t* byte_off_dev, int64_t n_str, int64_t total_bytes,
                                void* counts_dev, void* spans_dev, int64_t spans_cap, int64_t* result_dev, int flags) {
    return flow_utf8_compact_entry(kU8Spans, utf8_dev, byte_off_dev, n_str, total_bytes, counts_dev, spans_dev, nullptr, spans_cap, result_dev,
                                   flags);
}
int latok_flow_token_features_utf8(const uint8_t* utf8_dev, const int64_t* byte_off_dev, int64_t n_str, int64_t total_bytes,
                                   void* counts_dev, void* spans4_dev, int8_t* features_dev, int64_t cap, int64_t* result_dev, int flags) {
    return flow_utf8_compact_entry(kU8Feats, utf8_dev, byte_off_dev, n_str, total_bytes, counts_dev, spans4_dev, features_dev, cap,
                                   result_dev, flags);
}
int latok_flow_token_features_utf8_bytes(const uint8_t* utf8_dev, const int64_t* byte_off_dev, int64_t n_str, int64_t total_bytes,
                                         void* counts_dev, void* spans4_dev, int8_t* features_dev, int64_t cap, int64_t* result_dev, int flags) {
    return flow_utf8_compact_entry(kU8BytesFeats, utf8_dev, byte_off_dev, n_str, total_bytes, counts_dev, spans4_dev, features_dev, cap,
                                   result_dev, flags);
}
// ---- byte-space token batches in a flow: the checks ahead of flow_open ---------------------------------------------------------
// What the join entry and the hash / id entry check alike once their own flag check, need_init and object checks are done (each
// keeps those, in its own order): the counts, the payload pointer `out` against its capacity (named in the message), the result
// pointer, the outputs' alignment ({pointer, mask} pairs; a NULL pointer is aligned), then the total -- read on the context's
// stream when the caller passed a negative one -- and, for a batch that is not empty, its two inputs.
struct PtrMask {
    const void* p;
    size_t mask;
};
static int flow_bytes_checks(Ctx& g, const uint8_t* utf8_dev, const int64_t* byte_off_dev, int64_t n_str, int64_t* total_io, const void* out,
                             int64_t cap, const char* out_name, const char* cap_name, const int64_t* result_dev,
                             std::initializer_list<PtrMask> outputs, bool* empty) {
    int rc;
    if (n_str < 0) return fail(LATOK_ERR_INVALID, "n_str must be >= 0");
    if (cap < 0) return fail(LATOK_ERR_INVALID, "capacity must be >= 0");
    if (!out && cap > 0) return fail(LATOK_ERR_INVALID, "%s is NULL but %s > 0 (a size query passes %s = 0)", out_name, cap_name, cap_name);
    if (!result_dev) return fail(LATOK_ERR_INVALID, "NULL result pointer");
    if (((uintptr_t)result_dev & 7) != 0) return fail(LATOK_ERR_INVALID, "result pointer must be 8-byte aligned");
    for (const PtrMask& o : outputs)
        if (((uintptr_t)o.p & o.mask) != 0) return fail(LATOK_ERR_INVALID, "misaligned output buffer");
    if (*total_io < 0 && (rc = resolve_total_device(byte_off_dev, n_str, total_io, g.stream))) return rc;
    *empty = n_str == 0 || *total_io <= 0;
    if (!*empty) {
        if (!utf8_dev || !byte_off_dev) return fail(LATOK_ERR_INVALID, "NULL buffer");
        if (((uintptr_t)utf8_dev & 15) != 0) return fail(LATOK_ERR_INVALID, "device UTF-8 pointer must be 16-byte aligned");
    }
    return LATOK_OK;
}

// ---- joined token text in a flow -----------------------------------------------------------------------------------------------
constexpr int kJoinFlowRanges = 6;
// every range of caller memory the batch touches, outputs first; returns their number.  The tracked output length is what can be
// written at most -- min(out_cap, 2 * total_bytes) --, so a huge "unbounded" capacity cannot wrap it into an empty range.
static int join_flow_ranges(const uint8_t* u8, const int64_t* boff, int64_t n_str_in, int64_t total_bytes, uint8_t* out, int64_t cap,
                            int64_t* out_off, void* counts, int64_t* result, bool o32, latok::FlowRange* r) {
    const size_t n_str = (size_t)std::max<int64_t>(n_str_in, 0), bytes = (size_t)std::max<int64_t>(total_bytes, 0);
    const size_t out_len = std::min((size_t)std::max<int64_t>(cap, 0), 2 * bytes);
    int n = 0;
    r[n++] = latok::flow_range(result, 16, true);
    r[n++] = latok::flow_range(out, out_len, true);
    r[n++] = latok::flow_range(out_off, (n_str + 1) * 8, true);
    r[n++] = latok::flow_range(counts, n_str * (o32 ? 4 : 8), true);
    r[n++] = latok::flow_range(u8, bytes, false);
    r[n++] = latok::flow_range(boff, n_str ? (n_str + 1) * 8 : 0, false);
    return n;
}

/* test hook (not part of the ABI; needs no device): the ranges a join batch of a flow notes, in the form latok_debug_flow_route
 * takes them.  addr[6] = {utf8, byte_off, out_bytes, out_off, counts, result}.  Returns the number of ranges written to lo / bytes /
 * is_write (at most n_max), < 0 on a bad argument. */
extern "C" int latok_debug_flow_join_ranges(const uint64_t* addr, int64_t n_str, int64_t total_bytes, int64_t cap, int flags, uint64_t* lo,
                                            uint64_t* bytes, int* is_write, int n_max) {
    if (!addr || !lo || !bytes || !is_write) return fail(LATOK_ERR_INVALID, "bad argument");
    latok::FlowRange r[kJoinFlowRanges];
    const int n = join_flow_ranges((const uint8_t*)(uintptr_t)addr[0], (const int64_t*)(uintptr_t)addr[1], n_str, total_bytes,
                                   (uint8_t*)(uintptr_t)addr[2], cap, (int64_t*)(uintptr_t)addr[3], (void*)(uintptr_t)addr[4],
                                   (int64_t*)(uintptr_t)addr[5], (flags & LATOK_OUT_INT32) != 0, r);
    return export_flow_ranges(r, n, lo, bytes, is_write, n_max);
}

int latok_flow_join_tokens_utf8_bytes(const uint8_t* utf8_dev, const int64_t* byte_off_dev, int64_t n_str, int64_t total_bytes, int sep,
                                      uint8_t* out_bytes_dev, int64_t out_cap, int64_t* out_off_dev, void* counts_dev, int64_t* result_dev,
                                      int flags) {
    LATOK_ENTER();
    if (sep < 0 || sep > 255) return fail(LATOK_ERR_INVALID, "sep must be one byte (0..255), got %d", sep);
    int rc = need_init(g);
    if (rc) return rc;
    if (flags & ~(LATOK_OUT_INT32 | LATOK_DEVICE_PTRS)) return fail(LATOK_ERR_INVALID, "unknown flag");
    if (!out_off_dev) return fail(LATOK_ERR_INVALID, "out_off is NULL");
    const bool o32 = (flags & LATOK_OUT_INT32) != 0;
    const size_t rec = o32 ? 4 : 8;
    bool empty = false;   // empty rows
    if ((rc = flow_bytes_checks(g, utf8_dev, byte_off_dev, n_str, &total_bytes, out_bytes_dev, out_cap, "out_bytes", "out_cap", result_dev,
                                {{out_off_dev, 7}, {counts_dev, rec - 1}}, &empty)))
        return rc;
    latok::FlowRange r[kJoinFlowRanges];
    const int n_r = join_flow_ranges(utf8_dev, byte_off_dev, n_str, total_bytes, out_bytes_dev, out_cap, out_off_dev, counts_dev, result_dev, o32, r);
    const FlowOpen o{.r = r, .n_r = n_r, .empty = empty, .result = {result_dev, 16},
                     .zero = {{out_off_dev, (size_t)(n_str + 1) * 8}, {counts_dev, (size_t)n_str * rec}}, .units = total_bytes,
                     .shape = {.spans = true, .join = true}};
    int slot = 0;
    if ((rc = flow_open(g, o, &slot)) || empty) return rc;
    Ctx::FlowSlot& f = g.flow[slot];
    JoinTokens a;
    a.b = Batch{Input{utf8_dev, Form::Utf8}, byte_off_dev, n_str, total_bytes};
    a.sep = sep;
    a.out = out_bytes_dev;
    a.cap = out_bytes_dev ? std::min(out_cap, 2 * total_bytes) : 0;
    a.out_off = out_off_dev;
    a.counts = counts_dev;
    a.o32 = o32;
    a.r_bytes = result_dev;
    a.r_err = result_dev + 1;
    a.st = f.st;
    return enqueue_join_tokens(g, f.ws, a);
}

// ---- token hashes and token ids in a flow -------------------------------------------------------------------------------------
constexpr int kHashFlowRanges = 6;
// every range of caller memory the batch touches, outputs first; returns their number.  The tracked length of the hashes and of
// the records is what can be written at most -- min(cap, total_bytes) tokens, a token has at least one byte --, so a huge
// "unbounded" capacity cannot wrap a range into an empty one.
static int hash_flow_ranges(const uint8_t* u8, const int64_t* boff, int64_t n_str_in, int64_t total_bytes, void* counts, void* spans,
                            void* hashes, int64_t cap, int64_t* result, bool o32, latok::FlowRange* r) {
    const size_t n_str = (size_t)std::max<int64_t>(n_str_in, 0), bytes = (size_t)std::max<int64_t>(total_bytes, 0);
    const size_t tokens = std::min((size_t)std::max<int64_t>(cap, 0), bytes), rec = o32 ? 4 : 8;
    int n = 0;
    r[n++] = latok::flow_range(result, 16, true);
    r[n++] = latok::flow_range(hashes, tokens * 4, true);
    r[n++] = latok::flow_range(spans, tokens * 2 * rec, true);
    r[n++] = latok::flow_range(counts, n_str * rec, true);
    r[n++] = latok::flow_range(u8, bytes, false);
    r[n++] = latok::flow_range(boff, n_str ? (n_str + 1) * 8 : 0, false);
    return n;
}

/* test hooks (not part of the ABI; need no device): the ranges a token-hash or token-id batch of a flow notes, in the form
 * latok_debug_flow_route takes them.  addr[6] = {utf8, byte_off, counts, spans, hashes or ids, result}: the ranges are the same with
 * the ids in the hashes' place (both are 4 bytes per token); the vocabulary table is library-owned read-only memory and is not
 * tracked.  Returns the number of ranges written to lo / bytes / is_write (at most n_max), < 0 on a bad argument. */
extern "C" int latok_debug_flow_hashes_ranges(const uint64_t* addr, int64_t n_str, int64_t total_bytes, int64_t cap, int flags, uint64_t* lo,
                                              uint64_t* bytes, int* is_write, int n_max) {
    if (!addr || !lo || !bytes || !is_write) return fail(LATOK_ERR_INVALID, "bad argument");
    latok::FlowRange r[kHashFlowRanges];
    const int n = hash_flow_ranges((const uint8_t*)(uintptr_t)addr[0], (const int64_t*)(uintptr_t)addr[1], n_str, total_bytes,
                                   (void*)(uintptr_t)addr[2], (void*)(uintptr_t)addr[3], (void*)(uintptr_t)addr[4], cap,
                                   (int64_t*)(uintptr_t)addr[5], (flags & LATOK_OUT_INT32) != 0, r);
    return export_flow_ranges(r, n, lo, bytes, is_write, n_max);
}
extern "C" int latok_debug_flow_ids_ranges(const uint64_t* addr, int64_t n_str, int64_t total_bytes, int64_t cap, int flags, uint64_t* lo,
                                           uint64_t* bytes, int* is_write, int n_max) {
    return latok_debug_flow_hashes_ranges(addr, n_str, total_bytes, cap, flags, lo, bytes, is_write, n_max);
}

// the two flow entry points' shared body: ids = the batch takes a vocabulary
static int flow_token_words(const uint8_t* utf8_dev, const int64_t* byte_off_dev, int64_t n_str, int64_t total_bytes, bool ids,
                            const latok_vocab* vocab, uint32_t seed, int32_t unk_id, void* counts_dev, void* spans_dev, void* words_dev, int64_t cap,
                            int64_t* result_dev, int flags) {
    LATOK_ENTER();
    if (flags & ~(LATOK_OUT_INT32 | LATOK_DEVICE_PTRS)) return fail(LATOK_ERR_INVALID, "unknown flag");
    int rc = need_init(g);
    if (rc) return rc;
    const Vocab* v = nullptr;
    if (ids && (rc = check_object(g, vocab, "vocab is NULL", &v))) return rc;
    const bool o32 = (flags & LATOK_OUT_INT32) != 0;
    const size_t rec = o32 ? 4 : 8;
    bool empty = false;   // no token
    if ((rc = flow_bytes_checks(g, utf8_dev, byte_off_dev, n_str, &total_bytes, words_dev, cap, ids ? "ids" : "hashes", "cap", result_dev,
                                {{spans_dev, 2 * rec - 1}, {counts_dev, rec - 1}, {words_dev, 3}}, &empty)))
        return rc;
    latok::FlowRange r[kHashFlowRanges];
    const int n_r = hash_flow_ranges(utf8_dev, byte_off_dev, n_str, total_bytes, counts_dev, spans_dev, words_dev, cap, result_dev, o32, r);
    const FlowOpen o{.r = r, .n_r = n_r, .empty = empty, .result = {result_dev, 16}, .zero = {{counts_dev, (size_t)n_str * rec}},
                     .units = total_bytes, .shape = {.spans = true}};
    int slot = 0;
    if ((rc = flow_open(g, o, &slot)) || empty) return rc;
    Ctx::FlowSlot& f = g.flow[slot];
    TokenWords a;
    a.b = Batch{Input{utf8_dev, Form::Utf8}, byte_off_dev, n_str, total_bytes};
    a.vocab = v;
    a.seed = seed;
    a.unk = unk_id;
    a.counts = counts_dev;
    a.spans = spans_dev;
    a.words = words_dev;
    a.cap = words_dev ? std::min(cap, total_bytes) : 0;
    a.o32 = o32;
    a.r_tokens = result_dev;
    a.r_err = result_dev + 1;
    a.st = f.st;
    return enqueue_token_words(g, f.ws, a);
}
int latok_flow_token_hashes_utf8_bytes(const uint8_t* utf8_dev, const int64_t* byte_off_dev, int64_t n_str, int64_t total_bytes, uint32_t seed,
                                       void* counts_dev, void* spans_dev, uint32_t* hashes_dev, int64_t cap, int64_t* result_dev, int flags) {
    return flow_token_words(utf8_dev, byte_off_dev, n_str, total_bytes, false, nullptr, seed, -1, counts_dev, spans_dev, hashes_dev, cap, result_dev,
                            flags);
}
int latok_flow_token_ids_utf8_bytes(const uint8_t* utf8_dev, const int64_t* byte_off_dev, int64_t n_str, int64_t total_bytes,
                                    const latok_vocab* vocab, int32_t unk_id, void* counts_dev, void* spans_dev, int32_t* ids_dev, int64_t cap,
                                    int64_t* result_dev, int flags) {
    return flow_token_words(utf8_dev, byte_off_dev, n_str, total_bytes, true, vocab, 0, unk_id, counts_dev, spans_dev, ids_dev, cap, result_dev, flags);
}

int latok_flow_wait(void) {
    LATOK_ENTER();
    int rc = need_init(g);
    if (rc) return rc;
    return flow_drain(g);
}

int latok_bench_stream_read(const void* buf_dev, int64_t bytes, int warmup, int iters, float* ms_out) {
    LATOK_ENTER();
    int rc = need_init(g);
    if (rc) return rc;
    if (!buf_dev || !ms_out || bytes < 16384 || iters <= 0 || warmup < 0)
        return fail(LATOK_ERR_INVALID, "stream_read: need a device buffer of >= 16 KiB, iters > 0");
    if (((uintptr_t)buf_dev & 15) != 0) return fail(LATOK_ERR_INVALID, "device pointer must be 16-byte aligned");
    StreamTurn turn(g, nullptr);
    hipStream_t st = turn.st;
    uint32_t* sink = (uint32_t*)g.ws.scalar.p + 8;
    for (int i = 0; i < warmup; ++i) HIP_TRY(latok::launch_stream_read(buf_dev, bytes, sink, g.n_cu, st));
    HIP_TRY(hipEventRecord(g.ev[0], st));
    for (int i = 0; i < iters; ++i) HIP_TRY(latok::launch_stream_read(buf_dev, bytes, sink, g.n_cu, st));
    HIP_TRY(hipEventRecord(g.ev[1], st));
    HIP_TRY(hipEventSynchronize(g.ev[1]));
    HIP_TRY(hipEventElapsedTime(ms_out, g.ev[0], g.ev[1]));
    return LATOK_OK;
}

int latok_bench_split_mask(const uint32_t* cps_dev, const int64_t* row_off_dev, int64_t n_str, int64_t total,
                           uint64_t* mask_dev, int warmup, int iters, float* ms_total_out, float* ms_tiles_out,
                           int64_t* n_fix_tiles_out) {
    LATOK_ENTER();
    int rc = need_init(g);
    if (rc) return rc;
    if (iters < 0 || warmup < 0) return fail(LATOK_ERR_INVALID, "iters and warmup must be >= 0");
    if (((uintptr_t)cps_dev & 15) != 0) return fail(LATOK_ERR_INVALID, "device cps pointer must be 16-byte aligned");
    StreamTurn turn(g, nullptr);
    hipStream_t st = turn.st;
    if ((rc = resolve_total_device(row_off_dev, n_str, &total, st))) return rc;
    Pipe a;
    a.b = Batch{Input{cps_dev, Form::Utf32}, row_off_dev, n_str, total};
    a.bits = mask_dev;
    a.st = st;
    Pipe tiles = a;   // stage 2 alone
    tiles.stages = 2;
    for (int i = 0; i < warmup; ++i)
        if ((rc = run_pipeline(g, g.ws, a))) return rc;
    // (1) whole pipeline, `iters` passes between one pair of events on the launch stream
    if (ms_total_out) {
        HIP_TRY(hipEventRecord(g.ev[0], st));
        for (int i = 0; i < iters; ++i)
            if ((rc = run_pipeline(g, g.ws, a))) return rc;
        HIP_TRY(hipEventRecord(g.ev[1], st));
        HIP_TRY(hipEventSynchronize(g.ev[1]));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, g.ev[0], g.ev[1]));
        *ms_total_out = ms;
    }
    // (2) the dominant kernel alone: `iters` launches of stage 1 back to back between ONE pair of events (the kernel is
    //     idempotent: it reads the code points, row_off and the tile index of the batch, which stage 0 left in place, and
    //     rewrites the same provisional bitmask and summaries).  An event pair around every launch inside the pipeline
    //     charges each interval with the markers' own dispatch, ~6 us per launch (rocprofv3 kernel trace of such a run:
    //     5.8 us of idle queue in front of every k_tiles_main, 102 us by events against 96 us kernel time).
    if (ms_tiles_out) {
        HIP_TRY(hipEventRecord(g.ev[2], st));
        for (int i = 0; i < iters; ++i)
            if ((rc = run_pipeline(g, g.ws, tiles))) return rc;
        HIP_TRY(hipEventRecord(g.ev[3], st));
        HIP_TRY(hipEventSynchronize(g.ev[3]));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, g.ev[2], g.ev[3]));
        *ms_tiles_out = ms;
        // leave a resolved mask behind
        if ((rc = run_pipeline(g, g.ws, a))) return rc;
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (n_fix_tiles_out) {
        *n_fix_tiles_out = 0;
        if (total > 0) HIP_TRY(hipMemcpy(n_fix_tiles_out, g.ws.fix_count.p, 8, hipMemcpyDeviceToHost));
    }
    return LATOK_OK;
}


// ---- several contexts timed as one job ---------------------------------------------------------------------------------
}  // extern "C"
struct latok_gate {
    int parties = 1;
    std::atomic<int> arrived{0};
    std::atomic<unsigned> phase{0};
    std::atomic<bool> broken{false};
    std::atomic<unsigned> ready{0};      // shared gates: kGateReady once the creator has finished setting the object up
};
constexpr unsigned kGateReady = 0x6A7E0001u;
extern "C" {

int latok_gate_create(int parties, latok_gate** gate_out) {
    if (parties < 1 || !gate_out) return fail(LATOK_ERR_INVALID, "gate: parties must be >= 1");
    latok_gate* g = new (std::nothrow) latok_gate;
    if (!g) return fail(LATOK_ERR_NOMEM, "out of host memory");
    g->parties = parties;
    *gate_out = g;
    return LATOK_OK;
}
int latok_gate_destroy(latok_gate* gate) {
    delete gate;
    return LATOK_OK;
}
static int gate_map_shared(const char* name, bool create, int parties, latok_gate** gate_out) {
    if (!name || name[0] != '/' || !gate_out) return fail(LATOK_ERR_INVALID, "gate: shared name must start with '/'");
    const int fd = shm_open(name, create ? (O_CREAT | O_EXCL | O_RDWR) : O_RDWR, 0600);
    if (fd < 0) return fail(LATOK_ERR_INVALID, "gate: shm_open(%s) failed: %s", name, strerror(errno));
    if (create && ftruncate(fd, (off_t)sizeof(latok_gate)) != 0) {
        close(fd);
        shm_unlink(name);
        return fail(LATOK_ERR_NOMEM, "gate: ftruncate failed: %s", strerror(errno));
    }
    if (!create) {
        // the creator may be between shm_open and ftruncate (a zero-length object: touching the mapping would be SIGBUS) or
        // before its placement-new: attach only to an object of full size whose `ready` word says it is set up
        struct stat sb;
        if (fstat(fd, &sb) != 0 || sb.st_size < (off_t)sizeof(latok_gate)) {
            close(fd);
            return fail(LATOK_ERR_INVALID, "gate: %s is not ready yet", name);
        }
    }
    void* p = mmap(nullptr, sizeof(latok_gate), PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    close(fd);
    if (p == MAP_FAILED) return fail(LATOK_ERR_NOMEM, "gate: mmap failed: %s", strerror(errno));
    latok_gate* g;
    if (create) {
        g = new (p) latok_gate;
        g->parties = parties;
        g->ready.store(kGateReady, std::memory_order_release);      // last: everything above is visible to whoever sees it
    } else {
        g = reinterpret_cast<latok_gate*>(p);
        if (g->ready.load(std::memory_order_acquire) != kGateReady) {
            munmap(p, sizeof(latok_gate));
            return fail(LATOK_ERR_INVALID, "gate: %s is not ready yet", name);
        }
    }
    *gate_out = g;
    return LATOK_OK;
}
int latok_gate_create_shared(const char* name, int parties, latok_gate** gate_out) {
    if (parties < 1) return fail(LATOK_ERR_INVALID, "gate: parties must be >= 1");
    return gate_map_shared(name, true, parties, gate_out);
}
int latok_gate_attach_shared(const char* name, latok_gate** gate_out) { return gate_map_shared(name, false, 0, gate_out); }
int latok_gate_detach_shared(latok_gate* gate) {
    if (gate) munmap(gate, sizeof(latok_gate));
    return LATOK_OK;
}
int latok_gate_unlink_shared(const char* name) {
    if (name) shm_unlink(name);
    return LATOK_OK;
}
int latok_gate_break(latok_gate* gate) {
    if (gate) gate->broken.store(true, std::memory_order_release);
    return LATOK_OK;
}
int latok_gate_wait(latok_gate* gate, double timeout_s) {
    if (!gate) return LATOK_OK;
    if (gate->broken.load(std::memory_order_acquire)) return fail(LATOK_ERR_INVALID, "gate: broken by another party");
    const unsigned ph = gate->phase.load(std::memory_order_acquire);
    if (gate->arrived.fetch_add(1, std::memory_order_acq_rel) + 1 == gate->parties) {   // last one in opens the gate
        gate->arrived.store(0, std::memory_order_relaxed);
        gate->phase.store(ph + 1, std::memory_order_release);
        return LATOK_OK;
    }
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spins = 0;; ++spins) {
        if (gate->phase.load(std::memory_order_acquire) != ph) return LATOK_OK;
        if (gate->broken.load(std::memory_order_acquire)) return fail(LATOK_ERR_INVALID, "gate: broken by another party");
        cpu_relax();
        if ((spins & 1023) == 1023) {
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s)
                return fail(LATOK_ERR_INVALID, "gate: %d parties expected, not all arrived within %.1f s", gate->parties, timeout_s);
            std::this_thread::yield();   // more host threads than cores (rehearsals): let the others arrive
        }
    }
}

static inline int64_t mono_ns() {
    return (int64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

static thread_local int tl_bench_used_graph = 0;
/* measurement aid (not part of the ABI in include/latok_hip.h): 1 when this thread's last latok_bench_split_mask_gated replayed
 * a captured hipGraph (LATOK_BENCH_GRAPH=1 and the capture succeeded), 0 when it launched the passes one by one */
int latok_debug_bench_used_graph(void) { return tl_bench_used_graph; }

int latok_bench_split_mask_gated(const uint32_t* cps_dev, const int64_t* row_off_dev, int64_t n_str, int64_t total,
                                 uint64_t* mask_dev, int iters, latok_gate* gate, float* ms_events_out, int64_t* t0_ns_out,
                                 int64_t* t1_ns_out) {
    LATOK_ENTER();
    tl_bench_used_graph = 0;
    int rc = need_init(g);
    if (rc) return rc;
    if (iters < 1) return fail(LATOK_ERR_INVALID, "iters must be >= 1");
    if (((uintptr_t)cps_dev & 15) != 0) return fail(LATOK_ERR_INVALID, "device cps pointer must be 16-byte aligned");
    StreamTurn turn(g, nullptr);
    hipStream_t st = turn.st;
    if ((rc = resolve_total_device(row_off_dev, n_str, &total, st))) return rc;
    Pipe a;
    a.b = Batch{Input{cps_dev, Form::Utf32}, row_off_dev, n_str, total};
    a.bits = mask_dev;
    a.st = st;
    // LATOK_BENCH_GRAPH=1 (bench.py --launch threads, N > 1): the K passes are captured into ONE hipGraph outside the
    // timed region and replayed by one call inside it -- with N host threads of one process launching 3 kernels per 0.1 ms
    // step each, the threads would otherwise meet in the runtime's launch path.  Same kernels, same order, same stream.
    hipGraph_t graph = nullptr;
    hipGraphExec_t gexec = nullptr;
    {
        const char* e = getenv("LATOK_BENCH_GRAPH");
        if (e && e[0] == '1') {
            // (the workspaces are sized by the caller's warm-up passes; one eager pass here makes sure of it: nothing may
            // allocate during a capture)
            if ((rc = run_pipeline(g, g.ws, a))) return rc;
            HIP_TRY(hipStreamSynchronize(st));
            if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess) {
                for (int i = 0; i < iters && !rc; ++i)
                    rc = run_pipeline(g, g.ws, a);
                hipError_t ce = hipStreamEndCapture(st, &graph);
                if (!rc && ce == hipSuccess && graph) ce = hipGraphInstantiate(&gexec, graph, nullptr, nullptr, 0);
                if (rc || ce != hipSuccess || !gexec) {      // no graph on this runtime: the eager form below
                    if (gexec) (void)hipGraphExecDestroy(gexec);
                    if (graph) (void)hipGraphDestroy(graph);
                    graph = nullptr;
                    gexec = nullptr;
                    rc = LATOK_OK;
                    (void)hipGetLastError();
                }
            }
        }
    }
    HIP_TRY(hipStreamSynchronize(st));
    if ((rc = latok_gate_wait(gate, 120.0))) {
        if (gexec) (void)hipGraphExecDestroy(gexec);
        if (graph) (void)hipGraphDestroy(graph);
        return rc;
    }
    const int64_t t0 = mono_ns();
    HIP_TRY(hipEventRecord(g.ev[0], st));
    if (gexec) {
        tl_bench_used_graph = 1;
        if (hipGraphLaunch(gexec, st) != hipSuccess) rc = fail(LATOK_ERR_HIP, "hipGraphLaunch failed");
    } else {
        for (int i = 0; i < iters; ++i)
            if ((rc = run_pipeline(g, g.ws, a))) break;
    }
    if (!rc) {
        hipError_t e = hipEventRecord(g.ev[1], st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) rc = fail(LATOK_ERR_HIP, "timed region failed: %s", hipGetErrorString(e));
    }
    const int64_t t1 = mono_ns();
    const int rc_gate = latok_gate_wait(gate, 120.0);   // also on failure: the other threads must not wait for this one
    if (gexec) (void)hipGraphExecDestroy(gexec);
    if (graph) (void)hipGraphDestroy(graph);
    if (rc) return rc;
    if (rc_gate) return rc_gate;
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, g.ev[0], g.ev[1]));
    if (ms_events_out) *ms_events_out = ms;
    if (t0_ns_out) *t0_ns_out = t0;
    if (t1_ns_out) *t1_ns_out = t1;
    return LATOK_OK;
}

int latok_bench_split_mask_flow_gated(const uint32_t* cps_dev, const int64_t* row_off_dev, int64_t n_str, int64_t total,
                                      uint64_t* mask_a_dev, uint64_t* mask_b_dev, int iters, latok_gate* gate,
                                      float* ms_events_out, int64_t* t0_ns_out, int64_t* t1_ns_out) {
    LATOK_ENTER();
    int rc = need_init(g);
    if (rc) return rc;
    if (iters < 1) return fail(LATOK_ERR_INVALID, "iters must be >= 1");
    if (!mask_a_dev || !mask_b_dev) return fail(LATOK_ERR_INVALID, "NULL buffer");
    if ((rc = resolve_total_device(row_off_dev, n_str, &total, g.stream))) return rc;
    if ((rc = flow_setup(g)) || (rc = flow_drain(g))) return rc;
    HIP_TRY(hipStreamSynchronize(g.stream));
    if ((rc = latok_gate_wait(gate, 120.0))) return rc;
    const int64_t t0 = mono_ns();
    HIP_TRY(hipEventRecord(g.ev[0], g.flow[g.flow_seq % (unsigned)g.flow_slots].st));   // the stream of the first submission
    int last_slot = 0;
    const uint32_t* cps_b = g.bench_cps_b ? g.bench_cps_b : cps_dev;     // (latok_bench_set_second_input: a copy at another address)
    const int64_t* row_b = g.bench_row_b ? g.bench_row_b : row_off_dev;
    for (int i = 0; i < iters; ++i)
        if ((rc = flow_submit(g, Batch{Input{(i & 1) ? cps_b : cps_dev, Form::Utf32}, (i & 1) ? row_b : row_off_dev, n_str, total},
                              (i & 1) ? mask_b_dev : mask_a_dev, &last_slot)))
            break;
    if (!rc) {
        hipError_t e = hipEventRecord(g.ev[1], g.flow[last_slot].st);   // ... of the last one
        if (e != hipSuccess) rc = fail(LATOK_ERR_HIP, "timed region failed: %s", hipGetErrorString(e));
    }
    const int rc_drain = flow_drain(g);
    const int64_t t1 = mono_ns();
    const int rc_gate = latok_gate_wait(gate, 120.0);   // also on failure: the other ranks must not wait for this one
    if (rc) return rc;
    if (rc_drain) return rc_drain;
    if (rc_gate) return rc_gate;
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, g.ev[0], g.ev[1]));
    if (ms_events_out) *ms_events_out = ms;
    if (t0_ns_out) *t0_ns_out = t0;
    if (t1_ns_out) *t1_ns_out = t1;
    return LATOK_OK;
}

int latok_bench_set_second_input(const uint32_t* cps_b_dev, const int64_t* row_off_b_dev) {
    LATOK_ENTER();
    if ((cps_b_dev == nullptr) != (row_off_b_dev == nullptr)) return fail(LATOK_ERR_INVALID, "both pointers or neither");
    if (((uintptr_t)cps_b_dev & 15) != 0) return fail(LATOK_ERR_INVALID, "device cps pointer must be 16-byte aligned");
    g.bench_cps_b = cps_b_dev;
    g.bench_row_b = row_off_b_dev;
    return LATOK_OK;
}

int latok_bench_tiles_flow(const uint32_t* cps_dev, const int64_t* row_off_dev, int64_t n_str, int64_t total, uint64_t* mask_a_dev,
                           uint64_t* mask_b_dev, int iters, float* ms_out) {
    LATOK_ENTER();
    int rc = need_init(g);
    if (rc) return rc;
    if (iters < 1 || !ms_out || !mask_a_dev || !mask_b_dev) return fail(LATOK_ERR_INVALID, "iters >= 1, two mask buffers and ms_out are needed");
    if ((rc = resolve_total_device(row_off_dev, n_str, &total, g.stream))) return rc;
    if (total <= 0) { *ms_out = 0.f; return LATOK_OK; }
    // one whole pass per slot first: workspaces sized, the per-tile string index of the batch in place in BOTH slots
    const uint32_t* cps_b = g.bench_cps_b ? g.bench_cps_b : cps_dev;
    const int64_t* row_b = g.bench_row_b ? g.bench_row_b : row_off_dev;
    int slot_of[2] = {0, 1};
    for (int i = 0; i < 2; ++i)
        if ((rc = flow_submit(g, Batch{Input{i ? cps_b : cps_dev, Form::Utf32}, i ? row_b : row_off_dev, n_str, total}, i ? mask_b_dev : mask_a_dev,
                              &slot_of[i])))
            return rc;
    if ((rc = flow_drain(g))) return rc;
    const int64_t t0 = mono_ns();
    for (int i = 0; i < iters && !rc; ++i) {
        Ctx::FlowSlot& f = g.flow[slot_of[i & 1]];
        Pipe a;
        a.b = Batch{Input{(i & 1) ? cps_b : cps_dev, Form::Utf32}, (i & 1) ? row_b : row_off_dev, n_str, total};
        a.bits = (i & 1) ? mask_b_dev : mask_a_dev;
        a.stages = 2;
        a.st = f.st;
        rc = run_pipeline(g, f.ws, a);
    }
    const int rc_drain = flow_drain(g);
    const int64_t t1 = mono_ns();
    if (rc) return rc;
    if (rc_drain) return rc_drain;
    *ms_out = (float)((t1 - t0) / 1e6);
    // leave resolved masks behind
    for (int i = 0; i < 2; ++i)
        if ((rc = flow_submit(g, Batch{Input{cps_dev, Form::Utf32}, row_off_dev, n_str, total}, i ? mask_b_dev : mask_a_dev))) return rc;
    return flow_drain(g);
}

}  // extern "C"
