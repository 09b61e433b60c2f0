#!/usr/bin/env python3
"""Measurement of the SURVEY 8(f) rows on device-resident data: one JSON line per path.

  mask            latok_split_mask_batch            (the north-star path; here for reference, bench.py is the contract)
  offsets         latok_split_offsets_batch         (8f-1: np.nonzero per string)
  spans           latok_token_spans_batch           (8f-1: slice / strip / drop-empty)
  features        latok_token_features_batch        (8f-2: featurize)
  utf8_mask       latok_split_mask_utf8_batch       (8f-3: UTF-8 in, code-point row offsets + mask out)
  utf8_offsets    latok_split_offsets_utf8_batch
  utf8_spans      latok_token_spans_utf8_batch
  utf8_features32 latok_token_features_utf8_batch with LATOK_OUT_INT32 (featurize of UTF-8 in code-point units, no UTF-32 copy)
  utf8_offsets32 / utf8_spans32   the same UTF-8 entry points with LATOK_OUT_INT32 records
  utf8_mask_flow / utf8_offsets_flow / utf8_offsets32_flow / utf8_spans_flow / utf8_spans32_flow / utf8_features32_flow
                  (the `utf8_flow` leg) UTF-8 in code-point units through the batch flow (latok_flow_*_utf8): two batches in
                  flight with alternating output buffers and result words, nothing read by the host between the launches;
                  the result words of the last two batches are checked after the wait (no malformed flag, the blocking item count)
  utf8_bytes_features32 / utf8_bytes_features32_flow   latok_token_features_utf8_bytes_batch / latok_flow_token_features_utf8_bytes
                  with LATOK_OUT_INT32: featurize in BYTE space (4-field byte records + the 25 sums per char)
  pair_features32_bytes_spans32 / pair_features32_bytes_spans32_flow   what a byte-space caller had to run before that call
                  existed: latok_token_features_utf8_batch, then latok_token_spans_utf8_bytes_batch on the same batch (their
                  flow forms for the flow line; records of the two calls in buffers of their own).  Only symbols that older
                  libraries have too, so the same two paths can be timed against a library built from an earlier commit
  utf8_decode_features32   what a UTF-8 caller had to compose before: latok_utf8_decode_batch into a device buffer, then
                  latok_token_features_batch on it (LATOK_OUT_INT32); same data, same process
  bytes_mask / bytes_offsets / bytes_spans   latok_*_utf8_bytes_batch (8f-3 fused: the tile kernel reads the bytes)
  bytes_join / bytes_join_flow   latok_join_tokens_utf8_bytes_batch / latok_flow_join_tokens_utf8_bytes: every string's tokens joined by
                  one space, UTF-8 out (no counts asked for); beside them, in the same process run,
  bytes_spans32 / bytes_spans32_flow   latok_token_spans_utf8_bytes_batch / latok_flow_token_spans(kind 0) with LATOK_OUT_INT32: the
                  stage the join replaces for a caller who wants text
  bytes_hashes32 / bytes_hashes32_flow / bytes_hashes_only / bytes_hashes_only_flow   latok_token_hashes_utf8_bytes_batch /
                  latok_flow_token_hashes_utf8_bytes: one MurmurHash3 x86_32 word per token, with the int32 counts and records of
                  bytes_spans32 (hashes32) or alone (hashes_only: no counts, no records); same process run as bytes_spans32
  bytes_ids32 / bytes_ids32_flow / bytes_ids_only / bytes_ids_only_flow   latok_token_ids_utf8_bytes_batch /
                  latok_flow_token_ids_utf8_bytes: every token's id in a vocabulary (--vocab all: every distinct token of the corpus,
                  so every lookup hits; half: every second distinct token, in order of first appearance), with the int32 counts and
                  records of bytes_spans32 (ids32) or alone (ids_only); same process run as bytes_spans32 and bytes_hashes32
  bytes_count_cold / bytes_count_warm   latok_count_tokens_utf8_bytes_batch into a counter sized for the corpus' distinct tokens
                  (2 x distinct slots): cold -- the counter was cleared before the call (the clear is not timed), every distinct
                  word is claimed, committed to the blob and counted; warm -- the same batch once more, every token finds its
                  word resident and nothing is committed; same process run as bytes_spans32 and bytes_ids32
  bytes_terms32 / bytes_terms_hashed   latok_term_counts_utf8_bytes_batch (the vocabulary of the ids paths, --vocab all|half) /
                  latok_hashed_term_counts_utf8_bytes_batch (2^20 features, alternating signs): the CSR rows of the document-term
                  matrix with int32 indptr (and oov), capacity = the token total; same process run as bytes_ids32 and bytes_hashes32
  bytes_ngrams32 / bytes_ngrams_hashed   latok_ngram_counts_utf8_bytes_batch / latok_hashed_ngram_counts_utf8_bytes_batch with the
                  range (1, 2) and the separator 0x20, everything else as bytes_terms32 / bytes_terms_hashed (the vocabulary of the ids
                  paths holds single tokens only, so every bigram's probe ends in a miss); capacity = twice the token bound; same
                  process run as bytes_terms32, bytes_terms_hashed and bytes_spans32
  bytes_chargrams32 / bytes_chargrams_hashed   latok_chargram_counts_utf8_bytes_batch / latok_hashed_chargram_counts_utf8_bytes_batch with
                  the character range (3, 5) and the pad 0x20, everything else as bytes_terms32 / bytes_terms_hashed (the vocabulary of
                  the ids paths holds whole tokens, so nearly every gram's probe ends in a miss); capacity = nnz of a size query, which
                  also prints one line with the token total, the gram total K and nnz; same process run as bytes_terms32,
                  bytes_terms_hashed, bytes_ngrams_hashed and bytes_spans32
  bytes_tfidf32 / bytes_tfidf_hashed   latok_tfidf_utf8_bytes_batch / latok_hashed_tfidf_utf8_bytes_batch with range (1, 1), L2, smooth
                  idf and an idf fitted on the corpus by one update call; everything else as bytes_terms32 / bytes_terms_hashed -- run
                  them in the same process: the ratio of the two times is what the weighting costs
  bytes_df_update   latok_idf_update_utf8_bytes_batch (vocabulary form) into an idf that is cleared before every call
  csr_tfidf / csr_df   latok_tfidf_csr / latok_idf_update_csr alone on the device-resident CSR that bytes_terms32's call has left;
                  csr_df prints csr_df_cached and csr_df_plain: k_df_add with its LDS table and the plain form (latok_debug_set_df_add)
  py_tfidf        batch.tfidf_utf8_batch end to end against batch.term_counts_utf8_batch plus scikit-learn's TfidfTransformer on the
                  host (numpy where scikit-learn is absent)
  bytes_wp32 / bytes_wp_padded   latok_wordpiece_ids_utf8_bytes_batch (int32 indptr and spans, capacity = the token bound) /
                  latok_wordpiece_padded_utf8_bytes_batch ([n, 64] block with [CLS] / [SEP]) against a WordPiece vocabulary of the words
                  of the ids paths (--vocab all|half; no continuation words, so a token is one piece: with `all` its id, with `half`
                  every second distinct token misses at every candidate end); same process run as bytes_ids32 and bytes_spans32
  py_wp          end to end in Python on host blobs (the first --py-strings strings): batch.wordpiece_ids_utf8_batch(blobs, wp) against
                  batch.tokenize_utf8_batch(blobs) + the greedy longest-match loop over a dict; the vocabulary there also holds 2-byte
                  stems and ##-suffixes, so tokens do split; one line each
  bytes_bpe32 / bytes_bpe_padded   latok_bpe_ids_utf8_bytes_batch (int32 indptr and spans, capacity = the piece total of a size query) /
                  latok_bpe_padded_utf8_bytes_batch ([n, 64] block with BOS / EOS); the vocabulary is the 256 single bytes plus the merges
                  of a small byte-pair trainer over the 5000 most frequent tokens of the first --py-strings strings of the leg's own corpus (--bpe-merges,
                  lead_space = 1); same process run as bytes_ids32 and bytes_wp32, which are its yardsticks
  ids_detok_bpe / ids_detok_wp   latok_detok_csr on the resident int32 CSR that bytes_bpe32 / bytes_wp32 leave (CONCAT / WORDPIECE decoder
                 of the same words; yardsticks: bytes_join of the same run and the HBM cost of 4 B/id + the output bytes + 8 B/row)
  py_detok       end to end in Python: batch.decode_batch(detok, rows) against the host loop b"".join(words[i] for i in row)
  py_bpe         end to end in Python on host blobs (the first --py-strings strings): batch.bpe_ids_utf8_batch(blobs, bpe) against
                  batch.tokenize_utf8_batch(blobs) + the merge loop over a dict (lead_space = 0 there: the host route has no spans);
                  equal rows asserted first; one line each
  bytes_pretok_gpt2   latok_pretokens_utf8_bytes_batch with LATOK_PRETOK_GPT2 and LATOK_OUT_INT32: the span records of GPT-2's pre-tokens
                  (white-space pre-tokens are records too: items per call are reported beside the time); yardstick: bytes_spans32 of the same
                  process run
  bytes_bpe_gpt2  latok_bpe_ids_utf8_bytes_batch on an object of the same trained words as bytes_bpe32, made with pretokenizer="gpt2"
                  (lead_space = 0: the space is in the pre-token); yardstick: bytes_bpe32 of the same process run
  py_bpe_gpt2    end to end in Python on host blobs (the first min(--py-strings, 50000) strings): batch.bpe_ids_utf8_batch(blobs, bpe) of a
                  pretokenizer="gpt2" object against the `regex` package with GPT-2's pattern + the merge loop over a dict on the host;
                  equal rows asserted first; skipped with a note where `regex` is not importable
  bytes_pretok_spm    latok_pretokens_utf8_bytes_batch with LATOK_PRETOK_SPM and LATOK_OUT_INT32: the span records of SentencePiece's segments
                  (one launch for the planes, like GPT-2's front); yardstick: bytes_pretok_gpt2 of the same process run
  bytes_spbpe32 / bytes_spbpe_padded   latok_bpe_ids_utf8_bytes_batch / latok_bpe_padded_utf8_bytes_batch on a SentencePiece BPE object
                  (latok_bpe_create_spm, byte fallback, dummy prefix): the words are bytes_bpe32's trainer on the same tokens with U+2581 in
                  front of every second one, kept where they are well-formed UTF-8; yardstick: bytes_bpe_gpt2 of the same process run
  py_spbpe       end to end in Python on host blobs (the first min(--py-strings, 50000) strings): batch.bpe_ids_utf8_batch(blobs, bpe) of
                  such an object against a host loop (replace, split into segments, a memoised merge walk over characters, byte fallback),
                  equal rows asserted first; beside it, where the package is importable and not as a pass condition, sentencepiece's own
                  encode of a model made of the same words
  bytes_pretok_cl100k / bytes_bpe_cl100k / py_bpe_cl100k   the same three with LATOK_PRETOK_CL100K / pretokenizer="cl100k" (the cl100k /
                  Llama 3 pattern: two launches for the planes); yardsticks: bytes_pretok_gpt2 and bytes_bpe_gpt2 of the same process run
  bytes_uni32 / bytes_uni_padded   latok_unigram_ids_utf8_bytes_batch (int32 indptr and spans, capacity = the piece total of a size query) /
                  latok_unigram_padded_utf8_bytes_batch ([n, 64] block with BOS / EOS); the vocabulary is the characters of the 256 single
                  bytes plus the --uni-words most frequent tokens of the first --py-strings strings of the leg's own corpus, their
                  prefixes and suffixes, and the tokens once more behind the marker U+2581 (and the marker alone); scores = log of the
                  relative frequency, rounded to 1/64; same process run as bytes_bpe32, bytes_wp32 and bytes_ids32, which are its yardsticks
  py_uni         end to end in Python on host blobs (the first --py-strings strings): batch.unigram_ids_utf8_batch(blobs, unigram) against
                  batch.token_spans_utf8_bytes_csr + the Viterbi loop over a dict (memoised per distinct token); equal rows asserted first;
                  one line each
  py_terms       end to end in Python on host blobs (the first --py-strings strings): batch.term_counts_utf8_batch(blobs, vocab)
                  against batch.tokenize_utf8_batch(blobs) + a dict and collections.Counter per row; one line each
  py_count       end to end in Python on host blobs (the first --py-strings strings): TokenCounter.update_utf8 + most_common()
                  against collections.Counter over batch.tokenize_utf8_batch(blobs), sorted the same way; one line each
  py_ids         end to end in Python on host blobs (the first --py-strings strings): batch.token_ids_utf8_batch(blobs, vocab)
                  against [[d.get(t, -1) for t in row] for row in batch.tokenize_utf8_batch(blobs)]; one line each
  bytes_fold / bytes_fold_wp   latok_fold_utf8_bytes_batch (LOWER | STRIP_MARKS, device pointers; yardstick: bytes_join of the same run) /
                 the same, then latok_wordpiece_padded_utf8_bytes_batch on the folded bytes (yardstick: bytes_wp_padded alone)
  py_fold        end to end in Python on host blobs: batch.fold_utf8_batch(blobs) against NFD(t.lower()) without Mn on the host
  py_join        end to end in Python on host blobs (the first --py-strings strings): batch.join_tokens_utf8_batch(blobs) against the
                  only route to the same rows without it, [b" ".join(t) for t in batch.tokenize_utf8_batch(blobs)]; one line each
  rules_mask      latok_split_mask_batch after latok_set_rules(built-in tables)   (8f-4)
  offsets32 / spans32 / features32 / kind_offsets32 / kind_spans32   the same entry points with LATOK_OUT_INT32 records
  mask_flow / bytes_mask_flow / kind_mask_flow   the same mask paths through the batch flow (latok_flow_split_mask*: two
                  batches in flight, the small launches of one in the shadow of the other's tile kernel)
  kind_mask / kind_offsets / kind_spans      latok_*_kind_batch on PEP 393 code units: kind 1 (uint8) when every char
                  of the corpus is <= U+00FF (C2), else kind 2 (uint16) with the corpus' astral chars folded into the BMP
                  (cp & 0xFFFF; timing only -- C3 as CPython would store it without its emoji)

Every line carries: ms per call (wall clock around `--iters` blocking calls, inputs and outputs in HBM; the
compaction calls contain one 8-byte blocking read of the item total), the UTF-8 GB/s of the corpus through that path,
the path's ALGORITHMIC bytes (inputs that must be read + outputs that must be written, stated per line) and their rate
as a fraction of the 8 TB/s HBM peak.  `--cpu N` adds the reference's own C functions + its Python glue (oracle/_ref,
test infrastructure, timed here as the baseline only) on the first N strings for offsets and tokens.

`--repeat R` prints every line R times (R measurements in one warm process: the run-to-run spread of a path).

usage: tools/path_bench.py [--workload C2|C3] [--strings N] [--iters K] [--repeat R] [--cpu N]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from latok_amd import _lib  # noqa: E402

HBM_PEAK = 8000.0
WORKLOADS = {"C2": (_lib.CORPUS_ASCII, 0x1A70C0DE, 64, 192), "C3": (_lib.CORPUS_UNICODE, 0x1A70C0DF, 128, 384)}


def utf8_of(cps, row):
    """packed UTF-32 -> (utf8 bytes uint8[], byte offsets int64[n+1]) on the host (setup, not timed)."""
    lens = 1 + (cps >= 0x80).astype(np.int64) + (cps >= 0x800) + (cps >= 0x10000)
    pref = np.zeros(cps.size + 1, np.int64)
    np.cumsum(lens, out=pref[1:])
    boff = pref[row]
    if int(pref[-1]) == cps.size:
        u8 = cps.astype(np.uint8)
    else:
        u8 = np.frombuffer(cps.astype("<u4").tobytes().decode("utf-32-le", "surrogatepass").encode("utf-8", "surrogatepass"),
                           np.uint8)
    assert u8.size == int(pref[-1])
    return np.ascontiguousarray(u8), np.ascontiguousarray(boff)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C2", choices=sorted(WORKLOADS))
    ap.add_argument("--strings", type=int, default=1_000_000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeat", type=int, default=1, help="measurements per path, one JSON line each")
    ap.add_argument("--cpu", type=int, default=0, help="strings of CPU baseline (0 = skip)")
    ap.add_argument("--paths", default="mask,mask_flow,bytes_mask_flow,kind_mask_flow,offsets32_flow,spans32_flow,features32_flow,offsets,offsets32,spans,spans32,features,features32,utf8_mask,utf8_offsets,utf8_offsets32,utf8_spans,utf8_spans32,utf8_features32,"
                                       "utf8_mask_flow,utf8_offsets_flow,utf8_offsets32_flow,utf8_spans_flow,utf8_spans32_flow,utf8_features32_flow,utf8_decode_features32,"
                                       "utf8_bytes_features32,utf8_bytes_features32_flow,pair_features32_bytes_spans32,pair_features32_bytes_spans32_flow,"
                                       "bytes_mask,bytes_offsets,bytes_spans,bytes_spans32,bytes_spans32_flow,bytes_join,bytes_join_flow,"
                                       "bytes_hashes32,bytes_hashes32_flow,bytes_hashes_only,bytes_hashes_only_flow,"
                                       "bytes_ids32,bytes_ids32_flow,bytes_ids_only,bytes_ids_only_flow,bytes_terms32,bytes_terms_hashed,"
                                       "rules_mask,kind_mask,kind_offsets,kind_offsets32,"
                                       "kind_spans,kind_spans32")
    ap.add_argument("--py-strings", type=int, default=200_000, help="strings of the py_join / py_ids / py_terms paths (host blobs)")
    ap.add_argument("--bpe-merges", type=int, default=400, help="merges of the byte-pair trainer of the bpe paths")
    ap.add_argument("--uni-words", type=int, default=4000, help="most frequent tokens that seed the vocabulary of the unigram paths")
    ap.add_argument("--vocab", default="all", choices=("all", "half"), help="vocabulary of the ids paths: every distinct token of the corpus, or every second one")
    args = ap.parse_args()
    lib = _lib.ensure_init()
    model, seed, lo, hi = WORKLOADS[args.workload]
    n = args.strings
    row = np.zeros(n + 1, np.int64)
    _lib.check(lib.latok_corpus_offsets(seed, 0, n, lo, hi, row.ctypes.data))
    total = int(row[-1])
    words = (total + 63) // 64
    d_row = lib.latok_dev_alloc(row.nbytes)
    d_cps = lib.latok_dev_alloc(total * 4)
    _lib.check(lib.latok_memcpy_h2d(d_row, row.ctypes.data, row.nbytes))
    _lib.check(lib.latok_corpus_fill_device(seed, model, 0, n, d_row, d_cps, None))
    cps = np.empty(total, np.uint32)
    _lib.check(lib.latok_memcpy_d2h(cps.ctypes.data, d_cps, total * 4))
    u8, boff = utf8_of(cps, row)
    n8 = int(u8.size)
    d_u8 = lib.latok_dev_alloc(n8 + 64)
    d_boff = lib.latok_dev_alloc(boff.nbytes)
    _lib.check(lib.latok_memcpy_h2d(d_u8, u8.ctypes.data, n8))
    _lib.check(lib.latok_memcpy_h2d(d_boff, boff.ctypes.data, boff.nbytes))
    cap = total // 2 + 4096
    d_bits = lib.latok_dev_alloc(words * 8 + 8)
    d_counts = lib.latok_dev_alloc(n * 8)
    d_items = lib.latok_dev_alloc(cap * 32)
    d_feat = lib.latok_dev_alloc(cap * 25)
    d_cprow = lib.latok_dev_alloc((n + 1) * 8)
    for p in (d_row, d_cps, d_u8, d_boff, d_bits, d_counts, d_items, d_feat, d_cprow):
        if not p:
            raise RuntimeError(_lib.last_error())
    nout, tcp = C.c_int64(0), C.c_int64(0)
    D = _lib.DEVICE_PTRS
    csr = 8 * (n + 1)

    def run(name, fn, alg, note):
        _lib.check(fn())
        _lib.check(lib.latok_sync())
        for r in range(args.repeat):
            t = time.perf_counter()
            for _ in range(args.iters):
                _lib.check(fn())
            _lib.check(lib.latok_sync())
            dt = (time.perf_counter() - t) / args.iters
            a = alg()
            print(json.dumps({"path": name, "workload": args.workload, "strings": n, "chars": total, "utf8_bytes": n8,
                              "items": nout.value, "ms_per_call": dt * 1e3, "utf8_GBps": n8 / dt / 1e9,
                              "alg_bytes": a, "alg_GBps": a / dt / 1e9, "frac_of_hbm_peak": a / dt / 1e9 / HBM_PEAK,
                              "alg_bytes_are": note, "repeat": r}), flush=True)

    paths = args.paths.split(",")
    flow_buf = {}

    def flow_pair(n_words):   # two output bitmasks: consecutive submissions of a flow alternate between them
        if n_words not in flow_buf:
            flow_buf[n_words] = (lib.latok_dev_alloc(n_words * 8 + 8), lib.latok_dev_alloc(n_words * 8 + 8))
        return flow_buf[n_words]

    def run_flow(name, submit, alg, note):
        """the same measurement through the batch flow (include/latok_hip.h): `--iters` submissions, then one latok_flow_wait"""
        a_, b_ = None, None
        for i in range(4):
            _lib.check(submit(i))
        _lib.check(lib.latok_flow_wait())
        k = max(args.iters, 100)   # long enough that filling and draining the two-batch pipeline is noise
        for r in range(args.repeat):
            t = time.perf_counter()
            for i in range(k):
                _lib.check(submit(i))
            _lib.check(lib.latok_flow_wait())
            dt = (time.perf_counter() - t) / k
            a = alg()
            print(json.dumps({"path": name, "workload": args.workload, "strings": n, "chars": total, "utf8_bytes": n8,
                              "items": 0, "ms_per_call": dt * 1e3, "utf8_GBps": n8 / dt / 1e9,
                              "alg_bytes": a, "alg_GBps": a / dt / 1e9, "frac_of_hbm_peak": a / dt / 1e9 / HBM_PEAK,
                              "alg_bytes_are": note + "; batch flow: two batches in flight, per-batch time of " + str(k) + " submissions + one wait",
                              "repeat": r}), flush=True)

    if "mask_flow" in paths:
        fa, fb = flow_pair(words)
        run_flow("mask_flow", lambda i: lib.latok_flow_split_mask(d_cps, d_row, n, total, fb if i & 1 else fa),
                 lambda: 4 * total + csr + words * 8, "4 B/char + 8 B/string read, 1 bit/char written")
    if "bytes_mask_flow" in paths:
        bw_ = (n8 + 63) // 64
        fa, fb = flow_pair(bw_)
        run_flow("bytes_mask_flow", lambda i: lib.latok_flow_split_mask_utf8_bytes(d_u8, d_boff, n, n8, fb if i & 1 else fa),
                 lambda: n8 + csr + bw_ * 8, "UTF-8 bytes + 8 B/string read; 1 bit/byte written (byte space, fused ingest)")
    d_res = lib.latok_dev_alloc(64)
    for name, spans, width in (("offsets32_flow", False, 4), ("spans32_flow", True, 8)):
        if name in paths:
            if "items2" not in flow_buf:
                flow_buf["items2"] = (lib.latok_dev_alloc(cap * 32), lib.latok_dev_alloc(n * 8))
            d_items2, d_counts2 = flow_buf["items2"]
            fn = lib.latok_flow_token_spans if spans else lib.latok_flow_split_offsets
            run("offsets32" if not spans else "spans32", (lambda s_=spans: (lib.latok_token_spans_batch if s_ else lib.latok_split_offsets_batch)(
                d_cps, d_row, n, total, d_counts, d_items, cap, C.byref(nout), D | _lib.OUT_INT32, None)), lambda: 0, "(item count for the flow line)")
            items_n = nout.value
            run_flow(name, lambda i, fn=fn: fn(d_cps, 4, d_row, n, total, d_counts2 if i & 1 else d_counts, d_items2 if i & 1 else d_items, cap,
                                               C.c_void_p(d_res + 16 * (i & 1)), _lib.OUT_INT32),
                     lambda: 4 * total + csr + 4 * n + width * items_n,
                     f"4 B/char + 8 B/string read; 4 B/string counts + {width} B/item written (LATOK_OUT_INT32)")
    if "features32_flow" in paths:
        if "feat2" not in flow_buf:
            flow_buf["feat2"] = (lib.latok_dev_alloc(cap * 32), lib.latok_dev_alloc(n * 8), lib.latok_dev_alloc(cap * 25))
        d_items3, d_counts3, d_feat3 = flow_buf["feat2"]
        run("features32", lambda: lib.latok_token_features_batch(d_cps, d_row, n, total, d_counts, d_items, d_feat, cap, C.byref(nout), D | _lib.OUT_INT32, None),
            lambda: 0, "(item count for the flow line)")
        items_f = nout.value
        run_flow("features32_flow", lambda i: lib.latok_flow_token_features(d_cps, 4, d_row, n, total, d_counts3 if i & 1 else d_counts,
                                                                            d_items3 if i & 1 else d_items, d_feat3 if i & 1 else d_feat, cap,
                                                                            C.c_void_p(d_res + 16 * (i & 1)), _lib.OUT_INT32),
                 lambda: 4 * total + csr + 4 * n + (16 + 25) * items_f,
                 "SURVEY 8f-2 accounting: 4 B/char + 8 B/string read (the input ONCE); 4 B/string + 41 B/token written (LATOK_OUT_INT32)")
    if "mask" in paths:
        run("mask", lambda: lib.latok_split_mask_batch(d_cps, d_row, n, total, d_bits, D, None),
            lambda: 4 * total + csr + words * 8, "4 B/char + 8 B/string read, 1 bit/char written")
    if "offsets" in paths:
        run("offsets", lambda: lib.latok_split_offsets_batch(d_cps, d_row, n, total, d_counts, d_items, cap, C.byref(nout), D, None),
            lambda: 4 * total + csr + 8 * n + 8 * nout.value, "4 B/char + 8 B/string read; 8 B/string counts + 8 B/boundary written")
    if "spans" in paths:
        run("spans", lambda: lib.latok_token_spans_batch(d_cps, d_row, n, total, d_counts, d_items, cap, C.byref(nout), D, None),
            lambda: 4 * total + csr + 8 * n + 16 * nout.value, "4 B/char + 8 B/string read; 8 B/string counts + 16 B/token written")
    D32 = D | _lib.OUT_INT32
    if "offsets32" in paths:
        run("offsets32", lambda: lib.latok_split_offsets_batch(d_cps, d_row, n, total, d_counts, d_items, cap, C.byref(nout), D32, None),
            lambda: 4 * total + csr + 4 * n + 4 * nout.value, "4 B/char + 8 B/string read; 4 B/string counts + 4 B/boundary written (LATOK_OUT_INT32)")
    if "spans32" in paths:
        run("spans32", lambda: lib.latok_token_spans_batch(d_cps, d_row, n, total, d_counts, d_items, cap, C.byref(nout), D32, None),
            lambda: 4 * total + csr + 4 * n + 8 * nout.value, "4 B/char + 8 B/string read; 4 B/string counts + 8 B/token written (LATOK_OUT_INT32)")
    if "features32" in paths:
        run("features32", lambda: lib.latok_token_features_batch(d_cps, d_row, n, total, d_counts, d_items, d_feat, cap, C.byref(nout), D32, None),
            lambda: 4 * total + csr + 4 * n + (16 + 25) * nout.value,
            "SURVEY 8f-2 accounting: 4 B/char + 8 B/string read (the input ONCE); 4 B/string + 41 B/token written (LATOK_OUT_INT32)")
    if "features" in paths:
        run("features", lambda: lib.latok_token_features_batch(d_cps, d_row, n, total, d_counts, d_items, d_feat, cap, C.byref(nout), D, None),
            lambda: 4 * total + csr + 8 * n + (32 + 25) * nout.value,
            "SURVEY 8f-2 accounting: 4 B/char + 8 B/string read (the input ONCE); 8 B/string + 57 B/token written")
    if "utf8_mask" in paths:
        nout.value = 0
        run("utf8_mask", lambda: lib.latok_split_mask_utf8_batch(d_u8, d_boff, n, n8, d_bits, words + 1, d_cprow, C.byref(tcp), D, None),
            lambda: n8 + csr + words * 8 + csr, "UTF-8 bytes + 8 B/string read; 1 bit/char + 8 B/string cp offsets written")
        assert tcp.value == total
    if "utf8_offsets" in paths:
        run("utf8_offsets", lambda: lib.latok_split_offsets_utf8_batch(d_u8, d_boff, n, n8, d_counts, d_items, cap, C.byref(nout), D, None),
            lambda: n8 + csr + 8 * n + 8 * nout.value, "UTF-8 bytes + 8 B/string read; 8 B/string + 8 B/boundary written")
    if "utf8_spans" in paths:
        run("utf8_spans", lambda: lib.latok_token_spans_utf8_batch(d_u8, d_boff, n, n8, d_counts, d_items, cap, C.byref(nout), D, None),
            lambda: n8 + csr + 8 * n + 16 * nout.value, "UTF-8 bytes + 8 B/string read; 8 B/string + 16 B/token written")
    if "utf8_offsets32" in paths:
        run("utf8_offsets32", lambda: lib.latok_split_offsets_utf8_batch(d_u8, d_boff, n, n8, d_counts, d_items, cap, C.byref(nout), D32, None),
            lambda: n8 + csr + 4 * n + 4 * nout.value, "UTF-8 bytes + 8 B/string read; 4 B/string + 4 B/boundary written (LATOK_OUT_INT32)")
    if "utf8_spans32" in paths:
        run("utf8_spans32", lambda: lib.latok_token_spans_utf8_batch(d_u8, d_boff, n, n8, d_counts, d_items, cap, C.byref(nout), D32, None),
            lambda: n8 + csr + 4 * n + 8 * nout.value, "UTF-8 bytes + 8 B/string read; 4 B/string + 8 B/token written (LATOK_OUT_INT32)")
    if "utf8_features32" in paths:
        run("utf8_features32", lambda: lib.latok_token_features_utf8_batch(d_u8, d_boff, n, n8, d_counts, d_items, d_feat, cap, C.byref(nout), D32, None),
            lambda: n8 + csr + 4 * n + (16 + 25) * nout.value,
            "UTF-8 bytes + 8 B/string read (the input ONCE); 4 B/string + 41 B/token written (LATOK_OUT_INT32)")
    # the utf8_flow leg: the same code-point results through the batch flow, two batches in flight with alternating buffers
    u8_flow = [p for p in paths if p.startswith("utf8_") and p.endswith("_flow")]
    if u8_flow:
        bw8 = (n8 + 63) // 64
        fa, fb = flow_pair(bw8)
        d_cprow2, d_items4, d_counts4, d_feat4 = (lib.latok_dev_alloc((n + 1) * 8), lib.latok_dev_alloc(cap * 32), lib.latok_dev_alloc(n * 8),
                                                   lib.latok_dev_alloc(cap * 25))
        d_res4 = lib.latok_dev_alloc(128)
        if not (d_cprow2 and d_items4 and d_counts4 and d_feat4 and d_res4):
            raise RuntimeError(_lib.last_error())
        res_of = lambda i: C.c_void_p(d_res4 + 32 * (i & 1))  # noqa: E731

        def checked(name, blocking, submit, alg, note):
            """the blocking call once (item count), the flow measurement, then the result words of the last two batches"""
            _lib.check(blocking())
            items_n = 0 if name == "utf8_mask_flow" else nout.value
            run_flow(name, submit, lambda: alg(items_n), note)
            res = np.empty(8, np.int64)
            _lib.check(lib.latok_memcpy_d2h(res.ctypes.data, d_res4, 64))
            for r4 in res.reshape(2, 4):
                assert r4[3] == 0 and r4[1] == 0 and r4[2] == total and r4[0] == items_n, (name, r4.tolist())

        if "utf8_mask_flow" in u8_flow:
            checked("utf8_mask_flow", lambda: lib.latok_split_mask_utf8_batch(d_u8, d_boff, n, n8, d_bits, words + 1, d_cprow, C.byref(tcp), D, None),
                    lambda i: lib.latok_flow_split_mask_utf8(d_u8, d_boff, n, n8, fb if i & 1 else fa, bw8, d_cprow2 if i & 1 else d_cprow, res_of(i)),
                    lambda _: n8 + csr + words * 8 + csr, "UTF-8 bytes + 8 B/string read; 1 bit/char + 8 B/string cp offsets written")
        for name, fn_b, fn_f, fl, rec, per in (
                ("utf8_offsets_flow", lib.latok_split_offsets_utf8_batch, lib.latok_flow_split_offsets_utf8, 0, 8, 1),
                ("utf8_offsets32_flow", lib.latok_split_offsets_utf8_batch, lib.latok_flow_split_offsets_utf8, _lib.OUT_INT32, 4, 1),
                ("utf8_spans_flow", lib.latok_token_spans_utf8_batch, lib.latok_flow_token_spans_utf8, 0, 8, 2),
                ("utf8_spans32_flow", lib.latok_token_spans_utf8_batch, lib.latok_flow_token_spans_utf8, _lib.OUT_INT32, 4, 2)):
            if name in u8_flow:
                checked(name, lambda fn_b=fn_b, fl=fl: fn_b(d_u8, d_boff, n, n8, d_counts, d_items, cap, C.byref(nout), D | fl, None),
                        lambda i, fn_f=fn_f, fl=fl: fn_f(d_u8, d_boff, n, n8, d_counts4 if i & 1 else d_counts, d_items4 if i & 1 else d_items, cap,
                                                         res_of(i), fl),
                        lambda k, rec=rec, per=per: n8 + csr + rec * n + rec * per * k,
                        f"UTF-8 bytes + 8 B/string read; {rec} B/string + {rec * per} B/item written")
        if "utf8_features32_flow" in u8_flow:
            checked("utf8_features32_flow",
                    lambda: lib.latok_token_features_utf8_batch(d_u8, d_boff, n, n8, d_counts, d_items, d_feat, cap, C.byref(nout), D32, None),
                    lambda i: lib.latok_flow_token_features_utf8(d_u8, d_boff, n, n8, d_counts4 if i & 1 else d_counts, d_items4 if i & 1 else d_items,
                                                                 d_feat4 if i & 1 else d_feat, cap, res_of(i), _lib.OUT_INT32),
                    lambda k: n8 + csr + 4 * n + (16 + 25) * k,
                    "UTF-8 bytes + 8 B/string read (the input ONCE); 4 B/string + 41 B/token written (LATOK_OUT_INT32)")
    # featurize in byte space, and the pair of calls it replaces; every line of this leg in one process run
    bytes_leg = [p for p in paths if p.startswith("utf8_bytes_features32") or p.startswith("pair_features32_bytes_spans32")]
    if bytes_leg:
        bufs = [lib.latok_dev_alloc(sz) for sz in (cap * 16, n * 4, cap * 25, cap * 8, n * 4, cap * 16, n * 4, cap * 25, cap * 8, n * 4, 256)]
        if not all(bufs):
            raise RuntimeError(_lib.last_error())
        (b_items, b_counts, b_feat, b_spans, b_scounts), (c_items, c_counts, c_feat, c_spans, c_scounts), d_resb = bufs[:5], bufs[5:10], bufs[10]
        res4 = lambda i: C.c_void_p(d_resb + 32 * (i & 1))        # noqa: E731 -- four result words per batch in flight
        res2 = lambda i: C.c_void_p(d_resb + 128 + 16 * (i & 1))  # noqa: E731 -- two for the byte-space spans of the pair
        note41 = "UTF-8 bytes + 8 B/string read (the input ONCE); 4 B/string + 41 B/token written (LATOK_OUT_INT32)"
        note_pair = "two calls: " + note41 + ", then UTF-8 bytes + 8 B/string read again; 4 B/string + 8 B/token written"

        def pair_blocking():
            rc = lib.latok_token_features_utf8_batch(d_u8, d_boff, n, n8, b_counts, b_items, b_feat, cap, C.byref(nout), D32, None)
            return rc or lib.latok_token_spans_utf8_bytes_batch(d_u8, d_boff, n, n8, b_scounts, b_spans, cap, C.byref(nout), D32, None)

        def pair_flow(i):
            x = (c_items, c_counts, c_feat, c_spans, c_scounts) if i & 1 else (b_items, b_counts, b_feat, b_spans, b_scounts)
            rc = lib.latok_flow_token_features_utf8(d_u8, d_boff, n, n8, x[1], x[0], x[2], cap, res4(i), _lib.OUT_INT32)
            return rc or lib.latok_flow_token_spans(d_u8, 0, d_boff, n, n8, x[4], x[3], cap, res2(i), _lib.OUT_INT32)

        def flow_words(name, items_n, pair):
            res = np.empty(24, np.int64)
            _lib.check(lib.latok_memcpy_d2h(res.ctypes.data, d_resb, 192))
            for r4 in res[:8].reshape(2, 4):
                assert r4[3] == 0 and r4[1] == 0 and r4[2] == total and r4[0] == items_n, (name, r4.tolist())
            for r2 in res[16:20].reshape(2, 2) if pair else ():
                assert r2[1] == 0 and r2[0] == items_n, (name, r2.tolist())

        for name in bytes_leg:   # in the order given
            if name == "pair_features32_bytes_spans32":
                run(name, pair_blocking, lambda: 2 * (n8 + csr) + 8 * n + (16 + 25 + 8) * nout.value, note_pair)
            elif name == "pair_features32_bytes_spans32_flow":
                _lib.check(pair_blocking())
                items_n = nout.value
                run_flow(name, pair_flow, lambda: 2 * (n8 + csr) + 8 * n + (16 + 25 + 8) * items_n, note_pair)
                flow_words(name, items_n, True)
            elif name == "utf8_bytes_features32":
                run(name, lambda: lib.latok_token_features_utf8_bytes_batch(d_u8, d_boff, n, n8, b_counts, b_items, b_feat, cap, C.byref(nout), D32, None),
                    lambda: n8 + csr + 4 * n + (16 + 25) * nout.value, note41 + "; byte positions")
            elif name == "utf8_bytes_features32_flow":
                _lib.check(lib.latok_token_features_utf8_bytes_batch(d_u8, d_boff, n, n8, b_counts, b_items, b_feat, cap, C.byref(nout), D32, None))
                items_n = nout.value
                run_flow(name, lambda i: lib.latok_flow_token_features_utf8_bytes(d_u8, d_boff, n, n8, c_counts if i & 1 else b_counts,
                                                                                  c_items if i & 1 else b_items, c_feat if i & 1 else b_feat, cap,
                                                                                  res4(i), _lib.OUT_INT32),
                         lambda: n8 + csr + 4 * n + (16 + 25) * items_n, note41 + "; byte positions")
                flow_words(name, items_n, False)
            else:
                raise SystemExit("unknown path " + name)
        for p_ in bufs:
            lib.latok_dev_free(p_)
    if "utf8_decode_features32" in paths:
        d_dec, d_decrow = lib.latok_dev_alloc(total * 4 + 64), lib.latok_dev_alloc((n + 1) * 8)
        if not d_dec or not d_decrow:
            raise RuntimeError(_lib.last_error())

        def decode_features():
            rc = lib.latok_utf8_decode_batch(d_u8, d_boff, n, n8, d_dec, total, d_decrow, C.byref(tcp), D, None)
            return rc or lib.latok_token_features_batch(d_dec, d_decrow, n, total, d_counts, d_items, d_feat, cap, C.byref(nout), D32, None)
        run("utf8_decode_features32", decode_features, lambda: n8 + csr + 4 * n + (16 + 25) * nout.value,
            "UTF-8 bytes + 8 B/string read; 4 B/string + 41 B/token written (LATOK_OUT_INT32); the 4 B/char UTF-32 copy is not counted")
        lib.latok_dev_free(d_dec)
        lib.latok_dev_free(d_decrow)
    bwords = (n8 + 63) // 64
    if "bytes_mask" in paths:
        d_bbits = lib.latok_dev_alloc(bwords * 8 + 8)
        nout.value = 0
        run("bytes_mask", lambda: lib.latok_split_mask_utf8_bytes_batch(d_u8, d_boff, n, n8, d_bbits, D, None),
            lambda: n8 + csr + bwords * 8, "UTF-8 bytes + 8 B/string read; 1 bit/byte written (byte space, fused ingest)")
    if "bytes_offsets" in paths:
        run("bytes_offsets", lambda: lib.latok_split_offsets_utf8_bytes_batch(d_u8, d_boff, n, n8, d_counts, d_items, cap, C.byref(nout), D, None),
            lambda: n8 + csr + 8 * n + 8 * nout.value, "UTF-8 bytes + 8 B/string read; 8 B/string + 8 B/boundary written (byte offsets)")
    if "bytes_spans" in paths:
        run("bytes_spans", lambda: lib.latok_token_spans_utf8_bytes_batch(d_u8, d_boff, n, n8, d_counts, d_items, cap, C.byref(nout), D, None),
            lambda: n8 + csr + 8 * n + 16 * nout.value, "UTF-8 bytes + 8 B/string read; 8 B/string + 16 B/token written (byte ranges)")
    # joined token text and the byte-space spans beside it: every line of this leg in one process run, in the order given
    join_leg = [p for p in paths if p in ("bytes_join", "bytes_join_flow", "bytes_spans32", "bytes_spans32_flow", "bytes_hashes32",
                                          "bytes_hashes32_flow", "bytes_hashes_only", "bytes_hashes_only_flow", "bytes_ids32", "bytes_ids32_flow",
                                          "bytes_ids_only", "bytes_ids_only_flow", "bytes_terms32", "bytes_terms_hashed", "bytes_ngrams32", "bytes_ngrams_hashed", "py_terms",
                                          "bytes_chargrams32", "bytes_chargrams_hashed", "bytes_tfidf32", "bytes_tfidf_hashed", "bytes_df_update", "csr_tfidf", "csr_df", "py_tfidf",
                                          "bytes_count_cold", "bytes_count_warm", "py_count", "py_ids", "py_join", "bytes_wp32", "bytes_wp_padded", "py_wp",
                                          "bytes_bpe32", "bytes_bpe_padded", "py_bpe", "bytes_pretok_gpt2", "bytes_bpe_gpt2", "py_bpe_gpt2", "bytes_pretok_cl100k", "bytes_bpe_cl100k", "py_bpe_cl100k",
                                          "bytes_pretok_spm", "bytes_spbpe32", "bytes_spbpe_padded", "py_spbpe", "bytes_uni32", "bytes_uni_padded", "py_uni", "ids_detok_bpe", "ids_detok_wp", "py_detok",
                                          "bytes_fold", "bytes_fold_wp", "py_fold")]
    if join_leg:
        jb = [lib.latok_dev_alloc(sz) for sz in (2 * n8 + 64, (n + 1) * 8, 2 * n8 + 64, (n + 1) * 8, cap * 8, n * 4, cap * 8, n * 4, 64, cap * 4, cap * 4)]
        if not all(jb):
            raise RuntimeError(_lib.last_error())
        j_out, j_off, k_out, k_off, s_items, s_counts, t_items, t_counts, j_res, h_a, h_b = jb
        resj = lambda i: C.c_void_p(j_res + 16 * (i & 1))  # noqa: E731
        note_j = "UTF-8 bytes + 8 B/string read; body / head planes 2 x 1 bit/byte written and read; 1 B/output byte + 8 B/string row offsets written"
        note_s = "UTF-8 bytes + 8 B/string read; 4 B/string + 8 B/token written (byte ranges, LATOK_OUT_INT32)"
        join_blocking = lambda: lib.latok_join_tokens_utf8_bytes_batch(d_u8, d_boff, n, n8, 32, j_out, 2 * n8, j_off, None, C.byref(nout), D, None)  # noqa: E731
        spans_blocking = lambda: lib.latok_token_spans_utf8_bytes_batch(d_u8, d_boff, n, n8, s_counts, s_items, cap, C.byref(nout), D32, None)  # noqa: E731

        note_h = "UTF-8 bytes + 8 B/string read, the bytes of every token read once more; 4 B/token written (MurmurHash3 x86_32)"
        SEED = 0x9747B28C

        def hashes_blocking(rec):
            return lib.latok_token_hashes_utf8_bytes_batch(d_u8, d_boff, n, n8, SEED, s_counts if rec else None, s_items if rec else None, h_a, cap,
                                                           C.byref(nout), D32, None)

        note_i = ("UTF-8 bytes + 8 B/string read, the bytes of every token read once more, one 16-byte slot per probe step and the word of a "
                  "candidate read from the table; 4 B/token written (exact id, --vocab " + args.vocab + ")")
        vocab_box, words_box = [], []

        def corpus_vocab():
            """the vocabulary of the ids paths, built once: distinct tokens in order of first appearance, told apart by two hashes"""
            if vocab_box:
                return vocab_box[0]
            from latok_amd import batch
            keys = []
            for seed in (1, 2):
                _lib.check(lib.latok_token_hashes_utf8_bytes_batch(d_u8, d_boff, n, n8, seed, s_counts, s_items, h_a, cap, C.byref(nout), D32, None))
                h = np.empty(nout.value, np.uint32)
                _lib.check(lib.latok_memcpy_d2h(h.ctypes.data, h_a, h.nbytes))
                keys.append(h.astype(np.uint64))
            sp, cnt = np.empty((nout.value, 2), np.int32), np.empty(n, np.int32)
            _lib.check(lib.latok_memcpy_d2h(sp.ctypes.data, s_items, sp.nbytes))
            _lib.check(lib.latok_memcpy_d2h(cnt.ctypes.data, s_counts, cnt.nbytes))
            first = np.sort(np.unique((keys[0] << np.uint64(32)) | keys[1], return_index=True)[1])
            n_distinct = first.size
            first = first[::2] if args.vocab == "half" else first
            base = np.repeat(boff[:-1], cnt)[first]
            raw = u8.tobytes()
            words = [raw[a:b] for a, b in zip((base + sp[first, 0]).tolist(), (base + sp[first, 1]).tolist())]
            t = time.perf_counter()
            v = batch.Vocab(words, seed=SEED)
            print(json.dumps({"vocab": args.vocab, "workload": args.workload, "distinct_tokens": int(n_distinct), "words": len(words),
                              "n_slots": v.n_slots, "table_MiB": v.n_slots * 16 / 2**20, "word_bytes": sum(map(len, words)),
                              "create_ms": (time.perf_counter() - t) * 1e3}), flush=True)
            vocab_box.append(v)
            words_box.append(words)
            return v

        def ids_blocking(rec):
            return lib.latok_token_ids_utf8_bytes_batch(d_u8, d_boff, n, n8, corpus_vocab().handle, -1, s_counts if rec else None,
                                                        s_items if rec else None, h_a, cap, C.byref(nout), D32, None)

        note_t = ("as the ids / hashes path up to the key; 8 B/token keys written, read by the sort and written back; 4 B/string indptr "
                  "(+ 4 B/string oov) and 8 B/entry written (--vocab " + args.vocab + " / 2^20 features)")
        terms_box = []

        def terms_blocking(hashed):
            if not terms_box:
                tb = [lib.latok_dev_alloc(sz) for sz in ((n + 1) * 4 + 64, n * 4 + 64)]
                if not all(tb):
                    raise RuntimeError(_lib.last_error())
                terms_box.extend(tb)
            t_indptr, t_oov = terms_box
            if hashed:
                return lib.latok_hashed_term_counts_utf8_bytes_batch(d_u8, d_boff, n, n8, SEED, 1 << 20, 1, t_indptr, h_a, h_b, cap, C.byref(nout),
                                                                     None, D32, None)
            return lib.latok_term_counts_utf8_bytes_batch(d_u8, d_boff, n, n8, corpus_vocab().handle, t_indptr, t_oov, h_a, h_b, cap, C.byref(nout),
                                                          None, D32, None)

        # TF-IDF: the idf of the leg is fitted on the corpus itself by one update call; L2, smooth idf
        TFIDF_OPTS = _lib.TFIDF_SMOOTH_IDF | _lib.TFIDF_NORM_L2
        tfidf_box, tfidf_bufs = {}, []

        def tfidf_idf(hashed, fitted=True):
            """the fitted idf of the vocabulary / hashed form, or (fitted=False) an empty one of that size for the update legs"""
            from latok_amd import batch
            key = (hashed, fitted)
            if key not in tfidf_box:
                vh = None if hashed else corpus_vocab().handle
                f = batch.Idf((1 << 20) if hashed else len(words_box[0]))
                if fitted:
                    _lib.check(lib.latok_idf_update_utf8_bytes_batch(d_u8, d_boff, n, n8, vh, SEED, (1 << 20) if hashed else 0, 1, 1, 32, f.handle,
                                                                     C.byref(nout), None, D, None))
                tfidf_box[key] = f
            return tfidf_box[key]

        def tfidf_blocking(hashed):
            t_indptr, t_oov = terms_box
            f = tfidf_idf(hashed)
            if hashed:
                return lib.latok_hashed_tfidf_utf8_bytes_batch(d_u8, d_boff, n, n8, SEED, 1 << 20, 1, 1, 1, 32, f.handle, TFIDF_OPTS, t_indptr, h_a, h_b,
                                                               cap, C.byref(nout), D32, None)
            return lib.latok_tfidf_utf8_bytes_batch(d_u8, d_boff, n, n8, corpus_vocab().handle, 1, 1, 32, f.handle, TFIDF_OPTS, t_indptr, t_oov, h_a,
                                                    h_b, cap, C.byref(nout), D32, None)

        def df_update_blocking():
            f = tfidf_idf(False, fitted=False)
            _lib.check(lib.latok_idf_clear(f.handle))   # (n_docs stays below 2^31 whatever --iters is)
            return lib.latok_idf_update_utf8_bytes_batch(d_u8, d_boff, n, n8, corpus_vocab().handle, SEED, 0, 1, 1, 32, f.handle, C.byref(nout), None,
                                                         D, None)

        note_g = ("as bytes_terms32 / bytes_terms_hashed with one key per unigram and bigram: 16 B/token span records written and read, the "
                  "bytes of every token read by the walks of two tokens; 8 B/gram keys written, read by the sort and written back; 4 B/string "
                  "indptr (+ 4 B/string oov) and 8 B/entry written (--vocab " + args.vocab + " / 2^20 features)")
        ngrams_box = []

        def ngrams_blocking(hashed):
            if not ngrams_box:
                nb = [lib.latok_dev_alloc(sz) for sz in ((n + 1) * 4 + 64, n * 4 + 64, 2 * cap * 4, 2 * cap * 4)]
                if not all(nb):
                    raise RuntimeError(_lib.last_error())
                ngrams_box.extend(nb)
            g_indptr, g_oov, g_a, g_b = ngrams_box
            if hashed:
                return lib.latok_hashed_ngram_counts_utf8_bytes_batch(d_u8, d_boff, n, n8, SEED, 1 << 20, 1, 1, 2, 32, g_indptr, g_a, g_b, 2 * cap,
                                                                      C.byref(nout), None, D32, None)
            return lib.latok_ngram_counts_utf8_bytes_batch(d_u8, d_boff, n, n8, corpus_vocab().handle, 1, 2, 32, g_indptr, g_oov, g_a, g_b, 2 * cap,
                                                           C.byref(nout), None, D32, None)

        note_cg = ("as bytes_terms32 / bytes_terms_hashed with one key per character gram of the orders 3 .. 5 of every token's padded word: "
                   "16 B/token span records, 8 B/token gram counts and 8 B/token key ranks written and read, the bytes of every token read by "
                   "the walk from each of its characters; 8 B/gram keys written, read by the sort and written back; 4 B/string indptr "
                   "(+ 4 B/string oov) and 8 B/entry written (--vocab " + args.vocab + " / 2^20 features)")
        chargrams_box = {}

        def chargrams_call(hashed, indices, data, cap_, n_grams=None):
            g_indptr, g_oov = chargrams_box["rows"]
            if hashed:
                return lib.latok_hashed_chargram_counts_utf8_bytes_batch(d_u8, d_boff, n, n8, SEED, 1 << 20, 1, 3, 5, 32, g_indptr, indices, data, cap_,
                                                                         C.byref(nout), n_grams, D32, None)
            return lib.latok_chargram_counts_utf8_bytes_batch(d_u8, d_boff, n, n8, corpus_vocab().handle, 3, 5, 32, g_indptr, g_oov, indices, data, cap_,
                                                              C.byref(nout), n_grams, D32, None)

        def chargrams_blocking(hashed):
            if "rows" not in chargrams_box:
                chargrams_box["rows"] = [lib.latok_dev_alloc(sz) for sz in ((n + 1) * 4 + 64, n * 4 + 64)]
                if not all(chargrams_box["rows"]):
                    raise RuntimeError(_lib.last_error())
            if hashed not in chargrams_box:   # the size query: K and nnz of the workload, one line; then buffers of exactly nnz entries
                k = C.c_int64(0)
                chargrams_call(hashed, None, None, 0, C.byref(k))
                need = nout.value
                n_tok = C.c_int64(0)   # (a size query of the plain counts: the token total of the same batch)
                lib.latok_hashed_term_counts_utf8_bytes_batch(d_u8, d_boff, n, n8, SEED, 1 << 20, 1, chargrams_box["rows"][0], None, None, 0,
                                                              C.byref(nout), C.byref(n_tok), D32, None)
                print(json.dumps({"chargrams": "hashed" if hashed else "vocab", "workload": args.workload, "strings": n, "utf8_bytes": n8,
                                  "range": [3, 5], "pad": 32, "tokens": n_tok.value, "n_grams": k.value, "nnz": need}), flush=True)
                bufs = [lib.latok_dev_alloc(need * 4 + 64), lib.latok_dev_alloc(need * 4 + 64)]
                if not all(bufs):
                    raise RuntimeError(_lib.last_error())
                chargrams_box[hashed] = bufs + [need]
            g_a, g_b, need = chargrams_box[hashed]
            return chargrams_call(hashed, g_a, g_b, need)

        note_w = ("UTF-8 bytes + 8 B/string read; 4 B/string indptr + 4 B/piece ids + 8 B/piece spans written (--vocab " + args.vocab + "). NOT "
                  "counted: the workspace traffic (16 B/token span records, 8 B/token piece counts, 8 B/token piece ranks, each written "
                  "once and read once or twice), the two walks of every token's bytes and the table reads of every candidate end")
        WP_LEN = 64
        wp_box = []

        def corpus_wordpiece():
            """the WordPiece vocabulary of the wp paths, built once: the words of the ids paths (no continuation words: a token is one
            piece, its own id or unk -- with --vocab half every second distinct token misses at every candidate end)"""
            if not wp_box:
                from latok_amd import batch
                corpus_vocab()
                t = time.perf_counter()
                w = batch.WordPiece(words_box[0], max_chars=100, seed=SEED)
                print(json.dumps(dict(w.info(), prefix="##", wordpiece=args.vocab, workload=args.workload,
                                      create_ms=(time.perf_counter() - t) * 1e3)), flush=True)
                bufs = [lib.latok_dev_alloc(sz) for sz in ((n + 1) * 4 + 64, n * WP_LEN * 4 + 64, n * 4 + 64)]
                if not all(bufs):
                    raise RuntimeError(_lib.last_error())
                wp_box.extend([w] + bufs)
            return wp_box

        def wp_blocking():
            w, w_indptr, _, _ = corpus_wordpiece()
            return lib.latok_wordpiece_ids_utf8_bytes_batch(d_u8, d_boff, n, n8, w.handle, -1, w_indptr, h_a, s_items, cap, C.byref(nout), None,
                                                            D32, None)

        def wp_padded_blocking():
            w, _, w_block, w_len = corpus_wordpiece()
            return lib.latok_wordpiece_padded_utf8_bytes_batch(d_u8, d_boff, n, n8, w.handle, -1, WP_LEN, 1, 101, 102, 0, w_block, w_len,
                                                               C.byref(nout), D, None)

        note_b = ("UTF-8 bytes + 8 B/string read; 4 B/string indptr + 4 B/piece ids + 8 B/piece spans written. NOT counted: the workspace "
                  "traffic (16 B/token span records, 8 B/token piece counts, ranks and part-start masks), the walks of every token's bytes and "
                  "the table reads of every pair lookup")
        bpe_box, bpe_words, detok_box = [], [], {}

        def bpe_train(tokens, n_merges):
            """the 256 single bytes, then n_merges times the most frequent adjacent pair of the tokens (bytes), merged everywhere"""
            from collections import Counter
            freq = dict(Counter(tokens).most_common(5000))   # (the trainer is plain Python: the frequent tokens decide the merges anyway)
            seqs = {t: [t[i:i + 1] for i in range(len(t))] for t in freq}
            words = [bytes([b]) for b in range(256)]
            for _ in range(n_merges):
                pairs = Counter()
                for t, parts in seqs.items():
                    for x, y in zip(parts, parts[1:]):
                        pairs[(x, y)] += freq[t]
                if not pairs:
                    break
                x, y = min(pairs.items(), key=lambda kv: (-kv[1], kv[0]))[0]
                words.append(x + y)
                for t, parts in seqs.items():
                    if len(parts) < 2:
                        continue
                    i, out = 0, []
                    while i < len(parts):
                        if i + 1 < len(parts) and parts[i] == x and parts[i + 1] == y:
                            out.append(x + y)
                            i += 2
                        else:
                            out.append(parts[i])
                            i += 1
                    seqs[t] = out
            return words

        def bpe_sample_tokens(lead):
            from latok_amd import batch
            m = min(args.py_strings, n)
            blob = u8[:int(boff[m])].tobytes()
            blobs = [blob[int(a):int(b)] for a, b in zip(boff[:m], boff[1:m + 1])]
            toks = [t for row in batch.tokenize_utf8_batch(blobs) for t in row]
            return blobs, blob, ([b" " + t for t in toks[::2]] + toks[1::2] if lead else toks)

        def corpus_bpe():
            """the BPE vocabulary of the bpe paths and their buffers, built once (the ids are sized by a size query)"""
            if not bpe_box:
                from latok_amd import batch
                t = time.perf_counter()
                words = bpe_train(bpe_sample_tokens(True)[2], args.bpe_merges)
                train_ms = (time.perf_counter() - t) * 1e3
                t = time.perf_counter()
                b = batch.BPE(words, lead_space=True, seed=SEED)
                bpe_words.extend(words)
                print(json.dumps(dict(b.info(), bpe_merges=len(words) - 256, workload=args.workload, train_ms=train_ms,
                                      create_ms=(time.perf_counter() - t) * 1e3)), flush=True)
                bufs = [lib.latok_dev_alloc(sz) for sz in ((n + 1) * 4 + 64, n * WP_LEN * 4 + 64, n * 4 + 64)]
                if not all(bufs):
                    raise RuntimeError(_lib.last_error())
                need = C.c_int64(0)
                rc = lib.latok_bpe_ids_utf8_bytes_batch(d_u8, d_boff, n, n8, b.handle, -1, bufs[0], None, None, 0, C.byref(need), None, D32, None)
                if rc != _lib.OK and need.value <= 0:
                    _lib.check(rc)
                pieces = [lib.latok_dev_alloc(need.value * 4 + 64), lib.latok_dev_alloc(need.value * 8 + 64)]
                if not all(pieces):
                    raise RuntimeError(_lib.last_error())
                bpe_box.extend([b] + bufs + pieces + [need.value])
            return bpe_box

        def bpe_blocking():
            b, b_indptr, _, _, b_ids, b_spans, need = corpus_bpe()
            return lib.latok_bpe_ids_utf8_bytes_batch(d_u8, d_boff, n, n8, b.handle, -1, b_indptr, b_ids, b_spans, need, C.byref(nout), None, D32, None)

        def bpe_padded_blocking():
            b, _, b_block, b_len = corpus_bpe()[:4]
            return lib.latok_bpe_padded_utf8_bytes_batch(d_u8, d_boff, n, n8, b.handle, -1, WP_LEN, 1, 1, 2, 0, b_block, b_len, C.byref(nout), D, None)

        # GPT-2's pre-tokenizer: the span call, and the BPE call on an object of bytes_bpe32's words that brings it as its front
        pretok_gpt2_blocking = lambda: lib.latok_pretokens_utf8_bytes_batch(d_u8, d_boff, n, n8, _lib.PRETOK_GPT2, s_counts, s_items, cap, C.byref(nout), D32, None)  # noqa: E731
        pretok_cl100k_blocking = lambda: lib.latok_pretokens_utf8_bytes_batch(d_u8, d_boff, n, n8, _lib.PRETOK_CL100K, s_counts, s_items, cap, C.byref(nout), D32, None)  # noqa: E731
        pretok_spm_blocking = lambda: lib.latok_pretokens_utf8_bytes_batch(d_u8, d_boff, n, n8, _lib.PRETOK_SPM, s_counts, s_items, cap, C.byref(nout), D32, None)  # noqa: E731
        gpt2_box, cl100k_box, spm_box = [], [], []
        SPM_MARK = "\u2581".encode()

        def spm_words(toks):
            """the words of the spbpe paths: bpe_train on the tokens with the marker in front of every second one, the well-formed ones"""
            def ok(w):
                try:
                    w.decode("utf-8")
                    return True
                except UnicodeDecodeError:
                    return False
            return [w for w in bpe_train([SPM_MARK + t for t in toks[::2]] + toks[1::2], args.bpe_merges) if ok(w)]

        def corpus_spbpe():
            if not spm_box:
                from latok_amd import batch
                words = spm_words(bpe_sample_tokens(False)[2])
                b = batch.BPE.sentencepiece(words, byte_ids=[len(words) + x for x in range(256)], seed=SEED)
                bufs = [lib.latok_dev_alloc(sz) for sz in ((n + 1) * 4 + 64, n * WP_LEN * 4 + 64, n * 4 + 64)]
                need, n_seg = C.c_int64(0), C.c_int64(0)
                rc = lib.latok_bpe_ids_utf8_bytes_batch(d_u8, d_boff, n, n8, b.handle, -1, bufs[0], None, None, 0, C.byref(need), C.byref(n_seg), D32, None)
                if rc != _lib.OK and need.value <= 0:
                    _lib.check(rc)
                pieces = [lib.latok_dev_alloc(need.value * 4 + 64), lib.latok_dev_alloc(need.value * 8 + 64)]
                if not (all(bufs) and all(pieces)):
                    raise RuntimeError(_lib.last_error())
                print(json.dumps(dict(b.info(), **b.spm_info(), spbpe_words=len(words), workload=args.workload, segments=n_seg.value, pieces=need.value,
                                      pieces_per_segment=need.value / max(n_seg.value, 1))), flush=True)
                spm_box.extend([b] + bufs + pieces + [need.value])
            return spm_box

        def spbpe_blocking():
            b, g_indptr, _, _, g_ids, g_spans, need = corpus_spbpe()
            return lib.latok_bpe_ids_utf8_bytes_batch(d_u8, d_boff, n, n8, b.handle, -1, g_indptr, g_ids, g_spans, need, C.byref(nout), None, D32, None)

        def spbpe_padded_blocking():
            b, _, g_block, g_len = corpus_spbpe()[:4]
            return lib.latok_bpe_padded_utf8_bytes_batch(d_u8, d_boff, n, n8, b.handle, -1, WP_LEN, 1, 1, 2, 0, g_block, g_len, C.byref(nout), D, None)

        def corpus_bpe_gpt2(gpt2_box=gpt2_box, pretokenizer="gpt2"):
            if not gpt2_box:
                from latok_amd import batch
                corpus_bpe()
                b = batch.BPE(bpe_words, pretokenizer=pretokenizer, seed=SEED)
                g_indptr = lib.latok_dev_alloc((n + 1) * 4 + 64)
                need = C.c_int64(0)
                rc = lib.latok_bpe_ids_utf8_bytes_batch(d_u8, d_boff, n, n8, b.handle, -1, g_indptr, None, None, 0, C.byref(need), None, D32, None)
                if rc != _lib.OK and need.value <= 0:
                    _lib.check(rc)
                pieces = [lib.latok_dev_alloc(need.value * 4 + 64), lib.latok_dev_alloc(need.value * 8 + 64)]
                if not (g_indptr and all(pieces)):
                    raise RuntimeError(_lib.last_error())
                gpt2_box.extend([b, g_indptr] + pieces + [need.value])
            return gpt2_box

        def bpe_gpt2_blocking():
            b, g_indptr, g_ids, g_spans, need = corpus_bpe_gpt2()
            return lib.latok_bpe_ids_utf8_bytes_batch(d_u8, d_boff, n, n8, b.handle, -1, g_indptr, g_ids, g_spans, need, C.byref(nout), None, D32, None)

        def bpe_cl100k_blocking():
            b, g_indptr, g_ids, g_spans, need = corpus_bpe_gpt2(cl100k_box, "cl100k")
            return lib.latok_bpe_ids_utf8_bytes_batch(d_u8, d_boff, n, n8, b.handle, -1, g_indptr, g_ids, g_spans, need, C.byref(nout), None, D32, None)

        uni_box = []
        UNI_MARKER = "\u2581".encode()

        def uni_vocab(tokens):
            """(words, scores): the characters of the 256 single bytes, the --uni-words most frequent tokens with their prefixes and
            suffixes (cut at character starts), the tokens behind the marker, the marker alone; scores = log relative frequency in 1/64"""
            import math
            from collections import Counter
            freq = Counter()
            for t, c in Counter(tokens).most_common(args.uni_words):
                starts = [i for i in range(len(t)) if i == 0 or (t[i] & 0xC0) != 0x80] + [len(t)]
                for k in starts[1:]:
                    freq[t[:k]] += c
                for k in starts[1:-1]:
                    freq[t[k:]] += c
                freq[UNI_MARKER + t] += c
                freq[UNI_MARKER] += c
            for b in range(256):
                freq[chr(b).encode()] += 1
            total = sum(freq.values())
            words = sorted(freq, key=lambda w: (-freq[w], w))
            return words, [round(math.log(freq[w] / total) * 64) / 64 for w in words]

        def corpus_uni():
            """the Unigram vocabulary of the uni paths and their buffers, built once (the ids are sized by a size query)"""
            if not uni_box:
                from latok_amd import batch
                t = time.perf_counter()
                words, scores = uni_vocab(bpe_sample_tokens(False)[2])
                train_ms = (time.perf_counter() - t) * 1e3
                t = time.perf_counter()
                u = batch.Unigram(words, scores, seed=SEED)
                create_ms = (time.perf_counter() - t) * 1e3
                bufs = [lib.latok_dev_alloc(sz) for sz in ((n + 1) * 4 + 64, n * WP_LEN * 4 + 64, n * 4 + 64)]
                if not all(bufs):
                    raise RuntimeError(_lib.last_error())
                need, n_tok = C.c_int64(0), C.c_int64(0)
                rc = lib.latok_unigram_ids_utf8_bytes_batch(d_u8, d_boff, n, n8, u.handle, -1, bufs[0], None, None, 0, C.byref(need), C.byref(n_tok), D32, None)
                if rc != _lib.OK and need.value <= 0:
                    _lib.check(rc)
                info = u.info()
                info["marker"] = info["marker"].hex()
                print(json.dumps(dict(info, unigram_words=len(words), workload=args.workload, train_ms=train_ms, create_ms=create_ms, pieces=need.value,
                                      tokens=n_tok.value, pieces_per_token=need.value / max(n_tok.value, 1))), flush=True)
                pieces = [lib.latok_dev_alloc(need.value * 4 + 64), lib.latok_dev_alloc(need.value * 8 + 64)]
                if not all(pieces):
                    raise RuntimeError(_lib.last_error())
                uni_box.extend([u] + bufs + pieces + [need.value])
            return uni_box

        def uni_blocking():
            u, u_indptr, _, _, u_ids, u_spans, need = corpus_uni()
            return lib.latok_unigram_ids_utf8_bytes_batch(d_u8, d_boff, n, n8, u.handle, -1, u_indptr, u_ids, u_spans, need, C.byref(nout), None, D32, None)

        def uni_padded_blocking():
            u, _, u_block, u_len = corpus_uni()[:4]
            return lib.latok_unigram_padded_utf8_bytes_batch(d_u8, d_boff, n, n8, u.handle, -1, WP_LEN, 1, 1, 2, 0, u_block, u_len, C.byref(nout), D, None)

        note_d = ("4 B/id read + 4 B/string indptr read; 1 B/output byte + 8 B/string row offsets written. NOT counted: the second read of the "
                  "ids and the 4 B/piece byte counts written and read (workspace), the id map and entry records (cache resident), the blob bytes")

        def detok_of(kind):
            """the decoder of the detok paths, built once per kind, behind one encode call that leaves the ids resident (int32 indptr)"""
            if kind not in detok_box:
                from latok_amd import batch
                if kind == "bpe":
                    _lib.check(bpe_blocking())
                    _, indptr, _, _, ids = corpus_bpe()[:5]
                    dt_ = batch.Detokenizer(bpe_words)
                else:
                    _lib.check(wp_blocking())
                    indptr, ids = corpus_wordpiece()[1], h_a
                    dt_ = batch.Detokenizer(words_box[0], mode="wordpiece")
                print(json.dumps(dict(dt_.info(), detok=kind, workload=args.workload, pieces=nout.value)), flush=True)
                detok_box[kind] = (dt_, indptr, ids, nout.value)
            return detok_box[kind]

        def detok_blocking(kind):
            dt_, indptr, ids, n_pieces = detok_of(kind)
            return lib.latok_detok_csr(dt_.handle, indptr, ids, n, n_pieces, None, 0, j_out, 2 * n8, j_off, C.byref(nout), None, D32, None)

        note_f = ("UTF-8 bytes + 8 B/string read twice (count pass, write pass); 1 bit/byte string-end bitmap written and read; 2 B per 16 bytes "
                  "group prefixes written and read; 1 B/output byte + 8 B/string row offsets written (LOWER | STRIP_MARKS)")
        FOLD = _lib.FOLD_LOWER | _lib.FOLD_STRIP_MARKS
        fold_box, fold_wp_box = [], []

        def fold_bufs():
            if not fold_box:
                fb = [lib.latok_dev_alloc(sz) for sz in (3 * n8 + 64, (n + 1) * 8 + 64)]
                if not all(fb):
                    raise RuntimeError(_lib.last_error())
                fold_box.extend(fb)
            return fold_box

        def fold_blocking():
            f_out, f_off = fold_bufs()
            return lib.latok_fold_utf8_bytes_batch(d_u8, d_boff, n, n8, FOLD, f_out, 3 * n8, f_off, C.byref(nout), D, None)

        def folded_wordpiece():
            """the WordPiece vocabulary of bytes_fold_wp, built once: the words of bytes_wp_padded, folded (of words that fold alike the first wins)"""
            if not fold_wp_box:
                from latok_amd import batch
                corpus_wordpiece()
                fold_wp_box.append(batch.WordPiece(batch.fold_utf8_batch(words_box[0], FOLD), max_chars=100, seed=SEED))
            return fold_wp_box[0]

        def fold_wp_blocking():
            """fold, then the padded WordPiece call on the folded bytes, both with device pointers"""
            f_out, f_off = fold_bufs()
            _, _, w_block, w_len = corpus_wordpiece()
            folded = C.c_int64(0)
            rc = lib.latok_fold_utf8_bytes_batch(d_u8, d_boff, n, n8, FOLD, f_out, 3 * n8, f_off, C.byref(folded), D, None)
            if rc:
                return rc
            return lib.latok_wordpiece_padded_utf8_bytes_batch(f_out, f_off, n, folded.value, folded_wordpiece().handle, -1, WP_LEN, 1, 101, 102, 0,
                                                               w_block, w_len, C.byref(nout), D, None)

        note_c = ("UTF-8 bytes + 8 B/string read, the bytes of every token read once more, one 8-byte slot per probe step and the word of a "
                  "candidate read from the text or the blob; per tile and distinct word one 8-byte atomic add; two passes over the slots")
        counter_box = []

        def corpus_counter():
            """the counter of the count paths, made once: sized for the corpus' distinct tokens (found with a first, generous one)"""
            if counter_box:
                return counter_box[0]
            from latok_amd import batch
            guess = 1 << 20
            while True:
                with batch.TokenCounter(guess, seed=SEED) as probe:
                    st = np.zeros(4, np.int64)
                    _lib.check(lib.latok_count_tokens_utf8_bytes_batch(d_u8, d_boff, n, n8, probe.handle, st.ctypes.data, D, None))
                    distinct, dropped = probe.stats["distinct"], int(st[3])
                if dropped == 0 and distinct <= guess:
                    break
                guess *= 4
            tc = batch.TokenCounter(max(distinct, 1), seed=SEED)
            print(json.dumps({"counter": "corpus", "workload": args.workload, "distinct_tokens": distinct, "tokens": int(st[0]), "long": int(st[2]),
                              "n_slots": tc.n_slots, "table_MiB": tc.n_slots * 16 / 2**20}), flush=True)
            counter_box.append(tc)
            return tc

        def run_count(name, warm):
            tc = corpus_counter()
            st = np.zeros(4, np.int64)
            call = lambda: lib.latok_count_tokens_utf8_bytes_batch(d_u8, d_boff, n, n8, tc.handle, st.ctypes.data, D, None)  # noqa: E731
            tc.clear()
            _lib.check(call())
            for r in range(args.repeat):
                dt = 0.0
                for _ in range(args.iters):
                    if not warm:
                        tc.clear()                   # (waits for the device; not timed)
                    t = time.perf_counter()
                    _lib.check(call())               # (blocking: the commit is inside)
                    dt += time.perf_counter() - t
                dt /= args.iters
                assert st[3] == 0 and st[0] == st[1] + st[2], st.tolist()
                distinct = tc.stats["distinct"]
                a = n8 + csr + 2 * tc.n_slots * 8
                print(json.dumps({"path": name, "workload": args.workload, "strings": n, "utf8_bytes": n8, "items": int(st[0]), "distinct": distinct,
                                  "long": int(st[2]), "n_slots": tc.n_slots, "ms_per_call": dt * 1e3, "utf8_GBps": n8 / dt / 1e9, "alg_bytes": a,
                                  "alg_GBps": a / dt / 1e9, "frac_of_hbm_peak": a / dt / 1e9 / HBM_PEAK, "alg_bytes_are": note_c, "repeat": r}),
                      flush=True)

        def two_words(name, want):
            res = np.empty(4, np.int64)
            _lib.check(lib.latok_memcpy_d2h(res.ctypes.data, j_res, 32))
            for r2 in res.reshape(2, 2):
                assert r2[1] == 0 and r2[0] == want, (name, r2.tolist())

        for name in join_leg:
            if name == "bytes_join":
                run(name, join_blocking, lambda: n8 + csr + 4 * ((n8 + 63) // 64) * 8 + nout.value + csr, note_j)
            elif name == "bytes_join_flow":
                _lib.check(join_blocking())
                out_n = nout.value
                run_flow(name, lambda i: lib.latok_flow_join_tokens_utf8_bytes(d_u8, d_boff, n, n8, 32, k_out if i & 1 else j_out, 2 * n8,
                                                                               k_off if i & 1 else j_off, None, resj(i), 0),
                         lambda: n8 + csr + 4 * ((n8 + 63) // 64) * 8 + out_n + csr, note_j)
                two_words(name, out_n)
            elif name == "bytes_spans32":
                run(name, spans_blocking, lambda: n8 + csr + 4 * n + 8 * nout.value, note_s)
            elif name == "bytes_spans32_flow":
                _lib.check(spans_blocking())
                items_n = nout.value
                run_flow(name, lambda i: lib.latok_flow_token_spans(d_u8, 0, d_boff, n, n8, t_counts if i & 1 else s_counts,
                                                                    t_items if i & 1 else s_items, cap, resj(i), _lib.OUT_INT32),
                         lambda: n8 + csr + 4 * n + 8 * items_n, note_s)
                two_words(name, items_n)
            elif name in ("bytes_hashes32", "bytes_hashes_only"):
                rec = name == "bytes_hashes32"
                run(name, lambda: hashes_blocking(rec), lambda: n8 + csr + 4 * nout.value + (4 * n + 8 * nout.value if rec else 0),
                    note_h + (" + " + note_s if rec else ""))
            elif name in ("bytes_hashes32_flow", "bytes_hashes_only_flow"):
                rec = name == "bytes_hashes32_flow"
                _lib.check(hashes_blocking(rec))
                items_n = nout.value
                run_flow(name, lambda i: lib.latok_flow_token_hashes_utf8_bytes(d_u8, d_boff, n, n8, SEED, (t_counts if i & 1 else s_counts) if rec else None,
                                                                                (t_items if i & 1 else s_items) if rec else None,
                                                                                h_b if i & 1 else h_a, cap, resj(i), _lib.OUT_INT32),
                         lambda: n8 + csr + 4 * items_n + (4 * n + 8 * items_n if rec else 0), note_h + (" + " + note_s if rec else ""))
                two_words(name, items_n)
            elif name in ("bytes_ids32", "bytes_ids_only"):
                rec = name == "bytes_ids32"
                run(name, lambda: ids_blocking(rec), lambda: n8 + csr + 4 * nout.value + (4 * n + 8 * nout.value if rec else 0),
                    note_i + (" + " + note_s if rec else ""))
            elif name in ("bytes_ids32_flow", "bytes_ids_only_flow"):
                rec = name == "bytes_ids32_flow"
                _lib.check(ids_blocking(rec))
                items_n = nout.value
                vh = corpus_vocab().handle
                run_flow(name, lambda i: lib.latok_flow_token_ids_utf8_bytes(d_u8, d_boff, n, n8, vh, -1, (t_counts if i & 1 else s_counts) if rec else None,
                                                                             (t_items if i & 1 else s_items) if rec else None,
                                                                             h_b if i & 1 else h_a, cap, resj(i), _lib.OUT_INT32),
                         lambda: n8 + csr + 4 * items_n + (4 * n + 8 * items_n if rec else 0), note_i + (" + " + note_s if rec else ""))
                two_words(name, items_n)
            elif name == "bytes_wp32":   # (items = pieces)
                run(name, wp_blocking, lambda: n8 + csr + 4 * n + 12 * nout.value, note_w)
            elif name == "bytes_wp_padded":   # (items = the untruncated piece total; the block is [n, WP_LEN] with [CLS] / [SEP])
                run(name, wp_padded_blocking, lambda: n8 + csr + 4 * n + 4 * n * WP_LEN,
                    note_w.replace("4 B/string indptr + 4 B/piece ids + 8 B/piece spans", "4 B/string lengths + 4 B/cell of the [n, %d] block" % WP_LEN))
            elif name == "bytes_fold":   # (items = output bytes)
                run(name, fold_blocking, lambda: 2 * (n8 + csr) + 2 * (n8 // 8) + 2 * (n8 // 8) + nout.value + csr, note_f)
            elif name == "bytes_fold_wp":   # (items = the untruncated piece total of the folded batch)
                run(name, fold_wp_blocking, lambda: n8 + csr + 4 * n + 4 * n * WP_LEN,
                    "bytes_fold, then bytes_wp_padded on the folded bytes (vocabulary folded alike); alg_bytes are those of bytes_wp_padded alone")
            elif name == "py_fold":   # host blobs in, host rows out, against the host expression
                import unicodedata
                from latok_amd import batch
                m = min(args.py_strings, n)
                blob = u8[:int(boff[m])].tobytes()
                blobs = [blob[int(a):int(b)] for a, b in zip(boff[:m], boff[1:m + 1])]

                def on_host():
                    out = []
                    for b in blobs:
                        t = unicodedata.normalize("NFD", b.decode("utf-8", "surrogatepass").lower())
                        out.append("".join(ch for ch in t if unicodedata.category(ch) != "Mn").encode("utf-8", "surrogatepass"))
                    return out

                routes = (("py_fold_utf8_batch", lambda: batch.fold_utf8_batch(blobs, FOLD)), ("py_lower_nfd_strip_mn", on_host))
                a_rows, b_rows = routes[0][1](), routes[1][1]()
                differ = sum(x != y for x, y in zip(a_rows, b_rows))   # (final sigma, reordered marks: out of scope of the device call)
                for r in range(args.repeat):
                    for rname, fn in routes:
                        t = time.perf_counter()
                        rows = fn()
                        dt = time.perf_counter() - t
                        print(json.dumps({"path": rname, "workload": args.workload, "strings": m, "utf8_bytes": len(blob),
                                          "out_bytes": sum(map(len, rows)), "rows_that_differ": differ, "ms_per_call": dt * 1e3,
                                          "utf8_GBps": len(blob) / dt / 1e9,
                                          "note": "end to end in Python: list[bytes] in, list[bytes] out, pack and host slicing included",
                                          "repeat": r}), flush=True)
            elif name == "py_wp":   # host blobs in, the CSR arrays out, both routes in this process
                from latok_amd import batch
                m = min(args.py_strings, n)
                blob = u8[:int(boff[m])].tobytes()
                blobs = [blob[int(a):int(b)] for a, b in zip(boff[:m], boff[1:m + 1])]
                distinct = list(dict.fromkeys(t for row in batch.tokenize_utf8_batch(blobs) for t in row))
                words = distinct[::2] if args.vocab == "half" else distinct
                words = words + [b"##" + w[2:] for w in words[::3] if len(w) > 3] + list(dict.fromkeys(w[:2] for w in words))
                d = {}
                for i, w in enumerate(words):
                    d.setdefault(w, i)

                def cut(tok):
                    if sum((b & 0xC0) != 0x80 for b in tok[1:]) + 1 > 100:
                        return [-1]
                    out, start, n_tok = [], 0, len(tok)
                    while start < n_tok:
                        for e in range(n_tok, start, -1):
                            if e < n_tok and (tok[e] & 0xC0) == 0x80:
                                continue
                            pid = d.get(tok[start:e] if start == 0 else b"##" + tok[start:e])
                            if pid is not None:
                                break
                        else:
                            return [-1]
                        out.append(pid)
                        start = e
                    return out

                def on_host():
                    indptr, ids = [0], []
                    for row in batch.tokenize_utf8_batch(blobs):
                        for tok in row:
                            ids.extend(cut(tok))
                        indptr.append(len(ids))
                    return np.array(indptr, np.int64), np.array(ids, np.int32)

                with batch.WordPiece(words, seed=SEED) as w:
                    routes = (("py_wordpiece_ids_utf8_batch", lambda: batch.wordpiece_ids_utf8_batch(blobs, w)[:2]),
                              ("py_tokenize_utf8_batch_then_wordpiece_loop", on_host))
                    assert all(np.array_equal(a, b) for a, b in zip(routes[0][1](), routes[1][1]()))
                    for r in range(args.repeat):
                        for rname, fn in routes:
                            t = time.perf_counter()
                            got = fn()
                            dt = time.perf_counter() - t
                            print(json.dumps({"path": rname, "workload": args.workload, "strings": m, "utf8_bytes": len(blob), "vocab": args.vocab,
                                              "words": len(words), "pieces": int(got[1].size), "unk": int((got[1] == -1).sum()), "ms_per_call": dt * 1e3,
                                              "utf8_GBps": len(blob) / dt / 1e9,
                                              "note": "end to end in Python: list[bytes] in, (indptr, ids) out, pack and host work included",
                                              "repeat": r}), flush=True)
            elif name == "bytes_bpe32":   # (items = pieces)
                run(name, bpe_blocking, lambda: n8 + csr + 4 * n + 12 * nout.value, note_b)
            elif name == "bytes_pretok_gpt2":   # (items = pre-tokens, white space included)
                run(name, pretok_gpt2_blocking, lambda: n8 + csr + 4 * n + 8 * nout.value,
                    "UTF-8 bytes + 8 B/string read once by one launch; 2 x 1 bit/byte planes written; 4 B/string + 8 B/pre-token written "
                    "(byte ranges, LATOK_OUT_INT32); every byte lies in a pre-token, so there are more records than bytes_spans32 has")
            elif name == "bytes_bpe_gpt2":   # (items = pieces)
                run(name, bpe_gpt2_blocking, lambda: n8 + csr + 4 * n + 12 * nout.value,
                    note_b + "; the front is GPT-2's pre-tokenizer: one launch for the planes, white-space pre-tokens are merged too")
            elif name == "bytes_pretok_cl100k":   # (items = pre-tokens, white space included)
                run(name, pretok_cl100k_blocking, lambda: 2 * n8 + csr + 4 * n + 8 * nout.value,
                    "UTF-8 bytes + 8 B/string read TWICE by two launches (carry records of 4 B/tile between them); 2 x 1 bit/byte planes written; "
                    "4 B/string + 8 B/pre-token written (byte ranges, LATOK_OUT_INT32)")
            elif name == "bytes_bpe_cl100k":   # (items = pieces)
                run(name, bpe_cl100k_blocking, lambda: 2 * n8 + csr + 4 * n + 12 * nout.value,
                    note_b + "; the front is the cl100k pre-tokenizer: two launches for the planes, white-space pre-tokens are merged too")
            elif name == "bytes_pretok_spm":   # (items = segments, white space included)
                run(name, pretok_spm_blocking, lambda: n8 + csr + 4 * n + 8 * nout.value,
                    "UTF-8 bytes + 8 B/string read once by one launch; 2 x 1 bit/byte planes written; 4 B/string + 8 B/segment written "
                    "(byte ranges, LATOK_OUT_INT32); no class table is read")
            elif name == "bytes_spbpe32":   # (items = pieces)
                run(name, spbpe_blocking, lambda: n8 + csr + 4 * n + 12 * nout.value,
                    note_b + "; the front is SentencePiece's segments: one launch for the planes; the lookups read a virtual text composed on the fly")
            elif name == "bytes_spbpe_padded":   # (items = the untruncated piece total; the block is [n, WP_LEN] with BOS / EOS)
                run(name, spbpe_padded_blocking, lambda: n8 + csr + 4 * n + 4 * n * WP_LEN,
                    note_b.replace("4 B/string indptr + 4 B/piece ids + 8 B/piece spans", "4 B/string lengths + 4 B/cell of the [n, %d] block" % WP_LEN))
            elif name == "py_spbpe":   # host blobs in, the CSR arrays out, both routes in this process
                import re
                from latok_amd import batch
                blobs, blob, toks = bpe_sample_tokens(False)
                blobs = blobs[:50000]
                blob = b"".join(blobs)
                words = spm_words(toks)
                d = {}
                for i, w in enumerate(words):
                    d.setdefault(w.decode(), i)
                n_w, mark, memo = len(words), "\u2581", {}
                seg_pat = re.compile(mark + "*[^" + mark + "]*")

                def cut_spm(seg):
                    got = memo.get(seg)
                    if got is None:
                        parts = list(seg)
                        while True:
                            best = None
                            for i in range(len(parts) - 1):
                                r = d.get(parts[i] + parts[i + 1])
                                if r is not None and (best is None or r < best[0]):
                                    best = (r, i)
                            if best is None:
                                break
                            parts[best[1]:best[1] + 2] = [parts[best[1]] + parts[best[1] + 1]]
                        got = []
                        for p_ in parts:
                            r = d.get(p_)
                            got.extend([r] if r is not None else [n_w + x for x in p_.encode("utf-8", "surrogatepass")])
                        memo[seg] = got
                    return got

                def on_host_spm():
                    memo.clear()   # (the memo is part of the loop: one merge walk per distinct segment of the call)
                    indptr, ids = [0], []
                    for b_ in blobs:
                        if b_:
                            text = mark + b_.decode("utf-8", "surrogatepass").replace(" ", mark)   # (the dummy joins the first lead run)
                            for seg in seg_pat.findall(text):
                                if seg:
                                    ids.extend(cut_spm(seg))
                        indptr.append(len(ids))
                    return np.array(indptr, np.int64), np.array(ids, np.int32)

                with batch.BPE.sentencepiece(words, byte_ids=[n_w + x for x in range(256)], seed=SEED) as b:
                    routes = [("py_spbpe_ids_utf8_batch", lambda: batch.bpe_ids_utf8_batch(blobs, b)[:2]), ("py_replace_split_then_bpe_loop", on_host_spm)]
                    assert all(np.array_equal(x, y) for x, y in zip(routes[0][1](), routes[1][1]()))
                    try:   # beside the two, not a pass condition: the package's own encode of a model made of the same words
                        import sentencepiece as spm
                        from sentencepiece import sentencepiece_model_pb2 as pb2
                        mp = pb2.ModelProto()
                        mp.trainer_spec.model_type, mp.trainer_spec.byte_fallback, mp.trainer_spec.vocab_size = 2, True, 3 + 256 + n_w
                        mp.normalizer_spec.name, mp.normalizer_spec.add_dummy_prefix, mp.normalizer_spec.remove_extra_whitespaces = "identity", True, False
                        for piece, kind in (("<unk>", 2), ("<s>", 3), ("</s>", 3)):
                            mp.pieces.add(piece=piece, score=0.0, type=kind)
                        for x in range(256):
                            mp.pieces.add(piece="<0x%02X>" % x, score=0.0, type=6)
                        for i, w in enumerate(words):
                            mp.pieces.add(piece=w.decode(), score=-float(i), type=1)
                        sp = spm.SentencePieceProcessor(model_proto=mp.SerializeToString())
                        texts = [b_.decode("utf-8", "replace") for b_ in blobs]
                        routes.append(("py_sentencepiece_encode", lambda: (np.zeros(1, np.int64), np.fromiter((i for row in sp.encode(texts) for i in row), np.int32))))
                    except Exception as exc:   # noqa: BLE001
                        print(json.dumps({"path": "py_sentencepiece_encode", "workload": args.workload, "note": "skipped: %s" % str(exc)[:200]}), flush=True)
                    for r in range(args.repeat):
                        for rname, fn in routes:
                            t = time.perf_counter()
                            got = fn()
                            dt = time.perf_counter() - t
                            print(json.dumps({"path": rname, "workload": args.workload, "strings": len(blobs), "utf8_bytes": len(blob),
                                              "words": len(words), "pieces": int(got[1].size), "ms_per_call": dt * 1e3, "utf8_GBps": len(blob) / dt / 1e9,
                                              "note": "end to end in Python: list[bytes] in, (indptr, ids) out, pack and host work included",
                                              "repeat": r}), flush=True)
            elif name in ("py_bpe_gpt2", "py_bpe_cl100k"):   # host blobs in, the CSR arrays out, both routes in this process
                pretokenizer = name[len("py_bpe_"):]
                from latok_amd import batch
                try:
                    import regex
                except ImportError:
                    print(json.dumps({"path": name, "workload": args.workload, "note": "skipped: the `regex` package is not importable"}), flush=True)
                    continue
                blobs, blob, toks = bpe_sample_tokens(False)
                blobs = blobs[:50000]
                blob = b"".join(blobs)
                pat = regex.compile(r"'s|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+" if pretokenizer == "gpt2"
                                    else batch.BPE.CL100K_PATTERN)
                words = bpe_train([b" " + t for t in toks[::2]] + toks[1::2], args.bpe_merges)
                d = {}
                for i, w in enumerate(words):
                    d.setdefault(w, i)
                memo = {}

                def cut_gpt2(tok):
                    got = memo.get(tok)
                    if got is None:
                        if tok in d:
                            got = [d[tok]]
                        else:
                            parts = [tok[i:i + 1] for i in range(len(tok))]
                            while True:
                                best = None
                                for i in range(len(parts) - 1):
                                    r = d.get(parts[i] + parts[i + 1])
                                    if r is not None and (best is None or r < best[0]):
                                        best = (r, i)
                                if best is None:
                                    break
                                parts[best[1]:best[1] + 2] = [parts[best[1]] + parts[best[1] + 1]]
                            got = [d.get(p, -1) for p in parts]
                        memo[tok] = got
                    return got

                def on_host_gpt2():
                    memo.clear()   # (the memo is part of the loop: one merge walk per distinct pre-token of the call)
                    indptr, ids = [0], []
                    for b_ in blobs:
                        for piece in pat.findall(b_.decode("utf-8", "surrogatepass")):
                            ids.extend(cut_gpt2(piece.encode("utf-8", "surrogatepass")))
                        indptr.append(len(ids))
                    return np.array(indptr, np.int64), np.array(ids, np.int32)

                with batch.BPE(words, pretokenizer=pretokenizer, seed=SEED) as b:
                    routes = (("py_bpe_%s_ids_utf8_batch" % pretokenizer, lambda: batch.bpe_ids_utf8_batch(blobs, b)[:2]),
                              ("py_regex_findall_then_bpe_loop", on_host_gpt2))
                    assert all(np.array_equal(x, y) for x, y in zip(routes[0][1](), routes[1][1]()))
                    for r in range(args.repeat):
                        for rname, fn in routes:
                            t = time.perf_counter()
                            got = fn()
                            dt = time.perf_counter() - t
                            print(json.dumps({"path": rname, "workload": args.workload, "strings": len(blobs), "utf8_bytes": len(blob),
                                              "words": len(words), "pieces": int(got[1].size), "unk": int((got[1] == -1).sum()), "ms_per_call": dt * 1e3,
                                              "utf8_GBps": len(blob) / dt / 1e9,
                                              "note": "end to end in Python: list[bytes] in, (indptr, ids) out, pack and host work included",
                                              "repeat": r}), flush=True)
            elif name == "bytes_bpe_padded":   # (items = the untruncated piece total; the block is [n, WP_LEN] with BOS / EOS)
                run(name, bpe_padded_blocking, lambda: n8 + csr + 4 * n + 4 * n * WP_LEN,
                    note_b.replace("4 B/string indptr + 4 B/piece ids + 8 B/piece spans", "4 B/string lengths + 4 B/cell of the [n, %d] block" % WP_LEN))
            elif name == "bytes_uni32":   # (items = pieces)
                run(name, uni_blocking, lambda: n8 + csr + 4 * n + 12 * nout.value,
                    note_b.replace("ranks and part-start masks", "ranks and 24 B/token piece masks").replace("every pair lookup", "every (start, end) lookup"))
            elif name == "bytes_uni_padded":   # (items = the untruncated piece total; the block is [n, WP_LEN] with BOS / EOS)
                run(name, uni_padded_blocking, lambda: n8 + csr + 4 * n + 4 * n * WP_LEN,
                    note_b.replace("4 B/string indptr + 4 B/piece ids + 8 B/piece spans", "4 B/string lengths + 4 B/cell of the [n, %d] block" % WP_LEN)
                    .replace("ranks and part-start masks", "ranks and 24 B/token piece masks").replace("every pair lookup", "every (start, end) lookup"))
            elif name == "py_uni":   # host blobs in, the CSR arrays out, both routes in this process
                from latok_amd import batch
                blobs, blob, toks = bpe_sample_tokens(False)
                words, scores = uni_vocab(toks)
                d = {}
                for i, w in enumerate(words):
                    d.setdefault(w, i)
                unk_score = min(scores) - 10
                longest = max(map(len, words))
                memo = {}

                def cut(tok, marked):
                    got = memo.get((tok, marked))
                    if got is None:
                        text = UNI_MARKER + tok if marked else tok
                        pos = [i for i in range(len(text)) if i == 0 or (text[i] & 0xC0) != 0x80] + [len(text)]
                        k = len(pos) - 1
                        best, back = [None] * (k + 1), [None] * (k + 1)
                        best[0] = 0.0
                        for i in range(k):
                            single = False
                            for j in range(i + 1, k + 1):
                                if pos[j] - pos[i] > longest:
                                    break
                                w = d.get(text[pos[i]:pos[j]])
                                if w is not None:
                                    single = single or j == i + 1
                                    c = best[i] + scores[w]
                                    if best[j] is None or c > best[j]:
                                        best[j], back[j] = c, (i, w)
                            if not single:
                                c = best[i] + unk_score
                                if best[i + 1] is None or c > best[i + 1]:
                                    best[i + 1], back[i + 1] = c, (i, -1)
                        got, j = [], k
                        while j > 0:
                            i, w = back[j]
                            if not (w == -1 and got and got[-1] == -1):   # (fused)
                                got.append(w)
                            j = i
                        got.reverse()
                        memo[(tok, marked)] = got
                    return got

                def on_host():
                    memo.clear()   # (the memo is part of the loop: one search per distinct (token, marked) of the call)
                    u8h, offh = batch.pack_utf8(blobs)
                    counts, spans = batch.token_spans_utf8_bytes_csr(u8h, offh)
                    raw, sp = u8h.tobytes(), spans.tolist()
                    indptr, ids, t = [0], [], 0
                    for s, c in enumerate(counts.tolist()):
                        base, prev = int(offh[s]), -1
                        for _ in range(c):
                            a, e = sp[t]
                            ids.extend(cut(raw[base + a:base + e], prev < a))
                            prev = e
                            t += 1
                        indptr.append(len(ids))
                    return np.array(indptr, np.int64), np.array(ids, np.int32)

                with batch.Unigram(words, scores, seed=SEED) as u:
                    routes = (("py_unigram_ids_utf8_batch", lambda: batch.unigram_ids_utf8_batch(blobs, u)[:2]),
                              ("py_token_spans_then_viterbi_loop", on_host))
                    assert all(np.array_equal(x, y) for x, y in zip(routes[0][1](), routes[1][1]()))
                    for r in range(args.repeat):
                        for rname, fn in routes:
                            t = time.perf_counter()
                            got = fn()
                            dt = time.perf_counter() - t
                            print(json.dumps({"path": rname, "workload": args.workload, "strings": len(blobs), "utf8_bytes": len(blob),
                                              "words": len(words), "pieces": int(got[1].size), "unk": int((got[1] == -1).sum()), "ms_per_call": dt * 1e3,
                                              "utf8_GBps": len(blob) / dt / 1e9,
                                              "note": "end to end in Python: list[bytes] in, (indptr, ids) out, pack and host work included",
                                              "repeat": r}), flush=True)
            elif name in ("ids_detok_bpe", "ids_detok_wp"):   # (items = output bytes) the resident ids of one encode call decoded back
                kind = name[len("ids_detok_"):]
                n_pieces = detok_of(kind)[3]
                _lib.check(bpe_blocking() if kind == "bpe" else wp_blocking())   # (the ids again: another leg may have used their buffer since)
                assert nout.value == n_pieces
                run(name, lambda: detok_blocking(kind), lambda: 4 * n_pieces + 4 * (n + 1) + nout.value + csr, note_d)
            elif name == "py_detok":   # host rows in, list[bytes] out, against the join loop of the host
                from latok_amd import batch
                blobs, blob, toks = bpe_sample_tokens(False)
                words = bpe_train(toks, args.bpe_merges)
                with batch.BPE(words, seed=SEED) as b:
                    indptr, ids, _ = batch.bpe_ids_utf8_batch(blobs, b)
                rows = [ids[a:e] for a, e in zip(indptr[:-1].tolist(), indptr[1:].tolist())]
                with batch.Detokenizer(words) as dt_:
                    routes = (("py_decode_batch", lambda: batch.decode_batch(dt_, rows)),
                              ("py_join_loop", lambda: [b"".join(words[i] for i in row) for row in rows]))
                    assert routes[0][1]() == routes[1][1]()
                    for r in range(args.repeat):
                        for rname, fn in routes:
                            t = time.perf_counter()
                            got = fn()
                            dt = time.perf_counter() - t
                            print(json.dumps({"path": rname, "workload": args.workload, "strings": len(blobs), "pieces": int(ids.size),
                                              "out_bytes": sum(map(len, got)), "ms_per_call": dt * 1e3, "out_GBps": sum(map(len, got)) / dt / 1e9,
                                              "note": "end to end in Python: list of int32 rows in, list[bytes] out, pack and host slicing included",
                                              "repeat": r}), flush=True)
            elif name == "py_bpe":   # host blobs in, the CSR arrays out, both routes in this process
                from latok_amd import batch
                blobs, blob, toks = bpe_sample_tokens(False)
                words = bpe_train(toks, args.bpe_merges)
                d = {}
                for i, w in enumerate(words):
                    d.setdefault(w, i)
                memo = {}

                def cut(tok):
                    got = memo.get(tok)
                    if got is None:
                        if tok in d:
                            got = [d[tok]]
                        else:
                            parts = [tok[i:i + 1] for i in range(len(tok))]
                            while True:
                                best = None
                                for i in range(len(parts) - 1):
                                    r = d.get(parts[i] + parts[i + 1])
                                    if r is not None and (best is None or r < best[0]):
                                        best = (r, i)
                                if best is None:
                                    break
                                parts[best[1]:best[1] + 2] = [parts[best[1]] + parts[best[1] + 1]]
                            got = [d.get(p, -1) for p in parts]
                        memo[tok] = got
                    return got

                def on_host():
                    memo.clear()   # (the memo is part of the loop: one merge walk per distinct token of the call)
                    indptr, ids = [0], []
                    for row in batch.tokenize_utf8_batch(blobs):
                        for tok in row:
                            ids.extend(cut(tok))
                        indptr.append(len(ids))
                    return np.array(indptr, np.int64), np.array(ids, np.int32)

                with batch.BPE(words, seed=SEED) as b:
                    routes = (("py_bpe_ids_utf8_batch", lambda: batch.bpe_ids_utf8_batch(blobs, b)[:2]),
                              ("py_tokenize_utf8_batch_then_bpe_loop", on_host))
                    assert all(np.array_equal(x, y) for x, y in zip(routes[0][1](), routes[1][1]()))
                    for r in range(args.repeat):
                        for rname, fn in routes:
                            t = time.perf_counter()
                            got = fn()
                            dt = time.perf_counter() - t
                            print(json.dumps({"path": rname, "workload": args.workload, "strings": len(blobs), "utf8_bytes": len(blob),
                                              "words": len(words), "pieces": int(got[1].size), "unk": int((got[1] == -1).sum()), "ms_per_call": dt * 1e3,
                                              "utf8_GBps": len(blob) / dt / 1e9,
                                              "note": "end to end in Python: list[bytes] in, (indptr, ids) out, pack and host work included",
                                              "repeat": r}), flush=True)
            elif name in ("bytes_terms32", "bytes_terms_hashed"):   # (items = nnz; the keys are sized by the token total)
                hashed = name == "bytes_terms_hashed"
                run(name, lambda: terms_blocking(hashed), lambda: n8 + csr + 4 * n + (0 if hashed else 4 * n) + 8 * nout.value, note_t)
            elif name in ("bytes_tfidf32", "bytes_tfidf_hashed"):   # (items = nnz) the count call plus the weighting behind it, in place
                hashed = name == "bytes_tfidf_hashed"
                _lib.check(terms_blocking(hashed))
                run(name, lambda: tfidf_blocking(hashed), lambda: n8 + csr + 4 * n + (0 if hashed else 4 * n) + 8 * nout.value + 12 * nout.value,
                    note_t + "; then 8 B/entry read, 4 B/entry written and the idf gathered (L2, smooth idf, an idf fitted on the corpus)")
            elif name == "bytes_df_update":   # (items = nnz) the count call into the context's own buffers plus k_csr_check and k_df_add
                run(name, df_update_blocking, lambda: n8 + csr + 8 * nout.value + 8 * nout.value,
                    note_t + "; then the indices read twice (check, df); timed with the latok_idf_clear in front of every call")
            elif name in ("csr_tfidf", "csr_df"):   # on the device-resident CSR the count call has left: (t_indptr, h_a, h_b)
                _lib.check(terms_blocking(False))
                nnz = nout.value
                t_indptr = terms_box[0]
                if name == "csr_tfidf":
                    if not tfidf_bufs:
                        tfidf_bufs.append(lib.latok_dev_alloc(cap * 4 + 64))
                    f, d_w = tfidf_idf(False), tfidf_bufs[0]
                    run(name, lambda: lib.latok_tfidf_csr(t_indptr, h_a, h_b, n, nnz, f.handle, TFIDF_OPTS, d_w, D32, None),
                        lambda: 12 * nnz + 8 * n, "4 B index + 4 B count read, 4 B weight written per entry; 2 x 4 B/row indptr; the idf gather, "
                        "k_csr_check's pass over the indices and the call's one wait are not counted")
                else:
                    f = tfidf_idf(False, fitted=False)
                    fn_mode = lib.latok_debug_set_df_add
                    fn_mode.restype, fn_mode.argtypes = C.c_int, [C.c_int]
                    for mode, label in ((1, "csr_df_cached"), (0, "csr_df_plain")):
                        fn_mode(mode)

                        def one():
                            _lib.check(lib.latok_idf_clear(f.handle))
                            return lib.latok_idf_update_csr(f.handle, t_indptr, h_a, n, nnz, D32, None)

                        run(label, one, lambda: 8 * nnz + 4 * n, "the indices read twice (k_csr_check, k_df_add), 4 B/row indptr; one global "
                            "atomic per entry (plain) or per occupied LDS slot (cached); timed with the latok_idf_clear in front of every call")
                    fn_mode(1)
            elif name == "py_tfidf":   # host blobs in, the CSR arrays out: the fused call against the count call plus the host transform
                from latok_amd import batch
                m = min(args.py_strings, n)
                blob = u8[:int(boff[m])].tobytes()
                blobs = [blob[int(a):int(b)] for a, b in zip(boff[:m], boff[1:m + 1])]
                words = list(dict.fromkeys(t for row in batch.tokenize_utf8_batch(blobs) for t in row))
                words = words[::2] if args.vocab == "half" else words
                try:
                    import scipy.sparse as sp
                    from sklearn.feature_extraction.text import TfidfTransformer
                    host_name = "py_term_counts_utf8_batch_then_TfidfTransformer"
                except ImportError:
                    sp = None
                    host_name = "py_term_counts_utf8_batch_then_numpy"
                with batch.Vocab(words, seed=SEED) as v, batch.Idf(len(words)) as f:
                    f.update_utf8(blobs, vocab=v)
                    df, n_docs = f.df().astype(np.float64), f.n_docs
                    idf_vec = np.log((n_docs + 1.0) / (df + 1.0)) + 1.0
                    tr = None
                    if sp is not None:
                        tr = TfidfTransformer()
                        tr.idf_ = idf_vec

                    def on_host():
                        indptr, indices, data, oov = batch.term_counts_utf8_batch(blobs, v)
                        if tr is not None:
                            x = tr.transform(sp.csr_matrix((data.astype(np.float64), indices, indptr), shape=(m, len(words))))
                            return indptr, indices, x.data.astype(np.float32), oov
                        w = data * idf_vec[indices]
                        norms = np.sqrt(np.add.reduceat(np.append(w * w, 0.0), np.minimum(indptr[:-1], w.size))) if w.size else np.zeros(m)
                        norms = np.where(np.diff(indptr) > 0, norms, 1.0)
                        return indptr, indices, (w / np.repeat(norms, np.diff(indptr))).astype(np.float32), oov

                    routes = (("py_tfidf_utf8_batch", lambda: batch.tfidf_utf8_batch(blobs, v, f)), (host_name, on_host))
                    a_, b_ = routes[0][1](), routes[1][1]()
                    assert np.array_equal(a_[0], b_[0]) and np.array_equal(a_[1], b_[1]) and np.allclose(a_[2], b_[2], rtol=1e-5, atol=0)
                    for r in range(args.repeat):
                        for rname, fn in routes:
                            t = time.perf_counter()
                            got = fn()
                            dt = time.perf_counter() - t
                            print(json.dumps({"path": rname, "workload": args.workload, "strings": m, "utf8_bytes": len(blob), "vocab": args.vocab,
                                              "words": len(words), "nnz": int(got[1].size), "ms_per_call": dt * 1e3, "utf8_GBps": len(blob) / dt / 1e9,
                                              "note": "end to end in Python: list[bytes] in, (indptr, indices, data float32, oov) out, L2 and smooth "
                                                      "idf, pack and host work included", "repeat": r}), flush=True)
            elif name in ("bytes_ngrams32", "bytes_ngrams_hashed"):   # (items = nnz; the keys are sized by the gram total)
                hashed = name == "bytes_ngrams_hashed"
                run(name, lambda: ngrams_blocking(hashed), lambda: n8 + csr + 4 * n + (0 if hashed else 4 * n) + 8 * nout.value, note_g)
            elif name in ("bytes_chargrams32", "bytes_chargrams_hashed"):   # (items = nnz; the keys are sized by the gram total K)
                hashed = name == "bytes_chargrams_hashed"
                run(name, lambda: chargrams_blocking(hashed), lambda: n8 + csr + 4 * n + (0 if hashed else 4 * n) + 8 * nout.value, note_cg)
            elif name == "py_terms":   # host blobs in, the CSR arrays out, both routes in this process
                import collections
                from latok_amd import batch
                m = min(args.py_strings, n)
                blob = u8[:int(boff[m])].tobytes()
                blobs = [blob[int(a):int(b)] for a, b in zip(boff[:m], boff[1:m + 1])]
                distinct = list(dict.fromkeys(t for row in batch.tokenize_utf8_batch(blobs) for t in row))
                words = distinct[::2] if args.vocab == "half" else distinct
                d = {w: i for i, w in enumerate(words)}

                def on_host():
                    indptr, indices, data, oov = [0], [], [], []
                    for row in batch.tokenize_utf8_batch(blobs):
                        c = collections.Counter(d[t] for t in row if t in d)
                        keys = sorted(c)
                        indices.extend(keys)
                        data.extend(c[k] for k in keys)
                        indptr.append(len(indices))
                        oov.append(len(row) - sum(c.values()))
                    return np.array(indptr, np.int64), np.array(indices, np.int32), np.array(data, np.int32), np.array(oov, np.int64)

                with batch.Vocab(words, seed=SEED) as v:
                    routes = (("py_term_counts_utf8_batch", lambda: batch.term_counts_utf8_batch(blobs, v)),
                              ("py_tokenize_utf8_batch_then_dict_counter", on_host))
                    assert all(np.array_equal(a, b) for a, b in zip(routes[0][1](), routes[1][1]()))
                    for r in range(args.repeat):
                        for rname, fn in routes:
                            t = time.perf_counter()
                            got = fn()
                            dt = time.perf_counter() - t
                            print(json.dumps({"path": rname, "workload": args.workload, "strings": m, "utf8_bytes": len(blob), "vocab": args.vocab,
                                              "words": len(words), "nnz": int(got[1].size), "oov": int(got[3].sum()), "ms_per_call": dt * 1e3,
                                              "utf8_GBps": len(blob) / dt / 1e9,
                                              "note": "end to end in Python: list[bytes] in, (indptr, indices, data, oov) out, pack and host work included",
                                              "repeat": r}), flush=True)
            elif name in ("bytes_count_cold", "bytes_count_warm"):
                run_count(name, name == "bytes_count_warm")
            elif name == "py_count":   # host blobs in, a ranked vocabulary out, both routes in this process
                import collections
                from latok_amd import batch
                m = min(args.py_strings, n)
                blob = u8[:int(boff[m])].tobytes()
                blobs = [blob[int(a):int(b)] for a, b in zip(boff[:m], boff[1:m + 1])]
                rank = lambda items: sorted(items, key=lambda wc: (-wc[1], wc[0]))  # noqa: E731

                def on_device():
                    with batch.TokenCounter(len(blob) // 4 + 64, seed=SEED) as tc:
                        tc.update_utf8(blobs)
                        assert tc.stats["dropped"] == 0
                        return tc.most_common()

                routes = (("py_token_counter_most_common", on_device),
                          ("py_tokenize_utf8_batch_then_counter", lambda: rank(collections.Counter(
                              t for row in batch.tokenize_utf8_batch(blobs) for t in row if len(t) <= 256).items())))
                assert routes[0][1]() == routes[1][1]()
                for r in range(args.repeat):
                    for rname, fn in routes:
                        t = time.perf_counter()
                        ranked = fn()
                        dt = time.perf_counter() - t
                        print(json.dumps({"path": rname, "workload": args.workload, "strings": m, "utf8_bytes": len(blob), "distinct": len(ranked),
                                          "tokens": sum(c for _, c in ranked), "ms_per_call": dt * 1e3, "utf8_GBps": len(blob) / dt / 1e9,
                                          "note": "end to end in Python: list[bytes] in, [(word, count)] ranked by (-count, bytes) out, pack and host work included",
                                          "repeat": r}), flush=True)
            elif name == "py_ids":   # host blobs in, host id rows out, both routes in this process
                from latok_amd import batch
                m = min(args.py_strings, n)
                blob = u8[:int(boff[m])].tobytes()
                blobs = [blob[int(a):int(b)] for a, b in zip(boff[:m], boff[1:m + 1])]
                distinct = list(dict.fromkeys(t for row in batch.tokenize_utf8_batch(blobs) for t in row))
                words = distinct[::2] if args.vocab == "half" else distinct
                d = {w: i for i, w in enumerate(words)}
                with batch.Vocab(words, seed=SEED) as v:
                    routes = (("py_token_ids_utf8_batch", lambda: batch.token_ids_utf8_batch(blobs, v)),
                              ("py_tokenize_utf8_batch_then_dict_get", lambda: [[d.get(t, -1) for t in row] for row in batch.tokenize_utf8_batch(blobs)]))
                    assert [r.tolist() for r in routes[0][1]()] == routes[1][1]()
                    for r in range(args.repeat):
                        for rname, fn in routes:
                            t = time.perf_counter()
                            rows = fn()
                            dt = time.perf_counter() - t
                            print(json.dumps({"path": rname, "workload": args.workload, "strings": m, "utf8_bytes": len(blob), "vocab": args.vocab,
                                              "words": len(words), "tokens": sum(map(len, rows)), "ms_per_call": dt * 1e3,
                                              "utf8_GBps": len(blob) / dt / 1e9,
                                              "note": "end to end in Python: list[bytes] in, one id row per string out, pack and host work included",
                                              "repeat": r}), flush=True)
            else:   # py_join: host blobs in, host rows out, both routes in this process
                from latok_amd import batch
                m = min(args.py_strings, n)
                blob = u8[:int(boff[m])].tobytes()
                blobs = [blob[int(a):int(b)] for a, b in zip(boff[:m], boff[1:m + 1])]
                routes = (("py_join_tokens_utf8_batch", lambda: batch.join_tokens_utf8_batch(blobs)),
                          ("py_tokenize_utf8_batch_then_join", lambda: [b" ".join(t) for t in batch.tokenize_utf8_batch(blobs)]))
                assert routes[0][1]() == routes[1][1]()
                for r in range(args.repeat):
                    for rname, fn in routes:
                        t = time.perf_counter()
                        rows = fn()
                        dt = time.perf_counter() - t
                        print(json.dumps({"path": rname, "workload": args.workload, "strings": m, "utf8_bytes": len(blob),
                                          "out_bytes": sum(map(len, rows)), "ms_per_call": dt * 1e3, "utf8_GBps": len(blob) / dt / 1e9,
                                          "note": "end to end in Python: list[bytes] in, list[bytes] out, pack and host slicing included",
                                          "repeat": r}), flush=True)
        for v_ in detok_box.values():
            v_[0].close()
        if vocab_box:
            vocab_box[0].close()
        if counter_box:
            counter_box[0].close()
        if fold_wp_box:
            fold_wp_box[0].close()
        for p_ in fold_box:
            lib.latok_dev_free(p_)
        if wp_box:
            wp_box[0].close()
            for p_ in wp_box[1:]:
                lib.latok_dev_free(p_)
        for f_ in tfidf_box.values():
            f_.close()
        for p_ in terms_box + ngrams_box + tfidf_bufs + [q for v_ in chargrams_box.values() for q in v_[:2]]:
            lib.latok_dev_free(p_)
        for p_ in jb:
            lib.latok_dev_free(p_)
    if "rules_mask" in paths:
        from latok_amd import batch
        from latok_amd.core import default_tokenizer as dt
        batch.set_rules(dt.C_SPLIT, dt.C_MASK, dt.C_SYM)
        nout.value = 0
        try:
            run("rules_mask", lambda: lib.latok_split_mask_batch(d_cps, d_row, n, total, d_bits, D, None),
                lambda: 4 * total + csr + words * 8, "as mask; tables interpreted at run time")
        finally:
            batch.reset_rules()

    if any(p.startswith("kind_") for p in paths):
        kind = 1 if int(cps.max()) < 256 else 2
        units = cps.astype(np.uint8) if kind == 1 else (cps & 0xFFFF).astype(np.uint16)
        d_units = lib.latok_dev_alloc(units.nbytes + 64)
        _lib.check(lib.latok_memcpy_h2d(d_units, units.ctypes.data, units.nbytes))
        note = f"{kind} B/char + 8 B/string read"
        if "kind_mask_flow" in paths:
            fa, fb = flow_pair(words)
            run_flow("kind_mask_flow", lambda i: lib.latok_flow_split_mask_kind(d_units, kind, d_row, n, total, fb if i & 1 else fa),
                     lambda: kind * total + csr + words * 8, note + "; 1 bit/char written")
        if "kind_mask" in paths:
            nout.value = 0
            run("kind_mask", lambda: lib.latok_split_mask_kind_batch(d_units, kind, d_row, n, total, d_bits, D, None),
                lambda: kind * total + csr + words * 8, note + "; 1 bit/char written")
        if "kind_offsets" in paths:
            run("kind_offsets", lambda: lib.latok_split_offsets_kind_batch(d_units, kind, d_row, n, total, d_counts, d_items, cap, C.byref(nout), D, None),
                lambda: kind * total + csr + 8 * n + 8 * nout.value, note + "; 8 B/string counts + 8 B/boundary written")
        if "kind_offsets32" in paths:
            run("kind_offsets32", lambda: lib.latok_split_offsets_kind_batch(d_units, kind, d_row, n, total, d_counts, d_items, cap, C.byref(nout), D32, None),
                lambda: kind * total + csr + 4 * n + 4 * nout.value, note + "; 4 B/string counts + 4 B/boundary written (LATOK_OUT_INT32)")
        if "kind_spans32" in paths:
            run("kind_spans32", lambda: lib.latok_token_spans_kind_batch(d_units, kind, d_row, n, total, d_counts, d_items, cap, C.byref(nout), D32, None),
                lambda: kind * total + csr + 4 * n + 8 * nout.value, note + "; 4 B/string counts + 8 B/token written (LATOK_OUT_INT32)")
        if "kind_spans" in paths:
            run("kind_spans", lambda: lib.latok_token_spans_kind_batch(d_units, kind, d_row, n, total, d_counts, d_items, cap, C.byref(nout), D, None),
                lambda: kind * total + csr + 8 * n + 16 * nout.value, note + "; 8 B/string counts + 16 B/token written")

    if args.cpu > 0:   # baseline only: the reference's own C (oracle/_ref) under its restated glue, one string at a time
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        import latok_oracle as orc
        m = min(args.cpu, n)
        text = cps[:row[m]].astype("<u4").tobytes().decode("utf-32-le", "surrogatepass")
        strs = [text[row[i]:row[i + 1]] for i in range(m)]
        b8 = int(boff[m])
        try:
            glue = orc.RefGlue()
            kind = "reference"
            offsets = lambda s: np.nonzero(glue.split_values(s))[0]  # noqa: E731
        except Exception:
            kind = "port"
            offsets = orc.split_offsets
        t = time.perf_counter()
        for s in strs:
            offsets(s)
        dt_off = time.perf_counter() - t
        t = time.perf_counter()
        for s in strs:
            nz = offsets(s)
            a, b, toks = int(nz[0]), 0, []
            for b in nz[1:]:
                b = int(b)
                w = s[a:b].strip()
                if w:
                    toks.append(w)
                a = b
            w = s[b:].strip()
            if w:
                toks.append(w)
        dt_tok = time.perf_counter() - t
        for name, dt_ in (("offsets", dt_off), ("tokens", dt_tok)):
            print(json.dumps({"cpu_baseline": name, "kind": kind, "cores": 1, "strings": m, "utf8_bytes": b8,
                              "seconds": dt_, "utf8_GBps": b8 / dt_ / 1e9}), flush=True)


if __name__ == "__main__":
    main()
