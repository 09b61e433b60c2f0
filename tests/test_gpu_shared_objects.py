"""The threading contract of the device objects (include/latok_hip.h), under the serving pattern of INTEGRATION.md: several threads, each
in a context of its own on ONE device, sharing the objects.

  latok_vocab, latok_wordpiece   "any context of the same device may use it, concurrently"
  latok_bpe, latok_unigram,      "may be used by any context of its device, concurrently"
  latok_detok
  latok_counter                  "calls on one counter are serialised by a lock inside it; two contexts of one device may share it"
  latok_idf                      "calls on one object are serialised by a lock inside it", and the float32 idf vector it keeps per smoothing
                                 mode, computed on one context's stream and handed to the others through an event, dropped by every
                                 update, load and clear
  latok_last_error               the message of the last failure ON THIS THREAD

Every test has the same shape: at most 4 workers, each inside its own _lib.Context(device of the object), released together by a
threading.Barrier; a fixed number of rounds; a worker that raises records the exception and breaks the barrier; the main thread joins with
a timeout and raises the first error; the contexts are destroyed in a finally.

The expected values are plain Python, computed before any thread starts and never by the library under load.  Every document is words
joined by single spaces and tabs, the words hold nothing the default rules split on, so ``blob.split()`` is the tokenisation -- the spans
call confirms that once, from one thread.  Then: ids are a dict lookup; term counts, word n-grams and the counter are collections.Counter
over tokens and over sep.join windows; hashed columns are helpers/murmur3_ref.py under the key rule of the header; WordPiece is
helpers/wordpiece_ref.py; fold is helpers/fold_ref.py; TF-IDF is helpers/tfidf_ref.py under the header's bound ((k + 16) * 2^-23 for a
normalised row of k entries, 8 * 2^-23 without a norm); idf vectors are held to 2^-24 of their largest weight, as tests/test_gpu_tfidf.py
holds them.  Which state of an idf a call saw is decided by helpers/shared_state.py (tests/test_shared_objects_host.py shows what that
judge refuses).  Batch sizes change from round to round (60, 1500 and 300 strings of 0 .. 40 tokens), so that every context's workspaces
and pinned buffers grow and are reused while the other contexts run; a row longer than kTermsRowMax tokens, a row of more than
kTfidfWaveMax distinct entries, runs of empty strings and an all-OOV row sit in the rotation."""
import collections
import ctypes as C
import functools
import threading

import numpy as np
import pytest

from helpers import bpe_ref
from helpers import detok_ref
from helpers import fold_ref
from helpers import pretok_ref
from helpers import shared_state as ss
from helpers import tfidf_ref as ref
from helpers import unigram_ref as uni_ref
from helpers import wordpiece_ref as wpr
from helpers.murmur3_ref import murmur3_ref

pytestmark = pytest.mark.gpu

N_WORDS, IN_VOCAB, N_GRAM_WORDS = 3000, 2600, 300
N_FEATURES, SEED = 1 << 12, 0
SIZES = (60, 1500, 300)                  # strings per batch; round r of a worker takes batch r % 3: grow, reuse, shrink
ROUNDS = 6                               # two turns through the sizes
IDS_ROUTE, TERMS_ROUTE, HASHED_ROUTE, WP_ROUTE, WP_PADDED_ROUTE, NGRAM_ROUTE = 7, 9, 10, 11, 12, 14
WP_UNK, WP_CLS, WP_SEP, WP_PAD, WP_LEN = 1, 2, 3, 0, 12
BARRIER_S, JOIN_S = 60, 180


def _word(i):
    return bytes(97 + (i // 26 ** k) % 26 for k in (2, 1, 0)) + b"q"


WORDS = [_word(i) for i in range(N_WORDS)]
GRAMS = [WORDS[i] + b" " + WORDS[i + 1] for i in range(0, 2 * N_GRAM_WORDS, 2)]     # vocabulary words that hold the separator
VOCAB_WORDS = WORDS[:IN_VOCAB] + GRAMS                                              # WORDS[IN_VOCAB:] are out of vocabulary
VOCAB = {w: i for i, w in enumerate(VOCAB_WORDS)}
LETTERS = range(97, 123)
WP_WORDS = ([b"[PAD]", b"[UNK]", b"[CLS]", b"[SEP]"] + WORDS[:400] + [bytes([x, y]) for x in LETTERS for y in LETTERS if (x * 26 + y) % 5] +
            [b"##" + bytes([y]) + b"q" for y in LETTERS if y % 4] + [b"##q"] + [b"##" + bytes([y]) for y in range(103, 110)])
WP_DICT = wpr.vocab_dict(WP_WORDS)


@functools.lru_cache(maxsize=1)
def _limits():
    """(kTermsRowMax, kTfidfWaveMax)"""
    from latok_amd import _lib
    lib = _lib.load()
    out = np.zeros(4, np.int64)
    for fn in (lib.latok_debug_tfidf_limits, lib.latok_debug_terms_limits):
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    assert lib.latok_debug_tfidf_limits(out.ctypes.data, 3) == 3
    wave = int(out[1])
    assert lib.latok_debug_terms_limits(out.ctypes.data, 2) == 2
    row_max = int(out[1])
    assert max(wave, row_max) + 8 < IN_VOCAB
    return row_max, wave


# ---- the runner every test uses -------------------------------------------------------------------------------------------------------
def _run_workers(jobs, own_context=True, device=0):
    """jobs[k](k, gate) on a thread of its own, inside a context of its own (or, own_context=False, on the default context); all are
    released together by ``gate``, which a job may use again between its rounds"""
    from latok_amd import _lib
    errors = []
    gate = threading.Barrier(len(jobs), timeout=BARRIER_S)
    ctxs = [_lib.Context(device) for _ in jobs] if own_context else []

    def run(k):
        try:
            if own_context:
                with ctxs[k]:
                    gate.wait()
                    jobs[k](k, gate)
            else:
                gate.wait()
                jobs[k](k, gate)
        except BaseException as exc:   # noqa: BLE001 - reported to the main thread
            errors.append(exc)
            try:
                gate.abort()
            except Exception:
                pass

    ths = [threading.Thread(target=run, args=(k,)) for k in range(len(jobs))]
    try:
        for t in ths:
            t.start()
        for t in ths:
            t.join(JOIN_S)
        alive = [t.is_alive() for t in ths]
    finally:
        for ctx, t in zip(ctxs, ths):
            if not t.is_alive():
                ctx.destroy()
    if errors:
        raise errors[0]
    assert not any(alive), "a worker did not finish"


# ---- documents and their references ---------------------------------------------------------------------------------------------------
def _join(words, rng):
    """the words joined by single spaces and (one in four) tabs"""
    if not words:
        return b""
    out = bytearray()
    for w, tab in zip(words, rng.random(len(words)) < 0.25):
        out += w
        out.append(9 if tab else 32)
    return bytes(out[:-1])


def _doc(rng, n_tok, lo=0, hi=N_WORDS):
    """n_tok words of WORDS[lo:hi], skewed to the low ones; every third is followed by its successor, so that the bigram words occur"""
    idx = (rng.random(n_tok) ** 2 * (hi - lo)).astype(np.int64) + lo
    idx[1::3] = np.minimum(idx[0::3][:idx[1::3].size] + 1, hi - 1)
    return _join([WORDS[i] for i in idx], rng)


def _specials(rng):
    """the shapes that matter: a row of more than kTermsRowMax tokens (with repeats), a row of more than kTfidfWaveMax distinct entries, an
    all-OOV row, a run of empty strings"""
    row_max, wave = _limits()
    return [_doc(rng, row_max + 7, 0, 300), _join([WORDS[i] for i in rng.permutation(wave + 9)], rng),
            _join([WORDS[i] for i in rng.integers(IN_VOCAB, N_WORDS, 9)], rng), b"", b"", b"", b"", b""]


def _docs(rng, n_str, special):
    docs = [_doc(rng, int(k)) for k in rng.integers(0, 41, n_str)]
    if special:
        at = n_str // 3
        docs[at:at] = _specials(rng)
    return docs


def _ref_spans(toks):
    """counts and byte spans of the tokens of documents built by _join: one separator byte between two words, none at the ends"""
    spans = []
    for t in toks:
        a = 0
        for w in t:
            spans.append((a, a + len(w)))
            a += len(w) + 1
    return np.array([len(t) for t in toks], np.int64), np.array(spans, np.int64).reshape(-1, 2)


def _ref_csr(rows):
    """rows of (key, value) pairs -> the canonical CSR: distinct keys ascending, values summed (a sum of 0 is kept)"""
    indptr, indices, data = [0], [], []
    for row in rows:
        c = collections.Counter()
        for key, v in row:
            c[key] += v
        for key in sorted(c):
            indices.append(key)
            data.append(c[key])
        indptr.append(len(indices))
    return np.array(indptr, np.int64), np.array(indices, np.int32), np.array(data, np.int32)


def _ref_terms(toks, bigrams=False):
    """(indptr, indices, data, oov) against VOCAB; with bigrams: the grams of orders 1 and 2, joined by one space"""
    rows, oov = [], []
    for t in toks:
        grams = t + [a + b" " + b for a, b in zip(t, t[1:])] if bigrams else t
        rows.append([(VOCAB[g], 1) for g in grams if g in VOCAB])
        oov.append(len(grams) - len(rows[-1]))
    return _ref_csr(rows) + (np.array(oov, np.int64),)


@functools.lru_cache(maxsize=None)
def _hash_key(word):
    """(column, sign) of the header's key rule: h = MurmurHash3 as int32, column = |h| mod n_features, sign = -1 for h < 0"""
    h = murmur3_ref(word, SEED)
    h = h - (1 << 32) if h >= (1 << 31) else h
    return abs(h) % N_FEATURES, (1 if h >= 0 else -1)


def _ref_hashed(toks, alternate_sign=True):
    return _ref_csr([[(_hash_key(w)[0], _hash_key(w)[1] if alternate_sign else 1) for w in t] for t in toks])


@functools.lru_cache(maxsize=None)
def _pieces(word):
    return tuple(wpr.cut(word, WP_DICT, b"##", 100, WP_UNK))


def _ref_wordpiece(toks):
    """(indptr, ids, spans) and the padded block with its attention mask"""
    indptr, ids, spans = [0], [], []
    block = np.full((len(toks), WP_LEN), WP_PAD, np.int32)
    mask = np.zeros((len(toks), WP_LEN), np.int32)
    for s, t in enumerate(toks):
        a, row = 0, []
        for w in t:
            for pid, p0, p1 in _pieces(w):
                row.append(pid)
                spans.append((a + p0, a + p1))
            a += len(w) + 1
        ids += row
        indptr.append(len(ids))
        cells = [WP_CLS] + row[:WP_LEN - 2] + [WP_SEP]
        block[s, :len(cells)] = cells
        mask[s, :len(cells)] = 1
    return (np.array(indptr, np.int64), np.array(ids, np.int32), np.array(spans, np.int64).reshape(-1, 2)), (block, mask)


def _upper(docs):
    """upper-cased text; in every fifth document E carries an acute accent, which FOLD_UNCASED strips"""
    return [d.upper().replace(b"E", "É".encode()) if i % 5 == 0 else d.upper() for i, d in enumerate(docs)]


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        if w is None:
            assert g is None, (what, i)
            continue
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, "array %d" % i, g.shape, w.shape)


class Family:
    """One call family on one batch: ``expect`` (Python, made before any thread starts) and ``check`` (the calls, held to it exactly)"""

    def __init__(self, kind, docs):
        from latok_amd import batch
        self.kind, self.docs = kind, docs
        self.u8, self.off = batch.pack_utf8(docs)
        if kind == 3:
            self.text = _upper(docs)
            fu8, foff = fold_ref.fold_batch(*batch.pack_utf8(self.text), fold_ref.UNCASED)
            raw = bytes(bytearray(fu8))
            self.tok_text = [raw[int(a):int(b)] for a, b in zip(foff[:-1], foff[1:])]       # the tokens are those of the folded strings
            assert self.tok_text != self.text and any(b"\xc3\x89" in t for t in self.text)
        else:
            self.text = self.tok_text = docs
        toks = self.toks = [d.split() for d in self.tok_text]
        self.spans = _ref_spans(toks)
        if kind == 0:
            ids = np.array([VOCAB.get(w, -1) for t in toks for w in t], np.int32)
            self.expect = ((self.spans[0], ids, self.spans[1]), _ref_terms(toks))
        elif kind == 1:
            self.expect = (_ref_terms(toks, bigrams=True), _ref_hashed(toks))
        elif kind == 2:
            self.expect = _ref_wordpiece(toks)
        else:
            self.expect = ([np.array([VOCAB.get(w, -1) for w in t], np.int32) for t in toks], _ref_terms(toks))

    def confirm_tokenisation(self):
        """once, from one thread: the spans call cuts the text the tokens come from exactly where ``split()`` does"""
        from latok_amd import batch
        counts, spans = batch.token_spans_utf8_bytes_csr(*batch.pack_utf8(self.tok_text))
        _same((counts, spans), self.spans, ("spans", self.kind))

    def check(self, objects, route=None):
        """the family's calls against ``expect``; route: the library's debug hook, asked where the context is the thread's own"""
        from latok_amd import batch
        vocab, wp = objects
        if self.kind == 0:
            _same(batch.token_ids_utf8_csr(self.u8, self.off, vocab, -1, spans=True), self.expect[0], "ids with spans")
            assert route is None or route() == IDS_ROUTE
            _same(batch.term_counts_utf8_csr(self.u8, self.off, vocab), self.expect[1], "term counts")
            assert route is None or route() == TERMS_ROUTE
        elif self.kind == 1:
            _same(batch.term_counts_utf8_batch(self.docs, vocab, ngram_range=(1, 2)), self.expect[0], "n-gram counts (1, 2)")
            assert route is None or route() == NGRAM_ROUTE
            _same(batch.hashed_term_counts_utf8_batch(self.docs, N_FEATURES, SEED, alternate_sign=True), self.expect[1], "hashed term counts")
            assert route is None or route() == HASHED_ROUTE
        elif self.kind == 2:
            _same(batch.wordpiece_ids_utf8_batch(self.docs, wp, WP_UNK), self.expect[0], "wordpiece ids")
            assert route is None or route() == WP_ROUTE
            _same(batch.wordpiece_encode_utf8_batch(self.docs, wp, WP_LEN, WP_CLS, WP_SEP, WP_PAD, WP_UNK), self.expect[1], "wordpiece padded")
            assert route is None or route() == WP_PADDED_ROUTE
        else:
            _same(batch.token_ids_utf8_batch(self.text, vocab, -1, fold=batch.FOLD_UNCASED), self.expect[0], "folded ids")
            assert route is None or route() == IDS_ROUTE
            _same(batch.term_counts_utf8_batch(self.text, vocab, fold=batch.FOLD_UNCASED), self.expect[1], "folded term counts")
            assert route is None or route() == TERMS_ROUTE


@pytest.fixture(scope="module")
def shared(gpu):
    """the two immutable objects and, per family, its three batches with their references (made once, never changed)"""
    from latok_amd import batch
    rng = np.random.default_rng(20240)
    families = [[Family(k, _docs(rng, n, special=(n == SIZES[2]))) for n in SIZES] for k in range(4)]
    for fam in families:
        for f in fam:
            f.confirm_tokenisation()
    row_max, wave = _limits()
    long_terms = families[0][2].expect[1]
    assert families[0][2].spans[0].max() > row_max and (families[0][2].spans[0] == 0).sum() >= 5   # a row of more than kTermsRowMax tokens,
    assert np.diff(long_terms[0]).max() > wave and (long_terms[3] > 0).any()                       # one of more than kTfidfWaveMax entries,
    assert ((np.diff(long_terms[0]) == 0) & (long_terms[3] > 0)).any()                             # an all-OOV row
    assert len(families[1][1].expect[0][1]) and (families[1][1].expect[0][1] >= IN_VOCAB).any()    # bigram words are found
    assert (families[1][1].expect[1][2] < 0).any() and (families[2][1].expect[0][1] == WP_UNK).any()
    with batch.Vocab(VOCAB_WORDS) as vocab, batch.WordPiece(WP_WORDS) as wp:
        yield (vocab, wp), families


def _device_of(gpu):
    return gpu.latok_ctx_device(None)


def test_immutable_objects_serve_four_contexts_with_different_families_at_once(gpu, shared):
    """latok_vocab / latok_wordpiece: "any context of the same device may use it, concurrently".  Worker k runs family k -- 0: ids with
    spans and term counts; 1: word n-grams (1, 2) and hashed counts with alternate_sign; 2: WordPiece CSR and padded; 3: fold chained in
    front of ids and term counts, on upper-cased text -- ROUNDS times, on batches of changing size; every array equals the reference."""
    objects, families = shared

    def job(k, gate):
        for r in range(ROUNDS):
            families[k][r % len(SIZES)].check(objects, route=gpu.latok_debug_last_route)

    _run_workers([job] * 4, device=_device_of(gpu))
    assert gpu.latok_ctx_get_current() is None
    for k in range(4):                                               # the default context, from this thread: the same answers
        families[k][2].check(objects, route=gpu.latok_debug_last_route)


def test_three_threads_share_the_default_context_with_different_families(gpu, shared):
    """the same calls where the CONTEXT is shared: its lock serialises the threads, and a call's staging, workspaces and pinned words are
    not touched by the call of another thread that runs in between"""
    objects, families = shared

    def job(k, gate):
        for r in range(3):
            families[(0, 2, 3)[k]][r % len(SIZES)].check(objects)

    _run_workers([job] * 3, own_context=False)


# ---- the counter ----------------------------------------------------------------------------------------------------------------------
COUNTER_MAX_BYTES = 6


def _counter_corpus():
    """[worker][round] -> documents over 1200 short words (5 bytes) and 150 long ones (9 bytes, beyond max_word_bytes)"""
    rng = np.random.default_rng(77)
    short = [bytes(97 + (i // 26 ** k) % 26 for k in (2, 1, 0)) + b"cw" for i in range(1200)]
    long_ = [w[:3] + b"toolong" for w in short[:150]]
    words = short + long_
    slices = []
    for k in range(4):
        slices.append([])
        for r in range(ROUNDS):
            docs = [_join([words[i] for i in (rng.random(int(n)) ** 2 * len(words)).astype(np.int64)], rng) for n in rng.integers(0, 31, 150 + 60 * r)]
            docs[5:5] = [b""] * 3
            slices[k].append(docs)
    return slices


def test_counter_shared_by_four_contexts_counts_exactly(gpu):
    """latok_counter: "calls on one counter are serialised by a lock inside it; two contexts of one device may share it".  Four contexts
    update one counter with disjoint slices, host pointers and LATOK_DEVICE_PTRS in turn, and read it between their rounds."""
    from latok_amd import _lib, batch
    slices = _counter_corpus()
    per_slice = [[collections.Counter(w for d in docs for w in d.split()) for docs in rounds] for rounds in slices]
    total = sum((c for rounds in per_slice for c in rounds), collections.Counter())
    want = collections.Counter({w: c for w, c in total.items() if len(w) <= COUNTER_MAX_BYTES})
    want_long = sum(c for w, c in total.items() if len(w) > COUNTER_MAX_BYTES)
    max_words = 2048
    assert 0 < want_long and len(want) <= max_words and len(want) > 1000
    Family(0, slices[0][0]).confirm_tokenisation()
    snapshots = [[] for _ in slices]

    with batch.TokenCounter(max_words, COUNTER_MAX_BYTES) as tc:
        def job(k, gate):
            lib = _lib.load()
            own = collections.Counter()
            for r, docs in enumerate(slices[k]):
                mine = per_slice[k][r]
                if (k + r) % 2 == 0:
                    st = tc.update_utf8(docs)
                else:
                    u8, off = batch.pack_utf8(docs)
                    d_u8, d_off = lib.latok_dev_alloc(u8.nbytes + 256), lib.latok_dev_alloc(off.nbytes)
                    try:
                        assert d_u8 and d_off and d_u8 % 16 == 0
                        _lib.check(lib.latok_memset_dev(d_u8, 0, u8.nbytes + 256))
                        _lib.check(lib.latok_memcpy_h2d(d_u8, u8.ctypes.data, u8.nbytes))
                        _lib.check(lib.latok_memcpy_h2d(d_off, off.ctypes.data, off.nbytes))
                        _lib.check(lib.latok_sync())
                        out = np.full(4, -7, np.int64)
                        _lib.check(lib.latok_count_tokens_utf8_bytes_batch(d_u8, d_off, len(docs), -1, tc.handle, out.ctypes.data, _lib.DEVICE_PTRS, None))
                        st = dict(zip(tc.STATS[:4], map(int, out)))
                    finally:
                        lib.latok_dev_free(d_u8)
                        lib.latok_dev_free(d_off)
                n_long = sum(c for w, c in mine.items() if len(w) > COUNTER_MAX_BYTES)
                assert st == dict(tokens=sum(mine.values()), counted=sum(mine.values()) - n_long, long=n_long, dropped=0), (k, r, st)
                own += mine
                snap = tc.stats
                words, counts = tc.items()
                snapshots[k].append((snap, dict(zip(words, map(int, counts))), len(words), sum(own.values())))

        _run_workers([job] * 4, device=_device_of(gpu))
        for k, snaps in enumerate(snapshots):                        # every snapshot is one state of the counter
            assert len(snaps) == ROUNDS
            own = collections.Counter()
            for r, (snap, held, n_listed, own_tokens) in enumerate(snaps):
                own += per_slice[k][r]
                assert snap["tokens"] == snap["counted"] + snap["long"] + snap["dropped"] and snap["dropped"] == 0, (k, r, snap)
                assert own_tokens <= snap["tokens"] <= sum(total.values()) and (r == 0 or snap["tokens"] >= snaps[r - 1][0]["tokens"]), (k, r, snap)
                assert len(held) == n_listed, "a word sits in two slots"
                assert all(c <= want.get(w, 0) for w, c in held.items()), (k, r, [w for w, c in held.items() if c > want.get(w, 0)][:5])
                assert all(held.get(w, 0) >= c for w, c in own.items() if len(w) <= COUNTER_MAX_BYTES), (k, r)   # its own updates are in
                assert sum(held.values()) >= snap["counted"] and len(held) >= snap["distinct"]                   # (items() came after stats)
        st = tc.stats
        assert st == dict(tokens=sum(total.values()), counted=sum(want.values()), long=want_long, dropped=0, distinct=len(want)), st
        words, counts = tc.items()
        assert len(set(words)) == len(words) and dict(zip(words, map(int, counts))) == dict(want)
        ranked = [w for w, _ in tc.most_common()]
        assert ranked == [w for w, _ in sorted(want.items(), key=lambda wc: (-wc[1], wc[0]))]
        with tc.to_vocab() as v:                                      # the round trip: a held word's id is its rank, a long word has none
            a_long = next(w for w in total if len(w) > COUNTER_MAX_BYTES)
            ids = batch.token_ids_utf8_batch([b" ".join(ranked), a_long + b"\t" + ranked[7]], v)
            assert ids[0].tolist() == list(range(len(ranked))) and ids[1].tolist() == [-1, 7]


# ---- the idf --------------------------------------------------------------------------------------------------------------------------
def _idf_slices(rng, n_workers, n_rounds):
    slices = [[_docs(rng, 120 + 40 * r, special=(k == 1 and r == 1)) for r in range(n_rounds)] for k in range(n_workers)]
    slices[0][0][3:3] = [b"", b"\t", b" "]
    return slices


@pytest.mark.parametrize("form", ["vocabulary", "hashed"])
def test_idf_updates_from_three_contexts_add_up(gpu, shared, form):
    """latok_idf: "calls on one object are serialised by a lock inside it".  Three contexts update one idf with disjoint slices through
    update_utf8 on text, update_csr with int64 indptr and update_csr with int32 indptr, each worker every route once; df is the reference's
    document frequency over all slices and n_docs counts every string, the empty ones included."""
    from latok_amd import batch
    (vocab, _), _ = shared
    hashed = form == "hashed"
    n_cols = N_FEATURES if hashed else len(VOCAB_WORDS)
    rng = np.random.default_rng(5 + hashed)
    slices = _idf_slices(rng, 3, 3)
    rows = [[(_ref_hashed if hashed else _ref_terms)([d.split() for d in docs]) for docs in rounds] for rounds in slices]
    want_df = sum(ref.document_frequency(c[1], n_cols) for rounds in rows for c in rounds)
    n_docs = sum(len(docs) for rounds in slices for docs in rounds)
    assert want_df.max() > 1 and (want_df == 0).any() and any(d.strip() == b"" for d in slices[0][0])

    with batch.Idf(n_cols) as idf:
        def job(k, gate):
            seen = 0
            for r, docs in enumerate(slices[k]):
                indptr, indices = rows[k][r][:2]
                route = (k + r) % 3
                if route == 0:
                    nnz = idf.update_utf8(docs, n_features=N_FEATURES, seed=SEED) if hashed else idf.update_utf8(docs, vocab=vocab)
                    assert nnz == indices.size, (k, r, nnz, indices.size)
                else:
                    idf.update_csr(indptr if route == 1 else indptr.astype(np.int32), indices)
                seen += len(docs)
                assert seen <= idf.n_docs <= n_docs

        _run_workers([job] * 3, device=_device_of(gpu))
        got = idf.df()
        assert idf.n_docs == n_docs
        assert np.array_equal(got, want_df), np.flatnonzero(got != want_df)[:8]


def _tfidf_batch(rng):
    """the batch the idf tests transform, with the reference's counts"""
    docs = _docs(rng, 200, special=True)
    counts = _ref_terms([d.split() for d in docs])
    return docs, counts


CALLS = [("text", True), ("csr", False), ("weights", True), ("text", False), ("csr", True), ("weights", False)]     # (call, smooth_idf)


def _tfidf_call(call, smooth, docs, counts, vocab, idf):
    from latok_amd import batch
    if call == "text":
        got = batch.tfidf_utf8_batch(docs, vocab, idf, smooth, False, "l2")
        _same((got[0], got[1], got[3]), (counts[0], counts[1], counts[3]), "the rows of the fused call")
        return got[2]
    if call == "csr":
        return batch.tfidf_csr(counts[0], counts[1], counts[2], idf, smooth, False, "l2")
    return idf.weights(smooth)


def _cold_start(gpu, idf, vocab, docs, counts, df, n_docs):
    """one invalidation of the cached vectors, then four contexts at once; returns the largest error over its bound"""
    idf.load(df, n_docs)                                              # drops both cached vectors
    results = [dict() for _ in range(4)]

    def job(k, gate):
        for i in range(len(CALLS)):
            call, smooth = CALLS[(i + (0, 3, 1, 4)[k]) % len(CALLS)]    # the first arrivals ask for different modes through different calls
            results[k][(call, smooth)] = _tfidf_call(call, smooth, docs, counts, vocab, idf)

    _run_workers([job] * 4, device=_device_of(gpu))
    worst = 0.0
    for call, smooth in CALLS:
        vec = ref.idf(df, n_docs, smooth)
        mine = _tfidf_call(call, smooth, docs, counts, vocab, idf)    # the main thread, afterwards, on the default context
        for k in range(4):
            got = results[k][(call, smooth)]
            assert got.dtype == np.float32
            if call == "weights":
                assert ss.match_vector(got, [vec]) == 0, (k, call, smooth)
            else:
                w, i = ref.worst(got, ref.weigh(counts[0], counts[1], counts[2], vec, False, "l2"), counts[0], "l2")
                assert w <= 1, (k, call, smooth, "entry %d, %.2f of the bound" % (i, w))
                worst = max(worst, w)
            assert np.array_equal(got.view(np.uint32), mine.view(np.uint32)), (k, call, smooth, "bits differ from the main thread's")
    for smooth in (True, False):                                      # the fused call is tfidf_csr on the counts, bit for bit
        assert np.array_equal(results[0][("text", smooth)].view(np.uint32), results[3][("csr", smooth)].view(np.uint32))
    return worst


def test_idf_cached_vector_under_a_cold_concurrent_start(gpu, shared):
    """The float32 idf vector is computed once per smoothing mode by the first call that asks, on ITS stream; a call of another context
    waits for that vector's event.  After a load() has dropped both vectors, four contexts ask at once, for both modes in different
    orders, through the fused text call, tfidf_csr and weights().  Every result lies within the header's bound of the reference and has
    the bits the main thread gets afterwards ("a row's output bits depend on that row alone").  Two invalidations, with different df
    and n_docs: a vector that survived the second load would miss the second reference."""
    from latok_amd import batch
    (vocab, _), _ = shared
    rng = np.random.default_rng(404)
    docs, counts = _tfidf_batch(rng)
    n_cols = len(VOCAB_WORDS)
    assert np.diff(counts[0]).max() > _limits()[1]
    fit = [_ref_terms([d.split() for d in _docs(rng, n, special=False)]) for n in (300, 500)]
    states = [(ref.document_frequency(fit[0][1], n_cols), 300),
              (ref.document_frequency(fit[0][1], n_cols) + ref.document_frequency(fit[1][1], n_cols), 800)]
    both = [ref.idf(df, n, True) for df, n in states]
    assert ss.assert_vectors_separable(both) >= 64                   # the two loads cannot be taken for one another
    with batch.Idf(n_cols) as idf:
        first = _cold_start(gpu, idf, vocab, docs, counts, *states[0])
        second = _cold_start(gpu, idf, vocab, docs, counts, *states[1])
        print("cold start: worst error %.2f and %.2f of the bound" % (first, second))


def test_every_transform_sees_one_whole_state_of_the_idf(gpu):
    """One updater takes an idf through J = 6 updates that each double n_docs, over columns the probe rows do not hold (df of the probe
    columns stands still while k_df_add runs); three readers transform the probe batch meanwhile, with and without the L2 norm, in both
    smoothing modes, and read weights().  Every output lies within the bound of exactly one of the J + 1 references, as a whole; in round
    r, between the barrier behind update r - 1 and the one behind update r, that state is r or r + 1; a reader's states never go backwards;
    behind the last update every reader sees state J."""
    from latok_amd import batch
    corpus = ss.StateCorpus()
    J = corpus.n_updates
    words = WORDS[:corpus.n_cols]
    modes = [(True, None), (True, "l2"), (False, None), (False, "l2")]
    indptr, indices, data = corpus.csr
    # on the CPU, before any device work: the states can be told apart
    expected = {m: corpus.expected(*m) for m in modes}
    margins = {m: ss.assert_separable(expected[m], indptr, m[1]) for m in modes}
    vectors = {s: corpus.idf_vectors(s) for s in (True, False)}
    vec_margin = min(ss.assert_vectors_separable(vectors[s]) for s in (True, False))
    print("separation: %s; idf vectors %.0f bounds" % (", ".join("%r %.0f" % (m, v) for m, v in margins.items()), vec_margin))
    rng = np.random.default_rng(1)
    spell = lambda docs: [_join([words[c] for c in doc], rng) for doc in docs]      # noqa: E731
    probe, base, updates = spell(corpus.probe), spell(corpus.base), [spell(u) for u in corpus.updates]
    update_csr = [ss.rows_csr(u)[:2] for u in corpus.updates]
    Family(0, probe + updates[0]).confirm_tokenisation()
    reader_calls = [modes[0], modes[1], "weights", modes[2], modes[3]]
    seen = [[] for _ in range(3)]

    with batch.Vocab(words) as vocab, batch.Idf(corpus.n_cols) as idf:
        assert idf.update_utf8(base, vocab=vocab) == ss.rows_csr(corpus.base)[1].size
        assert np.array_equal(idf.df(), corpus.df[0]) and idf.n_docs == corpus.n_docs[0]
        got = batch.term_counts_utf8_batch(probe, vocab)
        _same(got[:3], corpus.csr, "the probe rows")
        assert not got[3].any()

        def observe(call, n_call):
            if call == "weights":
                smooth = n_call % 2 == 0
                return ss.match_vector(idf.weights(smooth), vectors[smooth])
            smooth, norm = call
            out = batch.tfidf_utf8_batch(probe, vocab, idf, smooth, False, norm)
            _same((out[0], out[1]), (indptr, indices), "the probe rows under load")
            return ss.match_state(out[2], expected[call], indptr, norm)

        def updater(k, gate):
            for j in range(J):
                if j % 3 == 0:
                    assert idf.update_utf8(updates[j], vocab=vocab) == update_csr[j][1].size
                else:
                    idf.update_csr(update_csr[j][0] if j % 3 == 1 else update_csr[j][0].astype(np.int32), update_csr[j][1])
                gate.wait()                                            # update j has returned

        def reader(k, gate):
            n_call = 0
            for r in range(J):
                for i in range(len(reader_calls)):
                    call = reader_calls[(i + k) % len(reader_calls)]
                    seen[k - 1].append(ss.check_window(observe(call, n_call), r, r + 1))
                    n_call += 1
                gate.wait()
            for call in reader_calls:                                  # behind the last update: state J, whatever is asked
                seen[k - 1].append(ss.check_window(observe(call, n_call), J, J))
                n_call += 1

        _run_workers([updater, reader, reader, reader], device=_device_of(gpu))
        for states in seen:
            assert len(states) == (J + 1) * len(reader_calls)
            ss.check_order(states)
        assert np.array_equal(idf.df(), corpus.df[J]) and idf.n_docs == corpus.n_docs[J]
        print("states seen per reader: %s" % [sorted(set(s)) for s in seen])


# ---- the error text -------------------------------------------------------------------------------------------------------------------
THEIR_TEXTS = ("unknown opts bit", "max_n must not exceed", "n_features must be in", "the idf has")


def test_the_error_text_is_the_threads_own(gpu, shared):
    """latok_last_error: "message of the last failure on this thread".  Two workers run exact calls while a third provokes argument
    refusals only -- an unknown opts bit, max_n = 9, n_features = 0, a hashed n_features that is not n_cols: all refused before any device
    work -- and reads its own message each time; the other two never see a word of it."""
    from latok_amd import _lib, batch
    objects, families = shared
    vocab = objects[0]
    lib = _lib.load()
    u8, off = families[0][0].u8, families[0][0].off
    n_str, total = off.size - 1, int(off[-1])
    indptr, indices, data = (np.ascontiguousarray(a) for a in families[0][0].expect[1][:3])
    n_cols = 64
    rounds = 3

    with batch.Idf(n_cols) as idf:
        def exact(k, gate):
            for r in range(rounds):
                families[(0, 2)[k]][r % 2].check(objects, route=gpu.latok_debug_last_route)
                text = _lib.last_error()
                assert not any(t in text for t in THEIR_TEXTS), (k, r, text)

        def refused(k, gate):
            out_ptr, nnz = np.full(n_str + 1, -7, np.int64), C.c_int64(-7)
            out = np.full(data.size, 7.0, np.float32)
            for r in range(rounds * 8):
                rc = lib.latok_tfidf_csr(indptr.ctypes.data, indices.ctypes.data, data.ctypes.data, n_str, data.size, None, 16, out.ctypes.data, 0, None)
                assert rc == _lib.ERR_INVALID and _lib.last_error() == "unknown opts bit"
                rc = lib.latok_ngram_counts_utf8_bytes_batch(u8.ctypes.data, off.ctypes.data, n_str, total, vocab.handle, 1, 9, 32, out_ptr.ctypes.data,
                                                             None, None, None, 0, C.byref(nnz), None, 0, None)
                assert rc == _lib.ERR_INVALID and _lib.last_error() == "max_n must not exceed 8"
                rc = lib.latok_hashed_term_counts_utf8_bytes_batch(u8.ctypes.data, off.ctypes.data, n_str, total, SEED, 0, 1, out_ptr.ctypes.data, None,
                                                                   None, 0, C.byref(nnz), None, 0, None)
                assert rc == _lib.ERR_INVALID and _lib.last_error() == "n_features must be in 1 .. 2^31 - 1"
                rc = lib.latok_idf_update_utf8_bytes_batch(u8.ctypes.data, off.ctypes.data, n_str, total, None, SEED, n_cols + 1, 1, 1, 32, idf.handle,
                                                           C.byref(nnz), None, 0, None)
                assert rc == _lib.ERR_INVALID and _lib.last_error() == "n_features is %d, the idf has %d columns" % (n_cols + 1, n_cols)
                with pytest.raises(ValueError, match="the idf has %d columns" % n_cols):
                    idf.update_utf8(families[0][0].docs, n_features=n_cols + 1)
            assert (out == 7.0).all() and (out_ptr == -7).all()           # nothing was written

        _run_workers([exact, exact, refused], device=_device_of(gpu))
        assert idf.n_docs == 0 and not idf.df().any()


# ---- one lifecycle ----------------------------------------------------------------------------------------------------------------------
LIFE_BLOBS = [b"ab cd ab", b""]                                    # the smallest batch that reaches every object's tables
LIFE_VOCAB = [b"ab", b"cd", b"ef"]
LIFE_WP = [b"[UNK]", b"a", b"##b", b"cd", b"##d"]                  # ab -> a ##b, cd -> cd


def _life_round(lib, device):
    """create, one call that reads the object's device memory, info, close, close again -- for each of the four objects; returns what the
    calls gave, as plain Python"""
    from latok_amd import batch
    i64, u32, ci = C.c_int64, C.c_uint32, C.c_int
    got = {}

    vocab = batch.Vocab(LIFE_VOCAB)
    got["ids"] = [a.tolist() for a in batch.token_ids_utf8_batch(LIFE_BLOBS, vocab)]
    n_words, n_slots, seed, dev = i64(-1), i64(-1), u32(7), ci(-1)
    assert lib.latok_vocab_info(vocab.handle, C.byref(n_words), C.byref(n_slots), C.byref(seed), C.byref(dev)) == 0
    got["vocab"] = (len(vocab), vocab.n_slots, n_words.value, n_slots.value, seed.value, dev.value)

    wp = batch.WordPiece(LIFE_WP)
    indptr, ids, spans = batch.wordpiece_ids_utf8_batch(LIFE_BLOBS, wp, unk_id=0)
    got["wp"] = (indptr.tolist(), ids.tolist(), spans.tolist())
    got["wp_info"] = wp.info()

    idf = batch.Idf(3)
    got["nnz"] = idf.update_utf8(LIFE_BLOBS, vocab=vocab)
    got["df"], got["weights"] = idf.df().tolist(), idf.weights().tolist()
    n_cols, n_docs = i64(-1), i64(-1)
    assert lib.latok_idf_info(idf.handle, C.byref(n_cols), C.byref(n_docs), C.byref(dev)) == 0
    got["idf"] = (n_cols.value, n_docs.value, idf.n_docs, dev.value)

    counter = batch.TokenCounter(4)
    got["update"] = counter.update_utf8(LIFE_BLOBS)
    words, counts = counter.items()
    got["items"] = sorted(zip(words, counts.tolist()))
    max_words, max_bytes = i64(-1), ci(-1)
    assert lib.latok_counter_info(counter.handle, C.byref(max_words), C.byref(n_slots), C.byref(max_bytes), C.byref(seed), C.byref(dev), None) == 0
    got["counter"] = (max_words.value, max_bytes.value, seed.value, dev.value, n_slots.value == counter.n_slots, counter.stats)

    for obj in (counter, idf, wp, vocab):
        obj.close()
        assert obj.handle is None
        obj.close()                                                  # the second close is no call at all
    assert got["vocab"][5] == got["idf"][3] == got["counter"][3] == got["wp_info"]["device"] == device
    return got


def test_the_four_objects_share_one_lifecycle(gpu):
    """Vocab, WordPiece, Idf and TokenCounter on the two-string batch: every value is written out here.  The idf weights are
    ln((n_docs + 1) / (df + 1)) + 1 with n_docs = 2 and df = [1, 1, 0], held to 2^-24 of the largest weight as everywhere in this file.
    Then the NULL handle, and 32 more rounds on the same context that must give the first round's values bit for bit (the library
    exposes no free-memory figure: latok_device_props reports the device's total)."""
    device = _device_of(gpu)
    first = _life_round(gpu, device)
    assert first["ids"] == [[0, 1, 0], []]
    assert first["vocab"] == (3, 64, 3, 64, 0, device)
    assert first["wp"] == ([0, 5, 5], [1, 2, 3, 1, 2], [[0, 1], [1, 2], [3, 5], [6, 7], [7, 8]])
    assert first["wp_info"] == dict(n_words=5, n_slots_initial=64, n_slots_cont=64, max_len_initial=5, max_len_cont=1, prefix=b"##", max_chars=100,
                                    seed=0, device=device)
    assert first["nnz"] == 2 and first["df"] == [1, 1, 0] and first["idf"] == (3, 2, 2, device)
    want = np.array([1.4054651081081644, 1.4054651081081644, 2.09861228866811])
    assert np.abs(np.array(first["weights"]) - want).max() <= 2.0 ** -24 * want.max(), first["weights"]
    assert first["update"] == dict(tokens=3, counted=3, long=0, dropped=0)
    assert first["items"] == [(b"ab", 2), (b"cd", 1)]
    assert first["counter"] == (4, 256, 0, device, True, dict(tokens=3, counted=3, long=0, dropped=0, distinct=2))
    for destroy in (gpu.latok_vocab_destroy, gpu.latok_wordpiece_destroy, gpu.latok_idf_destroy, gpu.latok_counter_destroy):
        assert destroy(None) == 0
    for r in range(32):
        assert _life_round(gpu, device) == first, r


# ---- the later immutable objects: BPE, Unigram, Detokenizer ------------------------------------------------------------------------------
# latok_bpe, latok_unigram, latok_detok: "may be used by any context of its device, concurrently".  The word lists are fixed and built
# without the library; the expected values are helpers/bpe_ref.py, unigram_ref.py, pretok_ref.py and detok_ref.py over the file's tokens.
PIECE_UNK, PIECE_BOS, PIECE_EOS, PIECE_PAD, PIECE_LEN, PIECE_MAX_BYTES = -1, 5001, 5002, 5003, 12, 24
P_BPE_WORDS = bpe_ref.train(WORDS[:500], 120, base=[x for x in range(256) if x != ord("z")])       # no `z`: every word with one leaves an unk piece
P_GPT2_WORDS = P_BPE_WORDS + [b" " + w for w in P_BPE_WORDS if len(w) > 1] + [b" ", b"  ", b"\t"]
P_BPE_DICT, P_GPT2_DICT = bpe_ref.rank_dict(P_BPE_WORDS), bpe_ref.rank_dict(P_GPT2_WORDS)
P_UNI_PLAIN = [bytes([x]) for x in LETTERS if x != ord("z")] + sorted({w[:k] for w in WORDS[:900] for k in (2, 3, 4)})
P_UNI_WORDS = [w for i, p in enumerate(P_UNI_PLAIN) for w in ([p, uni_ref.MARKER + p] if i % 3 == 0 else [p])] + [uni_ref.MARKER]
P_UNI_SCORES = np.array([-(8 + (i * 7) % 13) / 8 for i in range(len(P_UNI_WORDS))], np.float32)   # multiples of 1/8: every sum is exact
P_UNI_DICT, P_UNI_UNK_SCORE = uni_ref.word_dict(P_UNI_WORDS), -20.0
P_DETOK_MAP = detok_ref.id_map(P_BPE_WORDS)
P_DETOK_SKIP = (P_BPE_DICT[b"a"], P_BPE_DICT[b"q"])
assert len(P_GPT2_WORDS) < PIECE_BOS


@functools.lru_cache(maxsize=None)
def _bpe_cut(token, gpt2=False):
    return tuple(bpe_ref.cut(token, P_GPT2_DICT if gpt2 else P_BPE_DICT, PIECE_MAX_BYTES, PIECE_UNK))


@functools.lru_cache(maxsize=None)
def _uni_cut(token, marked):
    return tuple(uni_ref.cut(token, marked, P_UNI_DICT, P_UNI_SCORES, P_UNI_UNK_SCORE, uni_ref.MARKER, True, PIECE_MAX_BYTES, PIECE_UNK))


def _piece_rows(rows):
    """rows of [(id, start, end)] -> (indptr, ids, spans) as the ids calls return them"""
    indptr = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=indptr[1:])
    flat = [p for r in rows for p in r]
    return indptr, np.array([p[0] for p in flat], np.int32), np.array([p[1:] for p in flat], np.int64).reshape(-1, 2)


class Pieces:
    """One of the four later call families on one batch of documents built by _join (a token touches no other: one separator byte lies
    between two): 0 BPE ids on the latok-token object with lead_space, 1 the padded BPE block on the GPT-2 object, 2 Unigram ids, 3 the
    decoder on the reference BPE ids of kind 0"""

    def __init__(self, kind, docs):
        self.kind, self.docs = kind, docs
        rows = []
        for d in docs:
            row = []
            if kind == 1:
                for a, e in pretok_ref.pretokens(d):
                    row += [(i, a + p0, a + p1) for i, p0, p1 in _bpe_cut(d[a:e], True)]
            else:
                a = 0
                for w in d.split():
                    if kind == 2:                                    # behind a separator or at the start: every token takes the marker
                        row += [(i, a + p0, a + p1) for i, p0, p1 in _uni_cut(w, True)]
                    else:
                        lead = 1 if a > 0 and d[a - 1] == 0x20 else 0
                        row += [(i, a - lead + p0, a - lead + p1) for i, p0, p1 in _bpe_cut(d[a - lead:a + len(w)])]
                    a += len(w) + 1
            rows.append(row)
        self.csr = _piece_rows(rows)
        if kind == 1:
            block, mask = np.full((len(docs), PIECE_LEN), PIECE_PAD, np.int32), np.zeros((len(docs), PIECE_LEN), np.int32)
            for s, r in enumerate(rows):
                cells = [PIECE_BOS] + [p[0] for p in r][:PIECE_LEN - 2] + [PIECE_EOS]
                block[s, :len(cells)], mask[s, :len(cells)] = cells, 1
            self.expect = (block, mask)
        elif kind == 3:
            texts, self.unknown = detok_ref.decode([[p[0] for p in r] for r in rows], P_DETOK_MAP, detok_ref.CONCAT, skip=P_DETOK_SKIP)
            off = np.zeros(len(docs) + 1, np.int64)
            np.cumsum([len(t) for t in texts], out=off[1:])
            self.expect = (np.frombuffer(b"".join(texts), np.uint8), off)
        else:
            self.expect = self.csr

    def check(self, objects):
        from latok_amd import batch
        bpe, gpt2, uni, detok = objects
        if self.kind == 0:
            _same(batch.bpe_ids_utf8_batch(self.docs, bpe, PIECE_UNK), self.expect, "bpe ids")
        elif self.kind == 1:
            _same(batch.bpe_encode_utf8_batch(self.docs, gpt2, PIECE_LEN, PIECE_BOS, PIECE_EOS, PIECE_PAD, PIECE_UNK), self.expect, "bpe padded on GPT-2's pre-tokens")
        elif self.kind == 2:
            _same(batch.unigram_ids_utf8_batch(self.docs, uni, PIECE_UNK), self.expect, "unigram ids")
        else:
            _same(batch.decode_csr(detok, self.csr[0], self.csr[1], P_DETOK_SKIP, errors="ignore"), self.expect, "decoded rows")
            with pytest.raises(ValueError, match="^%d ids are not in the decoder" % self.unknown):
                batch.decode_csr(detok, self.csr[0], self.csr[1], P_DETOK_SKIP)


@pytest.fixture(scope="module")
def shared_pieces(gpu, shared):
    """the shared fixture's first family's three batches under the four later families, and the objects they share"""
    from latok_amd import batch
    _, families = shared
    pieces = [[Pieces(k, f.docs) for f in families[0]] for k in range(4)]
    for f in families[0]:
        assert f.toks == [d.split() for d in f.docs]                  # the tokens confirm_tokenisation held the spans call to
    big = pieces[0][1]
    assert (big.csr[1] == PIECE_UNK).any() and (np.diff(big.csr[2], axis=1) > 1).any()                      # unk pieces, merged pieces,
    assert pieces[3][1].unknown > 0 and any((big.csr[1] == s).any() for s in P_DETOK_SKIP)                  # unknown and skipped ids,
    assert (pieces[1][1].expect[1].sum(axis=1) == PIECE_LEN).any() and (pieces[1][2].expect[1].sum(axis=1) == 2).any()   # truncated and empty rows,
    assert (pieces[2][1].csr[1] == PIECE_UNK).any() and len(set(pieces[2][1].csr[1].tolist())) > 100        # many Unigram words
    with batch.BPE(P_BPE_WORDS, max_bytes=PIECE_MAX_BYTES, lead_space=True) as bpe, \
            batch.BPE(P_GPT2_WORDS, max_bytes=PIECE_MAX_BYTES, pretokenizer="gpt2") as gpt2, \
            batch.Unigram(P_UNI_WORDS, P_UNI_SCORES, unk_score=P_UNI_UNK_SCORE, fuse_unk=True, max_bytes=PIECE_MAX_BYTES) as uni, \
            batch.Detokenizer(P_BPE_WORDS) as detok:
        yield (bpe, gpt2, uni, detok), pieces


def test_piece_objects_serve_four_contexts_with_different_families_at_once(gpu, shared_pieces):
    """latok_bpe / latok_unigram / latok_detok: "may be used by any context of its device, concurrently".  Worker k runs family k -- 0: BPE
    ids on the latok-token object; 1: the padded BPE block on the GPT-2 object; 2: Unigram ids; 3: the decoder on the reference BPE ids --
    ROUNDS times, on batches of changing size; every array equals the reference."""
    objects, pieces = shared_pieces

    def job(k, gate):
        for r in range(ROUNDS):
            pieces[k][r % len(SIZES)].check(objects)

    _run_workers([job] * 4, device=_device_of(gpu))
    assert gpu.latok_ctx_get_current() is None
    for k in range(4):                                               # the default context, from this thread: the same answers
        pieces[k][2].check(objects)


LIFE_BPE = [b"a", b"b", b"ab", b"c"]                               # ab -> ab, cd -> c and an unknown byte
LIFE_UNI = [b"ab", uni_ref.MARKER + b"ab", b"c", b"d", uni_ref.MARKER]
LIFE_DETOK = [b"ab", b"cd", b" "]


DRAIN_BYTES, DRAIN_SETS = 256 << 20, 8                             # 2 GiB of device memsets: far longer in flight than the way to destroy


def _destroy_behind_work(lib, obj, d_buf, flag):
    """The object's destroy behind asynchronous work of the current context: DRAIN_SETS memsets of DRAIN_BYTES and then one of the pinned
    ``flag``, all enqueued by latok_memset_dev, which returns without waiting.  "latok_*_destroy drains the current context first": when
    the destroy has returned 0 the flag, read from pinned memory with no further wait of any kind, is set everywhere.  Returns whether
    the flag was still clear when the destroy was called, that is, whether there was something to drain."""
    from latok_amd import _lib
    flag[:] = 0                                                      # (nothing is in flight: the close before this one drained)
    for _ in range(DRAIN_SETS):
        _lib.check(lib.latok_memset_dev(d_buf, 0, DRAIN_BYTES))
    _lib.check(lib.latok_memset_dev(flag.ctypes.data, 0x5A, flag.nbytes))
    pending = not flag.any()
    h, obj.handle = obj.handle, None
    assert getattr(lib, obj._destroy)(h) == 0
    assert (flag == 0x5A).all(), "%s returned before the context's stream had drained" % obj._destroy
    return pending


def _life_round_pieces(lib, device, d_buf, flag, pending):
    """create, one call that reads the object's device memory, info, destroy behind work in flight, a refused use, close again -- for BPE,
    Unigram, Detokenizer"""
    from latok_amd import batch
    got = {}
    bpe = batch.BPE(LIFE_BPE)
    got["bpe"] = [a.tolist() for a in batch.bpe_ids_utf8_batch(LIFE_BLOBS, bpe)]
    got["bpe_info"] = bpe.info()
    uni = batch.Unigram(LIFE_UNI, [-1.0] * 5, unk_score=-11.0)
    got["uni"] = [a.tolist() for a in batch.unigram_ids_utf8_batch(LIFE_BLOBS, uni)]
    got["uni_info"] = uni.info()
    detok = batch.Detokenizer(LIFE_DETOK)
    got["detok"] = batch.decode_batch(detok, [[0, 2, 1, 7], []], errors="ignore")
    got["detok_info"] = detok.info()
    for obj, use in ((detok, lambda: batch.decode_batch(detok, [[0]])), (uni, lambda: batch.unigram_ids_utf8_batch(LIFE_BLOBS, uni)),
                     (bpe, lambda: batch.bpe_ids_utf8_batch(LIFE_BLOBS, bpe))):
        pending.append(_destroy_behind_work(lib, obj, d_buf, flag))
        assert obj.handle is None
        with pytest.raises(ValueError, match="must be an open latok_amd.batch"):     # the wrapper's refusal: the library never sees the handle
            use()
        with pytest.raises(ValueError, match="must be an open latok_amd.batch"):
            obj.info()
        obj.close()                                                  # the second close is no call at all
    assert got["bpe_info"]["device"] == got["uni_info"]["device"] == got["detok_info"]["device"] == device
    return got


def test_the_three_piece_objects_share_that_lifecycle(gpu):
    """BPE, Unigram and Detokenizer on the two-string batch of test_the_four_objects_share_one_lifecycle, every value written out.
    * The destroy drains the current context: it is called behind 2 GiB of asynchronous memsets and a last one that sets a pinned flag,
      it returns 0, and the flag is then set with no further wait (_destroy_behind_work).  In at least one of the 99 destroys the flag
      was still clear when the destroy was called; the count is printed.
    * Use after close is refused BY THE WRAPPER, which drops the handle: a ValueError before any library call.  The library cannot
      refuse a freed handle, it is a plain pointer; that a closed object never reaches it is what is pinned here.
    * The second close is harmless, the NULL handle is accepted, and 32 more rounds give the first round's values."""
    from latok_amd import batch
    device = _device_of(gpu)
    flag, pending = batch.pinned_empty(64, np.uint8), []
    d_buf = gpu.latok_dev_alloc(DRAIN_BYTES)
    assert d_buf
    try:
        first = _life_round_pieces(gpu, device, d_buf, flag, pending)
        rounds = [_life_round_pieces(gpu, device, d_buf, flag, pending) for _ in range(32)]
    finally:
        gpu.latok_sync()
        gpu.latok_dev_free(d_buf)
    print("destroys that found work in flight: %d of %d" % (sum(pending), len(pending)))
    assert len(pending) == 99 and any(pending)
    assert first["bpe"] == [[0, 4, 4], [2, 3, -1, 2], [[0, 2], [3, 4], [4, 5], [6, 8]]]
    info = dict(first["bpe_info"])
    assert info.pop("n_slots") >= 4 and info == dict(n_words=4, max_len=2, max_bytes=4096, lead_space=0, seed=0, device=device)
    assert first["uni"] == [[0, 5, 5], [1, 4, 2, 3, 1], [[0, 2], [3, 3], [3, 4], [4, 5], [6, 8]]]
    info = dict(first["uni_info"])
    assert info.pop("n_slots_plain") >= 5 and info.pop("n_slots_marked") >= 1
    assert info == dict(n_words=5, max_len=5, marker_word=4, marker=uni_ref.MARKER, unk_score=-11.0, fuse_unk=1, max_bytes=4096, seed=0, device=device)
    assert first["detok"] == [b"ab cd", b""]
    assert first["detok_info"] == dict(n_words=3, n_ids=3, blob_bytes=12, max_len=2, mode=0, dense=1, device=device)       # (the blob holds every word in whole 4-byte units)
    for destroy in (gpu.latok_bpe_destroy, gpu.latok_unigram_destroy, gpu.latok_detok_destroy):
        assert destroy(None) == 0
    for r, got in enumerate(rounds):
        assert got == first, r
