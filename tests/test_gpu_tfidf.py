"""TF-IDF on the device (latok_idf_*, latok_tfidf_csr, latok_tfidf_utf8_bytes_batch, latok_hashed_tfidf_utf8_bytes_batch,
include/latok_hip.h).

The inputs are the existing count calls' output on the same batch: indptr, indices and oov must be equal to theirs, and data is held to
tests/helpers/tfidf_ref.py (numpy float64) under the bound of the header: (k + 16) * 2^-23 relative for a normalised row of k stored
entries, 8 * 2^-23 without a norm, exact zeros where the rule says zero.  Document frequencies are held to np.bincount over the count
calls' indices.  The shapes sit on both sides of every threshold latok_debug_tfidf_limits and latok_debug_terms_limits report."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

from helpers import murmur3_collide as mc
from helpers import murmur3_target as mt
from helpers import tfidf_ref as ref
from helpers.murmur3_ref import murmur3_ref

pytestmark = pytest.mark.gpu

OPTS = list(itertools.product((False, True), (False, True), ("l1", "l2", None)))   # smooth_idf, sublinear_tf, norm
N_WORDS = 3000
M32 = 0xFFFFFFFF


def _word(i):
    return bytes(97 + (i // 26 ** k) % 26 for k in (2, 1, 0)) + b"q"


WORDS = [_word(i) for i in range(N_WORDS)]


@functools.lru_cache(maxsize=1)
def limits():
    """(kTfidfSubMax, kTfidfWaveMax, kDfSlots, kTermsRowMax)"""
    from latok_amd import _lib
    lib = _lib.load()
    out = np.zeros(4, np.int64)
    for fn in (lib.latok_debug_tfidf_limits, lib.latok_debug_terms_limits):
        fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    assert lib.latok_debug_tfidf_limits(out.ctypes.data, 3) == 3
    sub, wave, slots = (int(v) for v in out[:3])
    assert lib.latok_debug_terms_limits(out.ctypes.data, 2) == 2
    assert 16 <= sub < wave < N_WORDS - 2 and int(out[1]) < N_WORDS - 2
    return sub, wave, slots, int(out[1])


def _row(k, start=0, repeat=True):
    """a string of k distinct vocabulary words from WORDS[start], word j (1 + j % 3) times"""
    out = []
    for j in range(k):
        out += [WORDS[(start + j) % N_WORDS]] * ((1 + j % 3) if repeat else 1)
    return b" ".join(out)


def _shapes():
    sub, wave, _, row_max = limits()
    ks = sorted({1, 2, 63, 64, 65, sub - 1, sub, sub + 1, wave - 1, wave, wave + 1, row_max + 1, 2500})
    docs = [b"", _row(7, 3), b"  \t ", b"zzzzzz yyyyyy zzzzzz"]
    for i, k in enumerate(ks):
        docs += [_row(k, 11 * i, repeat=k < 200)]
        if i % 4 == 1:
            docs += [b"", b" "]
    return docs + [_row(5, 40), _row(wave + 7, 100, repeat=False)]     # the last row is a long one


@pytest.fixture(scope="module")
def vocab(gpu):
    from latok_amd import batch
    with batch.Vocab(WORDS) as v:
        yield v


@pytest.fixture(scope="module")
def shapes(gpu, vocab):
    """the batch of shapes, its counts (computed once) and an idf fitted on it"""
    from latok_amd import batch
    docs = _shapes()
    counts = batch.term_counts_utf8_batch(docs, vocab)
    idf = batch.Idf(N_WORDS)
    idf.update_utf8(docs, vocab=vocab)
    df = ref.document_frequency(counts[1], N_WORDS)
    assert np.array_equal(idf.df(), df) and idf.n_docs == len(docs)
    yield docs, counts, idf, df
    idf.close()


def _hold(got, counts, idf_vec, sublinear_tf, norm, what=""):
    """got = (indptr, indices, data[, oov]) of a TF-IDF call against the counts' rows and the reference"""
    indptr, indices, data = counts[0], counts[1], counts[2]
    assert np.array_equal(got[0], indptr) and np.array_equal(got[1], indices), what
    if len(got) > 3 and len(counts) > 3 and counts[3] is not None:
        assert np.array_equal(got[3], counts[3]), what
    assert got[2].dtype == np.float32 and got[2].shape == data.shape
    want = ref.weigh(indptr, indices, data, idf_vec, sublinear_tf, norm)
    w, i = ref.worst(got[2], want, indptr, norm)
    assert w <= 1, (what, "entry %d: got %r, want %r, %.2f of the bound" % (i, got[2][i], want[i], w))
    assert (got[2][data == 0] == 0).all() and np.isfinite(got[2]).all()


@pytest.mark.parametrize("use_idf", [False, True])
def test_shapes_every_option(shapes, vocab, use_idf):
    from latok_amd import batch
    docs, counts, idf, df = shapes
    assert counts[3][3] == 3 and np.diff(counts[0])[3] == 0                      # the all-OOV row
    assert np.diff(counts[0]).max() == 2500 and np.diff(counts[0])[-1] > limits()[1]
    for smooth, sub, norm in OPTS:
        got = batch.tfidf_utf8_batch(docs, vocab, idf if use_idf else None, smooth, sub, norm)
        _hold(got, counts, ref.idf(df, len(docs), smooth) if use_idf else None, sub, norm, (use_idf, smooth, sub, norm))


def test_empty_batch_and_one_string(gpu, vocab, shapes):
    from latok_amd import batch
    _, _, idf, df = shapes
    indptr, indices, data, oov = batch.tfidf_utf8_batch([], vocab, idf)
    assert indptr.tolist() == [0] and indices.size == 0 and data.size == 0 and data.dtype == np.float32 and oov.size == 0
    indptr, indices, data, oov = batch.tfidf_utf8_batch([b"", b" "], vocab, idf)
    assert indptr.tolist() == [0, 0, 0] and data.size == 0
    for doc in (_row(1), _row(3, 5), _row(limits()[1] + 1, repeat=False)):
        _hold(batch.tfidf_utf8_batch([doc], vocab, idf), batch.term_counts_utf8_batch([doc], vocab), ref.idf(df, idf.n_docs, True), False, "l2")
    one = batch.tfidf_utf8_batch([_row(1, 9)], vocab, idf)[2]
    assert one.view(np.uint32).tolist() == [0x3F800000]                          # a single entry under L2: exactly 1.0f


def test_widths_pointers_fold_and_ngrams(shapes, vocab):
    """int32 indptr; device pointers (the folded route runs on device buffers) with per-row bit equality to host pointers; fold;
    word n-grams"""
    from latok_amd import batch
    docs, counts, idf, df = shapes
    idf_vec = ref.idf(df, len(docs), True)
    host = batch.tfidf_utf8_batch(docs, vocab, idf, sublinear_tf=True)
    u8, off = batch.pack_utf8(docs)
    narrow = batch.tfidf_utf8_csr(u8, off, vocab, idf, sublinear_tf=True, dtype=np.int32)
    assert narrow[0].dtype == np.int32 and narrow[3].dtype == np.int32
    assert np.array_equal(narrow[0], host[0]) and np.array_equal(narrow[2].view(np.uint32), host[2].view(np.uint32))
    dev = batch.tfidf_utf8_batch(docs, vocab, idf, sublinear_tf=True, fold=batch.FOLD_LOWER)   # lower-case text folds to itself
    for a, b in zip(host, dev):
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    upper = [d.upper() for d in docs[:12]]
    assert batch.tfidf_utf8_batch(upper, vocab, idf)[2].size == 0                # nothing of the upper-case text is in the vocabulary
    _hold(batch.tfidf_utf8_batch(upper, vocab, idf, fold=batch.FOLD_UNCASED), batch.term_counts_utf8_batch(upper, vocab, fold=batch.FOLD_UNCASED),
          idf_vec, False, "l2", "fold")
    grams = [WORDS[i] + b" " + WORDS[i + 1] for i in range(0, 400, 3)] + WORDS[:200]
    with batch.Vocab(grams) as gv, batch.Idf(len(grams)) as gi:
        for rng in ((1, 2), (2, 2)):
            sub_docs = docs[:14]
            gi.clear()
            gi.update_utf8(sub_docs, vocab=gv, ngram_range=rng)
            c = batch.term_counts_utf8_batch(sub_docs, gv, ngram_range=rng)
            assert c[1].size > 0 and np.array_equal(gi.df(), ref.document_frequency(c[1], len(grams)))
            for smooth, sub, norm in ((True, False, "l2"), (False, True, "l1")):
                _hold(batch.tfidf_utf8_batch(sub_docs, gv, gi, smooth, sub, norm, ngram_range=rng), c,
                      ref.idf(gi.df(), gi.n_docs, smooth), sub, norm, ("ngram", rng))
        # a batch with tokens and no key (no string has three tokens): an empty matrix; documents all the same, df as it was
        none = [b"a b", b"c", b""]
        got = batch.tfidf_utf8_batch(none, gv, gi, ngram_range=(3, 3))
        assert got[0].tolist() == [0, 0, 0, 0] and got[1].size == 0 and got[2].size == 0 and got[2].dtype == np.float32 and not got[3].any()
        df_before, docs_before = gi.df().copy(), gi.n_docs
        assert gi.update_utf8(none, vocab=gv, ngram_range=(3, 3)) == 0
        assert gi.n_docs == docs_before + len(none) and np.array_equal(gi.df(), df_before)


def _i32(u):
    return u - (1 << 32) if u >= (1 << 31) else u


def test_hashed_rows_with_alternate_sign(gpu):
    """negative sums, zero sums (two tokens whose hashes are h and -h share a column with opposite signs), a row of zero sums only,
    sublinear tf on negative sums, two colliding words in one column, single entries under L2"""
    from latok_amd import batch
    n_features = 1 << 20
    neg = next(w for w in WORDS if _i32(murmur3_ref(w, 0)) < 0)
    pos = next(w for w in WORDS if _i32(murmur3_ref(w, 0)) > 0)
    pairs = [(mt.token_with_hash(h, 0), mt.token_with_hash((-h) & M32, 0)) for h in (0x12345678, 0x0BADCAFE)]
    a, b = mc.KNOWN_WORD_PAIRS[0]
    assert murmur3_ref(a, 0) == murmur3_ref(b, 0) and a != b
    docs = [b" ".join([neg] * 3 + [pos]),                                    # a negative sum
            b" ".join([pairs[0][0], pairs[0][1], pos, pos, neg]),            # one zero sum among others
            b" ".join([pairs[0][0], pairs[0][1], pairs[1][1], pairs[1][0]]),  # zero sums only
            neg, pos, a + b" " + b + b" " + a, b""]
    counts = batch.hashed_term_counts_utf8_batch(docs, n_features, 0, True)
    rows = [counts[2][counts[0][r]:counts[0][r + 1]].tolist() for r in range(len(docs))]
    assert sorted(rows[0]) == [-3, 1] and 0 in rows[1] and rows[2] == [0, 0] and rows[3] == [-1] and abs(rows[5][0]) == 3
    with batch.Idf(n_features) as idf:
        assert idf.update_utf8(docs, n_features=n_features) == counts[1].size
        df = ref.document_frequency(counts[1], n_features)                      # explicit zeros count
        assert np.array_equal(idf.df(), df) and idf.n_docs == len(docs)
        for use_idf in (False, True):
            for smooth, sub, norm in OPTS:
                got = batch.hashed_tfidf_utf8_batch(docs, n_features, 0, True, idf if use_idf else None, smooth, sub, norm)
                _hold(got, counts, ref.idf(df, len(docs), smooth) if use_idf else None, sub, norm, ("hashed", use_idf, smooth, sub, norm))
                d = got[2]
                assert (d[got[0][2]:got[0][3]].view(np.uint32) == 0).all()          # the zeros are kept: +0.0f, no NaN
                if norm == "l2":
                    assert d[got[0][3]:got[0][5]].view(np.uint32).tolist() == [0xBF800000, 0x3F800000]   # -1.0f, +1.0f
        unsigned = batch.hashed_tfidf_utf8_batch(docs, n_features, 0, False, idf)
        _hold(unsigned, batch.hashed_term_counts_utf8_batch(docs, n_features, 0, False), ref.idf(df, len(docs), True), False, "l2")


def _row_bits(res):
    indptr, indices, data = res[0], res[1], res[2].view(np.uint32)
    return [(indices[a:b].tobytes(), data[a:b].tobytes()) for a, b in zip(indptr[:-1], indptr[1:])]


def test_a_rows_bits_depend_on_the_row_alone(shapes, vocab):
    from latok_amd import batch
    docs, _, idf, _ = shapes
    sub, wave = limits()[:2]
    base = [_row(k, 7 * k % 500, repeat=False) for k in (1, 3, 16, 17, sub, sub + 1, 200, wave, wave + 1)] + [docs[1], b""]
    first = batch.tfidf_utf8_batch(base, vocab, idf, sublinear_tf=True)
    want = dict(zip(base, _row_bits(first)))
    assert _row_bits(batch.tfidf_utf8_batch(base, vocab, idf, sublinear_tf=True)) == _row_bits(first)     # the same batch twice
    rng = np.random.default_rng(3)
    for trial in range(3):
        order = [base[i] for i in rng.permutation(len(base))]
        filler = [_row(int(k), int(s)) for k, s in zip(rng.integers(0, 40, len(order)), rng.integers(0, 900, len(order)))]
        mixed = [d for pair in zip(filler, order) for d in pair][trial % 2:]          # every row starts at another entry offset
        got = _row_bits(batch.tfidf_utf8_batch(mixed, vocab, idf, sublinear_tf=True))
        for doc, bits in zip(mixed, got):
            if doc in want:
                assert bits == want[doc], (trial, len(doc))
    one = batch.tfidf_utf8_batch([base[7]], vocab, idf, sublinear_tf=True)             # another batch size
    assert _row_bits(one) == [want[base[7]]]
    for norm in ("l1", None):
        a = batch.tfidf_utf8_batch(base, vocab, idf, norm=norm)
        b = batch.tfidf_utf8_batch(base[::-1], vocab, idf, norm=norm)
        assert _row_bits(a) == _row_bits(b)[::-1]


def test_fused_call_is_tfidf_csr_on_the_counts(shapes, vocab):
    """bit for bit, with host pointers in both widths of indptr and with device pointers in place"""
    from latok_amd import _lib, batch
    docs, counts, idf, _ = shapes
    lib = _lib.load()
    indptr, indices, data = counts[:3]
    for smooth, sub, norm in OPTS:
        fused = batch.tfidf_utf8_batch(docs, vocab, idf, smooth, sub, norm)[2].view(np.uint32)
        assert np.array_equal(batch.tfidf_csr(indptr, indices, data, idf, smooth, sub, norm).view(np.uint32), fused)
    assert np.array_equal(batch.tfidf_csr(indptr.astype(np.int32), indices, data, idf).view(np.uint32),
                          batch.tfidf_utf8_batch(docs, vocab, idf)[2].view(np.uint32))
    assert np.array_equal(batch.tfidf_csr(indptr, indices, data).view(np.uint32), batch.tfidf_utf8_batch(docs, vocab)[2].view(np.uint32))
    bufs = [lib.latok_dev_alloc(a.nbytes + 64) for a in (indptr, indices, data)]
    try:
        assert all(bufs)
        for p, a in zip(bufs, (indptr, indices, data)):
            _lib.check(lib.latok_memcpy_h2d(p, a.ctypes.data, a.nbytes))
        opts = _lib.TFIDF_SMOOTH_IDF | _lib.TFIDF_SUBLINEAR_TF | _lib.TFIDF_NORM_L2
        _lib.check(lib.latok_tfidf_csr(bufs[0], bufs[1], bufs[2], indptr.size - 1, data.size, idf.handle, opts, bufs[2], _lib.DEVICE_PTRS, None))
        out = np.empty(data.size, np.float32)
        _lib.check(lib.latok_memcpy_d2h(out.ctypes.data, bufs[2], out.nbytes))
        assert np.array_equal(out.view(np.uint32), batch.tfidf_utf8_batch(docs, vocab, idf, True, True, "l2")[2].view(np.uint32))
    finally:
        for p in bufs:
            lib.latok_dev_free(p)


def test_idf_updates_read_load_clear_weights(shapes, vocab):
    from latok_amd import batch
    docs, counts, _, _ = shapes
    thirds = [docs[0::3], docs[1::3], docs[2::3]]
    with batch.Idf(N_WORDS) as idf:
        assert idf.n_docs == 0 and not idf.df().any()
        want = np.zeros(N_WORDS, np.int64)
        for i, part in enumerate(thirds):
            c = batch.term_counts_utf8_batch(part, vocab)
            if i == 1:
                idf.update_csr(c[0].astype(np.int32), c[1])
            elif i == 2:
                idf.update_csr(c[0], c[1])
            else:
                assert idf.update_utf8(part, vocab=vocab) == c[1].size
            want += ref.document_frequency(c[1], N_WORDS)
        assert np.array_equal(idf.df(), want) and idf.n_docs == len(docs)
        assert np.array_equal(want, ref.document_frequency(counts[1], N_WORDS))
        assert (want == 0).any()                                                     # columns no document holds
        for smooth in (True, False):
            got, exact = idf.weights(smooth), ref.idf(want, len(docs), smooth)
            assert np.abs(got - exact).max() <= 2.0 ** -24 * np.abs(exact).max() and ((got == 0) == (exact == 0)).all()
        assert (idf.weights(False)[want == 0] == 0).all() and (idf.weights(True)[want == 0] > 1).all()
        saved, n = idf.df(), idf.n_docs
        idf.clear()
        assert idf.n_docs == 0 and not idf.df().any() and (idf.weights(True) == 1).all()     # the cached vector went with the state
        idf.load(saved, n)
        assert np.array_equal(idf.df(), saved) and idf.n_docs == n
        assert np.abs(idf.weights(True) - ref.idf(want, n, True)).max() <= 2.0 ** -24 * ref.idf(want, n, True).max()


def test_hot_column_and_both_forms_of_df_add(gpu):
    """20 000 rows that all hold column 0 plus one column of their own: the LDS table of k_df_add and its flush, against the plain form"""
    from latok_amd import batch
    lib = gpu
    n = 20000
    indptr = 2 * np.arange(n + 1, dtype=np.int64)
    indices = np.empty(2 * n, np.int32)
    indices[0::2], indices[1::2] = 0, 1 + np.arange(n)
    want = np.bincount(indices, minlength=n + 1)
    lib.latok_debug_set_df_add.restype, lib.latok_debug_set_df_add.argtypes = C.c_int, [C.c_int]
    try:
        for cached in (1, 0):
            lib.latok_debug_set_df_add(cached)
            with batch.Idf(n + 1) as idf:
                idf.update_csr(indptr, indices)
                idf.update_csr(indptr[:-3], indices[3:-3])                               # an odd length (host arrays are staged: an aligned start)
                assert np.array_equal(idf.df(), want + np.bincount(indices[3:-3], minlength=n + 1)) and idf.n_docs == 2 * n - 3
    finally:
        lib.latok_debug_set_df_add(1)


def test_refusals_change_nothing(shapes, vocab):
    from latok_amd import _lib, batch
    docs, counts, idf, df = shapes
    lib = _lib.load()
    n_docs = idf.n_docs
    indptr, indices, data = counts[:3]
    for bad_id in (-1, N_WORDS):
        ids = np.arange(N_WORDS)
        ids[7] = bad_id
        with batch.Vocab(WORDS, ids) as bad:
            with pytest.raises(ValueError, match="column"):
                idf.update_utf8(docs, vocab=bad)
            with pytest.raises(ValueError, match="column"):
                batch.tfidf_utf8_batch(docs, bad, idf)
            assert batch.tfidf_utf8_batch(docs, bad)[2].size == data.size             # without an idf any id is a column
            bad_indices = indices.copy()
            bad_indices[5] = bad_id
            with pytest.raises(ValueError, match="column"):
                idf.update_csr(indptr, bad_indices)
            out = np.full(data.size, 7.0, np.float32)
            rc = lib.latok_tfidf_csr(indptr.ctypes.data, bad_indices.ctypes.data, data.ctypes.data, indptr.size - 1, data.size, idf.handle, 9,
                                     out.ctypes.data, 0, None)
            assert rc == _lib.ERR_INVALID and (out == 7.0).all()
    for broken in (np.concatenate([indptr[:4], indptr[3:4] - 1, indptr[5:]]), np.concatenate([indptr[:-1], indptr[-1:] - 1]),
                   np.concatenate([[1], indptr[1:]])):
        with pytest.raises(ValueError, match="indptr"):
            idf.update_csr(broken, indices)
        with pytest.raises(ValueError, match="indptr"):
            batch.tfidf_csr(broken, indices, data, idf)
        with pytest.raises(ValueError, match="indptr"):
            batch.tfidf_csr(broken, indices, data)
    too_many = df.copy()
    too_many[3] = n_docs + 1
    with pytest.raises(ValueError, match="n_docs"):
        idf.load(too_many, n_docs)
    with pytest.raises(ValueError):
        idf.load(df, -1)
    with pytest.raises(ValueError, match="n_features"):
        idf.update_utf8(docs, n_features=N_WORDS + 1)
    with pytest.raises(ValueError, match="n_features"):
        batch.hashed_tfidf_utf8_batch(docs, N_WORDS + 1, idf=idf)
    with pytest.raises(ValueError):
        idf.update_utf8(docs)
    with pytest.raises(ValueError):
        idf.update_utf8(docs, vocab=vocab, n_features=8)
    for n_cols in (0, 2 ** 28 + 1):
        with pytest.raises(ValueError, match="n_cols"):
            batch.Idf(n_cols)
    with batch.Idf(4) as full:                                                         # df is int32: n_docs stays below 2^31
        full.load(np.array([0, 1, 2, 3]), 2 ** 31 - 3)
        full.update_csr([0, 1, 1], [2])
        with pytest.raises(ValueError, match="2\\^31"):
            full.update_csr([0, 1, 1], [2])
        with pytest.raises(ValueError, match="2\\^31"):
            full.update([""], n_features=4)
        assert full.df().tolist() == [0, 1, 3, 3] and full.n_docs == 2 ** 31 - 1
        full.clear()
        nnz = full.update(["the the cat", "", "cat"], n_features=4)                   # (two words may share one of four columns)
        assert nnz in (2, 3) and full.n_docs == 3 and full.df().sum() == nnz
    u8, off = batch.pack_utf8(docs)
    ip, oov = np.full(len(docs) + 1, -7, np.int64), np.full(len(docs), -7, np.int64)
    ix, out, nnz = np.full(data.size, -7, np.int32), np.full(data.size, 7.0, np.float32), C.c_int64(0)
    for opts in (12, 16):                                                              # both norm bits; an unknown bit
        rc = lib.latok_tfidf_utf8_bytes_batch(u8.ctypes.data, off.ctypes.data, len(docs), u8.size, vocab.handle, 1, 1, 32, idf.handle, opts,
                                              ip.ctypes.data, oov.ctypes.data, ix.ctypes.data, out.ctypes.data, data.size, C.byref(nnz), 0, None)
        assert rc == _lib.ERR_INVALID and (ip == -7).all() and (out == 7.0).all()
    rc = lib.latok_tfidf_utf8_bytes_batch(u8.ctypes.data, off.ctypes.data, len(docs), u8.size, vocab.handle, 1, 1, 32, idf.handle, 9,
                                          ip.ctypes.data, oov.ctypes.data, ix.ctypes.data, out.ctypes.data, data.size - 1, C.byref(nnz), 0, None)
    assert rc == _lib.ERR_INVALID and nnz.value == data.size                           # capacity too small: the need is reported,
    assert np.array_equal(ip, indptr) and np.array_equal(oov, counts[3])               # indptr and oov stay valid,
    assert (ix == -7).all() and (out == 7.0).all()                                     # and no entry is written
    assert np.array_equal(idf.df(), df) and idf.n_docs == n_docs                       # nothing above touched the idf
    _hold(batch.tfidf_utf8_batch(docs, vocab, idf), counts, ref.idf(df, n_docs, True), False, "l2")
