"""Per-string term counts on the device (latok_term_counts_utf8_bytes_batch, latok_hashed_term_counts_utf8_bytes_batch,
include/latok_hip.h): the CSR rows of a document-term matrix.

The result is DEFINED by a call the parity tests already pin and by Python's own containers: the byte slices
latok_token_spans_utf8_bytes_batch reports for string s, fed to a dict (vocabulary form: the ids with their counts, ascending as
signed int32, plus the number of slices the dict does not hold) or to tests/helpers/murmur3_ref.py (hashed form: column = |h| mod
n_features, value = -1 iff alternate_sign and h < 0, sums that may be 0 kept).  Every batch goes through the C ABI with poisoned
guard bands round every output and is checked in full against that definition.  The shapes are the smallest at which the kernels
can go wrong, with the tile and the longest short row read from the library (latok_debug_terms_limits)."""
import ctypes as C
import functools
import os
import random
import subprocess
from collections import Counter

import numpy as np
import pytest

from conftest import ALPHABETS, ROOT, random_strings
from helpers import murmur3_target as mt
from helpers import span_strip_content as ssc
from helpers.murmur3_ref import murmur3_ref

pytestmark = pytest.mark.gpu

POISON = 0xA5
POISON_32 = np.int32(-0x5A5A5A5B)        # 0xA5A5A5A5 as int32
GUARD = 16
TERMS_ROUTE, HASHED_ROUTE, IDS_ROUTE, HASH_ROUTE = 9, 10, 7, 6
ONE_TOKEN_PER_STRING = (ssc._NONE, ssc._NONE, ssc._NONE)
SOFT = [b"ab\xe6\x97 cd", b"\xc3 x", b"lone \xf0\x9f\x98", b"end\xe6", b"next starts ascii", b"\xe6\x97\xa5\xe6", b"\xf0", b"x\xc3"]
HARD = [b"a\x80\x80\x80\x80b", b"\xa9 starts with a continuation byte"]
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
EDGE_IDS = [INT32_MIN, -1, 0, 1, 255, 256, 65535, 65536, 1 << 24, INT32_MAX]
ONE_BYTE_APART = [0x01020304, 0x01020305, 0x01020404, 0x01030304, 0x02020304, 0x0102FF04, 0x01FF0304, 0x7F020304]


@functools.lru_cache(maxsize=1)
def limits():
    """(kTermsTile, kTermsRowMax) from latok_debug_terms_limits"""
    from latok_amd import _lib
    fn = _lib.load().latok_debug_terms_limits
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    out = np.zeros(4, np.int64)
    assert fn(out.ctypes.data, 4) == 2
    tile, row_max = int(out[0]), int(out[1])
    assert 64 <= row_max <= tile <= 1 << 16
    return tile, row_max


def wave_bytes():
    """kHashWaveBytes: entry 14 of latok_debug_limits"""
    from latok_amd import _lib
    fn = _lib.load().latok_debug_limits
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    out = np.zeros(15, np.int64)
    assert fn(out.ctypes.data, 15) == 15 and out[14] >= 64
    return int(out[14])


# ---- the definition --------------------------------------------------------------------------------------------------------
def _i32(u):
    return u - (1 << 32) if u >= (1 << 31) else u


def _rows_of_slices(u8, boff):
    """the byte slices of the spans call, one list per string"""
    from latok_amd import batch
    counts, spans = batch.token_spans_utf8_bytes_csr(u8, boff)
    raw = u8.tobytes()
    base = np.repeat(boff[:-1], counts)
    lo, hi = (base + spans[:, 0]).tolist(), (base + spans[:, 1]).tolist()
    toks = [raw[a:b] for a, b in zip(lo, hi)]
    ends = np.cumsum(counts).tolist()
    return [toks[a:b] for a, b in zip([0] + ends[:-1], ends)]


def _dict(words, ids=None):
    d = {}
    for i, w in enumerate(words):
        if w:
            d.setdefault(w, i if ids is None else ids[i])
    return d


def _csr(counters):
    """sorted rows -> (indptr, indices, data)"""
    indptr, indices, data = [0], [], []
    for c in counters:
        for k in sorted(c):
            indices.append(k)
            data.append(c[k])
        indptr.append(len(indices))
    return np.array(indptr, np.int64), np.array(indices, np.int64).astype(np.int32), np.array(data, np.int64).astype(np.int32)


def want_vocab(rows, d):
    counters = [Counter(d[t] for t in row if t in d) for row in rows]
    oov = np.array([sum(t not in d for t in row) for row in rows], np.int64)
    return _csr(counters) + (oov,)


_HASHES = {}


def want_hashed(rows, n_features, seed, alternate_sign):
    counters = []
    for row in rows:
        c = Counter()
        for t in row:
            h = _HASHES.get((t, seed))
            if h is None:
                h = _HASHES[(t, seed)] = _i32(murmur3_ref(t, seed))
            c[abs(h) % n_features] += -1 if alternate_sign and h < 0 else 1
        counters.append(c)
    return _csr(counters)


# ---- the calls, with guard bands ---------------------------------------------------------------------------------------------
class _Out:
    def __init__(self, n_str, cap, dt):
        self.n_str, self.cap = n_str, cap
        self.indptr = np.full(n_str + 1 + GUARD, -7, dt)
        self.oov = np.full(n_str + GUARD, -7, dt)
        self.indices = np.full(cap + GUARD, POISON_32, np.int32)
        self.data = np.full(cap + GUARD, POISON_32, np.int32)

    def entries_untouched(self):
        return (self.indices == POISON_32).all() and (self.data == POISON_32).all()


def _call(lib, u8, boff, vocab=None, hashed=None, cap=0, dt=np.int64, want_oov=True, want_entries=True, total=None, flags=0):
    """one blocking call with host pointers -> (rc, nnz, n_tokens, _Out); hashed = (n_features, seed, alternate_sign)"""
    from latok_amd import _lib
    n_str = boff.size - 1
    total = (int(boff[-1]) if n_str > 0 else 0) if total is None else total
    o = _Out(n_str, cap, dt)
    nnz, n_tok = C.c_int64(-1), C.c_int64(-1)
    flags |= _lib.OUT_INT32 if dt == np.int32 else 0
    ix, da = (o.indices.ctypes.data, o.data.ctypes.data) if want_entries else (None, None)
    if hashed is not None:
        n_features, seed, alt = hashed
        rc = lib.latok_hashed_term_counts_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, n_str, total, seed, n_features, int(alt),
                                                           o.indptr.ctypes.data, ix, da, cap, C.byref(nnz), C.byref(n_tok), flags, None)
    else:
        rc = lib.latok_term_counts_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, n_str, total, vocab.handle if vocab is not None else None,
                                                    o.indptr.ctypes.data, o.oov.ctypes.data if want_oov else None, ix, da, cap, C.byref(nnz),
                                                    C.byref(n_tok), flags, None)
    return rc, nnz.value, n_tok.value, o


def _compare(what, o, n_tok_got, rows, want, dt, has_oov):
    indptr, indices, data = want[:3]
    n_str, nnz = len(rows), len(indices)
    assert n_tok_got == sum(map(len, rows)), (what, "token total", n_tok_got)
    assert o.indptr.dtype == dt and np.array_equal(o.indptr[:n_str + 1], indptr), (what, "indptr")
    assert (o.indptr[n_str + 1:] == -7).all(), (what, "guard words behind indptr")
    if not np.array_equal(o.indices[:nnz], indices) or not np.array_equal(o.data[:nnz], data):
        bad = np.nonzero((o.indices[:nnz] != indices) | (o.data[:nnz] != data))[0]
        k = int(bad[0])
        s = int(np.searchsorted(indptr, k, "right")) - 1
        raise AssertionError((what, "entry", k, "of", nnz, "row", s, "of", len(rows[s]), "tokens; entries wrong:", len(bad), "got",
                              (int(o.indices[k]), int(o.data[k])), "want", (int(indices[k]), int(data[k]))))
    assert (o.indices[nnz:] == POISON_32).all() and (o.data[nnz:] == POISON_32).all(), (what, "guard words behind the entries")
    if has_oov:
        assert np.array_equal(o.oov[:n_str], want[3]) and (o.oov[n_str:] == -7).all(), (what, "oov")
        assert int(data.astype(np.int64).sum()) + int(want[3].sum()) == n_tok_got, (what, "data + oov = tokens")
    else:
        assert (o.oov == -7).all()


def check_vocab(lib, blobs, words, ids=None, what="", seed=0, dtypes=(np.int64, np.int32)):
    """the whole definition of the vocabulary form for one batch; returns (rows, want)"""
    from latok_amd import _lib, batch
    u8, boff = batch.pack_utf8(blobs)
    rows = _rows_of_slices(u8, boff)
    want = want_vocab(rows, _dict(words, ids))
    with batch.Vocab(words, ids=ids, seed=seed) as vocab:
        for dt in dtypes:
            rc, nnz, n_tok, o = _call(lib, u8, boff, vocab, cap=len(want[1]), dt=dt)
            assert rc == 0, (what, _lib.last_error())
            assert nnz == len(want[1]), (what, nnz, len(want[1]))
            assert lib.latok_debug_last_route() == TERMS_ROUTE or int(boff[-1]) == 0
            _compare((what, dt.__name__), o, n_tok, rows, want, dt, True)
    return rows, want


def check_hashed(lib, blobs, n_features, seed=0, alternate_sign=True, what="", dtypes=(np.int64,)):
    from latok_amd import _lib, batch
    u8, boff = batch.pack_utf8(blobs)
    rows = _rows_of_slices(u8, boff)
    want = want_hashed(rows, n_features, seed, alternate_sign)
    for dt in dtypes:
        rc, nnz, n_tok, o = _call(lib, u8, boff, hashed=(n_features, seed, alternate_sign), cap=len(want[1]), dt=dt)
        assert rc == 0, (what, _lib.last_error())
        assert nnz == len(want[1]), (what, nnz, len(want[1]))
        assert lib.latok_debug_last_route() == HASHED_ROUTE or int(boff[-1]) == 0
        _compare((what, n_features, alternate_sign, dt.__name__), o, n_tok, rows, want, dt, False)
    return rows, want


# ---- material: rows of lower-case words, one per token index -------------------------------------------------------------------
def _word(i):
    s = bytearray()
    i += 26                                  # at least two letters
    while i:
        s.append(97 + i % 26)
        i //= 26
    return bytes(s)


def _scrambled_id(i):
    """a distinct int32 per word, spread over the whole range and both signs: every radix digit takes part"""
    return _i32(((i + 1) * 2654435761) & 0xFFFFFFFF)


def _row(pattern, n, base=0):
    if pattern == "equal":
        return [base] * n
    if pattern == "distinct":
        return [base + j for j in range(n)][::-1]
    return [base + (j * 7 % 3 == 0) for j in range(n)]          # two values, interleaved


def _blob(tokens):
    return b" ".join(_word(t) for t in tokens)


def _vocabulary(n, oov_every=0):
    """words 0 .. n - 1 with scrambled ids; with oov_every, every oov_every-th index has no word"""
    idx = [i for i in range(n) if not (oov_every and i % oov_every == oov_every - 1)]
    return [_word(i) for i in idx], [_scrambled_id(i) for i in idx]


def _lengths():
    tile, row_max = limits()
    return [0, 1, 2, 63, 64, 65, row_max - 1, row_max, row_max + 1, 8 * row_max + 3]


# ---- 1. row lengths ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", ["equal", "distinct", "two"])
def test_row_lengths(gpu, pattern):
    tile, row_max = limits()
    lens = _lengths()
    blobs = [_blob(_row(pattern, n, base=3 * k)) for k, n in enumerate(lens)]
    words, ids = _vocabulary(max(lens) + 64, oov_every=5)
    rows, want = check_vocab(gpu, blobs, words, ids, ("lengths", pattern))
    assert [len(r) for r in rows] == lens
    long_row = len(lens) - 1
    got = want[1][want[0][long_row]:want[0][long_row + 1]].astype(np.int64)
    assert (np.diff(got) > 0).all() and (pattern != "distinct" or (got[0] < 0 < got[-1] and len(got) > 6 * row_max))   # signed order, both signs
    for n_features, alt in ((1 << 20, True), (64, True), (7, False)):
        check_hashed(gpu, blobs, n_features, 0, alt, ("lengths", pattern))


# ---- 2. tile edges -------------------------------------------------------------------------------------------------------------
def _short_rows(rng, n_rows, lo, hi, n_words):
    return [[rng.randrange(n_words) for _ in range(rng.randint(lo, hi))] for _ in range(n_rows)]


@pytest.mark.parametrize("where", ["first", "last", "between"])
def test_a_long_row_among_short_rows_and_runs_of_empty_strings(gpu, where):
    tile, row_max = limits()
    rng = random.Random(tile + len(where))
    n_words = 300
    long_row = [rng.randrange(n_words) for _ in range(8 * row_max + 3)]
    short = _short_rows(rng, 60, 1, 100, n_words)                    # ~3000 tokens: rows straddle the edges of three tiles
    rows = {"first": [long_row] + short, "last": short + [long_row], "between": short[:30] + [long_row] + short[30:]}[where]
    blobs = [_blob(r) for r in rows]
    mid = len(blobs) // 2
    blobs = [b""] * 200 + blobs[:mid] + [b""] * 200 + blobs[mid:] + [b""] * 200
    words, ids = _vocabulary(n_words, oov_every=7)
    got, want = check_vocab(gpu, blobs, words, ids, ("long row", where))
    assert sorted(len(r) for r in got)[-1] == 8 * row_max + 3 and sum(len(r) == 0 for r in got) == 600
    check_hashed(gpu, blobs, 1 << 20, 3, True, ("long row", where), dtypes=(np.int32,))
    check_hashed(gpu, blobs, 2, 0, True, ("long row", where))


def _run(i, n):
    """one lower-case token of n bytes, its own for every i"""
    return bytes(97 + (i + j * j) % 26 for j in range(n))


def test_every_path_of_the_token_walk(gpu):
    """Term keys on every path the token walk has: a token that ends in the word after its own (65 .. 128 bytes) and beyond it (more
    than 128), tokens the whole wave takes (more than kHashWaveBytes bytes: a word, absent, one byte off a word), a tile of two rounds
    (2048 tokens in 4096 bytes) and a string that began before the tile it is in."""
    T = wave_bytes()
    sizes = [70, 127, 129, 200, T - 1, T, T + 1, T + 3, 2 * T + 50, 3000]
    toks = [_run(i, n) for i, n in enumerate(sizes)]
    near = [t[:-1] + bytes([97 + (t[-1] - 96) % 26]) for t in toks]              # the last byte is another letter
    blobs = [b"a " * 2048, b" ".join(toks) + b" xy " + b" ".join(near), b"xy", toks[6] + b" " + toks[2], b""]
    assert len(blobs[0]) == 4096 and len(blobs[1]) > 2 * 4096 and not set(toks) & set(near)
    words = toks[::2] + near[1::2] + [b"a", b"xy"]
    rows, want = check_vocab(gpu, blobs, words, None, "token walk")
    assert [len(r) for r in rows] == [2048, 21, 1, 2, 0] and rows[1][:10] == toks and rows[1][11:] == near
    assert want[3].tolist() == [0, 10, 0, 0, 0] and np.diff(want[0]).tolist() == [1, 11, 1, 2, 0]
    check_hashed(gpu, blobs, 1 << 20, 5, True, "token walk", dtypes=(np.int32,))


def test_rows_that_start_exactly_on_a_tile_edge(gpu):
    tile, row_max = limits()
    rng = random.Random(2)
    n_words = 50
    # tokens before the row: exactly one tile, exactly two (with a row that straddles the first edge), then empty rows ON the edge
    lens = [tile - 10, 10, 7, tile - 7 - 3, 3, 0, 0, row_max, 0, 5, tile - 5 - 1, 1, row_max + 1, 0, 2]
    rows = [[rng.randrange(n_words) for _ in range(n)] for n in lens]
    words, ids = _vocabulary(n_words, oov_every=4)
    got, want = check_vocab(gpu, [_blob(r) for r in rows], words, ids, "rows on tile edges")
    starts = np.concatenate([[0], np.cumsum([len(r) for r in got])])
    assert [len(r) for r in got] == lens and sum(int(s) % tile == 0 for s in starts[:-1]) >= 6
    check_hashed(gpu, [_blob(r) for r in rows], 7, 1, True, "rows on tile edges")


def test_the_smallest_batches(gpu):
    words, ids = _vocabulary(4)
    for blobs in ([b""], [_word(1)], [b"zzzzzz"], [b"   "], [b"", b""], [_word(0) + b" " + _word(0)]):
        got, want = check_vocab(gpu, blobs, words, ids, ("smallest", blobs))
        check_hashed(gpu, blobs, 1 << 20, 0, True, ("smallest", blobs), dtypes=(np.int64, np.int32))
    from latok_amd import _lib, batch
    with batch.Vocab(words) as vocab:
        # n_str = 0: nnz = 0, indptr[0] cleared; total_bytes = 0 with strings: indptr and oov cleared
        rc, nnz, n_tok, o = _call(gpu, np.zeros(0, np.uint8), np.zeros(1, np.int64), vocab, cap=4)
        assert rc == 0 and nnz == 0 and n_tok == 0 and o.indptr[0] == 0 and (o.indptr[1:] == -7).all() and o.entries_untouched()
        rc, nnz, n_tok, o = _call(gpu, np.zeros(0, np.uint8), np.zeros(6, np.int64), vocab, cap=4, dt=np.int32)
        assert rc == 0 and nnz == 0 and not o.indptr[:6].any() and not o.oov[:5].any() and (o.indptr[6:] == -7).all() and o.entries_untouched()
        rc, nnz, n_tok, o = _call(gpu, np.zeros(0, np.uint8), np.zeros(6, np.int64), hashed=(8, 0, True), cap=0, want_entries=False)
        assert rc == 0 and nnz == 0 and not o.indptr[:6].any()


# ---- 3. key order and radix digits ---------------------------------------------------------------------------------------------
def test_explicit_ids_come_out_in_signed_order_in_short_and_long_rows(gpu):
    tile, row_max = limits()
    rng = random.Random(3)
    ids = EDGE_IDS + ONE_BYTE_APART + [-1, 7, 7]                       # an id twice over; -1 is an id like any other
    words = [_word(i) for i in range(len(ids))]
    unknown = [_word(1000 + i) for i in range(5)]
    short = [rng.choice(words + unknown) for _ in range(60)]
    long_row = [rng.choice(words + unknown) for _ in range(row_max + 5)]
    merged = [words[-1], words[-2], words[-1], unknown[0], words[-3], unknown[1]]            # 7, 7, 7, oov, -1, oov
    blobs = [b" ".join(short), b" ".join(long_row), b" ".join(merged), b" ".join(words), b" ".join(words[::-1] + unknown)]
    rows, (indptr, indices, data, oov) = check_vocab(gpu, blobs, words, ids, "explicit ids")
    assert indices[indptr[2]:indptr[3]].tolist() == [-1, 7] and data[indptr[2]:indptr[3]].tolist() == [1, 3] and oov[2] == 2
    want_ids = sorted(set(ids))
    assert indices[indptr[3]:indptr[4]].tolist() == want_ids == indices[indptr[4]:indptr[5]].tolist() and oov[4] == 5 and oov[3] == 0
    for s in (0, 1):
        row = indices[indptr[s]:indptr[s + 1]].astype(np.int64)
        assert (np.diff(row) > 0).all() and row[0] == INT32_MIN and row[-1] == INT32_MAX and oov[s] > 0


# ---- 4. out of vocabulary ------------------------------------------------------------------------------------------------------
def test_out_of_vocabulary_tokens(gpu):
    from latok_amd import _lib, batch
    tile, row_max = limits()
    rng = random.Random(4)
    words, ids = _vocabulary(40)
    known, unknown = list(range(40)), list(range(500, 540))
    rows = [[rng.choice(unknown) for _ in range(n)] for n in (1, 30, row_max + 2)]                       # all OOV: empty rows
    rows += [[rng.choice(known if j % 2 else unknown) for j in range(n)] for n in (2, 77, row_max + 9)]   # interleaved
    rows += [[], [rng.choice(known) for _ in range(50)]]
    blobs = [_blob(r) for r in rows]
    got, (indptr, indices, data, oov) = check_vocab(gpu, blobs, words, ids, "oov")
    assert (np.diff(indptr)[:3] == 0).all() and oov[:3].tolist() == [1, 30, row_max + 2] and oov[-1] == 0
    u8, boff = batch.pack_utf8(blobs)
    with batch.Vocab(words, ids=ids) as vocab:
        rc, nnz, n_tok, o = _call(gpu, u8, boff, vocab, cap=len(indices), want_oov=False)          # oov_out = NULL
        assert rc == 0, _lib.last_error()
        _compare("oov_out = NULL", o, n_tok, got, (indptr, indices, data), np.int64, False)
    got, (indptr, indices, data, oov) = check_vocab(gpu, blobs, [], None, "V = 0")
    assert len(indices) == 0 and not indptr.any() and oov.tolist() == [len(r) for r in rows]


# ---- 5. the hashed form --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _text_blobs():
    rng = random.Random(5)
    return [t.encode("utf-8", "surrogatepass") for t in random_strings(rng, 600, 0, 120, ALPHABETS["mixed"])] + [b"", b"a a a b", b"  "]


@pytest.mark.parametrize("alternate_sign", [True, False])
@pytest.mark.parametrize("n_features", [1, 2, 1 << 20, (1 << 31) - 1])
def test_hashed_columns(gpu, n_features, alternate_sign):
    blobs = _text_blobs()
    rows, (indptr, indices, data) = check_hashed(gpu, blobs, n_features, 0, alternate_sign, "text", dtypes=(np.int64, np.int32))
    check_hashed(gpu, blobs[:50], n_features, 0x9747B28C, alternate_sign, "text, another seed")
    if n_features == 1:
        assert np.diff(indptr).tolist() == [int(len(r) > 0) for r in rows]                  # one entry per non-empty row
        assert alternate_sign or data.tolist() == [len(r) for r in rows if r]
    if n_features == 2 and alternate_sign:
        assert (data == 0).sum() > 0                                                        # explicit zeros: kept
    if not alternate_sign:
        assert (data > 0).all()


def test_a_token_whose_hash_is_int32_min(gpu):
    from latok_amd import batch
    tok = mt.INT32_MIN_TOKEN
    assert murmur3_ref(tok, 0) == 0x80000000
    cases = [(7, True), (1 << 20, True), ((1 << 31) - 1, True), (3, False), (1, True)]
    batch.set_rules(*ONE_TOKEN_PER_STRING)
    try:
        for n_features, alt in cases:                                                        # alone: the string is the token
            rows, (indptr, indices, data) = check_hashed(gpu, [tok], n_features, 0, alt, "int32 min alone")
            assert rows == [[tok]] and indices.tolist() == [(1 << 31) % n_features] and data.tolist() == [-1 if alt else 1]
        rows, want = check_hashed(gpu, [b"ab", tok, b"", tok + b"x", tok], 7, 0, True, "int32 min, one token per string")
        assert rows[1] == rows[4] == [tok]
    finally:
        batch.reset_rules()
    row = b"some words " + tok + b" and " + tok + b" again , " + b" ".join(_word(i) for i in range(40))
    for n_features, alt in cases:                                                            # inside a row of ordinary tokens
        rows, (indptr, indices, data) = check_hashed(gpu, [b"first row", row, b"last"], n_features, 0, alt, "int32 min in a row")
        assert rows[1].count(tok) == 2 and (1 << 31) % n_features in indices[indptr[1]:indptr[2]].tolist()


# ---- 6. calls ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _protocol_batch():
    from latok_amd import batch
    tile, row_max = limits()
    rng = random.Random(9)
    blobs = [t.encode("utf-8", "surrogatepass") for t in random_strings(rng, 700, 0, 90, ALPHABETS["mixed"])]
    blobs.insert(300, _blob([rng.randrange(90) for _ in range(row_max + 40)]))               # one long row
    u8, boff = batch.pack_utf8(blobs)
    rows = _rows_of_slices(u8, boff)
    distinct = list(dict.fromkeys(t for r in rows for t in r))
    return u8, boff, rows, distinct[::2] + distinct[:6]


def test_capacity_protocol(gpu):
    from latok_amd import _lib, batch
    u8, boff, rows, words = _protocol_batch()
    for hashed in (None, (1 << 20, 0, True)):
        want = want_hashed(rows, *hashed) if hashed else want_vocab(rows, _dict(words))
        need = len(want[1])
        with batch.Vocab(words, seed=11) as vocab:
            # the size query: no entry buffers, capacity 0
            rc, nnz, n_tok, o = _call(gpu, u8, boff, vocab, hashed, cap=0, want_entries=False)
            assert rc == _lib.ERR_INVALID and nnz == need and n_tok == sum(map(len, rows))
            assert np.array_equal(o.indptr[:len(rows) + 1], want[0]) and (hashed or np.array_equal(o.oov[:len(rows)], want[3]))
            # one short: nothing written to indices or data, indptr and oov valid, the need returned
            rc, nnz, n_tok, o = _call(gpu, u8, boff, vocab, hashed, cap=need - 1, dt=np.int32)
            assert rc == _lib.ERR_INVALID and "capacity" in _lib.last_error() and nnz == need and o.entries_untouched()
            assert np.array_equal(o.indptr[:len(rows) + 1], want[0]) and (o.indptr[len(rows) + 1:] == -7).all()
            assert hashed or np.array_equal(o.oov[:len(rows)], want[3])
            # exact, with total_bytes = -1; larger than needed
            for cap in (need, need + 5, 1 << 40):
                rc, nnz, n_tok, o = _call(gpu, u8, boff, vocab, hashed, cap=min(cap, need + 5), total=-1)
                assert rc == 0 and nnz == need, _lib.last_error()
                _compare(("capacity", cap), o, n_tok, rows, want, np.int64, not hashed)
            # refused before any device work: one of the two buffers NULL, both NULL with a capacity, a stray flag bit
            n_str = len(rows)
            o = _Out(n_str, need, np.int64)
            nnz = C.c_int64(-1)
            for ix, da, cap, needle in ((o.indices.ctypes.data, None, need, "go together"), (None, o.data.ctypes.data, need, "go together"),
                                        (None, None, need, "cap > 0")):
                if hashed:
                    rc = gpu.latok_hashed_term_counts_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, n_str, -1, 0, 8, 1, o.indptr.ctypes.data,
                                                                       ix, da, cap, C.byref(nnz), None, 0, None)
                else:
                    rc = gpu.latok_term_counts_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, n_str, -1, vocab.handle, o.indptr.ctypes.data,
                                                                o.oov.ctypes.data, ix, da, cap, C.byref(nnz), None, 0, None)
                assert rc == _lib.ERR_INVALID and needle in _lib.last_error(), _lib.last_error()
                assert o.entries_untouched() and (o.indptr == -7).all() and (o.oov == -7).all()
            for flag in (4, 64, 1 << 30):
                rc, nnz2, n_tok, o = _call(gpu, u8, boff, vocab, hashed, cap=need, flags=flag)
                assert rc == _lib.ERR_INVALID and "unknown flag" in _lib.last_error() and o.entries_untouched() and (o.indptr == -7).all()
    for bad in (0, -1, 1 << 31, 1 << 40):
        rc, nnz, n_tok, o = _call(gpu, u8, boff, hashed=(bad, 0, True), cap=8)
        assert rc == _lib.ERR_INVALID and "n_features" in _lib.last_error() and o.entries_untouched() and (o.indptr == -7).all()
    rc, nnz, n_tok, o = _call(gpu, u8, boff, None, cap=8)
    assert rc == _lib.ERR_INVALID and "vocab" in _lib.last_error() and (o.indptr == -7).all()


def test_device_pointers_equal_host_pointers(gpu):
    from latok_amd import _lib, batch
    u8, boff, rows, words = _protocol_batch()
    n_str = len(rows)
    for hashed in (None, (64, 7, True)):
        want = want_hashed(rows, *hashed) if hashed else want_vocab(rows, _dict(words))
        need = len(want[1])
        sizes = (u8.nbytes + 256, boff.nbytes, (n_str + 1 + GUARD) * 4, (n_str + GUARD) * 4, (need + GUARD) * 4, (need + GUARD) * 4)
        ptrs = [gpu.latok_dev_alloc(s) for s in sizes]
        assert all(ptrs)
        try:
            d_u8, d_boff, d_indptr, d_oov, d_ix, d_da = ptrs
            _lib.check(gpu.latok_memset_dev(d_u8, 0xFF, sizes[0]))
            for p, s in zip(ptrs[2:], sizes[2:]):
                _lib.check(gpu.latok_memset_dev(p, POISON, s))
            _lib.check(gpu.latok_memcpy_h2d(d_u8, u8.ctypes.data, u8.nbytes))
            _lib.check(gpu.latok_memcpy_h2d(d_boff, boff.ctypes.data, boff.nbytes))
            _lib.check(gpu.latok_sync())
            nnz, n_tok = C.c_int64(-1), C.c_int64(-1)
            flags = _lib.DEVICE_PTRS | _lib.OUT_INT32
            with batch.Vocab(words) as vocab:
                if hashed:
                    rc = gpu.latok_hashed_term_counts_utf8_bytes_batch(d_u8, d_boff, n_str, -1, hashed[1], hashed[0], 1, d_indptr, d_ix, d_da, need,
                                                                       C.byref(nnz), C.byref(n_tok), flags, None)
                else:
                    rc = gpu.latok_term_counts_utf8_bytes_batch(d_u8, d_boff, n_str, -1, vocab.handle, d_indptr, d_oov, d_ix, d_da, need,
                                                                C.byref(nnz), C.byref(n_tok), flags, None)
                assert rc == 0 and nnz.value == need, _lib.last_error()
                assert gpu.latok_debug_last_route() == (HASHED_ROUTE if hashed else TERMS_ROUTE)
                o = _Out(n_str, need, np.int32)
                for a, p in ((o.indptr, d_indptr), (o.oov, d_oov), (o.indices, d_ix), (o.data, d_da)):
                    _lib.check(gpu.latok_memcpy_d2h(a.ctypes.data, p, a.nbytes))
                assert np.array_equal(o.indptr[:n_str + 1], want[0]) and (o.indptr[n_str + 1:].view(np.uint8) == POISON).all()
                assert np.array_equal(o.indices[:need], want[1]) and np.array_equal(o.data[:need], want[2])
                assert (o.indices[need:] == POISON_32).all() and (o.data[need:] == POISON_32).all()
                if hashed:
                    assert (o.oov.view(np.uint8) == POISON).all()
                else:
                    assert np.array_equal(o.oov[:n_str], want[3]) and (o.oov[n_str:].view(np.uint8) == POISON).all()
                    rc = gpu.latok_term_counts_utf8_bytes_batch(d_u8 + 4, d_boff, n_str, int(boff[-1]), vocab.handle, d_indptr, d_oov, d_ix, d_da,
                                                                need, C.byref(nnz), None, flags, None)
                    assert rc == _lib.ERR_INVALID and "16-byte aligned" in _lib.last_error()
        finally:
            for p in ptrs:
                gpu.latok_dev_free(p)


def test_a_vocabulary_serves_a_second_context_of_its_device(gpu):
    from latok_amd import _lib, batch
    u8, boff, rows, words = _protocol_batch()
    want = want_vocab(rows, _dict(words))
    with batch.Vocab(words, seed=5) as vocab:
        device = C.c_int(-1)
        _lib.check(gpu.latok_vocab_info(vocab.handle, None, None, None, C.byref(device)))
        first = batch.term_counts_utf8_csr(u8, boff, vocab)
        ctx = _lib.Context(device.value)
        try:
            with ctx:
                second = batch.term_counts_utf8_csr(u8, boff, vocab)
                hashed = batch.hashed_term_counts_utf8_csr(u8, boff, n_features=1 << 10)
        finally:
            ctx.destroy()
        for got in (first, second, batch.term_counts_utf8_csr(u8, boff, vocab)):
            assert all(np.array_equal(a, b) for a, b in zip(got, want))
        assert all(np.array_equal(a, b) for a, b in zip(hashed, want_hashed(rows, 1 << 10, 0, True)))


@pytest.mark.parametrize("table", sorted(ssc.TABLES))
def test_tables_that_leave_whitespace_inside_tokens(gpu, table):
    """interior whitespace is part of the word, only the two ends of a token are stripped"""
    from latok_amd import batch
    batch.set_rules(*ssc.TABLES[table])
    try:
        for i, texts in enumerate(ssc.content(table, ssc.SIZES[0], "bytes", "full")):
            blobs = [t.encode("utf-8", "surrogatepass") for t in texts]
            u8, boff = batch.pack_utf8(blobs)
            toks = [t for r in _rows_of_slices(u8, boff) for t in r]
            distinct = list(dict.fromkeys(toks))
            words = distinct[::2] + [t.strip() + b" " for t in toks[:50]]
            check_vocab(gpu, blobs, words, None, (table, "ABCD"[i]), seed=i, dtypes=(np.int64,))
            check_hashed(gpu, blobs, 64, i, True, (table, "ABCD"[i]))
    finally:
        batch.reset_rules()


def test_malformed_bytes_are_counted_as_they_are(gpu):
    rng = random.Random(5)
    body = [t.encode("utf-8", "surrogatepass") for t in random_strings(rng, 800, 0, 120, ALPHABETS["mixed"])]
    odd = [b"\xe6\x97", b"\xc3", b"\xf0\x9f\x98", b"end\xe6", b"\xf0", b"x\xc3", b"a\x80\x80\x80\x80b", b"\xe6\x97\xa5\xe6", b"\xa9"]
    words = odd + [b"ab", b"cd", b"lone", b"x", b"\xe6\x97\xa5"]
    check_vocab(gpu, body[:400] + SOFT + body[400:] + HARD + SOFT, words, None, "malformed")
    rows, (indptr, indices, data, oov) = check_vocab(gpu, SOFT + HARD, words, None, "small malformed batch")
    assert 0 in indices.tolist() and 1 in indices.tolist()                                   # nothing refused, nothing repaired
    check_hashed(gpu, SOFT + HARD + body[:100], 1 << 20, 0, True, "malformed")


def test_two_identical_calls_give_identical_bytes_and_the_neighbours_their_words(gpu):
    from latok_amd import batch
    u8, boff, rows, words = _protocol_batch()
    toks = [t for r in rows for t in r]
    with batch.Vocab(words, seed=5) as vocab:
        ids_before = batch.token_ids_utf8_csr(u8, boff, vocab, spans=True)
        assert gpu.latok_debug_last_route() == IDS_ROUTE
        hashes_before = batch.token_hashes_utf8_csr(u8, boff, seed=5, spans=True)
        assert gpu.latok_debug_last_route() == HASH_ROUTE
        a = batch.term_counts_utf8_csr(u8, boff, vocab)
        assert gpu.latok_debug_last_route() == TERMS_ROUTE
        b = batch.term_counts_utf8_csr(u8, boff, vocab)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
        h1 = batch.hashed_term_counts_utf8_csr(u8, boff, n_features=2, seed=5)
        assert gpu.latok_debug_last_route() == HASHED_ROUTE
        h2 = batch.hashed_term_counts_utf8_csr(u8, boff, n_features=2, seed=5)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(h1, h2))
        ids_after = batch.token_ids_utf8_csr(u8, boff, vocab, spans=True)
        assert gpu.latok_debug_last_route() == IDS_ROUTE
        hashes_after = batch.token_hashes_utf8_csr(u8, boff, seed=5, spans=True)
        assert gpu.latok_debug_last_route() == HASH_ROUTE
    assert all(np.array_equal(x, y) for x, y in zip(ids_before, ids_after))
    assert all(np.array_equal(x, y) for x, y in zip(hashes_before, hashes_after))
    d = _dict(words)
    assert ids_before[1].tolist() == [d.get(t, -1) for t in toks] and hashes_before[1].tolist() == [murmur3_ref(t, 5) for t in toks]


# ---- 7. wrappers and the example -------------------------------------------------------------------------------------------------
def test_python_wrappers(gpu, oracle):
    from latok_amd import batch
    rng = random.Random(3)
    texts = [t for t in random_strings(rng, 400, 0, 80, ALPHABETS["mixed"]) + ["", "   ", "x", "a,b a,b"] if "\ud800" not in t]
    tokens = [oracle.tokenize(text) if text != "" else [] for text in texts]
    distinct = list(dict.fromkeys(t for row in tokens for t in row))
    words = distinct[::2] + [","]
    d = _dict([w.encode() for w in words])
    rows = [[t.encode() for t in row] for row in tokens]
    want = want_vocab(rows, d)
    with batch.Vocab(words) as vocab:
        got = batch.term_counts_batch(texts, vocab)
        assert [g.dtype for g in got] == [np.int64, np.int32, np.int32, np.int64] and all(np.array_equal(a, b) for a, b in zip(got, want))
        blobs = [t.encode() for t in texts]
        got = batch.term_counts_utf8_batch(blobs, vocab)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        u8, boff = batch.pack_utf8(blobs)
        got32 = batch.term_counts_utf8_csr(u8, boff, vocab, dtype=np.int32)
        assert got32[0].dtype == got32[3].dtype == np.int32 and all(np.array_equal(a, b) for a, b in zip(got32, want))
        empty = batch.term_counts_utf8_batch([], vocab)
        assert empty[0].tolist() == [0] and len(empty[1]) == len(empty[2]) == len(empty[3]) == 0
    with pytest.raises(ValueError):
        batch.term_counts_batch(texts, vocab)                     # closed
    for n_features, alt in ((1 << 20, True), (2, True), (5, False)):
        wanth = want_hashed(rows, n_features, 0, alt)
        got = batch.hashed_term_counts_batch(texts, n_features=n_features, alternate_sign=alt)
        assert len(got) == 3 and all(np.array_equal(a, b) for a, b in zip(got, wanth))
    got = batch.hashed_term_counts_utf8_csr(u8, boff, n_features=64, seed=9, dtype=np.int32)
    assert got[0].dtype == np.int32 and all(np.array_equal(a, b) for a, b in zip(got, want_hashed(rows, 64, 9, True)))
    sparse = pytest.importorskip("scipy.sparse")
    indptr, indices, data, oov = want
    with batch.Vocab(words) as vocab:
        indptr, indices, data, oov = batch.term_counts_batch(texts, vocab)
    m = sparse.csr_matrix((data, indices, indptr), shape=(len(texts), len(words)))
    assert m.has_canonical_format and m.has_sorted_indices
    built = sparse.lil_matrix((len(texts), len(words)), dtype=np.int32)
    for s, row in enumerate(rows):
        for k, v in Counter(d[t] for t in row if t in d).items():
            built[s, k] = v
    assert (m != built.tocsr()).nnz == 0
    indptr, indices, data = batch.hashed_term_counts_batch(texts, n_features=2)
    h = sparse.csr_matrix((data, indices, indptr), shape=(len(texts), 2))
    assert h.has_canonical_format and h.nnz == len(data) and (data == 0).any()              # explicit zeros stay entries
    assert np.array_equal(h.toarray(), sparse.csr_matrix(want_hashed(rows, 2, 0, True)[::-1], shape=(len(texts), 2)).toarray())


def test_c_example(gpu, tmp_path):
    exe = str(tmp_path / "term_counts_utf8")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "term_counts_utf8.c"),
                           "-L" + os.path.join(ROOT, "latok_amd"), "-llatok_hip", "-Wl,-rpath," + os.path.join(ROOT, "latok_amd"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0] == "19 tokens, 12 entries" and lines[1].startswith("vocabulary ids")
    assert lines[2] == "  row 0: 0:1 1:1 2:1 3:1 4:1 5:2 6:2 7:1 8:1   (oov 1)"
    assert lines[3] == "  row 1: 1:1   (oov 2)" and lines[4] == "  row 2:   (oov 0)" and lines[5] == "  row 3:   (oov 0)"
    assert lines[6] == "  row 4: 2:2 9:1   (oov 1)"
    toks = [[b"This", b"is", b"a", b"#test", b"!", b"Testing", b",", b"Testing", b",", b"1", b"2", b"3"], [b"this", b"is", b"not"], [], [],
            [b"a", "日本語".encode(), b"a", "🤓".encode()]]
    indptr, indices, data = want_hashed(toks, 16, 0, True)
    for s in range(5):
        want = "  row %d:" % s + "".join(" %d:%d" % (indices[k], data[k]) for k in range(indptr[s], indptr[s + 1]))
        assert lines[8 + s] == want, (s, lines[8 + s], want)
