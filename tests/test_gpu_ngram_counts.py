"""Word n-grams in the term counts on the device (latok_ngram_counts_utf8_bytes_batch, latok_hashed_ngram_counts_utf8_bytes_batch,
include/latok_hip.h).

The result is DEFINED by a call the parity tests already pin and by Python's own containers: the byte slices
latok_token_spans_utf8_bytes_batch reports for string s, joined in Python -- sep.join(row[i:i + n]) for every n in [min_n, max_n] and
every i -- and fed to a dict (vocabulary form) or to tests/helpers/murmur3_ref.py (hashed form), exactly as test_gpu_term_counts.py
feeds the tokens themselves.  Every batch goes through the C ABI with poisoned guard bands round every output and is checked in
full against that definition.  The shapes are the smallest at which the kernels can go wrong, with the workgroup size in tokens and
the highest order read from latok_debug_ngram_limits and the longest short row of the reduce from latok_debug_terms_limits."""
import ctypes as C
import functools
import os
import random
import subprocess

import numpy as np
import pytest

import test_gpu_term_counts as tc
from conftest import ALPHABETS, ROOT, random_strings
from helpers import murmur3_collide as mc
from helpers import span_strip_content as ssc
from helpers.murmur3_ref import murmur3_ref

pytestmark = pytest.mark.gpu

NGRAM_ROUTE, HASHED_NGRAM_ROUTE = 14, 15
POISON_32, GUARD = tc.POISON_32, tc.GUARD


@functools.lru_cache(maxsize=1)
def ng_limits():
    """(kNgBlock, kNgMax) from latok_debug_ngram_limits"""
    from latok_amd import _lib
    fn = _lib.load().latok_debug_ngram_limits
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    out = np.zeros(4, np.int64)
    assert fn(out.ctypes.data, 4) == 2
    block, ng_max = int(out[0]), int(out[1])
    assert 64 <= block <= 1024 and 2 <= ng_max <= 16
    return block, ng_max


def ranges():
    block, ng_max = ng_limits()
    return [(1, 1), (1, 2), (2, 2), (1, 3), (2, ng_max), (ng_max, ng_max)]


# ---- the definition --------------------------------------------------------------------------------------------------------
def grams(row, min_n, max_n, sep):
    s = bytes([sep])
    return [s.join(row[i:i + n]) for n in range(min_n, max_n + 1) for i in range(len(row) - n + 1)]


def gram_rows(rows, min_n, max_n, sep):
    return [grams(r, min_n, max_n, sep) for r in rows]


def n_grams_of(c, min_n, max_n):
    return sum(max(0, c - n + 1) for n in range(min_n, max_n + 1))


# ---- the calls, with guard bands ---------------------------------------------------------------------------------------------
def _call(lib, u8, boff, ng, vocab=None, hashed=None, cap=0, dt=np.int64, want_oov=True, want_entries=True, total=None, flags=0):
    """one blocking call with host pointers -> (rc, nnz, n_grams, _Out); ng = (min_n, max_n, sep), hashed = (n_features, seed, alternate_sign)"""
    from latok_amd import _lib
    n_str = boff.size - 1
    total = (int(boff[-1]) if n_str > 0 else 0) if total is None else total
    o = tc._Out(n_str, cap, dt)
    nnz, n_g = C.c_int64(-1), C.c_int64(-1)
    flags |= _lib.OUT_INT32 if dt == np.int32 else 0
    ix, da = (o.indices.ctypes.data, o.data.ctypes.data) if want_entries else (None, None)
    if hashed is not None:
        n_features, seed, alt = hashed
        rc = lib.latok_hashed_ngram_counts_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, n_str, total, seed, n_features, int(alt), ng[0], ng[1],
                                                            ng[2], o.indptr.ctypes.data, ix, da, cap, C.byref(nnz), C.byref(n_g), flags, None)
    else:
        rc = lib.latok_ngram_counts_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, n_str, total, vocab.handle if vocab is not None else None,
                                                     ng[0], ng[1], ng[2], o.indptr.ctypes.data, o.oov.ctypes.data if want_oov else None, ix, da,
                                                     cap, C.byref(nnz), C.byref(n_g), flags, None)
    return rc, nnz.value, n_g.value, o


def check_vocab(lib, blobs, ng, words, ids=None, what="", seed=0, dtypes=(np.int64, np.int32), rows=None):
    """the whole definition of the vocabulary form for one batch and one range; returns (token rows, want)"""
    from latok_amd import _lib, batch
    u8, boff = batch.pack_utf8(blobs)
    rows = tc._rows_of_slices(u8, boff) if rows is None else rows
    g = gram_rows(rows, *ng)
    want = tc.want_vocab(g, tc._dict(words, ids))
    with batch.Vocab(words, ids=ids, seed=seed) as vocab:
        for dt in dtypes:
            rc, nnz, n_g, o = _call(lib, u8, boff, ng, vocab, cap=len(want[1]), dt=dt)
            assert rc == 0, (what, ng, _lib.last_error())
            assert nnz == len(want[1]), (what, ng, nnz, len(want[1]))
            assert lib.latok_debug_last_route() == NGRAM_ROUTE or int(boff[-1]) == 0
            tc._compare((what, ng, dt.__name__), o, n_g, g, want, dt, True)
    return rows, want


def check_hashed(lib, blobs, ng, n_features, seed=0, alternate_sign=True, what="", dtypes=(np.int64,), rows=None):
    from latok_amd import _lib, batch
    u8, boff = batch.pack_utf8(blobs)
    rows = tc._rows_of_slices(u8, boff) if rows is None else rows
    g = gram_rows(rows, *ng)
    want = tc.want_hashed(g, n_features, seed, alternate_sign)
    for dt in dtypes:
        rc, nnz, n_g, o = _call(lib, u8, boff, ng, hashed=(n_features, seed, alternate_sign), cap=len(want[1]), dt=dt)
        assert rc == 0, (what, ng, _lib.last_error())
        assert nnz == len(want[1]), (what, ng, nnz, len(want[1]))
        assert lib.latok_debug_last_route() == HASHED_NGRAM_ROUTE or int(boff[-1]) == 0
        tc._compare((what, ng, n_features, alternate_sign, dt.__name__), o, n_g, g, want, dt, False)
    return rows, want


def _some_grams(rows, ng, every=2):
    """a vocabulary for a batch: every `every`-th distinct gram, a few of them twice"""
    distinct = list(dict.fromkeys(g for r in rows for g in grams(r, *ng)))
    return distinct[::every] + distinct[:6]


# ---- 1. ranges, and equality with the existing calls ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _alphabet_batch(name):
    from latok_amd import batch
    rng = random.Random(len(name))
    blobs = [t.encode("utf-8", "surrogatepass") for t in random_strings(rng, 160, 0, 70, ALPHABETS[name])] + [b"", b"a a a b a a", b"  "]
    u8, boff = batch.pack_utf8(blobs)
    return blobs, u8, boff, tc._rows_of_slices(u8, boff)


@pytest.mark.parametrize("alphabet", sorted(ALPHABETS))
def test_ranges_over_random_strings(gpu, alphabet):
    blobs, u8, boff, rows = _alphabet_batch(alphabet)
    for k, (lo, hi) in enumerate(ranges()):
        ng = (lo, hi, 0x20)
        check_vocab(gpu, blobs, ng, _some_grams(rows, ng), None, alphabet, seed=k, dtypes=(np.int64,), rows=rows)
        check_hashed(gpu, blobs, ng, 1 << 20 if k % 2 else 64, k, True, alphabet, rows=rows)


@pytest.mark.parametrize("alphabet", ["mixed", "words"])
def test_range_1_1_equals_the_existing_calls_array_for_array(gpu, alphabet):
    from latok_amd import _lib, batch
    blobs, u8, boff, rows = _alphabet_batch(alphabet)
    words = _some_grams(rows, (1, 1, 0x20))
    ids = [tc._scrambled_id(i) for i in range(len(words))]
    with batch.Vocab(words, ids=ids, seed=3) as vocab:
        for dt in (np.int64, np.int32):
            rc, nnz, n_tok, old = tc._call(gpu, u8, boff, vocab, cap=len(u8), dt=dt)
            assert rc == 0 and gpu.latok_debug_last_route() == tc.TERMS_ROUTE
            for sep in (0x20, 0x00):                                                   # no separator is ever used
                rc, nnz2, n_g, new = _call(gpu, u8, boff, (1, 1, sep), vocab, cap=len(u8), dt=dt)
                assert rc == 0 and gpu.latok_debug_last_route() == NGRAM_ROUTE and (nnz2, n_g) == (nnz, n_tok), _lib.last_error()
                for a, b in ((old.indptr, new.indptr), (old.oov, new.oov), (old.indices, new.indices), (old.data, new.data)):
                    assert a.tobytes() == b.tobytes()
    for hashed in ((1 << 20, 0, True), (7, 9, False)):
        rc, nnz, n_tok, old = tc._call(gpu, u8, boff, hashed=hashed, cap=len(u8))
        assert rc == 0 and gpu.latok_debug_last_route() == tc.HASHED_ROUTE
        rc, nnz2, n_g, new = _call(gpu, u8, boff, (1, 1, 0x20), hashed=hashed, cap=len(u8))
        assert rc == 0 and gpu.latok_debug_last_route() == HASHED_NGRAM_ROUTE and (nnz2, n_g) == (nnz, n_tok)
        for a, b in ((old.indptr, new.indptr), (old.oov, new.oov), (old.indices, new.indices), (old.data, new.data)):
            assert a.tobytes() == b.tobytes()


# ---- 2. strings with few tokens ------------------------------------------------------------------------------------------------
def test_strings_with_few_tokens_and_runs_of_empty_strings_across_a_workgroup_edge(gpu):
    block, ng_max = ng_limits()
    counts = sorted({0, 1, 2, 3, 4, ng_max - 1, ng_max, ng_max + 1})
    blobs = []
    for rep in range(3):
        for c in counts:
            blobs.append(tc._blob([(7 * c + j + rep) % 11 for j in range(c)]))
        blobs += [b" ", b"   \t  ", b"\n"]
    # tokens up to a workgroup's last one, then a run of empty and whitespace-only strings ON the edge, then the next workgroup's rows
    have = sum(len(b.split()) for b in blobs)
    fill = (-have) % block
    blobs += [tc._blob([j % 5 for j in range(fill)])] + [b"", b"  ", b""] * 100 + [tc._blob([1, 2, 3, 1, 2, 3])] + [b""] * 70 + [tc._blob([4])]
    for lo, hi in ranges():
        ng = (lo, hi, 0x20)
        rows, want = check_hashed(gpu, blobs, ng, 1 << 20, 0, True, "few tokens")
        starts = np.cumsum([0] + [len(r) for r in rows])
        assert block in starts.tolist() and sum(len(r) == 0 for r in rows) >= 380
        for r, a, b in zip(rows, want[0][:-1], want[0][1:]):
            assert len(r) >= lo or a == b                                              # fewer than min_n tokens: an empty row
        check_vocab(gpu, blobs, ng, _some_grams(rows, ng), None, "few tokens", dtypes=(np.int64,), rows=rows)
    # a whole batch with tokens and no key (K == 0): no key launch and no reduce, the rows are still delivered -- all empty
    blobs, ng = [b"a b", b"c", b""], (3, 3, 0x20)
    for check in (lambda: check_hashed(gpu, blobs, ng, 1 << 20, 0, True, "tokens, no key", dtypes=(np.int64, np.int32)),
                  lambda: check_vocab(gpu, blobs, ng, [b"a b c", b"a"], None, "tokens, no key")):
        rows, want = check()                                                           # (rc == 0, n_grams == 0 and the guard bands: _compare)
        assert [len(r) for r in rows] == [2, 1, 0] and len(want[1]) == 0 and not want[0].any() and all(not w.any() for w in want[3:])


# ---- 3. bigram shapes ----------------------------------------------------------------------------------------------------------
def test_the_bigram_grid_of_token_lengths_at_every_alignment(gpu):
    rng = random.Random(8)
    letters = b"abcdefghijklmnopqrstuvwxyz"
    word = lambda n: bytes(rng.choice(letters) for _ in range(n))
    blobs = [b" " * pad + word(la) + b" " + word(lb) for la in range(1, 9) for lb in range(1, 9) for pad in range(4)]
    blobs = [b + b" " * (-len(b) % 4) for b in blobs]                                  # every string starts on a dword: the pad is the alignment
    from latok_amd import batch
    u8, boff = batch.pack_utf8(blobs)
    rows = tc._rows_of_slices(u8, boff)
    assert len(rows) == 256 and all(len(r) == 2 for r in rows)
    seen = {(len(r[0]), len(r[1]), (int(boff[s]) + blobs[s].index(r[0])) % 4) for s, r in enumerate(rows)}
    assert len(seen) == 8 * 8 * 4                                                      # every pair of lengths at every start alignment
    for ng in ((2, 2, 0x20), (1, 2, 0x20), (2, 2, 0x00), (2, 2, 0xFF)):
        check_hashed(gpu, blobs, ng, (1 << 31) - 1, 5, True, "bigram grid", rows=rows)
        check_vocab(gpu, blobs, ng, _some_grams(rows, ng), None, "bigram grid", seed=5, dtypes=(np.int64,), rows=rows)


def test_adjacent_tokens_long_whitespace_and_a_long_token_inside_a_gram(gpu):
    from latok_amd import batch
    wave = tc_hash_wave_bytes()
    long_tok = b"x" * (wave + 44)
    blobs = [b"a,b", b"a,b a,b", b"x.y,z", b"a" + b" " * 300 + b"b", b"a \t\n  b" + b" " * 4100 + b"c d",
             b"in " + long_tok + b" out", long_tok + b" " + long_tok[:-1] + b" y", b"q " + b"y" * (3 * wave + 1)]
    u8, boff = batch.pack_utf8(blobs)
    rows = tc._rows_of_slices(u8, boff)
    assert rows[0] == [b"a", b",", b"b"] and rows[3] == [b"a", b"b"] and rows[5] == [b"in", long_tok, b"out"]
    for lo, hi in ((1, 2), (2, 2), (1, 3), (2, 3)):
        ng = (lo, hi, 0x20)
        check_hashed(gpu, blobs, ng, 1 << 20, 1, True, "shapes", rows=rows)
        words = _some_grams(rows, ng, every=1)
        got, (indptr, indices, data, oov) = check_vocab(gpu, blobs, ng, words, None, "shapes", rows=rows)
        assert not oov.any()
        check_vocab(gpu, blobs, ng, words[::2], None, "shapes, half known", dtypes=(np.int64,), rows=rows)
    got, (indptr, indices, data, oov) = check_vocab(gpu, blobs[:2], (2, 2, 0x20), [b"a ,", b", b", b"b a", b"a,b", b"a, b"], None, "a,b")
    assert indices.tolist() == [0, 1, 0, 1, 2] and data.tolist() == [1, 1, 2, 2, 1] and not oov.any()


def tc_hash_wave_bytes():
    """entry 14 of latok_debug_limits: kHashWaveBytes"""
    from latok_amd import _lib
    fn = _lib.load().latok_debug_limits
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    out = np.zeros(15, np.int64)
    assert fn(out.ctypes.data, 15) == 15
    return int(out[14])


# ---- 4. token-space edges ------------------------------------------------------------------------------------------------------
def test_rows_at_the_edges_of_a_workgroup_of_tokens(gpu):
    block, ng_max = ng_limits()
    rng = random.Random(block)
    # a row that ends exactly at a workgroup's last token and one that starts there; grams whose tokens lie in two workgroups (rows that
    # straddle an edge by 1 .. ng_max tokens on either side); a row longer than a workgroup
    lens = [block - 5, 5, 7, block - 7 - 3, 3 + 4, block - 4 - 1, 1 + 1, block - 1 - ng_max, 2 * ng_max, block - ng_max, 2 * block + 3, block - 3, 2]
    rows = [[rng.randrange(6) for _ in range(n)] for n in lens]
    blobs = [tc._blob(r) for r in rows]
    for lo, hi in ranges():
        ng = (lo, hi, 0x20)
        got, want = check_hashed(gpu, blobs, ng, 1 << 20, 0, True, "workgroup edges")
        starts = np.cumsum([0] + [len(r) for r in got]).tolist()
        assert [len(r) for r in got] == lens and block in starts and sum(s % block == 0 for s in starts[1:]) >= 3
        check_vocab(gpu, blobs, ng, _some_grams(got, ng), None, "workgroup edges", dtypes=(np.int64,), rows=got)


# ---- 5. key-space edges --------------------------------------------------------------------------------------------------------
def _short_row_for(n_keys, row_max, ng_max):
    """(min_n, max_n, c): a range and a token count c <= row_max -- a SHORT row of the existing call -- with exactly n_keys grams;
    None if no range has one"""
    for lo in range(1, ng_max + 1):
        for hi in range(lo + 1, ng_max + 1):
            m, const = hi - lo + 1, sum(n - 1 for n in range(lo, hi + 1))
            if (n_keys + const) % m == 0:
                c = (n_keys + const) // m
                if hi <= c <= row_max and n_grams_of(c, lo, hi) == n_keys:
                    return lo, hi, c
    return None


def _key_edge_cases():
    tile, row_max = tc.limits()
    block, ng_max = ng_limits()
    cases = []
    for n_keys in (row_max - 1, row_max, row_max + 1, 2 * row_max + 1):
        found = _short_row_for(n_keys, row_max, ng_max)
        if found is None:
            # m orders give m * c - (a constant) keys; with row_max a power of two no range of two or more orders meets it at a token
            # count <= row_max (m = 2, 4, 8 leave an odd or 2-mod-4 remainder; 3, 5, 6, 7 do not divide it).  The order-2 row of
            # row_max + 1 tokens has exactly that many keys: one token longer than a short row of the existing call.
            found = (2, 2, n_keys + 1)
        cases.append((n_keys,) + found)
    return cases


def test_rows_short_in_tokens_and_long_in_keys(gpu):
    tile, row_max = tc.limits()
    cases = _key_edge_cases()
    assert [c[0] for c in cases] == [row_max - 1, row_max, row_max + 1, 2 * row_max + 1]
    assert sum(c[3] <= row_max for c in cases) >= 3                                   # short for the existing call, at or over the edge here
    rng = random.Random(7)
    for n_keys, lo, hi, c in cases:
        ng = (lo, hi, 0x20)
        row = [rng.randrange(12) for _ in range(c)]
        around = [tc._blob([rng.randrange(12) for _ in range(n)]) for n in (3, 40, 0, 9)]
        for blobs, what in (([tc._blob(row)], "one row"), (around[:2] + [tc._blob(row)] + around[2:], "among short rows")):
            got, want = check_hashed(gpu, blobs, ng, 1 << 20, 0, True, (what, n_keys))
            assert max(np.diff(np.cumsum([0] + [n_grams_of(len(r), lo, hi) for r in got]))) == n_keys
            words = _some_grams(got, ng)
            check_vocab(gpu, blobs, ng, words, [tc._scrambled_id(i) for i in range(len(words))], (what, n_keys), dtypes=(np.int64,), rows=got)


# ---- 6. the vocabulary form ----------------------------------------------------------------------------------------------------
def _colliding_bigrams(seed, want=3):
    """pairs (a, b) of distinct bigrams "w1 w2" of lower-case words, equally long, with one hash: block 1 of a gets one byte changed
    and block 2 is solved (murmur3_collide); kept if every byte of the second word is still a lower-case letter"""
    rng = random.Random(seed + 17)
    low = range(0x61, 0x7B)
    pairs = []
    for _ in range(4000):
        a = bytes(rng.choice(low) for _ in range(3)) + b" " + bytes(rng.choice(low) for _ in range(rng.choice((9, 10, 11, 13))))
        h_before = mc._state(a, seed, 1)
        h_a = mc.mix_h(h_before, mc.mix_k(int.from_bytes(a[4:8], "little")))
        mk_next = mc.mix_k(int.from_bytes(a[8:12], "little"))
        for pos in range(4):
            for new in low:
                if new == a[4 + pos]:
                    continue
                blk = bytearray(a[4:8])
                blk[pos] = new
                h_b = mc.mix_h(h_before, mc.mix_k(int.from_bytes(blk, "little")))
                nxt = mc.unmix_k(mk_next ^ h_a ^ h_b).to_bytes(4, "little")
                if all(x in low for x in nxt):
                    pairs.append((a, a[:4] + bytes(blk) + nxt + a[12:]))
        if len(pairs) >= want:
            break
    assert len(pairs) >= want
    assert all(a != b and len(a) == len(b) and murmur3_ref(a, seed) == murmur3_ref(b, seed) for a, b in pairs)
    return pairs[:want]


@pytest.mark.parametrize("seed", [0, 0x9747B28C])
def test_grams_that_collide_in_hash_and_length_are_told_apart_by_their_bytes(gpu, seed):
    pairs = _colliding_bigrams(seed)
    blobs = [a for a, _ in pairs] + [b for _, b in pairs] + [b"lead " + a + b" then " + b + b" end" for a, b in pairs]
    ng = (1, 2, 0x20)
    only_a = [a for a, _ in pairs]
    rows, (indptr, indices, data, oov) = check_vocab(gpu, blobs, ng, only_a, None, "collisions, a known", seed=seed)
    n = len(pairs)
    assert all(len(r) == 2 for r in rows[:2 * n]) and [b" ".join(r) for r in rows[:2 * n]] == blobs[:2 * n]
    assert np.diff(indptr)[:2 * n].tolist() == [1] * n + [0] * n and oov[:2 * n].tolist() == [2] * n + [3] * n     # every b is unknown
    both = [w for p in pairs for w in p]
    rows, (indptr, indices, data, oov) = check_vocab(gpu, blobs, ng, both, None, "collisions, both known", seed=seed, rows=rows)
    assert indices[:2 * n].tolist() == [2 * k for k in range(n)] + [2 * k + 1 for k in range(n)]                    # each its own id
    check_vocab(gpu, blobs, ng, both[::-1], list(range(100, 100 + len(both))), "collisions, reversed", seed=seed, dtypes=(np.int64,), rows=rows)


def test_vocabulary_words_with_separators_edge_ids_duplicate_ids_and_no_words(gpu):
    rng = random.Random(6)
    cities = [b"new york", b"new york city", b"york city", b"los angeles", b"new", b"york", b"san francisco bay area"]
    text = [b"i love new york city and los angeles", b"new york new york", b"york new", b"the san francisco bay area , new york",
            b"", b"newyork new_york new  york", b"city"]
    ng = (1, 4, 0x20)
    rows, (indptr, indices, data, oov) = check_vocab(gpu, text, ng, cities, None, "cities")
    assert indices[indptr[1]:indptr[2]].tolist() == [0, 4, 5] and data[indptr[1]:indptr[2]].tolist() == [2, 2, 2]
    assert indices[indptr[5]:indptr[6]].tolist() == [0, 4, 5]                         # "new  york": two tokens, one gram "new york"
    assert indices[indptr[3]:indptr[4]].tolist() == [0, 4, 5, 6] and oov[6] == 1 and oov[4] == 0
    # ids at the edges of int32 and ids that occur twice: grams of different orders count into one entry
    ids = tc.EDGE_IDS[:len(cities) - 2] + [7, 7]
    rows, (indptr, indices, data, oov) = check_vocab(gpu, text, ng, cities, ids, "edge ids", rows=rows)
    assert (np.diff(indices[indptr[0]:indptr[1]].astype(np.int64)) > 0).all() and tc.INT32_MIN in indices.tolist()
    body = [tc._blob([rng.randrange(9) for _ in range(rng.randrange(0, 30))]) for _ in range(120)]
    for lo, hi in ranges():
        got, (indptr, indices, data, oov) = check_vocab(gpu, body, (lo, hi, 0x20), [], None, "V = 0", dtypes=(np.int64,))
        assert len(indices) == 0 and not indptr.any() and oov.tolist() == [n_grams_of(len(r), lo, hi) for r in got]
    # a vocabulary whose grams use another separator: every gram of two or more tokens is out of vocabulary, row by row
    got, _ = check_vocab(gpu, body, (2, 3, 0x5F), [], None, "rows", dtypes=(np.int64,))
    words = _some_grams(got, (2, 3, 0x5F), every=1)
    got, (indptr, indices, data, oov) = check_vocab(gpu, body, (2, 3, 0x5F), words, None, "the vocabulary's separator", rows=got)
    assert not oov.any() and len(indices) > 100
    got, (indptr, indices, data, oov) = check_vocab(gpu, body, (2, 3, 0x20), words, None, "another separator", rows=got)
    assert len(indices) == 0 and oov.tolist() == [n_grams_of(len(r), 2, 3) for r in got]


# ---- 7. mixed-form checks ------------------------------------------------------------------------------------------------------
def test_malformed_bytes_are_joined_as_they_are(gpu):
    rng = random.Random(5)
    body = [t.encode("utf-8", "surrogatepass") for t in random_strings(rng, 150, 0, 90, ALPHABETS["mixed"])]
    blobs = body[:80] + tc.SOFT + body[80:] + tc.HARD + tc.SOFT
    for ng in ((1, 2, 0x20), (2, 3, 0xFF)):
        rows, _ = check_hashed(gpu, blobs, ng, 1 << 20, 0, True, "malformed")
        check_vocab(gpu, blobs, ng, _some_grams(rows, ng), None, "malformed", dtypes=(np.int64,), rows=rows)
    rows, _ = check_hashed(gpu, tc.SOFT + tc.HARD, (1, 3, 0x20), 64, 0, True, "small malformed batch")
    check_vocab(gpu, tc.SOFT + tc.HARD, (1, 3, 0x20), _some_grams(rows, (1, 3, 0x20), every=1), None, "small malformed batch", rows=rows)


@pytest.mark.parametrize("table", sorted(ssc.TABLES))
def test_tables_that_leave_whitespace_inside_tokens(gpu, table):
    """interior whitespace is part of the token, so a gram may hold the separator's byte inside a token as well as between two"""
    from latok_amd import batch
    batch.set_rules(*ssc.TABLES[table])
    try:
        texts = ssc.content(table, ssc.SIZES[0], "bytes", "full")[0]
        blobs = [t.encode("utf-8", "surrogatepass") for t in texts]
        for ng in ((1, 2, 0x20), (2, 3, 0x00)):
            rows, _ = check_hashed(gpu, blobs, ng, 64, 1, True, table)
            check_vocab(gpu, blobs, ng, _some_grams(rows, ng), None, table, dtypes=(np.int64,), rows=rows)
    finally:
        batch.reset_rules()


@pytest.mark.parametrize("sep", [0x00, 0x20, 0xFF])
def test_separator_bytes(gpu, sep):
    blobs, u8, boff, rows = _alphabet_batch("words")
    for lo, hi in ((1, 2), (2, 3)):
        ng = (lo, hi, sep)
        check_hashed(gpu, blobs, ng, 1 << 20, 0, True, "sep", dtypes=(np.int64, np.int32), rows=rows)
        check_vocab(gpu, blobs, ng, _some_grams(rows, ng), None, "sep", rows=rows)
    other = tc.want_hashed(gram_rows(rows, 2, 2, sep ^ 0x01), 1 << 20, 0, True)
    mine = tc.want_hashed(gram_rows(rows, 2, 2, sep), 1 << 20, 0, True)
    assert not np.array_equal(other[1], mine[1])                                       # the separator reaches the hash


@functools.lru_cache(maxsize=1)
def _protocol_batch():
    from latok_amd import batch
    tile, row_max = tc.limits()
    rng = random.Random(9)
    blobs = [t.encode("utf-8", "surrogatepass") for t in random_strings(rng, 300, 0, 90, ALPHABETS["mixed"])]
    blobs.insert(100, tc._blob([rng.randrange(90) for _ in range(row_max // 2 + 40)]))     # short in tokens, long in keys
    u8, boff = batch.pack_utf8(blobs)
    rows = tc._rows_of_slices(u8, boff)
    return u8, boff, rows, _some_grams(rows, (1, 2, 0x20))


def test_capacity_protocol_and_refused_arguments(gpu):
    from latok_amd import _lib, batch
    block, ng_max = ng_limits()
    u8, boff, rows, words = _protocol_batch()
    ng = (1, 2, 0x20)
    g = gram_rows(rows, *ng)
    n_str, n_g_want = len(rows), sum(map(len, g))
    for hashed in (None, (1 << 20, 0, True)):
        want = tc.want_hashed(g, *hashed) if hashed else tc.want_vocab(g, tc._dict(words))
        need = len(want[1])
        with batch.Vocab(words, seed=11) as vocab:
            # the size query: no entry buffers, capacity 0
            rc, nnz, n_g, o = _call(gpu, u8, boff, ng, vocab, hashed, cap=0, want_entries=False)
            assert rc == _lib.ERR_INVALID and nnz == need and n_g == n_g_want
            assert np.array_equal(o.indptr[:n_str + 1], want[0]) and (hashed or np.array_equal(o.oov[:n_str], want[3]))
            # one short: nothing written to indices or data, indptr and oov valid, the need returned
            rc, nnz, n_g, o = _call(gpu, u8, boff, ng, vocab, hashed, cap=need - 1, dt=np.int32)
            assert rc == _lib.ERR_INVALID and "capacity" in _lib.last_error() and nnz == need and o.entries_untouched()
            assert np.array_equal(o.indptr[:n_str + 1], want[0]) and (o.indptr[n_str + 1:] == -7).all()
            assert hashed or np.array_equal(o.oov[:n_str], want[3])
            # exact, with total_bytes = -1; larger than needed
            for cap in (need, need + 5, 1 << 40):
                rc, nnz, n_g, o = _call(gpu, u8, boff, ng, vocab, hashed, cap=min(cap, need + 5), total=-1)
                assert rc == 0 and nnz == need, _lib.last_error()
                tc._compare(("capacity", cap), o, n_g, g, want, np.int64, not hashed)
            # n_grams_out = NULL, oov_out = NULL
            o = tc._Out(n_str, need, np.int64)
            nnz = C.c_int64(-1)
            if hashed:
                rc = gpu.latok_hashed_ngram_counts_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, n_str, -1, hashed[1], hashed[0], 1, 1, 2, 0x20,
                                                                    o.indptr.ctypes.data, o.indices.ctypes.data, o.data.ctypes.data, need, C.byref(nnz),
                                                                    None, 0, None)
            else:
                rc = gpu.latok_ngram_counts_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, n_str, -1, vocab.handle, 1, 2, 0x20, o.indptr.ctypes.data,
                                                             None, o.indices.ctypes.data, o.data.ctypes.data, need, C.byref(nnz), None, 0, None)
            assert rc == 0 and nnz.value == need, _lib.last_error()
            tc._compare("NULL outputs", o, n_g_want, g, want[:3], np.int64, False)
            # refused before any device work, with every output untouched
            bad_ng = ((0, 1, 0x20, "min_n"), (-3, 2, 0x20, "min_n"), (3, 2, 0x20, "max_n"), (1, ng_max + 1, 0x20, "max_n"),
                      (ng_max + 1, ng_max + 1, 0x20, "max_n"), (1, 2, -1, "sep"), (1, 2, 256, "sep"), (1, 2, 0x2020, "sep"))
            for lo, hi, sep, needle in bad_ng:
                rc, nnz, n_g, o = _call(gpu, u8, boff, (lo, hi, sep), vocab, hashed, cap=need)
                assert rc == _lib.ERR_INVALID and needle in _lib.last_error(), (lo, hi, sep, _lib.last_error())
                assert (nnz, n_g) == (-1, -1) and o.entries_untouched() and (o.indptr == -7).all() and (o.oov == -7).all()
            for flag in (4, 64, 1 << 30):
                rc, nnz, n_g, o = _call(gpu, u8, boff, ng, vocab, hashed, cap=need, flags=flag)
                assert rc == _lib.ERR_INVALID and "unknown flag" in _lib.last_error() and o.entries_untouched() and (o.indptr == -7).all()
            o = tc._Out(n_str, need, np.int64)
            nnz = C.c_int64(-1)
            for ix, da, cap, needle in ((o.indices.ctypes.data, None, need, "go together"), (None, o.data.ctypes.data, need, "go together"),
                                        (None, None, need, "cap > 0")):
                if hashed:
                    rc = gpu.latok_hashed_ngram_counts_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, n_str, -1, 0, 8, 1, 1, 2, 0x20,
                                                                        o.indptr.ctypes.data, ix, da, cap, C.byref(nnz), None, 0, None)
                else:
                    rc = gpu.latok_ngram_counts_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, n_str, -1, vocab.handle, 1, 2, 0x20,
                                                                 o.indptr.ctypes.data, o.oov.ctypes.data, ix, da, cap, C.byref(nnz), None, 0, None)
                assert rc == _lib.ERR_INVALID and needle in _lib.last_error(), _lib.last_error()
                assert o.entries_untouched() and (o.indptr == -7).all() and (o.oov == -7).all()
    for bad in (0, -1, 1 << 31):
        rc, nnz, n_g, o = _call(gpu, u8, boff, ng, hashed=(bad, 0, True), cap=8)
        assert rc == _lib.ERR_INVALID and "n_features" in _lib.last_error() and o.entries_untouched() and (o.indptr == -7).all()
    rc, nnz, n_g, o = _call(gpu, u8, boff, ng, None, cap=8)
    assert rc == _lib.ERR_INVALID and "vocab" in _lib.last_error() and (o.indptr == -7).all()
    # the empty batch
    with batch.Vocab(words) as vocab:
        rc, nnz, n_g, o = _call(gpu, np.zeros(0, np.uint8), np.zeros(1, np.int64), ng, vocab, cap=4)
        assert rc == 0 and nnz == 0 and n_g == 0 and o.indptr[0] == 0 and (o.indptr[1:] == -7).all() and o.entries_untouched()
        rc, nnz, n_g, o = _call(gpu, np.zeros(0, np.uint8), np.zeros(6, np.int64), ng, vocab, cap=4, dt=np.int32)
        assert rc == 0 and nnz == 0 and not o.indptr[:6].any() and not o.oov[:5].any() and (o.indptr[6:] == -7).all() and o.entries_untouched()
        rc, nnz, n_g, o = _call(gpu, np.zeros(0, np.uint8), np.zeros(6, np.int64), ng, hashed=(8, 0, True), cap=0, want_entries=False)
        assert rc == 0 and nnz == 0 and not o.indptr[:6].any()


def test_device_pointers_equal_host_pointers(gpu):
    from latok_amd import _lib, batch
    u8, boff, rows, words = _protocol_batch()
    n_str = len(rows)
    ng = (1, 2, 0x20)
    g = gram_rows(rows, *ng)
    for hashed in (None, (64, 7, True)):
        want = tc.want_hashed(g, *hashed) if hashed else tc.want_vocab(g, tc._dict(words))
        need = len(want[1])
        sizes = (u8.nbytes + 256, boff.nbytes, (n_str + 1 + GUARD) * 4, (n_str + GUARD) * 4, (need + GUARD) * 4, (need + GUARD) * 4)
        ptrs = [gpu.latok_dev_alloc(s) for s in sizes]
        assert all(ptrs)
        try:
            d_u8, d_boff, d_indptr, d_oov, d_ix, d_da = ptrs
            _lib.check(gpu.latok_memset_dev(d_u8, 0xFF, sizes[0]))
            for p, s in zip(ptrs[2:], sizes[2:]):
                _lib.check(gpu.latok_memset_dev(p, tc.POISON, s))
            _lib.check(gpu.latok_memcpy_h2d(d_u8, u8.ctypes.data, u8.nbytes))
            _lib.check(gpu.latok_memcpy_h2d(d_boff, boff.ctypes.data, boff.nbytes))
            _lib.check(gpu.latok_sync())
            nnz, n_g = C.c_int64(-1), C.c_int64(-1)
            flags = _lib.DEVICE_PTRS | _lib.OUT_INT32
            with batch.Vocab(words) as vocab:
                if hashed:
                    rc = gpu.latok_hashed_ngram_counts_utf8_bytes_batch(d_u8, d_boff, n_str, -1, hashed[1], hashed[0], 1, ng[0], ng[1], ng[2], d_indptr,
                                                                        d_ix, d_da, need, C.byref(nnz), C.byref(n_g), flags, None)
                else:
                    rc = gpu.latok_ngram_counts_utf8_bytes_batch(d_u8, d_boff, n_str, -1, vocab.handle, ng[0], ng[1], ng[2], d_indptr, d_oov, d_ix, d_da,
                                                                 need, C.byref(nnz), C.byref(n_g), flags, None)
                assert rc == 0 and nnz.value == need and n_g.value == sum(map(len, g)), _lib.last_error()
                assert gpu.latok_debug_last_route() == (HASHED_NGRAM_ROUTE if hashed else NGRAM_ROUTE)
                o = tc._Out(n_str, need, np.int32)
                for a, p in ((o.indptr, d_indptr), (o.oov, d_oov), (o.indices, d_ix), (o.data, d_da)):
                    _lib.check(gpu.latok_memcpy_d2h(a.ctypes.data, p, a.nbytes))
                assert np.array_equal(o.indptr[:n_str + 1], want[0]) and (o.indptr[n_str + 1:].view(np.uint8) == tc.POISON).all()
                assert np.array_equal(o.indices[:need], want[1]) and np.array_equal(o.data[:need], want[2])
                assert (o.indices[need:] == POISON_32).all() and (o.data[need:] == POISON_32).all()
                if hashed:
                    assert (o.oov.view(np.uint8) == tc.POISON).all()
                else:
                    assert np.array_equal(o.oov[:n_str], want[3]) and (o.oov[n_str:].view(np.uint8) == tc.POISON).all()
                    rc = gpu.latok_ngram_counts_utf8_bytes_batch(d_u8 + 4, d_boff, n_str, int(boff[-1]), vocab.handle, 1, 2, 0x20, d_indptr, d_oov,
                                                                 d_ix, d_da, need, C.byref(nnz), None, flags, None)
                    assert rc == _lib.ERR_INVALID and "16-byte aligned" in _lib.last_error()
        finally:
            for p in ptrs:
                gpu.latok_dev_free(p)


def test_routes_and_the_neighbouring_calls(gpu):
    from latok_amd import batch
    u8, boff, rows, words = _protocol_batch()
    with batch.Vocab(words, seed=5) as vocab:
        plain = batch.term_counts_utf8_csr(u8, boff, vocab)
        assert gpu.latok_debug_last_route() == tc.TERMS_ROUTE
        a = batch.term_counts_utf8_csr(u8, boff, vocab, ngram_range=(1, 2))
        assert gpu.latok_debug_last_route() == NGRAM_ROUTE
        b = batch.term_counts_utf8_csr(u8, boff, vocab, ngram_range=(1, 2), sep=0x20)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
        assert all(np.array_equal(x, y) for x, y in zip(a, tc.want_vocab(gram_rows(rows, 1, 2, 0x20), tc._dict(words))))
        again = batch.term_counts_utf8_csr(u8, boff, vocab, ngram_range=(1, 1))
        assert gpu.latok_debug_last_route() == tc.TERMS_ROUTE and all(x.tobytes() == y.tobytes() for x, y in zip(plain, again))
        h = batch.hashed_term_counts_utf8_csr(u8, boff, n_features=1 << 10, seed=5, ngram_range=(2, 3), sep=b"_", dtype=np.int32)
        assert gpu.latok_debug_last_route() == HASHED_NGRAM_ROUTE and h[0].dtype == np.int32
        assert all(np.array_equal(x, y) for x, y in zip(h, tc.want_hashed(gram_rows(rows, 2, 3, 0x5F), 1 << 10, 5, True)))
        batch.hashed_term_counts_utf8_csr(u8, boff, n_features=1 << 10, seed=5)
        assert gpu.latok_debug_last_route() == tc.HASHED_ROUTE
        ids = batch.token_ids_utf8_csr(u8, boff, vocab)
        assert gpu.latok_debug_last_route() == tc.IDS_ROUTE
    d = tc._dict(words)
    assert ids[1].tolist() == [d.get(t, -1) for r in rows for t in r]


# ---- 8. wrappers and the example -------------------------------------------------------------------------------------------------
def test_python_wrappers(gpu):
    from latok_amd import batch
    texts = ["I love New York City", "new york , New York !", "", "   ", "x", "Ünïcode Straße straße", "a,b a,b"]
    blobs = [t.encode("utf-8") for t in texts]
    u8, boff = batch.pack_utf8(blobs)
    rows = tc._rows_of_slices(u8, boff)
    words = ["new york", "New York", "york", "a ,", "straße", "Straße straße", "ünïcode straße"]
    d = tc._dict([w.encode() for w in words])
    with batch.Vocab(words) as vocab:
        want = tc.want_vocab(gram_rows(rows, 1, 2, 0x20), d)
        for got in (batch.term_counts_batch(texts, vocab, ngram_range=(1, 2)), batch.term_counts_utf8_batch(blobs, vocab, ngram_range=(1, 2), sep=b" "),
                    batch.term_counts_utf8_csr(u8, boff, vocab, ngram_range=(1, 2), sep=32)):
            assert [x.dtype for x in got] == [np.int64, np.int32, np.int32, np.int64] and all(np.array_equal(a, b) for a, b in zip(got, want))
        # fold= chains on the device: the grams are those of the folded strings
        folded = batch.fold_utf8_batch(blobs, batch.FOLD_LOWER)
        fu8, fboff = batch.pack_utf8(folded)
        wantf = tc.want_vocab(gram_rows(tc._rows_of_slices(fu8, fboff), 1, 2, 0x20), d)
        got = batch.term_counts_utf8_batch(blobs, vocab, fold=batch.FOLD_LOWER, ngram_range=(1, 2))
        assert all(np.array_equal(a, b) for a, b in zip(got, wantf)) and 6 in got[1].tolist() and 1 not in got[1].tolist()
        wanth = tc.want_hashed(gram_rows(tc._rows_of_slices(fu8, fboff), 2, 2, 0x5F), 1 << 12, 3, True)
        goth = batch.hashed_term_counts_utf8_batch(blobs, n_features=1 << 12, seed=3, fold=batch.FOLD_LOWER, ngram_range=(2, 2), sep=b"_")
        assert len(goth) == 3 and all(np.array_equal(a, b) for a, b in zip(goth, wanth))
        empty = batch.term_counts_utf8_batch([], vocab, ngram_range=(1, 3))
        assert empty[0].tolist() == [0] and len(empty[1]) == len(empty[2]) == len(empty[3]) == 0
    for lo, hi in ranges():
        got = batch.hashed_term_counts_batch(texts, n_features=64, alternate_sign=False, ngram_range=(lo, hi))
        assert all(np.array_equal(a, b) for a, b in zip(got, tc.want_hashed(gram_rows(rows, lo, hi, 0x20), 64, 0, False)))
    for kw in (dict(ngram_range=(0, 1)), dict(ngram_range=(2, 1)), dict(ngram_range=(1, 9)), dict(ngram_range=(1, 2), sep=b"ab")):
        with pytest.raises(ValueError):
            batch.hashed_term_counts_batch(texts, **kw)


def test_c_example(gpu, tmp_path):
    exe = str(tmp_path / "ngram_counts_utf8")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "ngram_counts_utf8.c"),
                           "-L" + os.path.join(ROOT, "latok_amd"), "-llatok_hip", "-Wl,-rpath," + os.path.join(ROOT, "latok_amd"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    toks = [[b"i", b"love", b"new", b"york"], [b"new", b"york", b"new", b"york", b"city"], [], [b"york"]]
    g = gram_rows(toks, 1, 2, 0x20)
    d = tc._dict([b"new york", b"york", b"love", b"york city", b"new"])
    indptr, indices, data, oov = tc.want_vocab(g, d)
    assert lines[0] == "%d grams, %d entries" % (sum(map(len, g)), len(indices))
    for s in range(4):
        want = "  row %d:" % s + "".join(" %d:%d" % (indices[k], data[k]) for k in range(indptr[s], indptr[s + 1])) + "   (oov %d)" % oov[s]
        assert lines[2 + s] == want, (s, lines[2 + s], want)
    indptr, indices, data = tc.want_hashed(g, 16, 0, True)
    for s in range(4):
        want = "  row %d:" % s + "".join(" %d:%d" % (indices[k], data[k]) for k in range(indptr[s], indptr[s + 1]))
        assert lines[7 + s] == want, (s, lines[7 + s], want)
