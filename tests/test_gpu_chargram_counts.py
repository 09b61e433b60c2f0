"""Character n-grams inside tokens in the term counts on the device (latok_chargram_counts_utf8_bytes_batch,
latok_hashed_chargram_counts_utf8_bytes_batch, include/latok_hip.h; analyzer="char_wb" of latok_amd.batch).

The result is DEFINED by a call the parity tests already pin and by Python's own containers: the byte slices
latok_token_spans_utf8_bytes_batch reports for string s, cut into the grams of every token's padded word by
tests/helpers/chargram_ref.py (list slicing over characters) and fed to a dict (vocabulary form) or to tests/helpers/murmur3_ref.py
(hashed form), exactly as test_gpu_term_counts.py feeds the tokens themselves.  Every batch goes through the C ABI with poisoned guard
bands round every output and is checked in full against that definition; scikit-learn's own char_wb vectorizers are the outside
yardstick.  The shapes are the smallest at which the kernels can go wrong, with the workgroup size in tokens from
latok_debug_chargram_limits, the scan's chunk from latok_debug_wordpiece_limits and the longest short row of the reduce from
latok_debug_terms_limits."""
import ctypes as C
import functools
import os
import random
import subprocess

import numpy as np
import pytest

import test_gpu_term_counts as tc
from conftest import ALPHABETS, ROOT, random_strings
from helpers import chargram_ref as cr
from helpers import murmur3_collide as mc
from helpers import span_strip_content as ssc
from helpers.murmur3_ref import murmur3_ref

pytestmark = pytest.mark.gpu

CHARGRAM_ROUTE, HASHED_CHARGRAM_ROUTE = 16, 17
POISON_32, GUARD = tc.POISON_32, tc.GUARD
WIDE = ["a", "b", "é", "ω", "日", "の", "𠀀", "𝐚"]          # letters of 1, 2, 3 and 4 bytes: a run of them is one token


@functools.lru_cache(maxsize=1)
def cg_limits():
    """(kCgBlock, kNgMax) from latok_debug_chargram_limits"""
    from latok_amd import _lib
    fn = _lib.load().latok_debug_chargram_limits
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    out = np.zeros(4, np.int64)
    assert fn(out.ctypes.data, 4) == 2
    block, ng_max = int(out[0]), int(out[1])
    assert 64 <= block <= 1024 and ng_max == 8
    return block, ng_max


@functools.lru_cache(maxsize=1)
def scan_chunk():
    """entries one workgroup of the chained scan takes: entry 1 of latok_debug_wordpiece_limits"""
    from latok_amd import _lib
    fn = _lib.load().latok_debug_wordpiece_limits
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    out = np.zeros(4, np.int64)
    assert fn(out.ctypes.data, 4) == 4 and 64 <= out[1] <= 1 << 16
    return int(out[1])


# ---- the definition --------------------------------------------------------------------------------------------------------
def gram_rows(rows, min_n, max_n, pad):
    return [cr.row_grams(r, min_n, max_n, pad) for r in rows]


def n_keys_of(row, min_n, max_n):
    return sum(cr.gram_count(len(cr.chars_of(t)), min_n, max_n) for t in row)


# ---- the calls, with guard bands ---------------------------------------------------------------------------------------------
def _call(lib, u8, boff, cg, vocab=None, hashed=None, cap=0, dt=np.int64, want_oov=True, want_entries=True, total=None, flags=0):
    """one blocking call with host pointers -> (rc, nnz, n_grams, _Out); cg = (min_n, max_n, pad), hashed = (n_features, seed, alternate_sign)"""
    from latok_amd import _lib
    n_str = boff.size - 1
    total = (int(boff[-1]) if n_str > 0 else 0) if total is None else total
    o = tc._Out(n_str, cap, dt)
    nnz, n_g = C.c_int64(-1), C.c_int64(-1)
    flags |= _lib.OUT_INT32 if dt == np.int32 else 0
    ix, da = (o.indices.ctypes.data, o.data.ctypes.data) if want_entries else (None, None)
    if hashed is not None:
        n_features, seed, alt = hashed
        rc = lib.latok_hashed_chargram_counts_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, n_str, total, seed, n_features, int(alt), cg[0], cg[1],
                                                               cg[2], o.indptr.ctypes.data, ix, da, cap, C.byref(nnz), C.byref(n_g), flags, None)
    else:
        rc = lib.latok_chargram_counts_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, n_str, total, vocab.handle if vocab is not None else None,
                                                        cg[0], cg[1], cg[2], o.indptr.ctypes.data, o.oov.ctypes.data if want_oov else None, ix, da,
                                                        cap, C.byref(nnz), C.byref(n_g), flags, None)
    return rc, nnz.value, n_g.value, o


def check_vocab(lib, blobs, cg, words, ids=None, what="", seed=0, dtypes=(np.int64, np.int32), rows=None):
    """the whole definition of the vocabulary form for one batch and one range; returns (token rows, want)"""
    from latok_amd import _lib, batch
    u8, boff = batch.pack_utf8(blobs)
    rows = tc._rows_of_slices(u8, boff) if rows is None else rows
    g = gram_rows(rows, *cg)
    want = tc.want_vocab(g, tc._dict(words, ids))
    with batch.Vocab(words, ids=ids, seed=seed) as vocab:
        for dt in dtypes:
            rc, nnz, n_g, o = _call(lib, u8, boff, cg, vocab, cap=len(want[1]), dt=dt)
            assert rc == 0, (what, cg, _lib.last_error())
            assert nnz == len(want[1]), (what, cg, nnz, len(want[1]))
            assert lib.latok_debug_last_route() == CHARGRAM_ROUTE or int(boff[-1]) == 0
            tc._compare((what, cg, dt.__name__), o, n_g, g, want, dt, True)
    return rows, want


def check_hashed(lib, blobs, cg, n_features, seed=0, alternate_sign=True, what="", dtypes=(np.int64,), rows=None):
    from latok_amd import _lib, batch
    u8, boff = batch.pack_utf8(blobs)
    rows = tc._rows_of_slices(u8, boff) if rows is None else rows
    g = gram_rows(rows, *cg)
    want = tc.want_hashed(g, n_features, seed, alternate_sign)
    for dt in dtypes:
        rc, nnz, n_g, o = _call(lib, u8, boff, cg, hashed=(n_features, seed, alternate_sign), cap=len(want[1]), dt=dt)
        assert rc == 0, (what, cg, _lib.last_error())
        assert nnz == len(want[1]), (what, cg, nnz, len(want[1]))
        assert lib.latok_debug_last_route() == HASHED_CHARGRAM_ROUTE or int(boff[-1]) == 0
        tc._compare((what, cg, n_features, alternate_sign, dt.__name__), o, n_g, g, want, dt, False)
    return rows, want


def _some_grams(rows, cg, every=2):
    """a vocabulary for a batch: every `every`-th distinct gram, a few of them twice"""
    distinct = list(dict.fromkeys(g for r in rows for g in cr.row_grams(r, *cg)))
    return distinct[::every] + distinct[:6]


# ---- 1. ranges over random strings ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _alphabet_batch(name):
    from latok_amd import batch
    rng = random.Random(len(name))
    blobs = [t.encode("utf-8", "surrogatepass") for t in random_strings(rng, 160, 0, 70, ALPHABETS[name])] + [b"", b"  ", b"a a a b a a"]
    u8, boff = batch.pack_utf8(blobs)
    return blobs, u8, boff, tc._rows_of_slices(u8, boff)


@pytest.mark.parametrize("alphabet", sorted(ALPHABETS))
def test_ranges_over_random_strings(gpu, alphabet):
    """the eight ranges, both forms; n_features 64 and 2^20, alternate_sign on and off, int64 and int32 indptr (one hash seed per
    alphabet, so that the reference hashes every distinct gram once)"""
    blobs, u8, boff, rows = _alphabet_batch(alphabet)
    seed = sorted(ALPHABETS).index(alphabet)
    for k, (lo, hi) in enumerate(cr.RANGES):
        cg = (lo, hi, 0x20)
        check_vocab(gpu, blobs, cg, _some_grams(rows, cg), None, alphabet, seed=k, dtypes=(np.int32 if k % 2 else np.int64,), rows=rows)
        check_hashed(gpu, blobs, cg, 64 if k % 2 else 1 << 20, seed, k % 4 < 2, alphabet, dtypes=(np.int64 if k % 2 else np.int32,), rows=rows)


@pytest.mark.parametrize("pad", [0x00, 0xFF])
def test_other_pads(gpu, pad):
    blobs, u8, boff, rows = _alphabet_batch("mixed")
    for lo, hi in ((1, 2), (3, 5)):
        cg = (lo, hi, pad)
        check_hashed(gpu, blobs, cg, 1 << 20, 3, True, "pad", rows=rows)
        check_vocab(gpu, blobs, cg, _some_grams(rows, cg), None, "pad", dtypes=(np.int64,), rows=rows)
    other = tc.want_hashed(gram_rows(rows, 2, 2, 0x20), 1 << 20, 3, True)
    mine = tc.want_hashed(gram_rows(rows, 2, 2, pad), 1 << 20, 3, True)
    assert not np.array_equal(other[1], mine[1])                                       # the pad reaches the hash


def test_grams_that_collide_in_hash_and_length_are_told_apart_by_their_bytes(gpu):
    """crafted collisions (murmur3_collide, seed 0): pairs of 8-letter words with one hash; as tokens, each is the middle 8-gram of its
    padded word, and with range (1, 8) one of the grams among many"""
    pairs = list(mc.KNOWN_WORD_PAIRS)
    assert all(a != b and len(a) == len(b) == 8 and murmur3_ref(a, 0) == murmur3_ref(b, 0) for a, b in pairs)
    blobs = [a for a, _ in pairs] + [b for _, b in pairs] + [b"lead " + a + b" then " + b + b" end" for a, b in pairs]
    n = len(pairs)
    only_a = [a for a, _ in pairs]
    rows, (indptr, indices, data, oov) = check_vocab(gpu, blobs, (8, 8, 0x20), only_a, None, "collisions, a known", seed=0)
    assert [r[0] for r in rows[:2 * n]] == blobs[:2 * n]
    assert np.diff(indptr)[:2 * n].tolist() == [1] * n + [0] * n and oov[:2 * n].tolist() == [2] * n + [3] * n     # every b is unknown
    both = [w for p in pairs for w in p]
    rows, (indptr, indices, data, oov) = check_vocab(gpu, blobs, (8, 8, 0x20), both, None, "collisions, both known", seed=0, rows=rows)
    assert indices[:2 * n].tolist() == [2 * k for k in range(n)] + [2 * k + 1 for k in range(n)]                    # each its own id
    check_vocab(gpu, blobs, (1, 8, 0x20), both[::-1] + [b" " + a[:3] for a in only_a], None, "collisions, reversed", seed=0, dtypes=(np.int64,), rows=rows)


def test_vocabulary_words_with_the_pad_and_short_words_counted_once(gpu):
    text = [b"the other theme", b"a the", b"", b"there a a", b"I", b"to be"]
    words = [b" th", b"the", b"he ", b" a ", b"her", b" I ", b" to ", b" be ", b"a", b" "]
    rows, (indptr, indices, data, oov) = check_vocab(gpu, text, (3, 3, 0x20), words, None, "trigrams")
    assert indices[indptr[0]:indptr[1]].tolist() == [0, 1, 2, 4] and data[indptr[0]:indptr[1]].tolist() == [2, 3, 1, 1]
    assert indices[indptr[1]:indptr[2]].tolist() == [0, 1, 2, 3] and indices[indptr[3]:indptr[4]].tolist() == [0, 1, 3, 4]
    assert data[indptr[3]:indptr[4]].tolist() == [1, 1, 2, 1] and indices[indptr[4]:indptr[5]].tolist() == [5]
    # " to " has 4 characters: with (3, 5) it gives " to", "to ", then the whole word ONCE at order 4 and nothing at order 5
    rows, (indptr, indices, data, oov) = check_vocab(gpu, text, (3, 5, 0x20), words, None, "short words", rows=rows)
    assert indices[indptr[5]:indptr[6]].tolist() == [6, 7] and data[indptr[5]:indptr[6]].tolist() == [1, 1] and oov[5] == 4
    assert indices[indptr[4]:indptr[5]].tolist() == [5] and data[indptr[4]:indptr[5]].tolist() == [1] and oov[4] == 0
    rows, (indptr, indices, data, oov) = check_vocab(gpu, text, (1, 1, 0x20), words, None, "single characters", rows=rows)
    assert indices[indptr[1]:indptr[2]].tolist() == [8, 9] and data[indptr[1]:indptr[2]].tolist() == [1, 4] and oov[1] == 3
    got, (indptr, indices, data, oov) = check_vocab(gpu, text, (2, 8, 0x20), [], None, "V = 0", dtypes=(np.int64,), rows=rows)
    assert len(indices) == 0 and not indptr.any() and oov.tolist() == [n_keys_of(r, 2, 8) for r in rows]


# ---- 2. workgroup edges ------------------------------------------------------------------------------------------------------------
def _wide_word(rng, n_chars):
    return "".join(rng.choice(WIDE) for _ in range(n_chars)).encode()


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_batches_of_about_one_workgroup_of_tokens(gpu, delta):
    block, ng_max = cg_limits()
    rng = random.Random(block + delta)
    n_tok = block + delta
    toks = [_wide_word(rng, rng.randrange(1, 12)) for _ in range(n_tok)]
    for blobs, what in (([b" ".join(toks)], "one string"), ([b" ".join(toks[k:k + 7]) for k in range(0, n_tok, 7)], "rows of seven")):
        rows, _ = check_hashed(gpu, blobs, (3, 5, 0x20), 1 << 20, 0, True, what)
        assert sum(map(len, rows)) == n_tok
        check_vocab(gpu, blobs, (1, 8, 0x20), _some_grams(rows, (1, 8, 0x20)), None, what, dtypes=(np.int64,), rows=rows)


def test_rows_at_the_edges_of_a_workgroup_of_tokens(gpu):
    """a string whose tokens straddle a block edge, strings that start exactly at one, runs of empty strings on the edge"""
    block, ng_max = cg_limits()
    rng = random.Random(block)
    lens = [block - 5, 5 + 7, block - 7, 0, 0, 3, block - 3, 2 * block + 3, block - 3]
    rows = [[rng.randrange(40) for _ in range(n)] for n in lens]
    blobs = [tc._blob(r) for r in rows]
    blobs = blobs[:3] + [b"", b"  ", b""] * 50 + blobs[3:7] + [b""] * 70 + blobs[7:] + [b" ", b""]
    for cg in ((1, 2, 0x20), (3, 5, 0x20), (8, 8, 0x20)):
        got, want = check_hashed(gpu, blobs, cg, 1 << 20, 0, True, "workgroup edges")
        starts = np.cumsum([0] + [len(r) for r in got]).tolist()
        assert sum(s % block == 0 and s > 0 for s in set(starts)) >= 3 and sum(len(r) == 0 for r in got) >= 220
        assert any(a < k * block < b - 1 for a, b in zip(starts, starts[1:]) for k in (1, 2, 3))        # a row across an edge
        check_vocab(gpu, blobs, cg, _some_grams(got, cg), None, "workgroup edges", dtypes=(np.int64,), rows=got)


@pytest.mark.parametrize("delta", [-1, 0])
def test_token_counts_about_one_chunk_of_the_chained_scan(gpu, delta):
    """n_tok + 1 entries are scanned: exactly one chunk, and one entry more"""
    chunk = scan_chunk()
    rng = random.Random(chunk + delta)
    n_tok = chunk + delta
    toks = [_wide_word(rng, rng.randrange(1, 5)) for _ in range(n_tok)]
    cuts = sorted(rng.sample(range(1, n_tok), 60))
    blobs = [b" ".join(toks[a:b]) for a, b in zip([0] + cuts, cuts + [n_tok])]
    rows, _ = check_hashed(gpu, blobs, (2, 3, 0x20), 64, 1, False, "scan chunk")
    assert sum(map(len, rows)) == n_tok
    check_vocab(gpu, blobs, (2, 3, 0x20), _some_grams(rows, (2, 3, 0x20)), None, "scan chunk", dtypes=(np.int64,), rows=rows)


# ---- 3. long rows and long tokens ----------------------------------------------------------------------------------------------------
def _chars_for_keys(n_keys):
    """character counts of tokens that give n_keys grams at range (1, 1) -- a token of L characters gives L + 2 --, eight keys a token"""
    out = []
    while n_keys > 16:
        out.append(6)
        n_keys -= 8
    a = n_keys // 2
    return out + [a - 2, n_keys - a - 2]


def test_rows_short_in_tokens_and_long_in_keys(gpu):
    tile, row_max = tc.limits()
    rng = random.Random(7)
    letters = "abcdefghij"
    around = [tc._blob([rng.randrange(12) for _ in range(n)]) for n in (3, 40, 0, 9)]
    for n_keys in (row_max - 1, row_max, row_max + 1, 2 * row_max + 1):
        chars = _chars_for_keys(n_keys)
        assert sum(c + 2 for c in chars) == n_keys and min(chars) >= 1 and len(chars) <= n_keys // 8 + 1        # far fewer tokens than keys
        row = b" ".join("".join(rng.choice(letters) for _ in range(c)).encode() for c in chars)
        for blobs, what in (([row], "one row"), (around[:2] + [row] + around[2:], "among short rows")):
            got, want = check_hashed(gpu, blobs, (1, 1, 0x20), 1 << 20, 0, True, (what, n_keys))
            assert max(n_keys_of(r, 1, 1) for r in got) == n_keys and max(map(len, got)) == len(chars)
            words = _some_grams(got, (1, 1, 0x20))
            check_vocab(gpu, blobs, (1, 1, 0x20), words, [tc._scrambled_id(i) for i in range(len(words))], (what, n_keys), dtypes=(np.int64,), rows=got)
        got, want = check_hashed(gpu, around[:2] + [row] + around[2:], (2, 8, 0x20), 64, 0, True, ("orders 2 .. 8", n_keys))
        assert max(n_keys_of(r, 2, 8) for r in got) > 3 * n_keys


def test_one_token_of_5000_mixed_width_characters(gpu):
    rng = random.Random(5000)
    tok = _wide_word(rng, 5000)
    blobs = [b"short words", tok, b"", b"and " + tok[:401] + b" after"]
    rows, want = check_hashed(gpu, blobs, (1, 8, 0x20), 1 << 20, 0, True, "a long token")
    assert rows[1] == [tok] and len(cr.chars_of(tok)) == 5000 and n_keys_of(rows[1], 1, 8) == sum(5002 - n + 1 for n in range(1, 9))
    check_vocab(gpu, blobs, (1, 8, 0x20), _some_grams(rows, (1, 8, 0x20), every=3), None, "a long token", dtypes=(np.int64,), rows=rows)


def test_a_table_that_leaves_whitespace_inside_tokens(gpu):
    """under a custom rule table a token may hold whitespace: the bytes are characters like any other, next to the pad's"""
    from latok_amd import batch
    table = "UPPER_ONLY"
    batch.set_rules(*ssc.TABLES[table])
    try:
        texts = ssc.content(table, ssc.SIZES[0], "bytes", "full")[0]
        blobs = [t.encode("utf-8", "surrogatepass") for t in texts]
        rows, _ = check_hashed(gpu, blobs, (3, 5, 0x20), 64, 1, True, table)
        assert any(b" " in t for r in rows for t in r)
        check_vocab(gpu, blobs, (1, 2, 0x20), _some_grams(rows, (1, 2, 0x20)), None, table, dtypes=(np.int64,), rows=rows)
    finally:
        batch.reset_rules()


# ---- 4. malformed UTF-8 ----------------------------------------------------------------------------------------------------------------
def test_malformed_bytes_are_characters_by_the_same_rule(gpu):
    rng = random.Random(5)
    body = [t.encode("utf-8", "surrogatepass") for t in random_strings(rng, 60, 0, 60, ALPHABETS["mixed"])]
    bad = cr.MALFORMED + [b" ".join(cr.MALFORMED), b"x " + b" y ".join(cr.MALFORMED) + b" z"] + [b" " * k + t for k, t in enumerate(cr.MALFORMED)]
    blobs = body[:30] + tc.SOFT + bad + body[30:] + tc.HARD + tc.SOFT
    for cg in ((1, 1, 0x20), (3, 5, 0x20), (1, 8, 0xFF)):
        rows, _ = check_hashed(gpu, blobs, cg, 1 << 20, 0, True, "malformed")
        check_vocab(gpu, blobs, cg, _some_grams(rows, cg), None, "malformed", dtypes=(np.int64,), rows=rows)
    seen = {t for r in rows for t in r}
    assert sum(t in seen for t in cr.MALFORMED) >= len(cr.MALFORMED) // 2               # most of them come through the tokenizer whole
    rows, _ = check_hashed(gpu, bad, (2, 8, 0x20), 64, 0, False, "small malformed batch")
    check_vocab(gpu, bad, (2, 8, 0x20), _some_grams(rows, (2, 8, 0x20), every=1), None, "small malformed batch", rows=rows)


# ---- 5. protocol -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _protocol_batch():
    from latok_amd import batch
    rng = random.Random(9)
    blobs = [t.encode("utf-8", "surrogatepass") for t in random_strings(rng, 200, 0, 60, ALPHABETS["mixed"])]
    blobs.insert(100, b" ".join(_wide_word(rng, 9) for _ in range(130)))                  # a row that is long in keys
    u8, boff = batch.pack_utf8(blobs)
    rows = tc._rows_of_slices(u8, boff)
    return u8, boff, rows, _some_grams(rows, (3, 5, 0x20))


def test_capacity_protocol_and_refused_arguments(gpu):
    from latok_amd import _lib, batch
    block, ng_max = cg_limits()
    u8, boff, rows, words = _protocol_batch()
    cg = (3, 5, 0x20)
    g = gram_rows(rows, *cg)
    n_str, n_g_want = len(rows), sum(map(len, g))
    for hashed in (None, (1 << 20, 0, True)):
        want = tc.want_hashed(g, *hashed) if hashed else tc.want_vocab(g, tc._dict(words))
        need = len(want[1])
        with batch.Vocab(words, seed=11) as vocab:
            # the size query: no entry buffers, capacity 0
            rc, nnz, n_g, o = _call(gpu, u8, boff, cg, vocab, hashed, cap=0, want_entries=False)
            assert rc == _lib.ERR_INVALID and nnz == need and n_g == n_g_want
            assert np.array_equal(o.indptr[:n_str + 1], want[0]) and (hashed or np.array_equal(o.oov[:n_str], want[3]))
            # one short: nothing written to indices or data, guards intact, indptr and oov valid, the need returned
            rc, nnz, n_g, o = _call(gpu, u8, boff, cg, vocab, hashed, cap=need - 1, dt=np.int32)
            assert rc == _lib.ERR_INVALID and "capacity" in _lib.last_error() and nnz == need and o.entries_untouched()
            assert np.array_equal(o.indptr[:n_str + 1], want[0]) and (o.indptr[n_str + 1:] == -7).all()
            assert (hashed and (o.oov == -7).all()) or (np.array_equal(o.oov[:n_str], want[3]) and (o.oov[n_str:] == -7).all())
            # exact, with total_bytes = -1; larger than needed
            for cap in (need, need + 5):
                rc, nnz, n_g, o = _call(gpu, u8, boff, cg, vocab, hashed, cap=cap, total=-1)
                assert rc == 0 and nnz == need, _lib.last_error()
                tc._compare(("capacity", cap), o, n_g, g, want, np.int64, not hashed)
            # n_grams_out = NULL, oov_out = NULL
            o = tc._Out(n_str, need, np.int64)
            nnz = C.c_int64(-1)
            if hashed:
                rc = gpu.latok_hashed_chargram_counts_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, n_str, -1, hashed[1], hashed[0], 1, 3, 5, 0x20,
                                                                       o.indptr.ctypes.data, o.indices.ctypes.data, o.data.ctypes.data, need,
                                                                       C.byref(nnz), None, 0, None)
            else:
                rc = gpu.latok_chargram_counts_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, n_str, -1, vocab.handle, 3, 5, 0x20, o.indptr.ctypes.data,
                                                                None, o.indices.ctypes.data, o.data.ctypes.data, need, C.byref(nnz), None, 0, None)
            assert rc == 0 and nnz.value == need, _lib.last_error()
            tc._compare("NULL outputs", o, n_g_want, g, want[:3], np.int64, False)
            # refused before any device work, with every output untouched
            bad = ((0, 1, 0x20, "min_n"), (-3, 2, 0x20, "min_n"), (3, 2, 0x20, "max_n"), (1, ng_max + 1, 0x20, "max_n"),
                   (ng_max + 1, ng_max + 1, 0x20, "max_n"), (1, 2, -1, "pad"), (1, 2, 256, "pad"), (1, 2, 0x2020, "pad"))
            for lo, hi, pad, needle in bad:
                rc, nnz, n_g, o = _call(gpu, u8, boff, (lo, hi, pad), vocab, hashed, cap=need)
                assert rc == _lib.ERR_INVALID and needle in _lib.last_error(), (lo, hi, pad, _lib.last_error())
                assert (nnz, n_g) == (-1, -1) and o.entries_untouched() and (o.indptr == -7).all() and (o.oov == -7).all()
            for flag in (4, 64, 1 << 30):
                rc, nnz, n_g, o = _call(gpu, u8, boff, cg, vocab, hashed, cap=need, flags=flag)
                assert rc == _lib.ERR_INVALID and "unknown flag" in _lib.last_error() and o.entries_untouched() and (o.indptr == -7).all()
            o = tc._Out(n_str, need, np.int64)
            nnz = C.c_int64(-1)
            for ix, da, cap, needle in ((o.indices.ctypes.data, None, need, "go together"), (None, o.data.ctypes.data, need, "go together"),
                                        (None, None, need, "cap > 0")):
                if hashed:
                    rc = gpu.latok_hashed_chargram_counts_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, n_str, -1, 0, 8, 1, 3, 5, 0x20,
                                                                           o.indptr.ctypes.data, ix, da, cap, C.byref(nnz), None, 0, None)
                else:
                    rc = gpu.latok_chargram_counts_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, n_str, -1, vocab.handle, 3, 5, 0x20,
                                                                    o.indptr.ctypes.data, o.oov.ctypes.data, ix, da, cap, C.byref(nnz), None, 0, None)
                assert rc == _lib.ERR_INVALID and needle in _lib.last_error(), _lib.last_error()
                assert o.entries_untouched() and (o.indptr == -7).all() and (o.oov == -7).all()
    for bad_f in (0, -1, 1 << 31):
        rc, nnz, n_g, o = _call(gpu, u8, boff, cg, hashed=(bad_f, 0, True), cap=8)
        assert rc == _lib.ERR_INVALID and "n_features" in _lib.last_error() and o.entries_untouched() and (o.indptr == -7).all()
    rc, nnz, n_g, o = _call(gpu, u8, boff, cg, None, cap=8)
    assert rc == _lib.ERR_INVALID and "vocab" in _lib.last_error() and (o.indptr == -7).all()
    # the empty batch
    with batch.Vocab(words) as vocab:
        rc, nnz, n_g, o = _call(gpu, np.zeros(0, np.uint8), np.zeros(1, np.int64), cg, vocab, cap=4)
        assert rc == 0 and nnz == 0 and n_g == 0 and o.indptr[0] == 0 and (o.indptr[1:] == -7).all() and o.entries_untouched()
        rc, nnz, n_g, o = _call(gpu, np.zeros(0, np.uint8), np.zeros(6, np.int64), cg, vocab, cap=4, dt=np.int32)
        assert rc == 0 and nnz == 0 and not o.indptr[:6].any() and not o.oov[:5].any() and (o.indptr[6:] == -7).all() and o.entries_untouched()
        rc, nnz, n_g, o = _call(gpu, np.zeros(0, np.uint8), np.zeros(6, np.int64), cg, hashed=(8, 0, True), cap=0, want_entries=False)
        assert rc == 0 and nnz == 0 and not o.indptr[:6].any()
        # strings without a token: every row is empty
        u8e, boffe = batch.pack_utf8([b"  ", b"", b"\t \n"])
        rc, nnz, n_g, o = _call(gpu, u8e, boffe, cg, vocab, cap=4)
        assert rc == 0 and nnz == 0 and n_g == 0 and not o.indptr[:4].any() and not o.oov[:3].any() and o.entries_untouched()


def test_device_pointers_equal_host_pointers(gpu):
    from latok_amd import _lib, batch
    u8, boff, rows, words = _protocol_batch()
    n_str = len(rows)
    cg = (3, 5, 0x20)
    g = gram_rows(rows, *cg)
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
                # the host call's arrays, for the comparison array for array
                rc, h_nnz, h_ng, host = _call(gpu, u8, boff, cg, vocab, hashed, cap=need, dt=np.int32)
                assert rc == 0 and h_nnz == need
                if hashed:
                    rc = gpu.latok_hashed_chargram_counts_utf8_bytes_batch(d_u8, d_boff, n_str, -1, hashed[1], hashed[0], 1, cg[0], cg[1], cg[2],
                                                                           d_indptr, d_ix, d_da, need, C.byref(nnz), C.byref(n_g), flags, None)
                else:
                    rc = gpu.latok_chargram_counts_utf8_bytes_batch(d_u8, d_boff, n_str, -1, vocab.handle, cg[0], cg[1], cg[2], d_indptr, d_oov, d_ix,
                                                                    d_da, need, C.byref(nnz), C.byref(n_g), flags, None)
                assert rc == 0 and nnz.value == need and n_g.value == sum(map(len, g)) == h_ng, _lib.last_error()
                assert gpu.latok_debug_last_route() == (HASHED_CHARGRAM_ROUTE if hashed else CHARGRAM_ROUTE)
                o = tc._Out(n_str, need, np.int32)
                for a, p in ((o.indptr, d_indptr), (o.oov, d_oov), (o.indices, d_ix), (o.data, d_da)):
                    _lib.check(gpu.latok_memcpy_d2h(a.ctypes.data, p, a.nbytes))
                assert np.array_equal(o.indptr[:n_str + 1], want[0]) and (o.indptr[n_str + 1:].view(np.uint8) == tc.POISON).all()
                assert np.array_equal(o.indices[:need], want[1]) and np.array_equal(o.data[:need], want[2])
                assert (o.indices[need:] == POISON_32).all() and (o.data[need:] == POISON_32).all()
                assert np.array_equal(o.indptr[:n_str + 1], host.indptr[:n_str + 1]) and np.array_equal(o.indices[:need], host.indices[:need])
                assert np.array_equal(o.data[:need], host.data[:need])
                if hashed:
                    assert (o.oov.view(np.uint8) == tc.POISON).all()
                else:
                    assert np.array_equal(o.oov[:n_str], want[3]) and (o.oov[n_str:].view(np.uint8) == tc.POISON).all()
                    assert np.array_equal(o.oov[:n_str], host.oov[:n_str])
                    rc = gpu.latok_chargram_counts_utf8_bytes_batch(d_u8 + 4, d_boff, n_str, int(boff[-1]), vocab.handle, 3, 5, 0x20, d_indptr, d_oov,
                                                                    d_ix, d_da, need, C.byref(nnz), None, flags, None)
                    assert rc == _lib.ERR_INVALID and "16-byte aligned" in _lib.last_error()
        finally:
            for p in ptrs:
                gpu.latok_dev_free(p)


def test_routes_the_neighbouring_calls_and_a_second_context(gpu):
    from latok_amd import _lib, batch
    u8, boff, rows, words = _protocol_batch()
    want = tc.want_vocab(gram_rows(rows, 3, 5, 0x20), tc._dict(words))
    wanth = tc.want_hashed(gram_rows(rows, 2, 2, 0x5F), 1 << 10, 5, True)
    with batch.Vocab(words, seed=5) as vocab:
        plain = batch.term_counts_utf8_csr(u8, boff, vocab)
        assert gpu.latok_debug_last_route() == tc.TERMS_ROUTE
        a = batch.term_counts_utf8_csr(u8, boff, vocab, ngram_range=(3, 5), analyzer="char_wb")
        assert gpu.latok_debug_last_route() == CHARGRAM_ROUTE and all(np.array_equal(x, y) for x, y in zip(a, want))
        word_grams = batch.term_counts_utf8_csr(u8, boff, vocab, ngram_range=(1, 2))
        assert gpu.latok_debug_last_route() == 14
        b = batch.term_counts_utf8_csr(u8, boff, vocab, ngram_range=(3, 5), analyzer="char_wb", pad=0x20, sep=b"_")     # sep is ignored
        assert gpu.latok_debug_last_route() == CHARGRAM_ROUTE and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
        again = batch.term_counts_utf8_csr(u8, boff, vocab)
        assert gpu.latok_debug_last_route() == tc.TERMS_ROUTE and all(x.tobytes() == y.tobytes() for x, y in zip(plain, again))
        h = batch.hashed_term_counts_utf8_csr(u8, boff, n_features=1 << 10, seed=5, ngram_range=(2, 2), analyzer="char_wb", pad=b"_", dtype=np.int32)
        assert gpu.latok_debug_last_route() == HASHED_CHARGRAM_ROUTE and h[0].dtype == np.int32
        assert all(np.array_equal(x, y) for x, y in zip(h, wanth))
        # a second context of the same device: the vocabulary serves it, its workspace starts empty
        device = C.c_int(-1)
        _lib.check(gpu.latok_vocab_info(vocab.handle, None, None, None, C.byref(device)))
        ctx = _lib.Context(device.value)
        try:
            with ctx:
                second = batch.term_counts_utf8_csr(u8, boff, vocab, ngram_range=(3, 5), analyzer="char_wb")
                second_h = batch.hashed_term_counts_utf8_csr(u8, boff, n_features=1 << 10, seed=5, ngram_range=(2, 2), analyzer="char_wb", pad=b"_")
        finally:
            ctx.destroy()
        assert all(np.array_equal(x, y) for x, y in zip(second, want)) and all(np.array_equal(x, y) for x, y in zip(second_h, wanth))
        third = batch.term_counts_utf8_csr(u8, boff, vocab, ngram_range=(3, 5), analyzer="char_wb")
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, third))


# ---- 6. scikit-learn as the outside yardstick --------------------------------------------------------------------------------------------
SK_ALPHABET = list("abcdefgXYZ0123456789.,;:!?()'\"-éüñßÀαβγωΩ日本語のテキ🤓🎉") + [" "] * 12


@functools.lru_cache(maxsize=1)
def _sk_batch():
    from latok_amd import batch
    rng = random.Random(2024)
    texts = random_strings(rng, 120, 0, 60, SK_ALPHABET) + ["", "  ", "a", "to be or not to be", "I"]
    blobs = [t.encode("utf-8") for t in texts]
    u8, boff = batch.pack_utf8(blobs)
    rows = [[t.decode("utf-8") for t in r] for r in tc._rows_of_slices(u8, boff)]
    for r in rows:
        assert " ".join(r).split() == r, r                                             # no row may be left out
    return blobs, rows, [" ".join(r) for r in rows]


def _sk_grams(docs, r):
    from sklearn.feature_extraction.text import CountVectorizer
    an = CountVectorizer(analyzer="char_wb", ngram_range=r, lowercase=False).build_analyzer()
    return [an(d) for d in docs]


@pytest.mark.parametrize("r", cr.RANGES)
def test_scikit_learn_hashing_vectorizer(gpu, r):
    sk = pytest.importorskip("sklearn.feature_extraction.text")
    from latok_amd import batch
    blobs, rows, docs = _sk_batch()
    for n_features, alt in ((64, True), (1 << 20, False), (1 << 20, True)):
        X = sk.HashingVectorizer(analyzer="char_wb", ngram_range=r, norm=None, alternate_sign=alt, n_features=n_features, lowercase=False).transform(docs)
        X.sort_indices()
        indptr, indices, data = batch.hashed_term_counts_utf8_batch(blobs, n_features=n_features, alternate_sign=alt, analyzer="char_wb", ngram_range=r)
        assert np.array_equal(indptr, X.indptr) and np.array_equal(indices, X.indices) and np.array_equal(data, X.data.astype(np.int64))
        assert X.data.dtype.kind == "f" and (X.data == np.rint(X.data)).all()


@pytest.mark.parametrize("r", cr.RANGES)
def test_scikit_learn_count_vectorizer(gpu, r):
    sk = pytest.importorskip("sklearn.feature_extraction.text")
    from latok_amd import batch
    blobs, rows, docs = _sk_batch()
    grams = _sk_grams(docs, r)
    V = list(dict.fromkeys(g for row in grams for g in row))[::2]
    X = sk.CountVectorizer(analyzer="char_wb", ngram_range=r, vocabulary=V, lowercase=False).transform(docs)
    X.sort_indices()
    with batch.Vocab(V) as vocab:
        indptr, indices, data, oov = batch.term_counts_utf8_batch(blobs, vocab, analyzer="char_wb", ngram_range=r)
    assert np.array_equal(indptr, X.indptr) and np.array_equal(indices, X.indices) and np.array_equal(data, X.data)
    known = set(V)
    assert oov.tolist() == [sum(g not in known for g in row) for row in grams]


def test_scikit_learn_tfidf_by_composition(gpu):
    """counts -> Idf.update_csr -> tfidf_csr against TfidfVectorizer fitted on the same rows; the bound is the header's for a normalised
    row of k entries: (k + 16) * 2^-23 relative"""
    sk = pytest.importorskip("sklearn.feature_extraction.text")
    from latok_amd import batch
    blobs, rows, docs = _sk_batch()
    r = (3, 5)
    V = list(dict.fromkeys(g for row in _sk_grams(docs, r) for g in row))[::2]
    X = sk.TfidfVectorizer(analyzer="char_wb", ngram_range=r, vocabulary=V, lowercase=False).fit_transform(docs)
    X.sort_indices()
    with batch.Vocab(V) as vocab, batch.Idf(len(V)) as idf:
        indptr, indices, data, oov = batch.term_counts_utf8_batch(blobs, vocab, analyzer="char_wb", ngram_range=r)
        idf.update_csr(indptr, indices)
        got = batch.tfidf_csr(indptr, indices, data, idf)
    assert np.array_equal(indptr, X.indptr) and np.array_equal(indices, X.indices) and got.dtype == np.float32 and len(got) > 1000
    k = np.repeat(np.diff(indptr), np.diff(indptr))
    err = np.abs(got.astype(np.float64) - X.data)
    print("tfidf composition: worst error / bound = %.3f" % float((err / ((k + 16) * 2.0 ** -23 * np.abs(X.data))).max()))
    assert (err <= (k + 16) * 2.0 ** -23 * np.abs(X.data)).all()


# ---- 7. the Python surface ----------------------------------------------------------------------------------------------------------------
def test_analyzer_word_returns_todays_arrays(gpu):
    from latok_amd import batch
    blobs, u8, boff, rows = _alphabet_batch("mixed")
    texts = [b.decode("utf-8", "surrogatepass") for b in blobs]
    words = list(dict.fromkeys(t for r in rows for t in r))[::2] + [b"a a", b"b a"]
    same = lambda x, y: len(x) == len(y) and all(a.dtype == b.dtype and a.tobytes() == b.tobytes() for a, b in zip(x, y))
    with batch.Vocab(words) as vocab:
        for r in ((1, 1), (1, 2)):
            assert same(batch.term_counts_utf8_csr(u8, boff, vocab, ngram_range=r), batch.term_counts_utf8_csr(u8, boff, vocab, ngram_range=r, analyzer="word"))
            assert gpu.latok_debug_last_route() == (tc.TERMS_ROUTE if r == (1, 1) else 14)
            assert same(batch.term_counts_utf8_batch(blobs, vocab, ngram_range=r), batch.term_counts_utf8_batch(blobs, vocab, ngram_range=r, analyzer="word", pad=b"x"))
            assert same(batch.term_counts_batch(texts, vocab, ngram_range=r), batch.term_counts_batch(texts, vocab, ngram_range=r, analyzer="word"))
            assert same(batch.hashed_term_counts_utf8_csr(u8, boff, 64, ngram_range=r), batch.hashed_term_counts_utf8_csr(u8, boff, 64, ngram_range=r, analyzer="word"))
            assert gpu.latok_debug_last_route() == (tc.HASHED_ROUTE if r == (1, 1) else 15)
            assert same(batch.hashed_term_counts_utf8_batch(blobs, 64, ngram_range=r), batch.hashed_term_counts_utf8_batch(blobs, 64, ngram_range=r, analyzer="word"))
            assert same(batch.hashed_term_counts_batch(texts, 64, ngram_range=r), batch.hashed_term_counts_batch(texts, 64, ngram_range=r, analyzer="word"))
        want = tc.want_vocab(rows, tc._dict(words))
        assert all(np.array_equal(a, b) for a, b in zip(batch.term_counts_utf8_csr(u8, boff, vocab, analyzer="word"), want))


def test_python_wrappers_and_fold(gpu):
    from latok_amd import batch
    texts = ["I love New York City", "new york , New York !", "", "   ", "x", "Unicode STRASSE strasse", "a,b a,b"]
    blobs = [t.encode("utf-8") for t in texts]
    u8, boff = batch.pack_utf8(blobs)
    rows = tc._rows_of_slices(u8, boff)
    words = [" ne", "new", "ew ", " Ne", "yor", " x ", "ss", " a ", " , "]
    d = tc._dict([w.encode() for w in words])
    with batch.Vocab(words) as vocab:
        want = tc.want_vocab(gram_rows(rows, 2, 3, 0x20), d)
        for got in (batch.term_counts_batch(texts, vocab, ngram_range=(2, 3), analyzer="char_wb"),
                    batch.term_counts_utf8_batch(blobs, vocab, ngram_range=(2, 3), analyzer="char_wb", pad=b" "),
                    batch.term_counts_utf8_csr(u8, boff, vocab, ngram_range=(2, 3), analyzer="char_wb", pad=32)):
            assert [x.dtype for x in got] == [np.int64, np.int32, np.int32, np.int64] and all(np.array_equal(a, b) for a, b in zip(got, want))
        # (1, 1) is a real request with char_wb, not the plain counts
        got = batch.term_counts_utf8_batch(blobs, vocab, analyzer="char_wb")
        assert gpu.latok_debug_last_route() == CHARGRAM_ROUTE
        assert all(np.array_equal(a, b) for a, b in zip(got, tc.want_vocab(gram_rows(rows, 1, 1, 0x20), d)))
        # fold= chains on the device: char_wb of the folded batch equals char_wb on the host-lowered ASCII text
        lowered = [t.lower().encode("utf-8") for t in texts]
        lu8, lboff = batch.pack_utf8(lowered)
        lrows = tc._rows_of_slices(lu8, lboff)
        wantf = tc.want_vocab(gram_rows(lrows, 2, 3, 0x20), d)
        gotf = batch.term_counts_utf8_batch(blobs, vocab, fold=batch.FOLD_LOWER, ngram_range=(2, 3), analyzer="char_wb")
        assert all(np.array_equal(a, b) for a, b in zip(gotf, wantf)) and 3 not in gotf[1].tolist() and 3 in want[1].tolist()
        assert all(np.array_equal(a, b) for a, b in zip(gotf, batch.term_counts_utf8_batch(lowered, vocab, ngram_range=(2, 3), analyzer="char_wb")))
        wanth = tc.want_hashed(gram_rows(lrows, 3, 5, 0x5F), 1 << 12, 3, True)
        goth = batch.hashed_term_counts_utf8_batch(blobs, n_features=1 << 12, seed=3, fold=batch.FOLD_LOWER, ngram_range=(3, 5), analyzer="char_wb", pad=b"_")
        assert len(goth) == 3 and all(np.array_equal(a, b) for a, b in zip(goth, wanth))
        empty = batch.term_counts_utf8_batch([], vocab, ngram_range=(1, 3), analyzer="char_wb")
        assert empty[0].tolist() == [0] and len(empty[1]) == len(empty[2]) == len(empty[3]) == 0
    for lo, hi in cr.RANGES:
        got = batch.hashed_term_counts_batch(texts, n_features=64, alternate_sign=False, ngram_range=(lo, hi), analyzer="char_wb")
        assert all(np.array_equal(a, b) for a, b in zip(got, tc.want_hashed(gram_rows(rows, lo, hi, 0x20), 64, 0, False)))
    for kw in (dict(analyzer="char"), dict(analyzer="char_wb", ngram_range=(0, 1)), dict(analyzer="char_wb", ngram_range=(1, 9)),
               dict(analyzer="char_wb", pad=b"ab"), dict(analyzer=None)):
        with pytest.raises(ValueError):
            batch.hashed_term_counts_batch(texts, **kw)


def test_c_example(gpu, tmp_path):
    exe = str(tmp_path / "chargram_counts_utf8")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "chargram_counts_utf8.c"),
                           "-L" + os.path.join(ROOT, "latok_amd"), "-llatok_hip", "-Wl,-rpath," + os.path.join(ROOT, "latok_amd"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    toks = [[b"the", b"other", b"theme"], [b"a", b"the"], [], [b"there"]]
    g = gram_rows(toks, 3, 3, 0x20)
    d = tc._dict([b" th", b"the", b"he ", b" a ", b"her"])
    indptr, indices, data, oov = tc.want_vocab(g, d)
    assert lines[0] == "%d grams, %d entries" % (sum(map(len, g)), len(indices))
    for s in range(4):
        want = "  row %d:" % s + "".join(" %d:%d" % (indices[k], data[k]) for k in range(indptr[s], indptr[s + 1])) + "   (oov %d)" % oov[s]
        assert lines[2 + s] == want, (s, lines[2 + s], want)
    indptr, indices, data = tc.want_hashed(g, 16, 0, True)
    for s in range(4):
        want = "  row %d:" % s + "".join(" %d:%d" % (indices[k], data[k]) for k in range(indptr[s], indptr[s + 1]))
        assert lines[7 + s] == want, (s, lines[7 + s], want)
