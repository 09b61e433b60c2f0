"""Byte-level BPE on the device (latok_bpe_ids_utf8_bytes_batch, latok_bpe_padded_utf8_bytes_batch, include/latok_hip.h).

The result is DEFINED by a call the parity tests already pin and by tests/helpers/bpe_ref.py, a plain restatement of the definition
over bytes and one dict: the byte slices latok_token_spans_utf8_bytes_batch reports for string s (with the space in front under
lead_space), each cut by the reference.  Every batch goes through the C ABI with poisoned guard bands round every output and is
checked in full.  The shapes are the smallest at which the kernels can go wrong: the sizes of a workgroup, of a scan block, of the
lane form and the ceiling of max_bytes come from the library (latok_debug_bpe_limits).  Where a case needs a token with chosen bytes,
rule tables that never split make every string one token (its bytes minus the whitespace at both ends)."""
import ctypes as C
import functools
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import ALPHABETS, ROOT, random_strings
from helpers import bpe_ref as ref
from helpers import murmur3_collide as mc
from helpers import span_strip_content as ssc
from helpers.murmur3_ref import murmur3_ref

pytestmark = pytest.mark.gpu

POISON_32 = np.int32(-0x5A5A5A5B)        # 0xA5A5A5A5 as int32
GUARD = 16
IDS_ROUTE, PADDED_ROUTE = 18, 19
ONE_TOKEN_PER_STRING = (ssc._NONE, ssc._NONE, ssc._NONE)
UNK = -1
WORKED = ref.WORKED_WORDS


@functools.lru_cache(maxsize=1)
def limits():
    """(kBpeBlock, entries of one scan block, kBpeLaneBytes, the ceiling of max_bytes)"""
    from latok_amd import _lib
    fn = _lib.load().latok_debug_bpe_limits
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    out = np.zeros(4, np.int64)
    assert fn(out.ctypes.data, 4) == 4
    block, chunk, lane_bytes, ceiling = map(int, out)
    assert 64 <= block <= chunk <= 1 << 16 and block % 64 == 0 and 4 <= lane_bytes < ceiling
    return block, chunk, lane_bytes, ceiling


@pytest.fixture
def one_token_per_string(gpu):
    from latok_amd import batch
    batch.set_rules(*ONE_TOKEN_PER_STRING)
    yield
    batch.reset_rules()


@functools.lru_cache(maxsize=None)
def _trained(alphabet=b"abc", n_merges=50, seed=5):
    rng = random.Random(seed)
    return tuple(ref.train([bytes(rng.choice(alphabet) for _ in range(rng.randint(1, 10))) for _ in range(300)], n_merges))


def _rand(rng, n, alphabet=b"abc"):
    return bytes(rng.choice(alphabet) for _ in range(n))


# ---- the definition --------------------------------------------------------------------------------------------------------
def want_of(u8, boff, words, ids=None, max_bytes=4096, lead_space=False, unk=UNK):
    """(indptr, ids, spans[n, 2], n_tokens) by the reference on the slices of the spans call"""
    from latok_amd import batch
    counts, spans = batch.token_spans_utf8_bytes_csr(u8, boff)
    indptr, pids, sp = ref.cut_rows(u8, boff, counts, spans, ref.rank_dict(words), max_bytes, lead_space, unk, ids)
    return (np.array(indptr, np.int64), np.array(pids, np.int64).astype(np.int32), np.array(sp, np.int64).reshape(-1, 2), int(counts.sum()))


# ---- the calls, with guard bands ---------------------------------------------------------------------------------------------
class _Out:
    def __init__(self, n_str, cap, dt):
        self.n_str, self.cap = n_str, cap
        self.indptr = np.full(n_str + 1 + GUARD, -7, dt)
        self.ids = np.full(cap + GUARD, POISON_32, np.int32)
        self.spans = np.full(2 * (cap + GUARD), -7, dt)

    def pieces_untouched(self):
        return (self.ids == POISON_32).all() and (self.spans == -7).all()


def _call(lib, u8, boff, bpe, cap=0, dt=np.int64, unk=UNK, want_ids=True, want_spans=True, total=None, flags=0, dev=False):
    """one blocking call -> (rc, n_pieces, n_tokens, _Out); dev: everything in device memory, copied back into the _Out"""
    from latok_amd import _lib
    n_str = boff.size - 1
    total = (int(boff[-1]) if n_str > 0 else 0) if total is None else total
    o = _Out(n_str, cap, dt)
    n, n_tok = C.c_int64(-1), C.c_int64(-1)
    flags |= _lib.OUT_INT32 if dt == np.int32 else 0
    handle = bpe.handle if bpe is not None else None
    if not dev:
        rc = lib.latok_bpe_ids_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, n_str, total, handle, unk, o.indptr.ctypes.data,
                                                o.ids.ctypes.data if want_ids else None, o.spans.ctypes.data if want_spans else None, cap,
                                                C.byref(n), C.byref(n_tok), flags, None)
        return rc, n.value, n_tok.value, o
    arrays = (o.indptr, o.ids, o.spans)
    sizes = [u8.nbytes + 256, boff.nbytes] + [a.nbytes for a in arrays]
    ptrs = [lib.latok_dev_alloc(s) for s in sizes]
    assert all(ptrs)
    try:
        _lib.check(lib.latok_memset_dev(ptrs[0], 0xFF, sizes[0]))
        _lib.check(lib.latok_memcpy_h2d(ptrs[0], u8.ctypes.data, u8.nbytes))
        _lib.check(lib.latok_memcpy_h2d(ptrs[1], boff.ctypes.data, boff.nbytes))
        for a, p in zip(arrays, ptrs[2:]):
            _lib.check(lib.latok_memcpy_h2d(p, a.ctypes.data, a.nbytes))
        _lib.check(lib.latok_sync())
        rc = lib.latok_bpe_ids_utf8_bytes_batch(ptrs[0], ptrs[1], n_str, total, handle, unk, ptrs[2], ptrs[3] if want_ids else None,
                                                ptrs[4] if want_spans else None, cap, C.byref(n), C.byref(n_tok), flags | _lib.DEVICE_PTRS, None)
        for a, p in zip(arrays, ptrs[2:]):
            _lib.check(lib.latok_memcpy_d2h(a.ctypes.data, p, a.nbytes))
    finally:
        for p in ptrs:
            lib.latok_dev_free(p)
    return rc, n.value, n_tok.value, o


def _compare(what, o, n_tok_got, want, dt, has_spans=True):
    indptr, ids, spans, n_tok = want
    n_str, n = len(indptr) - 1, len(ids)
    assert n_tok_got == n_tok, (what, "token total", n_tok_got, n_tok)
    assert o.indptr.dtype == dt and np.array_equal(o.indptr[:n_str + 1], indptr), (what, "indptr")
    assert (o.indptr[n_str + 1:] == -7).all(), (what, "guard words behind indptr")
    if not np.array_equal(o.ids[:n], ids):
        k = int(np.nonzero(o.ids[:n] != ids)[0][0])
        s = int(np.searchsorted(indptr, k, "right")) - 1
        raise AssertionError((what, "piece", k, "of", n, "row", s, "got", int(o.ids[k]), "want", int(ids[k]), "wrong:", int((o.ids[:n] != ids).sum())))
    assert (o.ids[n:] == POISON_32).all(), (what, "guard words behind the ids")
    if has_spans:
        got = o.spans[:2 * n].reshape(-1, 2)
        if not np.array_equal(got, spans):
            k = int(np.nonzero((got != spans).any(axis=1))[0][0])
            raise AssertionError((what, "span of piece", k, "got", got[k].tolist(), "want", spans[k].tolist()))
        assert (o.spans[2 * n:] == -7).all(), (what, "guard words behind the spans")
    else:
        assert (o.spans == -7).all()


# width of indptr / spans x host / device pointers x with / without spans
FORMS = ((np.int64, False, True), (np.int32, False, True), (np.int64, True, True), (np.int32, True, True), (np.int64, False, False),
         (np.int32, True, False))


def check(lib, blobs, words, ids=None, max_bytes=4096, lead_space=False, seed=0, unk=UNK, what="", forms=FORMS[:2]):
    """the whole definition for one batch; returns want = (indptr, ids, spans, n_tokens)"""
    from latok_amd import _lib, batch
    u8, boff = batch.pack_utf8(blobs)
    want = want_of(u8, boff, words, ids, max_bytes, lead_space, unk)
    need = len(want[1])
    with batch.BPE(words, ids=ids, max_bytes=max_bytes, lead_space=lead_space, seed=seed) as bpe:
        for dt, dev, with_spans in forms:
            rc, n, n_tok, o = _call(lib, u8, boff, bpe, cap=need, dt=dt, unk=unk, dev=dev, want_spans=with_spans)
            assert rc == 0, (what, _lib.last_error())
            assert n == need, (what, n, need)
            assert lib.latok_debug_last_route() == IDS_ROUTE or int(boff[-1]) == 0
            _compare((what, dt.__name__, "device" if dev else "host"), o, n_tok, want, dt, has_spans=with_spans)
    return want


def _rows(want):
    return [list(zip(want[1][a:b].tolist(), *want[2][a:b].T.tolist())) for a, b in zip(want[0][:-1], want[0][1:])]


# ---- 1. the worked table and lead_space ----------------------------------------------------------------------------------------
def test_the_worked_table(gpu, one_token_per_string):
    for max_bytes in (4096, 2):
        cases = [c for c in ref.WORKED_CASES if c[1] == max_bytes]
        # (a token that begins with a space stands behind a letter-free front: the strip of the one-token rules would take the space)
        tokens = [t for t, _, _ in cases if not t.startswith(b" ")]
        want = check(gpu, tokens, WORKED, max_bytes=max_bytes, what=("worked", max_bytes), forms=FORMS)
        rows = _rows(want)
        for t, row in zip(tokens, rows):
            assert row == [c[2] for c in cases if c[0] == t][0], (t, row)
    # (` ab` is reached through lead_space, the token `ab` behind one space: test_lead_space)


def test_lead_space(gpu):
    blobs = [b"ab", b"ab ab", b"ab  ab", b"ab\tab", b"ab,ab", b" ab", b"  a", b"\ta", b"a \ta", b"", b" ", b"ab a a"]
    plain = check(gpu, blobs, WORKED, lead_space=False, what="lead_space off", forms=FORMS)
    led = check(gpu, blobs, WORKED, lead_space=True, what="lead_space on", forms=FORMS)
    assert plain[3] == led[3]
    p, q = _rows(plain), _rows(led)
    assert p[0] == q[0] == [(4, 0, 2)]                                            # at the string start
    assert p[1] == [(4, 0, 2), (4, 3, 5)] and q[1] == [(4, 0, 2), (9, 2, 3), (4, 3, 5)]   # after one space: ` ab` = ` ` + `ab` (rank 4 before 10)
    assert q[2] == [(4, 0, 2), (9, 3, 4), (4, 4, 6)]                              # after two spaces: one of them
    assert q[3] == p[3] == [(4, 0, 2), (4, 3, 5)]                                 # after a tab: dropped
    assert q[4] == p[4] and len(q[4]) == 3                                        # directly after another token
    assert q[5] == [(9, 0, 1), (4, 1, 3)] and q[6] == [(10, 1, 3)] and q[7] == [(0, 1, 2)] and q[8] == [(0, 0, 1), (0, 3, 4)]
    assert q[11] == [(4, 0, 2), (10, 2, 4), (10, 4, 6)]
    # max_bytes counts the space
    want = check(gpu, [b"ab ab"], WORKED, lead_space=True, max_bytes=2, what="lead_space, max_bytes")
    assert _rows(want)[0] == [(4, 0, 2), (-1, 2, 5)]


# ---- 2. every length at every phase ------------------------------------------------------------------------------------------------
def test_every_length_at_every_start_phase(gpu, one_token_per_string):
    lane_bytes = limits()[2]
    rng = random.Random(1)
    words = list(_trained())
    blobs, at, combos = [], 0, set()
    for n in range(1, lane_bytes + 3):
        for phase in range(4):
            pad = (phase - at) % 4
            blobs.append(b" " * pad + _rand(rng, n))
            combos.add(((at + pad) % 4, n))
            at += pad + n
    assert len(combos) == 4 * (lane_bytes + 2)
    want = check(gpu, blobs, words, what="lengths x phases", forms=FORMS)
    assert want[3] == len(blobs) and (want[1] != UNK).all() and len(want[1]) < sum(map(len, blobs)) // 2
    for k in range(4):                                                            # the batch's last byte at every phase
        check(gpu, blobs[:40] + [_rand(rng, 5 + (k - sum(map(len, blobs[:40])) - 5) % 4)], words, what=("last byte", k), forms=FORMS[:1])


# ---- 3. the edges of the two forms ---------------------------------------------------------------------------------------------------
def test_the_edges_of_the_lane_form_and_the_wave_form(gpu, one_token_per_string):
    block, chunk, lane_bytes, ceiling = limits()
    rng = random.Random(2)
    sizes = [lane_bytes - 1, lane_bytes, lane_bytes + 1, 127, 128, 129]
    tokens = [_rand(rng, n, b"abcd") for n in sizes] + [(b"ab" * n)[:n] for n in sizes] + [b"abcd" * 16, b"abcd" * 17, b"x" * 100, b"adc" * 30]
    want = check(gpu, tokens, WORKED, what="form edges", forms=FORMS)
    assert np.diff(want[0]).tolist()[6:12] == [(n + 1) // 2 for n in sizes]
    want = check(gpu, tokens, list(_trained(b"abcd", 60, 8)), what="form edges, trained", forms=FORMS[:2])
    assert (want[1] == UNK).sum() == 100
    # max_bytes below the ceiling: one byte less, exactly, one more (one unk piece); lane form and wave form
    for mb in (lane_bytes - 1, lane_bytes, lane_bytes + 1, 200):
        toks = [_rand(rng, n, b"abcd") for n in (mb - 1, mb, mb + 1)]
        want = check(gpu, toks, WORKED, max_bytes=mb, what=("max_bytes", mb))
        assert _rows(want)[2] == [(UNK, 0, mb + 1)] and len(_rows(want)[1]) > 1


def test_tokens_at_the_ceiling_of_max_bytes(gpu, one_token_per_string):
    ceiling = limits()[3]
    no_merge = (b"ad" * ceiling)[:ceiling]                                        # no adjacent pair is a word: no merge at all
    most = (b"ab" * ceiling)[:ceiling]                                            # every pair merges: the most rounds possible
    tokens = [no_merge[:-1], no_merge, no_merge + b"a", most, b"ab", (b"adc" * ceiling)[:ceiling - 1]]
    want = check(gpu, tokens, WORKED, max_bytes=ceiling, what="ceiling", forms=FORMS[:1] + FORMS[3:4])
    assert np.diff(want[0]).tolist() == [ceiling - 1, ceiling, 1, ceiling // 2, 1, ceiling - 1]
    assert _rows(want)[2] == [(UNK, 0, ceiling + 1)] and set(want[1][want[0][3]:want[0][4]].tolist()) == {4}


# ---- 4. long and short tokens in one wave ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, n_tok, long_at", [("lane 0", 64, (0,)), ("lane 63", 64, (63,)), ("the middle", 64, (17,)),
                                                  ("several", 130, (3, 4, 40, 64, 127, 129)), ("the last, partly filled wave", 64 + 10, (64 + 9,)),
                                                  ("a wave of long tokens only", 192, tuple(range(64, 128)))])
def test_long_and_short_tokens_in_one_wave(gpu, one_token_per_string, name, n_tok, long_at):
    lane_bytes = limits()[2]
    rng = random.Random(len(name))
    words = list(_trained())
    tokens = [_rand(rng, rng.randint(lane_bytes + 1, lane_bytes + 120)) if i in long_at else _rand(rng, rng.randint(1, 14)) for i in range(n_tok)]
    want = check(gpu, tokens, words, what=name, forms=FORMS[:1] + FORMS[3:4])
    assert want[3] == n_tok and (want[1] != UNK).all()
    # ... and with tokens that are words as a whole among them (the shortcut in both forms)
    whole = [tokens[i] for i in long_at[:2]] + [tokens[1]]
    check(gpu, tokens, words + whole, what=(name, "whole words"), forms=FORMS[:1])


# ---- 5. totals round a workgroup and a scan block -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_token_totals_round_a_workgroup_and_a_scan_block(gpu, delta):
    block, chunk, lane_bytes, _ = limits()
    words = list(_trained())
    rng = random.Random(delta)
    n = block + delta                                                             # n_tok = kBpeBlock - 1, kBpeBlock, kBpeBlock + 1
    toks = [_rand(rng, rng.randint(1, 9)) for _ in range(n)]
    want = check(gpu, [b" ".join(toks[:n // 3]), b"", b"  ", b" ".join(toks[n // 3:])], words, what=("workgroup", n), forms=FORMS[:1] + FORMS[3:4])
    assert want[3] == n
    m = chunk - 1 + delta                                                         # n_tok + 1 = one scan block - 1, exactly, + 1
    toks = [(b"ab", b"c", b"abcab")[i % 3] for i in range(m)]
    # strings with no token between strings with many; one token per string; one string holding every token
    many = [b"", b" "] + [b" ".join(toks[i:i + 500]) for i in range(0, m, 500)] + [b"", b"\t", b""]
    want = check(gpu, many[:4] + [b"", b""] + many[4:], words, lead_space=True, what=("scan block", m), forms=FORMS[:1])
    assert want[3] == m
    want = check(gpu, [b" ".join(toks)], words, what=("scan block, one string", m), forms=FORMS[1:2])
    assert want[3] == m
    want = check(gpu, toks[:m // 2] + [b"", b""] + toks[m // 2:], words, what=("scan block, one token per string", m), forms=FORMS[:1])
    assert want[3] == m


# ---- 6. the table -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 0x9747B28C])
def test_crafted_hash_collisions_at_a_pair_and_at_a_whole_token(gpu, one_token_per_string, seed):
    rng = random.Random(seed)
    pairs = []
    for n in (5, 6, 7, 8, 9, 12, 13, 17):
        a = bytes(rng.randrange(0x61, 0x7B) for _ in range(n))
        pairs += [(a, mc.collide(a, seed, w)) for w in mc.positions(n)[:2]]
    if seed == 0:
        pairs += list(mc.KNOWN_WORD_PAIRS)
    assert all(murmur3_ref(a, seed) == murmur3_ref(b, seed) and a != b and len(a) == len(b) for a, b in pairs)
    # at a whole token: a is a word, b has its hash and its length
    words = list(dict.fromkeys(a for a, _ in pairs))
    want = check(gpu, [b for _, b in pairs] + [a for a, _ in pairs], words, seed=seed, what="collision, whole token")
    n = len(pairs)
    assert (want[1][:want[0][n]] == UNK).all() and want[1][want[0][n]:].tolist() == [words.index(a) for a, _ in pairs]
    # at a pair: the prefixes of a and of b are words, the longest of b is not: b's last merge asks for bytes with a's hash
    for a, b in pairs[:6]:
        singles = sorted({bytes([x]) for x in a + b})
        chain_a = [a[:i] for i in range(2, len(a) + 1)]
        words = singles + chain_a + [b[:i] for i in range(2, len(b)) if b[:i] not in chain_a]
        want = check(gpu, [a, b, b + a, a + b], words, seed=seed, what=("collision, pair", a), forms=FORMS[:1])
        assert np.diff(want[0])[0] == 1 and np.diff(want[0])[1] > 1
        check(gpu, [a, b, b + a], words + [b], seed=seed, what=("collision, both resident", a), forms=FORMS[:1])


def test_word_ids_duplicates_and_an_empty_vocabulary(gpu):
    blobs = [b"ab abcd bcd", b"abab xab", b"", b"adc adcb abcde"]
    ids = [5, -3, 7, 0x7FFFFFFF, -0x80000000, 0, 0, 1, 2, 3, 4, -1, 9, 10, 11, 12]
    want = check(gpu, blobs, WORKED, ids=ids, unk=-7, seed=0x9747B28C, what="explicit ids", forms=FORMS)
    assert want[1][:4].tolist() == [-0x80000000, 1, -3, 0] and -7 in want[1].tolist()
    want = check(gpu, blobs, [b"a", b"b", b"ab", b"a", b"ab", b"", b"b"], what="duplicates: the first wins")
    assert want[1][0] == 2 and set(want[1].tolist()) <= {0, 1, 2, UNK}
    want = check(gpu, blobs, [], what="V = 0", forms=FORMS)
    assert (want[1] == UNK).all() and len(want[1]) == sum(len(b.replace(b" ", b"")) for b in blobs)
    want = check(gpu, blobs, [], max_bytes=3, what="V = 0, max_bytes")
    assert np.diff(want[0]).tolist() == [2 + 1 + 3, 1 + 3, 0, 3 + 1 + 1]
    check(gpu, blobs, [b"", b"", b""], what="empty words")


@pytest.mark.parametrize("n_merges", [10, 300])
def test_table_sizes(gpu, n_merges):
    from latok_amd import batch
    rng = random.Random(n_merges)
    corpus = [_rand(rng, rng.randint(2, 12), b"abcdefgh") for _ in range(500)]
    words = ref.train(corpus, n_merges)
    with batch.BPE(words) as bpe:
        assert bpe.info()["n_slots"] == (64 if n_merges == 10 else 1024) and bpe.info()["n_words"] == len(words) == 8 + n_merges
    blobs = [b" ".join(corpus[i:i + 6]) for i in range(0, 498, 6)]
    want = check(gpu, blobs, words, what=("table", n_merges))
    assert (want[1] != UNK).all() and want[3] == 498 < len(want[1]) < sum(map(len, corpus))


# ---- 7. the calls --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _protocol_batch():
    rng = random.Random(9)
    words = list(_trained())
    blobs = [b" ".join(_rand(rng, rng.randint(1, 12)) for _ in range(rng.randrange(0, 9))) for _ in range(200)]
    blobs[7] = _rand(rng, 150) + b" " + _rand(rng, 70)
    return blobs, words


def test_capacity_protocol_and_refusals(gpu):
    from latok_amd import _lib, batch
    blobs, words = _protocol_batch()
    u8, boff = batch.pack_utf8(blobs)
    want = want_of(u8, boff, words)
    need, n_str = len(want[1]), len(blobs)
    assert need > want[3] > 0
    with batch.BPE(words, seed=11) as bpe:
        for dev in (False, True):
            # the size query: no id buffer, capacity 0
            rc, n, n_tok, o = _call(gpu, u8, boff, bpe, cap=0, want_ids=False, want_spans=False, dev=dev)
            assert rc == _lib.ERR_INVALID and n == need and n_tok == want[3] and np.array_equal(o.indptr[:n_str + 1], want[0])
            # one short: nothing written to ids or spans, indptr valid, the need returned
            rc, n, n_tok, o = _call(gpu, u8, boff, bpe, cap=need - 1, dt=np.int32, dev=dev)
            assert rc == _lib.ERR_INVALID and "capacity" in _lib.last_error() and n == need and o.pieces_untouched()
            assert np.array_equal(o.indptr[:n_str + 1], want[0]) and (o.indptr[n_str + 1:] == -7).all()
            # exact, with total_bytes = -1; larger than needed
            for cap in (need, need + 5):
                rc, n, n_tok, o = _call(gpu, u8, boff, bpe, cap=cap, total=-1, dev=dev)
                assert rc == 0 and n == need, _lib.last_error()
                _compare(("capacity", cap, dev), o, n_tok, want, np.int64)
            assert gpu.latok_debug_last_route() == IDS_ROUTE
        # refused before any device work
        rc, n, n_tok, o = _call(gpu, u8, boff, bpe, cap=need, want_ids=False)
        assert rc == _lib.ERR_INVALID and "cap > 0" in _lib.last_error() and o.pieces_untouched() and (o.indptr == -7).all()
        rc, n, n_tok, o = _call(gpu, u8, boff, bpe, cap=-1)
        assert rc == _lib.ERR_INVALID and "capacity" in _lib.last_error() and (o.indptr == -7).all()
        for flag in (4, 64, 1 << 30):
            rc, n, n_tok, o = _call(gpu, u8, boff, bpe, cap=need, flags=flag)
            assert rc == _lib.ERR_INVALID and "unknown flag" in _lib.last_error() and o.pieces_untouched() and (o.indptr == -7).all()
        rc, n, n_tok, o = _call(gpu, u8, boff, None, cap=need)
        assert rc == _lib.ERR_INVALID and "bpe is NULL" in _lib.last_error() and (o.indptr == -7).all()
        o = _Out(n_str, need, np.int64)
        n = C.c_int64(-1)
        rc = gpu.latok_bpe_ids_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, n_str, -1, bpe.handle, UNK, None, o.ids.ctypes.data, None, need,
                                                C.byref(n), None, 0, None)
        assert rc == _lib.ERR_INVALID and "indptr_out" in _lib.last_error() and o.pieces_untouched()
        # n_str = 0 and total_bytes = 0
        rc, n, n_tok, o = _call(gpu, np.zeros(0, np.uint8), np.zeros(1, np.int64), bpe, cap=4)
        assert rc == 0 and n == 0 and n_tok == 0 and o.pieces_untouched() and (o.indptr[1:] == -7).all(), _lib.last_error()
        for dev in (False, True):
            e8, eoff = batch.pack_utf8([b"", b"", b""])
            rc, n, n_tok, o = _call(gpu, e8 if e8.size else np.zeros(1, np.uint8), eoff, bpe, cap=4, dev=dev)
            assert rc == 0 and n == 0 and n_tok == 0 and o.pieces_untouched() and o.indptr[:4].tolist() == [0] * 4 and (o.indptr[4:] == -7).all()
        # an object of another device index is refused
        device = bpe.info()["device"]
        ctx = _lib.Context(device)                                            # another context of the same device may use it
        try:
            with ctx:
                rc, n, n_tok, o = _call(gpu, u8, boff, bpe, cap=need)
                assert rc == 0
                _compare("second context", o, n_tok, want, np.int64)
        finally:
            ctx.destroy()
        if gpu.latok_device_count() > 1:
            other = _lib.Context((device + 1) % gpu.latok_device_count())
            try:
                with other:
                    rc, n, n_tok, o = _call(gpu, u8, boff, bpe, cap=need)
                    assert rc == _lib.ERR_INVALID and "device" in _lib.last_error() and o.pieces_untouched()
            finally:
                other.destroy()
    assert gpu.latok_bpe_info(None, *[None] * 7) == _lib.ERR_INVALID


def test_info_reports_what_was_built(gpu):
    from latok_amd import batch
    with batch.BPE([b"abc", b"defghij", b"", b"x", b"abc"], max_bytes=9, lead_space=True, seed=77) as bpe:
        assert bpe.info() == dict(n_words=5, n_slots=64, max_len=7, max_bytes=9, lead_space=1, seed=77, device=bpe.info()["device"]) and len(bpe) == 5
    with pytest.raises(ValueError):
        bpe.info()


# ---- 8. the padded form -----------------------------------------------------------------------------------------------------------
def _padded(lib, u8, boff, bpe, max_length, special, bos=101, eos=102, pad=0, unk=UNK, dev=False):
    from latok_amd import _lib
    n_str = boff.size - 1
    block = np.full(n_str * max_length + GUARD, POISON_32, np.int32)
    lengths = np.full(n_str + GUARD, POISON_32, np.int32)
    n = C.c_int64(-1)
    total = int(boff[-1]) if n_str else 0
    if not dev:
        rc = lib.latok_bpe_padded_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, n_str, total, bpe.handle, unk, max_length, int(special), bos, eos,
                                                   pad, block.ctypes.data, lengths.ctypes.data, C.byref(n), 0, None)
        return rc, n.value, block, lengths
    arrays = (block, lengths)
    sizes = [u8.nbytes + 256, boff.nbytes] + [a.nbytes for a in arrays]
    ptrs = [lib.latok_dev_alloc(s) for s in sizes]
    assert all(ptrs)
    try:
        _lib.check(lib.latok_memcpy_h2d(ptrs[0], u8.ctypes.data, u8.nbytes))
        _lib.check(lib.latok_memcpy_h2d(ptrs[1], boff.ctypes.data, boff.nbytes))
        for a, p in zip(arrays, ptrs[2:]):
            _lib.check(lib.latok_memcpy_h2d(p, a.ctypes.data, a.nbytes))
        _lib.check(lib.latok_sync())
        rc = lib.latok_bpe_padded_utf8_bytes_batch(ptrs[0], ptrs[1], n_str, -1, bpe.handle, unk, max_length, int(special), bos, eos, pad, ptrs[2],
                                                   ptrs[3], C.byref(n), _lib.DEVICE_PTRS | _lib.OUT_INT32, None)
        for a, p in zip(arrays, ptrs[2:]):
            _lib.check(lib.latok_memcpy_d2h(a.ctypes.data, p, a.nbytes))
    finally:
        for p in ptrs:
            lib.latok_dev_free(p)
    return rc, n.value, block, lengths


def _want_padded(want, max_length, special, bos=101, eos=102, pad=0):
    indptr, ids = want[0], want[1]
    rows, lengths = [], []
    for s in range(len(indptr) - 1):
        body = ids[indptr[s]:indptr[s + 1]].tolist()[:max_length - 2 * special]
        row = ([bos] if special else []) + body + ([eos] if special else [])
        lengths.append(len(row))
        rows.append(row + [pad] * (max_length - len(row)))
    return np.array(rows, np.int32).reshape(len(rows), max_length), np.array(lengths, np.int32)


def test_the_padded_form(gpu):
    from latok_amd import _lib, batch
    blobs = [b"", b"ab", b"abcb c", b"bcd adc", b"adcb a", b"ab ab ab ab ab ab", b"  ", b"xab a", b"ab " * 11 + b"abcde " + b"x" * 70]
    u8, boff = batch.pack_utf8(blobs)
    want = want_of(u8, boff, WORKED)
    assert np.diff(want[0]).tolist() == [0, 1, 3, 3, 5, 6, 0, 3, 11 + 2 + 70]
    with batch.BPE(WORKED) as bpe:
        for max_length, special, dev in ((6, True, False), (4, False, False), (7, True, True), (5, False, True), (1, False, False), (2, False, True),
                                         (3, True, False), (3, False, False), (128, True, False)):
            rc, n, block, lengths = _padded(gpu, u8, boff, bpe, max_length, special, pad=-9, dev=dev)
            assert rc == 0 and n == len(want[1]), _lib.last_error()
            assert gpu.latok_debug_last_route() == PADDED_ROUTE
            w_block, w_len = _want_padded(want, max_length, special, pad=-9)
            assert np.array_equal(block[:w_block.size].reshape(w_block.shape), w_block), (max_length, special, dev)
            assert np.array_equal(lengths[:len(blobs)], w_len) and (block[w_block.size:] == POISON_32).all() and (lengths[len(blobs):] == POISON_32).all()
        # refusals: a block too narrow for its specials, a stray flag bit
        for max_length, special in ((0, False), (2, True), (-1, False)):
            rc, n, block, lengths = _padded(gpu, u8, boff, bpe, 1, False)
            rc = gpu.latok_bpe_padded_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, len(blobs), -1, bpe.handle, UNK, max_length, int(special), 1, 2, 0,
                                                       block.ctypes.data, lengths.ctypes.data, None, 0, None)
            assert rc == _lib.ERR_INVALID and "max_length" in _lib.last_error()
        rc = gpu.latok_bpe_padded_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, len(blobs), -1, bpe.handle, UNK, 8, 1, 1, 2, 0, block.ctypes.data,
                                                   lengths.ctypes.data, None, 8, None)
        assert rc == _lib.ERR_INVALID and "unknown flag" in _lib.last_error()
        # a batch without a byte and a batch without a token: rows of specials and padding
        for empty in ([b"", b"", b""], [b" ", b"\t\t", b""]):
            e8, eoff = batch.pack_utf8(empty)
            e8 = e8 if e8.size else np.zeros(1, np.uint8)
            rc, n, block, lengths = _padded(gpu, e8, eoff, bpe, 4, True, pad=7)
            assert rc == 0 and n == 0 and block[:12].tolist() == [101, 102, 7, 7] * 3 and lengths[:3].tolist() == [2, 2, 2], empty
            rc, n, block, lengths = _padded(gpu, e8, eoff, bpe, 2, False, pad=7)
            assert rc == 0 and block[:6].tolist() == [7] * 6 and lengths[:3].tolist() == [0, 0, 0] and (block[6:] == POISON_32).all()
        # the Python wrapper and its attention mask
        ids, mask = batch.bpe_encode_utf8_batch(blobs, bpe, 6, bos_id=101, eos_id=102, pad_id=0)
        w_block, w_len = _want_padded(want, 6, True)
        assert ids.dtype == mask.dtype == np.int32 and np.array_equal(ids, w_block)
        assert np.array_equal(mask, (np.arange(6)[None, :] < w_len[:, None]).astype(np.int32)) and mask.sum() == w_len.sum()
        ids, mask = batch.bpe_encode_utf8_batch(blobs, bpe, 4, pad_id=-1)
        assert np.array_equal(ids, _want_padded(want, 4, False, pad=-1)[0]) and mask[0].sum() == 0 and mask[8].sum() == 4
        ids, mask = batch.bpe_encode_utf8_batch([], bpe, 4)
        assert ids.shape == mask.shape == (0, 4)


# ---- 9. text under the default rules ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alphabet", ["mixed", "words", "bmp"])
def test_random_strings_under_the_default_rules(gpu, alphabet):
    from latok_amd import batch
    rng = random.Random(len(alphabet))
    blobs = [t.encode("utf-8", "surrogatepass") for t in random_strings(rng, 250, 0, 60, ALPHABETS[alphabet])]
    blobs += [b"ab\xe6\x97 cd", b"\xc3 x", b"lone \xf0\x9f\x98", b"end\xe6", b"\xf0", b"a\x80\x80\x80\x80b", b"\xa9 cont", b"x" * 300 + b" y"]
    u8, boff = batch.pack_utf8(blobs)
    counts, spans = batch.token_spans_utf8_bytes_csr(u8, boff)
    raw, base = u8.tobytes(), np.repeat(boff[:-1], counts)
    toks = [raw[a:b] for a, b in zip((base + spans[:, 0]).tolist(), (base + spans[:, 1]).tolist())]
    words = ref.train([b" " + t for t in toks[::4]] + toks[1::8], 200)
    for lead_space in (False, True):
        want = check(gpu, blobs, words, lead_space=lead_space, what=(alphabet, lead_space), forms=FORMS[:1] + FORMS[3:4])
        assert want[3] == len(toks) and len(want[1]) >= want[3]
    assert len(words) > 100


# ---- 10. one context, shared workspace -------------------------------------------------------------------------------------------------
def test_wordpiece_then_bpe_then_term_counts_on_one_context(gpu):
    from latok_amd import batch
    rng = random.Random(4)
    words = list(_trained())
    large = [b" ".join(_rand(rng, rng.randint(1, 30)) for _ in range(rng.randrange(0, 12))) for _ in range(400)] + [_rand(rng, 300)]
    small = large[5:25]
    wp_words = [w for w in words[:30]] + [b"##" + w for w in words[:30]]
    with batch.BPE(words, lead_space=True) as bpe, batch.WordPiece(wp_words) as wp, batch.Vocab(words) as vocab:
        alone = (batch.wordpiece_ids_utf8_batch(large, wp), batch.bpe_ids_utf8_batch(large, bpe), batch.term_counts_utf8_batch(large, vocab),
                 batch.bpe_ids_utf8_batch(small, bpe))
        for _ in range(2):
            mixed = (batch.wordpiece_ids_utf8_batch(large, wp), batch.bpe_ids_utf8_batch(large, bpe), batch.term_counts_utf8_batch(large, vocab),
                     batch.bpe_ids_utf8_batch(small, bpe))           # a smaller batch behind a larger one
            for a, b in zip(alone, mixed):
                assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
        for blobs, got in ((large, alone[1]), (small, alone[3])):
            u8, boff = batch.pack_utf8(blobs)
            want = want_of(u8, boff, words, lead_space=True)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


# ---- 11. wrappers and the example -------------------------------------------------------------------------------------------------
def test_python_wrappers(gpu, tmp_path):
    import base64
    from latok_amd import batch
    texts = ["low lower lowest", "slowest  low", "", "   ", "low é", "x"]
    words = [b" ", b"l", b"o", b"w", b"e", b"r", b"s", b"t", b"lo", b"low", b" low", b"er", b"es", b"est"]
    path = tmp_path / "tiny.tiktoken"
    path.write_bytes(b"".join(base64.b64encode(w) + b" %d\n" % i for i, w in enumerate(words)))
    blobs = [t.encode() for t in texts]
    u8, boff = batch.pack_utf8(blobs)
    want = want_of(u8, boff, words, lead_space=True, unk=-2)
    with batch.BPE.from_tiktoken_file(str(path), lead_space=True) as bpe:
        assert len(bpe) == len(words)
        got = batch.bpe_ids_batch(texts, bpe, unk_id=-2)
        assert [g.dtype for g in got] == [np.int64, np.int32, np.int64]
        assert all(np.array_equal(a, b) for a, b in zip(got, want[:3]))
        assert got[1][:4].tolist() == [9, 10, 11, 10]                 # low | ' low' er | ' low' est
        got_b = batch.bpe_ids_utf8_batch(blobs, bpe, unk_id=-2)
        assert all(np.array_equal(a, b) for a, b in zip(got, got_b))
        got32 = batch.bpe_ids_utf8_csr(u8, boff, bpe, unk_id=-2, dtype=np.int32)
        assert got32[0].dtype == got32[2].dtype == np.int32 and all(np.array_equal(a, b) for a, b in zip(got, got32))
        assert batch.bpe_ids_utf8_csr(u8, boff, bpe, spans=False)[2] is None
        empty = batch.bpe_ids_utf8_batch([], bpe)
        assert empty[0].tolist() == [0] and len(empty[1]) == 0 and empty[2].shape == (0, 2)
    with pytest.raises(ValueError):
        batch.bpe_ids_batch(texts, bpe)                               # closed


def test_c_example(gpu, tmp_path):
    exe = str(tmp_path / "bpe_utf8")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "bpe_utf8.c"),
                           "-L" + os.path.join(ROOT, "latok_amd"), "-llatok_hip", "-Wl,-rpath," + os.path.join(ROOT, "latok_amd"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0] == "7 tokens, 13 pieces", lines[0]
    assert lines[1] == "  row 0: 'low'[0,3) ' low'[3,7) 'er'[7,9) ' low'[9,13) 'est'[13,16)"
    assert lines[2] == "  row 1: 's'[0,1) 'low'[1,4) 'est'[4,7) ' low'[8,12)"
    assert lines[3] == "  row 2:" and lines[4] == "  row 3:" and lines[5] == "  row 4: 'low'[0,3) ' '[3,4) '?'[4,5) '?'[5,6)"
    assert lines[6] == "  input_ids 0 (7 used): 1 109 110 111 110 113 2 0 0 0 0 0"
    assert lines[8] == "  input_ids 2 (2 used): 1 2 0 0 0 0 0 0 0 0 0 0"
