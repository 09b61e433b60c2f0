"""Token ids on the device (latok_vocab_*, latok_token_ids_utf8_bytes_batch / latok_flow_token_ids_utf8_bytes, include/latok_hip.h).

The result is DEFINED by a call the parity tests already pin and by a Python dict: ids[rank(s, k)] = d.get(slice, unk_id) for the
k-th byte slice latok_token_spans_utf8_bytes_batch reports for string s, d = the vocabulary built with setdefault (the first of
a duplicate wins).  Every batch here is checked against that definition in full -- counts and records against the spans call for
int64 and int32, every id against the dict, guard words behind ids[n] and behind the records that must stay untouched, the route
-- for two unk_id values and for default and explicit word ids.  What makes the byte compare visible are crafted strings with the
hash of a vocabulary word (tests/helpers/murmur3_collide.py): they must come out as unk_id."""
import ctypes as C
import functools
import os
import random
import subprocess
import zlib

import numpy as np
import pytest

from conftest import ALPHABETS, ROOT, RULE_SETS, random_strings
from helpers import murmur3_collide as mc
from helpers import span_strip_content as ssc
from helpers.murmur3_ref import murmur3_ref

pytestmark = pytest.mark.gpu

POISON = 0xA5
POISON_ID = np.int32(-0x5A5A5A5B)        # 0xA5A5A5A5 as int32
GUARD = 16
IDS_ROUTE = 7
HASH_ROUTE = 6
UNKS = (-1, 0x7FFFFFFF)
ONE_TOKEN_PER_STRING = (ssc._NONE, ssc._NONE, ssc._NONE)      # no rule holds anywhere: the only boundary is the string's start
SOFT = [b"ab\xe6\x97 cd", b"\xc3 x", b"lone \xf0\x9f\x98", b"end\xe6", b"next starts ascii", b"\xe6\x97\xa5\xe6", b"\xf0", b"x\xc3"]
HARD = [b"a\x80\x80\x80\x80b", b"\xa9 starts with a continuation byte"]


def wave_bytes():
    """kHashWaveBytes: entry 14 of latok_debug_limits"""
    from latok_amd import _lib
    fn = _lib.load().latok_debug_limits
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    out = np.zeros(15, np.int64)
    assert fn(out.ctypes.data, 15) == 15 and out[14] >= 64
    return int(out[14])


def _enc(texts):
    return [t.encode("utf-8", "surrogatepass") for t in texts]


def _slices(u8, boff, counts, spans):
    """the byte slices the records of the spans call name, in rank order"""
    raw = u8.tobytes()
    base = np.repeat(boff[:-1], counts.astype(np.int64))
    lo, hi = (base + spans[:, 0]).tolist(), (base + spans[:, 1]).tolist()
    return [raw[a:b] for a, b in zip(lo, hi)]


def _explicit_ids(n):
    """negative and repeated values"""
    return [(-3, 5, 5, 0x7FFFFFFF, -0x80000000, 0, -1)[i % 7] + (i // 7 if i % 7 == 1 else 0) for i in range(n)]


def _dict(words, ids=None):
    d = {}
    for i, w in enumerate(words):
        if w:
            d.setdefault(w, i if ids is None else ids[i])
    return d


def _ids_host(lib, u8, boff, vocab, unk, cap, dt=np.int64, want_spans=True, want_counts=True, want_ids=True, total=None, flags=0):
    """the blocking call with host pointers -> (rc, n, ids incl. guard words, records incl. guard rows, counts)"""
    from latok_amd import _lib
    n_str = boff.size - 1
    total = (int(boff[-1]) if n_str > 0 else 0) if total is None else total
    ids = np.full(cap + GUARD, POISON_ID, np.int32)
    sp = np.full((cap + GUARD, 2), -7, dt)
    counts = np.full(n_str, -7, dt)
    n = C.c_int64(-1)
    rc = lib.latok_token_ids_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, n_str, total, vocab.handle if vocab is not None else None, unk,
                                              counts.ctypes.data if want_counts else None, sp.ctypes.data if want_spans else None,
                                              ids.ctypes.data if want_ids else None, cap, C.byref(n),
                                              flags | (_lib.OUT_INT32 if dt == np.int32 else 0), None)
    return rc, n.value, ids, sp, counts


def _check_definition(lib, blobs, words, what, seed=0, dtypes=(np.int64, np.int32), unks=UNKS, id_forms=(False, True)):
    """the whole definition for one batch and one vocabulary; returns (u8, boff, counts, slices, ids under the default ids and unks[0])"""
    from latok_amd import _lib, batch
    u8, boff = batch.pack_utf8(blobs)
    toks, first = None, None
    for explicit in id_forms:
        word_ids = _explicit_ids(len(words)) if explicit else None
        d = _dict(words, word_ids)
        with batch.Vocab(words, ids=word_ids, seed=seed) as vocab:
            assert len(vocab) == len(words) and vocab.n_slots >= max(64, 2 * len(words)) and vocab.n_slots & (vocab.n_slots - 1) == 0
            for dt in dtypes:
                counts, spans = batch.token_spans_utf8_bytes_csr(u8, boff, dt)
                if toks is None:
                    toks = _slices(u8, boff, counts, spans)
                n_tok = len(toks)
                for unk in unks:
                    want = np.fromiter((d.get(t, unk) for t in toks), np.int32, n_tok)
                    rc, n, ids, sp, c = _ids_host(lib, u8, boff, vocab, unk, n_tok, dt)
                    assert rc == 0, (what, unk, _lib.last_error())
                    assert lib.latok_debug_last_route() == IDS_ROUTE or int(boff[-1]) == 0
                    assert n == n_tok, (what, unk, n, n_tok)
                    assert c.dtype == dt and np.array_equal(c, counts), (what, unk, "counts")
                    assert np.array_equal(sp[:n], spans.reshape(-1, 2)), (what, unk, "records")
                    if not np.array_equal(ids[:n], want):
                        k = int(np.nonzero(ids[:n] != want)[0][0])
                        raise AssertionError((what, unk, explicit, "id of token", k, "of", n, len(toks[k]), toks[k][:40], int(ids[k]), int(want[k])))
                    assert (ids[n:] == POISON_ID).all(), (what, unk, "guard words behind the ids")
                    assert (sp[n:] == -7).all(), (what, unk, "guard rows behind the records")
                    if first is None:
                        first = ids[:n].copy()
    return u8, boff, counts, toks, first


@pytest.fixture
def one_token_per_string(gpu):
    from latok_amd import batch
    batch.set_rules(*ONE_TOKEN_PER_STRING)
    yield
    batch.reset_rules()


def _token(rng, n):
    """n bytes, none of them whitespace at either end, blanks inside now and then"""
    body = bytearray(rng.choice(b"abcdefghijklmnopqrstuvwxyzABCXYZ0123456789.,:/@#$!?-_(){}[]") for _ in range(n))
    for i in range(1, n - 1):
        if rng.random() < 0.08:
            body[i] = 0x20
    return bytes(body)


def _lengths():
    T = wave_bytes()
    return list(range(1, 81)) + list(range(T - 3, T + 4))


def _placed(tokens_at):
    """blobs that put token i at absolute byte `at` of the packed batch: every token is a string of its own, the gaps are
    whitespace-only strings (no token)"""
    blobs, pos = [], 0
    for at, tok in tokens_at:
        assert at >= pos, (at, pos)
        if at > pos:
            blobs.append(b" " * (at - pos))
        blobs.append(tok)
        pos = at + len(tok)
    return blobs


def _partner(tok, seed, k):
    """a string with tok's length and hash and other bytes, None where none exists (1 to 4 bytes: the function is injective)"""
    where = mc.positions(len(tok))
    return mc.collide(tok, seed, where[k % len(where)]) if where else None


# ---- 1. lengths and alignments ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _aligned_tokens():
    rng = random.Random(50)
    at, pos = [], 0
    for n in _lengths():
        for al in range(16):
            start = pos + ((al - pos) % 16)
            at.append((start, _token(rng, n)))
            pos = start + n
    return at


@pytest.mark.parametrize("vocabulary", ["the tokens", "their partners", "both"])
def test_every_length_at_every_start_alignment(gpu, one_token_per_string, vocabulary):
    SEED = 0x9747B28C
    at = _aligned_tokens()
    toks = [t for _, t in at]
    partners = [p for p in (_partner(t, SEED, k) for k, t in enumerate(toks)) if p is not None]
    assert len(partners) == sum(len(t) >= 5 for t in toks) and not set(partners) & set(toks)
    assert all(murmur3_ref(p, SEED) == murmur3_ref(t, SEED) for p, t in zip(partners[::37], [t for t in toks if len(t) >= 5][::37]))
    words = {"the tokens": toks, "their partners": partners, "both": partners + toks}[vocabulary]
    u8, boff, counts, got, ids = _check_definition(gpu, _placed(at), words, ("start alignments", vocabulary), seed=SEED)
    assert got == toks                                   # every string is one whole token
    if vocabulary == "their partners":
        assert (ids == UNKS[0]).all()                    # the same hash, the same length, other bytes: unknown
    else:
        assert (ids != UNKS[0]).all()
    # the partners as the batch, the tokens as the vocabulary: each crafted string is one whole token, and unknown
    if vocabulary == "the tokens":
        pat = [(a, _partner(t, SEED, k)) for k, (a, t) in enumerate(at) if len(t) >= 5]
        u8, boff, counts, got, ids = _check_definition(gpu, _placed(pat), toks, "partners as tokens", seed=SEED, dtypes=(np.int64,), id_forms=(False,))
        assert got == [p for _, p in pat] and (ids == UNKS[0]).all()


@pytest.mark.parametrize("edge", [64, 4096, 4 * 4096])
def test_tokens_that_cross_a_word_a_tile_and_a_workgroup_edge(gpu, one_token_per_string, edge):
    """a token that begins in the last 8 bytes in front of the edge and ends behind it: every length that can"""
    rng = random.Random(edge)
    at, e = [], 0
    step = edge * (8 if edge == 64 else 1)      # (64-byte words: the longest token is shorter than 8 words)
    for n in _lengths():
        for d in range(1, 9):
            if n > d:
                e += step
                at.append((e - d, _token(rng, n)))
    toks = [t for _, t in at]
    words = toks[::2] + [p for p in (_partner(t, 1, k) for k, t in enumerate(toks[1::2])) if p]      # half known, half look-alikes
    u8, boff, counts, got, ids = _check_definition(gpu, _placed(at), words, ("edge", edge), seed=1, unks=(-1,))
    assert got == toks and (ids[::2] >= 0).all() and (ids[1::2] == -1).mean() > 0.9


class _Dev:
    """device buffers of one batch: the input (with room behind it) and poisoned outputs"""

    def __init__(self, lib, in_bytes, n_str, cap):
        self.lib, self.cap, self.n_str = lib, cap, n_str
        self.sizes = (in_bytes + 256, (n_str + 1) * 8, n_str * 8 + 16, (cap + GUARD) * 16, (cap + GUARD) * 4, 64)
        self.ptrs = [lib.latok_dev_alloc(s) for s in self.sizes]
        assert all(self.ptrs)
        self.u8, self.boff, self.counts, self.spans, self.ids, self.res = self.ptrs

    def load(self, u8, boff, fill=0):
        from latok_amd import _lib
        _lib.check(self.lib.latok_memset_dev(self.u8, fill, self.sizes[0]))
        for p, s in zip(self.ptrs[2:], self.sizes[2:]):
            _lib.check(self.lib.latok_memset_dev(p, POISON, s))
        if u8.nbytes:
            _lib.check(self.lib.latok_memcpy_h2d(self.u8, u8.ctypes.data, u8.nbytes))
        _lib.check(self.lib.latok_memcpy_h2d(self.boff, boff.ctypes.data, boff.nbytes))
        _lib.check(self.lib.latok_sync())

    def read(self, dt=np.int64):
        from latok_amd import _lib
        ids, sp = np.empty(self.cap + GUARD, np.int32), np.empty((self.cap + GUARD, 2), dt)
        counts, res = np.empty(self.n_str, dt), np.empty(2, np.int64)
        for a, p in ((ids, self.ids), (sp, self.spans), (counts, self.counts), (res, self.res)):
            if a.nbytes:
                _lib.check(self.lib.latok_memcpy_d2h(a.ctypes.data, p, a.nbytes))
        return ids, sp, counts, res

    def free(self):
        for p in self.ptrs:
            self.lib.latok_dev_free(p)


def test_a_token_that_ends_on_the_last_byte_of_the_batch(gpu, one_token_per_string):
    """total_bytes = 0 .. 3 (mod 4); whatever the device buffer holds behind total_bytes (0x00, then 0xFF) stays out of the compare"""
    from latok_amd import _lib, batch
    rng = random.Random(52)
    lengths = _lengths()
    toks = [_token(rng, n) for n in lengths]
    # the vocabulary also holds every token + one more byte (0x00 and 0xFF): what lies behind the batch must not make those match
    words = toks + [b"xxxxxxxx", b"xxxxxxxxx", b"xxxxxxxxxx", b"xxxxxxxxxxx"] + [t + b"\x00" for t in toks] + [t + b"\xff" for t in toks]
    d = _Dev(gpu, 64 + max(lengths) + 8, 2, 2)
    n = C.c_int64(-1)
    try:
        with batch.Vocab(words, seed=3) as vocab:
            for k, tok in enumerate(toks):
                for m in range(4):
                    head = b"x" * (8 + (m - len(tok)) % 4) + b" " * 4          # total = 12 + length + ((m - length) mod 4) = m (mod 4)
                    u8, boff = batch.pack_utf8([head, tok])
                    assert int(boff[-1]) % 4 == m
                    got = []
                    for fill in (0x00, 0xFF):
                        d.load(u8, boff, fill)
                        rc = gpu.latok_token_ids_utf8_bytes_batch(d.u8, d.boff, 2, int(boff[-1]), vocab.handle, -1, d.counts, d.spans, d.ids, 2,
                                                                  C.byref(n), _lib.DEVICE_PTRS, None)
                        assert rc == 0 and n.value == 2, _lib.last_error()
                        ids, sp, c, _ = d.read()
                        assert c.tolist() == [1, 1] and sp[:2].tolist() == [[0, len(head) - 4], [0, len(tok)]]
                        assert ids[:2].tolist() == [len(toks) + len(head) - 12, k], (len(tok), m, fill, ids[:2])
                        assert (ids[2:] == POISON_ID).all()
                        got.append(ids[:2].tolist())
                    assert got[0] == got[1], (len(tok), m)
    finally:
        d.free()


# ---- 2. long tokens --------------------------------------------------------------------------------------------------------
def _long_token(seed, n):
    body = np.random.default_rng(seed).integers(0x21, 0x7F, n, dtype=np.uint8)      # no whitespace: nothing to strip
    return body.tobytes()


@functools.lru_cache(maxsize=1)
def _long_cases():
    """(token, [crafted partners: other bytes in block 0, 63, 64, the last whole block, the tail -- where the length has them])"""
    T = wave_bytes()
    out = []
    for i, n in enumerate((T - 1, T, T + 1, 5003, 1 << 20)):
        tok = _long_token(10 + i, n)
        nb = n // 4
        where = [w for w in (0, 63, 64, nb - 2) if 0 <= w < nb - 1] + (["tail"] if n % 4 else [])
        out.append((tok, [mc.collide(tok, 7, w) for w in dict.fromkeys(where)]))
    return out


def test_long_tokens_hit_and_their_look_alikes_miss(gpu, one_token_per_string):
    cases = _long_cases()
    T = wave_bytes()
    assert [len(t) for t, _ in cases] == [T - 1, T, T + 1, 5003, 1 << 20] and [len(p) for _, p in cases] == [3, 2, 3, 5, 4]
    toks = [t for t, _ in cases]
    look_alikes = [p for _, ps in cases for p in ps]
    blobs = [b"xy"] + toks + [b"", b"ab cd"] + look_alikes
    # the tokens are words: hits; the look-alikes are not: unknown, each still one whole token
    u8, boff, counts, got, ids = _check_definition(gpu, blobs, toks + [b"xy"], "long tokens", seed=7, dtypes=(np.int64,))
    assert got == [b"xy"] + toks + [b"ab cd"] + look_alikes
    assert ids.tolist() == [5, 0, 1, 2, 3, 4, -1] + [-1] * len(look_alikes)
    # the look-alikes are the words: now the tokens are unknown
    u8, boff, counts, got, ids = _check_definition(gpu, blobs, look_alikes, "long look-alikes", seed=7, dtypes=(np.int32,), unks=(-1,), id_forms=(False,))
    assert ids.tolist() == [-1] * 7 + list(range(len(look_alikes)))


def test_a_tile_of_two_rounds_and_a_string_that_began_before_its_tile(gpu):
    """2048 tokens in one 4096-byte tile (two rounds of its wave), then one string over three tiles with long tokens in it"""
    T = wave_bytes()
    long_toks = [bytes(97 + (i + j * j) % 26 for j in range(n)) for i, n in enumerate((70, 129, T + 1, 3000, 2 * T, 5000))]
    blobs = [b"a " * 2048, b" ".join(long_toks), b"xy"]
    u8, boff, counts, toks, ids = _check_definition(gpu, blobs, [b"a"] + long_toks[::2], "two rounds", dtypes=(np.int64,), unks=(-1,), id_forms=(False,))
    assert counts.tolist() == [2048, 6, 1] and ids.tolist() == [0] * 2048 + [1, -1, 2, -1, 3, -1, -1]


def test_many_long_tokens_meet_in_one_wave(gpu, one_token_per_string):
    rng = random.Random(53)
    T = wave_bytes()
    sizes = [rng.randint(300, 340) for _ in range(40)] + [rng.randint(300, 5000) for _ in range(22)] + [T + 1, 5000]
    assert len(sizes) == 64 and min(sizes) > T
    blobs = [_long_token(100 + i, n) for i, n in enumerate(sizes)]
    words = blobs[::3] + [mc.collide(b, 0, "tail" if len(b) % 4 else 1) for b in blobs[1::3]] + [b"short"]
    blobs[5:5] = [b"short", b"  ", b"", b"tok"]                     # short tokens between them: both forms in one round
    u8, boff, counts, toks, ids = _check_definition(gpu, blobs, words, "64 long tokens")
    assert sorted(len(t) for t in toks if len(t) > T) == sorted(sizes)
    assert (ids >= 0).sum() == 22 + 1                   # every third long token and "short"; no look-alike, no other token


# ---- 3. vocabulary sizes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("v", [0, 1, 32, 33])
def test_small_vocabularies(gpu, v):
    from latok_amd import batch
    rng = random.Random(v)
    texts = random_strings(rng, 300, 0, 60, ALPHABETS["mixed"])
    blobs = _enc(texts)
    u8, boff = batch.pack_utf8(blobs)
    counts, spans = batch.token_spans_utf8_bytes_csr(u8, boff)
    distinct = sorted(set(_slices(u8, boff, counts, spans)))
    words = [distinct[(7 * i) % len(distinct)] for i in range(v)]
    u8, boff, counts, toks, ids = _check_definition(gpu, blobs, words, ("V", v))
    assert (ids == -1).all() if v == 0 else (ids >= 0).any() and (ids == -1).any()
    with batch.Vocab(words) as vocab:
        assert vocab.n_slots == (64 if v <= 32 else 128)


def _fast_strings(seed, n, hi, alpha):
    g = np.random.default_rng(seed)
    lens = g.integers(0, hi + 1, n)
    s = "".join(np.array(alpha, dtype=object)[g.integers(0, len(alpha), int(lens.sum()))].tolist())
    off = np.concatenate([[0], np.cumsum(lens)]).tolist()
    return [s[a:b] for a, b in zip(off[:-1], off[1:])]


def test_a_vocabulary_of_about_fifty_thousand_words(gpu):
    """the distinct tokens of random `mixed` strings, every second one left out: a table of 2^17 slots, 2 MiB"""
    from latok_amd import batch
    blobs = _enc(_fast_strings(91, 80000, 150, ALPHABETS["mixed"]))
    u8, boff = batch.pack_utf8(blobs)
    counts, spans = batch.token_spans_utf8_bytes_csr(u8, boff, np.int32)
    distinct = list(dict.fromkeys(_slices(u8, boff, counts, spans)))        # in order of first appearance
    words = distinct[::2]
    assert 40000 <= len(words) <= 65000, len(words)
    probe = blobs[:20000]
    u8, boff, counts, toks, ids = _check_definition(gpu, probe, words, "50 000 words", seed=0xFFFFFFFF, dtypes=(np.int32,), unks=(-1,), id_forms=(False,))
    known = (ids >= 0).mean()
    assert 0.3 < known < 0.999, known                   # both outcomes occur in bulk (frequent tokens are mostly early, even-ranked or not)
    with batch.Vocab(words) as vocab:
        assert vocab.n_slots == 1 << 17


def test_a_cluster_at_the_last_slot_wraps(gpu):
    """20 words whose home is the last slot of the table (slot count from latok_vocab_info): they spill over slot 0 .. 18"""
    from latok_amd import _lib, batch
    seed = 3
    filler = [b"f%d" % i for i in range(20)]
    with batch.Vocab(filler + [b"p%d" % i for i in range(20)], seed=seed) as probe_size:
        n_slots, s2 = C.c_int64(0), C.c_uint32(0)
        _lib.check(gpu.latok_vocab_info(probe_size.handle, None, C.byref(n_slots), C.byref(s2), None))
        assert n_slots.value == probe_size.n_slots == 128 and s2.value == seed
    n_slots = n_slots.value
    cluster, i = [], 0
    while len(cluster) < 21:
        w = b"k%d" % i
        if murmur3_ref(w, seed) & (n_slots - 1) == n_slots - 1:
            cluster.append(w)
        i += 1
    outsider = cluster.pop()
    words = cluster + filler
    blobs = [b" ".join(cluster[::-1]), outsider + b" " + b" ".join(filler), b"k0 k1 " + outsider + b" " + cluster[19] + b" " + cluster[0]]
    u8, boff, counts, toks, ids = _check_definition(gpu, blobs, words, "wrapped cluster", seed=seed)
    assert ids[:20].tolist() == list(range(19, -1, -1)) and ids[20] == -1 and ids[21:41].tolist() == list(range(20, 40))


# ---- 4. content and rules --------------------------------------------------------------------------------------------------
def _half_vocabulary(toks):
    distinct = list(dict.fromkeys(toks))
    return distinct[::2] + distinct[:6]                   # (a few duplicates behind)


@functools.lru_cache(maxsize=1)
def _three_sizes(alphabet):
    rng = random.Random(zlib.crc32(alphabet.encode()))
    alpha = ALPHABETS[alphabet]
    return ((random_strings(rng, 200, 0, 12, alpha), "one tile"),                 # (cut below to what fits one tile)
            (random_strings(rng, 3000, 0, 40, alpha), "<= 262144 bytes"),
            (random_strings(rng, 24000, 0, 120, alpha) + ["".join(rng.choice(alpha) for _ in range(150000))], "several hundred tiles"))


@pytest.mark.parametrize("alphabet", sorted(ALPHABETS))
def test_random_strings_at_three_sizes(gpu, oracle, alphabet):
    from latok_amd import batch
    for texts, what in _three_sizes(alphabet):
        texts = list(texts)
        blobs = _enc(texts)
        total = sum(map(len, blobs))
        if what == "one tile":
            while total > 4096:
                blobs.pop()
                texts.pop()
                total = sum(map(len, blobs))
            assert len(blobs) < 512 and total <= 4096
        elif what == "<= 262144 bytes":
            assert 4096 < total <= 262144
        else:
            assert total > 300 * 4096
        u8, boff = batch.pack_utf8(blobs)
        counts, spans = batch.token_spans_utf8_bytes_csr(u8, boff)
        words = _half_vocabulary(_slices(u8, boff, counts, spans))
        big = total > 262144
        u8, boff, counts, toks, ids = _check_definition(gpu, blobs, words, (alphabet, what), seed=zlib.crc32(what.encode()),
                                                        dtypes=(np.int32,) if big else (np.int64, np.int32), unks=UNKS[:1] if big else UNKS,
                                                        id_forms=(False,) if big else (False, True))
        assert (ids >= 0).any() and (ids == -1).any()
        if not big:                 # built-in tables: the slices are the reference's tokens
            want = [tok.encode("utf-8", "surrogatepass") for t in texts if t != "" for tok in oracle.tokenize(t)]
            assert toks == want, (alphabet, what)


@pytest.mark.parametrize("name", sorted(RULE_SETS))
def test_runtime_rule_tables(gpu, name):
    from latok_amd import batch
    rng = random.Random(77)
    texts = random_strings(rng, 2500, 0, 150, ALPHABETS["mixed"]) + ["   ", "", " a ", "　x　"]
    batch.set_rules(*RULE_SETS[name])
    try:
        blobs = _enc(texts)
        u8, boff = batch.pack_utf8(blobs)
        counts, spans = batch.token_spans_utf8_bytes_csr(u8, boff)
        words = _half_vocabulary(_slices(u8, boff, counts, spans))
        _check_definition(gpu, blobs, words, ("rules", name), unks=UNKS[:1])
        _check_definition(gpu, blobs[:40], words, ("rules small", name), unks=UNKS[1:], id_forms=(True,))
    finally:
        batch.reset_rules()


@functools.lru_cache(maxsize=2)
def _ssc_content(table, size):
    return [_enc(texts) for texts in ssc.content(table, size, "bytes", "full")]


@pytest.mark.parametrize("size", ssc.SIZES)
@pytest.mark.parametrize("table", sorted(ssc.TABLES))
def test_tables_that_leave_whitespace_inside_tokens(gpu, table, size):
    """interior whitespace is part of the word, only the two ends of a token are stripped"""
    from latok_amd import batch
    batch.set_rules(*ssc.TABLES[table])
    try:
        for i, blobs in enumerate(_ssc_content(table, size)):
            u8, boff = batch.pack_utf8(blobs)
            counts, spans = batch.token_spans_utf8_bytes_csr(u8, boff)
            toks = _slices(u8, boff, counts, spans)
            words = _half_vocabulary(toks) + [t.strip() + b" " for t in toks[:50]]       # with a blank behind: never a token
            _check_definition(gpu, blobs, words, (table, size, "ABCD"[i]), seed=i, dtypes=(np.int64,), unks=UNKS[:1])
    finally:
        batch.reset_rules()


def test_malformed_bytes_are_compared_as_they_are(gpu):
    rng = random.Random(5)
    body = _enc(random_strings(rng, 3000, 0, 120, ALPHABETS["mixed"]))
    odd = [b"\xe6\x97", b"\xc3", b"\xf0\x9f\x98", b"end\xe6", b"\xf0", b"x\xc3", b"a\x80\x80\x80\x80b", b"\xe6\x97\xa5\xe6", b"\xa9"]
    words = odd + [b"ab", b"cd", b"lone", b"x", b"\xe6\x97\xa5"]
    _check_definition(gpu, body[:1500] + SOFT + body[1500:] + SOFT, words, "soft malformed", dtypes=(np.int64,))
    _check_definition(gpu, body[:700] + HARD + SOFT + body[700:] + HARD, words, "hard malformed", dtypes=(np.int32,))
    u8, boff, counts, toks, ids = _check_definition(gpu, SOFT + HARD, words, "small malformed batch")
    assert b"\xe6\x97" in toks and b"\xc3" in toks and any(b"\x80" in t for t in toks)    # nothing refused, nothing repaired
    assert ids[toks.index(b"\xe6\x97")] == 0 and ids[toks.index(b"\xc3")] == 1


# ---- 5. protocol -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _protocol_batch():
    from latok_amd import batch
    rng = random.Random(9)
    blobs = _enc(random_strings(rng, 900, 0, 90, ALPHABETS["mixed"]))
    u8, boff = batch.pack_utf8(blobs)
    counts, spans = batch.token_spans_utf8_bytes_csr(u8, boff)
    toks = _slices(u8, boff, counts, spans)
    return u8, boff, counts, spans, toks, _half_vocabulary(toks)


def test_capacity_protocol_and_optional_outputs(gpu):
    from latok_amd import _lib, batch
    u8, boff, counts, spans, toks, words = _protocol_batch()
    need = len(toks)
    d = _dict(words)
    with batch.Vocab(words, seed=11) as vocab:
        for unk in UNKS:
            want = np.array([d.get(t, unk) for t in toks], np.int32)
            # size query
            rc, n, ids, sp, c = _ids_host(gpu, u8, boff, vocab, unk, 0, want_ids=False, want_spans=False)
            assert rc == _lib.ERR_INVALID and n == need and np.array_equal(c, counts)
            # one short: nothing written, counts valid, the needed count returned
            rc, n, ids, sp, c = _ids_host(gpu, u8, boff, vocab, unk, need - 1)
            assert rc == _lib.ERR_INVALID and "capacity" in _lib.last_error() and n == need
            assert (ids == POISON_ID).all() and (sp == -7).all() and np.array_equal(c, counts)
            # spans_out = NULL, counts_out = NULL, each alone and together; total_bytes = -1 is resolved from byte_off
            for ws, wc in ((False, True), (True, False), (False, False)):
                rc, n, ids, sp, c = _ids_host(gpu, u8, boff, vocab, unk, need, np.int32, want_spans=ws, want_counts=wc, total=-1)
                assert rc == 0 and n == need and np.array_equal(ids[:n], want) and (ids[n:] == POISON_ID).all(), (ws, wc)
                assert np.array_equal(sp[:n], spans) and (sp[n:] == -7).all() if ws else (sp == -7).all()
                assert np.array_equal(c, counts) if wc else (c == -7).all()
                assert gpu.latok_debug_last_route() == IDS_ROUTE
        # ids_out = NULL with a capacity is refused; so are a stray flag bit and a NULL vocabulary
        rc, n, ids, sp, c = _ids_host(gpu, u8, boff, vocab, -1, need, want_ids=False)
        assert rc == _lib.ERR_INVALID and "ids_out" in _lib.last_error() and (sp == -7).all() and (c == -7).all()
        for flag in (4, 64, 1 << 30):
            rc, n, ids, sp, c = _ids_host(gpu, u8, boff, vocab, -1, need, flags=flag)
            assert rc == _lib.ERR_INVALID and "unknown flag" in _lib.last_error()
            assert (ids == POISON_ID).all() and (sp == -7).all() and (c == -7).all()
        rc, n, ids, sp, c = _ids_host(gpu, u8, boff, None, -1, need)
        assert rc == _lib.ERR_INVALID and "vocab" in _lib.last_error() and (ids == POISON_ID).all()


def test_device_pointers_equal_host_pointers(gpu):
    from latok_amd import _lib, batch
    rng = random.Random(21)
    blobs = _enc(random_strings(rng, 4000, 0, 200, ALPHABETS["mixed"]))
    u8, boff = batch.pack_utf8(blobs)
    counts, spans = batch.token_spans_utf8_bytes_csr(u8, boff, np.int32)
    words = _half_vocabulary(_slices(u8, boff, counts, spans))
    u8, boff, counts, toks, want = _check_definition(gpu, blobs, words, "host pointers", seed=1, dtypes=(np.int32,), unks=(-1,), id_forms=(False,))
    need = len(toks)
    d = _Dev(gpu, u8.nbytes, boff.size - 1, need)
    try:
        d.load(u8, boff)
        n = C.c_int64(-1)
        flags = _lib.DEVICE_PTRS | _lib.OUT_INT32
        with batch.Vocab(words, seed=1) as vocab:
            rc = gpu.latok_token_ids_utf8_bytes_batch(d.u8, d.boff, d.n_str, -1, vocab.handle, -1, d.counts, d.spans, d.ids, need, C.byref(n), flags, None)
            assert rc == 0 and n.value == need, _lib.last_error()
            assert gpu.latok_debug_last_route() == IDS_ROUTE
            ids, sp, c, _ = d.read(np.int32)
            assert np.array_equal(ids[:need], want) and (ids[need:] == POISON_ID).all()
            assert np.array_equal(sp[:need], spans) and (sp[need:].view(np.uint8) == POISON).all() and np.array_equal(c, counts)
            # an unaligned device input is refused
            rc = gpu.latok_token_ids_utf8_bytes_batch(d.u8 + 4, d.boff, d.n_str, int(boff[-1]), vocab.handle, -1, d.counts, d.spans, d.ids, need,
                                                      C.byref(n), flags, None)
            assert rc == _lib.ERR_INVALID and "16-byte aligned" in _lib.last_error()
    finally:
        d.free()


def test_empty_strings_whitespace_and_nothing(gpu):
    from latok_amd import batch
    body = [b"some text, here", b"more"]
    words = [b"some", b",", b"more", b""]
    for blobs in ([b""] * 70 + body + [b""] * 130 + body + [b""] * 70, [b""] * 200 + body, [b""] * 5, [b"", b"x", b""]):
        _check_definition(gpu, blobs, words, "runs of empty strings")
    ws = [b"   ", b"\t\n", "　　".encode(), b" " * 5000, b""] * 3
    u8, boff, counts, toks, ids = _check_definition(gpu, ws, words, "all whitespace")
    assert toks == [] and not counts.any()
    with batch.Vocab(words) as vocab:
        # n_str = 0
        rc, n, ids, sp, c = _ids_host(gpu, np.zeros(0, np.uint8), np.zeros(1, np.int64), vocab, -1, 4)
        assert rc == 0 and n == 0 and (ids == POISON_ID).all() and (sp == -7).all()
        # total_bytes = 0 with strings: counts cleared
        rc, n, ids, sp, c = _ids_host(gpu, np.zeros(0, np.uint8), np.zeros(6, np.int64), vocab, -1, 4)
        assert rc == 0 and n == 0 and not c.any() and (ids == POISON_ID).all()
        assert batch.token_ids_utf8_batch([], vocab) == [] and [a.tolist() for a in batch.token_ids_batch(["", " "], vocab)] == [[], []]


def test_a_vocabulary_serves_a_second_context_of_its_device(gpu):
    from latok_amd import _lib, batch
    u8, boff, counts, spans, toks, words = _protocol_batch()
    d = _dict(words)
    want = [d.get(t, -1) for t in toks]
    with batch.Vocab(words, seed=5) as vocab:
        device = C.c_int(-1)
        _lib.check(gpu.latok_vocab_info(vocab.handle, None, None, None, C.byref(device)))
        first = batch.token_ids_utf8_csr(u8, boff, vocab)[1].tolist()
        ctx = _lib.Context(device.value)
        try:
            with ctx:
                assert batch.token_ids_utf8_csr(u8, boff, vocab)[1].tolist() == want
        finally:
            ctx.destroy()
        assert first == want == batch.token_ids_utf8_csr(u8, boff, vocab)[1].tolist()
        if gpu.latok_device_count() > 1:      # a context of another device is refused
            other = _lib.Context((device.value + 1) % gpu.latok_device_count())
            try:
                with other:
                    rc, n, ids, sp, c = _ids_host(gpu, u8, boff, vocab, -1, len(toks))
                    assert rc == _lib.ERR_INVALID and "device" in _lib.last_error() and (ids == POISON_ID).all()
            finally:
                other.destroy()


# ---- 6. the flow -----------------------------------------------------------------------------------------------------------
def test_flow_batches_alternating_over_two_id_buffers(gpu):
    from latok_amd import _lib, batch
    rng = random.Random(33)
    batches = [_enc(random_strings(rng, n, 0, hi, ALPHABETS[a])) for n, hi, a in ((3000, 150, "mixed"), (50, 30, "words"), (6000, 90, "bmp"),
                                                                                 (2000, 300, "latin1"))]
    packed = [batch.pack_utf8(b) for b in batches]
    sliced = []
    for u8, boff in packed:
        counts, spans = batch.token_spans_utf8_bytes_csr(u8, boff)
        sliced.append((counts, spans, _slices(u8, boff, counts, spans)))
    words = _half_vocabulary([t for _, _, toks in sliced for t in toks])
    d_words = _dict(words)
    want = [(len(toks), np.array([d_words.get(t, -9) for t in toks], np.int32), spans, counts) for counts, spans, toks in sliced]
    cap = max(w[0] for w in want)
    devs = [_Dev(gpu, u8.nbytes, boff.size - 1, cap) for u8, boff in packed]
    outs = [gpu.latok_dev_alloc((cap + GUARD) * 4) for _ in range(2)]

    def ids_of(p):
        got = np.empty(cap + GUARD, np.int32)
        _lib.check(gpu.latok_memcpy_d2h(got.ctypes.data, p, got.nbytes))
        return got

    vocab = batch.Vocab(words, seed=0x9747B28C)                 # one shared vocabulary
    try:
        for d, (u8, boff) in zip(devs, packed):
            d.load(u8, boff)
        for first in (0, 2):                # two batches in flight at a time, one per id buffer; nothing waits in between
            pair = devs[first:first + 2]
            for i, d in enumerate(pair):
                total = int(packed[first + i][1][-1])
                batch.flow_token_ids_utf8_bytes(d.u8, d.boff, d.n_str, total if i else -1, vocab, d.counts, d.spans, outs[i], cap, d.res, unk_id=-9)
            batch.flow_wait()
            for i, d in enumerate(pair):
                n, wi, wsp, wc = want[first + i]
                _, sp, c, res = d.read()
                assert res.tolist() == [n, 0], (first + i, res)
                assert np.array_equal(sp[:n], wsp) and np.array_equal(c, wc), first + i
                assert np.array_equal(ids_of(outs[i])[:n], wi), first + i
        # resubmission into the same id buffer with no wait between: the second result wins
        a, b = devs[0], devs[2]
        batch.flow_token_ids_utf8_bytes(a.u8, a.boff, a.n_str, int(packed[0][1][-1]), vocab, a.counts, a.spans, outs[0], cap, a.res, unk_id=-9)
        batch.flow_token_ids_utf8_bytes(b.u8, b.boff, b.n_str, int(packed[2][1][-1]), vocab, b.counts, b.spans, outs[0], cap, b.res, unk_id=-9)
        batch.flow_wait()
        assert np.array_equal(ids_of(outs[0])[:want[2][0]], want[2][1])
        # a batch whose capacity is too small leaves ids and records untouched and reports the needed count, read late
        d = devs[0]
        d.load(*packed[0])
        _lib.check(gpu.latok_memset_dev(outs[1], POISON, (cap + GUARD) * 4))
        _lib.check(gpu.latok_sync())
        batch.flow_token_ids_utf8_bytes(d.u8, d.boff, d.n_str, int(packed[0][1][-1]), vocab, d.counts, d.spans, outs[1], want[0][0] - 1, d.res, unk_id=-9)
        batch.flow_wait()
        _, sp, c, res = d.read()
        assert (ids_of(outs[1]) == POISON_ID).all() and (sp.view(np.uint8) == POISON).all()
        assert res.tolist() == [want[0][0], 0] and np.array_equal(c, want[0][3])
        # an "unbounded" capacity works like the exact one; counts and records are optional; int32 records
        batch.flow_token_ids_utf8_bytes(d.u8, d.boff, d.n_str, int(packed[0][1][-1]), vocab, None, None, outs[1], 1 << 62, d.res, unk_id=-9, dtype=np.int32)
        batch.flow_wait()
        n = want[0][0]
        got = ids_of(outs[1])
        assert np.array_equal(got[:n], want[0][1]) and (got[n:] == POISON_ID).all() and d.read()[3].tolist() == [n, 0]
        # an empty batch in the flow: zero counts, zero total
        e = _Dev(gpu, 0, 3, 4)
        try:
            e.load(np.zeros(0, np.uint8), np.zeros(4, np.int64))
            batch.flow_token_ids_utf8_bytes(e.u8, e.boff, 3, 0, vocab, e.counts, e.spans, e.ids, 4, e.res)
            batch.flow_wait()
            ids, sp, c, res = e.read()
            assert res.tolist() == [0, 0] and not c.any() and (ids == POISON_ID).all()
        finally:
            e.free()
    finally:
        vocab.close()
        for d in devs:
            d.free()
        for p in outs:
            gpu.latok_dev_free(p)


# ---- 7. wrappers, example, neighbours --------------------------------------------------------------------------------------
def test_python_wrappers(gpu, oracle):
    from latok_amd import batch
    rng = random.Random(3)
    texts = random_strings(rng, 500, 0, 80, ALPHABETS["mixed"]) + ["", "   ", "x", "a,b"]
    texts = [t for t in texts if "\ud800" not in t]
    tokens = [oracle.tokenize(text) if text != "" else [] for text in texts]
    distinct = list(dict.fromkeys(t for row in tokens for t in row))
    words = distinct[::2] + [",", b"b"]                       # str and bytes, mixed
    d = _dict([w.encode() if isinstance(w, str) else w for w in words])
    with batch.Vocab(words) as vocab:
        assert len(vocab) == len(words)
        for unk in (-1, 0, 0x7FFFFFFF, -0x80000000):
            got = batch.token_ids_batch(texts, vocab, unk_id=unk)
            assert all(g.dtype == np.int32 for g in got) and [g.tolist() for g in got] == [[d.get(t.encode(), unk) for t in row] for row in tokens]
        blobs = _enc(texts + ["\ud800 lone"])
        u8, boff = batch.pack_utf8(blobs)
        counts, ids, spans = batch.token_ids_utf8_csr(u8, boff, vocab, dtype=np.int32, spans=True)
        c2, s2 = batch.token_spans_utf8_bytes_csr(u8, boff, np.int32)
        assert ids.dtype == np.int32 and counts.dtype == spans.dtype == np.int32 and np.array_equal(counts, c2) and np.array_equal(spans, s2)
        assert ids.tolist() == [d.get(t, -1) for t in _slices(u8, boff, c2, s2)]
        c3, i3 = batch.token_ids_utf8_csr(u8, boff, vocab)
        assert c3.dtype == np.int64 and np.array_equal(c3, counts) and np.array_equal(i3, ids)
        rows = batch.token_ids_utf8_batch(blobs, vocab)
        assert [len(r) for r in rows] == counts.tolist() and np.array_equal(np.concatenate(rows), ids)
    assert vocab.handle is None
    with pytest.raises(ValueError):
        batch.token_ids_batch(texts, vocab)                   # closed
    v2 = batch.Vocab(["a", "日本"], ids=[4, -4], seed=9)
    assert [r.tolist() for r in batch.token_ids_batch(["a 日本 b"], v2, unk_id=7)] == [[4, -4, 7]]
    v2.close()
    v2.close()


def test_c_example(gpu, tmp_path):
    exe = str(tmp_path / "token_ids_utf8")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "token_ids_utf8.c"),
                           "-L" + os.path.join(ROOT, "latok_amd"), "-llatok_hip", "-Wl,-rpath," + os.path.join(ROOT, "latok_amd"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0] == "0 (12 tokens): This=0 is=1 a=2 #test=3 !=4 Testing=5 ,=6 Testing=5 ,=6 1=7 2=8 3=-1"
    assert lines[1] == "1 (3 tokens): this=-1 is=1 not=-1"
    assert lines[2] == "2 (0 tokens):" and lines[3] == "3 (0 tokens):"
    assert lines[4] == "4 (3 tokens): a=2 日本語=9 🤓=-1"


def test_the_hashes_call_is_unchanged_by_an_ids_call(gpu):
    """in one session: the hashes of a batch before and after an ids call on it are the same words, and the routes stay apart"""
    from latok_amd import batch
    u8, boff, counts, spans, toks, words = _protocol_batch()
    before = batch.token_hashes_utf8_csr(u8, boff, seed=5, spans=True)
    assert gpu.latok_debug_last_route() == HASH_ROUTE
    with batch.Vocab(words, seed=5) as vocab:
        batch.token_ids_utf8_csr(u8, boff, vocab)
        assert gpu.latok_debug_last_route() == IDS_ROUTE
        after = batch.token_hashes_utf8_csr(u8, boff, seed=5, spans=True)
        assert gpu.latok_debug_last_route() == HASH_ROUTE
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert before[1].tolist() == [murmur3_ref(t, 5) for t in toks]
