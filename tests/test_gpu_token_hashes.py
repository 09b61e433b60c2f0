"""Token hashes on the device (latok_token_hashes_utf8_bytes_batch / latok_flow_token_hashes_utf8_bytes, include/latok_hip.h).

The result is DEFINED by a call the parity tests already pin: hashes[rank(s, k)] = MurmurHash3 x86_32 of the k-th byte slice
latok_token_spans_utf8_bytes_batch reports for string s.  Every batch here is checked against that definition in full -- counts
and records against the spans call for int64 and int32, every hash against tests/helpers/murmur3_ref.py of the slice, guard words
behind hashes[n] and behind the records that must stay untouched, the route -- for the seeds 0, 1, 0x9747b28c and 0xffffffff; the
published vectors of the function go through the device, under the built-in tables the slices are also what the oracle's
tokenize() gives, and a golden file replays tokens the real reference produced.

Mutants of the new code (scratch builds, one change each) and the tests here that caught them:
  tail bytes taken in the wrong order    published vectors, lengths and alignments (all three), long tokens, random content
  length not xored in                    published vectors, lengths and alignments (all three), long tokens, random content
  the wave fold started from lane 1      lengths and alignments (the lengths above kHashWaveBytes), long tokens (both)
  the mask of the last dword dropped     published vectors, lengths and alignments (all three), long tokens, random content"""
import ctypes as C
import functools
import json
import os
import random
import subprocess
import zlib

import numpy as np
import pytest

from conftest import ALPHABETS, GOLDEN, ROOT, RULE_SETS, random_strings
from helpers import span_strip_content as ssc
from helpers.murmur3_ref import SEEDS, VECTORS, murmur3_ref

pytestmark = pytest.mark.gpu

POISON = 0xA5
POISON32 = 0xA5A5A5A5
GUARD = 16
HASH_ROUTE = 6
ONE_TOKEN_PER_STRING = (ssc._NONE, ssc._NONE, ssc._NONE)      # no rule holds anywhere: the only boundary is the string's start
SOFT = [b"ab\xe6\x97 cd", b"\xc3 x", b"lone \xf0\x9f\x98", b"end\xe6", b"next starts ascii", b"\xe6\x97\xa5\xe6", b"\xf0", b"x\xc3"]
HARD = [b"a\x80\x80\x80\x80b", b"\xa9 starts with a continuation byte"]

_H = {}


def H(seed, tok):
    """murmur3_ref of a slice (tokens repeat: each (seed, token) is hashed on the host once)"""
    k = (seed, tok)
    v = _H.get(k)
    if v is None:
        if len(_H) > 400000:
            _H.clear()
        v = _H[k] = murmur3_ref(tok, seed)
    return v


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


def _hash_host(lib, u8, boff, seed, cap, dt=np.int64, want_spans=True, want_counts=True, want_hashes=True, total=None, flags=0):
    """the blocking call with host pointers -> (rc, n, hashes incl. guard words, records incl. guard rows, counts)"""
    from latok_amd import _lib
    n_str = boff.size - 1
    total = (int(boff[-1]) if n_str > 0 else 0) if total is None else total
    h = np.full(cap + GUARD, POISON32, np.uint32)
    sp = np.full((cap + GUARD, 2), -7, dt)
    counts = np.full(n_str, -7, dt)
    n = C.c_int64(-1)
    rc = lib.latok_token_hashes_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, n_str, total, seed, counts.ctypes.data if want_counts else None,
                                                 sp.ctypes.data if want_spans else None, h.ctypes.data if want_hashes else None, cap,
                                                 C.byref(n), flags | (_lib.OUT_INT32 if dt == np.int32 else 0), None)
    return rc, n.value, h, sp, counts


def _check_definition(lib, blobs, what, seeds=SEEDS, dtypes=(np.int64, np.int32)):
    """the whole definition for one batch; returns (u8, boff, counts, slices)"""
    from latok_amd import _lib, batch
    u8, boff = batch.pack_utf8(blobs)
    toks = None
    for dt in dtypes:
        counts, spans = batch.token_spans_utf8_bytes_csr(u8, boff, dt)
        if toks is None:
            toks = _slices(u8, boff, counts, spans)
        n_tok = len(toks)
        for seed in seeds:
            want = np.fromiter((H(seed, t) for t in toks), np.uint32, n_tok)
            rc, n, h, sp, c = _hash_host(lib, u8, boff, seed, n_tok, dt)
            assert rc == 0, (what, seed, _lib.last_error())
            assert lib.latok_debug_last_route() == HASH_ROUTE or int(boff[-1]) == 0
            assert n == n_tok, (what, seed, n, n_tok)
            assert c.dtype == dt and np.array_equal(c, counts), (what, seed, "counts")
            assert np.array_equal(sp[:n], spans.reshape(-1, 2)), (what, seed, "records", int(np.nonzero(sp[:n] != spans.reshape(-1, 2))[0][0]))
            if not np.array_equal(h[:n], want):
                k = int(np.nonzero(h[:n] != want)[0][0])
                raise AssertionError((what, hex(seed), "hash of token", k, "of", n, len(toks[k]), toks[k][:40], hex(int(h[k])), hex(int(want[k]))))
            assert (h[n:] == POISON32).all(), (what, seed, "guard words behind the hashes")
            assert (sp[n:] == -7).all(), (what, seed, "guard rows behind the records")
    return u8, boff, counts, toks


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


# ---- 1. the published vectors through the device ----------------------------------------------------------------------------
def test_published_vectors_through_the_device(gpu, one_token_per_string):
    strings = []
    for data, _, _ in VECTORS:
        if data not in strings:
            strings.append(data)
    u8, boff, counts, toks = _check_definition(gpu, strings, "published vectors")
    assert counts.tolist() == [0 if s == b"" else 1 for s in strings]          # "The quick brown fox ..." is ONE token, blanks inside
    assert toks == [s for s in strings if s]
    for seed in sorted({s for _, s, _ in VECTORS}):
        rc, n, h, _, _ = _hash_host(gpu, u8, boff, seed, len(toks))
        assert rc == 0 and n == len(toks)
        for data, s, word in VECTORS:
            if s == seed and data:
                assert int(h[toks.index(data)]) == word, (data, hex(seed), hex(int(h[toks.index(data)])), hex(word))


# ---- 2. lengths and alignments ---------------------------------------------------------------------------------------------
def test_every_length_at_every_start_alignment(gpu, one_token_per_string):
    rng = random.Random(50)
    at, pos = [], 0
    for n in _lengths():
        for al in range(16):
            start = pos + ((al - pos) % 16)
            at.append((start, _token(rng, n)))
            pos = start + n
    _check_definition(gpu, _placed(at), "start alignments")


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
    _check_definition(gpu, _placed(at), ("edge", edge))


class _Dev:
    """device buffers of one batch: the input (with room behind it) and poisoned outputs"""

    def __init__(self, lib, in_bytes, n_str, cap):
        self.lib, self.cap, self.n_str = lib, cap, n_str
        self.sizes = (in_bytes + 256, (n_str + 1) * 8, n_str * 8 + 16, (cap + GUARD) * 16, (cap + GUARD) * 4, 64)
        self.ptrs = [lib.latok_dev_alloc(s) for s in self.sizes]
        assert all(self.ptrs)
        self.u8, self.boff, self.counts, self.spans, self.hashes, self.res = self.ptrs

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
        h, sp = np.empty(self.cap + GUARD, np.uint32), np.empty((self.cap + GUARD, 2), dt)
        counts, res = np.empty(self.n_str, dt), np.empty(2, np.int64)
        for a, p in ((h, self.hashes), (sp, self.spans), (counts, self.counts), (res, self.res)):
            if a.nbytes:
                _lib.check(self.lib.latok_memcpy_d2h(a.ctypes.data, p, a.nbytes))
        return h, sp, counts, res

    def free(self):
        for p in self.ptrs:
            self.lib.latok_dev_free(p)


def test_a_token_that_ends_on_the_last_byte_of_the_batch(gpu, one_token_per_string):
    """total_bytes = 0 .. 4 (mod 4); whatever the device buffer holds behind total_bytes (0x00, then 0xFF) stays out of the hash"""
    from latok_amd import _lib, batch
    rng = random.Random(52)
    lengths = _lengths()
    d = _Dev(gpu, 64 + max(lengths) + 8, 2, 2)
    n = C.c_int64(-1)
    try:
        for length in lengths:
            tok = _token(rng, length)
            for m in range(5):
                head = b"x" * (8 + (m - length) % 4) + b" " * 4          # total = 12 + length + ((m - length) mod 4) = m (mod 4)
                u8, boff = batch.pack_utf8([head, tok])
                assert int(boff[-1]) % 4 == m % 4
                got = []
                for fill in (0x00, 0xFF):
                    d.load(u8, boff, fill)
                    for seed in SEEDS:
                        rc = gpu.latok_token_hashes_utf8_bytes_batch(d.u8, d.boff, 2, int(boff[-1]), seed, d.counts, d.spans, d.hashes, 2,
                                                                     C.byref(n), _lib.DEVICE_PTRS, None)
                        assert rc == 0 and n.value == 2, _lib.last_error()
                        h, sp, c, _ = d.read()
                        assert c.tolist() == [1, 1] and sp[:2].tolist() == [[0, len(head) - 4], [0, length]]
                        assert int(h[1]) == H(seed, tok) and int(h[0]) == H(seed, head[:-4]), (length, m, fill, hex(seed))
                        assert (h[2:] == POISON32).all()
                        got.append(h[:2].tolist())
                assert got[:4] == got[4:], (length, m)
    finally:
        d.free()


# ---- 3. long tokens --------------------------------------------------------------------------------------------------------
def _long_token(seed, n):
    body = np.random.default_rng(seed).integers(0x21, 0x7F, n, dtype=np.uint8)      # no whitespace: nothing to strip
    return body.tobytes()


def test_one_token_of_a_mebibyte_and_the_threshold_beside_it(gpu, one_token_per_string):
    T = wave_bytes()
    blobs = [b"xy", _long_token(1, T - 1), _long_token(2, 1 << 20), _long_token(3, T), b"", _long_token(4, T + 1), b"ab cd"]
    u8, boff, counts, toks = _check_definition(gpu, blobs, "1 MiB token", dtypes=(np.int64,))
    assert counts.tolist() == [1, 1, 1, 1, 0, 1, 1] and [len(t) for t in toks] == [2, T - 1, 1 << 20, T, T + 1, 5]
    _check_definition(gpu, blobs, "1 MiB token, int32 records", seeds=(1,), dtypes=(np.int32,))


def test_a_mebibyte_token_under_the_built_in_tables(gpu):
    u8, boff, counts, toks = _check_definition(gpu, [b"xy", b"q" * (1 << 20), b"ab cd"], "1 M-char token between strings",
                                               seeds=(0x9747B28C,), dtypes=(np.int64,))
    assert [len(t) for t in toks] == [2, 1 << 20, 2, 2]


def test_a_tile_of_two_rounds_and_a_string_that_began_before_its_tile(gpu):
    """2048 tokens in one 4096-byte tile (two rounds of its wave), then one string over three tiles with long tokens in it"""
    T = wave_bytes()
    blobs = [b"a " * 2048, b" ".join(bytes(97 + (i + j * j) % 26 for j in range(n)) for i, n in enumerate((70, 129, T + 1, 3000, 2 * T, 5000))), b"xy"]
    u8, boff, counts, toks = _check_definition(gpu, blobs, "two rounds")
    assert counts.tolist() == [2048, 6, 1] and [len(t) for t in toks[2048:]] == [70, 129, T + 1, 3000, 2 * T, 5000, 2]


def test_many_long_tokens_meet_in_one_wave(gpu, one_token_per_string):
    rng = random.Random(53)
    T = wave_bytes()
    sizes = [rng.randint(300, 340) for _ in range(40)] + [rng.randint(300, 5000) for _ in range(22)] + [T + 1, 5000]
    assert len(sizes) == 64 and min(sizes) > T
    blobs = [_long_token(100 + i, n) for i, n in enumerate(sizes)]
    blobs[5:5] = [b"short", b"  ", b"", b"tok"]                     # short tokens between them: both forms in one round
    u8, boff, counts, toks = _check_definition(gpu, blobs, "64 long tokens")
    assert sorted(len(t) for t in toks if len(t) > T) == sorted(sizes)


# ---- 4. random content -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _three_sizes(alphabet):
    rng = random.Random(zlib.crc32(alphabet.encode()))
    alpha = ALPHABETS[alphabet]
    return ((random_strings(rng, 200, 0, 12, alpha), "one tile"),                 # (cut below to what fits one tile)
            (random_strings(rng, 3000, 0, 40, alpha), "<= 262144 bytes"),
            (random_strings(rng, 24000, 0, 120, alpha) + ["".join(rng.choice(alpha) for _ in range(150000))], "several hundred tiles"))


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("alphabet", sorted(ALPHABETS))
def test_random_strings_at_three_sizes(gpu, oracle, alphabet, seed):
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
        u8, boff, counts, toks = _check_definition(gpu, blobs, (alphabet, what), seeds=(seed,))
        if total <= 262144:         # built-in tables: the hashed slices are the reference's tokens
            want = [tok.encode("utf-8", "surrogatepass") for t in texts if t != "" for tok in oracle.tokenize(t)]
            assert toks == want, (alphabet, what)


@pytest.mark.parametrize("name", sorted(RULE_SETS))
def test_runtime_rule_tables(gpu, name):
    from latok_amd import batch
    rng = random.Random(77)
    texts = random_strings(rng, 2500, 0, 150, ALPHABETS["mixed"]) + ["   ", "", " a ", "　x　"]
    batch.set_rules(*RULE_SETS[name])
    try:
        _check_definition(gpu, _enc(texts), ("rules", name))
        _check_definition(gpu, _enc(texts[:40]), ("rules small", name))
    finally:
        batch.reset_rules()


@functools.lru_cache(maxsize=2)
def _ssc_content(table, size):
    return [_enc(texts) for texts in ssc.content(table, size, "bytes", "full")]


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("size", ssc.SIZES)
@pytest.mark.parametrize("table", sorted(ssc.TABLES))
def test_tables_that_leave_whitespace_inside_tokens(gpu, table, size, seed):
    """interior whitespace is hashed, only the two ends of a token are stripped; long whitespace in front of, inside and behind tokens"""
    from latok_amd import batch
    batch.set_rules(*ssc.TABLES[table])
    try:
        for i, blobs in enumerate(_ssc_content(table, size)):
            _check_definition(gpu, blobs, (table, size, "ABCD"[i]), seeds=(seed,))
    finally:
        batch.reset_rules()


def test_malformed_bytes_are_hashed_as_they_are(gpu):
    rng = random.Random(5)
    body = _enc(random_strings(rng, 3000, 0, 120, ALPHABETS["mixed"]))
    _check_definition(gpu, body[:1500] + SOFT + body[1500:] + SOFT, "soft malformed")
    _check_definition(gpu, body[:700] + HARD + SOFT + body[700:] + HARD, "hard malformed")
    u8, boff, counts, toks = _check_definition(gpu, SOFT + HARD, "small malformed batch")
    assert b"\xe6\x97" in toks and b"\xc3" in toks and any(b"\x80" in t for t in toks)    # nothing refused, nothing repaired


# ---- 5. protocol -----------------------------------------------------------------------------------------------------------
def test_capacity_protocol_and_optional_outputs(gpu):
    from latok_amd import _lib, batch
    rng = random.Random(9)
    blobs = _enc(random_strings(rng, 900, 0, 90, ALPHABETS["mixed"]))
    u8, boff = batch.pack_utf8(blobs)
    counts, spans = batch.token_spans_utf8_bytes_csr(u8, boff)
    toks = _slices(u8, boff, counts, spans)
    need = len(toks)
    for seed in SEEDS:
        want = np.array([H(seed, t) for t in toks], np.uint32)
        # size query
        rc, n, h, sp, c = _hash_host(gpu, u8, boff, seed, 0, want_hashes=False, want_spans=False)
        assert rc == _lib.ERR_INVALID and n == need and np.array_equal(c, counts)
        # one short: nothing written, counts valid, the needed count returned
        rc, n, h, sp, c = _hash_host(gpu, u8, boff, seed, need - 1)
        assert rc == _lib.ERR_INVALID and "capacity" in _lib.last_error() and n == need
        assert (h == POISON32).all() and (sp == -7).all() and np.array_equal(c, counts)
        # spans_out = NULL, counts_out = NULL, each alone and together; total_bytes = -1 is resolved from byte_off
        for ws, wc in ((False, True), (True, False), (False, False)):
            rc, n, h, sp, c = _hash_host(gpu, u8, boff, seed, need, np.int32, want_spans=ws, want_counts=wc, total=-1)
            assert rc == 0 and n == need and np.array_equal(h[:n], want) and (h[n:] == POISON32).all(), (ws, wc)
            assert np.array_equal(sp[:n], spans) and (sp[n:] == -7).all() if ws else (sp == -7).all()
            assert np.array_equal(c, counts) if wc else (c == -7).all()
            assert gpu.latok_debug_last_route() == HASH_ROUTE
    # hashes_out = NULL with a capacity is refused; so is a stray flag bit
    rc, n, h, sp, c = _hash_host(gpu, u8, boff, 0, need, want_hashes=False)
    assert rc == _lib.ERR_INVALID and "hashes_out" in _lib.last_error() and (sp == -7).all() and (c == -7).all()
    for flag in (4, 64, 1 << 30):
        rc, n, h, sp, c = _hash_host(gpu, u8, boff, 0, need, flags=flag)
        assert rc == _lib.ERR_INVALID and "unknown flag" in _lib.last_error()
        assert (h == POISON32).all() and (sp == -7).all() and (c == -7).all()


def test_device_pointers_equal_host_pointers(gpu):
    from latok_amd import _lib, batch
    rng = random.Random(21)
    blobs = _enc(random_strings(rng, 4000, 0, 200, ALPHABETS["mixed"]))
    u8, boff, counts, toks = _check_definition(gpu, blobs, "host pointers", seeds=(1,), dtypes=(np.int32,))
    spans = batch.token_spans_utf8_bytes_csr(u8, boff, np.int32)[1]
    need = len(toks)
    d = _Dev(gpu, u8.nbytes, boff.size - 1, need)
    try:
        d.load(u8, boff)
        n = C.c_int64(-1)
        flags = _lib.DEVICE_PTRS | _lib.OUT_INT32
        for seed in SEEDS:
            rc = gpu.latok_token_hashes_utf8_bytes_batch(d.u8, d.boff, d.n_str, -1, seed, d.counts, d.spans, d.hashes, need, C.byref(n), flags, None)
            assert rc == 0 and n.value == need, _lib.last_error()
            assert gpu.latok_debug_last_route() == HASH_ROUTE
            h, sp, c, _ = d.read(np.int32)
            assert np.array_equal(h[:need], [H(seed, t) for t in toks]) and (h[need:] == POISON32).all()
            assert np.array_equal(sp[:need], spans) and (sp[need:].view(np.uint8) == POISON).all() and np.array_equal(c, counts)
        # an unaligned device input is refused
        rc = gpu.latok_token_hashes_utf8_bytes_batch(d.u8 + 4, d.boff, d.n_str, int(boff[-1]), 0, d.counts, d.spans, d.hashes, need, C.byref(n),
                                                     flags, None)
        assert rc == _lib.ERR_INVALID and "16-byte aligned" in _lib.last_error()
    finally:
        d.free()


def test_empty_strings_whitespace_and_nothing(gpu):
    from latok_amd import _lib, batch
    body = [b"some text, here", b"more"]
    for blobs in ([b""] * 70 + body + [b""] * 130 + body + [b""] * 70, [b""] * 200 + body, [b""] * 5, [b"", b"x", b""]):
        _check_definition(gpu, blobs, "runs of empty strings")
    ws = [b"   ", b"\t\n", "　　".encode(), b" " * 5000, b""] * 3
    u8, boff, counts, toks = _check_definition(gpu, ws, "all whitespace")
    assert toks == [] and not counts.any()
    # n_str = 0
    rc, n, h, sp, c = _hash_host(gpu, np.zeros(0, np.uint8), np.zeros(1, np.int64), 0, 4)
    assert rc == 0 and n == 0 and (h == POISON32).all() and (sp == -7).all()
    # total_bytes = 0 with strings: counts cleared
    rc, n, h, sp, c = _hash_host(gpu, np.zeros(0, np.uint8), np.zeros(6, np.int64), 0, 4)
    assert rc == 0 and n == 0 and not c.any() and (h == POISON32).all()
    assert batch.token_hashes_utf8_batch([]) == [] and [a.tolist() for a in batch.token_hashes_batch(["", " "])] == [[], []]


# ---- 6. the flow -----------------------------------------------------------------------------------------------------------
def test_flow_batches_alternating_over_two_hash_buffers(gpu):
    from latok_amd import _lib, batch
    rng = random.Random(33)
    batches = [_enc(random_strings(rng, n, 0, hi, ALPHABETS[a])) for n, hi, a in ((3000, 150, "mixed"), (50, 30, "words"), (6000, 90, "bmp"),
                                                                                 (2000, 300, "latin1"))]
    packed = [batch.pack_utf8(b) for b in batches]
    SEED = 0x9747B28C
    want = []
    for u8, boff in packed:
        counts, spans = batch.token_spans_utf8_bytes_csr(u8, boff)
        rc, n, h, sp, c = _hash_host(gpu, u8, boff, SEED, len(spans))
        assert rc == 0 and n == len(spans)
        want.append((n, h[:n].copy(), spans, counts))
    cap = max(w[0] for w in want)
    devs = [_Dev(gpu, u8.nbytes, boff.size - 1, cap) for u8, boff in packed]
    outs = [gpu.latok_dev_alloc((cap + GUARD) * 4) for _ in range(2)]

    def hashes_of(p):
        got = np.empty(cap + GUARD, np.uint32)
        _lib.check(gpu.latok_memcpy_d2h(got.ctypes.data, p, got.nbytes))
        return got

    try:
        for d, (u8, boff) in zip(devs, packed):
            d.load(u8, boff)
        for first in (0, 2):                # two batches in flight at a time, one per hash buffer; nothing waits in between
            pair = devs[first:first + 2]
            for i, d in enumerate(pair):
                total = int(packed[first + i][1][-1])
                batch.flow_token_hashes_utf8_bytes(d.u8, d.boff, d.n_str, total if i else -1, d.counts, d.spans, outs[i], cap, d.res, seed=SEED)
            batch.flow_wait()
            for i, d in enumerate(pair):
                n, wh, wsp, wc = want[first + i]
                _, sp, c, res = d.read()
                assert res.tolist() == [n, 0], (first + i, res)
                assert np.array_equal(sp[:n], wsp) and np.array_equal(c, wc), first + i
                assert np.array_equal(hashes_of(outs[i])[:n], wh), first + i
        # resubmission into the same hash buffer with no wait between: the second result wins
        a, b = devs[0], devs[2]
        batch.flow_token_hashes_utf8_bytes(a.u8, a.boff, a.n_str, int(packed[0][1][-1]), a.counts, a.spans, outs[0], cap, a.res, seed=SEED)
        batch.flow_token_hashes_utf8_bytes(b.u8, b.boff, b.n_str, int(packed[2][1][-1]), b.counts, b.spans, outs[0], cap, b.res, seed=SEED)
        batch.flow_wait()
        assert np.array_equal(hashes_of(outs[0])[:want[2][0]], want[2][1])
        # a batch whose capacity is too small leaves hashes and records untouched and reports the needed count
        d = devs[0]
        d.load(*packed[0])
        _lib.check(gpu.latok_memset_dev(outs[1], POISON, (cap + GUARD) * 4))
        _lib.check(gpu.latok_sync())
        batch.flow_token_hashes_utf8_bytes(d.u8, d.boff, d.n_str, int(packed[0][1][-1]), d.counts, d.spans, outs[1], want[0][0] - 1, d.res, seed=SEED)
        batch.flow_wait()
        _, sp, c, res = d.read()
        assert (hashes_of(outs[1]) == POISON32).all() and (sp.view(np.uint8) == POISON).all()
        assert res.tolist() == [want[0][0], 0] and np.array_equal(c, want[0][3])
        # an "unbounded" capacity works like the exact one; counts and records are optional; int32 records
        batch.flow_token_hashes_utf8_bytes(d.u8, d.boff, d.n_str, int(packed[0][1][-1]), None, None, outs[1], 1 << 62, d.res, seed=SEED, dtype=np.int32)
        batch.flow_wait()
        n = want[0][0]
        got = hashes_of(outs[1])
        assert np.array_equal(got[:n], want[0][1]) and (got[n:] == POISON32).all() and d.read()[3].tolist() == [n, 0]
        # an empty batch in the flow: zero counts, zero total
        e = _Dev(gpu, 0, 3, 4)
        try:
            e.load(np.zeros(0, np.uint8), np.zeros(4, np.int64))
            batch.flow_token_hashes_utf8_bytes(e.u8, e.boff, 3, 0, e.counts, e.spans, e.hashes, 4, e.res)
            batch.flow_wait()
            h, sp, c, res = e.read()
            assert res.tolist() == [0, 0] and not c.any() and (h == POISON32).all()
        finally:
            e.free()
    finally:
        for d in devs:
            d.free()
        for p in outs:
            gpu.latok_dev_free(p)


def test_python_wrappers(gpu, oracle):
    from latok_amd import batch
    rng = random.Random(3)
    texts = random_strings(rng, 500, 0, 80, ALPHABETS["mixed"]) + ["", "   ", "x", "a,b"]
    texts = [t for t in texts if "\ud800" not in t]
    for seed in SEEDS:
        want = [[murmur3_ref(t.encode(), seed) for t in oracle.tokenize(text)] if text != "" else [] for text in texts]
        got = batch.token_hashes_batch(texts, seed=seed)
        assert all(g.dtype == np.uint32 for g in got) and [g.tolist() for g in got] == want
        assert want[-1] == [batch.murmur3_32(t, seed) for t in (b"a", b",", b"b")]
    blobs = _enc(texts + ["\ud800 lone"])
    u8, boff = batch.pack_utf8(blobs)
    counts, hashes, spans = batch.token_hashes_utf8_csr(u8, boff, seed=1, dtype=np.int32, spans=True)
    c2, s2 = batch.token_spans_utf8_bytes_csr(u8, boff, np.int32)
    assert hashes.dtype == np.uint32 and counts.dtype == spans.dtype == np.int32 and np.array_equal(counts, c2) and np.array_equal(spans, s2)
    assert hashes.tolist() == [murmur3_ref(t, 1) for t in _slices(u8, boff, c2, s2)]
    c3, h3 = batch.token_hashes_utf8_csr(u8, boff, seed=1)
    assert c3.dtype == np.int64 and np.array_equal(c3, counts) and np.array_equal(h3, hashes)
    rows = batch.token_hashes_utf8_batch(blobs, 1)
    assert [len(r) for r in rows] == counts.tolist() and np.array_equal(np.concatenate(rows), hashes)


# ---- 7. golden, example ----------------------------------------------------------------------------------------------------
def test_golden_tokens_of_the_real_reference(gpu):
    from latok_amd import batch
    g = json.load(open(os.path.join(GOLDEN, "token_hashes.json")))
    lines, tokens = g["lines"], g["tokens"]
    assert len(lines) == len(tokens) and len(g["hashes"]) == 2
    for seed, rows in g["hashes"].items():
        assert [len(r) for r in rows] == [len(t) for t in tokens]
        got = batch.token_hashes_batch(lines, seed=int(seed))
        assert [r.tolist() for r in got] == rows, seed
        assert rows == [[murmur3_ref(t.encode("utf-8", "surrogatepass"), int(seed)) for t in toks] for toks in tokens]
        for line, row in zip(lines[:20], rows):   # one string per call as well
            assert batch.token_hashes_batch([line], seed=int(seed))[0].tolist() == row


def test_c_example(gpu, tmp_path):
    exe = str(tmp_path / "token_hashes_utf8")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "token_hashes_utf8.c"),
                           "-L" + os.path.join(ROOT, "latok_amd"), "-llatok_hip", "-Wl,-rpath," + os.path.join(ROOT, "latok_amd"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    first = " ".join("%s=%08x/%d" % (t, murmur3_ref(t.encode(), 0), murmur3_ref(t.encode(), 0) & 0x3FFFF)
                     for t in ["This", "is", "a", "#test", "!", "Testing", ",", "Testing", ",", "1", "2", "3"])
    assert lines[0] == "0 (12 tokens): " + first
    assert lines[2] == "2 (0 tokens):" and lines[3] == "3 (0 tokens):"
    assert lines[4].startswith("4 (") and "🤓=" in lines[4]
