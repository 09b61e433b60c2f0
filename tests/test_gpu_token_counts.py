"""Token counting on the device (include/latok_hip.h: latok_counter_*, latok_count_tokens_utf8_bytes_batch; batch.TokenCounter).
The oracle of every case is collections.Counter over the byte slices token_spans_utf8_bytes_csr reports; slices of more than
max_word_bytes bytes are counted as `long`.  Counters are compared as dicts, no word may be listed twice, and
tokens == counted + long + dropped is asserted after every update."""
import collections
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

COUNT_ROUTE = 8
TILE = 4096
ONE_TOKEN_PER_STRING = (ssc._NONE, ssc._NONE, ssc._NONE)      # no rule holds anywhere: the only boundary is the string's start
SOFT = [b"ab\xe6\x97 cd", b"\xc3 x", b"lone \xf0\x9f\x98", b"end\xe6", b"next starts ascii", b"\xe6\x97\xa5\xe6", b"\xf0", b"x\xc3"]
HARD = [b"a\x80\x80\x80\x80b", b"\xa9 starts with a continuation byte"]
LETTERS = b"abcdefghijklmnopqrstuvwxyz"


def acc_entries():
    """kCountAccEntries: entry 18 of latok_debug_limits"""
    from latok_amd import _lib
    fn = _lib.load().latok_debug_limits
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    out = np.zeros(19, np.int64)
    assert fn(out.ctypes.data, 19) == 19
    return int(out[18])


def _enc(texts):
    return [t.encode("utf-8", "surrogatepass") for t in texts]


def _tokens(blobs):
    """the byte slices the records of the spans call name"""
    from latok_amd import batch
    u8, boff = batch.pack_utf8(blobs)
    if u8.size == 0:
        return []
    counts, spans = batch.token_spans_utf8_bytes_csr(u8, boff)
    raw = u8.tobytes()
    base = np.repeat(boff[:-1], counts.astype(np.int64))
    return [raw[a:b] for a, b in zip((base + spans[:, 0]).tolist(), (base + spans[:, 1]).tolist())]


def _oracle(blobs, max_word_bytes=256):
    """-> (Counter of the tokens of at most max_word_bytes bytes, tokens, long)"""
    toks = _tokens(blobs)
    return collections.Counter(t for t in toks if len(t) <= max_word_bytes), len(toks), sum(len(t) > max_word_bytes for t in toks)


def _held(tc):
    """the counter as a dict; a word listed twice fails"""
    words, counts = tc.items()
    assert counts.dtype == np.uint64 and len(words) == len(counts)
    assert len(set(words)) == len(words), "a word sits in two slots"
    return dict(zip(words, map(int, counts)))


def _identity(st):
    assert st["tokens"] == st["counted"] + st["long"] + st["dropped"], st
    return st


def _exact(tc, want, tokens, long_, what=None):
    st = _identity(tc.stats)
    assert st["dropped"] == 0 and st["tokens"] == tokens and st["long"] == long_ and st["counted"] == sum(want.values()), (what, st)
    got = _held(tc)
    if got != dict(want):
        bad = [(w[:40], got.get(w), want.get(w)) for w in set(got) | set(want) if got.get(w) != want.get(w)]
        raise AssertionError((what, len(got), len(want), bad[:5]))
    assert st["distinct"] == len(want)


def _state(lib, tc):
    from latok_amd import _lib
    fn = lib.latok_debug_counter_state
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p]
    out = np.zeros(4, np.int64)
    _lib.check(fn(tc.handle, out.ctypes.data))
    return dict(zip(("blob_dwords", "used_dwords", "grown", "failed"), map(int, out)))


class _DevText:
    """a device copy of a batch: 16-byte aligned bytes (with room behind them) and the byte offsets"""

    def __init__(self, lib, max_bytes, max_str):
        self.lib, self.sizes = lib, (max_bytes + 256, (max_str + 1) * 8)
        self.u8, self.boff = (lib.latok_dev_alloc(s) for s in self.sizes)
        assert self.u8 and self.boff and self.u8 % 16 == 0

    def load(self, blobs, fill=0):
        from latok_amd import _lib, batch
        u8, boff = batch.pack_utf8(blobs)
        assert u8.nbytes + 256 <= self.sizes[0] and boff.nbytes <= self.sizes[1]
        _lib.check(self.lib.latok_memset_dev(self.u8, fill, self.sizes[0]))        # (whatever the batch before left is gone)
        if u8.nbytes:
            _lib.check(self.lib.latok_memcpy_h2d(self.u8, u8.ctypes.data, u8.nbytes))
        _lib.check(self.lib.latok_memcpy_h2d(self.boff, boff.ctypes.data, boff.nbytes))
        _lib.check(self.lib.latok_sync())
        return boff.size - 1

    def count(self, tc, n_str, total=-1, offset=0):
        st = np.full(4, -7, np.int64)
        rc = self.lib.latok_count_tokens_utf8_bytes_batch(self.u8 + offset, self.boff, n_str, total, tc.handle, st.ctypes.data, 1, None)
        return rc, dict(zip(tc.STATS[:4], map(int, st)))

    def free(self):
        self.lib.latok_dev_free(self.u8)
        self.lib.latok_dev_free(self.boff)


def _both_ways(gpu, blobs, what, max_word_bytes=256, seed=0, dev=None):
    """the definition for one batch: host pointers (TokenCounter.update_utf8) and device pointers with total_bytes = -1"""
    from latok_amd import _lib, batch
    want, tokens, long_ = _oracle(blobs, max_word_bytes)
    own = dev is None
    if own:
        dev = _DevText(gpu, sum(map(len, blobs)), len(blobs))
    try:
        with batch.TokenCounter(max(len(want), 1), max_word_bytes, seed) as tc:
            assert tc.n_slots >= max(64, 2 * len(want)) and tc.n_slots & (tc.n_slots - 1) == 0
            st = _identity(tc.update_utf8(blobs))
            assert gpu.latok_debug_last_route() == COUNT_ROUTE or tokens == 0
            assert st == dict(tokens=tokens, counted=sum(want.values()), long=long_, dropped=0), (what, st)
            _exact(tc, want, tokens, long_, (what, "host"))
            tc.clear()
            assert tc.stats == dict.fromkeys(tc.STATS, 0) and _held(tc) == {}
            rc, st = dev.count(tc, dev.load(blobs))
            assert rc == 0, _lib.last_error()
            assert st == dict(tokens=tokens, counted=sum(want.values()), long=long_, dropped=0), (what, st)
            _exact(tc, want, tokens, long_, (what, "device"))
    finally:
        if own:
            dev.free()
    return want


# ---- 1. the definition -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alphabet", sorted(ALPHABETS))
def test_random_strings_are_counted_as_a_counter_counts_them(gpu, alphabet):
    rng = random.Random(zlib.crc32(alphabet.encode()))
    texts = random_strings(rng, 300, 0, 120, ALPHABETS[alphabet]) + ["", "   ", "x", "a,b"]
    want = _both_ways(gpu, _enc(texts), alphabet, seed=rng.getrandbits(32))
    assert len(want) > 10


@pytest.mark.parametrize("name", sorted(RULE_SETS))
def test_runtime_rule_tables(gpu, name):
    from latok_amd import batch
    rng = random.Random(77)
    texts = random_strings(rng, 300, 0, 150, ALPHABETS["mixed"]) + ["   ", "", " a ", "　x　"]
    batch.set_rules(*RULE_SETS[name])
    try:
        _both_ways(gpu, _enc(texts), ("rules", name))
    finally:
        batch.reset_rules()


def test_malformed_bytes_are_counted_as_they_are(gpu):
    rng = random.Random(5)
    body = _enc(random_strings(rng, 300, 0, 120, ALPHABETS["mixed"]))
    _both_ways(gpu, body[:150] + SOFT + body[150:] + SOFT, "soft malformed")
    _both_ways(gpu, body[:70] + HARD + SOFT + body[70:] + HARD, "hard malformed")
    want = _both_ways(gpu, SOFT + HARD, "small malformed batch")
    assert want[b"\xe6\x97"] >= 1 and want[b"\xc3"] >= 1 and any(b"\x80" in t for t in want)      # nothing refused, nothing repaired


# ---- 2. races on claims ----------------------------------------------------------------------------------------------------
def _word(i, n=7):
    out = bytearray()
    for _ in range(n):
        out.append(LETTERS[i % 26])
        i //= 26
    return bytes(out)


def test_every_workgroup_first_claims_the_same_words_at_once(gpu):
    """256 KiB = 64 tiles = 16 workgroups; 512 distinct 7-letter words, every tile holds all of them in another rotation"""
    from latok_amd import batch
    words = [_word(i * 7919 + 13) for i in range(512)]
    assert len(set(words)) == 512
    blobs = []
    for t in range(64):
        r = (t * 37) % 512
        blobs.append(b"".join(w + b" " for w in words[r:] + words[:r]))
    assert sum(map(len, blobs)) == 64 * TILE == 256 << 10
    want, tokens, long_ = _oracle(blobs)
    assert want == collections.Counter(dict.fromkeys(words, 64))
    for seed in (0, 1, 2):                       # three tables, three layouts
        with batch.TokenCounter(512, seed=seed) as tc:
            _identity(tc.update_utf8(blobs))
            _exact(tc, want, tokens, long_, ("claims", seed))
            _identity(tc.update_utf8(blobs))     # and once more, every word resident
            _exact(tc, collections.Counter(dict.fromkeys(words, 128)), 2 * tokens, 0, ("claims again", seed))


# ---- 3. hot words and the accumulator --------------------------------------------------------------------------------------
def test_one_hot_word(gpu):
    from latok_amd import batch
    blobs = [b"a " * (128 << 10)]
    with batch.TokenCounter(16) as tc:
        st = _identity(tc.update_utf8(blobs))
        assert st == dict(tokens=131072, counted=131072, long=0, dropped=0)
        assert _held(tc) == {b"a": 131072} and tc.stats["distinct"] == 1
        assert tc.most_common() == [(b"a", 131072)]


def test_more_distinct_words_in_a_tile_than_the_accumulator_has_entries(gpu):
    """every tile: 676 two-letter words, each twice, in two rounds of the tile's wave -- conflicts in the accumulator and flushes"""
    from latok_amd import batch
    entries = acc_entries()
    words = [bytes([a, b]) for a in LETTERS for b in LETTERS]
    assert len(words) > entries, "the accumulator outgrew this test's tiles: use more distinct words per tile"
    tile = b"".join(w + b" " for w in words + words[::-1])
    assert len(tile) <= TILE
    tile += b" " * (TILE - len(tile))
    blobs = [tile] * 8 + [tile[:999]]
    want, tokens, long_ = _oracle(blobs)
    assert len(want) == 676 and min(want.values()) >= 16
    with batch.TokenCounter(676, seed=4) as tc:
        _identity(tc.update_utf8(blobs))
        _exact(tc, want, tokens, long_, "accumulator")


# ---- 4. crafted collisions -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _pairs():
    pairs = list(mc.KNOWN_WORD_PAIRS) + mc.word_pairs(0)
    assert len(pairs) >= 3 and all(murmur3_ref(a, 0) == murmur3_ref(b, 0) and a != b and len(a) == len(b) for a, b in pairs)
    return pairs


@pytest.mark.parametrize("order", ["ab", "ba"])
def test_crafted_collisions_get_two_entries_with_their_own_counts(gpu, order):
    from latok_amd import batch
    pairs = [p if order == "ab" else p[::-1] for p in _pairs()]
    # one batch: first word 3 times, second 5 times, interleaved behind the first occurrence of each
    blob = b" ".join(b" ".join([a, b, a, b, b, a, b, b]) for a, b in pairs)
    want = collections.Counter()
    for a, b in pairs:
        want[a] += 3
        want[b] += 5
    assert _oracle([blob])[0] == want
    with batch.TokenCounter(64, seed=0) as tc:
        tc.update_utf8([blob])
        _exact(tc, want, sum(want.values()), 0, ("one batch", order))
    # two updates: the first word is resident when the second arrives fresh
    with batch.TokenCounter(64, seed=0) as tc:
        tc.update_utf8([b" ".join(a for a, _ in pairs)] * 3)
        tc.update_utf8([b" ".join(b for _, b in pairs)] * 5)
        _exact(tc, want, sum(want.values()), 0, ("two updates", order))


# ---- 5. accumulation over updates ------------------------------------------------------------------------------------------
def test_updates_add_up_and_the_counter_keeps_no_pointer_into_the_text(gpu):
    from latok_amd import _lib, batch
    rng = random.Random(11)
    long_words = [bytes(rng.choice(LETTERS) for _ in range(rng.randint(12, 40))) for _ in range(1500)]
    A = [b" ".join(rng.choices(long_words[:1000], k=30)) for _ in range(200)]
    B = [b" ".join(rng.choices(long_words[500:], k=30)) for _ in range(200)] + A[:50]
    wa, ta, _ = _oracle(A)
    wb, tb, _ = _oracle(B)
    assert len(set(wa) & set(wb)) > 300 and len(set(wb) - set(wa)) > 300
    dev = _DevText(gpu, max(sum(map(len, A)), sum(map(len, B))), max(len(A), len(B)))
    try:
        with batch.TokenCounter(2048, seed=9) as tc:
            s0 = _state(gpu, tc)
            assert s0["grown"] == 0 and s0["used_dwords"] == 1 and s0["blob_dwords"] < sum((len(w) + 3) // 4 for w in wa)
            rc, st = dev.count(tc, dev.load(A))
            assert rc == 0, _lib.last_error()
            s1 = _state(gpu, tc)
            assert s1["grown"] >= 1 and s1["used_dwords"] == 1 + sum((len(w) + 3) // 4 for w in wa) <= s1["blob_dwords"]
            _exact(tc, wa, ta, 0, "A")
            # A's arrays are overwritten: 0xFF everywhere, then B in the same memory
            rc, st = dev.count(tc, dev.load(B, fill=0xFF))
            assert rc == 0, _lib.last_error()
            assert _identity(st)["tokens"] == tb
            _exact(tc, wa + wb, ta + tb, 0, "A + B")
            s2 = _state(gpu, tc)
            assert s2["used_dwords"] == 1 + sum((len(w) + 3) // 4 for w in set(wa) | set(wb))      # A's words were found, not entered again
            # host arrays likewise
            u8, boff = batch.pack_utf8(A)
            u8 = u8.copy()
            tc.update_utf8_csr(u8, boff)
            u8[:] = 0x20
            tc.update_utf8_csr(u8, boff)         # whitespace only: no token
            _exact(tc, wa + wb + wa, 2 * ta + tb, 0, "A + B + A")
    finally:
        dev.free()


# ---- 6. lengths ------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("max_word_bytes", [256, 5])
def test_every_length_at_four_start_phases(gpu, one_token_per_string, max_word_bytes):
    """tokens of 1 .. max_word_bytes + 1 bytes, each at the four start phases; the batch ends with a token's last byte"""
    rng = random.Random(max_word_bytes)
    blobs, pos = [], 0
    for n in range(1, max_word_bytes + 2):
        tok = _token(rng, n)
        for phase in range(4):
            gap = (phase - pos) % 4
            if gap:
                blobs.append(b" " * gap)         # a whitespace-only string: no token
                pos += gap
            assert pos % 4 == phase
            blobs.append(tok)
            pos += n
    for tail in (0, 1, 2, 3):                    # total_bytes = 0 .. 3 (mod 4), the last byte a token's
        last = b"!" * ((tail - pos - 1) % 4 + 1)
        assert (pos + len(last)) % 4 == tail
        want = _both_ways(gpu, blobs + [last], ("lengths", max_word_bytes, tail), max_word_bytes, seed=tail)
        assert sum(c == 4 for c in want.values()) >= max_word_bytes - 2 and max(map(len, want)) == max_word_bytes


def test_a_token_of_one_mebibyte_is_long_and_its_neighbours_are_counted(gpu, one_token_per_string):
    from latok_amd import batch
    big = np.random.default_rng(1).integers(0x21, 0x7F, 1 << 20, dtype=np.uint8).tobytes()      # no whitespace
    blobs = [b"before", b"  ", big, b"after", b"before"]
    with batch.TokenCounter(16, seed=2) as tc:
        st = _identity(tc.update_utf8(blobs))
        assert st == dict(tokens=4, counted=3, long=1, dropped=0)
        assert _held(tc) == {b"before": 2, b"after": 1}


# ---- 7. too small a table --------------------------------------------------------------------------------------------------
def test_a_table_too_small_drops_and_says_so(gpu):
    from latok_amd import batch
    words = [_word(i * 104729 + 7, 6) for i in range(1000)]
    assert len(set(words)) == 1000
    blobs = [b" ".join(words[i::10] * 3) for i in range(10)]
    want, tokens, _ = _oracle(blobs)
    assert want == collections.Counter(dict.fromkeys(words, 3))
    with batch.TokenCounter(4) as tc:
        assert tc.n_slots == 64
        st = _identity(tc.update_utf8(blobs))                 # the call returns
        assert st["tokens"] == tokens == 3000 and st["dropped"] > 0 and st["long"] == 0
        held = _held(tc)
        assert 0 < len(held) <= 64 and tc.stats["distinct"] == len(held)
        assert all(w in want and 0 < c <= want[w] for w, c in held.items())
        assert sum(held.values()) == st["counted"]
        tc.clear()
        fit = [b" ".join(words[:30] * 2)]
        tc.update_utf8(fit)
        _exact(tc, collections.Counter(dict.fromkeys(words[:30], 2)), 60, 0, "after clear")


# ---- 8. corpus -> vocabulary -> ids ----------------------------------------------------------------------------------------
def test_round_trip_through_a_vocabulary(gpu):
    from latok_amd import batch
    rng = random.Random(21)
    blobs = _enc(random_strings(rng, 400, 0, 100, ALPHABETS["words"]))
    want, tokens, _ = _oracle(blobs)
    with batch.TokenCounter(len(want)) as tc:
        tc.update_utf8(blobs)
        ranked = tc.most_common()
        assert ranked == sorted(want.items(), key=lambda wc: (-wc[1], wc[0]))
        assert tc.most_common(5) == ranked[:5] and tc.most_common(0) == []
        rank = {w: i for i, (w, _) in enumerate(ranked)}
        with tc.to_vocab() as vocab:
            assert len(vocab) == len(ranked)
            rows = batch.token_ids_utf8_batch(blobs, vocab, unk_id=-1)
            ids = np.concatenate(rows)
            assert ids.size == tokens and (ids != -1).all()
            assert ids.tolist() == [rank[t] for t in _tokens(blobs)]
        with tc.to_vocab(min_count=2, max_size=50, seed=3) as small:
            kept = [w for w, c in ranked[:50] if c >= 2]
            assert len(small) == len(kept) > 0
            ids = np.concatenate(batch.token_ids_utf8_batch(blobs, small, unk_id=-9)).tolist()
            assert ids == [rank[t] if t in kept else -9 for t in _tokens(blobs)]


# ---- 9. protocol and arguments ---------------------------------------------------------------------------------------------
def _read(lib, tc, bytes_cap, cap, guard=16):
    words = np.full(bytes_cap + guard, 0xA5, np.uint8)
    off = np.full(cap + 1 + guard, -7, np.int64)
    counts = np.full(cap + guard, 0xA5A5A5A5A5A5A5A5, np.uint64)
    n, nb = C.c_int64(-1), C.c_int64(-1)
    rc = lib.latok_counter_read(tc.handle, words.ctypes.data if bytes_cap else None, bytes_cap, off.ctypes.data if cap else None,
                                counts.ctypes.data if cap else None, cap, C.byref(n), C.byref(nb))
    return rc, n.value, nb.value, words, off, counts


def test_capacity_protocol_of_the_read(gpu):
    from latok_amd import _lib, batch
    blobs = [b"one two three two three three", b"  ", b"four"]
    want = {b"one": 1, b"two": 2, b"three": 3, b"four": 1}
    with batch.TokenCounter(8) as tc:
        rc, n, nb, *_ = _read(gpu, tc, 0, 0)
        assert (rc, n, nb) == (0, 0, 0)                                        # empty: the size query succeeds
        tc.update_utf8(blobs)
        rc, n, nb, *_ = _read(gpu, tc, 0, 0)                                   # the size query
        assert rc == _lib.ERR_INVALID and (n, nb) == (4, 15) and "4 words" in _lib.last_error()
        for bytes_cap, cap in ((15, 3), (14, 4), (0, 4), (15, 0)):             # either capacity too small: nothing written
            rc, n, nb, words, off, counts = _read(gpu, tc, bytes_cap, cap)
            assert rc == _lib.ERR_INVALID and (n, nb) == (4, 15), (bytes_cap, cap)
            assert (words == 0xA5).all() and (off == -7).all() and (counts == 0xA5A5A5A5A5A5A5A5).all(), (bytes_cap, cap)
        for bytes_cap, cap in ((15, 4), (40, 9)):                              # the exact fit, and room to spare
            rc, n, nb, words, off, counts = _read(gpu, tc, bytes_cap, cap)
            assert rc == 0 and (n, nb) == (4, 15), _lib.last_error()
            assert off[0] == 0 and off[4] == 15 and (np.diff(off[:5]) > 0).all()
            raw = words.tobytes()
            assert {raw[off[i]:off[i + 1]]: int(counts[i]) for i in range(4)} == want
            assert (words[15:] == 0xA5).all() and (off[5:] == -7).all() and (counts[4:] == 0xA5A5A5A5A5A5A5A5).all()
        # what it wrote is what latok_vocab_create takes
        h = C.c_void_p()
        _lib.check(gpu.latok_vocab_create(words.ctypes.data, off.ctypes.data, 4, None, 0, C.byref(h)))
        _lib.check(gpu.latok_vocab_destroy(h))


def test_arguments_states_and_contexts(gpu):
    from latok_amd import _lib, batch
    blobs = [b"x yy zzz", b"yy"]
    want = collections.Counter({b"x": 1, b"yy": 2, b"zzz": 1})
    fail = gpu.latok_debug_counter_fail
    fail.restype, fail.argtypes = C.c_int, [C.c_void_p]
    dev = _DevText(gpu, 64, 4)
    try:
        with batch.TokenCounter(8, max_word_bytes=2, seed=0xFFFFFFFF) as tc:
            info = (C.c_int64(), C.c_int64(), C.c_int(), C.c_uint32(), C.c_int())
            _lib.check(gpu.latok_counter_info(tc.handle, *map(C.byref, info), None))
            assert [v.value for v in info[:4]] == [8, 64, 2, 0xFFFFFFFF] and info[4].value >= 0
            n_str = dev.load(blobs)
            # refused before anything happens: stray flags, a misaligned device pointer, a total that is not the offsets'
            st = np.full(4, -7, np.int64)
            for flags in (2, 3, 4):
                assert gpu.latok_count_tokens_utf8_bytes_batch(dev.u8, dev.boff, n_str, -1, tc.handle, st.ctypes.data, flags, None) == _lib.ERR_INVALID
            rc, _ = dev.count(tc, n_str, offset=4)
            assert rc == _lib.ERR_INVALID and "aligned" in _lib.last_error()
            with pytest.raises(ValueError):
                u8, boff = batch.pack_utf8(blobs)
                _lib.check(gpu.latok_count_tokens_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, 2, 5, tc.handle, None, 0, None))
            assert tc.stats == dict.fromkeys(tc.STATS, 0)
            # no string / no byte: untouched, the call's stats zeroed
            for n, total in ((0, 0), (2, 0)):
                empty = np.zeros(3, np.int64)
                st[:] = -7
                _lib.check(gpu.latok_count_tokens_utf8_bytes_batch(None, empty.ctypes.data, n, total, tc.handle, st.ctypes.data, 0, None))
                assert (st == 0).all() and tc.stats == dict.fromkeys(tc.STATS, 0)
            assert tc.update_utf8([]) == dict(tokens=0, counted=0, long=0, dropped=0) == tc.update(["", "  "])
            # max_word_bytes = 2: "zzz" is long
            rc, st1 = dev.count(tc, n_str)
            assert rc == 0 and st1 == dict(tokens=4, counted=3, long=1, dropped=0) and _held(tc) == {b"x": 1, b"yy": 2}
            # a second context of the same device shares the counter
            ctx = _lib.Context(info[4].value)
            try:
                with ctx:
                    tc.update_utf8(blobs)
                    assert _held(tc) == {b"x": 2, b"yy": 4}
            finally:
                ctx.destroy()
            if gpu.latok_device_count() > 1:      # a context of another device is refused
                other = _lib.Context((info[4].value + 1) % gpu.latok_device_count())
                try:
                    with other:
                        with pytest.raises(ValueError, match="device"):
                            tc.update_utf8(blobs)
                finally:
                    other.destroy()
            # the failed state: everything but info, clear and destroy is refused, nothing is counted
            before = tc.stats
            _lib.check(fail(tc.handle))
            assert _state(gpu, tc)["failed"] == 1
            for call in (lambda: tc.update_utf8(blobs), lambda: tc.items(), lambda: _lib.check(dev.count(tc, n_str)[0])):
                with pytest.raises(ValueError, match="failed state"):
                    call()
            assert tc.stats == before
            tc.clear()
            assert _state(gpu, tc)["failed"] == 0 and tc.stats == dict.fromkeys(tc.STATS, 0)
            tc.update_utf8(blobs)
            assert _held(tc) == {b"x": 1, b"yy": 2}
        assert tc.handle is None
        with pytest.raises(ValueError):
            tc.update_utf8(blobs)
        tc.close()
    finally:
        dev.free()
    with batch.TokenCounter(8) as tc:             # and with the default 256 bytes the whole batch
        tc.update_utf8(blobs)
        assert _held(tc) == dict(want)


# ---- 10. the wrappers and the example --------------------------------------------------------------------------------------
def test_python_wrappers(gpu, oracle):
    from latok_amd import batch
    rng = random.Random(3)
    texts = [t for t in random_strings(rng, 300, 0, 80, ALPHABETS["mixed"]) + ["", "   ", "x", "a,b"] if "\ud800" not in t]
    want = collections.Counter(t.encode() for text in texts if text != "" for t in oracle.tokenize(text))
    with batch.TokenCounter(len(want), seed=6) as tc:
        st = tc.update(texts)
        assert st["tokens"] == sum(want.values()) and _held(tc) == dict(want)
        assert tc.most_common(3) == sorted(want.items(), key=lambda wc: (-wc[1], wc[0]))[:3]
    got = batch.count_tokens_utf8_batch(_enc(texts))
    assert isinstance(got, collections.Counter) and got == want
    assert batch.count_tokens_utf8_batch(_enc(texts), max_words=len(want)) == want
    assert batch.count_tokens_utf8_batch([]) == collections.Counter() == batch.count_tokens_utf8_batch([b"", b"  "])
    # the host path it replaces gives the same counter
    assert collections.Counter(t for row in batch.tokenize_utf8_batch(_enc(texts)) for t in row) == want


def test_c_example(gpu, tmp_path):
    exe = str(tmp_path / "count_tokens_utf8")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "count_tokens_utf8.c"),
                           "-L" + os.path.join(ROOT, "latok_amd"), "-llatok_hip", "-Wl,-rpath," + os.path.join(ROOT, "latok_amd"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0] == "this batch: 21 tokens, 21 counted, 0 long, 0 dropped"
    words = dict(line.rsplit(" x", 1) for line in lines[1:-5])
    assert words == {"This": "1", "is": "2", "a": "4", "#test": "1", "!": "1", "Testing": "2", ",": "2", "1": "1", "2": "1", "3": "1", "this": "1",
                     "not": "1", "test": "1", "日本語": "1", "🤓": "1"}
    order = [line.rsplit(" x", 1)[0] for line in lines[1:-5]]
    ids = [[int(x) for x in line.split(":")[1].split()] for line in lines[-5:]]
    assert [[order[i] for i in row] for row in ids] == [["This", "is", "a", "#test", "!", "Testing", ",", "Testing", ",", "1", "2", "3"],
                                                        ["this", "is", "not", "a", "test"], [], [], ["a", "日本語", "🤓", "a"]]
