"""WordPiece on the device (latok_wordpiece_ids_utf8_bytes_batch, latok_wordpiece_padded_utf8_bytes_batch, include/latok_hip.h).

The result is DEFINED by a call the parity tests already pin and by tests/helpers/wordpiece_ref.py, a plain restatement of the
definition over bytes and one dict: the byte slices latok_token_spans_utf8_bytes_batch reports for string s, each cut by the
reference.  Every batch goes through the C ABI with poisoned guard bands round every output, with host and with device pointers, in
both widths, and is checked in full.  The shapes are the smallest at which the kernels can go wrong; the sizes of a workgroup and of
a scan block come from the library (latok_debug_wordpiece_limits, latok_debug_limits).  Where a case needs a token with chosen
bytes, rule tables that never split make every string one token (its bytes minus the whitespace at both ends)."""
import ctypes as C
import functools
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import ALPHABETS, ROOT, random_strings
from helpers import murmur3_collide as mc
from helpers import span_strip_content as ssc
from helpers import wordpiece_ref as ref
from helpers.murmur3_ref import murmur3_ref

pytestmark = pytest.mark.gpu

POISON = 0xA5
POISON_32 = np.int32(-0x5A5A5A5B)        # 0xA5A5A5A5 as int32
GUARD = 16
IDS_ROUTE, PADDED_ROUTE = 11, 12
ONE_TOKEN_PER_STRING = (ssc._NONE, ssc._NONE, ssc._NONE)
UNK = -1


@functools.lru_cache(maxsize=1)
def limits():
    """(kWpBlock, entries of one scan block, kHashWaveBytes)"""
    from latok_amd import _lib
    lib = _lib.load()
    out = np.zeros(19, np.int64)
    for name in ("latok_debug_wordpiece_limits", "latok_debug_limits"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = C.c_int, [C.c_void_p, C.c_int]
    assert lib.latok_debug_wordpiece_limits(out.ctypes.data, 4) == 4
    block, chunk = int(out[0]), int(out[1])
    assert lib.latok_debug_limits(out.ctypes.data, 19) == 19
    assert 64 <= block <= chunk <= 1 << 16 and out[14] >= 64
    return block, chunk, int(out[14])


@pytest.fixture
def one_token_per_string(gpu):
    from latok_amd import batch
    batch.set_rules(*ONE_TOKEN_PER_STRING)
    yield
    batch.reset_rules()


# ---- the definition --------------------------------------------------------------------------------------------------------
def want_of(u8, boff, words, ids=None, prefix=b"##", max_chars=100, unk=UNK):
    """(indptr, ids, spans[n, 2], n_tokens) by the reference on the slices of the spans call"""
    from latok_amd import batch
    counts, spans = batch.token_spans_utf8_bytes_csr(u8, boff)
    indptr, pids, sp = ref.cut_rows(u8, boff, counts, spans, ref.vocab_dict(words, ids), prefix, max_chars, unk)
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


def _call(lib, u8, boff, wp, cap=0, dt=np.int64, unk=UNK, want_ids=True, want_spans=True, total=None, flags=0, dev=False):
    """one blocking call -> (rc, n_pieces, n_tokens, _Out); dev: everything in device memory, copied back into the _Out"""
    from latok_amd import _lib
    n_str = boff.size - 1
    total = (int(boff[-1]) if n_str > 0 else 0) if total is None else total
    o = _Out(n_str, cap, dt)
    n, n_tok = C.c_int64(-1), C.c_int64(-1)
    flags |= _lib.OUT_INT32 if dt == np.int32 else 0
    handle = wp.handle if wp is not None else None
    if not dev:
        rc = lib.latok_wordpiece_ids_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, n_str, total, handle, unk, o.indptr.ctypes.data,
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
        rc = lib.latok_wordpiece_ids_utf8_bytes_batch(ptrs[0], ptrs[1], n_str, total, handle, unk, ptrs[2], ptrs[3] if want_ids else None,
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


FORMS = ((np.int64, False), (np.int32, False), (np.int64, True), (np.int32, True))   # width of indptr / spans x host / device pointers


def check(lib, blobs, words, ids=None, prefix=b"##", max_chars=100, seed=0, unk=UNK, what="", forms=FORMS[:2]):
    """the whole definition for one batch; returns want = (indptr, ids, spans, n_tokens)"""
    from latok_amd import _lib, batch
    u8, boff = batch.pack_utf8(blobs)
    want = want_of(u8, boff, words, ids, prefix, max_chars, unk)
    need = len(want[1])
    with batch.WordPiece(words, ids=ids, prefix=prefix, max_chars=max_chars, seed=seed) as wp:
        for dt, dev in forms:
            rc, n, n_tok, o = _call(lib, u8, boff, wp, cap=need, dt=dt, unk=unk, dev=dev)
            assert rc == 0, (what, _lib.last_error())
            assert n == need, (what, n, need)
            assert lib.latok_debug_last_route() == IDS_ROUTE or int(boff[-1]) == 0
            _compare((what, dt.__name__, "device" if dev else "host"), o, n_tok, want, dt)
    return want


def _word(i):
    s = bytearray()
    i += 26                                  # at least two letters
    while i:
        s.append(97 + i % 26)
        i //= 26
    return bytes(s)


# ---- 1. alignment: token starts, piece starts and piece lengths at every dword phase ---------------------------------------------
def test_every_phase_of_token_start_piece_start_and_piece_length(gpu, one_token_per_string):
    piece = [bytes([97 + n]) * n for n in range(10)]                       # piece[n]: n bytes, a letter of its own
    words = piece[1:] + [b"##" + p for p in piece[1:]]
    tokens = [piece[a] + piece[b] + (piece[3] if (a + b) % 3 == 0 else b"") for a in range(1, 10) for b in range(1, 10)]
    for shift in range(4):
        blobs = [b" " * ((i + shift) % 4) + t for i, t in enumerate(tokens)]
        for k in range(4):                                                 # the batch's last byte at every phase: it ends the last token
            last = piece[(k - sum(map(len, blobs)) - 1) % 4 + 1]
            want = check(gpu, blobs + [last], words, what=("phases", shift, k), forms=FORMS if shift == k else FORMS[:1])
            assert (sum(map(len, blobs)) + len(last)) % 4 == k and want[1][-1] == words.index(last)
            assert (want[1] != UNK).all() and len(want[1]) > 2 * len(tokens)
            starts = {(int(a) % 4, int(b - a)) for a, b in want[2]}
            assert shift or len(starts) >= 30                              # (string-relative starts: the absolute phases are the shifts')


# ---- 2. every outcome of the cut ---------------------------------------------------------------------------------------------------
def test_every_outcome_of_the_cut(gpu, one_token_per_string):
    words = [b"a", b"##a", b"ab", b"##b", b"##bc", b"abc", b"##x", b"##", b"##y##", b"#", b"###"]
    tokens = [b"a", b"ab", b"abc", b"abcb", b"aa", b"aaaa", b"a" * 7, b"a" * 8, b"x", b"ax", b"abx", b"abq", b"abbq", b"abcbq", b"q",
              b"##x", b"##", b"#", b"###", b"a##", b"ay##", b"a b", b"abcd" * 40]
    want = check(gpu, tokens, words, max_chars=7, what="outcomes", forms=FORMS)
    rows = [want[1][want[0][i]:want[0][i + 1]].tolist() for i in range(len(tokens))]
    assert rows[0] == [0] and rows[1] == [2] and rows[3] == [5, 3]          # one piece; the longest prefix first
    assert rows[6] == [0] + [1] * 6 and rows[7] == [UNK]                    # max_chars pieces; one char more
    assert rows[8] == [UNK] and rows[9] == [0, 6]                           # a word present only as ##x: not at a token's start
    assert rows[10] == [2, 6] and rows[11] == [UNK] and rows[12] == [UNK]   # a miss at the second piece and after two hits
    assert rows[14] == [UNK] and rows[15] == [6] and rows[16] == [7]        # a miss at the first piece; a token that starts with ##
    check(gpu, tokens, words, ids=[5, -3, 7, 0x7FFFFFFF, -0x80000000, 0, 0, 1, 2, 3, 4], unk=-7, seed=0x9747B28C, what="explicit ids")
    check(gpu, tokens, words, max_chars=100, what="max_chars 100")


def test_multi_byte_text(gpu, one_token_per_string):
    e2, e3, e4 = "é".encode(), "日".encode(), "🤓".encode()
    words = [b"h", b"h\xc3", b"\xc3", b"##\xa9", b"##\xc3", e2, b"##" + e2, e3, b"##" + e3, e4, b"##" + e4, b"a", b"##a", b"##\x80"]
    tokens = [b"h" + e2, e2, b"\xc3", b"a\xa9", b"\xa9", b"a\xc3", b"h\xc3", b"a\x80", b"\x80a", b"a" + e3[:2], e4[:3] + b"a", e3 + e2 + e4 + b"a"]
    for m in (1, 2, 5):
        for ch in (b"a", e2, e3, e4):
            tokens += [ch * m, ch * (m + 1), ch * m + b"\x80\x80", b"\x80" + ch * (m - 1) if m > 1 else ch]
        want = check(gpu, tokens, words, max_chars=m, what=("multi-byte", m))
        rows = [want[1][want[0][i]:want[0][i + 1]].tolist() for i in range(len(tokens))]
        assert rows[0] == ([0, words.index(b"##" + e2)] if m >= 2 else [UNK])    # never h\xc3 + \xa9: an end lies at a char start
    assert any(len(r) == 5 for r in rows) and [UNK] in rows


def test_long_tokens(gpu, one_token_per_string):
    block, chunk, wave_bytes = limits()
    words = [b"ab", b"##ab", b"##c"]
    n = wave_bytes // 2 + 20
    tokens = [b"ab" * n, b"ab" * n + b"c", b"ab" * n + b"q", b"q" * (wave_bytes + 5), b"ab" + b"q" * (2 * wave_bytes), b"ab" * 3, b"abq"]
    want = check(gpu, tokens, words, max_chars=1024, what="long tokens", forms=FORMS)
    assert np.diff(want[0]).tolist() == [n, n + 1, 1, 1, 1, 3, 1]
    want = check(gpu, tokens, words, max_chars=100, what="long tokens, more chars than max_chars")
    assert np.diff(want[0]).tolist() == [1, 1, 1, 1, 1, 3, 1]


@pytest.mark.parametrize("seed", [0, 0x9747B28C])
def test_a_crafted_hash_collision_at_a_piece(gpu, one_token_per_string, seed):
    rng = random.Random(seed)
    pairs = []
    for n in (5, 6, 7, 8, 9, 12, 13, 17):
        a = bytes(rng.randrange(0x61, 0x7B) for _ in range(n))
        pairs += [(a, mc.collide(a, seed, w)) for w in mc.positions(n)[:2]]
    if seed == 0:
        pairs += list(mc.KNOWN_WORD_PAIRS)
    assert all(murmur3_ref(a, seed) == murmur3_ref(b, seed) and a != b and len(a) == len(b) for a, b in pairs)
    words = [b"un"] + [a for a, _ in pairs] + [b"##" + a for a, _ in pairs]
    tokens = [b for _, b in pairs] + [b"un" + b for _, b in pairs] + [a for a, _ in pairs] + [b"un" + a for a, _ in pairs]
    want = check(gpu, tokens, words, seed=seed, what="collisions")
    n = len(pairs)
    assert (want[1][:2 * n] == UNK).all() and (want[1][2 * n:] != UNK).all()
    both = [w for p in pairs for w in p]
    want = check(gpu, both + [b"un" + w for w in both], both + [b"##" + w for w in both] + [b"un"], seed=seed, what="both resident")
    assert (want[1] != UNK).all()


def test_the_empty_prefix_and_an_empty_vocabulary(gpu):
    blobs = [b"abc abcd cab dd", b"abab abx xab", b"", b"cabcd"]
    want = check(gpu, blobs, [b"ab", b"c", b"abc", b"d"], prefix=b"", what="empty prefix", forms=FORMS)
    assert want[1].tolist()[:5] == [2, 2, 3, 1, 0]
    want = check(gpu, blobs, [], what="V = 0", forms=FORMS)
    assert (want[1] == UNK).all() and len(want[1]) == want[3] == 8
    check(gpu, blobs, [b"", b"##", b""], what="empty words")


@pytest.mark.parametrize("n_words", [20, 32, 5000])
def test_table_sizes(gpu, n_words):
    rng = random.Random(n_words)
    stems = [_word(i) for i in range(n_words // 2)]
    words = stems + [b"##" + _word(i) for i in range(n_words - len(stems))]
    rng.shuffle(words)
    toks = [rng.choice(stems) + b"".join(_word(rng.randrange(n_words)) for _ in range(rng.randrange(3))) for _ in range(1500)]
    blobs = [b" ".join(toks[i:i + 5]) for i in range(0, len(toks), 5)]
    from latok_amd import batch
    with batch.WordPiece(words) as wp:
        assert wp.info()["n_slots_initial"] == (64 if n_words <= 32 else 16384) and wp.info()["n_words"] == n_words
    want = check(gpu, blobs, words, what=("table", n_words))
    assert (want[1] == UNK).any() and (want[1] != UNK).sum() > 1000


# ---- 3. totals round one scan block, rows of every kind ---------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [-2, -1, 0, 1])
def test_token_and_piece_totals_round_one_scan_block(gpu, delta):
    block, chunk, _ = limits()
    words = [b"a", b"##b", b"c"]
    n = chunk + delta                                                       # (the scans take one entry more than there are tokens)
    one = [b"a"] * n
    # one token per string = one piece per token: tokens, pieces and rows cross the block together; empty runs first and last
    check(gpu, [b"", b"  ", b""] + one[:n // 2] + [b"", b" \t ", b""] + one[n // 2:] + [b" ", b""], words, what=("one per string", n), forms=FORMS[:1])
    # one string holding every token, n_str = 1; two pieces per token: the piece total crosses where the token total does not
    half = [b"ab"] * (n // 2) + [b"c"] * (n % 2)
    want = check(gpu, [b" ".join(half)], words, what=("one string", n), forms=FORMS[1:2])
    assert len(want[1]) == n and want[3] == (n + 1) // 2
    want = check(gpu, [b" ".join([b"ab"] * n)], words, what=("one string, tokens", n), forms=FORMS[:1])
    assert len(want[1]) == 2 * n and want[3] == n
    # a workgroup of the token kernels: the same at its own size
    m = block + delta
    check(gpu, [b"a ab"] * (m // 2) + [b"c"] * (m % 2) + [b"x"], words, what=("workgroup", m), forms=FORMS[:1])


def _rows_round_the_edges(block, total, opens_at, straddles):
    """rows of 1 .. 5 distinct short tokens, `total` tokens in all: a row begins at token `opens_at` behind a run of empty strings, a
    row of five holds token `straddles` as its third, the last row ends on the last token and a run of empty strings ends the batch
    -> (blobs, tokens per string)"""
    cuts, k, i = {0, total, opens_at, straddles - 2, straddles + 3}, 0, 0
    while k < total:
        cuts.add(k)
        k += (1, 3, 2, 5, 1, 4)[i % 6]
        i += 1
    cuts = sorted(c for c in cuts if not straddles - 2 < c < straddles + 3)
    blobs, counts = [], []
    for a, b in zip(cuts, cuts[1:]):
        if a == opens_at:
            blobs += [b"", b" ", b"", b""]
            counts += [0] * 4
        blobs.append(b" ".join(_word(t) for t in range(a, b)))
        counts.append(b - a)
    return blobs + [b"", b"", b" \t", b""], counts + [0] * 4


@pytest.mark.parametrize("opens_at, straddles, short", [(1, 2, 0), (2, 1, 3)])
def test_rows_at_the_edges_of_a_workgroup_of_tokens(gpu, opens_at, straddles, short):
    """The rows that touch a workgroup's tokens, on multi-token rows: about three workgroups of tokens, every token a word of its
    own, so a token read under a wrong row shows in its id and in its string-relative span.  At one edge between two workgroups a
    row begins exactly on the edge, behind empty strings whose row starts lie on it too; at the other a row of five tokens lies
    across it.  A row cannot both begin on an edge and lie across it, so the two layouts swap the edges.  The batch ends with empty
    strings whose row starts are the token total; with `short` = 0 that total is itself an edge (the count kernel's entry behind
    the last token is a workgroup's first)."""
    block = limits()[0]
    total = 3 * block - short
    blobs, counts = _rows_round_the_edges(block, total, opens_at * block, straddles * block)
    starts = np.concatenate(([0], np.cumsum(counts)))
    assert (starts[:-1] == opens_at * block).sum() == 5 and counts[int(np.searchsorted(starts, opens_at * block, "right")) - 1] > 0
    s = int(np.searchsorted(starts, straddles * block, "right")) - 1
    assert counts[s] == 5 and starts[s] == straddles * block - 2
    last = len(counts) - 5
    assert counts[last] > 0 and starts[last] + counts[last] == total and (starts[last + 1:] == total).all() and len(blobs) > 200
    stems = [bytes([c]) for c in range(97, 110)]
    words = [_word(t) for t in range(total) if t % 3] + stems + [b"##" + bytes([c]) for c in range(97, 123)]
    want = check(gpu, blobs, words, what=("edges", opens_at, straddles))
    assert want[3] == total and ((np.diff(want[0]) > 0) == (np.array(counts) > 0)).all()
    assert (want[1] == UNK).any() and len(want[1]) > total                 # whole words, words cut into letters, misses


def test_the_smallest_batches(gpu):
    words = [b"a", b"##b"]
    for blobs in ([b"a"], [b"ab"], [b"x"], [b""], [b" "], [b"", b""], [b"", b"ab", b""], [b"abb ab a"]):
        check(gpu, blobs, words, what=("small", blobs), forms=FORMS)
    from latok_amd import _lib, batch
    with batch.WordPiece(words) as wp:                                      # n_str = 0
        rc, n, n_tok, o = _call(gpu, np.zeros(0, np.uint8), np.zeros(1, np.int64), wp, cap=4)
        assert rc == 0 and n == 0 and n_tok == 0 and o.pieces_untouched() and (o.indptr[1:] == -7).all(), _lib.last_error()


def test_mixed_text_and_malformed_bytes(gpu):
    rng = random.Random(5)
    body = [t.encode("utf-8", "surrogatepass") for t in random_strings(rng, 300, 0, 60, ALPHABETS["mixed"])]
    odd = [b"ab\xe6\x97 cd", b"\xc3 x", b"lone \xf0\x9f\x98", b"end\xe6", b"\xe6\x97\xa5\xe6", b"\xf0", b"x\xc3", b"a\x80\x80\x80\x80b", b"\xa9 cont"]
    from latok_amd import batch
    u8, boff = batch.pack_utf8(body + odd)
    counts, spans = batch.token_spans_utf8_bytes_csr(u8, boff)
    raw, base = u8.tobytes(), np.repeat(boff[:-1], counts)
    toks = list(dict.fromkeys(raw[a:b] for a, b in zip((base + spans[:, 0]).tolist(), (base + spans[:, 1]).tolist())))
    words = [t[:2] for t in toks[::2]] + [b"##" + t[2:] for t in toks[::3] if len(t) > 2] + [b"##" + t[1:2] for t in toks[::5]] + [b"\xc3", b"##\x80"]
    want = check(gpu, body[:150] + odd + body[150:] + odd, words, what="mixed", forms=FORMS)
    assert (want[1] == UNK).any() and len(want[1]) > want[3]


# ---- 4. the calls --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _protocol_batch():
    rng = random.Random(9)
    stems = [_word(i) for i in range(60)]
    words = stems[::2] + [b"##" + w for w in stems[1::3]] + [b"##s"]
    blobs = [b" ".join(rng.choice(stems) + rng.choice([b"", b"s", stems[1], stems[4] + b"s"]) for _ in range(rng.randrange(0, 9))) for _ in range(200)]
    return blobs, words


def test_capacity_protocol_and_refusals(gpu):
    from latok_amd import _lib, batch
    blobs, words = _protocol_batch()
    u8, boff = batch.pack_utf8(blobs)
    want = want_of(u8, boff, words)
    need, n_str = len(want[1]), len(blobs)
    assert need > want[3] > 0
    with batch.WordPiece(words, seed=11) as wp:
        for dev in (False, True):
            # the size query: no id buffer, capacity 0
            rc, n, n_tok, o = _call(gpu, u8, boff, wp, cap=0, want_ids=False, want_spans=False, dev=dev)
            assert rc == _lib.ERR_INVALID and n == need and n_tok == want[3] and np.array_equal(o.indptr[:n_str + 1], want[0])
            # one short: nothing written to ids or spans, indptr valid, the need returned
            rc, n, n_tok, o = _call(gpu, u8, boff, wp, cap=need - 1, dt=np.int32, dev=dev)
            assert rc == _lib.ERR_INVALID and "capacity" in _lib.last_error() and n == need and o.pieces_untouched()
            assert np.array_equal(o.indptr[:n_str + 1], want[0]) and (o.indptr[n_str + 1:] == -7).all()
            # exact, with total_bytes = -1; larger than needed; without spans
            for cap in (need, need + 5):
                rc, n, n_tok, o = _call(gpu, u8, boff, wp, cap=cap, total=-1, dev=dev)
                assert rc == 0 and n == need, _lib.last_error()
                _compare(("capacity", cap, dev), o, n_tok, want, np.int64)
            rc, n, n_tok, o = _call(gpu, u8, boff, wp, cap=need, want_spans=False, dev=dev)
            assert rc == 0 and n == need
            _compare(("no spans", dev), o, n_tok, want, np.int64, has_spans=False)
            assert gpu.latok_debug_last_route() == IDS_ROUTE
        # refused before any device work
        rc, n, n_tok, o = _call(gpu, u8, boff, wp, cap=need, want_ids=False)
        assert rc == _lib.ERR_INVALID and "cap > 0" in _lib.last_error() and o.pieces_untouched() and (o.indptr == -7).all()
        rc, n, n_tok, o = _call(gpu, u8, boff, wp, cap=-1)
        assert rc == _lib.ERR_INVALID and "capacity" in _lib.last_error() and (o.indptr == -7).all()
        for flag in (4, 64, 1 << 30):
            rc, n, n_tok, o = _call(gpu, u8, boff, wp, cap=need, flags=flag)
            assert rc == _lib.ERR_INVALID and "unknown flag" in _lib.last_error() and o.pieces_untouched() and (o.indptr == -7).all()
        rc, n, n_tok, o = _call(gpu, u8, boff, None, cap=need)
        assert rc == _lib.ERR_INVALID and "wp is NULL" in _lib.last_error() and (o.indptr == -7).all()
        o = _Out(n_str, need, np.int64)
        n = C.c_int64(-1)
        rc = gpu.latok_wordpiece_ids_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, n_str, -1, wp.handle, UNK, None, o.ids.ctypes.data, None, need,
                                                      C.byref(n), None, 0, None)
        assert rc == _lib.ERR_INVALID and "indptr_out" in _lib.last_error() and o.pieces_untouched()
        rc = gpu.latok_wordpiece_ids_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, n_str, int(boff[-1]) + 1, wp.handle, UNK, o.indptr.ctypes.data,
                                                      o.ids.ctypes.data, None, need, C.byref(n), None, 0, None)
        assert rc == _lib.ERR_INVALID and o.pieces_untouched()
        # a device UTF-8 pointer that is not 16-byte aligned
        p = gpu.latok_dev_alloc(u8.nbytes + 256)
        q = gpu.latok_dev_alloc(boff.nbytes + (n_str + 1) * 8 + need * 4 + 64)
        try:
            rc = gpu.latok_wordpiece_ids_utf8_bytes_batch(p + 4, q, n_str, int(boff[-1]), wp.handle, UNK, q + boff.nbytes, q + boff.nbytes + (n_str + 1) * 8,
                                                          None, need, C.byref(n), None, _lib.DEVICE_PTRS, None)
            assert rc == _lib.ERR_INVALID and "16-byte aligned" in _lib.last_error()
        finally:
            gpu.latok_dev_free(p)
            gpu.latok_dev_free(q)
    info_args = [None] * 10
    assert gpu.latok_wordpiece_info(None, *info_args) == _lib.ERR_INVALID


def test_info_reports_what_was_built(gpu):
    from latok_amd import batch
    with batch.WordPiece([b"abc", b"##defgh", b"##", b"x", b"abc", b"@@yy"], prefix=b"@@", max_chars=9, seed=77) as wp:
        assert wp.info() == dict(n_words=6, n_slots_initial=64, n_slots_cont=64, max_len_initial=7, max_len_cont=2, prefix=b"@@", max_chars=9,
                                 seed=77, device=wp.info()["device"]) and len(wp) == 6
    with pytest.raises(ValueError):
        wp.info()


def test_a_vocabulary_that_holds_every_token_whole_gives_the_ids_call(gpu):
    from latok_amd import batch
    rng = random.Random(2)
    blobs = [t.encode("utf-8", "surrogatepass") for t in random_strings(rng, 300, 0, 80, ALPHABETS["mixed"])]
    u8, boff = batch.pack_utf8(blobs)
    counts, spans = batch.token_spans_utf8_bytes_csr(u8, boff)
    raw, base = u8.tobytes(), np.repeat(boff[:-1], counts)
    words = list(dict.fromkeys(raw[a:b] for a, b in zip((base + spans[:, 0]).tolist(), (base + spans[:, 1]).tolist())))
    with batch.Vocab(words, seed=3) as vocab, batch.WordPiece(words, max_chars=1024, seed=3) as wp:
        c2, ids2, sp2 = batch.token_ids_utf8_csr(u8, boff, vocab, spans=True)
        indptr, ids, sp = batch.wordpiece_ids_utf8_csr(u8, boff, wp)
    assert np.array_equal(ids, ids2) and (ids != UNK).all() and np.array_equal(sp, sp2) and np.array_equal(sp, spans)
    assert np.array_equal(indptr, np.concatenate([[0], np.cumsum(counts)]))


def test_the_same_call_twice_gives_identical_arrays(gpu):
    from latok_amd import batch
    blobs, words = _protocol_batch()
    u8, boff = batch.pack_utf8(blobs)
    need = len(want_of(u8, boff, words)[1])
    with batch.WordPiece(words) as wp:
        runs = [_call(gpu, u8, boff, wp, cap=need, dt=np.int32) for _ in range(2)]
        other = batch.token_spans_utf8_bytes_csr(u8[:64], np.array([0, 64], np.int64))      # another call in between shares the workspace
        runs.append(_call(gpu, u8, boff, wp, cap=need, dt=np.int32))
    assert other[0].sum() > 0 and all(r[0] == 0 and r[1] == need for r in runs)
    for r in runs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip((r[3].indptr, r[3].ids, r[3].spans), (runs[0][3].indptr, runs[0][3].ids, runs[0][3].spans)))


# ---- 5. the padded form -----------------------------------------------------------------------------------------------------------
def _padded(lib, u8, boff, wp, max_length, special, cls=101, sep=102, pad=0, unk=UNK, dev=False):
    from latok_amd import _lib
    n_str = boff.size - 1
    block = np.full(n_str * max_length + GUARD, POISON_32, np.int32)
    lengths = np.full(n_str + GUARD, POISON_32, np.int32)
    n = C.c_int64(-1)
    total = int(boff[-1]) if n_str else 0
    if not dev:
        rc = lib.latok_wordpiece_padded_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, n_str, total, wp.handle, unk, max_length, int(special), cls, sep,
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
        rc = lib.latok_wordpiece_padded_utf8_bytes_batch(ptrs[0], ptrs[1], n_str, -1, wp.handle, unk, max_length, int(special), cls, sep, pad, ptrs[2],
                                                         ptrs[3], C.byref(n), _lib.DEVICE_PTRS | _lib.OUT_INT32, None)
        for a, p in zip(arrays, ptrs[2:]):
            _lib.check(lib.latok_memcpy_d2h(a.ctypes.data, p, a.nbytes))
    finally:
        for p in ptrs:
            lib.latok_dev_free(p)
    return rc, n.value, block, lengths


def _want_padded(want, max_length, special, cls=101, sep=102, pad=0):
    indptr, ids = want[0], want[1]
    rows, lengths = [], []
    for s in range(len(indptr) - 1):
        body = ids[indptr[s]:indptr[s + 1]].tolist()[:max_length - 2 * special]
        row = ([cls] if special else []) + body + ([sep] if special else [])
        lengths.append(len(row))
        rows.append(row + [pad] * (max_length - len(row)))
    return np.array(rows, np.int32).reshape(len(rows), max_length), np.array(lengths, np.int32)


def test_the_padded_form(gpu):
    from latok_amd import _lib, batch
    words = [b"a", b"##b", b"c"]
    blobs = [b"", b"a", b"ab c", b"ab ab", b"ab ab a", b"ab ab ab", b"  ", b"x ab", b"ab ab ab ab ab c"]   # 0, 1, 3, 4, 5, 6, 0, 3, 11 pieces
    u8, boff = batch.pack_utf8(blobs)
    want = want_of(u8, boff, words)
    assert np.diff(want[0]).tolist() == [0, 1, 3, 4, 5, 6, 0, 3, 11]
    with batch.WordPiece(words) as wp:
        for max_length, special, dev in ((6, True, False), (4, False, False), (7, True, True), (5, False, True), (1, False, False), (3, True, False),
                                         (64, True, False)):
            rc, n, block, lengths = _padded(gpu, u8, boff, wp, max_length, special, pad=-9, dev=dev)
            assert rc == 0 and n == len(want[1]), _lib.last_error()
            assert gpu.latok_debug_last_route() == PADDED_ROUTE
            w_block, w_len = _want_padded(want, max_length, special, pad=-9)
            assert np.array_equal(block[:w_block.size].reshape(w_block.shape), w_block), (max_length, special, dev)
            assert np.array_equal(lengths[:len(blobs)], w_len) and (block[w_block.size:] == POISON_32).all() and (lengths[len(blobs):] == POISON_32).all()
        # refusals: a block too narrow for its specials, a stray flag bit, no vocabulary
        for max_length, special in ((0, False), (2, True), (-1, False)):
            rc, n, block, lengths = _padded(gpu, u8, boff, wp, max_length if max_length > 0 else 1, special)
            rc = gpu.latok_wordpiece_padded_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, len(blobs), -1, wp.handle, UNK, max_length, int(special), 1, 2,
                                                             0, block.ctypes.data, lengths.ctypes.data, None, 0, None)
            assert rc == _lib.ERR_INVALID and "max_length" in _lib.last_error()
        rc = gpu.latok_wordpiece_padded_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, len(blobs), -1, wp.handle, UNK, 8, 1, 1, 2, 0, block.ctypes.data,
                                                         lengths.ctypes.data, None, 8, None)
        assert rc == _lib.ERR_INVALID and "unknown flag" in _lib.last_error()
        # a batch without a byte: rows of specials and padding
        e8, eoff = batch.pack_utf8([b"", b"", b""])
        rc, n, block, lengths = _padded(gpu, e8, eoff, wp, 4, True, pad=7)
        assert rc == 0 and n == 0 and block[:12].tolist() == [101, 102, 7, 7] * 3 and lengths[:3].tolist() == [2, 2, 2]
        rc, n, block, lengths = _padded(gpu, e8, eoff, wp, 2, False, pad=7)
        assert rc == 0 and block[:6].tolist() == [7] * 6 and lengths[:3].tolist() == [0, 0, 0] and (block[6:] == POISON_32).all()
        # the Python wrapper and its attention mask
        ids, mask = batch.wordpiece_encode_utf8_batch(blobs, wp, 6, cls_id=101, sep_id=102, pad_id=0)
        w_block, w_len = _want_padded(want, 6, True)
        assert ids.dtype == mask.dtype == np.int32 and np.array_equal(ids, w_block)
        assert np.array_equal(mask, (np.arange(6)[None, :] < w_len[:, None]).astype(np.int32)) and mask.sum() == w_len.sum()
        ids, mask = batch.wordpiece_encode_utf8_batch(blobs, wp, 4, pad_id=-1)
        assert np.array_equal(ids, _want_padded(want, 4, False, pad=-1)[0]) and mask[0].sum() == 0 and mask[8].sum() == 4
        ids, mask = batch.wordpiece_encode_utf8_batch([], wp, 4)
        assert ids.shape == mask.shape == (0, 4)


# ---- 6. wrappers and the example -------------------------------------------------------------------------------------------------
def test_python_wrappers(gpu, oracle, tmp_path):
    from latok_amd import batch
    rng = random.Random(3)
    texts = [t for t in random_strings(rng, 200, 0, 60, ALPHABETS["mixed"]) + ["", "   ", "x", "unaffable unaff abé"] if "\ud800" not in t]
    tokens = [oracle.tokenize(text) if text != "" else [] for text in texts]
    distinct = list(dict.fromkeys(t for row in tokens for t in row))
    words = ["[UNK]", "un", "##aff", "##able", "a", "##b", "##é"] + [t[:1] for t in distinct[::2]] + ["##" + t[1:] for t in distinct[::2] if len(t) > 1]
    words = list(dict.fromkeys(words))
    d = ref.vocab_dict([w.encode() for w in words])
    indptr, ids, spans = [0], [], []
    for text, row in zip(texts, tokens):
        at, data = 0, text.encode()
        for t in row:
            tb = t.encode()
            at = data.index(tb, at)
            for pid, a, e in ref.cut(tb, d, b"##", 100, 0):
                ids.append(pid)
                spans.append((at + a, at + e))
            at += len(tb)
        indptr.append(len(ids))
    path = tmp_path / "vocab.txt"
    path.write_bytes("\n".join(words).encode() + b"\n")
    with batch.WordPiece.from_vocab_file(str(path)) as wp:
        assert len(wp) == len(words)
        got = batch.wordpiece_ids_batch(texts, wp, unk_id=0)
        assert [g.dtype for g in got] == [np.int64, np.int32, np.int64]
        assert got[0].tolist() == indptr and got[1].tolist() == ids and got[2].tolist() == [list(s) for s in spans]
        blobs = [t.encode() for t in texts]
        got_b = batch.wordpiece_ids_utf8_batch(blobs, wp, unk_id=0)
        assert all(np.array_equal(a, b) for a, b in zip(got, got_b))
        u8, boff = batch.pack_utf8(blobs)
        got32 = batch.wordpiece_ids_utf8_csr(u8, boff, wp, unk_id=0, dtype=np.int32)
        assert got32[0].dtype == got32[2].dtype == np.int32 and all(np.array_equal(a, b) for a, b in zip(got, got32))
        assert batch.wordpiece_ids_utf8_csr(u8, boff, wp, spans=False)[2] is None
        empty = batch.wordpiece_ids_utf8_batch([], wp)
        assert empty[0].tolist() == [0] and len(empty[1]) == 0 and empty[2].shape == (0, 2)
        row = got[1][got[0][-2]:got[0][-1]].tolist()
        assert [words[i] for i in row[:5]] == ["un", "##aff", "##able", "un", "##aff"] and len(got[1]) > int(sum(map(len, tokens)))
    with pytest.raises(ValueError):
        batch.wordpiece_ids_batch(texts, wp)                      # closed


def test_c_example(gpu, tmp_path):
    exe = str(tmp_path / "wordpiece_utf8")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "wordpiece_utf8.c"),
                           "-L" + os.path.join(ROOT, "latok_amd"), "-llatok_hip", "-Wl,-rpath," + os.path.join(ROOT, "latok_amd"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0] == "10 tokens, 16 pieces", lines[0]
    assert lines[1] == "  row 0: this[0,4) is[5,7) un[8,10) ##aff[10,13) ##able[13,17) ![18,19)"
    assert lines[2] == "  row 1: test[0,4) ##s[4,5) test[6,10) ##ing[10,13) un[14,16) ##aff[16,19) ##ing[19,22)"
    assert lines[3] == "  row 2:" and lines[4] == "  row 3:" and lines[5] == "  row 4: a[0,1) [UNK][2,11) a[12,13)"
    assert lines[6] == "  input_ids 0 (8 used): 2 11 10 4 5 6 12 3 0 0 0 0"
    assert lines[7] == "  input_ids 1 (9 used): 2 8 13 8 7 4 5 7 3 0 0 0"
    assert lines[8] == "  input_ids 2 (2 used): 2 3 0 0 0 0 0 0 0 0 0 0" and lines[10] == "  input_ids 4 (5 used): 2 9 1 9 3 0 0 0 0 0 0 0"
