"""Unigram on the device (latok_unigram_ids_utf8_bytes_batch, latok_unigram_padded_utf8_bytes_batch, include/latok_hip.h).

The result is DEFINED by a call the parity tests already pin and by tests/helpers/unigram_ref.py, a plain restatement of the definition
over bytes, one dict and numpy.float32: the byte slices latok_token_spans_utf8_bytes_batch reports for string s, each marked or not by
its predecessor's end, each cut by the reference.  Beside it stand the recorded cases of tokenizers.models.Unigram
(tests/golden/unigram_hf_cases.json).  Every batch goes through the C ABI with poisoned guard bands round every output and is checked
in full.  The shapes are the smallest at which the kernels can go wrong: the sizes of a workgroup, of a scan block, of the lane form
and the ceiling of max_bytes come from the library (latok_debug_unigram_limits).  Where a case needs a token with chosen bytes, rule
tables that never split make every string one token (its bytes minus the whitespace at both ends)."""
import ctypes as C
import functools
import json
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import ALPHABETS, ROOT, random_strings
from helpers import span_strip_content as ssc
from helpers import unigram_ref as ref

pytestmark = pytest.mark.gpu

POISON_32 = np.int32(-0x5A5A5A5B)        # 0xA5A5A5A5 as int32
GUARD = 16
IDS_ROUTE, PADDED_ROUTE = 22, 23
ONE_TOKEN_PER_STRING = (ssc._NONE, ssc._NONE, ssc._NONE)
UNK = -1
MK = ref.MARKER
GREEDY_WORDS = [b"ab", b"cd", b"abc", b"bcd", b"a", b"b", b"c", b"d"]
GREEDY_SCORES = [-1.0, -1.125, -1.0, -1.0, -4.0, -4.0, -4.0, -4.0]


@functools.lru_cache(maxsize=1)
def limits():
    """(kUniBlock, entries of one scan block, kUniLaneBytes, the ceiling of max_bytes)"""
    from latok_amd import _lib
    fn = _lib.load().latok_debug_unigram_limits
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
def _vocab(seed=5, alphabet=("a", "b", "c"), n_words=60, dyadic=True):
    """(words, scores): every single character, random words of 2 .. 5 characters, a third of them behind the marker too, the marker"""
    rng = random.Random(seed)
    chars = [c.encode() for c in alphabet]
    words = list(chars)
    while len(words) < len(chars) + n_words:
        w = b"".join(rng.choice(chars) for _ in range(rng.randint(2, 5)))
        if w not in words:
            words.append(w)
    words += [MK + w for w in words[::3]] + [MK]
    if dyadic:
        scores = [-rng.randint(1, 96) / 8.0 for _ in words]
    else:
        scores = (-np.random.default_rng(seed).random(len(words), np.float32) * np.float32(12) - np.float32(0.01)).astype(np.float32).tolist()
    return tuple(words), tuple(scores)


def _rand(rng, n, alphabet=b"abc"):
    return bytes(rng.choice(alphabet) for _ in range(n))


# ---- the definition --------------------------------------------------------------------------------------------------------
def want_of(u8, boff, words, scores, unk_score=None, marker=MK, fuse=True, max_bytes=4096, unk=UNK, ids=None):
    """(indptr, ids, spans[n, 2], n_tokens) by the reference on the slices of the spans call"""
    from latok_amd import batch
    counts, spans = batch.token_spans_utf8_bytes_csr(u8, boff)
    us = ref.default_unk_score(scores) if unk_score is None else np.float32(unk_score)
    with np.errstate(over="ignore"):
        indptr, pids, sp = ref.cut_rows(u8, boff, counts, spans, ref.word_dict(words), scores, us, marker, fuse, max_bytes, unk, ids)
    return indptr, pids, sp, int(counts.sum())


# ---- the calls, with guard bands ---------------------------------------------------------------------------------------------
class _Out:
    def __init__(self, n_str, cap, dt):
        self.n_str, self.cap = n_str, cap
        self.indptr = np.full(n_str + 1 + GUARD, -7, dt)
        self.ids = np.full(cap + GUARD, POISON_32, np.int32)
        self.spans = np.full(2 * (cap + GUARD), -7, dt)

    def pieces_untouched(self):
        return (self.ids == POISON_32).all() and (self.spans == -7).all()


def _call(lib, u8, boff, uni, cap=0, dt=np.int64, unk=UNK, want_ids=True, want_spans=True, total=None, flags=0, dev=False):
    """one blocking call -> (rc, n_pieces, n_tokens, _Out); dev: everything in device memory, copied back into the _Out"""
    from latok_amd import _lib
    n_str = boff.size - 1
    total = (int(boff[-1]) if n_str > 0 else 0) if total is None else total
    o = _Out(n_str, cap, dt)
    n, n_tok = C.c_int64(-1), C.c_int64(-1)
    flags |= _lib.OUT_INT32 if dt == np.int32 else 0
    handle = uni.handle if uni is not None else None
    if not dev:
        rc = lib.latok_unigram_ids_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, n_str, total, handle, unk, o.indptr.ctypes.data,
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
        rc = lib.latok_unigram_ids_utf8_bytes_batch(ptrs[0], ptrs[1], n_str, total, handle, unk, ptrs[2], ptrs[3] if want_ids else None,
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
    assert o.indptr.dtype == dt and np.array_equal(o.indptr[:n_str + 1], indptr), (what, "indptr", o.indptr[:n_str + 1].tolist()[:40], indptr.tolist()[:40])
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


def check(lib, blobs, words, scores, unk_score=None, marker=MK, fuse=True, max_bytes=4096, seed=0, unk=UNK, ids=None, what="", forms=FORMS[:2]):
    """the whole definition for one batch; returns want = (indptr, ids, spans, n_tokens)"""
    from latok_amd import _lib, batch
    u8, boff = batch.pack_utf8(blobs)
    want = want_of(u8, boff, words, scores, unk_score, marker, fuse, max_bytes, unk, ids)
    need = len(want[1])
    with batch.Unigram(words, scores, ids=ids, marker=marker, unk_score=unk_score, fuse_unk=fuse, max_bytes=max_bytes, seed=seed) as uni:
        for dt, dev, with_spans in forms:
            rc, n, n_tok, o = _call(lib, u8, boff, uni, cap=need, dt=dt, unk=unk, dev=dev, want_spans=with_spans)
            assert rc == 0, (what, _lib.last_error())
            assert n == need, (what, n, need)
            assert lib.latok_debug_last_route() == IDS_ROUTE or int(boff[-1]) == 0
            _compare((what, dt.__name__, "device" if dev else "host"), o, n_tok, want, dt, has_spans=with_spans)
    return want


def _rows(want):
    return [list(zip(want[1][a:b].tolist(), *want[2][a:b].T.tolist())) for a, b in zip(want[0][:-1], want[0][1:])]


# ---- 1. the recorded cases of the tokenizers package ---------------------------------------------------------------------------
def test_the_recorded_cases_of_the_tokenizers_package(gpu):
    from latok_amd import batch
    with open(os.path.join(ROOT, "tests", "golden", "unigram_hf_cases.json"), encoding="utf-8") as f:
        doc = json.load(f)
    n_cases = 0
    for v in doc["vocabularies"]:
        words = [w.encode() for w in v["words"]]
        # words joined by single spaces: every token is marked under the marker, none under the empty marker
        for marked, marker in ((True, MK), (False, b"")):
            cases = [c for c in v["cases"] if c["marked"] == marked]
            blobs = [b" ".join(c["word"].encode() for c in cases[i:i + 7]) for i in range(0, len(cases), 7)]
            u8, boff = batch.pack_utf8(blobs)
            with batch.Unigram(words, v["scores"], marker=marker) as uni:
                assert uni.unk_score == min(v["scores"]) - 10
                got = batch.unigram_ids_utf8_csr(u8, boff, uni, unk_id=v["unk_id"])
            counts, spans = batch.token_spans_utf8_bytes_csr(u8, boff)
            assert int(counts.sum()) == len(cases), "a word is not one token"      # so no case drops out
            m = len(MK) if marked else 0
            at = 0
            for t, c in enumerate(cases):
                a = int(spans[t][0])
                want_ids = c["ids"]
                want_spans = [[max(s - m, 0) + a, e - m + a] for s, e in c["offsets"]]
                assert got[1][at:at + len(want_ids)].tolist() == want_ids and got[2][at:at + len(want_ids)].tolist() == want_spans, (c, marked)
                at += len(want_ids)
                n_cases += 1
            assert at == len(got[1]) == got[0][-1]
    assert n_cases >= 300


# ---- 2. the search, the scores, the marker ---------------------------------------------------------------------------------------
def test_the_best_path_is_not_the_greedy_longest_match(gpu):
    want = check(gpu, [b"abcd", b"x abcd", b"abcd,abcd"], GREEDY_WORDS, GREEDY_SCORES, marker=b"", what="greedy", forms=FORMS)
    assert _rows(want)[0] == [(0, 0, 2), (1, 2, 4)]


def test_the_marker(gpu):
    words, scores = GREEDY_WORDS + [MK, MK + b"ab", b","], GREEDY_SCORES + [-2.0, -1.5, -3.0]
    blobs = [b"ab, cd", b"abcd", b"cd  cd,cd", b" ab", b"", b"x", b"xab x,x", b"  ", b"cd"]
    want = check(gpu, blobs, words, scores, what="marker", forms=FORMS)
    rows = _rows(want)
    assert rows[0] == [(9, 0, 2), (10, 2, 3), (8, 4, 4), (1, 4, 6)]               # marked | touches its predecessor | the marker alone, empty span
    assert rows[1] == [(9, 0, 2), (1, 2, 4)] and rows[3] == [(9, 1, 3)] and rows[8] == [(8, 0, 0), (1, 0, 2)]
    assert rows[5] == [(8, 0, 0), (UNK, 0, 1)]
    # a marker that is no word: unknown, fused with a following unknown character, or not fused
    want = check(gpu, blobs, GREEDY_WORDS, GREEDY_SCORES, what="marker unknown, fused", forms=FORMS[:1] + FORMS[3:4])
    assert _rows(want)[5] == [(UNK, 0, 1)] and _rows(want)[1][0] == (UNK, 0, 0) and _rows(want)[6][:2] == [(UNK, 0, 1), (0, 1, 3)]
    want = check(gpu, blobs, GREEDY_WORDS, GREEDY_SCORES, fuse=False, what="marker unknown, not fused")
    assert _rows(want)[5] == [(UNK, 0, 0), (UNK, 0, 1)]
    want = check(gpu, blobs, words, scores, marker=b"", what="empty marker")
    assert _rows(want)[1] == [(0, 0, 2), (1, 2, 4)] and all(s < e for row in _rows(want) for _, s, e in row)
    check(gpu, blobs, GREEDY_WORDS + [b"#ab", b"#"], GREEDY_SCORES + [-0.5, -0.25], marker=b"#", what="one-byte marker")


def test_ties_rounding_sums_and_a_fused_run_that_spells_a_word(gpu, one_token_per_string):
    rng = random.Random(3)
    # dyadic scores with ties at several positions: the lower start wins
    tokens = [b"a" * n for n in range(1, 40)] + [_rand(rng, rng.randint(1, 30), b"ab") for _ in range(60)]
    words = [b"a", b"aa", b"aaa", b"b", b"ab", b"ba", b"aab", MK + b"a", MK]
    want = check(gpu, tokens, words, [-1.0, -2.0, -3.0, -1.0, -2.0, -2.0, -3.0, -1.0, -1.0], what="ties", forms=FORMS[:1] + FORMS[3:4])
    assert _rows(want)[2] == [(7, 0, 1), (1, 1, 3)]                               # marker+a | aa ties with marker+a | a | a: the lower start stays
    # arbitrary float32 scores whose sums round: the order of addition
    for scale in (1.0, 1e7, 2.5e37):
        w, s = _vocab(seed=7, dyadic=False)
        s = (np.array(s, np.float32) * np.float32(scale)).astype(np.float32).tolist()
        tokens = [_rand(rng, rng.randint(1, 60)) for _ in range(150)] + [_rand(rng, 100), _rand(rng, 200)]
        check(gpu, tokens, list(w), s, what=("rounding", scale), forms=FORMS[:1])
    for fuse in (True, False):
        want = check(gpu, [b"xy", b"xyq", b"qxy", b"xyxy", b"xy" * 40], [b"xy", b"q"], [-100.0, -1.0], unk_score=-1.0, fuse=fuse, what=("fused run", fuse))
        assert _rows(want)[0] == ([(UNK, 0, 2)] if fuse else [(UNK, 0, 0), (UNK, 0, 1), (UNK, 1, 2)])


# ---- 3. the edges of the two forms ---------------------------------------------------------------------------------------------------
def test_the_edges_of_the_lane_form_and_the_wave_form(gpu, one_token_per_string):
    block, chunk, lane_bytes, ceiling = limits()
    rng = random.Random(2)
    words, scores = _vocab()
    sizes = [1, lane_bytes - 1, lane_bytes, lane_bytes + 1, 130]
    tokens = [_rand(rng, n) for n in sizes] + [(b"ab" * n)[:n] for n in sizes] + [b"x" * 100, b"z" * 64, b"z" * 65, b"abz" * 30]
    for fuse in (True, False):
        want = check(gpu, tokens, list(words), list(scores), fuse=fuse, what=("form edges", fuse), forms=FORMS)
        assert want[3] == len(tokens)
    # every length at every start phase around the edge
    blobs, at = [], 0
    for n in list(range(1, 9)) + list(range(lane_bytes - 3, lane_bytes + 4)):
        for phase in range(4):
            pad = (phase - at) % 4
            blobs.append(b" " * pad + _rand(rng, n))
            at += pad + n
    check(gpu, blobs, list(words), list(scores), what="lengths x phases", forms=FORMS[:1] + FORMS[3:4])
    # max_bytes = 80: one byte less, exactly, one more (one unk piece)
    toks = [_rand(rng, n) for n in (79, 80, 81)]
    want = check(gpu, toks, list(words), list(scores), max_bytes=80, what="max_bytes 80")
    assert _rows(want)[2] == [(UNK, 0, 81)] and len(_rows(want)[1]) > 1
    want = check(gpu, [_rand(rng, n) for n in (5, 6, 7)], list(words), list(scores), max_bytes=6, what="max_bytes 6")
    assert _rows(want)[2] == [(UNK, 0, 7)]


def test_one_token_at_the_ceiling_of_max_bytes(gpu, one_token_per_string):
    ceiling = limits()[3]
    rng = random.Random(4)
    words, scores = _vocab()
    tokens = [_rand(rng, ceiling), b"ab", _rand(rng, ceiling + 1)]
    want = check(gpu, tokens, list(words), list(scores), max_bytes=ceiling, what="ceiling", forms=FORMS[:1] + FORMS[3:4])
    assert _rows(want)[2] == [(UNK, 0, ceiling + 1)] and len(_rows(want)[0]) > ceiling // 6


@pytest.mark.parametrize("name, n_tok, long_at", [("lane 0", 64, (0,)), ("lane 63", 64, (63,)), ("several", 130, (3, 4, 40, 64, 127, 129)),
                                                  ("a wave of long tokens only", 192, tuple(range(64, 128)))])
def test_long_and_short_tokens_in_one_wave(gpu, one_token_per_string, name, n_tok, long_at):
    lane_bytes = limits()[2]
    rng = random.Random(len(name))
    words, scores = _vocab()
    tokens = [_rand(rng, rng.randint(lane_bytes + 1, lane_bytes + 120), b"abcz") if i in long_at else _rand(rng, rng.randint(1, 14), b"abcz") for i in range(n_tok)]
    want = check(gpu, tokens, list(words), list(scores), what=name, forms=FORMS[:1] + FORMS[3:4])
    assert want[3] == n_tok


# ---- 4. totals round a workgroup and a scan block -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("base, delta", [(b, d) for b in (256, "block") for d in (-1, 0, 1)])
def test_token_totals_round_a_workgroup(gpu, base, delta):
    n = (limits()[0] if base == "block" else base) + delta                        # 255 / 256 / 257 and the kernel's block - 1, exactly, + 1
    words, scores = _vocab()
    rng = random.Random(n)
    toks = [_rand(rng, rng.randint(1, 9)) for _ in range(n)]
    # a last string without a token, empty and whitespace-only strings between
    want = check(gpu, [b" ".join(toks[:n // 3]), b"", b"  ", b",".join(toks[n // 3:]).replace(b",", b" ", 5), b"\t"], list(words), list(scores),
                 what=("workgroup", n), forms=FORMS[:1] + FORMS[3:4])
    assert want[3] >= n


def test_token_totals_round_a_scan_block(gpu):
    block, chunk, lane_bytes, _ = limits()
    words, scores = _vocab()
    for delta in (-1, 0, 1):
        m = chunk - 1 + delta                                                     # n_tok + 1 = one scan block - 1, exactly, + 1
        toks = [(b"ab", b"c", b"abcab")[i % 3] for i in range(m)]
        many = [b"", b" "] + [b" ".join(toks[i:i + 500]) for i in range(0, m, 500)] + [b"", b"\t", b""]
        want = check(gpu, many, list(words), list(scores), what=("scan block", m), forms=FORMS[:1])
        assert want[3] == m


# ---- 5. characters ------------------------------------------------------------------------------------------------------------------
def test_characters_of_two_three_and_four_bytes_known_and_unknown(gpu):
    chars = ["a", "é", "日", "🤓"]
    words, scores = _vocab(seed=9, alphabet=tuple(chars), n_words=40)
    rng = random.Random(9)
    letters = chars + ["ß", "本", "🙂", "z"]
    blobs = [" ".join("".join(rng.choice(letters if rng.random() < 0.3 else chars) for _ in range(rng.randint(1, 12))) for _ in range(rng.randint(0, 6))).encode()
             for _ in range(120)]
    for fuse in (True, False):
        want = check(gpu, blobs, list(words), list(scores), fuse=fuse, what=("characters", fuse), forms=FORMS[:1] + FORMS[3:4])
        assert (want[1] == UNK).any() and (want[1] != UNK).any()


def test_malformed_bytes_inside_tokens(gpu, one_token_per_string):
    chars = ["a", "é", "日"]
    words, scores = _vocab(seed=10, alphabet=tuple(chars), n_words=30)
    # continuation bytes at a token's start (the marker's character takes them), a cut-off lead byte at its end
    tokens = [b"\xa9\xa9a", b"\xa9", b"\x97\xa5a\xe6", b"a\xe6\x97", b"\xf0\x9f", b"\x80" * 64, b"\x80" * 70, b"a\xc3", "é日a".encode() + b"\xe6", b"\xa9" + "日é".encode() * 30]
    for fuse in (True, False):
        for marker in (MK, b""):
            check(gpu, tokens, list(words) + [MK + b"\xa9"], list(scores) + [-0.5], fuse=fuse, marker=marker, what=("malformed", fuse, marker))


@pytest.mark.parametrize("alphabet", ["mixed", "bmp"])
def test_random_strings_under_the_default_rules(gpu, alphabet):
    from latok_amd import batch
    rng = random.Random(len(alphabet))
    blobs = [t.encode("utf-8", "surrogatepass") for t in random_strings(rng, 200, 0, 60, ALPHABETS[alphabet])]
    blobs += [b"ab\xe6\x97 cd", b"\xc3 x", b"lone \xf0\x9f\x98", b"end\xe6", b"\xf0", b"a\x80\x80\x80\x80b", b"\xa9 cont", b"x" * 300 + b" y"]
    u8, boff = batch.pack_utf8(blobs)
    counts, spans = batch.token_spans_utf8_bytes_csr(u8, boff)
    raw, base = u8.tobytes(), np.repeat(boff[:-1], counts)
    toks = [raw[a:b] for a, b in zip((base + spans[:, 0]).tolist(), (base + spans[:, 1]).tolist())]
    words = list(dict.fromkeys([t[:k] for t in toks[::3] for k in range(1, min(len(t), 6) + 1)] + [MK + t for t in toks[1::5]] + [MK]))
    scores = [-rng.randint(1, 200) / 16.0 for _ in words]
    want = check(gpu, blobs, words, scores, what=alphabet, forms=FORMS[:1] + FORMS[3:4])
    assert want[3] == len(toks) and len(want[1]) >= want[3]


# ---- 6. the vocabulary ----------------------------------------------------------------------------------------------------------------
def test_word_ids_duplicates_and_an_empty_vocabulary(gpu):
    blobs = [b"ab abcd bcd", b"abab xab", b"", b"dcb abcdx", b"a"]
    ids = [5, -3, 7, 0x7FFFFFFF, -0x80000000, 0, -1, 1]
    want = check(gpu, blobs, GREEDY_WORDS, GREEDY_SCORES, ids=ids, unk=-7, seed=0x9747B28C, marker=b"", what="explicit ids", forms=FORMS)
    assert want[1][:3].tolist() == [5, 5, -3] and -7 in want[1].tolist() and -0x80000000 in want[1].tolist()
    want = check(gpu, blobs, [b"a", b"b", b"ab", b"a", b"ab", b"", b"b"], [-1.0, -1.0, -1.5, -0.1, -0.1, -1.0, -0.1], marker=b"", what="duplicates: the first wins")
    assert want[1][0] == 2 and set(want[1].tolist()) <= {0, 1, 2, UNK}
    want = check(gpu, blobs, [], [], what="V = 0, fused", forms=FORMS)
    assert (want[1] == UNK).all() and len(want[1]) == want[3]
    want = check(gpu, blobs, [], [], fuse=False, marker=b"", what="V = 0, not fused")
    assert (want[1] == UNK).all() and len(want[1]) == sum(len(b.replace(b" ", b"")) for b in blobs)
    check(gpu, blobs, [b"", b"", b""], [-1.0, -1.0, -1.0], what="empty words")


def test_info_reports_what_was_built(gpu):
    from latok_amd import batch
    with batch.Unigram([b"abc", MK + b"defghij", b"", b"x", b"abc", MK], [-1, -2, -3, -4, -5, -6], max_bytes=9, fuse_unk=False, seed=77, unk_score=-3.5) as uni:
        assert uni.info() == dict(n_words=6, n_slots_plain=64, n_slots_marked=64, max_len=10, marker_word=5, marker=MK, unk_score=-3.5, fuse_unk=0,
                                  max_bytes=9, seed=77, device=uni.info()["device"]) and len(uni) == 6
    with pytest.raises(ValueError):
        uni.info()


# ---- 7. the calls --------------------------------------------------------------------------------------------------------------------
def test_capacity_protocol_and_refusals(gpu):
    from latok_amd import _lib, batch
    rng = random.Random(9)
    words, scores = _vocab()
    blobs = [b" ".join(_rand(rng, rng.randint(1, 12)) for _ in range(rng.randrange(0, 9))) for _ in range(200)]
    blobs[7] = _rand(rng, 150) + b" " + _rand(rng, 70)
    u8, boff = batch.pack_utf8(blobs)
    want = want_of(u8, boff, words, scores)
    need, n_str = len(want[1]), len(blobs)
    assert need > want[3] > 0
    with batch.Unigram(words, scores, seed=11) as uni:
        for dev in (False, True):
            # the size query: no id buffer, capacity 0
            rc, n, n_tok, o = _call(gpu, u8, boff, uni, cap=0, want_ids=False, want_spans=False, dev=dev)
            assert rc == _lib.ERR_INVALID and n == need and n_tok == want[3] and np.array_equal(o.indptr[:n_str + 1], want[0])
            # one short: nothing written to ids or spans, indptr valid, the need returned
            rc, n, n_tok, o = _call(gpu, u8, boff, uni, cap=need - 1, dt=np.int32, dev=dev)
            assert rc == _lib.ERR_INVALID and "capacity" in _lib.last_error() and n == need and o.pieces_untouched()
            assert np.array_equal(o.indptr[:n_str + 1], want[0]) and (o.indptr[n_str + 1:] == -7).all()
            # exact, with total_bytes = -1; larger than needed
            for cap in (need, need + 5):
                rc, n, n_tok, o = _call(gpu, u8, boff, uni, cap=cap, total=-1, dev=dev)
                assert rc == 0 and n == need, _lib.last_error()
                _compare(("capacity", cap, dev), o, n_tok, want, np.int64)
            assert gpu.latok_debug_last_route() == IDS_ROUTE
        # refused before any device work
        rc, n, n_tok, o = _call(gpu, u8, boff, uni, cap=need, want_ids=False)
        assert rc == _lib.ERR_INVALID and "cap > 0" in _lib.last_error() and o.pieces_untouched() and (o.indptr == -7).all()
        rc, n, n_tok, o = _call(gpu, u8, boff, uni, cap=-1)
        assert rc == _lib.ERR_INVALID and "capacity" in _lib.last_error() and (o.indptr == -7).all()
        for flag in (4, 64, 1 << 30):
            rc, n, n_tok, o = _call(gpu, u8, boff, uni, cap=need, flags=flag)
            assert rc == _lib.ERR_INVALID and "unknown flag" in _lib.last_error() and o.pieces_untouched() and (o.indptr == -7).all()
        rc, n, n_tok, o = _call(gpu, u8, boff, None, cap=need)
        assert rc == _lib.ERR_INVALID and "uni is NULL" in _lib.last_error() and (o.indptr == -7).all()
        o = _Out(n_str, need, np.int64)
        n = C.c_int64(-1)
        rc = gpu.latok_unigram_ids_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, n_str, -1, uni.handle, UNK, None, o.ids.ctypes.data, None, need,
                                                    C.byref(n), None, 0, None)
        assert rc == _lib.ERR_INVALID and "indptr_out" in _lib.last_error() and o.pieces_untouched()
        # n_str = 0 and total_bytes = 0
        rc, n, n_tok, o = _call(gpu, np.zeros(0, np.uint8), np.zeros(1, np.int64), uni, cap=4)
        assert rc == 0 and n == 0 and n_tok == 0 and o.pieces_untouched() and (o.indptr[1:] == -7).all(), _lib.last_error()
        for dev in (False, True):
            e8, eoff = batch.pack_utf8([b"", b"", b""])
            rc, n, n_tok, o = _call(gpu, e8 if e8.size else np.zeros(1, np.uint8), eoff, uni, cap=4, dev=dev)
            assert rc == 0 and n == 0 and n_tok == 0 and o.pieces_untouched() and o.indptr[:4].tolist() == [0] * 4 and (o.indptr[4:] == -7).all()
        device = uni.info()["device"]
        ctx = _lib.Context(device)                                            # another context of the same device may use the object
        try:
            with ctx:
                rc, n, n_tok, o = _call(gpu, u8, boff, uni, cap=need)
                assert rc == 0
                _compare("second context", o, n_tok, want, np.int64)
        finally:
            ctx.destroy()
        if gpu.latok_device_count() > 1:
            other = _lib.Context((device + 1) % gpu.latok_device_count())
            try:
                with other:
                    rc, n, n_tok, o = _call(gpu, u8, boff, uni, cap=need)
                    assert rc == _lib.ERR_INVALID and "device" in _lib.last_error() and o.pieces_untouched()
            finally:
                other.destroy()
    assert gpu.latok_unigram_info(None, *[None] * 12) == _lib.ERR_INVALID
    # the create call's refusals, with a device present
    for kw in (dict(scores=[-1.0, float("inf")]), dict(unk_score=float("nan")), dict(marker=b"ab"), dict(max_bytes=4097)):
        kw.setdefault("scores", [-1.0, -2.0])
        with pytest.raises(ValueError):
            batch.Unigram([b"a", b"b"], **kw)


# ---- 8. the padded form -----------------------------------------------------------------------------------------------------------
def _padded(lib, u8, boff, uni, max_length, special, bos=101, eos=102, pad=0, unk=UNK, dev=False):
    from latok_amd import _lib
    n_str = boff.size - 1
    block = np.full(n_str * max_length + GUARD, POISON_32, np.int32)
    lengths = np.full(n_str + GUARD, POISON_32, np.int32)
    n = C.c_int64(-1)
    total = int(boff[-1]) if n_str else 0
    if not dev:
        rc = lib.latok_unigram_padded_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, n_str, total, uni.handle, unk, max_length, int(special), bos, eos,
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
        rc = lib.latok_unigram_padded_utf8_bytes_batch(ptrs[0], ptrs[1], n_str, -1, uni.handle, unk, max_length, int(special), bos, eos, pad, ptrs[2],
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
    words, scores = GREEDY_WORDS + [MK, MK + b"ab"], GREEDY_SCORES + [-2.0, -1.5]
    blobs = [b"", b"ab", b"abcb c", b"bcd dcb", b"ab ab ab ab ab ab", b"  ", b"xab a", b"ab " * 11 + b"abcdx " + b"dx" * 35]
    u8, boff = batch.pack_utf8(blobs)
    want = want_of(u8, boff, words, scores)
    assert np.diff(want[0])[0] == 0 and np.diff(want[0])[-1] > 80
    with batch.Unigram(words, scores) as uni:
        for max_length, special, dev in ((6, True, False), (4, False, False), (7, True, True), (5, False, True), (1, False, False), (3, True, False),
                                         (128, True, False)):
            rc, n, block, lengths = _padded(gpu, u8, boff, uni, max_length, special, pad=-9, dev=dev)
            assert rc == 0 and n == len(want[1]), _lib.last_error()
            assert gpu.latok_debug_last_route() == PADDED_ROUTE
            w_block, w_len = _want_padded(want, max_length, special, pad=-9)
            assert np.array_equal(block[:w_block.size].reshape(w_block.shape), w_block), (max_length, special, dev)
            assert np.array_equal(lengths[:len(blobs)], w_len) and (block[w_block.size:] == POISON_32).all() and (lengths[len(blobs):] == POISON_32).all()
        for max_length, special in ((0, False), (2, True), (-1, False)):
            rc = gpu.latok_unigram_padded_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, len(blobs), -1, uni.handle, UNK, max_length, int(special), 1, 2, 0,
                                                           block.ctypes.data, lengths.ctypes.data, None, 0, None)
            assert rc == _lib.ERR_INVALID and "max_length" in _lib.last_error()
        rc = gpu.latok_unigram_padded_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, len(blobs), -1, uni.handle, UNK, 8, 1, 1, 2, 0, block.ctypes.data,
                                                       lengths.ctypes.data, None, 8, None)
        assert rc == _lib.ERR_INVALID and "unknown flag" in _lib.last_error()
        rc = gpu.latok_unigram_padded_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, len(blobs), -1, None, UNK, 8, 1, 1, 2, 0, block.ctypes.data,
                                                       lengths.ctypes.data, None, 0, None)
        assert rc == _lib.ERR_INVALID and "uni is NULL" in _lib.last_error()
        for empty in ([b"", b"", b""], [b" ", b"\t\t", b""]):
            e8, eoff = batch.pack_utf8(empty)
            e8 = e8 if e8.size else np.zeros(1, np.uint8)
            rc, n, block, lengths = _padded(gpu, e8, eoff, uni, 4, True, pad=7)
            assert rc == 0 and n == 0 and block[:12].tolist() == [101, 102, 7, 7] * 3 and lengths[:3].tolist() == [2, 2, 2], empty
        # the Python wrapper and its attention mask
        ids, mask = batch.unigram_encode_utf8_batch(blobs, uni, 6, bos_id=101, eos_id=102, pad_id=0)
        w_block, w_len = _want_padded(want, 6, True)
        assert ids.dtype == mask.dtype == np.int32 and np.array_equal(ids, w_block)
        assert np.array_equal(mask, (np.arange(6)[None, :] < w_len[:, None]).astype(np.int32)) and mask.sum() == w_len.sum()
        ids, mask = batch.unigram_encode_utf8_batch(blobs, uni, 4, pad_id=-1)
        assert np.array_equal(ids, _want_padded(want, 4, False, pad=-1)[0]) and mask[0].sum() == 0 and mask[7].sum() == 4
        ids, mask = batch.unigram_encode_utf8_batch([], uni, 4)
        assert ids.shape == mask.shape == (0, 4)


# ---- 9. one context, shared workspace; wrappers; the example ---------------------------------------------------------------------------
def test_bpe_then_unigram_then_wordpiece_on_one_context(gpu):
    from latok_amd import batch
    rng = random.Random(4)
    words, scores = _vocab()
    large = [b" ".join(_rand(rng, rng.randint(1, 30)) for _ in range(rng.randrange(0, 12))) for _ in range(300)] + [_rand(rng, 300)]
    small = large[5:25]
    plain = [w for w in words if not w.startswith(MK)]
    with batch.Unigram(words, scores) as uni, batch.BPE(plain) as bpe, batch.WordPiece(plain[:30] + [b"##" + w for w in plain[:30]]) as wp:
        alone = (batch.bpe_ids_utf8_batch(large, bpe), batch.unigram_ids_utf8_batch(large, uni), batch.wordpiece_ids_utf8_batch(large, wp),
                 batch.unigram_ids_utf8_batch(small, uni))
        for _ in range(2):
            mixed = (batch.bpe_ids_utf8_batch(large, bpe), batch.unigram_ids_utf8_batch(large, uni), batch.wordpiece_ids_utf8_batch(large, wp),
                     batch.unigram_ids_utf8_batch(small, uni))           # a smaller batch behind a larger one
            for a, b in zip(alone, mixed):
                assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
        for blobs, got in ((large, alone[1]), (small, alone[3])):
            u8, boff = batch.pack_utf8(blobs)
            want = want_of(u8, boff, words, scores)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


def test_python_wrappers_and_decoding(gpu, tmp_path):
    from latok_amd import batch
    texts = ["low lower lowest", "slowest,  low", "", "   ", "low é", "x"]
    words = ["▁", "l", "o", "w", "e", "r", "s", "t", "▁low", "low", "er", "est", "▁s", ","]
    scores = [-2.0, -5.0, -5.0, -5.0, -5.0, -5.0, -5.0, -5.0, -3.0, -3.5, -3.0, -3.25, -4.0, -2.5]
    path = tmp_path / "tiny.vocab"
    path.write_bytes("".join("%s\t%r\n" % (w, s) for w, s in zip(words, scores)).encode())
    blobs = [t.encode() for t in texts]
    u8, boff = batch.pack_utf8(blobs)
    bwords = [w.encode() for w in words]
    want = want_of(u8, boff, bwords, scores, unk=-2)
    with batch.Unigram.from_vocab_file(str(path)) as uni:
        assert len(uni) == len(words) and uni.unk_score == -15.0 and uni.marker == MK
        got = batch.unigram_ids_batch(texts, uni, unk_id=-2)
        assert [g.dtype for g in got] == [np.int64, np.int32, np.int64]
        assert all(np.array_equal(a, b) for a, b in zip(got, want[:3]))
        assert got[1][:5].tolist() == [8, 8, 10, 8, 11]                 # ▁low | ▁low er | ▁low est
        got_b = batch.unigram_ids_utf8_batch(blobs, uni, unk_id=-2)
        assert all(np.array_equal(a, b) for a, b in zip(got, got_b))
        got32 = batch.unigram_ids_utf8_csr(u8, boff, uni, unk_id=-2, dtype=np.int32)
        assert got32[0].dtype == got32[2].dtype == np.int32 and all(np.array_equal(a, b) for a, b in zip(got, got32))
        assert batch.unigram_ids_utf8_csr(u8, boff, uni, spans=False)[2] is None
        empty = batch.unigram_ids_utf8_batch([], uni)
        assert empty[0].tolist() == [0] and len(empty[1]) == 0 and empty[2].shape == (0, 2)
        # a Detokenizer built from the same word list decodes the ids in CONCAT mode, the marker in the bytes
        with batch.Detokenizer(bwords, mode="concat") as detok:
            out, off = batch.decode_csr(detok, got[0], got[1], errors="ignore")
        assert out[off[0]:off[1]].tobytes().decode() == "▁low▁lower▁lowest" and out[off[4]:off[5]].tobytes().decode() == "▁low▁"
    with pytest.raises(ValueError):
        batch.unigram_ids_batch(texts, uni)                               # closed


def test_c_example(gpu, tmp_path):
    exe = str(tmp_path / "unigram_utf8")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "unigram_utf8.c"),
                           "-L" + os.path.join(ROOT, "latok_amd"), "-llatok_hip", "-Wl,-rpath," + os.path.join(ROOT, "latok_amd"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    assert lines[0] == "8 tokens, 13 pieces", lines[0]
    assert lines[1] == "  row 0: '▁low'[0,3) '▁low'[4,7) 'er'[7,9) '▁low'[10,13) 'est'[13,16)"
    assert lines[2] == "  row 1: '▁s'[0,1) 'low'[1,4) 'est'[4,7) ','[7,8) '▁low'[10,13)"
    assert lines[3] == "  row 2:" and lines[4] == "  row 3:" and lines[5] == "  row 4: '▁low'[0,3) '▁'[4,4) '?'[4,6)"
    assert lines[6] == "  input_ids 0 (7 used): 1 108 108 110 108 111 2 0 0 0 0 0"
    assert lines[8] == "  input_ids 2 (2 used): 1 2 0 0 0 0 0 0 0 0 0 0"
