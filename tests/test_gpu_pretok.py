"""GPT-2's pre-tokenizer on the device (latok_pretokens_utf8_bytes_batch, latok_bpe_create_pretok; include/latok_hip.h).

The result is DEFINED by tests/helpers/pretok_ref.py, a plain restatement of the definition over bytes that reads its classes from
tests/golden/pretok_classes.json, and, for the ids, by tests/helpers/bpe_ref.py on the reference's pre-tokens; the recorded cases of
the ``regex`` and ``tokenizers`` packages (tests/golden/pretok_worked.json, pretok_gpt2_cases.json) are compared where named.  Every
batch goes through the C ABI with poisoned guard bands round every output and is checked in full.  The shapes are the smallest at which
the kernel can go wrong: the sizes of a word, of a tile and of a workgroup come from the library (latok_debug_pretok_limits)."""
import ctypes as C
import functools
import json
import os
import random
import threading

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import bpe_ref
from helpers import pretok_ref as ref
from helpers import span_strip_content as ssc

pytestmark = pytest.mark.gpu

GPT2, LATOK = 1, 0
POISON_32 = np.int32(-0x5A5A5A5B)
GUARD = 16
IDS_ROUTE, PADDED_ROUTE, SPANS_ROUTE = 24, 25, 26
UNK = -1


@functools.lru_cache(maxsize=1)
def limits():
    """(bytes per word, bytes per tile, threads per workgroup, halo)"""
    from latok_amd import _lib
    fn = _lib.load().latok_debug_pretok_limits
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    out = np.zeros(4, np.int64)
    assert fn(out.ctypes.data, 4) == 4
    word, tile, threads, halo = map(int, out)
    assert word == 64 and tile == 64 * word and threads % 64 == 0 and 7 <= halo <= word
    return word, tile, threads, halo


@functools.lru_cache(maxsize=None)
def _pretokens(blob):
    return tuple(ref.pretokens(blob))


def pack(blobs):
    from latok_amd import batch
    u8, boff = batch.pack_utf8(blobs)
    return np.ascontiguousarray(u8) if u8.size else np.zeros(1, np.uint8)[:0], boff


def want_spans(blobs):
    """(counts, spans[n, 2]) by the reference"""
    rows = [_pretokens(bytes(b)) for b in blobs]
    counts = np.array([len(r) for r in rows], np.int64)
    spans = np.array([p for r in rows for p in r], np.int64).reshape(-1, 2)
    return counts, spans


# ---- the span call, with guard bands -----------------------------------------------------------------------------------------
def spans_call(lib, u8, boff, pretok=GPT2, cap=None, dt=np.int64, dev=False, want_records=True, total=None):
    """one blocking call -> (rc, n, counts with guard, spans with guard)"""
    from latok_amd import _lib
    n_str = boff.size - 1
    nbytes = int(boff[-1]) if n_str > 0 else 0
    total = nbytes if total is None else total
    cap = nbytes if cap is None else cap
    counts = np.full(n_str + GUARD, -7, dt)
    spans = np.full(2 * (cap + GUARD), -7, dt)
    n = C.c_int64(-1)
    flags = _lib.OUT_INT32 if dt == np.int32 else 0
    if not dev:
        rc = lib.latok_pretokens_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, n_str, total, pretok, counts.ctypes.data,
                                                  spans.ctypes.data if want_records else None, cap, C.byref(n), flags, None)
        return rc, n.value, counts, spans
    arrays = (counts, spans)
    sizes = [u8.nbytes + 256, boff.nbytes] + [a.nbytes for a in arrays]
    ptrs = [lib.latok_dev_alloc(s) for s in sizes]
    assert all(ptrs)
    try:
        _lib.check(lib.latok_memset_dev(ptrs[0], 0xFF, sizes[0]))      # what lies behind the batch is not the batch
        _lib.check(lib.latok_memcpy_h2d(ptrs[0], u8.ctypes.data, u8.nbytes))
        _lib.check(lib.latok_memcpy_h2d(ptrs[1], boff.ctypes.data, boff.nbytes))
        for a, p in zip(arrays, ptrs[2:]):
            _lib.check(lib.latok_memcpy_h2d(p, a.ctypes.data, a.nbytes))
        _lib.check(lib.latok_sync())
        rc = lib.latok_pretokens_utf8_bytes_batch(ptrs[0], ptrs[1], n_str, total, pretok, ptrs[2], ptrs[3] if want_records else None, cap, C.byref(n),
                                                  flags | _lib.DEVICE_PTRS, None)
        for a, p in zip(arrays, ptrs[2:]):
            _lib.check(lib.latok_memcpy_d2h(a.ctypes.data, p, a.nbytes))
    finally:
        for p in ptrs:
            lib.latok_dev_free(p)
    return rc, n.value, counts, spans


def check_spans(lib, blobs, what="", dt=np.int64, dev=False, want=None):
    from latok_amd import _lib
    u8, boff = pack(blobs)
    w_counts, w_spans = want_spans(blobs) if want is None else want
    rc, n, counts, spans = spans_call(lib, u8, boff, dt=dt, dev=dev)
    assert rc == 0, (what, _lib.last_error())
    n_str = len(blobs)
    assert n == len(w_spans), (what, "total", n, len(w_spans))
    if not np.array_equal(counts[:n_str], w_counts):
        s = int(np.nonzero(counts[:n_str] != w_counts)[0][0])
        raise AssertionError((what, "count of string", s, bytes(blobs[s])[:80], int(counts[s]), int(w_counts[s])))
    assert (counts[n_str:] == -7).all(), (what, "guard words behind the counts")
    got = spans[:2 * n].reshape(-1, 2)
    if not np.array_equal(got, w_spans):
        k = int(np.nonzero((got != w_spans).any(axis=1))[0][0])
        s = int(np.searchsorted(np.cumsum(w_counts), k, "right"))
        raise AssertionError((what, "record", k, "string", s, bytes(blobs[s])[:80], got[k].tolist(), w_spans[k].tolist()))
    assert (spans[2 * n:] == -7).all(), (what, "guard words behind the records")
    if int(boff[-1]) > 0:
        assert lib.latok_debug_last_route() == SPANS_ROUTE


def golden(name):
    with open(os.path.join(GOLDEN, name), encoding="utf-8") as f:
        return json.load(f)["cases"]


# ---- pre-token spans -----------------------------------------------------------------------------------------------------------
def test_the_worked_table_and_the_recorded_texts(gpu):
    cases = golden("pretok_worked.json")
    blobs = [c["text"].encode() for c in cases]
    counts = np.array([len(c["starts"]) for c in cases], np.int64)
    spans = np.array([[a, e] for c, b in zip(cases, blobs) for a, e in zip(c["starts"], c["starts"][1:] + [len(b)])], np.int64).reshape(-1, 2)
    check_spans(gpu, blobs, "worked table against the regex package", want=(counts, spans))
    check_spans(gpu, blobs, "worked table")
    check_spans(gpu, [c["text"].encode() for c in golden("pretok_gpt2_cases.json")], "recorded texts", dt=np.int32, dev=True)


def test_every_scalar_value_has_its_class(gpu):
    """for each code point c the strings a c a, 1 c 1 and c followed by a space: the first tells L from the rest, the second N, the third S;
    the expectation is the reference's for one code point of each (class, length) group, which is all the reference looks at"""
    with open(ref.GOLDEN) as f:
        g = json.load(f)
    cls = np.zeros(0x110000, np.uint8)                       # 0 = O, 1 = L, 2 = N, 3 = S
    for code, key in ((1, "L"), (2, "N"), (3, "S")):
        for lo, hi in g[key]:
            cls[lo:hi + 1] = code
    blobs, rows, tmpl = [], [], {}
    for c in range(0x110000):
        if 0xD800 <= c <= 0xDFFF:
            continue
        e = chr(c).encode()
        trio = (b"a" + e + b"a", b"1" + e + b"1", e + b" ")
        key = (int(cls[c]), len(e), c == 0x20)               # (the byte 0x20 is the one S character that is a lead space)
        if key not in tmpl:
            assert ref.cp_class(c) == "OLNS"[key[0]]
            tmpl[key] = [tuple(ref.pretokens(t)) for t in trio]
        blobs += trio
        rows += tmpl[key] if c >= 0x80 else [tuple(ref.pretokens(t)) for t in trio]   # (the apostrophe and the contraction letters are ASCII)
    assert len(tmpl) >= 12 and len(blobs) == 3 * (0x110000 - 0x800)
    counts = np.fromiter((len(r) for r in rows), np.int64, len(rows))
    spans = np.array([p for r in rows for p in r], np.int64).reshape(-1, 2)
    # the templates are the reference's own answers: a sample of every kind against the reference itself
    rng = random.Random(3)
    for i in rng.sample(range(len(blobs)), 6000):
        assert tuple(ref.pretokens(blobs[i])) == rows[i], blobs[i]
    check_spans(gpu, blobs, "every scalar value", dt=np.int32, dev=True, want=(counts, spans))


FEATURES = [b"a's b", b"we'll go", b"x 's", b"!'s", b"a \nb", b"a  b", b"a \xc2\xa0b", b"a\xc2\xa0\xc2\xa0b", b"a\xe3\x80\x80\xe3\x80\x80b", b"a\xe3\x80\x80 b",
            b"\n a", b" a", b" 1", b" !", b"\xf0\x9d\x9f\x98\xf0\x9f\xa4\x93", b"\xf0\x9d\x9f\x98\xf0\x90\x80\x80", b"a\xe3\x80\x80's"]


def _placed(edge, cuts):
    """every feature with each of its bytes in turn as the first byte behind a multiple of `edge`, whole and cut in two strings at the
    places `cuts(feature, k)` names; the fillers between the cases are short strings, so a case is what lies across the edge"""
    blobs, at = [], 0

    def advance(to):
        nonlocal at
        while at < to:
            s = b"filler  "[:min(8, to - at)]
            blobs.append(s)
            at += len(s)

    for f in FEATURES:
        for k in range(len(f) + 1):
            for cut in [None] + list(cuts(f, k)):
                target = ((at + k) // edge + 1) * edge                        # the edge the case lies across
                advance(target - k)
                for s in ([f] if cut is None else [f[:cut], f[cut:]]):
                    blobs.append(s)
                    at += len(s)
    advance((at + edge) // edge * edge + 1)
    return blobs


def test_every_feature_at_every_offset_across_a_word_edge(gpu):
    word, tile, _, _ = limits()
    check_spans(gpu, _placed(word, lambda f, k: range(1, len(f))), "word edges")


def test_every_feature_at_every_offset_across_a_tile_edge(gpu):
    word, tile, _, _ = limits()
    blobs = _placed(tile, lambda f, k: [c for c in (k - 1, k, k + 1) if 0 < c < len(f)])
    check_spans(gpu, blobs, "tile edges")
    check_spans(gpu, blobs, "tile edges, device pointers", dt=np.int32, dev=True)


def test_a_contraction_cut_by_a_string_end_does_not_pair_with_the_next_string(gpu):
    word, tile, _, _ = limits()
    for pad in (0, word - 3, word - 2, word - 1, tile - 3, tile - 2, tile - 1):
        blobs = [b"x" * pad + b"it'", b"s it'l", b"l", b"'", b"t", b"we'", b"ve", b"a'r", b"e"]
        check_spans(gpu, blobs, "pad %d" % pad)
        assert _pretokens(blobs[1])[0] == (0, 1) and _pretokens(blobs[0])[-1] == (pad + 2, pad + 3)


def test_long_runs_and_empty_strings(gpu):
    word, tile, threads, _ = limits()
    group = threads // 64 * tile                      # the bytes of one workgroup
    check_spans(gpu, [b"a" * (3 * tile + 5)], "one L run of three tiles")
    check_spans(gpu, [b" " * (tile + 70) + b"a"], "white space of more than a tile in front of a letter")
    check_spans(gpu, [b"\xe3\x80\x80" * (tile // 3 + 30) + b"a b"], "ideographic spaces across a tile edge")
    check_spans(gpu, [b"x"], "one byte")
    check_spans(gpu, [b"", b"", b"a b", b"", b"", b" c", b"", b""], "empty strings at the start, in the middle and at the end")
    check_spans(gpu, [b"", b""], "only empty strings")
    check_spans(gpu, [b"ab " * ((tile - 3) // 3), b"xyz", b"!"], "a last tile of one byte")
    check_spans(gpu, [b"word " * (group // 5), b"tail's"], "more than one workgroup")
    check_spans(gpu, [b"it's " * 13] * (group // 64 + 3), "many strings, device pointers", dt=np.int32, dev=True)
    u8, boff = pack([])
    rc, n, counts, spans = spans_call(gpu, u8, np.zeros(1, np.int64))
    assert rc == 0 and n == 0 and (counts == -7).all() and (spans == -7).all()


@pytest.mark.parametrize("dt,dev", [(np.int64, False), (np.int32, False), (np.int64, True), (np.int32, True)])
def test_random_differential(gpu, dt, dev):
    rng = random.Random(17)
    blobs = []
    for _ in range(3000):      # (a cut inside a sequence leaves a truncated one: the reference says what it is)
        blobs.append(ref.random_text(rng, 100).encode()[:rng.randint(0, 300)])
    check_spans(gpu, blobs, "random text", dt=dt, dev=dev)


def test_malformed_bytes(gpu):
    rng = random.Random(6)
    pieces = [b"\x80", b"\xbf", b"\xc0\x80", b"\xc1\xbf", b"\xc2", b"\xe0\x80\x80", b"\xe0\xa0", b"\xed\xa0\x80", b"\xed\xbf\xbf", b"\xf0\x80\x80\x80",
              b"\xf0\x9f\xa4", b"\xf4\x90\x80\x80", b"\xf5\x80\x80\x80", b"\xf8\x88\x80\x80\x80", b"\xfe", b"\xff", b"\xe3\x80\x80", b"\xe3\x80\x80\x80",
              b"\xf0\x9d\x9f\x98", b"\xf0\x9d\x9f\x98\x80", b"a", b"1", b" ", b"'", b"s", b"'ll", b"\xc2\xa0", b"\xc3\xa9", b"\n", b"a\x80", b" \x80", b"'\x80"]
    blobs = [b"a\xe3", b"\x80\x80b", b"\xf0\x9f", b"\xa4\x93", b"\xe3\x80", b"\x80", b"\xc2", b"\x80", b"\xff" * 70, b"\x80" * 130, b"\xe3" + b"\x80" * 66 + b"a"]
    blobs += [b"".join(rng.choice(pieces) for _ in range(rng.randint(0, 40))) for _ in range(1500)]
    blobs += [bytes(rng.randrange(256) for _ in range(rng.randint(0, 200))) for _ in range(300)]
    check_spans(gpu, blobs, "malformed")
    check_spans(gpu, blobs[::-1], "malformed, device pointers", dt=np.int32, dev=True)


def test_pretok_latok_is_the_span_call_bit_for_bit(gpu):
    from latok_amd import batch
    rng = random.Random(4)
    blobs = [ref.random_text(rng, 60).encode() for _ in range(700)] + [b"see http://a.b/c or mail me@x.org, .@you #ok camelCase"] * 50
    u8, boff = pack(blobs)
    for dt in (np.int64, np.int32):
        rc, n, counts, spans = spans_call(gpu, u8, boff, pretok=LATOK, dt=dt)
        w_counts, w_spans = batch.token_spans_utf8_bytes_csr(u8, boff, dtype=dt)
        assert rc == 0 and n == len(w_spans) and np.array_equal(counts[:len(blobs)], w_counts) and np.array_equal(spans[:2 * n].reshape(-1, 2), w_spans)
        assert (counts[len(blobs):] == -7).all() and (spans[2 * n:] == -7).all()
        got = batch.pretokens_utf8_csr(u8, boff, "latok", dtype=dt)
        assert np.array_equal(got[0], w_counts) and np.array_equal(got[1], w_spans)
    assert n < want_spans(blobs)[1].shape[0]               # (GPT-2's pattern keeps the white space: more records)


def test_the_capacity_protocol_and_the_size_query(gpu):
    from latok_amd import _lib
    blobs = [b"don't  stop\n", b"", b" 12 apples"]
    u8, boff = pack(blobs)
    w_counts, w_spans = want_spans(blobs)
    need = len(w_spans)
    for dev in (False, True):
        rc, n, counts, spans = spans_call(gpu, u8, boff, cap=0, dev=dev, want_records=False)     # the size query
        assert rc == _lib.ERR_INVALID and n == need and np.array_equal(counts[:3], w_counts) and (spans == -7).all()
        rc, n, counts, spans = spans_call(gpu, u8, boff, cap=need - 1, dev=dev)
        assert rc == _lib.ERR_INVALID and "need %d" % need in _lib.last_error() and n == need
        assert np.array_equal(counts[:3], w_counts) and (spans == -7).all() and (counts[3:] == -7).all()
        rc, n, counts, spans = spans_call(gpu, u8, boff, cap=need, dev=dev)
        assert rc == 0 and n == need and np.array_equal(spans[:2 * need].reshape(-1, 2), w_spans) and (spans[2 * need:] == -7).all()
    rc, n, counts, spans = spans_call(gpu, u8, boff, total=-1)                                    # total_bytes = -1: read from byte_off
    assert rc == 0 and n == need and np.array_equal(spans[:2 * need].reshape(-1, 2), w_spans)
    rc, n, counts, spans = spans_call(gpu, u8, boff, total=-1, dev=True, dt=np.int32)
    assert rc == 0 and n == need and np.array_equal(spans[:2 * need].reshape(-1, 2), w_spans)


def test_custom_rule_tables_do_not_reach_this_pre_tokenizer(gpu):
    from latok_amd import batch
    rng = random.Random(8)
    blobs = [ref.random_text(rng, 80).encode() for _ in range(400)]
    batch.set_rules(ssc._NONE, ssc._NONE, ssc._NONE)
    try:
        assert batch.rules_active()
        check_spans(gpu, blobs, "under custom rules")
    finally:
        batch.reset_rules()
    check_spans(gpu, blobs, "after them")


def test_the_python_wrappers(gpu):
    from latok_amd import batch
    texts = ["don't  stop\n", "", "日本語 123", " lead", "🤓's"]
    assert batch.pretokenize_batch(texts) == [["don", "'t", " ", " stop", "\n"], [], ["日本語", " 123"], [" lead"], ["🤓'", "s"]]
    assert batch.pretokenize_utf8_batch([t.encode() for t in texts]) == [[p.encode() for p in row] for row in batch.pretokenize_batch(texts)]
    assert batch.pretokenize_batch(texts, "latok") == [list(map(bytes.decode, row)) for row in batch.tokenize_utf8_batch([t.encode() for t in texts])]


# ---- BPE behind it -----------------------------------------------------------------------------------------------------------------
def want_pieces(blobs, words, ids=None, max_bytes=4096, unk=UNK):
    """(indptr, ids, spans[n, 2], n_tokens) by the two references"""
    d = bpe_ref.rank_dict(words)
    indptr, pids, sp, n_tok = [0], [], [], 0
    for b in blobs:
        for a, e in _pretokens(bytes(b)):
            n_tok += 1
            for pid, p0, p1 in bpe_ref.cut(bytes(b)[a:e], d, max_bytes, unk, ids):
                pids.append(pid)
                sp.append((a + p0, a + p1))
        indptr.append(len(pids))
    return np.array(indptr, np.int64), np.array(pids, np.int64).astype(np.int32), np.array(sp, np.int64).reshape(-1, 2), n_tok


def bpe_call(lib, u8, boff, bpe, cap, dt=np.int64, unk=UNK, want_ids=True, dev=False):
    from latok_amd import _lib
    n_str = boff.size - 1
    total = int(boff[-1]) if n_str > 0 else 0
    indptr, ids, spans = np.full(n_str + 1 + GUARD, -7, dt), np.full(cap + GUARD, POISON_32, np.int32), np.full(2 * (cap + GUARD), -7, dt)
    n, n_tok = C.c_int64(-1), C.c_int64(-1)
    flags = _lib.OUT_INT32 if dt == np.int32 else 0
    if not dev:
        rc = lib.latok_bpe_ids_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, n_str, total, bpe.handle, unk, indptr.ctypes.data,
                                                ids.ctypes.data if want_ids else None, spans.ctypes.data if want_ids else None, cap, C.byref(n),
                                                C.byref(n_tok), flags, None)
        return rc, n.value, n_tok.value, indptr, ids, spans
    arrays = (indptr, ids, spans)
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
        rc = lib.latok_bpe_ids_utf8_bytes_batch(ptrs[0], ptrs[1], n_str, total, bpe.handle, unk, ptrs[2], ptrs[3] if want_ids else None,
                                                ptrs[4] if want_ids else None, cap, C.byref(n), C.byref(n_tok), flags | _lib.DEVICE_PTRS, None)
        for a, p in zip(arrays, ptrs[2:]):
            _lib.check(lib.latok_memcpy_d2h(a.ctypes.data, p, a.nbytes))
    finally:
        for p in ptrs:
            lib.latok_dev_free(p)
    return rc, n.value, n_tok.value, indptr, ids, spans


def check_pieces(lib, blobs, bpe, want, what="", dt=np.int64, dev=False, unk=UNK):
    from latok_amd import _lib
    u8, boff = pack(blobs)
    w_indptr, w_ids, w_spans, w_tok = want
    n_str, need = len(blobs), len(w_ids)
    rc, n, n_tok, indptr, ids, spans = bpe_call(lib, u8, boff, bpe, need, dt, unk, dev=dev)
    assert rc == 0, (what, _lib.last_error())
    assert (n, n_tok) == (need, w_tok), (what, n, need, n_tok, w_tok)
    assert np.array_equal(indptr[:n_str + 1], w_indptr) and (indptr[n_str + 1:] == -7).all(), (what, "indptr")
    if not np.array_equal(ids[:need], w_ids):
        k = int(np.nonzero(ids[:need] != w_ids)[0][0])
        s = int(np.searchsorted(w_indptr, k, "right")) - 1
        raise AssertionError((what, "piece", k, "string", s, bytes(blobs[s])[:80], int(ids[k]), int(w_ids[k])))
    assert (ids[need:] == POISON_32).all(), (what, "guard words behind the ids")
    assert np.array_equal(spans[:2 * need].reshape(-1, 2), w_spans) and (spans[2 * need:] == -7).all(), (what, "spans")
    if int(boff[-1]) > 0:
        assert lib.latok_debug_last_route() == IDS_ROUTE


@pytest.fixture(scope="module")
def gpt2_model(gpu):
    from latok_amd import batch
    model = os.path.join(GOLDEN, "pretok_gpt2")
    bpe = batch.BPE.from_gpt2_files(os.path.join(model, "vocab.json"), os.path.join(model, "merges.txt"))
    yield bpe
    bpe.close()


def test_the_recorded_ids_and_offsets_of_the_tokenizers_package(gpu, gpt2_model):
    """CSR form: ids AND piece spans against the package's; its offsets count characters, and a piece covers every character it holds a byte of"""
    from latok_amd import batch
    cases = golden("pretok_gpt2_cases.json")
    blobs = [c["text"].encode() for c in cases]
    assert gpt2_model.specials == {"<|endoftext|>": 0} and gpt2_model.pretokenizer == "gpt2" and gpt2_model.pretokenizer_of_object() == "gpt2"
    assert gpt2_model.info()["lead_space"] == 0
    indptr, ids, spans = batch.bpe_ids_utf8_batch(blobs, gpt2_model)
    assert gpu.latok_debug_last_route() == IDS_ROUTE
    for s, (c, b) in enumerate(zip(cases, blobs)):
        lo, hi = int(indptr[s]), int(indptr[s + 1])
        assert ids[lo:hi].tolist() == c["ids"], c["text"]
        char_of = [i for i, ch in enumerate(c["text"]) for _ in ch.encode()]
        assert [[char_of[a], char_of[e - 1] + 1] for a, e in spans[lo:hi].tolist()] == c["offsets"], c["text"]
    words, wids, _ = batch.BPE.gpt2_word_list(os.path.join(GOLDEN, "pretok_gpt2", "vocab.json"), os.path.join(GOLDEN, "pretok_gpt2", "merges.txt"))
    check_pieces(gpu, blobs, gpt2_model, want_pieces(blobs, words, wids), "recorded texts", dt=np.int32, dev=True)
    # the padded form with BOS / EOS: what a model takes
    L, bos, eos, pad = 24, 1000, 1001, 1002
    input_ids, mask = batch.bpe_encode_utf8_batch(blobs, gpt2_model, L, bos_id=bos, eos_id=eos, pad_id=pad)
    assert gpu.latok_debug_last_route() == PADDED_ROUTE
    for s, c in enumerate(cases):
        row = [bos] + c["ids"][:L - 2] + [eos]
        assert input_ids[s].tolist() == row + [pad] * (L - len(row)) and mask[s].tolist() == [1] * len(row) + [0] * (L - len(row)), c["text"]


def test_random_vocabularies_over_the_reference_pre_tokens(gpu):
    from latok_amd import batch
    rng = random.Random(12)
    blobs = [ref.random_text(rng, 60).encode() for _ in range(1200)]
    corpus = [bytes(b)[a:e] for b in blobs[:600] for a, e in _pretokens(b)]
    for n_merges, ids in ((40, None), (300, "random")):
        words = bpe_ref.train(corpus, n_merges)
        wids = [rng.randrange(-1 << 31, 1 << 31) for _ in words] if ids else None
        with batch.BPE(words, ids=wids, pretokenizer="gpt2", seed=n_merges) as bpe:
            check_pieces(gpu, blobs, bpe, want_pieces(blobs, words, wids, unk=-9), "%d merges" % n_merges, unk=-9)
            check_pieces(gpu, blobs[::-1], bpe, want_pieces(blobs[::-1], words, wids), "%d merges, device pointers" % n_merges, dt=np.int32, dev=True)


def test_long_pre_tokens_max_bytes_and_the_capacity_protocol(gpu):
    from latok_amd import _lib, batch
    words = [b" ", b"a", b"b", b"  ", b"ab", b"    ", b"abab", b"\n"]
    blobs = [b" " * 70 + b"ab", b"ab" * 40 + b" ab", b"a" * 9 + b" " * 9 + b"\n", b"", b"ab" * 5 + b" ab" * 3, b" " * 300]
    with batch.BPE(words, pretokenizer="gpt2", max_bytes=8) as bpe:       # longer than max_bytes: ONE unk piece
        want = want_pieces(blobs, words, max_bytes=8, unk=-3)
        assert (want[1] == -3).sum() >= 4
        check_pieces(gpu, blobs, bpe, want, "max_bytes 8", unk=-3)
    with batch.BPE(words, pretokenizer="gpt2") as bpe:                    # a white-space run of 65+ bytes: the wave form
        want = want_pieces(blobs, words)
        check_pieces(gpu, blobs, bpe, want, "wave form")
        check_pieces(gpu, blobs, bpe, want, "wave form, device pointers", dt=np.int32, dev=True)
        u8, boff = pack(blobs)
        need = len(want[1])
        for dev in (False, True):
            rc, n, n_tok, indptr, ids, spans = bpe_call(gpu, u8, boff, bpe, 0, want_ids=False, dev=dev)          # the size query
            assert n == need and n_tok == want[3] and np.array_equal(indptr[:len(blobs) + 1], want[0]) and (ids == POISON_32).all()
            rc, n, n_tok, indptr, ids, spans = bpe_call(gpu, u8, boff, bpe, need - 1, dev=dev)
            assert rc == _lib.ERR_INVALID and n == need and (ids == POISON_32).all() and (spans == -7).all() and np.array_equal(indptr[:len(blobs) + 1], want[0])
    try:
        batch.BPE(words, pretokenizer="gpt2", lead_space=True)
        raise AssertionError("lead_space with gpt2 was accepted")
    except ValueError:
        pass
    h = C.c_void_p()
    data, off = np.frombuffer(b"ab", np.uint8), np.array([0, 1, 2], np.int64)
    assert gpu.latok_bpe_create_pretok(data.ctypes.data, off.ctypes.data, 2, None, 64, 1, GPT2, 0, C.byref(h)) == _lib.ERR_INVALID and not h.value
    assert gpu.latok_bpe_create_pretok(data.ctypes.data, off.ctypes.data, 2, None, 64, 0, 7, 0, C.byref(h)) == _lib.ERR_INVALID and not h.value


def test_round_trip_through_the_decoder(gpu):
    from latok_amd import batch
    rng = random.Random(2)
    blobs = [ref.random_text(rng, 80).encode() for _ in range(500)] + [b"", b" ", b"\n\n", b" " * 200, b"don't  stop\n"]
    corpus = [bytes(b)[a:e] for b in blobs for a, e in _pretokens(b)]
    words = bpe_ref.train(corpus, 200, base=list(range(256)))
    with batch.BPE(words, pretokenizer="gpt2") as bpe, batch.Detokenizer(words) as detok:
        indptr, ids, _ = batch.bpe_ids_utf8_batch(blobs, bpe)
        assert (ids >= 0).all()
        out, off = batch.decode_csr(detok, indptr, ids)
        data = out.tobytes()
        assert [data[off[s]:off[s + 1]] for s in range(len(blobs))] == blobs


# ---- one context, several contexts -------------------------------------------------------------------------------------------------
def test_call_order_on_one_context(gpu):
    """the planes share the workspace: a latok call, a GPT-2 call and the latok call again; a GPT-2 BPE call between two lead_space calls"""
    from latok_amd import batch
    rng = random.Random(9)
    blobs = [ref.random_text(rng, 70).encode() for _ in range(600)]
    u8, boff = pack(blobs)
    corpus = [bytes(b)[a:e] for b in blobs[:300] for a, e in _pretokens(b)]
    words = bpe_ref.train(corpus, 80)
    first = batch.token_spans_utf8_bytes_csr(u8, boff)
    check_spans(gpu, blobs, "between two latok calls")
    again = batch.token_spans_utf8_bytes_csr(u8, boff)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    with batch.BPE(words, lead_space=True) as lead, batch.BPE(words, pretokenizer="gpt2") as gpt2:
        a = batch.bpe_ids_utf8_batch(blobs, lead)
        assert gpu.latok_debug_last_route() == 18
        check_pieces(gpu, blobs, gpt2, want_pieces(blobs, words), "between two lead_space calls")
        b = batch.bpe_ids_utf8_batch(blobs, lead)
        assert gpu.latok_debug_last_route() == 18
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
        check_spans(gpu, blobs[:50], "a smaller batch behind a larger one")


def test_a_second_context_and_one_object_shared_by_two_contexts(gpu):
    from latok_amd import _lib, batch
    rng = random.Random(10)
    blobs = [ref.random_text(rng, 70).encode() for _ in range(500)]
    corpus = [bytes(b)[a:e] for b in blobs[:300] for a, e in _pretokens(b)]
    words = bpe_ref.train(corpus, 80)
    want = want_pieces(blobs, words)
    device = gpu.latok_ctx_device(None)
    ctx = _lib.Context(device)
    try:
        with ctx:
            check_spans(gpu, blobs, "second context")
    finally:
        ctx.destroy()
    errors = []
    with batch.BPE(words, pretokenizer="gpt2") as bpe:
        ctxs = [_lib.Context(device) for _ in range(2)]
        gate = threading.Barrier(2, timeout=120)

        def work(k):
            try:
                with ctxs[k]:
                    gate.wait()
                    for r in range(3):
                        check_pieces(gpu, blobs if (k + r) % 2 else blobs[::-1], bpe, want if (k + r) % 2 else want_pieces(blobs[::-1], words), "worker %d" % k)
            except BaseException as exc:   # noqa: BLE001 - reported to the main thread
                errors.append(exc)
                try:
                    gate.abort()
                except Exception:
                    pass

        want_pieces(blobs[::-1], words)
        ths = [threading.Thread(target=work, args=(k,)) for k in range(2)]
        for t in ths:
            t.start()
        for t in ths:
            t.join(300)
        alive = [t.is_alive() for t in ths]
        for c, t in zip(ctxs, ths):
            if not t.is_alive():
                c.destroy()
        if errors:
            raise errors[0]
        assert not any(alive)
