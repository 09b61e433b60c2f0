"""The cl100k / Llama 3 pre-tokenizer on the device (LATOK_PRETOK_CL100K in latok_pretokens_utf8_bytes_batch and latok_bpe_create_pretok;
include/latok_hip.h).

The result is DEFINED by tests/helpers/pretok_cl100k_ref.py, a plain restatement of the definition over bytes that reads its classes
from tests/golden/pretok_classes.json, and, for the ids, by tests/helpers/bpe_ref.py on the reference's pre-tokens; the recorded cases
of the ``regex`` and ``tokenizers`` packages (tests/golden/pretok_cl100k_worked.json, pretok_cl100k_cases.json) are compared where
named.  Every batch goes through the C ABI with poisoned guard bands round every output and is checked in full.  The sizes of a word, a
tile, a workgroup, the halo and a step of the record walk come from the library (latok_debug_pretok_cl100k_limits).

The carries (d, absorbed, notopen, nl_ahead) are exercised by runs of every kind at the lengths 1..7, halo-1..halo+2, 63..66, 127..130,
tile-1..tile+2, 2 tiles+1, workgroup bytes+-1, 64 tiles+-1 and 64 tiles+tile+1, each at all twelve start offsets (0..2 mod 3 x 0..3 mod
4) in front of a word edge; the reference walks every distinct text once."""
import ctypes as C
import functools
import itertools
import os
import random
import threading

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import bpe_ref
from helpers import pretok_cl100k_ref as ref
from helpers import pretok_ref as gpt2_ref
from helpers import span_strip_content as ssc
from test_gpu_pretok import POISON_32, bpe_call, golden, pack, spans_call
from test_pretok_cl100k_host import FEATURES, run_cases, run_kinds
from test_pretok_host import MALFORMED

pytestmark = pytest.mark.gpu

LATOK, GPT2, CL100K = 0, 1, 3
IDS_ROUTE, PADDED_ROUTE, SPANS_ROUTE = 27, 28, 29
UNK = -1


@functools.lru_cache(maxsize=1)
def limits():
    """(bytes per word, bytes per tile, threads per workgroup, halo, tile records per walk step)"""
    from latok_amd import _lib
    fn = _lib.load().latok_debug_pretok_cl100k_limits
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_int]
    out = np.zeros(5, np.int64)
    assert fn(out.ctypes.data, 5) == 5
    word, tile, threads, halo, step = map(int, out)
    assert word == 64 and tile == 64 * word and threads % 64 == 0 and 8 <= halo <= word and 1 <= step <= 64
    return word, tile, threads, halo, step


@functools.lru_cache(maxsize=None)
def _pretokens(blob):
    return tuple(ref.pretokens(blob))


def want_spans(blobs, pretokens=_pretokens):
    rows = [pretokens(bytes(b)) for b in blobs]
    counts = np.array([len(r) for r in rows], np.int64)
    spans = np.array([p for r in rows for p in r], np.int64).reshape(-1, 2)
    return counts, spans


def check_spans(lib, blobs, what="", dt=np.int64, dev=False, want=None, pretok=CL100K, route=SPANS_ROUTE):
    from latok_amd import _lib
    u8, boff = pack(blobs)
    w_counts, w_spans = want_spans(blobs) if want is None else want
    rc, n, counts, spans = spans_call(lib, u8, boff, pretok=pretok, dt=dt, dev=dev)
    assert rc == 0, (what, _lib.last_error())
    n_str = len(blobs)
    assert n == len(w_spans), (what, "total", n, len(w_spans))
    if not np.array_equal(counts[:n_str], w_counts):
        s = int(np.nonzero(counts[:n_str] != w_counts)[0][0])
        raise AssertionError((what, "count of string", s, len(blobs[s]), bytes(blobs[s])[:80], int(counts[s]), int(w_counts[s])))
    assert (counts[n_str:] == -7).all(), (what, "guard words behind the counts")
    got = spans[:2 * n].reshape(-1, 2)
    if not np.array_equal(got, w_spans):
        k = int(np.nonzero((got != w_spans).any(axis=1))[0][0])
        s = int(np.searchsorted(np.cumsum(w_counts), k, "right"))
        raise AssertionError((what, "record", k, "string", s, len(blobs[s]), bytes(blobs[s])[:80], got[k].tolist(), w_spans[k].tolist()))
    assert (spans[2 * n:] == -7).all(), (what, "guard words behind the records")
    if int(boff[-1]) > 0:
        assert lib.latok_debug_last_route() == route


# ---- pre-token spans -----------------------------------------------------------------------------------------------------------
def test_the_worked_table_and_the_recorded_texts(gpu):
    cases = golden("pretok_cl100k_worked.json")
    blobs = [c["text"].encode() for c in cases]
    counts = np.array([len(c["starts"]) for c in cases], np.int64)
    spans = np.array([[a, e] for c, b in zip(cases, blobs) for a, e in zip(c["starts"], c["starts"][1:] + [len(b)])], np.int64).reshape(-1, 2)
    check_spans(gpu, blobs, "worked table against the regex package", want=(counts, spans))
    check_spans(gpu, blobs, "worked table")
    check_spans(gpu, [c["text"].encode() for c in golden("pretok_cl100k_cases.json")], "recorded texts", dt=np.int32, dev=True)
    text = "!\n\n  \n x 1234567  \t!"
    from latok_amd import batch
    assert batch.pretokenize_batch([text, "DON'T", ""], "cl100k") == [["!\n\n", "  \n", " x", " ", "123", "456", "7", "  ", "\t", "!"], ["DON", "'T"], []]
    assert batch.pretokenize_utf8_batch([text.encode()], "cl100k") == [[p.encode() for p in batch.pretokenize_batch([text], "cl100k")[0]]]


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
                target = ((at + k) // edge + 1) * edge
                advance(target - k)
                for s in ([f] if cut is None else [f[:cut], f[cut:]]):
                    blobs.append(s)
                    at += len(s)
    advance((at + edge) // edge * edge + 1)
    return blobs


def test_every_feature_at_every_offset_across_a_word_edge(gpu):
    word = limits()[0]
    check_spans(gpu, _placed(word, lambda f, k: range(1, len(f))), "word edges")


def test_every_feature_at_every_offset_across_a_tile_edge(gpu):
    tile = limits()[1]
    blobs = _placed(tile, lambda f, k: [c for c in (k - 1, k, k + 1) if 0 < c < len(f)])
    check_spans(gpu, blobs, "tile edges")
    check_spans(gpu, blobs, "tile edges, device pointers", dt=np.int32, dev=True)


def test_every_feature_at_every_offset_across_a_workgroup_edge(gpu):
    _, tile, threads, _, _ = limits()
    check_spans(gpu, _placed(threads // 64 * tile, lambda f, k: [c for c in (k,) if 0 < c < len(f)]), "workgroup edges")


def _aligned(cases):
    """[(text, offset)] -> the strings of one batch: every text starts `offset` bytes in front of a word edge, behind a filler string"""
    word = limits()[0]
    blobs, at = [], 0
    for text, offset in cases:
        fill = (-offset - at) % word
        if fill:
            blobs.append((b"fill " * 13)[:fill])
            at += fill
        for s in (text if isinstance(text, list) else [text]):
            blobs.append(s)
            at += len(s)
    return blobs


@pytest.mark.parametrize("kind", sorted(run_kinds()))
def test_the_runs_that_the_carries_cross(gpu, kind):
    word, tile, threads, halo, step = limits()
    make = run_kinds()[kind]
    lengths = run_cases(word, tile, threads // 64 * tile, halo, big=False)
    big = [step * tile - 1, step * tile + 1, step * tile + tile + 1]
    whole, split, ends = [], [], []
    k = 0
    for n in lengths:
        text = make(n)
        for offset in range(12):
            whole.append((text, offset))
            cut = len(text) // 2 + (offset % 3) - 1
            if 0 < cut < len(text):
                split.append(([text[:cut], text[cut:]], offset))          # a string boundary inside the run
        ends.append((text[:len(text) // 2 + 1], k % 12))                  # the run cut by the batch's end
        k += 1
    for j, n in enumerate(big):
        text = make(n)
        check_spans(gpu, _aligned([(text, offset) for offset in range(12)]), kind + ": whole runs of %d" % n, dt=np.int32, dev=True)
        split.append(([text[:len(text) // 3], text[len(text) // 3:]], j))
    ends.append((make(big[1])[:big[1] - 7], 5))
    check_spans(gpu, _aligned(whole), kind + ": whole runs")
    check_spans(gpu, _aligned(split), kind + ": a string boundary inside the run", dt=np.int32, dev=True)
    for text, offset in ends[::3] + ends[-2:]:
        check_spans(gpu, _aligned([(b"some text in front", 0), (text, offset)]), kind + ": cut by the batch's end")


def test_empty_strings_at_the_front_at_the_back_and_between_runs(gpu):
    _, tile, _, _, _ = limits()
    kinds = run_kinds()
    runs = [kinds[k](n) for k in ("N1", "O+NL", "NL+SP+NL", "Smixed", "Nmixed") for n in (5, 70, tile + 1)]
    blobs = [b"", b""]
    for r in runs:
        blobs += [r[:len(r) // 2], b"", r[len(r) // 2:], b"", b""]
    check_spans(gpu, blobs, "empty strings")
    check_spans(gpu, blobs[::-1], "empty strings, device pointers", dt=np.int32, dev=True)
    check_spans(gpu, [b"", b""], "only empty strings")
    check_spans(gpu, [b"x"], "one byte")
    u8, boff = pack([])
    rc, n, counts, spans = spans_call(gpu, u8, np.zeros(1, np.int64), pretok=CL100K)
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
    pieces = MALFORMED + [b"\n", b"\r", b"!", b"'\xc5\xbf", b"'S", b"'Re", b"7", b"\xd9\xa3"]
    blobs = [b"a\xe3", b"\x80\x80b", b"\xf0\x9f", b"\xa4\x93", b"\xe3\x80", b"\x80", b"\xc2", b"\x80", b"\xff" * 70, b"\x80" * 130, b"\xe3" + b"\x80" * 66 + b"a",
             b"!\xe3" + b"\x80" * 66 + b"a", b" !" + b"\x80" * 300 + b"a", b"b!" + b"\x80" * 5000 + b"a", b"it'\xc5", b"\xbf", b"1\x80" * 5 + b"1111"]
    blobs += [b"".join(rng.choice(pieces) for _ in range(rng.randint(0, 40))) for _ in range(1500)]
    blobs += [bytes(rng.randrange(256) for _ in range(rng.randint(0, 200))) for _ in range(300)]
    check_spans(gpu, blobs, "malformed")
    check_spans(gpu, blobs[::-1], "malformed, device pointers", dt=np.int32, dev=True)


def test_the_other_modes_do_not_change_when_cl100k_calls_run_in_between(gpu):
    from latok_amd import batch
    rng = random.Random(4)
    blobs = [ref.random_text(rng, 60).encode() for _ in range(700)] + [b"see http://a.b/c or mail me@x.org, .@you #ok camelCase 1234567"] * 50
    u8, boff = pack(blobs)
    gpt2_want = want_spans(blobs, lambda b: tuple(gpt2_ref.pretokens(b)))
    for dt in (np.int64, np.int32):
        latok_first = spans_call(gpu, u8, boff, pretok=LATOK, dt=dt)
        check_spans(gpu, blobs, "GPT-2 before", dt=dt, want=gpt2_want, pretok=GPT2, route=26)
        check_spans(gpu, blobs, "cl100k in between", dt=dt)
        check_spans(gpu, blobs, "GPT-2 after", dt=dt, want=gpt2_want, pretok=GPT2, route=26)
        check_spans(gpu, blobs[:100], "cl100k, a smaller batch", dt=dt)
        latok_again = spans_call(gpu, u8, boff, pretok=LATOK, dt=dt)
        w_counts, w_spans = batch.token_spans_utf8_bytes_csr(u8, boff, dtype=dt)
        for rc, n, counts, spans in (latok_first, latok_again):
            assert rc == 0 and n == len(w_spans) and np.array_equal(counts[:len(blobs)], w_counts) and np.array_equal(spans[:2 * n].reshape(-1, 2), w_spans)
    assert not np.array_equal(gpt2_want[1], want_spans(blobs)[1])


def test_the_capacity_protocol_and_the_size_query(gpu):
    from latok_amd import _lib
    blobs = [b"DON'T  stop\n\n", b"", b" 1234 apples!\n"]
    u8, boff = pack(blobs)
    w_counts, w_spans = want_spans(blobs)
    need = len(w_spans)
    for dev in (False, True):
        rc, n, counts, spans = spans_call(gpu, u8, boff, pretok=CL100K, cap=0, dev=dev, want_records=False)     # the size query
        assert rc == _lib.ERR_INVALID and n == need and np.array_equal(counts[:3], w_counts) and (spans == -7).all()
        rc, n, counts, spans = spans_call(gpu, u8, boff, pretok=CL100K, cap=need - 1, dev=dev)
        assert rc == _lib.ERR_INVALID and "need %d" % need in _lib.last_error() and n == need
        assert np.array_equal(counts[:3], w_counts) and (spans == -7).all() and (counts[3:] == -7).all()
        rc, n, counts, spans = spans_call(gpu, u8, boff, pretok=CL100K, cap=need, dev=dev)
        assert rc == 0 and n == need and np.array_equal(spans[:2 * need].reshape(-1, 2), w_spans) and (spans[2 * need:] == -7).all()
    rc, n, counts, spans = spans_call(gpu, u8, boff, pretok=CL100K, total=-1)
    assert rc == 0 and n == need and np.array_equal(spans[:2 * need].reshape(-1, 2), w_spans)
    rc, n, counts, spans = spans_call(gpu, u8, boff, pretok=CL100K, total=-1, dev=True, dt=np.int32)
    assert rc == 0 and n == need and np.array_equal(spans[:2 * need].reshape(-1, 2), w_spans)
    assert gpu.latok_debug_last_route() == SPANS_ROUTE
    rc, n, counts, spans = spans_call(gpu, u8, boff, pretok=2)
    assert rc == _lib.ERR_INVALID and "pretok" in _lib.last_error()


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
def model(gpu):
    from latok_amd import batch
    bpe = batch.BPE.from_tokenizer_json(os.path.join(GOLDEN, "pretok_cl100k", "tokenizer.json"))
    yield bpe
    bpe.close()


def test_the_recorded_ids_and_offsets_of_the_tokenizers_package(gpu, model):
    """CSR form: ids AND piece spans against the package's; its offsets count characters, and a piece covers every character it holds a byte of"""
    from latok_amd import batch
    cases = golden("pretok_cl100k_cases.json")
    blobs = [c["text"].encode() for c in cases]
    assert model.specials == {"<|end_of_text|>": 0} and model.pretokenizer == "cl100k" and model.pretokenizer_of_object() == "cl100k"
    assert model.info()["lead_space"] == 0
    indptr, ids, spans = batch.bpe_ids_utf8_batch(blobs, model)
    assert gpu.latok_debug_last_route() == IDS_ROUTE
    for s, (c, b) in enumerate(zip(cases, blobs)):
        lo, hi = int(indptr[s]), int(indptr[s + 1])
        assert ids[lo:hi].tolist() == c["ids"], c["text"]
        char_of = [i for i, ch in enumerate(c["text"]) for _ in ch.encode()]
        assert [[char_of[a], char_of[e - 1] + 1] for a, e in spans[lo:hi].tolist()] == c["offsets"], c["text"]
    words, wids, _, _ = batch.BPE.tokenizer_json_word_list(os.path.join(GOLDEN, "pretok_cl100k", "tokenizer.json"))
    want = want_pieces(blobs, words, wids)
    check_pieces(gpu, blobs, model, want, "recorded texts, int64")
    check_pieces(gpu, blobs, model, want, "recorded texts, int32, device pointers", dt=np.int32, dev=True)
    # the padded form with BOS / EOS: what a model takes
    L, bos, eos, pad = 24, 1000, 1001, 1002
    input_ids, mask = batch.bpe_encode_utf8_batch(blobs, model, L, bos_id=bos, eos_id=eos, pad_id=pad)
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
        with batch.BPE(words, ids=wids, pretokenizer="cl100k", seed=n_merges) as bpe:
            check_pieces(gpu, blobs, bpe, want_pieces(blobs, words, wids, unk=-9), "%d merges" % n_merges, unk=-9)
            check_pieces(gpu, blobs[::-1], bpe, want_pieces(blobs[::-1], words, wids), "%d merges, device pointers" % n_merges, dt=np.int32, dev=True)


def test_long_pre_tokens_max_bytes_and_the_capacity_protocol(gpu):
    from latok_amd import _lib, batch
    words = [b" ", b"a", b"b", b"  ", b"ab", b"    ", b"abab", b"\n", b"1", b"11", b"111"]
    blobs = [b" " * 70 + b"ab", b"ab" * 40 + b" ab", b"a" * 9 + b" " * 9 + b"\n", b"", b"ab" * 5 + b" ab" * 3, b" " * 300, b"1" * 20 + b"\n" * 12]
    with batch.BPE(words, pretokenizer="cl100k", max_bytes=8) as bpe:       # longer than max_bytes: ONE unk piece
        want = want_pieces(blobs, words, max_bytes=8, unk=-3)
        assert (want[1] == -3).sum() >= 4
        check_pieces(gpu, blobs, bpe, want, "max_bytes 8", unk=-3)
    with batch.BPE(words, pretokenizer="cl100k") as bpe:                    # a white-space run of 65+ bytes: the wave form
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
    with pytest.raises(ValueError):
        batch.BPE(words, pretokenizer="cl100k", lead_space=True)
    h = C.c_void_p()
    data, off = np.frombuffer(b"ab", np.uint8), np.array([0, 1, 2], np.int64)
    assert gpu.latok_bpe_create_pretok(data.ctypes.data, off.ctypes.data, 2, None, 64, 1, CL100K, 0, C.byref(h)) == _lib.ERR_INVALID and not h.value
    assert gpu.latok_bpe_create_pretok(data.ctypes.data, off.ctypes.data, 2, None, 64, 0, 2, 0, C.byref(h)) == _lib.ERR_INVALID and not h.value


def test_round_trip_through_the_decoder(gpu):
    from latok_amd import batch
    rng = random.Random(2)
    blobs = [ref.random_text(rng, 80).encode() for _ in range(500)] + [b"", b" ", b"\n\n", b" " * 200, b"DON'T  stop!\r\n\r\n 1234567"]
    corpus = [bytes(b)[a:e] for b in blobs for a, e in _pretokens(b)]
    words = bpe_ref.train(corpus, 200, base=list(range(256)))
    with batch.BPE(words, pretokenizer="cl100k") as bpe, batch.Detokenizer(words) as detok:
        indptr, ids, _ = batch.bpe_ids_utf8_batch(blobs, bpe)
        assert (ids >= 0).all()
        out, off = batch.decode_csr(detok, indptr, ids)
        data = out.tobytes()
        assert [data[off[s]:off[s + 1]] for s in range(len(blobs))] == blobs


# ---- one context, several contexts -------------------------------------------------------------------------------------------------
def test_the_three_routes_in_every_order_on_one_context(gpu):
    """spans (29), BPE ids (27) and the padded block (28) share the workspace: every order of the three, each checked in full"""
    from latok_amd import batch
    rng = random.Random(9)
    blobs = [ref.random_text(rng, 70).encode() for _ in range(400)] + [b"7" * 9000, b"!" + b"\n" * 5000 + b" x"]
    corpus = [bytes(b)[a:e] for b in blobs[:300] for a, e in _pretokens(b)]
    words = bpe_ref.train(corpus, 80)
    want = want_pieces(blobs, words)
    L = 16
    with batch.BPE(words, pretokenizer="cl100k") as bpe:
        def spans():
            check_spans(gpu, blobs, "spans")

        def ids():
            check_pieces(gpu, blobs, bpe, want, "ids")

        def padded():
            input_ids, mask = batch.bpe_encode_utf8_batch(blobs, bpe, L, pad_id=-5)
            assert gpu.latok_debug_last_route() == PADDED_ROUTE
            for s in range(len(blobs)):
                row = want[1][want[0][s]:want[0][s + 1]][:L].tolist()
                assert input_ids[s].tolist() == row + [-5] * (L - len(row)) and int(mask[s].sum()) == len(row), s

        for order in itertools.permutations((spans, ids, padded)):
            for call in order:
                call()


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
    with batch.BPE(words, pretokenizer="cl100k") as bpe:
        ctxs = [_lib.Context(device) for _ in range(2)]
        gate = threading.Barrier(2, timeout=120)
        want_rev = want_pieces(blobs[::-1], words)

        def work(k):
            try:
                with ctxs[k]:
                    gate.wait()
                    for r in range(3):
                        check_pieces(gpu, blobs if (k + r) % 2 else blobs[::-1], bpe, want if (k + r) % 2 else want_rev, "worker %d" % k)
            except BaseException as exc:   # noqa: BLE001 - reported to the main thread
                errors.append(exc)
                try:
                    gate.abort()
                except Exception:
                    pass

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
