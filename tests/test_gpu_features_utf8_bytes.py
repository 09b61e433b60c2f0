"""featurize of UTF-8 batches in BYTE space (latok_token_features_utf8_bytes_batch): span records in byte positions of the
caller's buffer, feature sums per char.  Modelled case for case on test_gpu_features_utf8.py.  Two references:

* the oracle: counts, raw spans and sums are the oracle's parse matrix summed over the oracle's own token spans, with the oracle's
  char positions mapped to bytes by a cumulative sum of the UTF-8 lengths of the chars (numpy, from the text, no product call);
* the definition of the result by three calls that are themselves pinned to the oracle ("three-way identity"): counts and the
  stripped range = latok_token_spans_utf8_bytes_batch, the raw range = the two consecutive entries of
  latok_split_offsets_utf8_bytes_batch that enclose it, the sums = latok_token_features_utf8_batch.

Every case is compared in full, int64 and int32 records."""
import ctypes as C
import random

import numpy as np
import pytest

from conftest import ALPHABETS, RULE_SETS, pack, random_strings
from test_gpu_features_utf8 import _edge_text, _oracle_raw

pytestmark = pytest.mark.gpu

SMALL_CHARS = 262144   # api.cpp: kSmallChars
BYTE_ROUTE, HOST_DECODE = 4, 1   # latok_debug_last_route
DTYPES = (np.int64, np.int32)
EXTRA = list("é日🤓ü　Жδ") + ["http://a.b/c?d=1", "see me@x.org", "#tag", ".@you", "a@b.c"]
SOFT = [b"ab\xe6\x97 cd", b"\xc3 x", b"lone \xf0\x9f\x98", b"end\xe6", b"next starts ascii", b"\xe6\x97\xa5\xe6", b"\xf0", b"x\xc3"]
HARD = [b"a\x80\x80\x80\x80b", b"\xa9 starts with a continuation byte"]
POISON = 0x7F


def _route():
    from latok_amd import _lib
    return _lib.load().latok_debug_last_route()


def _enc(texts):
    from latok_amd import batch
    return batch.pack_utf8([t.encode("utf-8", "surrogatepass") for t in texts])


def _byte_pos(texts):
    """global byte position of every char of the packed batch (+ one entry: the byte total), from the code points alone"""
    cps, row = pack(texts)
    lens = 1 + (cps >= 0x80).astype(np.int64) + (cps >= 0x800) + (cps >= 0x10000)
    pos = np.zeros(cps.size + 1, np.int64)
    np.cumsum(lens, out=pos[1:])
    return cps, row, pos


def _to_bytes(spans_cp, counts, row, pos):
    """string-relative char positions [n, k] -> string-relative byte positions, through the global position map"""
    s = np.repeat(np.arange(counts.size), counts)
    return pos[spans_cp.astype(np.int64) + row[s][:, None]] - pos[row[s]][:, None]


def _three_way(u8, boff, got, dt, what=""):
    """the definition of the result (include/latok_hip.h) by the three calls that already exist"""
    from latok_amd import batch
    counts, spans4, feats = got
    assert counts.dtype == dt and spans4.dtype == dt and feats.dtype == np.int8 and spans4.shape[1:] == (4,) and feats.shape[1:] == (25,)
    c_sp, sp = batch.token_spans_utf8_bytes_csr(u8, boff, dtype=dt)
    c_of, of = batch.split_offsets_utf8_bytes_csr(u8, boff, dtype=dt)
    c_ft, _, f_ft = batch.token_features_utf8_csr(u8, boff, dtype=dt)
    assert np.array_equal(counts, c_sp) and np.array_equal(counts, c_ft), (what, "counts")
    assert spans4.shape[0] == sp.shape[0] == f_ft.shape[0] == int(counts.sum()), (what, "token total")
    assert np.array_equal(spans4[:, 2:], sp), (what, "stripped byte range")
    assert np.array_equal(feats, f_ft), (what, "sums")
    # raw range: all boundary offsets of the batch as global byte positions, the byte total closing the last one (a string's
    # first byte is a boundary, so the next non-empty string's start closes the last token of a string)
    s_tok = np.repeat(np.arange(counts.size), counts)
    g_off = np.concatenate([of.astype(np.int64) + np.repeat(boff[:-1], c_of), [boff[-1]]])
    assert np.all(np.diff(g_off[:-1]) > 0)
    g_strip0 = spans4[:, 2].astype(np.int64) + boff[s_tok]
    i = np.searchsorted(g_off, g_strip0, side="right") - 1
    raw0, raw1 = g_off[i] - boff[s_tok], g_off[i + 1] - boff[s_tok]
    assert np.array_equal(spans4[:, 0], raw0) and np.array_equal(spans4[:, 1], raw1), (what, "raw byte range")
    assert np.all(spans4[:, 3] <= spans4[:, 1]) and np.all(spans4[:, 2] < spans4[:, 3]) and np.all(spans4[:, 1] <= (boff[1:] - boff[:-1])[s_tok])


def _check(texts, what, route=BYTE_ROUTE, three_way=True):
    """host call, both record widths: the route it took; the UTF-32 entry point's records on the same text mapped char -> byte
    by numpy, its sums as they are; the three-way identity"""
    from latok_amd import batch
    u8, boff = _enc(texts)
    cps, row, pos = _byte_pos(texts)
    assert pos[-1] == u8.size and np.array_equal(pos[row], boff)
    for dt in DTYPES:
        got = batch.token_features_utf8_bytes_csr(u8, boff, dtype=dt)
        assert route is None or _route() == route, (what, dt, _route())
        w_counts, w_spans, w_feats = batch.token_features_csr(cps, row, dtype=dt)
        assert np.array_equal(got[0], w_counts) and np.array_equal(got[2], w_feats), (what, dt)
        assert np.array_equal(got[1], _to_bytes(w_spans, w_counts, row, pos)), (what, dt)
        if three_way:
            _three_way(u8, boff, got, dt, (what, dt))
    return u8, boff


def _dev_features(lib, u8, boff, dt, total=-1, cap=None):
    """the entry point with device pointers (byte count read by the library when total = -1); the record and sum buffers are
    filled with canaries first -> (rc, n, (counts, spans4, feats), (all spans4 bytes, all feats bytes))"""
    from latok_amd import _lib
    n_str = boff.size - 1
    isz = np.dtype(dt).itemsize
    flags = _lib.DEVICE_PTRS | (_lib.OUT_INT32 if dt == np.int32 else 0)
    cap = max(int(boff[-1]), 1) if cap is None else cap
    sizes = (u8.nbytes + 64, boff.nbytes, n_str * isz + 16, cap * 4 * isz + 16, cap * 25 + 16)
    d_u8, d_boff, d_counts, d_items, d_feat = ptrs = [lib.latok_dev_alloc(s) for s in sizes]
    assert all(ptrs)
    try:
        if u8.nbytes:
            _lib.check(lib.latok_memcpy_h2d(d_u8, u8.ctypes.data, u8.nbytes))
        _lib.check(lib.latok_memcpy_h2d(d_boff, boff.ctypes.data, boff.nbytes))
        for p, s in zip(ptrs[2:], sizes[2:]):
            _lib.check(lib.latok_memset_dev(p, POISON, s))
        _lib.check(lib.latok_sync())
        n = C.c_int64(-1)
        rc = lib.latok_token_features_utf8_bytes_batch(d_u8, d_boff, n_str, total, d_counts, d_items, d_feat, cap, C.byref(n), flags, None)
        counts = np.empty(n_str, dt)
        spans = np.empty((max(n.value, 0) if rc == 0 else 0, 4), dt)
        feats = np.empty((spans.shape[0], 25), np.int8)
        raw_items, raw_feat = np.empty(cap * 4 * isz, np.uint8), np.empty(cap * 25, np.uint8)
        for a, p in ((counts, d_counts), (spans, d_items), (feats, d_feat), (raw_items, d_items), (raw_feat, d_feat)):
            if a.nbytes:
                _lib.check(lib.latok_memcpy_d2h(a.ctypes.data, p, a.nbytes))
        return rc, n.value, (counts, spans, feats), (raw_items, raw_feat)
    finally:
        for p in ptrs:
            lib.latok_dev_free(p)


def _same(a, b, what=""):
    for x, y, name in zip(a, b, ("counts", "spans4", "features")):
        assert x.shape == y.shape and np.array_equal(x, y), (what, name)


def test_oracle_parity_host_and_device(gpu, oracle):
    """cases 1, 2 and 4 of the issue on the mixed corpus incl. empty strings"""
    from latok_amd import _lib, batch
    rng = random.Random(0xB17E5)
    texts = [""] + random_strings(rng, 4000, 0, 90, ALPHABETS["mixed"] + EXTRA) + ["", ""]
    u8, boff = _enc(texts)
    assert u8.size > SMALL_CHARS
    cps, row, pos = _byte_pos(texts)
    w_counts, w_raw, w_feats = _oracle_raw(oracle, texts)
    w_raw_bytes = _to_bytes(w_raw, w_counts, row, pos)
    need = int(w_counts.sum())
    for dt in DTYPES:
        got = batch.token_features_utf8_bytes_csr(u8, boff, dtype=dt)
        assert _route() == BYTE_ROUTE
        assert np.array_equal(got[0], w_counts) and np.array_equal(got[1][:, :2], w_raw_bytes) and np.array_equal(got[2], w_feats), dt
        _three_way(u8, boff, got, dt, ("host", dt))
        rc, n, dgot, _ = _dev_features(gpu, u8, boff, dt)
        assert rc == 0 and n == need and _route() == BYTE_ROUTE
        _same(dgot, got, ("device", dt))
        # capacity protocol: one token short is refused, reports the count it needs, leaves valid counts and writes nothing
        rc, n, (counts, _, _), (raw_items, raw_feat) = _dev_features(gpu, u8, boff, dt, total=int(boff[-1]), cap=need - 1)
        assert rc == _lib.ERR_INVALID and n == need and np.array_equal(counts, w_counts)
        assert (raw_items == POISON).all() and (raw_feat == POISON).all()
        # an exact capacity fits
        rc, n, dgot, _ = _dev_features(gpu, u8, boff, dt, cap=need)
        assert rc == 0 and n == need
        _same(dgot, got, ("exact capacity", dt))
        # cap = 0 with NULL buffers is a size query (host pointers)
        counts, n_out = np.empty(len(texts), dt), C.c_int64(0)
        flags = _lib.OUT_INT32 if dt == np.int32 else 0
        rc = gpu.latok_token_features_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, len(texts), int(boff[-1]), counts.ctypes.data,
                                                       None, None, 0, C.byref(n_out), flags, None)
        assert rc == _lib.ERR_INVALID and n_out.value == need and np.array_equal(counts, w_counts)
    # no strings at all
    n_out = C.c_int64(7)
    z = np.zeros(1, np.int64)
    assert gpu.latok_token_features_utf8_bytes_batch(None, z.ctypes.data, 0, 0, None, None, None, 0, C.byref(n_out), 0, None) == 0
    assert n_out.value == 0
    # only empty strings
    counts, n_out = np.full(3, 9, np.int64), C.c_int64(7)
    assert gpu.latok_token_features_utf8_bytes_batch(None, np.zeros(4, np.int64).ctypes.data, 3, 0, counts.ctypes.data, None, None, 0,
                                                     C.byref(n_out), 0, None) == 0
    assert n_out.value == 0 and not counts.any()


def test_soft_malformed_input_keeps_the_three_way_identity(gpu):
    """truncated sequences and lone lead bytes, which byte space and the staged decoder read alike, inside a large body"""
    from latok_amd import batch
    rng = random.Random(0xBAD5)
    body = [t.encode("utf-8") for t in random_strings(rng, 3000, 0, 120, ALPHABETS["mixed"] + EXTRA)]
    blobs = body[:1500] + SOFT + body[1500:] + SOFT
    u8, boff = batch.pack_utf8(blobs)
    assert u8.size > SMALL_CHARS
    for dt in DTYPES:
        got = batch.token_features_utf8_bytes_csr(u8, boff, dtype=dt)
        assert _route() == BYTE_ROUTE
        _three_way(u8, boff, got, dt, ("soft", dt))
        rc, n, dgot, _ = _dev_features(gpu, u8, boff, dt)
        assert rc == 0
        _same(dgot, got, ("soft, device", dt))


def test_hard_malformed_input_is_refused(gpu):
    """a continuation byte without a lead byte in the 3 bytes before it, or at the start of a string: LATOK_ERR_INVALID naming
    malformed UTF-8, no token count, record and sum buffers untouched -- with device and with host pointers"""
    from latok_amd import _lib, batch
    rng = random.Random(0xBAD6)
    body = [t.encode("utf-8") for t in random_strings(rng, 3000, 0, 120, ALPHABETS["mixed"] + EXTRA)]
    for extra in (SOFT + HARD, HARD[:1], HARD[1:]):
        blobs = body[:1500] + extra + body[1500:]
        u8, boff = batch.pack_utf8(blobs)
        assert u8.size > SMALL_CHARS
        for dt in DTYPES:
            rc, n, _, (raw_items, raw_feat) = _dev_features(gpu, u8, boff, dt)
            assert rc == _lib.ERR_INVALID and n == 0 and "malformed UTF-8" in _lib.last_error() and _route() == BYTE_ROUTE
            assert (raw_items == POISON).all() and (raw_feat == POISON).all()
            cap = int(boff[-1])
            counts, spans, feats = np.empty(len(blobs), dt), np.full((cap, 4), 0x7F7F7F7F, dt), np.full((cap, 25), POISON, np.int8)
            n_out = C.c_int64(-1)
            rc = gpu.latok_token_features_utf8_bytes_batch(u8.ctypes.data, boff.ctypes.data, len(blobs), cap, counts.ctypes.data,
                                                           spans.ctypes.data, feats.ctypes.data, cap, C.byref(n_out),
                                                           _lib.OUT_INT32 if dt == np.int32 else 0, None)
            assert rc == _lib.ERR_INVALID and n_out.value == 0 and "malformed UTF-8" in _lib.last_error()
            assert (spans == 0x7F7F7F7F).all() and (feats == POISON).all()
            with pytest.raises(ValueError, match="malformed UTF-8"):
                batch.token_features_utf8_bytes_csr(u8, boff, dtype=dt)
        # where the header sends such input: byte ranges without sums, code-point results through the staged decoder
        batch.token_spans_utf8_bytes_csr(u8, boff)
        batch.token_features_utf8_csr(u8, boff)
    # a small batch that is malformed is refused as well (the host decoder leaves it to the device)
    u8, boff = batch.pack_utf8([b"fine", HARD[0], b"tail"])
    with pytest.raises(ValueError, match="malformed UTF-8"):
        batch.token_features_utf8_bytes_csr(u8, boff)


def test_long_tokens(gpu):
    rng = random.Random(4243)
    n = 1_000_000
    body = "".join(rng.choice("abcdefghXYZ019_") for _ in range(n))
    docs = [body, "see http://" + body[:n - 11], "http://" + body[:n - 7],
            "x " * 10 + "a@" + body[:300000] + "/.:" + body[:200000] + " tail",
            "é" * 5000 + "@" + "日" * 200000 + " end", "🤓" * 300000]
    _check(docs, "long documents")
    _check(["short one", docs[4], "", docs[0][:5000] + " x", docs[5], "tail #tag"], "long documents among short ones")


def test_a_tile_of_two_rounds_and_long_tokens_through_device_pointers(gpu):
    """The byte route at a small size (device pointers) against the host-decoded result of the same batch: 2048 tokens in one
    4096-byte tile (two rounds of its wave), then one string over several tiles whose tokens end in the next word and beyond it."""
    from latok_amd import batch
    runs = ["".join(chr(97 + (i + j * j) % 26) for j in range(n)) for i, n in enumerate((70, 127, 129, 200, 3000, 5000))]
    u8, boff = _check(["a " * 2048, " ".join(runs), "xy", ""], "two rounds", route=HOST_DECODE)
    for dt in DTYPES:
        want = batch.token_features_utf8_bytes_csr(u8, boff, dtype=dt)
        assert want[0].tolist() == [2048, 6, 1, 0]
        rc, n, got, _ = _dev_features(gpu, u8, boff, dt)
        assert rc == 0 and n == 2055 and _route() == BYTE_ROUTE
        _same(got, want, ("two rounds, device batch", dt))


def test_edges_of_words_tiles_and_workgroups(gpu):
    text = _edge_text()
    assert len(text.encode()) > 6 * 65536
    cuts = [0, 1000, 70001, 140003, 300007, len(text)]
    for texts in ([text], [text[a:b] for a, b in zip(cuts[:-1], cuts[1:])]):
        _check(texts, "edges")
    # a mixed prefix of exactly 16 tiles whose lead count is / is not a multiple of 64, then 3 x 65 536 + 37 ASCII bytes
    for e in (640, 641):
        a = 65536 - 2 * e
        rng = random.Random(e + 7)
        chars = ["é"] * e + [rng.choice("abc d.@") for _ in range(a)]
        rng.shuffle(chars)
        prefix = "".join(chars)
        assert len(prefix.encode()) == 65536 and (len(prefix) % 64 == 0) == (e == 640)
        tail = ("lorem ipsum #x a@b.c " * 10000)[:3 * 65536 + 37]
        for texts in ([prefix + tail], [prefix, tail], [prefix[:100], prefix[100:] + tail[:5000], tail[5000:]]):
            _check(texts, ("dense", e))


def test_unicode_sweep(gpu):
    cps = np.arange(0x110000, dtype=np.uint32)
    text = cps.astype("<u4").tobytes().decode("utf-32-le", "surrogatepass")
    texts = [text[i:i + 997] for i in range(0, len(text), 997)]
    _check(texts, "all code points")


def test_large_all_ascii_batch(gpu):
    """one byte per char: the byte records must BE the code-point records"""
    from latok_amd import batch
    rng = random.Random(0xA5D)
    texts = random_strings(rng, 6000, 0, 200, ALPHABETS["words"] + list("ABC,.:/!19\t"))
    assert sum(map(len, texts)) > 4 * 65536
    u8, boff = _check(texts, "ASCII")
    for dt in DTYPES:
        _same(batch.token_features_utf8_bytes_csr(u8, boff, dtype=dt), batch.token_features_utf8_csr(u8, boff, dtype=dt), ("ASCII", dt))


@pytest.mark.parametrize("name", ["sym_everywhere", "all_columns"])
def test_runtime_rule_tables(gpu, name):
    from latok_amd import batch
    rng = random.Random(0x5E8)
    texts = random_strings(rng, 8000, 0, 80, ALPHABETS["mixed"] + EXTRA)
    assert len("".join(texts).encode()) > SMALL_CHARS
    batch.set_rules(*RULE_SETS[name])
    try:
        _check(texts, name)
    finally:
        batch.reset_rules()


def test_small_batches_whatever_route_they_take(gpu):
    """one string; a few hundred strings of at most kSmallChars bytes (host pointers: decoded by the host, positions mapped back);
    the same through device pointers; a small batch the host decoder refuses (soft-malformed): the byte route at a small size"""
    from latok_amd import batch
    _check(["featurize é日🤓 me@x.org http://a.b #tag  "], "one string", route=HOST_DECODE)
    _check(["  "], "one whitespace string", route=HOST_DECODE)
    _check(["🤓"], "one char", route=HOST_DECODE)
    rng = random.Random(78)
    texts = ["", ""] + random_strings(rng, 500, 0, 100, ALPHABETS["mixed"] + EXTRA) + [""]
    u8, boff = _check(texts, "a few hundred strings", route=HOST_DECODE)
    assert u8.size <= SMALL_CHARS
    for dt in DTYPES:
        want = batch.token_features_utf8_bytes_csr(u8, boff, dtype=dt)
        rc, n, got, _ = _dev_features(gpu, u8, boff, dt)
        assert rc == 0 and n == want[1].shape[0] and _route() == BYTE_ROUTE
        _same(got, want, ("small device batch", dt))
        _three_way(u8, boff, got, dt, ("small device batch", dt))
    blobs = [t.encode("utf-8") for t in texts[:200]] + SOFT
    u8, boff = batch.pack_utf8(blobs)
    for dt in DTYPES:
        got = batch.token_features_utf8_bytes_csr(u8, boff, dtype=dt)
        assert _route() == BYTE_ROUTE
        _three_way(u8, boff, got, dt, ("small soft-malformed batch", dt))
    # an unaligned device pointer is refused, as in the other byte-space calls
    from latok_amd import _lib
    d = gpu.latok_dev_alloc(4096)
    try:
        n = C.c_int64(0)
        rc = gpu.latok_token_features_utf8_bytes_batch(d + 1 + 1024, d, 1, 16, d + 2048, d + 3072, d + 512, 1, C.byref(n), _lib.DEVICE_PTRS, None)
        assert rc == _lib.ERR_INVALID and "aligned" in _lib.last_error()
    finally:
        gpu.latok_dev_free(d)


def test_featurize_utf8_bytes_batch_matches_featurize_utf8_batch(gpu):
    from latok_amd import batch
    rng = random.Random(10)
    texts = ["", "x"] + random_strings(rng, 4000, 0, 100, ALPHABETS["mixed"] + EXTRA) + [""]
    blobs = [t.encode("utf-8", "surrogatepass") for t in texts]
    assert sum(map(len, blobs)) > SMALL_CHARS
    for sel in (slice(None), slice(0, 3), slice(0, 0)):
        got = batch.featurize_utf8_bytes_batch(blobs[sel])
        want = batch.featurize_utf8_batch(blobs[sel])
        assert len(got) == len(want) == len(blobs[sel])
        for blob, g, w in zip(blobs[sel], got, want):
            text = blob.decode("utf-8", "surrogatepass")
            assert len(g) == len(w)
            for x, y in zip(g, w):
                assert isinstance(x.text, bytes) and x.text == y.text.encode("utf-8", "surrogatepass")
                assert np.array_equal(x.features, y.features)
                assert blob[x.start_idx:x.end_idx].decode("utf-8", "surrogatepass") == text[y.start_idx:y.end_idx]
