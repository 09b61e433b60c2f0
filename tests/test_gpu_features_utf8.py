"""featurize of UTF-8 batches in code-point units (latok_token_features_utf8_batch): large well-formed batches take byte space
and the rule codes k_lead_codes stores at the lead bytes (route 3, no UTF-32 copy), everything else the existing decode routes.
Every result must be what latok_token_features_batch gives for the decoded text -- counts, spans4 and the 25 sums, int64 and
int32 records -- and, for the parity corpus, what the oracle's parse matrix summed over its own token spans gives."""
import ctypes as C
import random

import numpy as np
import pytest

from conftest import ALPHABETS, RULE_SETS, pack, random_strings
from helpers import utf8_ref

pytestmark = pytest.mark.gpu

SMALL_CHARS = 262144   # api.cpp: kSmallChars (batches above it take byte space)
DTYPES = (np.int64, np.int32)
EXTRA = list("é日🤓ü　Жδ") + ["http://a.b/c?d=1", "see me@x.org", "#tag", ".@you", "a@b.c"]


def _route():
    from latok_amd import _lib
    return _lib.load().latok_debug_last_route()


def _enc(texts):
    from latok_amd import batch
    return batch.pack_utf8([t.encode("utf-8", "surrogatepass") for t in texts])


def _same(a, b, what=""):
    assert len(a) == len(b) == 3
    for x, y, name in zip(a, b, ("counts", "spans4", "features")):
        assert x.shape == y.shape and np.array_equal(x, y), (what, name)


def _dev_features(lib, u8, boff, dt, total=-1, cap=None):
    """the entry point with device pointers (byte count read by the library when total = -1) -> (rc, n, counts, spans4, feats)"""
    from latok_amd import _lib
    n_str = boff.size - 1
    isz = np.dtype(dt).itemsize
    flags = _lib.DEVICE_PTRS | (_lib.OUT_INT32 if dt == np.int32 else 0)
    cap = max(int(boff[-1]), 1) if cap is None else cap
    d_u8, d_boff = lib.latok_dev_alloc(u8.nbytes + 64), lib.latok_dev_alloc(boff.nbytes)
    d_counts, d_items, d_feat = lib.latok_dev_alloc(n_str * isz + 16), lib.latok_dev_alloc(cap * 4 * isz + 16), lib.latok_dev_alloc(cap * 25 + 16)
    assert d_u8 and d_boff and d_counts and d_items and d_feat
    try:
        if u8.nbytes:
            _lib.check(lib.latok_memcpy_h2d(d_u8, u8.ctypes.data, u8.nbytes))
        _lib.check(lib.latok_memcpy_h2d(d_boff, boff.ctypes.data, boff.nbytes))
        n = C.c_int64(0)
        rc = lib.latok_token_features_utf8_batch(d_u8, d_boff, n_str, total, d_counts, d_items, d_feat, cap, C.byref(n), flags, None)
        counts = np.empty(n_str, dt)
        spans = np.empty((n.value, 4), dt)
        feats = np.empty((n.value, 25), np.int8)
        if rc == 0:
            _lib.check(lib.latok_memcpy_d2h(counts.ctypes.data, d_counts, counts.nbytes))
            _lib.check(lib.latok_memcpy_d2h(spans.ctypes.data, d_items, spans.nbytes))
            _lib.check(lib.latok_memcpy_d2h(feats.ctypes.data, d_feat, feats.nbytes))
        return rc, n.value, (counts, spans, feats)
    finally:
        for p in (d_u8, d_boff, d_counts, d_items, d_feat):
            lib.latok_dev_free(p)


def _oracle_raw(oracle, texts):
    """counts, raw spans and feature sums of the kept tokens: the oracle's parse matrix summed over its split_offsets spans"""
    counts, spans, feats = [], [], []
    for t in texts:
        k = 0
        if t:
            m = oracle.gen_parse_matrix(t).astype(np.uint8)
            csum = np.zeros((len(t) + 1, 25), np.uint64)
            np.cumsum(m, axis=0, dtype=np.uint64, out=csum[1:])
            nz = oracle.split_offsets(t).tolist() + [len(t)]
            for a, b in zip(nz[:-1], nz[1:]):
                if t[a:b].strip():
                    spans.append((a, b))
                    feats.append((csum[b] - csum[a]).astype(np.uint8).astype(np.int8))
                    k += 1
        counts.append(k)
    return np.array(counts), np.array(spans, np.int64).reshape(-1, 2), np.array(feats, np.int8).reshape(-1, 25)


def _check_against_utf32(texts, what, route=3):
    """host call, both record widths: equal to the UTF-32 entry point on the same text; the route the call took"""
    from latok_amd import batch
    u8, boff = _enc(texts)
    cps, row = pack(texts)
    for dt in DTYPES:
        got = batch.token_features_utf8_csr(u8, boff, dtype=dt)
        assert _route() == route, (what, dt)
        _same(got, batch.token_features_csr(cps, row, dtype=dt), (what, dt))
    return u8, boff


def test_oracle_parity_host_and_device(gpu, oracle):
    from latok_amd import _lib, batch
    rng = random.Random(0xF8)
    texts = [""] + random_strings(rng, 4000, 0, 90, ALPHABETS["mixed"] + EXTRA) + [""]
    u8, boff = _enc(texts)
    assert u8.size > SMALL_CHARS
    cps, row = pack(texts)
    w_counts, w_raw, w_feats = _oracle_raw(oracle, texts)
    for dt in DTYPES:
        want = batch.token_features_csr(cps, row, dtype=dt)
        got = batch.token_features_utf8_csr(u8, boff, dtype=dt)
        assert _route() == 3
        _same(got, want, ("host", dt))
        assert np.array_equal(got[0], w_counts) and np.array_equal(got[1][:, :2], w_raw) and np.array_equal(got[2], w_feats)
        rc, n, dgot = _dev_features(gpu, u8, boff, dt)
        assert rc == 0 and n == want[1].shape[0] and _route() == 3
        _same(dgot, want, ("device", dt))
        # capacity protocol: one token short is refused and reports the count it needs; cap = 0 is a size query
        rc, n, _ = _dev_features(gpu, u8, boff, dt, total=int(boff[-1]), cap=want[1].shape[0] - 1)
        assert rc == _lib.ERR_INVALID and n == want[1].shape[0]
        counts, n_out = np.empty(len(texts), dt), C.c_int64(0)
        flags = _lib.OUT_INT32 if dt == np.int32 else 0
        rc = gpu.latok_token_features_utf8_batch(u8.ctypes.data, boff.ctypes.data, len(texts), int(boff[-1]), counts.ctypes.data,
                                                 None, None, 0, C.byref(n_out), flags, None)
        assert rc == _lib.ERR_INVALID and n_out.value == want[1].shape[0] and np.array_equal(counts, want[0])
    # no strings at all
    n_out = C.c_int64(7)
    z = np.zeros(1, np.int64)
    assert gpu.latok_token_features_utf8_batch(None, z.ctypes.data, 0, 0, None, None, None, 0, C.byref(n_out), 0, None) == 0
    assert n_out.value == 0


def test_long_tokens(gpu):
    rng = random.Random(4242)
    n = 1_000_000
    body = "".join(rng.choice("abcdefghXYZ019_") for _ in range(n))
    docs = [body, "see http://" + body[:n - 11], "http://" + body[:n - 7],
            "x " * 10 + "a@" + body[:300000] + "/.:" + body[:200000] + " tail",
            "é" * 5000 + "@" + "日" * 200000 + " end", "🤓" * 300000]
    _check_against_utf32(docs, "long documents")
    _check_against_utf32(["short one", docs[4], "", docs[0][:5000] + " x", docs[5], "tail #tag"], "long documents among short ones")


def _edge_text():
    """multi-byte chars across 64-byte word, 4096-byte tile and 65 536-byte workgroup boundaries: every split of a 2-, 3- and
    4-byte char (the boundary j bytes after its lead, j = 1 .. length - 1) lands on each kind of boundary"""
    splits = [(ch, j) for ch in ("é", "日", "🤓") for j in range(1, len(ch.encode()))]
    parts, nbytes, seen = [], 0, {}
    filler = "ab cd.e f@g "
    bounds = sorted({64 * k for k in range(1, 200)} | {4096 * k for k in range(1, 40)} | {65536 * k for k in range(1, 7)})
    for B in bounds:
        kind = 65536 if B % 65536 == 0 else (4096 if B % 4096 == 0 else 64)
        ch, j = splits[seen.get(kind, 0) % len(splits)]
        seen[kind] = seen.get(kind, 0) + 1
        pad = B - j - nbytes
        parts.append((filler * (pad // len(filler) + 1))[:pad])
        parts.append(ch)
        nbytes = B - j + len(ch.encode())
    return "".join(parts) + "end"


def test_edges_of_words_tiles_and_workgroups(gpu):
    from latok_amd import batch
    text = _edge_text()
    assert len(text.encode()) > 6 * 65536
    # one string, then the same text cut into strings at places that are not on any boundary
    cuts = [0, 1000, 70001, 140003, 300007, len(text)]
    for texts in ([text], [text[a:b] for a, b in zip(cuts[:-1], cuts[1:])]):
        _check_against_utf32(texts, "edges")
    # a mixed prefix of exactly 16 tiles (one workgroup of k_lead_compress / k_lead_codes) whose lead count is / is not a multiple
    # of 64, then 3 x 65 536 + 37 ASCII bytes (the dense workgroups behind it; the batch stays above the small-batch size)
    for e in (640, 641):
        a = 65536 - 2 * e
        rng = random.Random(e)
        chars = ["é"] * e + [rng.choice("abc d.@") for _ in range(a)]
        rng.shuffle(chars)
        prefix = "".join(chars)
        assert len(prefix.encode()) == 65536 and (len(prefix) % 64 == 0) == (e == 640)
        tail = ("lorem ipsum #x a@b.c " * 10000)[:3 * 65536 + 37]
        for texts in ([prefix + tail], [prefix, tail], [prefix[:100], prefix[100:] + tail[:5000], tail[5000:]]):
            u8, boff = _check_against_utf32(texts, ("dense", e))
            cps, row = pack(texts)
            for dt in DTYPES:
                c1, s1 = batch.token_spans_utf8_csr(u8, boff, dtype=dt)
                c2, s2 = batch.token_spans_csr(cps, row, dtype=dt)
                assert np.array_equal(c1, c2) and np.array_equal(s1, s2)


def test_unicode_sweep(gpu):
    cps = np.arange(0x110000, dtype=np.uint32)
    text = cps.astype("<u4").tobytes().decode("utf-32-le", "surrogatepass")
    texts = [text[i:i + 997] for i in range(0, len(text), 997)]
    _check_against_utf32(texts, "all code points")


@pytest.mark.parametrize("name", ["sym_everywhere", "all_columns"])
def test_runtime_rule_tables(gpu, name):
    from latok_amd import batch
    rng = random.Random(0x5E7)
    texts = random_strings(rng, 8000, 0, 80, ALPHABETS["mixed"] + EXTRA)
    assert len("".join(texts).encode()) > SMALL_CHARS
    batch.set_rules(*RULE_SETS[name])
    try:
        _check_against_utf32(texts, name)
    finally:
        batch.reset_rules()


def test_malformed_input_equals_the_staged_decoder(gpu):
    from latok_amd import batch
    rng = random.Random(0xBAD)
    body = [t.encode("utf-8") for t in random_strings(rng, 3000, 0, 120, ALPHABETS["mixed"] + EXTRA)]
    # cut-short sequences and lone leads that both models read alike: the batch stays in byte space
    soft = [b"ab\xe6\x97 cd", b"\xc3 x", b"lone \xf0\x9f\x98", b"end\xe6", b"next starts ascii", b"\xe6\x97\xa5\xe6", b"\xf0", b"x\xc3"]
    # continuation bytes without a lead within 3 bytes before them, and a string that begins with one: the staged decoder
    hard = [b"a\x80\x80\x80\x80b", b"\xa9 starts with a continuation byte"]
    for extra, route in ((soft, 3), (soft + hard, 2)):
        blobs = body[:1500] + extra + body[1500:] + extra
        u8, boff = batch.pack_utf8(blobs)
        assert u8.size > SMALL_CHARS
        cps, row = batch.utf8_decode_csr(u8, boff)
        want_cps, want_row, _ = utf8_ref.decode_batch(u8, boff)        # the decoder's output is the rule's before it is the expectation
        assert np.array_equal(cps, want_cps) and np.array_equal(row, want_row), route
        for dt in DTYPES:
            got = batch.token_features_utf8_csr(u8, boff, dtype=dt)
            assert _route() == route, (route, dt)
            _same(got, batch.token_features_csr(cps, row, dtype=dt), (route, dt))


def test_small_and_mid_batches_keep_their_routes(gpu):
    from latok_amd import batch
    one = ["featurize é日🤓 me@x.org http://a.b #tag  "]
    _check_against_utf32(one, "one string", route=1)
    rng = random.Random(77)
    texts = random_strings(rng, 500, 0, 100, ALPHABETS["mixed"] + EXTRA)
    u8, boff = _enc(texts)
    assert u8.size <= SMALL_CHARS
    cps, row = pack(texts)
    for dt in DTYPES:
        rc, n, got = _dev_features(gpu, u8, boff, dt)
        assert rc == 0 and _route() == 2
        _same(got, batch.token_features_csr(cps, row, dtype=dt), ("mid device batch", dt))


def test_large_all_ascii_batch(gpu):
    rng = random.Random(0xA5C)
    texts = random_strings(rng, 6000, 0, 200, ALPHABETS["words"] + list("ABC,.:/!19\t"))
    assert sum(map(len, texts)) > 4 * 65536
    _check_against_utf32(texts, "ASCII")


def test_featurize_utf8_batch_matches_featurize_batch(gpu):
    from latok_amd import batch
    rng = random.Random(9)
    texts = ["", "x"] + random_strings(rng, 4000, 0, 100, ALPHABETS["mixed"] + EXTRA) + [""]
    blobs = [t.encode("utf-8", "surrogatepass") for t in texts]
    assert sum(map(len, blobs)) > SMALL_CHARS
    for sel in (slice(None), slice(0, 3), slice(0, 0)):
        got = batch.featurize_utf8_batch(blobs[sel])
        want = batch.featurize_batch([b.decode("utf-8", "surrogatepass") for b in blobs[sel]])
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert [(x.text, x.start_idx, x.end_idx) for x in g] == [(x.text, x.start_idx, x.end_idx) for x in w]
            assert all(np.array_equal(x.features, y.features) for x, y in zip(g, w))
