"""Every path of feature_tile (k_features_tiles, latok_amd/csrc/feature_kernels.hip) against the oracle.

tests/helpers/featurize_content.py plants, and names, what the kernel does differently from tile to tile: the word-major and the
token-major form on both sides of the form threshold, window rounds of either form and the int64 span rounds that are out of step
with them, a round that ends inside a word (low half, straddling token, high half), every alignment of flush_records, tokens that
leave their word and end in a later word, in the next tile's first word, or one to three whole-wave steps away, string ends that
only the carried string-start bits can tell the planes about, the batch tail, runs of empty strings, tiles without a token start,
sums that wrap, multi-byte text under the byte-space records.  tests/test_featurize_content.py proves on the CPU that the batches
reach every class; here each batch goes through every featurize form and is compared with the reference (the oracle alone) exactly
and in full: counts, spans4, the 25 sums, int64 and int32 records.  Each call asserts its route; test_zz_coverage asserts that every
(form, class) pair was reached.

What the classes are worth was measured once with single-value changes to the kernel, each of which fails here with the token, its
tile, word and bit, the columns and the class in the message: `Bn65` reduced to its first bit (STR_END:TILE+4161, AFTER_NEXT_ALPHA
one too high) and `Bnw` without its `rel == 65` term (STR_END:WALK_WORD_OFFSET_1) pass every earlier test of the suite; `h65.prev = 0`,
the straddling token's record one slot up and the token-major carry added to every token of a word fail here and in earlier tests.
Two changes cannot show in any result and are not asked of this module: a 16-byte head in flush_records for an aligned destination
copies the same bytes, and an int64 span round as long as the feature round differs only by writing past the window."""
import os
import sys

import numpy as np
import pytest

HELPERS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers")
sys.path.insert(0, HELPERS)
import featurize_content as fc  # noqa: E402
from test_gpu_flow_utf8 import _Arena  # noqa: E402
from test_gpu_span_strip import DTYPES, POISON, _dev, _host_route, _plan, _route  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ("main", "mid", "tail1", "tail63", "tail64", "tail65", "tail4095", "tail0")
KIND = {4: ("utf32", "full"), 1: ("kind1", "latin1"), 2: ("kind2", "bmp")}
REACHED = set()      # (form, class)
# forms that take batches of any size, and forms that only take small ones (featurize_content.REQUIRED_SMALL)
BIG = ("utf32_host", "utf32_device", "kind1", "kind2", "utf8_code_points_route3", "utf8_bytes_route4", "flow_utf32", "flow_utf8_code_points",
       "flow_utf8_bytes", "python")
SMALL = ("utf32_pinned", "utf8_code_points_route1", "utf8_code_points_route2", "utf8_bytes_host_decoded")
_CACHE = {}


def _lim():
    if "lim" not in _CACHE:
        _CACHE["lim"] = fc.limits()
    return _CACHE["lim"]


def _work(oracle, rg, name, padded=False, unit="chars"):
    """(strings, reference, classes) of a batch; padded: behind more than kSmallChars bytes of ordinary text, a whole number of tiles"""
    key = (rg, name, padded, unit)
    if key not in _CACHE:
        if len(_CACHE) > 12:
            lim = _CACHE["lim"]
            _CACHE.clear()
            _CACHE["lim"] = lim
        texts = fc.batches(_lim(), rg)[name]
        if padded:
            texts = fc.padding(_lim()) + texts
        r = fc.reference(oracle, texts, None, unit)
        _CACHE[key] = (texts, r, fc.census(oracle, texts, None, _lim(), r))
    return _CACHE[key]


def _check(got, r, dt, what):
    counts, spans4, feats = got
    ok = counts.dtype == dt and spans4.dtype == dt and feats.dtype == np.int8 and np.array_equal(counts, r.counts) and \
        spans4.shape == r.spans4.shape and feats.shape == r.feats.shape and np.array_equal(spans4, r.spans4) and np.array_equal(feats, r.feats)
    if not ok:
        raise AssertionError("%s: %s" % (what, fc.first_diff(got, r, _lim())))


def _note(form, classes):
    REACHED.update((form, c) for c in classes)


def _enc(texts):
    from latok_amd import batch
    return batch.pack_utf8([t.encode("utf-8") for t in texts])


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("kind", (4, 1, 2))
def test_code_unit_forms(gpu, oracle, kind, name):
    """UTF-32 with host and with device pointers, PEP 393 kind 1 and kind 2 with host pointers; the small batches also behind padding"""
    from latok_amd import batch
    form, rg = KIND[kind]
    for padded in ((False,) if name == "main" else (False, True)):
        texts, r, classes = _work(oracle, rg, name, padded)
        cps, row = fc.pack(texts)
        units = cps if kind == 4 else cps.astype(np.uint8 if kind == 1 else np.uint16)
        route = _host_route(r.total, r.n_str)
        tiles = (r.total + fc.TILE - 1) // fc.TILE
        assert route == ("staged" if padded or name == "main" else "pinned")
        ar = _Arena(gpu)
        try:
            d_units, d_row = ar.put(units), ar.put(row)
            for dt in DTYPES:
                what = (form, name, "padded" if padded else "", dt.__name__, route)
                got = batch.token_features_csr(units, row, dtype=dt) if kind == 4 else batch.token_features_kind_csr(units, row, dtype=dt)
                p = _plan()
                assert p[1] == int(route == "pinned") and p[14] == tiles, (what, p)
                _check(got, r, dt, what)
                if kind == 4:
                    rc, n, dgot, _ = _dev(ar, gpu.latok_token_features_batch, [d_units, d_row], r.n_str, r.total, 4, dt, True, len(r.spans4) + 8)
                    p = _plan()
                    assert rc == 0 and n == len(r.spans4) and p[1] == 0 and p[14] == tiles, (what, rc, n, p)
                    _check(dgot, r, dt, what + ("device",))
        finally:
            ar.free()
        _note(form if kind != 4 else "utf32_pinned" if route == "pinned" else "utf32_host", classes)
        if kind == 4:
            _note("utf32_device", classes)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("unit", ("chars", "bytes"))
def test_utf8_forms(gpu, oracle, unit, name):
    """UTF-8 in code-point units (host-decoded route 1, the staged decoder route 2, byte space route 3) and in byte space (route 4:
    the records come from k_counts_scatter<2> in bytes while feature_tile works on the code-point layout)"""
    from latok_amd import batch
    lim = _lim()
    for padded in ((False,) if name == "main" else (False, True)):
        texts, r, classes = _work(oracle, "full", name, padded, unit)
        u8, boff = _enc(texts)
        small = u8.size <= lim["SMALL_CHARS"] and r.n_str <= lim["SMALL_STRINGS"]
        assert small == (not padded and name != "main")
        host_fn, dev_fn = (batch.token_features_utf8_csr, gpu.latok_token_features_utf8_batch) if unit == "chars" else \
                          (batch.token_features_utf8_bytes_csr, gpu.latok_token_features_utf8_bytes_batch)
        host_route = 1 if small else 3 if unit == "chars" else 4
        dev_route = 4 if unit == "bytes" else 2 if u8.size <= lim["SMALL_CHARS"] else 3
        ar = _Arena(gpu)
        try:
            d_u8, d_boff = ar.put(u8), ar.put(boff)
            for dt in DTYPES:
                what = ("utf8", unit, name, "padded" if padded else "", dt.__name__)
                got = host_fn(u8, boff, dtype=dt)
                assert _route() == host_route, (what, _route())
                _check(got, r, dt, what + ("host", host_route))
                rc, n, dgot, _ = _dev(ar, dev_fn, [d_u8, d_boff], r.n_str, int(boff[-1]), 4, dt, True, len(r.spans4) + 8)
                assert rc == 0 and n == len(r.spans4) and _route() == dev_route, (what, rc, n, _route())
                _check(dgot, r, dt, what + ("device", dev_route))
        finally:
            ar.free()
        for route in (host_route, dev_route):
            _note(("utf8_code_points_route%d" % route) if unit == "chars" else "utf8_bytes_route4" if route == 4 else "utf8_bytes_host_decoded", classes)


@pytest.mark.parametrize("name", NAMES)
def test_batch_flow(gpu, oracle, name):
    """UTF-32, UTF-8 in code points and UTF-8 in bytes through the batch flow, int32 records, two different batches in flight"""
    from latok_amd import batch
    dt = np.int32
    pair = [("full", name, name != "main"), ("full", "mid" if name == "main" else name, False)]
    ar = _Arena(gpu)
    try:
        jobs = []
        for form in ("utf32", "utf8_code_points", "utf8_bytes"):
            for rg, nm, padded in pair:
                texts, r, classes = _work(oracle, rg, nm, padded, "bytes" if form == "utf8_bytes" else "chars")
                units, row = fc.pack(texts) if form == "utf32" else _enc(texts)
                n, words = len(r.spans4), 2 if form == "utf32" else 4
                o = (ar.alloc(r.n_str * 4, POISON), ar.alloc(n * 16, POISON), ar.alloc(n * 25, POISON), ar.alloc(8 * words, POISON))
                args = (ar.put(units), ar.put(row), r.n_str, int(row[-1]), o[0], o[1], o[2], n, o[3])
                if form == "utf32":
                    batch.flow_token_features(args[0], 4, *args[1:], dtype=dt)
                elif form == "utf8_code_points":
                    batch.flow_token_features_utf8(*args, dtype=dt)
                else:
                    batch.flow_token_features_utf8_bytes(*args, dtype=dt)
                jobs.append((form, nm, padded, r, classes, o, words))
        batch.flow_wait()
        for form, nm, padded, r, classes, o, words in jobs:
            n = len(r.spans4)
            res = ar.get(o[3], words, np.int64)
            assert res[0] == n and res[1] == 0 and (words == 2 or (res[2] == r.total_chars and res[3] == 0)), (form, nm, res)
            got = (ar.get(o[0], r.n_str, dt), ar.get(o[1], (n, 4), dt), ar.get(o[2], (n, 25), np.int8))
            _check(got, r, dt, ("flow", form, nm, "padded" if padded else ""))
            _note("flow_" + form, classes)
    finally:
        ar.free()


@pytest.mark.parametrize("name", NAMES)
def test_python_featurize_batch(gpu, oracle, name):
    """latok_amd.batch.featurize_batch: the tokens as strings, raw positions and sums"""
    from latok_amd import batch
    texts, r, classes = _work(oracle, "full", name)
    got = batch.featurize_batch(texts)
    assert len(got) == len(texts) and [len(g) for g in got] == r.counts.tolist()
    k = 0
    for t, toks in zip(texts, got):
        for tok in toks:
            a, b, c, d = r.spans4[k].tolist()
            assert tok.text == t[c:d] and (tok.start_idx, tok.end_idx) == (a, b) and np.array_equal(tok.features, r.feats[k]), (name, k)
            k += 1
    assert k == len(r.spans4)
    _note("python", classes)


def _module_case_count():
    n = 0
    for name, f in globals().items():
        if name.startswith("test_") and name != "test_zz_coverage" and callable(f):
            k = 1
            for m in getattr(f, "pytestmark", []):
                if m.name == "parametrize":
                    k *= len(m.args[1])
            n += k
    return n


def test_zz_coverage(request):
    """every (form, class) pair was reached (runs last; a -k subset of the module skips it)"""
    from latok_amd import batch
    here = [it for it in request.session.items if it.module is not None and it.module.__name__ == __name__ and it.originalname != "test_zz_coverage"]
    if len(here) < _module_case_count():
        pytest.skip("coverage is asserted over the whole module; only a subset of it was selected")
    want = {(f, c) for f in BIG for c in fc.REQUIRED} | {(f, c) for f in SMALL for c in fc.REQUIRED_SMALL}
    missing = sorted(want - REACHED)
    print("forms:", sorted({f for f, _ in REACHED}), "pairs:", len(REACHED & want), "of", len(want))
    assert not missing, ("(form, class) pairs not reached:", missing)
    assert not batch.rules_active()
