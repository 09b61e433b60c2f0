"""Strip and drop of the span and featurize kernels where only caller-installed rule tables can take them: tokens with long
leading / trailing whitespace runs and whitespace-only tokens of any length, planted at chosen bit, word, tile, string and batch
edges (tests/helpers/span_strip_content.py; tests/test_span_strip_content.py proves on the CPU which classes the content reaches).
Under the built-in tables a kept token has at most one leading whitespace char and a dropped one is one char long, so the kernels'
branches for longer extents never run there.

Every input form and route is compared with the reference (oracle boundaries, str.strip, parse-matrix sums) exactly and in full:
counts, span records, spans4 records, the 25 sums and the item total, int64 and int32 records.  Each case asserts the route it was
built for; the last test asserts that the module as a whole reached every route and form."""
import contextlib
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, pack

HELPERS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers")
sys.path.insert(0, HELPERS)
import span_strip_content as ssc  # noqa: E402
from test_gpu_features_utf8_bytes import _three_way  # noqa: E402
from test_gpu_flow_utf8 import _Arena, _Job  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = (np.int64, np.int32)
POISON = 0x7F
TABLE_NAMES = sorted(ssc.TABLES)
FORM = {4: ("utf32", "full"), 1: ("kind1", "latin1"), 2: ("kind2", "bmp")}      # PEP 393 kind -> form name, range of the content
BUILT_FOR = {"small": "one_launch", "mid": "pinned", "large": "staged"}
REACHED = set()      # (form, route) pairs, noted where a case has asserted its route
EXPECTED = {(f, r) for f in ("utf32", "kind1", "kind2") for r in ("one_launch", "pinned", "staged", "device", "pipeline", "flow")} | \
           {("utf8_bytes", r) for r in ("spans_host_decoded", "spans_own_units", "spans_device", "features_host_decoded", "features_route4_host",
                                        "features_route4_device", "flow_spans", "flow_features", "three_way", "pipeline")} | \
           {("utf8_code_points", r) for r in ("route1", "route2", "route3", "flow_mask", "flow_offsets", "flow_spans", "flow_features")} | \
           {("python", r) for r in ("tokenize_batch", "featurize_batch", "featurize_utf8_batch", "featurize_utf8_bytes_batch")} | \
           {("capacity", f) for f in ("utf32", "kind1", "kind2", "utf8_bytes", "utf8_code_points")}


def _hook(name, *argtypes):
    from latok_amd import _lib
    fn = getattr(_lib.load(), name)
    fn.restype, fn.argtypes = C.c_int, list(argtypes)
    return fn


def _limits():
    """kTile, kSmallChars, kSmallStrings of the library"""
    out = np.zeros(9, np.int64)
    assert _hook("latok_debug_limits", C.c_void_p, C.c_int)(out.ctypes.data, 9) == 9
    assert out[0] == ssc.TILE and out[6] == ssc.SMALL_CHARS
    return int(out[0]), int(out[6]), int(out[7])


def _plan():
    """latok_debug_last_plan: [1] = the `small` word (a host batch ran in place on pinned memory), [14] = tiles of the last pipeline"""
    out = np.zeros(15, np.int64)
    assert _hook("latok_debug_last_plan", C.c_void_p, C.c_int)(out.ctypes.data, 15) == 15
    return out.tolist()


def _route():
    return _hook("latok_debug_last_route")()


@contextlib.contextmanager
def _rules(table):
    from latok_amd import batch
    batch.set_rules(*ssc.TABLES[table])
    try:
        assert batch.rules_active()
        yield
    finally:
        batch.reset_rules()


_CACHE = {}


def _content(oracle, table, size, unit, rg="full", ref_unit=None):
    """[(texts, reference)] of a size; ref_unit: the reference in another unit than the content was laid out in"""
    key = (table, size, unit, rg, ref_unit or unit)
    if key not in _CACHE:
        if len(_CACHE) >= 4:
            _CACHE.clear()
        _CACHE[key] = [(texts, ssc.reference(oracle, texts, ssc.TABLES[table], ref_unit or unit)) for texts in ssc.content(table, size, unit, rg)]
    return _CACHE[key]


def _units(texts, kind):
    cps, row = pack(texts)
    return (cps if kind == 4 else cps.astype(np.uint8 if kind == 1 else np.uint16)), row


def _enc(texts):
    from latok_amd import batch
    return batch.pack_utf8([t.encode("utf-8") for t in texts])


def _host_route(total, n_str):
    tile, small_chars, small_strings = _limits()
    return "one_launch" if total <= tile and n_str <= small_strings else "pinned" if total <= small_chars and n_str <= small_strings else "staged"


def _prime():
    """a three-tile host call, so that the plan of the last tile pipeline is known not to be the next call's"""
    from latok_amd import batch
    batch.split_mask_batch(*pack(["ab " * 4000]))
    p = _plan()
    assert p[14] == 3 and p[1] == 1
    return p


def _dev(ar, fn, lead, n_str, total, width, dt, feats, cap):
    """fn(*lead, n_str, total, counts, records[, sums], cap, &n, flags, NULL) with device pointers and poisoned outputs
    -> rc, n, (counts, records, sums), every byte of the record and sum buffers"""
    from latok_amd import _lib
    isz = np.dtype(dt).itemsize
    room = max(cap, 1)
    d_counts, d_items = ar.alloc(n_str * isz, POISON), ar.alloc(room * width * isz, POISON)
    d_feat = ar.alloc(room * 25, POISON) if feats else None
    n = C.c_int64(-1)
    flags = _lib.DEVICE_PTRS | (_lib.OUT_INT32 if dt == np.int32 else 0)
    rc = fn(*(list(lead) + [n_str, total, d_counts, d_items] + ([d_feat] if feats else []) + [cap, C.byref(n), flags, None]))
    k = n.value if rc == 0 else 0
    got = (ar.get(d_counts, n_str, dt), ar.get(d_items, (k, width), dt), ar.get(d_feat, (k, 25), np.int8) if feats else None)
    raw = (ar.get(d_items, room * width * isz, np.uint8), ar.get(d_feat, room * 25, np.uint8) if feats else np.zeros(0, np.uint8))
    return rc, n.value, got, raw


def _flow_pair(gpu, pair, put, submit, forms, res_words, what):
    """the batches of `pair` in flight together, every (form, record width) of each: submit(form, d_units, d_row, r, d_counts, d_items,
    d_sums, cap, d_res, dt) enqueues one; the results are read after one flow_wait"""
    from latok_amd import batch
    ar = _Arena(gpu)
    try:
        per_batch = []
        for texts, r in pair:
            units, row = put(texts)
            d_units, d_row = ar.put(units), ar.put(row)
            jobs = []
            for dt in DTYPES:
                for form in forms:
                    isz, w, cap = np.dtype(dt).itemsize, 4 if form == "features" else 2, len(r.spans) + 8
                    jobs.append((r, dt, form, w, cap, d_units, d_row, ar.alloc(r.n_str * isz, POISON), ar.alloc(cap * w * isz, POISON),
                                 ar.alloc(cap * 25, POISON) if form == "features" else None, ar.alloc(8 * res_words, POISON)))
            per_batch.append(jobs)
        order = [j for js in zip(*per_batch) for j in js]          # A, B, A, B, ...: two different batches in flight
        for r, dt, form, w, cap, d_units, d_row, d_counts, d_items, d_sums, d_res in order:
            submit(form, d_units, d_row, r, d_counts, d_items, d_sums, cap, d_res, dt)
        batch.flow_wait()
        for r, dt, form, w, cap, d_units, d_row, d_counts, d_items, d_sums, d_res in order:
            res = ar.get(d_res, res_words, np.int64)
            assert res[0] == len(r.spans) and res[1] == 0, (what, form, dt, res)
            if res_words == 4:
                assert res[3] == 0 and res[2] == r.total_chars, (what, form, dt, res)
            got = (ar.get(d_counts, r.n_str, dt), ar.get(d_items, (len(r.spans), w), dt),
                   ar.get(d_sums, (len(r.spans), 25), np.int8) if form == "features" else None)
            ssc.compare(got, r, dt, form == "features", what + ("flow", form, dt.__name__))
    finally:
        ar.free()


@pytest.mark.parametrize("kind", (4, 1, 2))
@pytest.mark.parametrize("table", TABLE_NAMES)
def test_code_unit_forms(gpu, oracle, table, kind):
    """UTF-32 and PEP 393 kind 1 / 2 units: the one-launch path, the pinned path, the staged host path, device pointers and the flow"""
    from latok_amd import batch
    form, rg = FORM[kind]
    with _rules(table):
        for size in ssc.SIZES:
            work = _content(oracle, table, size, "chars", rg)
            for i, (texts, r) in enumerate(work):
                units, row = _units(texts, kind)
                route = _host_route(r.total, r.n_str)
                assert i != 0 or route == BUILT_FOR[size]
                tiles = (r.total + ssc.TILE - 1) // ssc.TILE
                ar = _Arena(gpu)
                try:
                    d_units, d_row = ar.put(units), ar.put(row)
                    for dt in DTYPES:
                        for feats in (False, True):
                            what = (table, form, size, "ABCD"[i], dt.__name__, "features" if feats else "spans")
                            before = _prime() if route == "one_launch" else None
                            if kind == 4:
                                got = (batch.token_features_csr if feats else batch.token_spans_csr)(units, row, dtype=dt)
                            else:
                                got = (batch.token_features_kind_csr if feats else batch.token_spans_kind_csr)(units, row, dtype=dt)
                            p = _plan()
                            if route == "one_launch":      # no tile pipeline was launched: the single-wave kernel did all of it
                                assert p == before, (what, p)
                            else:
                                assert p[1] == int(route == "pinned") and p[14] == tiles, (what, route, p)
                            ssc.compare(got, r, dt, feats, what + (route,))
                            REACHED.add((form, route))
                            if kind == 4:
                                fn, lead = (gpu.latok_token_features_batch if feats else gpu.latok_token_spans_batch), [d_units, d_row]
                            else:
                                fn, lead = (gpu.latok_token_features_kind_batch if feats else gpu.latok_token_spans_kind_batch), [d_units, kind, d_row]
                            rc, n, dgot, _ = _dev(ar, fn, lead, r.n_str, r.total, 4 if feats else 2, dt, feats, len(r.spans) + 8)
                            p = _plan()
                            assert rc == 0 and n == len(r.spans) and p[1] == 0 and p[14] == tiles, (what, rc, n, p)
                            ssc.compare(dgot, r, dt, feats, what + ("device",))
                            REACHED.add((form, "device"))
                finally:
                    ar.free()

            def submit(f, d_units, d_row, r, d_counts, d_items, d_sums, cap, d_res, dt):
                if f == "features":
                    batch.flow_token_features(d_units, kind, d_row, r.n_str, r.total, d_counts, d_items, d_sums, cap, d_res, dtype=dt)
                else:
                    batch.flow_token_spans(d_units, kind, d_row, r.n_str, r.total, d_counts, d_items, cap, d_res, dtype=dt)
            _flow_pair(gpu, work[:2], lambda texts: _units(texts, kind), submit, ("spans", "features"), 2, (table, form, size))
            REACHED.add((form, "flow"))


@pytest.mark.parametrize("table", TABLE_NAMES)
def test_utf8_in_byte_space(gpu, oracle, table):
    """positions are bytes: the whitespace chars are 1, 2 and 3 bytes wide, the chars next to them 1 to 4"""
    from latok_amd import batch
    _, small_chars, small_strings = _limits()
    with _rules(table):
        for size in ssc.SIZES:
            work = _content(oracle, table, size, "bytes")
            for i, (texts, r) in enumerate(work):
                u8, boff = _enc(texts)
                assert np.array_equal(boff, r.row)
                r.total_chars = sum(map(len, texts))
                decoded = u8.size <= small_chars and r.n_str <= small_strings       # small well-formed host batches: decoded by the host
                ar = _Arena(gpu)
                try:
                    d_u8, d_boff = ar.put(u8), ar.put(boff)
                    for dt in DTYPES:
                        what = (table, "utf8_bytes", size, "ABCD"[i], dt.__name__)
                        got = batch.token_spans_utf8_bytes_csr(u8, boff, dtype=dt)
                        assert _route() == (1 if decoded else 0), (what, _route())
                        ssc.compare(got, r, dt, False, what + ("spans, host",))
                        REACHED.add(("utf8_bytes", "spans_host_decoded" if decoded else "spans_own_units"))
                        got = batch.token_features_utf8_bytes_csr(u8, boff, dtype=dt)
                        assert _route() == (1 if decoded else 4), (what, _route())
                        ssc.compare(got, r, dt, True, what + ("features, host",))
                        REACHED.add(("utf8_bytes", "features_host_decoded" if decoded else "features_route4_host"))
                        if i == 0:
                            _three_way(u8, boff, got, dt, what)
                            REACHED.add(("utf8_bytes", "three_way"))
                        rc, n, dgot, _ = _dev(ar, gpu.latok_token_spans_utf8_bytes_batch, [d_u8, d_boff], r.n_str, r.total, 2, dt, False, len(r.spans) + 8)
                        assert rc == 0 and n == len(r.spans) and _route() == 0, (what, rc, n, _route())
                        ssc.compare(dgot, r, dt, False, what + ("spans, device",))
                        REACHED.add(("utf8_bytes", "spans_device"))
                        rc, n, dgot, _ = _dev(ar, gpu.latok_token_features_utf8_bytes_batch, [d_u8, d_boff], r.n_str, r.total, 4, dt, True, len(r.spans) + 8)
                        assert rc == 0 and n == len(r.spans) and _route() == 4, (what, rc, n, _route())
                        ssc.compare(dgot, r, dt, True, what + ("features, device",))
                        REACHED.add(("utf8_bytes", "features_route4_device"))
                finally:
                    ar.free()

            def spans(f, d_u8, d_boff, r, d_counts, d_items, d_sums, cap, d_res, dt):
                batch.flow_token_spans(d_u8, 0, d_boff, r.n_str, r.total, d_counts, d_items, cap, d_res, dtype=dt)

            def features(f, d_u8, d_boff, r, d_counts, d_items, d_sums, cap, d_res, dt):
                batch.flow_token_features_utf8_bytes(d_u8, d_boff, r.n_str, r.total, d_counts, d_items, d_sums, cap, d_res, dtype=dt)
            _flow_pair(gpu, work[:2], _enc, spans, ("spans",), 2, (table, "utf8_bytes", size))
            REACHED.add(("utf8_bytes", "flow_spans"))
            _flow_pair(gpu, work[:2], _enc, features, ("features",), 4, (table, "utf8_bytes", size))
            REACHED.add(("utf8_bytes", "flow_features"))


def _bits(r):
    """the boundary bitmask of the packed batch from the reference's offsets"""
    flags = np.zeros((r.total + 63) // 64 * 64, bool)
    flags[r.offsets + np.repeat(r.row[:-1], r.bound_counts)] = True
    return np.packbits(flags, bitorder="little").view(np.uint64)


@pytest.mark.parametrize("table", TABLE_NAMES)
def test_utf8_in_code_point_units(gpu, oracle, table):
    """the same bytes, results in code points: host-decoded (route 1), staged decoder (route 2: device pointers, at most kSmallChars
    bytes), via byte space (route 3), and the four flow calls with their code-point row offsets and totals"""
    from latok_amd import batch
    _, small_chars, small_strings = _limits()
    with _rules(table):
        for size in ssc.SIZES:
            work = _content(oracle, table, size, "bytes", ref_unit="chars")
            for i, (texts, r) in enumerate(work):
                u8, boff = _enc(texts)
                below = u8.size <= small_chars and r.n_str <= small_strings
                ar = _Arena(gpu)
                try:
                    d_u8, d_boff = ar.put(u8), ar.put(boff)
                    for dt in DTYPES:
                        for feats in (False, True):
                            what = (table, "utf8_code_points", size, "ABCD"[i], dt.__name__, "features" if feats else "spans")
                            got = (batch.token_features_utf8_csr if feats else batch.token_spans_utf8_csr)(u8, boff, dtype=dt)
                            assert _route() == (1 if below else 3), (what, _route())
                            ssc.compare(got, r, dt, feats, what + ("host",))
                            REACHED.add(("utf8_code_points", "route%d" % _route()))
                            fn = gpu.latok_token_features_utf8_batch if feats else gpu.latok_token_spans_utf8_batch
                            rc, n, dgot, _ = _dev(ar, fn, [d_u8, d_boff], r.n_str, int(boff[-1]), 4 if feats else 2, dt, feats, len(r.spans) + 8)
                            assert rc == 0 and n == len(r.spans) and _route() == (2 if u8.size <= small_chars else 3), (what, rc, n, _route())
                            ssc.compare(dgot, r, dt, feats, what + ("device",))
                            REACHED.add(("utf8_code_points", "route%d" % _route()))
                finally:
                    ar.free()
            # the four flow calls, two batches in flight
            ar = _Arena(gpu)
            try:
                jobs = []
                for texts, r in work[:2]:
                    u8, boff = _enc(texts)
                    d_u8, d_boff = ar.put(u8), ar.put(boff)
                    js = [(_Job(ar, d_u8, d_boff, r.n_str, u8.size, "mask"), r)]
                    js += [(_Job(ar, d_u8, d_boff, r.n_str, u8.size, f, dt, cap=(r.offsets.size if f == "offsets" else len(r.spans)) + 8), r)
                           for dt in DTYPES for f in ("offsets", "spans", "features")]
                    jobs.append(js)
                order = [j for js in zip(*jobs) for j in js]
                for job, _ in order:
                    job.submit()
                batch.flow_wait()
                for job, r in order:
                    what = (table, "utf8_code_points", size, "flow", job.form, np.dtype(job.dt).name)
                    if job.form == "mask":
                        res, bits, cp_row_off = job.mask()
                        assert res[0] == 0 and res[2] == r.total, (what, res)
                        assert np.array_equal(cp_row_off, r.row) and np.array_equal(bits, _bits(r)), what
                    else:
                        res, counts, items, sums = job.records()
                        assert res[2] == r.total, (what, res)
                        if job.form == "offsets":
                            assert res[0] == r.offsets.size and np.array_equal(counts, r.bound_counts) and np.array_equal(items, r.offsets), what
                        else:
                            assert res[0] == len(r.spans), (what, res)
                            ssc.compare((counts, items, sums), r, job.dt, job.form == "features", what)
                    REACHED.add(("utf8_code_points", "flow_" + job.form))
            finally:
                ar.free()


@pytest.mark.parametrize("table", TABLE_NAMES)
def test_python_surface(gpu, oracle, table):
    """tokenize_batch, featurize_batch, featurize_utf8_batch, featurize_utf8_bytes_batch: tokens as strings / bytes, raw positions, sums"""
    from latok_amd import batch

    def same(got, texts, r, call):
        assert len(got) == len(texts)
        k = 0
        for s, (t, toks) in enumerate(zip(texts, got)):
            assert len(toks) == r.counts[s], (table, call, s)
            for tok in toks:
                a, b, c, d = r.spans4[k].tolist()
                if call == "tokenize_batch":
                    assert tok == t[c:d], (table, call, s, k)
                else:
                    assert tok.text == t[c:d] and (tok.start_idx, tok.end_idx) == (a, b) and np.array_equal(tok.features, r.feats[k]), (table, call, s, k)
                k += 1
        assert k == len(r.spans4)
        REACHED.add(("python", call))

    with _rules(table):
        for size in ("small", "mid"):
            for texts, r in _content(oracle, table, size, "chars"):
                same(batch.tokenize_batch(texts), texts, r, "tokenize_batch")
                same(batch.featurize_batch(texts), texts, r, "featurize_batch")
            for texts, r in _content(oracle, table, size, "bytes", ref_unit="chars"):
                same(batch.featurize_utf8_batch([t.encode("utf-8") for t in texts]), texts, r, "featurize_utf8_batch")
            for texts, r in _content(oracle, table, size, "bytes"):
                blobs = [t.encode("utf-8") for t in texts]
                same(batch.featurize_utf8_bytes_batch(blobs), blobs, r, "featurize_utf8_bytes_batch")


def test_capacity_protocol_where_few_boundaries_are_kept(gpu, oracle):
    """AFTER_ALPHA drops a third of its tokens, so the token total is far from the boundary count: one token short writes nothing and
    leaves valid counts and the needed total; the exact capacity works.  Once per input form, featurize (records and sums)."""
    from latok_amd import _lib
    table = "AFTER_ALPHA"
    forms = [("utf32", "chars", None, lambda t: _units(t, 4), gpu.latok_token_features_batch, []),
             ("kind1", "chars", None, lambda t: _units(t, 1), gpu.latok_token_features_kind_batch, [1]),
             ("kind2", "chars", None, lambda t: _units(t, 2), gpu.latok_token_features_kind_batch, [2]),
             ("utf8_bytes", "bytes", None, _enc, gpu.latok_token_features_utf8_bytes_batch, []),
             ("utf8_code_points", "bytes", "chars", _enc, gpu.latok_token_features_utf8_batch, [])]
    with _rules(table):
        for form, unit, ref_unit, put, fn, kind in forms:
            rg = {"kind1": "latin1", "kind2": "bmp"}.get(form, "full")
            texts, r = _content(oracle, table, "mid", unit, rg, ref_unit)[0]
            units, row = put(texts)
            need, bounds = len(r.spans), int(r.bound_counts.sum())
            print(form, "tokens", need, "boundaries", bounds)
            assert 4 * need <= 3 * bounds
            ar = _Arena(gpu)
            try:
                d_units, d_row = ar.put(units), ar.put(row)
                for dt in DTYPES:
                    what = (table, form, dt.__name__)
                    rc, n, (counts, _, _), raw = _dev(ar, fn, [d_units] + kind + [d_row], r.n_str, int(row[-1]), 4, dt, True, need - 1)
                    assert rc == _lib.ERR_INVALID and n == need and np.array_equal(counts, r.counts), (what, rc, n)
                    assert (raw[0] == POISON).all() and (raw[1] == POISON).all(), what
                    rc, n, got, _ = _dev(ar, fn, [d_units] + kind + [d_row], r.n_str, int(row[-1]), 4, dt, True, need)
                    assert rc == 0 and n == need, (what, rc, n)
                    ssc.compare(got, r, dt, True, what + ("exact capacity",))
            finally:
                ar.free()
            REACHED.add(("capacity", form))


def test_chunked_host_pipeline():
    """host batches of at least two chunks: a process of its own with 4 K-position chunks (LATOK_PIPE_CHUNK_CHARS is read once), so
    that the planted runs lie around chunk cuts; every table, UTF-32, kind 1 / 2 and UTF-8 in byte space"""
    env = dict(os.environ, LATOK_PIPE_CHUNK_CHARS="4096")
    out = subprocess.run([sys.executable, os.path.join(HELPERS, "span_strip_pipeline_child.py"), ROOT], capture_output=True, text=True,
                         timeout=900, env=env)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), (out.stdout[-2000:], out.stderr[-3000:])
    for line in out.stdout.splitlines():
        if line.startswith("reached "):
            REACHED.add((line.split()[1], "pipeline"))


def test_every_route_and_form_was_reached(gpu, oracle):
    """(run the whole module: this test reads what the others noted)"""
    from latok_amd import batch
    missing = sorted(EXPECTED - REACHED)
    print("reached:", sorted(REACHED))
    assert not missing, ("routes and forms not reached:", missing)
    # the built-in tables are back
    assert not batch.rules_active()
    text = "This is a #test! Testing, http://a.b/c  me@x.org 1 2 3"
    cps, row = pack([text])
    assert batch.tokenize_batch([text]) == [oracle.tokenize(text)]
    assert np.array_equal(batch.split_mask_batch(cps, row), oracle.split_batch(cps, row, want_values=False)[1])
