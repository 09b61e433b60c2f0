"""Every code point through featurize, one token per char, against the oracle.

test_gpu_unicode_sweep.py sweeps the mask and values paths, which classify with the split-code table.  Featurize classifies with
the rule-code table, through a front end of its own per input form (UTF-32: the tile kernel in rules mode; PEP 393 kind 1: the
table-free lk_ascii_code_planes_t<RULE_CODES>; kind 2: the two-stage table; UTF-8: k_lead_codes with the byte-space rule-code
table), and a wrong code for one char shows only in that char's columns and its neighbours' context columns -- which dissolve in
a sum as soon as the char sits inside a longer token.  So this module installs featurize_content.SWEEP_TABLE, under which every
position of the interleavings of test_gpu_unicode_sweep._variants is a boundary (tests/test_featurize_content.py asserts that from
the oracle, and the token count with it): every non-space char is a kept token whose record is its own matrix row, in that
neighbourhood; the 29 whitespace chars show in their neighbours' columns.  Counts, spans4 and sums are compared exactly and in
full with featurize_content.batch_reference (the oracle alone), int64 and int32 records, as one string and cut every 7 chars.
A last case runs the natural order (long tokens) under the built-in tables.

No interleaving had to be thinned: the largest case (the 6-char "url" interleaving of 0x110000 code points, 6.7 M chars and 5.6 M
tokens) stays at a few seconds, most of it the reference."""
import contextlib
import os
import sys

import numpy as np
import pytest

HELPERS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers")
sys.path.insert(0, HELPERS)
import featurize_content as fc  # noqa: E402
import span_strip_content as ssc  # noqa: E402
from test_gpu_flow_utf8 import _Arena  # noqa: E402
from test_gpu_span_strip import DTYPES, POISON, _host_route, _plan, _route  # noqa: E402
from test_gpu_unicode_sweep import N_CP, OUT_OF_RANGE, _many_strings, _one_string, _utf8_encode, _variants  # noqa: E402

pytestmark = pytest.mark.gpu

SWEPT = ("spaces", "letters", "upper-lower", "at", "url", "period-at", "hash")
ROWS = ("one_string", "every_7")
_LAST = {}


@contextlib.contextmanager
def _rules(tables):
    from latok_amd import batch
    if tables is not None:
        batch.set_rules(*tables)
    try:
        assert batch.rules_active() == (tables is not None)
        yield
    finally:
        batch.reset_rules()


def _swept(form):
    """the values a form can hold"""
    if form == "kind1":
        return np.tile(np.arange(256, dtype=np.uint32), 40)
    if form == "kind2":
        return np.arange(0x10000, dtype=np.uint32)
    if form.startswith("utf8"):
        return np.arange(N_CP, dtype=np.uint32)
    return np.concatenate([np.arange(N_CP, dtype=np.uint32), OUT_OF_RANGE])


def _case(oracle, form, name, rows, unit, tables=fc.SWEEP_TABLE):
    """(code points, row offsets in chars, reference): one reference is kept, the forms that share it run one after the other"""
    key = (form if form in ("kind1", "kind2") else form.startswith("utf8"), name, rows, unit, tables is None)
    if _LAST.get("key") != key:
        _LAST.clear()
        cps0 = _swept(form)
        if name == "pairs":
            a = np.arange(256, dtype=np.uint32)
            cps = np.stack([np.repeat(a, 256), np.tile(a, 256)], axis=1).reshape(-1)
        else:
            cps = dict(_variants(cps0))[name]
        row = _one_string(cps) if rows == "one_string" else _many_strings(cps, 997 if name == "plain" else 7)
        _LAST.update(key=key, cps=cps, row=row, ref=fc.batch_reference(oracle, cps, row, tables, unit))
    return _LAST["cps"], _LAST["row"], _LAST["ref"]


def _compare(got, r, cps, dt, what):
    """ssc.compare, and on a mismatch the first token whose record or sums differ as a code point with its neighbours"""
    try:
        ssc.compare(got, r, dt, True, what)
    except AssertionError as e:
        items, sums = got[1].reshape(-1, 4), got[2].reshape(-1, 25)
        n = min(len(items), len(r.spans4))
        bad = np.nonzero((items[:n] != r.spans4[:n]).any(axis=1) | (sums[:n] != r.feats[:n]).any(axis=1))[0]
        k = int(bad[0]) if bad.size else n
        if k >= len(r.kp):
            raise
        p = int(r.kp[k])
        around = " ".join("U+%04X" % int(c) for c in cps[max(p - 2, 0):p + 3])
        raise AssertionError("%s: first differing token %d = char %d, U+%04X (chars %d.. are %s): record %s want %s, sums %s want %s"
                             % (e.args[0][:2], k, p, int(cps[p]), max(p - 2, 0), around, items[k].tolist() if k < n else None,
                                r.spans4[k].tolist(), sums[k].tolist() if k < n else None, r.feats[k].tolist())) from None


def _n_expected(cps0, name):
    fill = {"spaces": 0, "letters": 1, "upper-lower": 2, "at": 2, "url": 4, "period-at": 2, "hash": 1}[name]
    return int((~fc.ws_table()[np.minimum(cps0, N_CP)]).sum()) + fill * cps0.size


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("name", SWEPT)
def test_utf32(gpu, oracle, name, rows):
    """latok_token_features_batch: all 0x110000 code points and five values beyond them"""
    from latok_amd import batch
    cps, row, r = _case(oracle, "utf32", name, rows, "chars")
    assert len(r.spans4) == _n_expected(_swept("utf32"), name)
    with _rules(fc.SWEEP_TABLE):
        for dt in DTYPES:
            got = batch.token_features_csr(cps, row, dtype=dt)
            p = _plan()
            assert _host_route(r.total, r.n_str) == "staged" and p[1] == 0 and p[14] == (r.total + fc.TILE - 1) // fc.TILE, p
            _compare(got, r, cps, dt, ("utf32", name, rows, dt.__name__))


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("kind,name", [(1, n) for n in SWEPT + ("pairs",)] + [(2, n) for n in SWEPT])
def test_pep393_kinds(gpu, oracle, kind, name, rows):
    """latok_token_features_kind_batch.  Kind 2: U+0000..U+FFFF with surrogates and noncharacters as UCS-2 units; kind 1: the 256
    Latin-1 chars 40 times over, and ("pairs") every pair of them adjacent once"""
    from latok_amd import batch
    form = "kind%d" % kind
    cps, row, r = _case(oracle, form, name, rows, "chars")
    if name != "pairs":
        assert len(r.spans4) == _n_expected(_swept(form), name)
    units = cps.astype(np.uint8 if kind == 1 else np.uint16)
    route = _host_route(r.total, r.n_str)
    with _rules(fc.SWEEP_TABLE):
        for dt in DTYPES:
            assert route != "one_launch"
            got = batch.token_features_kind_csr(units, row, dtype=dt)
            p = _plan()
            assert p[1] == int(route == "pinned") and p[14] == (r.total + fc.TILE - 1) // fc.TILE, (route, p)
            _compare(got, r, cps, dt, (form, name, rows, dt.__name__, route))


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("name", SWEPT)
@pytest.mark.parametrize("unit", ssc.UNITS)
def test_utf8(gpu, oracle, unit, name, rows):
    """every scalar value and the surrogates as 3-byte sequences: in code-point units (route 3: byte space and the rule codes
    k_lead_codes leaves at the lead bytes) and in byte space (route 4, spans4 in bytes)"""
    from latok_amd import batch
    cps, row, r = _case(oracle, "utf8", name, rows, unit)
    assert len(r.spans4) == _n_expected(_swept("utf8"), name)
    u8, start = _utf8_encode(cps)
    boff = start[row]
    assert unit == "chars" or np.array_equal(boff, r.row)
    fn, route = (batch.token_features_utf8_csr, 3) if unit == "chars" else (batch.token_features_utf8_bytes_csr, 4)
    with _rules(fc.SWEEP_TABLE):
        for dt in DTYPES:
            got = fn(u8, boff, dtype=dt)
            assert _route() == route, _route()
            _compare(got, r, cps, dt, ("utf8", unit, name, rows, dt.__name__))


@pytest.mark.parametrize("form", ("utf32", "utf8_bytes"))
def test_batch_flow(gpu, oracle, form):
    """one interleaving each through the batch flow, int32 records: the same batch twice in flight"""
    from latok_amd import batch
    name, unit = ("at", "chars") if form == "utf32" else ("period-at", "bytes")
    cps, row, r = _case(oracle, form, name, "every_7", unit)
    dt, n = np.int32, len(r.spans4)
    ar = _Arena(gpu)
    try:
        with _rules(fc.SWEEP_TABLE):
            if form == "utf32":
                d_units, d_row, words = ar.put(cps), ar.put(row), 2
            else:
                u8, start = _utf8_encode(cps)
                d_units, d_row, words = ar.put(u8), ar.put(start[row]), 4
            outs = []
            for _ in range(2):
                o = (ar.alloc(r.n_str * 4, POISON), ar.alloc(n * 16, POISON), ar.alloc(n * 25, POISON), ar.alloc(8 * words, POISON))
                outs.append(o)
                if form == "utf32":
                    batch.flow_token_features(d_units, 4, d_row, r.n_str, r.total, o[0], o[1], o[2], n, o[3], dtype=dt)
                else:
                    batch.flow_token_features_utf8_bytes(d_units, d_row, r.n_str, r.total, o[0], o[1], o[2], n, o[3], dtype=dt)
            batch.flow_wait()
            for o in outs:
                res = ar.get(o[3], words, np.int64)
                assert res[0] == n and res[1] == 0 and (words == 2 or (res[2] == r.total_chars and res[3] == 0)), res
                got = (ar.get(o[0], r.n_str, dt), ar.get(o[1], (n, 4), dt), ar.get(o[2], (n, 25), np.int8))
                _compare(got, r, cps, dt, ("flow", form, name))
    finally:
        ar.free()


@pytest.mark.parametrize("form", ("utf32", "kind2", "utf8_chars", "utf8_bytes"))
def test_natural_order_under_the_built_in_tables(gpu, oracle, form):
    """no interleaving: the code points in their own order, cut every 997 chars, long tokens, the built-in tables"""
    from latok_amd import batch
    unit = "bytes" if form == "utf8_bytes" else "chars"
    cps, row, r = _case(oracle, form, "plain", "every_997", unit, tables=None)
    assert not batch.rules_active()
    for dt in DTYPES:
        if form == "utf32":
            got = batch.token_features_csr(cps, row, dtype=dt)
            assert _plan()[14] == (r.total + fc.TILE - 1) // fc.TILE
        elif form == "kind2":
            got = batch.token_features_kind_csr(cps.astype(np.uint16), row, dtype=dt)
            assert _plan()[14] == (r.total + fc.TILE - 1) // fc.TILE
        else:
            u8, start = _utf8_encode(cps)
            got = (batch.token_features_utf8_csr if unit == "chars" else batch.token_features_utf8_bytes_csr)(u8, start[row], dtype=dt)
            assert _route() == (3 if unit == "chars" else 4)
        _compare(got, r, cps, dt, ("natural order", form, dt.__name__))


def test_zz_the_built_in_tables_are_back(gpu, oracle):
    from latok_amd import batch
    _LAST.clear()
    assert not batch.rules_active()
    text = "This is a #test! Testing, http://a.b/c  me@x.org 1 2 3"
    assert batch.tokenize_batch([text]) == [oracle.tokenize(text)]
