"""The coverage claim of tests/test_gpu_span_strip.py, checkable without a GPU: for every rule table, size and unit the planted
content reaches every class of whitespace run, token length and word / tile / string / batch edge that the strip and drop logic
of the span and featurize kernels distinguishes (tests/helpers/span_strip_content.py: REQUIRED).  The census comes from the
reference alone (oracle boundaries + str.strip); the reference itself is pinned to oracle.tokenize under the built-in tables."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers"))
import span_strip_content as ssc  # noqa: E402


def test_tables_and_whitespace_against_the_oracle(oracle):
    ssc.validate(oracle)


def test_reference_on_hand_made_cases(oracle):
    t = "ab" + " " * 300 + "Cd　　" + "E"
    for unit, w in (("chars", 1), ("bytes", 3)):
        r = ssc.reference(oracle, ["", t, "  "], ssc.TABLES["UPPER_ONLY"], unit)
        assert r.counts.tolist() == [0, 3, 0] and r.bound_counts.tolist() == [0, 3, 1]
        assert r.spans4.tolist() == [[0, 302, 0, 2], [302, 304 + 2 * w, 302, 304], [304 + 2 * w, 305 + 2 * w, 304 + 2 * w, 305 + 2 * w]]
        assert r.spans.tolist() == [[0, 2], [302, 304], [304 + 2 * w, 305 + 2 * w]] and r.total == 305 + 2 * w + 2
        assert r.feats[0, ssc.SPACE] == np.int8(300 - 256) == 44 and r.feats[1, ssc.SPACE] == 2     # uint8 wrap-around, per char
        assert [k for *_, k, _, _ in r.tokens] == [True, True, True, False]


@pytest.mark.parametrize("size", ssc.SIZES)
@pytest.mark.parametrize("table", sorted(ssc.TABLES))
def test_census_reaches_every_required_class(oracle, table, size):
    for unit, rg in (("chars", "latin1"), ("chars", "bmp"), ("chars", "full"), ("bytes", "full")):
        batches = ssc.content(table, size, unit, rg)
        assert size == "large" or batches == ssc.content(table, size, unit, rg)    # deterministic
        got = set()
        for texts in batches:
            joined = "".join(texts)
            assert all(ssc.in_range(c, rg) for c in set(joined))
            n = len(joined.encode("utf-8")) if unit == "bytes" else len(joined)
            if size == "small":
                assert n <= ssc.TILE and len(texts) < 512                           # the one-launch path holds it
            elif size == "mid":
                assert n <= ssc.SMALL_CHARS                                         # pinned host route; host-decoded UTF-8
            got |= ssc.census(oracle, texts, ssc.TABLES[table], unit)
        if size == "large":
            assert sum(len(t) > 2 * ssc.TILE for texts in batches for t in texts) >= 3 and n > 0
            assert sum(map(len, batches[0])) > ssc.SMALL_CHARS and sum(map(len, batches[1])) > ssc.SMALL_CHARS
        missing = sorted(ssc.REQUIRED[size][unit] - got)
        assert not missing, (table, size, unit, rg, "classes not reached:", missing)
        print(table, size, unit, rg, "reaches", sorted(got & ssc.REQUIRED[size][unit]))


@pytest.mark.parametrize("size", ("small", "mid"))
def test_reference_equals_oracle_tokenize_under_the_built_in_tables(oracle, size):
    """the same content under the default tables (tables=None: oracle.split_values): the kept tokens of the reference are
    oracle.tokenize's, string by string"""
    for table in sorted(ssc.TABLES):
        for texts in ssc.content(table, size, "chars", "full"):
            r = ssc.reference(oracle, texts, None, "chars")
            k = 0
            for t, n in zip(texts, r.counts.tolist()):
                assert [t[a:b] for a, b in r.spans[k:k + n].tolist()] == (oracle.tokenize(t) if t else [])
                k += n
            assert k == len(r.spans)
