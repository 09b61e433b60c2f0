"""What tests/test_gpu_featurize_sweep.py and tests/test_gpu_featurize_forms.py rest on, checked without a GPU
(tests/helpers/featurize_content.py): the reference over arrays equals span_strip_content.reference, the sweep's rule table makes
every char of the interleavings a token of its own, the census names the classes of hand-made tiles, and the builders' batches
reach every class of REQUIRED.  The kernel's constants come from the built library (latok_debug_limits needs no device)."""
import os
import random
import sys

import numpy as np
import pytest

from conftest import ALPHABETS, DEFAULT_RULES, pack, random_strings

HELPERS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers")
sys.path.insert(0, HELPERS)
import featurize_content as fc  # noqa: E402
import span_strip_content as ssc  # noqa: E402
from test_gpu_unicode_sweep import N_CP, OUT_OF_RANGE, _many_strings, _one_string, _variants  # noqa: E402

TILE = fc.TILE
SWEPT = ("spaces", "letters", "upper-lower", "at", "url", "period-at", "hash")


@pytest.fixture(scope="module")
def lim():
    return fc.limits()


def test_limits_hook_reports_the_featurize_constants(lim):
    """entries 9..13 of latok_debug_limits; the first nine are what earlier callers read"""
    from test_host_api import debug_limits
    first = debug_limits()
    assert first["kTile"] == lim["TILE"] and first["kSmallChars"] == lim["SMALL_CHARS"]
    assert 1 <= lim["WAVES"] <= 16 and 0 < lim["RTM"] <= lim["R"] <= TILE and lim["THRESH"] >= 1
    assert lim["WIN"] >= lim["R"] * 25 and lim["WIN"] % 16 == 0 and lim["RTM"] * 27 + 16 <= lim["WIN"]
    assert lim["SR64"] <= lim["SR32"] <= lim["R"]


@pytest.mark.parametrize("unit", ssc.UNITS)
def test_array_reference_equals_the_string_reference(oracle, unit):
    """batch_reference is span_strip_content.reference: every field, under the built-in tables, the sweep's table and the tables that
    leave whitespace inside tokens"""
    rng = random.Random(0xFC)
    ws = ["\t", "\n", "\x0b", "\x1c", "\x85", "\xa0", " ", "　", "  ", "   "]
    texts = ["", " ", "x", "  \t"] + random_strings(rng, 600, 0, 120, ALPHABETS["mixed"] + ws + ["http://a.b/c", "me@x.org", "AbC"]) + ["", ""]
    cases = [("built-in", None), ("default rules", DEFAULT_RULES), ("sweep", fc.SWEEP_TABLE)] + sorted(ssc.TABLES.items())
    for name, tables in cases:
        a, b = fc.reference(oracle, texts, tables, unit), ssc.reference(oracle, texts, tables, unit)
        for f in ("counts", "bound_counts", "row", "spans4", "spans", "feats", "offsets"):
            x, y = getattr(a, f), getattr(b, f)
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), (name, f)
        assert (a.total, a.n_str, a.empty) == (b.total, b.n_str, b.empty), name
        kept = [(p, e) for s, p, e, lead, trail, k, last, widths in ssc.reference(oracle, texts, tables, "chars").tokens if k]
        assert kept == list(zip(a.kp.tolist(), a.ke.tolist())), name


def test_whitespace_table_is_the_oracles(oracle):
    ws = np.nonzero(fc.ws_table())[0]
    col = oracle.gen_parse_matrix(np.arange(N_CP, dtype=np.uint32))[:, fc.SPACE]
    assert ws.size == 29 and np.array_equal(np.nonzero(col)[0], ws)


@pytest.mark.parametrize("name", SWEPT)
def test_sweep_table_makes_every_char_a_token(oracle, name):
    """under SWEEP_TABLE every position of the interleaving is a boundary, as one string and cut every 7 chars, so the kept tokens
    are exactly the non-space chars: (swept values - 29 whitespace) + the non-space fillers, each with its matrix row as its sums"""
    cps0 = np.concatenate([np.arange(N_CP, dtype=np.uint32), OUT_OF_RANGE])
    cps = dict(_variants(cps0))[name]
    fillers = cps[1:cps.size // cps0.size]
    for row in (_one_string(cps), _many_strings(cps, 7)):
        vals = oracle.split_values_rules_batch(cps, row, *fc.SWEEP_TABLE)
        assert int((vals == 0).sum()) == 0
        r = fc.batch_reference(oracle, cps, row, fc.SWEEP_TABLE, "chars")
        want = (cps0.size - 29) + cps0.size * int((fillers != ord(" ")).sum())
        assert len(r.spans4) == want == int(r.counts.sum())
        assert ((r.ke - r.kp) == 1).all() and (r.spans4[:, 1] - r.spans4[:, 0] == 1).all()


def _tile_census(oracle, lim, text):
    return fc.census(oracle, [text], None, lim)


def test_census_on_hand_made_tiles(oracle, lim):
    """tiles whose classes are obvious (the constants as they stand: 896 / 768 / 5)"""
    assert (lim["R"], lim["RTM"], lim["THRESH"]) == (896, 768, 5), "re-derive the expectations of this test"
    c = _tile_census(oracle, lim, " abc" * 1024)                       # 16 tokens per word, 1024 per tile
    assert {"WM_MULTI", "SPAN64:WORD_SPLIT", "WM_EDGE:BETWEEN_WORDS"} <= c and not c & {"TM_1", "TM_MULTI", "WM_1"}
    c = _tile_census(oracle, lim, ",." * 2048)
    assert {"TM_MULTI", "TM_FULL_TILE", "TM_EDGE:WORD_AT_EDGE"} <= c and "WM_MULTI" not in c
    c = _tile_census(oracle, lim, ",." * 32 + ("abcdefg " * 8) * 63)
    assert "TM_1" in c and not c & {"TM_MULTI", "WM_MULTI"}
    c = _tile_census(oracle, lim, "abcdefg " * 512)
    assert "WM_1" in c and not c & {"TM_1", "TM_MULTI", "WM_MULTI", "NEAR_BELOW"}
    c = _tile_census(oracle, lim, ("abcd " * 820)[:TILE])
    assert "SPAN64:INSIDE_ONE_FEATURE_ROUND" in c and "WM_MULTI" not in c
    # a token from bit 0 of word 3 of a tile to bit 10 of the next tile's second word (behind a symbol a letter opens a token)
    c = _tile_census(oracle, lim, "xy," * 64 + "a" * (TILE + 64 + 10 - 192) + " b")
    assert {"LEAVE:LOW:NEXT_TILE_WORD1", "LEAVE:LOW:WALK_STEP1", "WRAP:CROSSES_TILE"} <= c and not [x for x in c if x.startswith("LEAVE:HIGH")]
    c = fc.census(oracle, ["xy," * 64 + "a" * (TILE + 1 - 192), "bc"], None, lim)
    assert "STR_END:TILE+4097" in c and "STR_END:TILE+4096" not in c
    c = fc.census(oracle, ["a" * (TILE + 1)], None, lim)
    assert {"TAIL:1", "LAST:NEXT_TILE_WORD0", "SHIFT:0", "SHIFT:SINGLE_TOKEN_TILE"} <= c
    c = fc.census(oracle, ["ab"] + [""] * 70 + ["cd"], None, lim)
    assert "LAST:OWN_WORD" in c and not [x for x in c if x.startswith("EMPTY_RUN")]


def test_first_diff_names_the_token_and_its_classes(oracle, lim):
    """what a GPU test prints when a record differs: the token, its tile, word and bit, the columns, and the classes it was planted for"""
    texts = ["xy," * 64 + "a" * (TILE + 1 - 192), "bc"]
    r = fc.reference(oracle, texts, None, "chars")
    j = int(np.nonzero(r.ke - r.kp > 64)[0][0])
    feats = r.feats.copy()
    feats[j, 23] ^= 1
    msg = fc.first_diff((r.counts, r.spans4, feats), r, lim)
    assert "token %d: tile 0 word 3 bit 0" % j in msg and "STR_END:TILE+4097" in msg and "columns [23]" in msg, msg
    assert fc.first_diff((r.counts + 1, r.spans4, r.feats), r, lim).startswith("counts differ")


@pytest.mark.parametrize("rg", ("full", "bmp", "latin1"))
def test_builders_reach_every_class(oracle, lim, rg):
    """the coverage claim of tests/test_gpu_featurize_forms.py: the batches are deterministic and together reach REQUIRED; the padding
    that lifts a small batch over the size of the large routes changes none of its classes but the rank-dependent ones"""
    work = fc.batches(lim, rg)
    assert work == fc.batches(lim, rg)
    hi = {"latin1": 0x100, "bmp": 0x10000, "full": N_CP}[rg]
    reached, small = set(), set()
    pad = fc.padding(lim)
    assert sum(map(len, pad)) % TILE == 0 and sum(map(len, pad)) > lim["SMALL_CHARS"]
    for name, texts in work.items():
        assert max(map(ord, "".join(texts))) < hi
        c = fc.census(oracle, texts, None, lim)
        print(rg, name, "%d strings, %d chars:" % (len(texts), sum(map(len, texts))), " ".join(sorted(c)))
        reached |= c
        if name != "main":
            small |= c
            assert len("".join(texts).encode("utf-8")) <= lim["SMALL_CHARS"] and len(texts) <= lim["SMALL_STRINGS"]
            rank_free = {x for x in c if not x.startswith("SHIFT")}
            assert rank_free <= fc.census(oracle, pad + texts, None, lim), name
    assert len("".join(work["main"]).encode("utf-8")) > lim["SMALL_CHARS"]
    missing = sorted(fc.REQUIRED - reached)
    assert not missing, ("classes no batch reaches:", missing)
    assert not fc.REQUIRED_SMALL - small, ("classes no small batch reaches:", sorted(fc.REQUIRED_SMALL - small))
